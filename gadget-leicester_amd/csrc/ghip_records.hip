// ghip_records.hip -- the whole-record (AoS) path, the drop-in boundary under accel.c: the raw P[] /
// SphP[] blocks cross the link as they are, and one kernel moves their members to and from the
// resident fields on the device image.  Which member goes where, and with which transfer, is one
// table (kRows): a new record member is one row.
#include "ghip_internal.h"

// ---------------------------------------------------------------------------------------------
// the member table
// ---------------------------------------------------------------------------------------------
// blocks: P[] over all n particles, P[] over the gas block [0, ngas), SphP[]
enum { B_P, B_PGAS, B_S, B_COUNT };
// conversions (the kinds of k_records): double[ncomp] <-> SoA component arrays of stride n;
// short <-> int; int <-> int; int -> float, pack only (P[].GravCost)
enum { K_F64, K_I16, K_I32, K_COST };
// transfers: UP = the uploads, the rest = what a download writes back.  Hsml / NumNgb are written
// back to the one block the PPP macro puts them in (allvars.h:266-270): DENS_P with p_hsml set
// (over the gas block only), DENS_S otherwise; DENS rows go with both.
enum { UP = 1, GRAV = 2, DENS_P = 4, DENS_S = 8, DENS = DENS_P | DENS_S, HYDRO = 16, KICK = 32 };

struct RecRow
{
  int ghip_layout::*off;   // -1 in a layout: the member is absent, the row is skipped
  int field;               // (its component count: kField[], through ghip_field_info)
  short kind, block;
  unsigned sets;
};

static constexpr RecRow kRows[] = {
  {&ghip_layout::p_pos, GHIP_F_POS, K_F64, B_P, UP},
  {&ghip_layout::p_vel, GHIP_F_VEL, K_F64, B_P, UP | KICK},
  {&ghip_layout::p_mass, GHIP_F_MASS, K_F64, B_P, UP},
  {&ghip_layout::p_oldacc, GHIP_F_OLDACC, K_F64, B_P, UP | GRAV},
  {&ghip_layout::p_type, GHIP_F_TYPE, K_I16, B_P, UP},
  {&ghip_layout::p_timebin, GHIP_F_TIMEBIN, K_I16, B_P, UP | KICK},
  {&ghip_layout::p_ti_begstep, GHIP_F_TI_BEGSTEP, K_I32, B_P, UP | KICK},
  {&ghip_layout::p_ti_current, GHIP_F_TI_CURRENT, K_I32, B_P, UP},
  {&ghip_layout::p_gravaccel, GHIP_F_GRAVACCEL, K_F64, B_P, UP | GRAV},
  {&ghip_layout::p_gravpm, GHIP_F_GRAVPM, K_F64, B_P, UP | GRAV},
  {&ghip_layout::p_gravcost, GHIP_F_GRAVCOST, K_COST, B_P, GRAV},
  {&ghip_layout::p_hsml, GHIP_F_HSML, K_F64, B_P, UP},
  {&ghip_layout::p_hsml, GHIP_F_HSML, K_F64, B_PGAS, DENS_P},
  {&ghip_layout::p_numngb, GHIP_F_NUMNGB, K_F64, B_PGAS, DENS_P},
  {&ghip_layout::s_hsml, GHIP_F_HSML, K_F64, B_S, UP | DENS_S},   // first ngas entries
  {&ghip_layout::s_numngb, GHIP_F_NUMNGB, K_F64, B_S, DENS_S},
  {&ghip_layout::s_velpred, GHIP_F_VELPRED, K_F64, B_S, UP | KICK},
  {&ghip_layout::s_entropy, GHIP_F_ENTROPY, K_F64, B_S, UP | KICK},
  {&ghip_layout::s_dtentropy, GHIP_F_DTENTROPY, K_F64, B_S, UP | HYDRO | KICK},
  {&ghip_layout::s_density, GHIP_F_DENSITY, K_F64, B_S, UP | DENS},
  {&ghip_layout::s_dhsmlfac, GHIP_F_DHSMLFAC, K_F64, B_S, UP | DENS},
  {&ghip_layout::s_divvel, GHIP_F_DIVVEL, K_F64, B_S, UP | DENS},
  {&ghip_layout::s_curlvel, GHIP_F_CURLVEL, K_F64, B_S, UP | DENS},
  {&ghip_layout::s_pressure, GHIP_F_PRESSURE, K_F64, B_S, UP | DENS},
  {&ghip_layout::s_hydroaccel, GHIP_F_HYDROACCEL, K_F64, B_S, UP | HYDRO},
  {&ghip_layout::s_maxsignalvel, GHIP_F_MAXSIGNALVEL, K_F64, B_S, UP | HYDRO},
};

// One pass over a record block for all of its fields (instead of one launch per field: every launch
// re-reads every line of the image).
struct RecField
{
  void *soa;
  int off;
  short ncomp, kind;
};
struct RecMap
{
  static constexpr int CAP = 16;
  size_t n;
  int stride, nf;
  RecField f[CAP];
};

// a map holds at most the rows of one block: all of them fit, whatever the sets asked for
static constexpr int rows_of(int block)
{
  int c = 0;
  for(const RecRow &r : kRows)
    c += r.block == block;
  return c;
}
static_assert(rows_of(B_P) <= RecMap::CAP && rows_of(B_PGAS) <= RecMap::CAP && rows_of(B_S) <= RecMap::CAP,
              "a block of kRows has more members than a RecMap holds: raise RecMap::CAP");

static RecMap rec_map(ghip_ctx *ctx, const ghip_layout *lay, int block, unsigned sets)
{
  RecMap m;
  m.n = (size_t) (block == B_P ? ctx->n : ctx->ngas);
  m.stride = block == B_S ? lay->s_stride : lay->p_stride;
  m.nf = 0;
  for(const RecRow &r : kRows)
    if(r.block == block && (r.sets & sets) && lay->*r.off >= 0)
      {
        int gas, ncomp, isint;
        ghip_field_info(r.field, &gas, &ncomp, &isint);
        m.f[m.nf++] = RecField{ctx->f[r.field].p, lay->*r.off, (short) ncomp, r.kind};
      }
  return m;
}

// type_off >= 0: the records [0, ngas) are supposed to be gas (allvars.h:1384); *mixed is set when
// one of them has another Type
template <bool PACK>
__global__ void k_records(RecMap m, char *__restrict__ rec, int type_off, int ngas, int *mixed)
{
  size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= m.n)
    return;
  char *r = rec + i * (size_t) m.stride;
  for(int k = 0; k < m.nf; k++)
    {
      const RecField f = m.f[k];
      if(f.kind == 0)
        {
          double *a = reinterpret_cast<double *>(r + f.off);
          double *s = reinterpret_cast<double *>(f.soa);
          for(int c = 0; c < f.ncomp; c++)
            {
              if(PACK)
                a[c] = s[(size_t) c * m.n + i];
              else
                s[(size_t) c * m.n + i] = a[c];
            }
        }
      else if(f.kind == 1)
        {
          if(PACK)
            *reinterpret_cast<short *>(r + f.off) = (short) reinterpret_cast<int *>(f.soa)[i];
          else
            reinterpret_cast<int *>(f.soa)[i] = (int) *reinterpret_cast<const short *>(r + f.off);
        }
      else if(f.kind == 2)
        {
          if(PACK)
            *reinterpret_cast<int *>(r + f.off) = reinterpret_cast<int *>(f.soa)[i];
          else
            reinterpret_cast<int *>(f.soa)[i] = *reinterpret_cast<const int *>(r + f.off);
        }
      else if(PACK)
        *reinterpret_cast<float *>(r + f.off) = (float) reinterpret_cast<int *>(f.soa)[i];
    }
  if(!PACK && type_off >= 0 && i < (size_t) ngas && *reinterpret_cast<const short *>(r + type_off) != 0)
    *mixed = 1;
}

// The kernels may run underneath a gravity pair in flight: one-wavefront workgroups then (ghip_wg)
template <bool PACK>
static int run_records(ghip_ctx *ctx, const RecMap &m, void *img, int type_off = -1,
                       hipStream_t st = nullptr)
{
  if(m.n == 0 || m.nf == 0)
    return GHIP_OK;
  const int wg = ghip_wg(ctx);
  k_records<PACK><<<cdiv((long long) m.n, wg), wg, 0, st ? st : ctx->stream>>>(
    m, (char *) img, type_off, ctx->ngas, ghip_gas_mixed_word(ctx));
  HIPCHK(hipGetLastError());
  return GHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// uploads
// ---------------------------------------------------------------------------------------------
// the P[] block: copy + unpack of the per-particle fields, and the Type check of the gas block
static int upload_p_block(ghip_ctx *ctx, const void *Pp, const ghip_layout *lay)
{
  const size_t n = (size_t) ctx->n;
  if(n == 0)
    return GHIP_OK;
  GCHK(ghip_ensure(ctx, ctx->aosP, n * lay->p_stride));
  HIPCHK(hipMemcpyAsync(ctx->aosP.p, Pp, n * lay->p_stride, hipMemcpyHostToDevice, ctx->stream));
  *ghip_gas_mixed_word(ctx) = 0;
  return run_records<false>(ctx, rec_map(ctx, lay, B_P, UP), ctx->aosP.p, lay->p_type);
}

// the SphP[] block: copy + unpack of the per-gas-particle fields
static int upload_s_block(ghip_ctx *ctx, const void *Sp, const ghip_layout *lay)
{
  const size_t ng = (size_t) ctx->ngas;
  if(ng == 0)
    return GHIP_OK;
  GCHK(ghip_ensure(ctx, ctx->aosS, ng * lay->s_stride));
  HIPCHK(hipMemcpyAsync(ctx->aosS.p, Sp, ng * lay->s_stride, hipMemcpyHostToDevice, ctx->stream));
  return run_records<false>(ctx, rec_map(ctx, lay, B_S, UP), ctx->aosS.p);
}

static int check_upload_args(ghip_ctx *ctx, const void *Pp, const void *Sp, const ghip_layout *lay,
                             int numpart, int ngas, bool need_s)
{
  if(!ctx || !lay || numpart < 0 || ngas < 0 || ngas > numpart || (numpart > 0 && !Pp) ||
     (need_s && ngas > 0 && !Sp))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_upload_aos: bad arguments");
  if(lay->p_stride <= 0 || (ngas > 0 && lay->s_stride <= 0))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_upload_aos: bad strides");
  if((lay->p_hsml >= 0) == (lay->s_hsml >= 0) && ngas > 0)
    return ghip_fail(ctx, GHIP_EINVAL,
                     "ghip_upload_aos: exactly one of p_hsml / s_hsml must be set (PPP macro)");
  return GHIP_OK;
}

// a new P[] block is resident: wait for it, and nothing built from the old one holds any more.
// gas_wait: the SphP[] block is still to come (whatever joins in between must leave the gas tree deferred)
static int p_block_uploaded(ghip_ctx *ctx, const ghip_layout *lay, bool gas_wait)
{
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  ctx->gt.built = false;
  ctx->st.built = false;
  ctx->dd.geom_kept = false;
  ctx->gas_wait_upload = gas_wait;
  ctx->gas_mixed = lay->p_type >= 0 && *reinterpret_cast<volatile int *>(ghip_gas_mixed_word(ctx)) != 0;
  ctx->gas_list_dirty = true;
  return GHIP_OK;
}

extern "C" int ghip_upload_aos(ghip_ctx *ctx, const void *Pp, const void *Sp, const ghip_layout *lay,
                               int numpart, int ngas)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(ctx)
    ctx->pot_n = -1;
  GCHK(check_upload_args(ctx, Pp, Sp, lay, numpart, ngas, true));
  GCHK(ghip_set_counts(ctx, numpart, ngas));
  if(numpart == 0)
    return GHIP_OK;
  GCHK(upload_p_block(ctx, Pp, lay));
  GCHK(upload_s_block(ctx, Sp, lay));
  return p_block_uploaded(ctx, lay, false);
}

// The same in two calls, for a host that starts gravity before the gas data are across: the P[]
// block (everything the gravity tree and its walks read -- unless the smoothing lengths, which
// ADAPTIVE_GRAVSOFT_FORGAS makes softenings, live in SphP[]) ...
extern "C" int ghip_upload_aos_particles(ghip_ctx *ctx, const void *Pp, const ghip_layout *lay,
                                         int numpart, int ngas)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(ctx)
    ctx->pot_n = -1;
  GCHK(check_upload_args(ctx, Pp, nullptr, lay, numpart, ngas, false));
  if(ctx->adaptive_gravsoft && lay->p_hsml < 0 && ngas > 0)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_upload_aos_particles: with adaptive gravitational softening "
                     "the smoothing lengths of SphP[] are needed first: use ghip_upload_aos");
  GCHK(ghip_set_counts(ctx, numpart, ngas));
  if(numpart == 0)
    return GHIP_OK;
  GCHK(upload_p_block(ctx, Pp, lay));
  return p_block_uploaded(ctx, lay, ngas > 0);
}

// ... and the SphP[] block, which may follow while a gravity pair is in flight (it is not waited
// for): before the first SPH call of the step.
extern "C" int ghip_upload_aos_gas(ghip_ctx *ctx, const void *Sp, const ghip_layout *lay)
{
  if(!ctx || !lay || (ctx->ngas > 0 && (!Sp || lay->s_stride <= 0)))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_upload_aos_gas: bad arguments");
  GCHK(upload_s_block(ctx, Sp, lay));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  ctx->gas_wait_upload = false;
  return GHIP_OK;
}

extern "C" int ghip_gas_block_mixed(ghip_ctx *ctx)
{
  if(!ctx)
    return GHIP_EINVAL;
  return *reinterpret_cast<volatile int *>(ghip_gas_mixed_word(ctx)) != 0;
}

// ---------------------------------------------------------------------------------------------
// downloads: results are packed into the device image of the records, then one D2H per block
// ---------------------------------------------------------------------------------------------
// what a download needs before it touches the images (ctx->n > 0): somewhere to put the blocks it
// writes -- SphP[] too with with_s -- and the images an upload left
static int check_download(ghip_ctx *ctx, const char *who, const void *Pp, const void *Sp,
                          const ghip_layout *lay, bool with_s)
{
  const size_t n = (size_t) ctx->n, ng = with_s ? (size_t) ctx->ngas : 0;
  if(!Pp || (ng > 0 && !Sp))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: null record pointer%s", who, with_s ? "s" : "");
  if(ctx->aosP.cap < n * lay->p_stride || (ng > 0 && ctx->aosS.cap < ng * lay->s_stride))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: no device image (call ghip_upload_aos)", who);
  return GHIP_OK;
}

static int copy_p_block(ghip_ctx *ctx, void *Pp, const ghip_layout *lay, hipStream_t st)
{
  HIPCHK(hipMemcpyAsync(Pp, ctx->aosP.p, (size_t) ctx->n * lay->p_stride, hipMemcpyDeviceToHost, st));
  return GHIP_OK;
}

static int copy_s_block(ghip_ctx *ctx, void *Sp, const ghip_layout *lay)
{
  HIPCHK(hipMemcpyAsync(Sp, ctx->aosS.p, (size_t) ctx->ngas * lay->s_stride, hipMemcpyDeviceToHost,
                        ctx->stream));
  return GHIP_OK;
}

// the records are complete on the host, and no kernel on the way has reported a broken invariant
static int finish_download(ghip_ctx *ctx, hipStream_t st)
{
  HIPCHK(ghip_stream_sync(ctx, st));
  return ghip_check_device_errors(ctx);
}

static int download_aos_impl(ghip_ctx *ctx, void *Pp, void *Sp, const ghip_layout *lay,
                             int want_gravity, int want_density, int want_hydro, bool sync)
{
  // the SPH results do not depend on a gravity pair still in flight underneath them
  if(ctx && want_gravity)
    GHIP_JOIN(ctx);
  if(!ctx || !lay)
    return GHIP_EINVAL;
  if(ctx->n == 0)
    return GHIP_OK;
  GCHK(check_download(ctx, "ghip_download_aos", Pp, Sp, lay, true));
  unsigned sets = want_gravity ? GRAV : 0;
  if(ctx->ngas > 0)
    sets |= (want_density ? (lay->p_hsml >= 0 ? DENS_P : DENS_S) : 0) | (want_hydro ? HYDRO : 0);
  GCHK(run_records<true>(ctx, rec_map(ctx, lay, B_P, sets), ctx->aosP.p));
  GCHK(run_records<true>(ctx, rec_map(ctx, lay, B_PGAS, sets), ctx->aosP.p));
  GCHK(run_records<true>(ctx, rec_map(ctx, lay, B_S, sets), ctx->aosS.p));
  if(sets & (GRAV | DENS_P))
    GCHK(copy_p_block(ctx, Pp, lay, ctx->stream));
  if(sets & (DENS | HYDRO))
    GCHK(copy_s_block(ctx, Sp, lay));
  return sync ? finish_download(ctx, ctx->stream) : GHIP_OK;
}

extern "C" int ghip_download_aos(ghip_ctx *ctx, void *Pp, void *Sp, const ghip_layout *lay,
                                 int want_gravity, int want_density, int want_hydro)
{
  return download_aos_impl(ctx, Pp, Sp, lay, want_gravity, want_density, want_hydro, true);
}

extern "C" int ghip_download_aos_async(ghip_ctx *ctx, void *Pp, void *Sp, const ghip_layout *lay,
                                       int want_gravity, int want_density, int want_hydro)
{
  return download_aos_impl(ctx, Pp, Sp, lay, want_gravity, want_density, want_hydro, false);
}

// gravity_tree()'s post-pass and the gravity fields of P[] for a host that called the SPH drivers
// underneath a pair in flight: ordered after the pair on the pair's own stream, not behind the SPH
// kernels queued on the main stream -- the P[] block crosses the link while hydro's tail still runs.
extern "C" int ghip_gravity_to_records(ghip_ctx *ctx, double G, int pmgrid, double comoving_fac,
                                       void *Pp, const ghip_layout *lay)
{
  if(!ctx || !lay)
    return GHIP_EINVAL;
  GCHK(ghip_tree_verify(ctx));
  if(ctx->n == 0)
    return GHIP_OK;
  GCHK(check_download(ctx, "ghip_gravity_to_records", Pp, nullptr, lay, false));
  // (records with Hsml in P[] carry SPH results in the same block: a download queued on the main
  // stream could then copy the block with stale gravity fields over this one -- everything in order on
  // the main stream for such layouts)
  const bool side = ctx->grav_pending && lay->p_hsml < 0;
  hipStream_t st = ctx->stream;
  if(side)
    st = ctx->stream2;   // (the pair's last kernel, the Ewald sums' combine, is on this stream)
  else
    GHIP_JOIN(ctx);
  GCHK(ghip_gravity_finish_on(ctx, G, pmgrid, comoving_fac, 0, st));
  GCHK(run_records<true>(ctx, rec_map(ctx, lay, B_P, GRAV), ctx->aosP.p, -1, st));
  GCHK(copy_p_block(ctx, Pp, lay, st));
  if(side)
    {
      // whatever the main stream does next comes after the pair and after this
      HIPCHK(hipEventRecord(ctx->ev_side, st));
      HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_side, 0));
      ctx->grav_pending = false;
    }
  return finish_download(ctx, st);
}

// results of ghip_advance_timesteps into the record images (timestep.c: P[].Vel, TimeBin,
// Ti_begstep; SphP[].VelPred, Entropy, e.DtEntropy)
extern "C" int ghip_download_aos_kick(ghip_ctx *ctx, void *Pp, void *Sp, const ghip_layout *lay)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !lay)
    return GHIP_EINVAL;
  if(ctx->n == 0)
    return GHIP_OK;
  GCHK(check_download(ctx, "ghip_download_aos_kick", Pp, Sp, lay, true));
  GCHK(run_records<true>(ctx, rec_map(ctx, lay, B_P, KICK), ctx->aosP.p));
  GCHK(run_records<true>(ctx, rec_map(ctx, lay, B_S, KICK), ctx->aosS.p));
  GCHK(copy_p_block(ctx, Pp, lay, ctx->stream));
  if(ctx->ngas > 0)
    GCHK(copy_s_block(ctx, Sp, lay));
  return finish_download(ctx, ctx->stream);
}

// ---------------------------------------------------------------------------------------------
// page-locked host arrays for the record copies
// ---------------------------------------------------------------------------------------------
extern "C" int ghip_pin_host(ghip_ctx *ctx, void *ptr, size_t bytes)
{
  if(!ctx || !ptr || bytes == 0)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_pin_host: bad arguments");
  (void) hipSetDevice(ctx->device);
  for(void *p : ctx->host_pins)
    if(p == ptr)
      return ghip_fail(ctx, GHIP_EINVAL, "ghip_pin_host: this array is already locked (ghip_unpin_host first)");
  hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterDefault);
  if(e != hipSuccess)
    {
      (void) hipGetLastError();   // not an error of the path: the copies stay staged
      ctx->err = std::string("ghip_pin_host: the range could not be page-locked (") + hipGetErrorString(e) +
                 "); record copies go through the runtime's staging buffers";
      return GHIP_OK;
    }
  ctx->host_pins.push_back(ptr);
  return GHIP_OK;
}

extern "C" int ghip_unpin_host(ghip_ctx *ctx, void *ptr)
{
  if(!ctx)
    return GHIP_EINVAL;
  for(size_t i = 0; i < ctx->host_pins.size(); i++)
    if(ctx->host_pins[i] == ptr)
      {
        // a copy in flight may still read the range
        GHIP_JOIN(ctx);
        (void) ghip_stream_sync(ctx, ctx->stream);
        (void) hipHostUnregister(ptr);
        (void) hipGetLastError();
        ctx->host_pins.erase(ctx->host_pins.begin() + (long) i);
        return GHIP_OK;
      }
  return GHIP_OK;   // never locked (or the lock had failed): nothing to do
}
