// ghip_sequence.hip -- the resident particles rearranged and put in Peano-Hilbert order on the device:
//   ghip_rearrange     rearrange_particle_sequence()   sfr_eff.c:1018-1129 (-DSFR, -DBLACK_HOLES, -DDUST)
//   ghip_peano_order   peano_hilbert_order()           peano.c:25-185
// what domain_Decomposition() runs around its cut (domain.c:120-135, 281-285).  Both are one permutation of the
// records: a map old_of_new[] is made (a scan of survivor flags / a stable pair sort of the two blocks), and ONE
// kernel moves every 8-byte and 4-byte plane of the state along it into shadow buffers, which are then swapped
// in.
#include "ghip_keys.h"
#include "ghip_prim.h"

// words of a call (SeqState::words)
enum { SW_ELIM, SW_GASELIM, SW_DUSTELIM, SW_CONVERTED, SW_OUTSIDE, SW_CHANGED, SW_COUNT = 8 };

// ---- the planes ----------------------------------------------------------------------------------------------
// One plane = one component of one array: [count] words of 8 or 4 bytes.  src is the plane in the old layout, dst
// in the new one (the component offsets, at the old and the new pitch, are already in the pointers).
struct SeqPlane
{
  const void *src;
  void *dst;
  int gas;   // 1: a plane of the gas block (ngas words), 0: of all particles
  int w4;    // 1: 4-byte words
};
#define SEQ_MAXPLANES 64
struct SeqPlanes
{
  int np;
  SeqPlane p[SEQ_MAXPLANES];
};

// dst[j] = src[old_of_new[j]]: thread = destination index, blockIdx.y = plane.  A wavefront writes 64 consecutive
// words of one plane -- full lines -- and only its reads gather; the plane record is wave-uniform (scalar loads).
__global__ void __launch_bounds__(256) k_seq_move(SeqPlanes T, int n_old, int ng_old, int n_new, int ng_new,
                                                  const int *__restrict__ old_of_new)
{
  const SeqPlane pl = T.p[blockIdx.y];
  const int j = blockIdx.x * 256 + threadIdx.x;
  if(j >= (pl.gas ? ng_new : n_new))
    return;
  const int i = old_of_new[j];
  if((unsigned int) i >= (unsigned int) (pl.gas ? ng_old : n_old))
    return;   // (never: the maps are permutations, or name a parent, by construction; a read outside the old layout is refused)
  if(pl.w4)
    reinterpret_cast<unsigned int *>(pl.dst)[j] = reinterpret_cast<const unsigned int *>(pl.src)[i];
  else
    reinterpret_cast<unsigned long long *>(pl.dst)[j] = reinterpret_cast<const unsigned long long *>(pl.src)[i];
}

// ---- rearrange: flags, maps ----------------------------------------------------------------------------------
// survivor flags for ONE scan (gas block: low word, everybody else: high word) and the counts of the call
__global__ void __launch_bounds__(256) k_seq_classify(int n, int ngas, int fix_converted, int eliminate,
                                                      const double *__restrict__ mass, const int *__restrict__ type,
                                                      unsigned long long *__restrict__ v, int *__restrict__ w)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool elim = false, conv = false;
  int ty = 0;
  if(i < n)
    {
      ty = type[i];
      elim = eliminate && mass[i] == 0;
      conv = !elim && fix_converted && i < ngas && ty != 0;
      v[i] = elim ? 0ULL : ((i < ngas && !conv) ? 1ULL : (1ULL << 32));
    }
  const unsigned long long me = __ballot(elim), mg = __ballot(elim && ty == 0), md = __ballot(elim && ty == 2),
                           mc = __ballot(conv);
  if((threadIdx.x & 63) == 0)
    {
      if(me)
        atomicAdd(&w[SW_ELIM], __popcll(me));
      if(mg)
        atomicAdd(&w[SW_GASELIM], __popcll(mg));
      if(md)
        atomicAdd(&w[SW_DUSTELIM], __popcll(md));
      if(mc)
        atomicAdd(&w[SW_CONVERTED], __popcll(mc));
    }
}

__global__ void __launch_bounds__(256) k_seq_maps(int n, int ng_new, const unsigned long long *__restrict__ v,
                                                  const unsigned long long *__restrict__ rank,
                                                  int *__restrict__ new_of_old, int *__restrict__ old_of_new)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if(i >= n)
    return;
  const unsigned long long f = v[i], r = rank[i];
  int j = -1;
  if(f)
    {
      j = (f & 1ULL) ? (int) (r & 0xffffffffULL) : ng_new + (int) (r >> 32);
      old_of_new[j] = i;
    }
  new_of_old[i] = j;
}

__global__ void __launch_bounds__(256) k_seq_iota(int n, int *__restrict__ a, int *__restrict__ b)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if(i < n)
    {
      a[i] = i;
      if(b)
        b[i] = i;
    }
}

// ---- order: keys, the inverse map ----------------------------------------------------------------------------
// domain.c's Key[i]; a position that is not finite or lies outside the cube raises w[SW_OUTSIDE] (d_cell21)
__global__ void __launch_bounds__(256) k_seq_keys(int n, const double *__restrict__ x, const double *__restrict__ y,
                                                  const double *__restrict__ z, double cx, double cy, double cz,
                                                  double fac, unsigned long long *__restrict__ key,
                                                  int *__restrict__ idx, int *__restrict__ w)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if(i >= n)
    return;
  key[i] = d_peano21(d_cell21(x[i], cx, fac, &w[SW_OUTSIDE]), d_cell21(y[i], cy, fac, &w[SW_OUTSIDE]),
                     d_cell21(z[i], cz, fac, &w[SW_OUTSIDE]));
  idx[i] = i;
}

__global__ void __launch_bounds__(256) k_seq_invert(int n, const int *__restrict__ old_of_new,
                                                    int *__restrict__ new_of_old, int *__restrict__ w)
{
  const int j = blockIdx.x * 256 + threadIdx.x;
  if(j >= n)
    return;
  const int i = old_of_new[j];
  new_of_old[i] = j;
  if(i != j)
    w[SW_CHANGED] = 1;
}

// ---- what travels ---------------------------------------------------------------------------------------------
// the optional resident arrays: present = held for the current counts (the rule of migrate_step, ghip_dd.hip)
struct SeqOpt
{
  DevBuf *buf;
  int gas, ncomp, w4;
  bool present;
};

static void seq_optional(ghip_ctx *ctx, SeqOpt o[SEQ_NOPT])
{
  const int n = ctx->n, ng = ctx->ngas;
  const size_t n1 = (size_t) (n > 0 ? n : 1), ng1 = (size_t) (ng > 0 ? ng : 1);
  const bool visc = ctx->visc_alpha.p && ctx->visc_dtalpha.p && ctx->visc_ngas == ng;
  const bool kick = ctx->kick_fields_n == n && ctx->kick_fields_ngas == ng;
  const bool sink = ctx->bh_swallow.p && ctx->bh_swallow.cap >= n1 * 4 && ctx->bh_injected.p &&
                    ctx->bh_injected.cap >= ng1 * 8;
  o[0] = {&ctx->dust_heat, 1, 1, 0, ctx->dust_heat.p && ctx->dust_heat.cap >= ng1 * 8};
  o[1] = {&ctx->visc_alpha, 1, 1, 0, visc};
  o[2] = {&ctx->visc_dtalpha, 1, 1, 0, visc};
  o[3] = {&ctx->wind_inj, 1, 3, 0, ctx->wind_inj.p && ctx->wind_inj_ngas == ng};
  o[4] = {&ctx->wind_ra, 1, 3, 0, ctx->wind_ra.p && ctx->wind_ra_ngas == ng};
  o[5] = {&ctx->bh_swallow, 0, 1, 1, sink};
  o[6] = {&ctx->bh_injected, 1, 1, 0, sink};
  o[7] = {&ctx->kick_drag, 1, 3, 0, kick && ctx->has_drag};
  o[8] = {&ctx->kick_ddm, 1, 3, 0, kick && ctx->has_ddm};
  o[9] = {&ctx->kick_newdens, 0, 1, 0, kick && ctx->has_newdens};
}

// Everything moves along seq.old_of_new into the new counts (nn, ngn), and the rest of the state is what it is
// after a migration: no tree, no kept tree, no lists, everybody active.  Every switch stays.
static int seq_apply(ghip_ctx *ctx, int nn, int ngn)
{
  SeqState &S = ctx->seq;
  DDState &D = ctx->dd;
  hipStream_t st = ctx->stream;
  const int n = ctx->n, ng = ctx->ngas;
  SeqOpt opt[SEQ_NOPT];
  seq_optional(ctx, opt);
  SeqPlanes T;
  T.np = 0;
  long long moved = 0;
  auto add = [&](DevBuf &src, DevBuf &dst, int gas, int ncomp, int w4) {
    const size_t po = (size_t) (gas ? ng : n), pn = (size_t) (gas ? ngn : nn), w = w4 ? 4 : 8;
    for(int c = 0; c < ncomp; c++)
      {
        SeqPlane &pl = T.p[T.np++];
        pl.src = reinterpret_cast<const char *>(src.p) + c * po * w;
        pl.dst = reinterpret_cast<char *>(dst.p) + c * pn * w;
        pl.gas = gas;
        pl.w4 = w4;
        moved += 2 * (long long) (pn * w);
      }
  };
  int planes = 18;   // the optional arrays' 18 planes + the fields' (36 today) must fit the table
  for(int f = 0; f < GHIP_F_COUNT; f++)
    {
      int gas, ncomp, isint;
      ghip_field_info(f, &gas, &ncomp, &isint);
      planes += ncomp;
    }
  if(planes > SEQ_MAXPLANES)
    return ghip_fail(ctx, GHIP_EINVAL, "the plane table of k_seq_move holds %d planes, the state has %d",
                     SEQ_MAXPLANES, planes);
  for(int f = 0; f < GHIP_F_COUNT; f++)
    {
      int gas, ncomp, isint;
      ghip_field_info(f, &gas, &ncomp, &isint);
      const size_t cnt = (size_t) (gas ? ngn : nn);
      GCHK(ghip_ensure(ctx, D.fshadow[f], (cnt > 0 ? cnt : 1) * ncomp * (isint ? 4 : 8)));
      add(ctx->f[f], D.fshadow[f], gas, ncomp, isint);
    }
  for(int k = 0; k < SEQ_NOPT; k++)
    if(opt[k].present)
      {
        const size_t cnt = (size_t) (opt[k].gas ? ngn : nn);
        GCHK(ghip_ensure(ctx, S.xshadow[k], (cnt > 0 ? cnt : 1) * opt[k].ncomp * (opt[k].w4 ? 4 : 8)));
        add(*opt[k].buf, S.xshadow[k], opt[k].gas, opt[k].ncomp, opt[k].w4);
      }
  moved += 4LL * nn * T.np;   // (the map, read once per plane)
  if(nn > 0)
    {
      k_seq_move<<<dim3(cdiv(nn, 256), T.np), 256, 0, st>>>(T, n, ng, nn, ngn, P<int>(S.old_of_new));
      HIPCHK(hipGetLastError());
    }
  HIPCHK(ghip_stream_sync(ctx, st));
  for(int f = 0; f < GHIP_F_COUNT; f++)
    ctx->f[f].swap(D.fshadow[f]);
  for(int k = 0; k < SEQ_NOPT; k++)
    if(opt[k].present)
      opt[k].buf->swap(S.xshadow[k]);
  // an array held for other counts is dropped with the layout it belonged to
  ctx->visc_ngas = opt[1].present ? ngn : -1;
  ctx->visc_epoch++;
  ctx->wind_inj_ngas = opt[3].present ? ngn : -1;
  ctx->wind_ra_ngas = opt[4].present ? ngn : -1;
  ctx->has_drag = opt[7].present;
  ctx->has_ddm = opt[8].present;
  ctx->has_newdens = opt[9].present;
  if(opt[7].present || opt[8].present || opt[9].present)
    {
      ctx->kick_fields_n = nn;
      ctx->kick_fields_ngas = ngn;
    }
  ctx->n = nn;
  ctx->ngas = ngn;
  ctx->gt.built = false;
  ctx->st.built = false;
  D.geom_kept = false;
  ctx->dyn_valid = ctx->dyn_use = false;   // a kept tree is refused until a full build
  ctx->nactive = -1;
  ctx->lists_dirty = ctx->gas_list_dirty = true;
  ctx->pot_n = -1;
  ctx->fof.n = -1;
  ctx->sfr_ncand = -1;   // (the candidates of ghip_sfr_cooling were indices of the old layout)
  S.bytes_moved = moved;
  S.planes = T.np;
  return GHIP_OK;
}

static int seq_identity(ghip_ctx *ctx, int n)
{
  SeqState &S = ctx->seq;
  if(n > 0)
    {
      k_seq_iota<<<cdiv(n, 256), 256, 0, ctx->stream>>>(n, P<int>(S.new_of_old), P<int>(S.old_of_new));
      HIPCHK(hipGetLastError());
    }
  S.n_before = S.n_after = n;
  S.bytes_moved = 0;
  S.planes = 0;
  return GHIP_OK;
}

static int seq_enter(ghip_ctx *ctx, const char *who)
{
  if(ctx->shard_n > 1)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: not on a replicated shard (ghip_set_shard): every rank holds all "
                     "particles there", who);
  HIPCHK(hipSetDevice(ctx->device));
  SeqState &S = ctx->seq;
  const size_t n1 = (size_t) (ctx->n > 0 ? ctx->n : 1);
  const void *before[2] = {S.new_of_old.p, S.old_of_new.p};
  GCHK(ghip_ensure(ctx, S.new_of_old, n1 * 4));
  GCHK(ghip_ensure(ctx, S.old_of_new, n1 * 4));
  if(before[0] != S.new_of_old.p || before[1] != S.old_of_new.p)
    S.n_before = S.n_after = -1;   // (the maps of the last call went with the blocks that grew)
  GCHK(ghip_ensure(ctx, S.words, SW_COUNT * 4));
  HIPCHK(hipMemsetAsync(S.words.p, 0, SW_COUNT * 4, ctx->stream));
  return GHIP_OK;
}

extern "C" int ghip_rearrange(ghip_ctx *ctx, const ghip_rearrange_params *p, ghip_rearrange_result *out)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !p || !out)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_rearrange: bad arguments");
  GCHK(seq_enter(ctx, "ghip_rearrange"));
  SeqState &S = ctx->seq;
  hipStream_t st = ctx->stream;
  const int n = ctx->n, ng = ctx->ngas;
  memset(out, 0, sizeof(*out));
  out->numpart = n;
  out->ngas = ng;
  if(n == 0)
    return seq_identity(ctx, 0);
  GCHK(ghip_ensure(ctx, S.flags, (size_t) (n + 1) * 8));
  GCHK(ghip_ensure(ctx, S.rank, (size_t) (n + 1) * 8));
  unsigned long long *v = P<unsigned long long>(S.flags), *rk = P<unsigned long long>(S.rank);
  HIPCHK(hipMemsetAsync(v + n, 0, 8, st));   // (the extra zero entry makes the last rank the total)
  k_seq_classify<<<cdiv(n, 256), 256, 0, st>>>(n, ng, p->fix_converted != 0, p->eliminate_massless != 0,
                                               P<double>(ctx->f[GHIP_F_MASS]), P<int>(ctx->f[GHIP_F_TYPE]), v,
                                               P<int>(S.words));
  HIPCHK(hipGetLastError());
  GCHK(ghip_scan(ctx, v, rk, n + 1, st));
  unsigned long long tot = 0;
  int w[SW_COUNT];
  HIPCHK(hipMemcpyAsync(&tot, rk + n, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(w, S.words.p, sizeof(w), hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  const int ngn = (int) (tot & 0xffffffffULL), nn = ngn + (int) (tot >> 32);
  if(nn != n - w[SW_ELIM] || ngn > ng || nn > n)
    return ghip_fail(ctx, GHIP_EDEVICE, "ghip_rearrange: %d of %d survive, %d eliminated", nn, n, w[SW_ELIM]);
  out->numpart = nn;
  out->ngas = ngn;
  out->converted = w[SW_CONVERTED];
  out->count_elim = w[SW_ELIM];
  out->count_gaselim = w[SW_GASELIM];
  out->count_dustelim = w[SW_DUSTELIM];
  out->changed = (w[SW_ELIM] || w[SW_CONVERTED]) ? 1 : 0;
  if(!out->changed)
    return seq_identity(ctx, n);
  k_seq_maps<<<cdiv(n, 256), 256, 0, st>>>(n, ngn, v, rk, P<int>(S.new_of_old), P<int>(S.old_of_new));
  HIPCHK(hipGetLastError());
  if(ctx->sk.on && !ctx->sk.stale && w[SW_ELIM])   // the rows of the eliminated Type-5 particles go with them
    GCHK(ghip_sinks_drop_eliminated(ctx, n, P<int>(S.new_of_old)));
  if(ctx->wk.on && !ctx->wk.stale)   // the wind table is keyed by index: it follows the map
    GCHK(ghip_winds_remap(ctx, "ghip_rearrange", n, P<int>(S.new_of_old)));
  GCHK(seq_apply(ctx, nn, ngn));
  S.n_before = n;
  S.n_after = nn;
  // the gas block is what its types say (all gas under fix_converted); an empty one is not mixed
  if(ngn == 0)
    *ghip_gas_mixed_word(ctx) = 0;
  return ghip_check_gas_types(ctx);
}

extern "C" int ghip_peano_order(ghip_ctx *ctx, const double DomainCorner[3], double DomainLen, int *changed)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx)
    return GHIP_EINVAL;
  double corner[3], len = DomainLen;
  if(DomainCorner)
    for(int j = 0; j < 3; j++)
      corner[j] = DomainCorner[j];
  else if(ctx->dd.on && ctx->dlen > 0)
    {
      for(int j = 0; j < 3; j++)
        corner[j] = ctx->corner[j];
      len = ctx->dlen;
    }
  else
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_peano_order: DomainCorner == NULL needs a ghip_dd_init context whose "
                     "domain is set (ghip_dd_set_domain, GHIP_DD_DECOMPOSE)");
  if(!(len > 0) || !(len < 1e300) || !(corner[0] - corner[0] == 0) || !(corner[1] - corner[1] == 0) ||
     !(corner[2] - corner[2] == 0))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_peano_order: the domain needs finite corners and DomainLen > 0");
  GCHK(seq_enter(ctx, "ghip_peano_order"));
  SeqState &S = ctx->seq;
  hipStream_t st = ctx->stream;
  const int n = ctx->n, ng = ctx->ngas;
  if(changed)
    *changed = 0;
  if(n == 0)
    return seq_identity(ctx, 0);
  GCHK(ghip_ensure(ctx, S.key, (size_t) n * 8));
  GCHK(ghip_ensure(ctx, S.skey, (size_t) n * 8));
  GCHK(ghip_ensure(ctx, S.idx, (size_t) n * 4));
  GCHK(ghip_ensure(ctx, S.sidx, (size_t) n * 4));
  const double *x = P<double>(ctx->f[GHIP_F_POS]);
  const double fac = 1.0 / len * (double) (1ULL << GHIP_BITS);
  unsigned long long *key = P<unsigned long long>(S.key), *skey = P<unsigned long long>(S.skey);
  int *idx = P<int>(S.idx), *sidx = P<int>(S.sidx), *w = P<int>(S.words);
  k_seq_keys<<<cdiv(n, 256), 256, 0, st>>>(n, x, x + n, x + 2 * (size_t) n, corner[0], corner[1], corner[2], fac,
                                           key, idx, w);
  HIPCHK(hipGetLastError());
  // the two blocks, each stably (mysort_peano is a merge sort that takes the left run on equal keys)
  if(ng > 0)
    GCHK(ghip_sort_pairs(ctx, key, skey, idx, sidx, ng, 3 * GHIP_BITS, st));
  if(n - ng > 0)
    GCHK(ghip_sort_pairs(ctx, key + ng, skey + ng, idx + ng, sidx + ng, n - ng, 3 * GHIP_BITS, st));
  // (into the work arrays: the maps of the last call stay in place if this one is refused)
  k_seq_invert<<<cdiv(n, 256), 256, 0, st>>>(n, sidx, idx, w);
  HIPCHK(hipGetLastError());
  int hw[SW_COUNT];
  HIPCHK(hipMemcpyAsync(hw, w, sizeof(hw), hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  if(hw[SW_OUTSIDE])
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_peano_order: a position is not finite or lies outside the cube "
                     "[corner, corner + %g): nothing was moved", len);
  if(!hw[SW_CHANGED])
    return seq_identity(ctx, n);
  S.old_of_new.swap(S.sidx);
  S.new_of_old.swap(S.idx);
  if(ctx->wk.on && !ctx->wk.stale)
    GCHK(ghip_winds_remap(ctx, "ghip_peano_order", n, P<int>(S.new_of_old)));
  GCHK(seq_apply(ctx, n, ng));
  S.n_before = S.n_after = n;
  if(changed)
    *changed = 1;
  return GHIP_OK;
}

extern "C" int ghip_sequence_get_map(ghip_ctx *ctx, int *new_of_old, int *old_of_new)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx)
    return GHIP_EINVAL;
  SeqState &S = ctx->seq;
  if(S.n_before < 0)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_sequence_get_map: no ghip_rearrange / ghip_peano_order yet");
  hipStream_t st = ctx->stream;
  if(new_of_old && S.n_before > 0)
    HIPCHK(hipMemcpyAsync(new_of_old, S.new_of_old.p, (size_t) S.n_before * 4, hipMemcpyDeviceToHost, st));
  if(old_of_new && S.n_after > 0)
    HIPCHK(hipMemcpyAsync(old_of_new, S.old_of_new.p, (size_t) S.n_after * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  return GHIP_OK;
}

extern "C" int ghip_sequence_get_info(ghip_ctx *ctx, long long out[4])
{
  if(!ctx || !out)
    return GHIP_EINVAL;
  out[0] = ctx->seq.n_before;
  out[1] = ctx->seq.n_after;
  out[2] = ctx->seq.bytes_moved;
  out[3] = ctx->seq.planes;
  return GHIP_OK;
}

// ---- growth (ghip_wind_spawn) ----------------------------------------------------------------------------------
// The one operation above that is not a permutation: the state goes from n to nn > n particles, and every record
// behind the old ones is a copy of an old record (its parent sink), P[NumPart + stars_spawned] = P[i].
int ghip_seq_grow_begin(ghip_ctx *ctx, int nn, int **old_of_new)
{
  SeqState &S = ctx->seq;
  if(nn < ctx->n)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_seq_grow: %d particles cannot grow to %d", ctx->n, nn);
  GCHK(ghip_ensure(ctx, S.old_of_new, (size_t) (nn > 0 ? nn : 1) * 4));
  GCHK(ghip_ensure(ctx, S.new_of_old, (size_t) (ctx->n > 0 ? ctx->n : 1) * 4));
  S.n_before = S.n_after = -1;   // (the maps of the last call are overwritten)
  *old_of_new = P<int>(S.old_of_new);
  return GHIP_OK;
}

int ghip_seq_grow_apply(ghip_ctx *ctx, int nn)
{
  SeqState &S = ctx->seq;
  const int n = ctx->n, ng = ctx->ngas;
  if(n > 0)
    {
      k_seq_iota<<<cdiv(n, 256), 256, 0, ctx->stream>>>(n, P<int>(S.new_of_old), nullptr);
      HIPCHK(hipGetLastError());
    }
  // k_seq_move with a map that is not a permutation and nn > n: thread j < nn writes dst[j] of a plane sized for nn
  // (seq_apply sizes the shadows by the new counts) and reads src[old_of_new[j]], which it refuses outside [0, n);
  // several j may read the same source.  A gas plane has ngn = ng <= n threads, and the map is the identity there.
  GCHK(seq_apply(ctx, nn, ng));
  S.n_before = n;
  S.n_after = nn;
  return GHIP_OK;
}
