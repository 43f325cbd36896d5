// ghip_dd.hip -- multi-GPU force path: Peano-Hilbert domain decomposition with tree-node and
// ghost-particle exchange.
//
// Replaces, for a run sharded over the GPUs of one node (one process per GPU):
//   domain_Decomposition / domain_findSplit_work_balanced     domain.c:100, 378-384, 1075-1113
//   force_create_empty_nodes / force_insert_pseudo_particles /
//   force_exchange_pseudodata / force_treeupdate_pseudos       forcetree.c:384-450, 879-1075
//   the export rounds of gravity_tree / density / hydro_force   gravtree.c:175-339, density.c:193-389,
//                                                               hydra.c:274-526
//
// The reference keeps one global oct-tree whose top part is replicated; a target whose walk opens
// another rank's top-leaf is EXPORTED there, walked remotely, and the partial sum comes back --
// rounds of small messages driven by the host.  On a node of GPUs with point-to-point xGMI links the
// data goes the other way, once per phase:
//   gravity   every shard sends every other shard the part of its tree that shard can possibly need
//             (a LOCALLY ESSENTIAL TREE): walking its own tree top-down against the receiver's
//             target groups (bounding boxes + the least OldAcc inside), a node that no target of the
//             receiver can open under the reference's opening rules is sent as ONE element with its
//             moments ("pruned node"), anything that could be opened is descended, particles that
//             are reached are sent as particles.  The receiver sorts its own particles and the
//             imported elements by key and builds ONE tree over both (ghip_tree.hip): cells shared
//             by several shards are re-created from their parts, so every node a target can test
//             has the moments of the global tree, and the walk (ghip_walk.h, unchanged) makes for
//             each target exactly the opening decisions of the reference's single global tree --
//             the interaction set is the same for every number of shards, as in the reference
//             (domain.c:20-22).  If a target ever has to open a pruned node the walk raises a
//             device error instead of losing mass.
//   SPH       gas particles within the (padded) search radius of another shard's target groups, or
//             whose own smoothing sphere reaches them, are sent as GHOSTS before density(); their
//             updated records follow once between density() and hydro_force().
// Ownership is by Peano-Hilbert key range [splits[r], splits[r+1]): a cell lies wholly inside a
// shard's range or it is "shared" and always descended.  With ghip_dd_set_guests a shard may hold
// particles outside its range (guests, between two migrations): a cell whose range holds the key of a
// guest held elsewhere is shared too, which its owner learns from the guests' keys (k_let_level).
#include <cstdarg>

#include "ghip_ngb.h"   // BoxK
#include "ghip_keys.h"
#include "ghip_prim.h"

// tree.hip
int ghip_dd_build_gas_tree(ghip_ctx *ctx);
int ghip_dd_refresh_ghosts(ghip_ctx *ctx);
void ghip_dd_comm_release(ghip_ctx *ctx);
extern "C" int ghip_dd_exchange(ghip_ctx *ctx);

// ---------------------------------------------------------------------------------------------
// set-up
// ---------------------------------------------------------------------------------------------
static int dd_store_segments(ghip_ctx *ctx, int nseg, const unsigned long long *keys, const int *owner);
extern "C" int ghip_dd_init(ghip_ctx *ctx, int rank, int nranks)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || nranks < 1 || nranks > GHIP_MAXRANKS || rank < 0 || rank >= nranks)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_init: need 0 <= rank < nranks <= %d", GHIP_MAXRANKS);
  DDState &D = ctx->dd;
  D.on = true;
  D.rank = rank;
  D.nranks = nranks;
  for(int r = 0; r <= nranks; r++)   // default: equal key ranges
    D.splits[r] = (r == nranks) ? (1ULL << 63) : ((1ULL << 63) / (unsigned long long) nranks) * r;
  D.gt_nimp = 0;
  D.nghost = 0;
  D.op = 0;   // (a new set-up abandons whatever operation was in progress, with its pending exchange)
  D.x.kind = 0;
  ctx->gt.built = false;
  ctx->st.built = false;
  ctx->dd.geom_kept = false;
  ctx->shard_rank = 0;   // (the replicated-source sharding of ghip_set_shard is a different mode)
  ctx->shard_n = 1;
  return ghip_dd_set_splits(ctx, D.splits);
}

extern "C" int ghip_dd_set_domain(ghip_ctx *ctx, const double corner[3], const double center[3],
                                  double len, const double soft[6])
{
  if(!ctx || !corner || !center || !soft || !(len > 0))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_set_domain: bad arguments");
  for(int j = 0; j < 3; j++)
    {
      ctx->corner[j] = corner[j];
      ctx->center[j] = center[j];
    }
  ctx->dlen = len;
  for(int j = 0; j < 6; j++)
    ctx->soft[j] = soft[j];
  ctx->gt.built = false;
  ctx->st.built = false;
  ctx->dd.geom_kept = false;
  return GHIP_OK;
}

// ownership of the curve: merge neighbours of one owner, drop empty pieces, keep device copies
static int dd_store_segments(ghip_ctx *ctx, int nseg, const unsigned long long *keys, const int *owner)
{
  DDState &D = ctx->dd;
  std::vector<unsigned long long> k, lo, hi;
  std::vector<int> o;
  for(int s = 0; s < nseg; s++)
    {
      if(keys[s + 1] == keys[s])
        continue;
      if(!o.empty() && o.back() == owner[s])
        continue;   // (same owner as the piece before: one piece)
      k.push_back(keys[s]);
      o.push_back(owner[s]);
    }
  if(k.empty() || k[0] != 0)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd: the key ranges do not start at 0");
  k.push_back(1ULL << 63);
  const int m = (int) o.size();
  for(int s = 0; s < m; s++)
    if(o[s] == D.rank)
      {
        lo.push_back(k[s]);
        hi.push_back(k[s + 1]);
      }
  D.nseg = m;
  D.nown = (int) lo.size();
  GCHK(ghip_ensure(ctx, D.segkey, (size_t) (m + 1) * 8));
  GCHK(ghip_ensure(ctx, D.segowner, (size_t) m * 4));
  GCHK(ghip_ensure(ctx, D.ownlo, (size_t) (D.nown > 0 ? D.nown : 1) * 8));
  GCHK(ghip_ensure(ctx, D.ownhi, (size_t) (D.nown > 0 ? D.nown : 1) * 8));
  HIPCHK(hipMemcpy(D.segkey.p, k.data(), (size_t) (m + 1) * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(D.segowner.p, o.data(), (size_t) m * 4, hipMemcpyHostToDevice));
  if(D.nown > 0)
    {
      HIPCHK(hipMemcpy(D.ownlo.p, lo.data(), (size_t) D.nown * 8, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(D.ownhi.p, hi.data(), (size_t) D.nown * 8, hipMemcpyHostToDevice));
    }
  return GHIP_OK;
}

extern "C" int ghip_dd_set_splits(ghip_ctx *ctx, const unsigned long long *splits)
{
  if(!ctx || !splits || !ctx->dd.on)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_set_splits: call ghip_dd_init first");
  DDState &D = ctx->dd;
  for(int r = 0; r <= D.nranks; r++)
    {
      if(r > 0 && splits[r] < splits[r - 1])
        return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_set_splits: keys must not decrease");
      D.splits[r] = splits[r];
    }
  if(D.splits[0] != 0 || D.splits[D.nranks] < (1ULL << 63))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_set_splits: the ranges must cover [0, 2^63)");
  std::vector<unsigned long long> keys(D.splits, D.splits + D.nranks + 1);
  std::vector<int> owner(D.nranks);
  for(int r = 0; r < D.nranks; r++)
    owner[r] = r;
  D.seg_layout = false;
  return dd_store_segments(ctx, D.nranks, keys.data(), owner.data());
}

extern "C" int ghip_dd_set_segments(ghip_ctx *ctx, int nseg, const unsigned long long *keys, const int *owner)
{
  if(!ctx || !keys || !owner || !ctx->dd.on || nseg < 1)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_set_segments: call ghip_dd_init first; nseg >= 1");
  DDState &D = ctx->dd;
  for(int s = 0; s < nseg; s++)
    {
      if(keys[s + 1] < keys[s])
        return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_set_segments: keys must not decrease");
      if(owner[s] < 0 || owner[s] >= D.nranks)
        return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_set_segments: owner %d of segment %d is not a rank", owner[s], s);
    }
  if(keys[0] != 0 || keys[nseg] < (1ULL << 63))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_set_segments: the segments must cover [0, 2^63)");
  GCHK(dd_store_segments(ctx, nseg, keys, owner));
  D.seg_layout = true;
  return GHIP_OK;
}

extern "C" int ghip_dd_get_splits(const ghip_ctx *ctx, unsigned long long *splits)
{
  if(!ctx || !splits || !ctx->dd.on || ctx->dd.seg_layout)   // (a ghip_dd_set_segments layout is not nranks+1 keys)
    return GHIP_EINVAL;
  for(int r = 0; r <= ctx->dd.nranks; r++)
    splits[r] = ctx->dd.splits[r];
  return GHIP_OK;
}

extern "C" int ghip_dd_get_domain(const ghip_ctx *ctx, double corner[3], double center[3], double *len)
{
  if(!ctx || !corner || !center || !len)
    return GHIP_EINVAL;
  for(int j = 0; j < 3; j++)
    {
      corner[j] = ctx->corner[j];
      center[j] = ctx->center[j];
    }
  *len = ctx->dlen;
  return GHIP_OK;
}

extern "C" int ghip_dd_set_ghost_margin(ghip_ctx *ctx, double margin)
{
  if(!ctx || !(margin >= 1.0))
    return GHIP_EINVAL;
  ctx->dd.gh_margin = margin;
  return GHIP_OK;
}

// domain_findSplit_work_balanced (domain.c:1075-1113) with equal speed factors: cut `ndomain`
// curve-ordered pieces of work into `ncpu` contiguous ranges so that the running sum follows the
// running average.  Pure host arithmetic (also what the CPU tests of the multi-rank logic call).
extern "C" int ghip_dd_find_split(int ncpu, int ndomain, const double *domainWork, int *start,
                                  int *end)
{
  if(ncpu < 1 || ndomain < ncpu || !domainWork || !start || !end)
    return GHIP_EINVAL;
  double work = 0;
  for(int i = 0; i < ndomain; i++)
    work += domainWork[i];
  const double workavg = work / ncpu;
  double work_before = 0, workavg_before = 0;
  int s = 0;
  for(int i = 0; i < ncpu; i++)
    {
      int e = s;
      work = domainWork[e];
      while((work + work_before < workavg + workavg_before) || (i == ncpu - 1 && e < ndomain - 1))
        {
          if((ndomain - e) > (ncpu - i))
            e++;
          else
            break;
          work += domainWork[e];
        }
      start[i] = s;
      end[i] = e;
      work_before += work;
      workavg_before += workavg;
      s = e + 1;
    }
  return GHIP_OK;
}

// Peano-Hilbert keys (21 bits per dimension, peano.c:300) of the resident particles in the domain
// cube of ghip_dd_set_domain / ghip_tree_build: what the decomposition orders and cuts
__global__ void k_dd_ph_keys(int n, const double *__restrict__ x, const double *__restrict__ y,
                             const double *__restrict__ z, double cx, double cy, double cz,
                             double fac, unsigned long long *__restrict__ key)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  key[i] = d_peano21(d_cell21(x[i], cx, fac), d_cell21(y[i], cy, fac), d_cell21(z[i], cz, fac));
}

extern "C" int ghip_dd_keys(ghip_ctx *ctx, unsigned long long *keys_host)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !keys_host || !(ctx->dlen > 0))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_keys: set the domain first");
  const int n = ctx->n;
  if(n == 0)
    return GHIP_OK;
  GCHK(ghip_ensure(ctx, ctx->stage, (size_t) n * 8));
  const double *x = P<double>(ctx->f[GHIP_F_POS]);
  const double fac = 1.0 / ctx->dlen * (double) (1ULL << GHIP_BITS);
  k_dd_ph_keys<<<cdiv(n, 256), 256, 0, ctx->stream>>>(n, x, x + n, x + 2 * (size_t) n, ctx->corner[0],
                                                      ctx->corner[1], ctx->corner[2], fac,
                                                      P<unsigned long long>(ctx->stage));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(keys_host, ctx->stage.p, (size_t) n * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  return GHIP_OK;
}

// every local particle must lie in this shard's key range (the host's domain decomposition, or
// ghip's own migration, guarantees it): a stray would be counted in nobody's cells
// does [lo, hi) lie inside ONE of this rank's own pieces of the curve?
__device__ __forceinline__ bool d_owned_range(unsigned long long lo, unsigned long long hi, int nown,
                                              const unsigned long long *__restrict__ ownlo,
                                              const unsigned long long *__restrict__ ownhi)
{
  int a = 0, b = nown - 1, j = -1;   // largest j with ownlo[j] <= lo
  while(a <= b)
    {
      int mid = (a + b) >> 1;
      if(ownlo[mid] <= lo)
        {
          j = mid;
          a = mid + 1;
        }
      else
        b = mid - 1;
    }
  return j >= 0 && hi <= ownhi[j];
}

__global__ void k_dd_check_range(int n, const double *__restrict__ x, const double *__restrict__ y,
                                 const double *__restrict__ z, double cx, double cy, double cz,
                                 double fac, int nown, const unsigned long long *__restrict__ ownlo,
                                 const unsigned long long *__restrict__ ownhi,
                                 int *__restrict__ errword)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  // (a particle outside the domain cube: error 6, the host must give a fresh extent first)
  unsigned long long k = d_peano21(d_cell21(x[i], cx, fac, errword), d_cell21(y[i], cy, fac, errword),
                                   d_cell21(z[i], cz, fac, errword));
  if(!d_owned_range(k, k + 1, nown, ownlo, ownhi))
    *(volatile int *) errword = 5;
}

// ghip_dd_set_guests: the same key, and in place of the error the guest's key and the shard that owns it (its
// host, found as the migration finds a destination: the last piece that starts at or before the key)
__global__ void k_dd_mark_guests(int n, const double *__restrict__ x, const double *__restrict__ y,
                                 const double *__restrict__ z, double cx, double cy, double cz,
                                 double fac, int nown, const unsigned long long *__restrict__ ownlo,
                                 const unsigned long long *__restrict__ ownhi, int nseg,
                                 const unsigned long long *__restrict__ segkey,
                                 const int *__restrict__ segowner, unsigned long long *__restrict__ key,
                                 unsigned long long *__restrict__ mask, int *__restrict__ errword)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  // (a particle outside the domain cube stays error 6)
  const unsigned long long k = d_peano21(d_cell21(x[i], cx, fac, errword), d_cell21(y[i], cy, fac, errword),
                                         d_cell21(z[i], cz, fac, errword));
  unsigned long long m = 0;
  if(!d_owned_range(k, k + 1, nown, ownlo, ownhi))
    {
      int lo = 0, hi = nseg - 1;   // largest s with segkey[s] <= k
      while(lo < hi)
        {
          int mid = (lo + hi + 1) >> 1;
          if(segkey[mid] <= k)
            lo = mid;
          else
            hi = mid - 1;
        }
      m = 1ULL << segowner[lo];
    }
  key[i] = k;
  mask[i] = m;
}

__global__ void k_dd_gather_u64(int n, const int *__restrict__ list, const unsigned long long *__restrict__ in,
                                unsigned long long *__restrict__ out)
{
  int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a < n)
    out[a] = in[list[a]];
}

// ---------------------------------------------------------------------------------------------
// target groups
// ---------------------------------------------------------------------------------------------
// minimum of every mn[] and maximum of every mx[] over the 64 lanes (in every lane), all in one butterfly.
// UNROLL writes its six steps out: the lane offsets become constants, which suits the selection kernel
// (2 vector registers fewer) and not the group kernels (13 more)
template <bool UNROLL, int NMIN, int NMAX>
__device__ __forceinline__ void d_wave_minmax(double (&mn)[NMIN], double (&mx)[NMAX])
{
  constexpr int steps = UNROLL ? 6 : 1;
#pragma unroll steps
  for(int off = 32; off > 0; off >>= 1)
    {
      for(int k = 0; k < NMIN; k++)
        {
          const double o = __shfl_xor(mn[k], off, 64);
          mn[k] = o < mn[k] ? o : mn[k];
        }
      for(int k = 0; k < NMAX; k++)
        {
          const double o = __shfl_xor(mx[k], off, 64);
          mx[k] = o > mx[k] ? o : mx[k];
        }
    }
}

// half extent of [lo, hi], rounded up a little: the box must contain every point.  `pad` covers the
// rounding of the centre: 1e-14 * (|c| + 1e-300) in the group tables, a bare 1e-14 for the chunk boxes
// of the selection kernel
__device__ __forceinline__ double d_half_extent(double lo, double hi, double pad)
{
  return 0.5 * (hi - lo) * (1 + 1e-12) + pad;
}

// the table entry of the box [lo, hi]; any = false: an empty group, which no test reaches
__device__ __forceinline__ DDGroup d_group_of_box(bool any, const double *lo, const double *hi,
                                                  double amin, double rmax)
{
  DDGroup G;
  if(any)
    {
      G.cx = 0.5 * (lo[0] + hi[0]);
      G.cy = 0.5 * (lo[1] + hi[1]);
      G.cz = 0.5 * (lo[2] + hi[2]);
      G.ex = d_half_extent(lo[0], hi[0], 1e-14 * (fabs(G.cx) + 1e-300));
      G.ey = d_half_extent(lo[1], hi[1], 1e-14 * (fabs(G.cy) + 1e-300));
      G.ez = d_half_extent(lo[2], hi[2], 1e-14 * (fabs(G.cz) + 1e-300));
      G.amin = amin;
      G.rmax = rmax;
    }
  else
    {
      G.cx = G.cy = G.cz = 0;
      G.ex = G.ey = G.ez = -1;
      G.amin = 1e300;
      G.rmax = 0;
    }
  return G;
}

// one wavefront per group of `gsz` consecutive targets of the curve-ordered list (indices of the
// gravity tree): positions in tree order, val (OldAcc or Hsml, host order) through perm
__global__ void __launch_bounds__(64)
k_dd_groups(int nt, int gsz, const int *__restrict__ tgt, const double *__restrict__ sx,
            const double *__restrict__ sy, const double *__restrict__ sz,
            const int *__restrict__ perm, const double *__restrict__ val, double margin,
            DDGroup *__restrict__ out)
{
  const int g = blockIdx.x, lane = threadIdx.x;
  const long long a0l = (long long) g * gsz;
  const int a0 = a0l > nt ? nt : (int) a0l;
  int a1 = (a0l + gsz > nt) ? nt : (int) (a0l + gsz);
  double lo[4] = {1e300, 1e300, 1e300, 1e300}, hi[4] = {-1e300, -1e300, -1e300, 0};   // x, y, z, val
  for(int a = a0 + lane; a < a1; a += 64)
    {
      const int s = tgt[a];
      const double p[4] = {sx[s], sy[s], sz[s], val[perm[s]]};
      for(int k = 0; k < 4; k++)
        {
          lo[k] = p[k] < lo[k] ? p[k] : lo[k];
          hi[k] = p[k] > hi[k] ? p[k] : hi[k];
        }
    }
  d_wave_minmax<false>(lo, hi);
  if(lane == 0)
    out[DD_NSUPER + g] = d_group_of_box(a1 > a0, lo, hi, lo[3], hi[3] * margin);
}

// super-group s = union of groups [s*DD_NSUB, (s+1)*DD_NSUB)
__global__ void __launch_bounds__(64) k_dd_supergroups(DDGroup *__restrict__ tab)
{
  const int s = blockIdx.x, lane = threadIdx.x;
  double lo[4] = {1e300, 1e300, 1e300, 1e300}, hi[4] = {-1e300, -1e300, -1e300, 0};   // x, y, z, amin / rmax
  if(lane < DD_NSUB)
    {
      const DDGroup G = tab[DD_NSUPER + s * DD_NSUB + lane];
      if(G.ex >= 0)
        {
          lo[0] = G.cx - G.ex;
          hi[0] = G.cx + G.ex;
          lo[1] = G.cy - G.ey;
          hi[1] = G.cy + G.ey;
          lo[2] = G.cz - G.ez;
          hi[2] = G.cz + G.ez;
          lo[3] = G.amin;
          hi[3] = G.rmax;
        }
    }
  d_wave_minmax<false>(lo, hi);
  if(lane == 0)
    tab[s] = d_group_of_box(hi[0] >= lo[0], lo, hi, lo[3], hi[3]);
}

// target list `tgt` (indices of the gravity tree, curve order).  gas = false: groups carry the least
// OldAcc; gas = true: the largest smoothing length times the ghost margin.  val: another per-particle
// array in place of OldAcc (for a caller whose tests do not read amin and that may hold no OldAcc).
static int build_groups(ghip_ctx *ctx, bool gas, const int *tgt, int nt, const double *val = nullptr)
{
  DDState &D = ctx->dd;
  hipStream_t st = ctx->stream;
  GCHK(ghip_ensure(ctx, D.grp_own, (size_t) DD_STRIDE * sizeof(DDGroup)));
  DDGroup *tab = P<DDGroup>(D.grp_own);
  int gsz = (nt + DD_NGROUPS - 1) / DD_NGROUPS;
  if(gsz < 1)
    gsz = 1;
  k_dd_groups<<<DD_NGROUPS, 64, 0, st>>>(nt, gsz, tgt, P<double>(ctx->sx), P<double>(ctx->sy),
                                         P<double>(ctx->sz), P<int>(ctx->gt.perm),
                                         val ? val : P<double>(ctx->f[gas ? GHIP_F_HSML : GHIP_F_OLDACC]),
                                         gas ? D.gh_margin_cur : 1.0, tab);
  k_dd_supergroups<<<DD_NSUPER, 64, 0, st>>>(tab);
  HIPCHK(hipGetLastError());
  // the status record behind the table: has anything gone wrong on this shard so far?  (The error,
  // if any, is kept: after the all-gather every shard fails, this one with its own message.)
  HIPCHK(ghip_stream_sync(ctx, st));
  DDGroup status;
  memset(&status, 0, sizeof(status));
  status.cx = ghip_dd_hold(ctx, ghip_check_device_errors(ctx)) ? 1.0 : 0.0;
  status.cy = D.guests_on ? (double) D.guests_held : 0.0;
  HIPCHK(hipMemcpyAsync(tab + DD_TABLE, &status, sizeof(status), hipMemcpyHostToDevice, st));
  HIPCHK(ghip_stream_sync(ctx, st));   // (`status` lives on this frame)
  return GHIP_OK;
}

// after the all-gather of the group tables: did every shard get this far without an error?
__global__ void k_dd_collect_status(int nranks, const DDGroup *__restrict__ all, double *__restrict__ out)
{
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  if(r < nranks)
    {
      out[r] = all[(size_t) r * DD_STRIDE + DD_TABLE].cx;
      out[nranks + r] = all[(size_t) r * DD_STRIDE + DD_TABLE].cy;
    }
}

// guests (if asked for): the guests all shards hold together, as the gravity tree's guest pass counted them
static int check_group_status(ghip_ctx *ctx, const char *what, long long *guests = nullptr)
{
  DDState &D = ctx->dd;
  hipStream_t st = ctx->stream;
  const int P_ = D.nranks;
  GCHK(ghip_ensure(ctx, D.status_all, (size_t) GHIP_MAXRANKS * 2 * 8));
  k_dd_collect_status<<<1, 64, 0, st>>>(P_, P<DDGroup>(D.grp_all), P<double>(D.status_all));
  double flags[2 * GHIP_MAXRANKS];
  HIPCHK(hipMemcpyAsync(flags, D.status_all.p, (size_t) P_ * 16, hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  int failed = -1;
  long long held = 0;
  for(int r = 0; r < P_; r++)
    {
      if(flags[r] != 0 && failed < 0)
        failed = r;
      held += (long long) flags[P_ + r];
    }
  if(guests)
    *guests = held;
  return ghip_dd_raise(ctx, failed, "%s: shard %d reported an error while it prepared its target "
                       "groups (its own message says what); every shard stops here", what, failed);
}

// ---- all shards stop together (ghip_internal.h): the held failure, and the status round it can travel in ----
bool ghip_dd_hold(ghip_ctx *ctx, int rc)
{
  ctx->dd.held.rc = rc;
  if(rc != GHIP_OK)
    ctx->dd.held.msg = ctx->err;
  return rc != GHIP_OK;
}

int ghip_dd_raise(ghip_ctx *ctx, int failed_rank, const char *fmt, ...)
{
  if(failed_rank < 0)
    return GHIP_OK;
  if(ctx->dd.held.rc != GHIP_OK)
    return ghip_fail(ctx, ctx->dd.held.rc, "%s", ctx->dd.held.msg.c_str());
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return ghip_fail(ctx, GHIP_EDEVICE, "%s", buf);
}

int dd_post_status(ghip_ctx *ctx, double value, bool failed)
{
  DDState &D = ctx->dd;
  const double mine[2] = {value, failed ? 1.0 : 0.0};
  GCHK(ghip_ensure(ctx, D.status_own, 16));
  HIPCHK(hipMemcpyAsync(D.status_own.p, mine, 16, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));   // (`mine` lives on this frame)
  ghip_dd_set_allgather(D, D.status_own.p, 16, &D.status_all);
  return GHIP_OK;
}

int dd_read_status(ghip_ctx *ctx, double *worst, int *first_failed)
{
  DDState &D = ctx->dd;
  double all[2 * GHIP_MAXRANKS];
  HIPCHK(hipMemcpyAsync(all, D.status_all.p, (size_t) D.nranks * 16, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  *worst = 0;
  *first_failed = -1;
  for(int r = 0; r < D.nranks; r++)
    {
      if(all[2 * r] > *worst)
        *worst = all[2 * r];
      if(all[2 * r + 1] != 0 && *first_failed < 0)
        *first_failed = r;
    }
  return GHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// gravity: selection of the locally essential trees
// ---------------------------------------------------------------------------------------------
struct LetK
{
  double theta2;     // ErrTolTheta^2 (0: relative criterion)
  double errtol;     // ErrTolForceAcc
  BoxK b;
  int unequal;
  int nranks, me;
  int nown;                                   // this rank's own pieces of the curve
  const unsigned long long *ownlo, *ownhi;
  int nguest;                                 // guests other shards hold inside this rank's pieces:
  const unsigned long long *guest;            // their keys in ascending order (ghip_dd_set_guests)
};

// squared distance between the box (c +- e; e = 0: a point) and the group's box, component-wise, with
// the nearest image when periodic (forcetree.c:2028-2032)
__device__ __forceinline__ double d_group_box_dist2(const DDGroup &G, double cx, double cy, double cz, double ex,
                                                    double ey, double ez, const BoxK &b)
{
  double d0 = cx - G.cx, d1 = cy - G.cy, d2 = cz - G.cz;
  if(b.periodic)
    {
      d0 = d_nearest(d0, b.boxsize, b.boxhalf);
      d1 = d_nearest(d1, b.boxsize, b.boxhalf);
      d2 = d_nearest(d2, b.boxsize, b.boxhalf);
    }
  d0 = fabs(d0) - G.ex - ex;
  d1 = fabs(d1) - G.ey - ey;
  d2 = fabs(d2) - G.ez - ez;
  d0 = d0 > 0 ? d0 : 0;
  d1 = d1 > 0 ? d1 : 0;
  d2 = d2 > 0 ? d2 : 0;
  return d0 * d0 + d1 * d1 + d2 * d2;
}

// Can ANY target inside the group's box (with OldAcc >= G.amin) open this node under the rules of
// force_treeevaluate (forcetree.c:2074-2139) and its short-range / Ewald variants (which open a
// subset)?  Conservative: a 1e-9 slack absorbs the rounding of the per-target arithmetic.
__device__ __forceinline__ bool d_group_can_open(const DDGroup &G, const double4 &xm, const double4 &cl,
                                                 double aux, const LetK &K)
{
  if(G.ex < 0)
    return false;
  const double slack = 1.0 - 1.0e-9;
  const double r2 = d_group_box_dist2(G, xm.x, xm.y, xm.z, 0, 0, 0, K.b) * slack;
  const double len = cl.w;
  if(K.theta2 != 0)
    {
      if(len * len >= r2 * K.theta2)   // forcetree.c:2076
        return true;
    }
  else
    {
      if(xm.w * len * len >= r2 * r2 * (K.errtol * G.amin))   // forcetree.c:2085
        return true;
      // forcetree.c:2093-2104: a target inside the 1.2*len box around the cell's centre (plain
      // coordinate differences, as the reference takes them)
      const double lim = 0.60 * len * (1.0 + 1.0e-9);
      if(fabs(cl.x - G.cx) - G.ex < lim && fabs(cl.y - G.cy) - G.ey < lim &&
         fabs(cl.z - G.cz) - G.ez < lim)
        return true;
    }
  // forcetree.c:2108-2139: a node that mixes softenings (or any node under
  // ADAPTIVE_GRAVSOFT_FORGAS) is opened by a softer target closer than the largest softening below
  if(K.unequal && aux < 0 && r2 < aux * aux)
    return true;
  return false;
}

__global__ void k_let_init(int nelem, unsigned long long allmask, unsigned long long *__restrict__ reach,
                           unsigned long long *__restrict__ sendm)
{
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if(e >= nelem)
    return;
  reach[e] = (e == 0) ? allmask : 0ULL;   // element 0 is the root cell (or the only particle)
  sendm[e] = 0ULL;
}

__device__ __forceinline__ double d_bcast(double v, int j)
{
  return __shfl(v, j, 64);
}

// One level of the top-down pass: a node some rank reaches is either left as it is for that rank
// (pruned: sent as one element) or descended (its children become reachable).
// One wavefront per LET_EPW consecutive elements (the candidates of a wavefront are tested one after
// the other, so few per wavefront keep a level's launch short; all 64 lanes take part in every
// test).  Lane-parallel: which of them are nodes of this level
// that somebody reaches, and does the cell lie wholly inside this shard's key range.  Then, rank by
// rank: lane l holds super-group l of that rank's table in registers, and the candidates that rank
// reaches are tested one after the other against all 64 super-groups at once (and against the 16
// groups of up to four hit super-groups at a time).  Finally every candidate lane publishes its own
// result and marks its children.
// GUESTS: somebody holds a particle inside this shard's pieces of the curve (K.guest, sorted).  A cell with
// such a key inside its range has partial moments here although it is wholly owned: it is descended like a
// shared one.  The other ranks need not know: to them the cell is not wholly theirs, so shared already.
// Without guests the kernel is the <false> one, the code it always was.
#define LET_EPW 16
template <bool GUESTS>
__global__ void __launch_bounds__(64)
k_let_level(int nelem, int level, const int4 *__restrict__ lk, const double4 *__restrict__ xm,
            const double4 *__restrict__ cl, const double *__restrict__ aux,
            const unsigned long long *__restrict__ skey, const DDGroup *__restrict__ groups, LetK K,
            unsigned long long *__restrict__ reach, unsigned long long *__restrict__ sendm)
{
  const int lane = threadIdx.x;
  const int e = blockIdx.x * LET_EPW + lane;
  bool cand = false;
  int4 me = make_int4(0, 0, 0, 0);
  unsigned long long r = 0;
  if(lane < LET_EPW && e < nelem)
    {
      me = lk[e];
      if(me.y == -(level + 1))
        {
          r = reach[e];
          cand = r != 0;
        }
    }
  if(__ballot(cand) == 0)
    return;
  // does the cell lie wholly inside this shard's key range?  (every octree cell is one contiguous
  // piece of the Peano-Hilbert curve)  If not, other shards hold particles of it too: its local
  // moments are partial and it must be descended for everybody.
  bool shared = true;
  double4 m4 = make_double4(0, 0, 0, 0), c4 = make_double4(0, 0, 0, 0);
  double a = 0;
  if(cand)
    {
      if(level > 0)
        {
          const int sh = 3 * (GHIP_BITS - level);
          const unsigned long long ph = d_peano_of_morton(skey[me.z]);
          const unsigned long long lo = (ph >> sh) << sh;
          const unsigned long long hi = lo + (1ULL << sh);
          shared = !d_owned_range(lo, hi, K.nown, K.ownlo, K.ownhi);
          if(GUESTS && !shared)
            {
              int a0 = 0, a1 = K.nguest;   // first guest key >= lo
              while(a0 < a1)
                {
                  const int mid = (a0 + a1) >> 1;
                  if(K.guest[mid] < lo)
                    a0 = mid + 1;
                  else
                    a1 = mid;
                }
              shared = a0 < K.nguest && K.guest[a0] < hi;
            }
        }
      m4 = xm[e];
      c4 = cl[e];
      a = aux[e];
    }
  unsigned long long X = (cand && shared) ? r : 0ULL;
  const bool test = cand && !shared;
  for(int b = 0; b < K.nranks; b++)
    {
      unsigned long long cm = __ballot(test && ((r >> b) & 1ULL));
      if(cm == 0)
        continue;
      const DDGroup *tab = groups + (size_t) b * DD_STRIDE;
      const DDGroup Gs = tab[lane];
      while(cm)
        {
          const int j = __builtin_ctzll(cm);
          cm &= cm - 1;
          const double4 mj = make_double4(d_bcast(m4.x, j), d_bcast(m4.y, j), d_bcast(m4.z, j),
                                          d_bcast(m4.w, j));
          const double4 cj = make_double4(d_bcast(c4.x, j), d_bcast(c4.y, j), d_bcast(c4.z, j),
                                          d_bcast(c4.w, j));
          const double aj = d_bcast(a, j);
          unsigned long long sm = __ballot(d_group_can_open(Gs, mj, cj, aj, K));
          bool open = false;
          while(sm && !open)
            {
              int sg = -1;
              for(int q = 0; q < 4 && sm; q++)
                {
                  const int s0 = __builtin_ctzll(sm);
                  sm &= sm - 1;
                  if((lane >> 4) == q)
                    sg = s0;
                }
              const bool hit = sg >= 0 && d_group_can_open(tab[DD_NSUPER + sg * DD_NSUB + (lane & 15)],
                                                           mj, cj, aj, K);
              open = __ballot(hit) != 0;
            }
          if(open && lane == j)
            X |= 1ULL << b;
        }
    }
  if(cand)
    {
      sendm[e] = r & ~X;
      if(X)
        for(int c = e + 1; c < me.x;)
          {
            const int4 ck = lk[c];
            reach[c] = X;
            if(ck.y >= 0)
              sendm[c] = X;   // a particle that is reached is sent
            c = ck.x;
          }
    }
}

__global__ void k_let_single(int nelem, const int4 *__restrict__ lk,
                             const unsigned long long *__restrict__ reach,
                             unsigned long long *__restrict__ sendm)
{
  // a shard with one particle has no root cell: element 0 is that particle
  if(blockIdx.x == 0 && threadIdx.x == 0 && nelem > 0 && lk[0].y >= 0)
    sendm[0] = reach[0];
}

// ---------------------------------------------------------------------------------------------
// order-preserving selection of the items whose mask has bit b set, for every rank b at once:
// count per block of SELM_BLOCK items and rank, offsets per rank (ghip_block_offsets), scatter the item indices
// ---------------------------------------------------------------------------------------------
#define SELM_ITEMS 16
#define SELM_BLOCK (64 * SELM_ITEMS)

__global__ void __launch_bounds__(64)
k_selm_count(int n, int nranks, const unsigned long long *__restrict__ mask, int nblk,
             int *__restrict__ blockcnt)
{
  __shared__ int cnt[GHIP_MAXRANKS];
  const int lane = threadIdx.x;
  cnt[lane] = 0;
  __syncthreads();
  const int base = blockIdx.x * SELM_BLOCK;
  for(int j = 0; j < SELM_ITEMS; j++)
    {
      const int a = base + j * 64 + lane;
      const unsigned long long m = a < n ? mask[a] : 0ULL;
      unsigned long long any = d_wave_or_u64(m);
      while(any)
        {
          const int b = __builtin_ctzll(any);
          any &= any - 1;
          const unsigned long long bal = __ballot((m >> b) & 1ULL);
          if(lane == 0)
            cnt[b] += __popcll(bal);
        }
    }
  __syncthreads();
  if(lane < nranks)
    blockcnt[(size_t) lane * nblk + blockIdx.x] = cnt[lane];
}

struct SelOff
{
  int off[GHIP_MAXRANKS];   // first slot of each rank's list in the output
};

__global__ void __launch_bounds__(64)
k_selm_scatter(int n, int nranks, const unsigned long long *__restrict__ mask, int nblk,
               const int *__restrict__ blockoff, SelOff S, int *__restrict__ out)
{
  __shared__ int pos[GHIP_MAXRANKS];
  const int lane = threadIdx.x;
  pos[lane] = lane < nranks ? S.off[lane] + blockoff[(size_t) lane * nblk + blockIdx.x] : 0;
  __syncthreads();
  const int base = blockIdx.x * SELM_BLOCK;
  const unsigned long long below = (1ULL << lane) - 1ULL;
  for(int j = 0; j < SELM_ITEMS; j++)
    {
      const int a = base + j * 64 + lane;
      const unsigned long long m = a < n ? mask[a] : 0ULL;
      unsigned long long any = d_wave_or_u64(m);
      while(any)
        {
          const int b = __builtin_ctzll(any);
          any &= any - 1;
          const unsigned long long bal = __ballot((m >> b) & 1ULL);
          const int p0 = pos[b];
          if((m >> b) & 1ULL)
            out[p0 + __popcll(bal & below)] = a;
          __syncthreads();
          if(lane == 0)
            pos[b] = p0 + __popcll(bal);
          __syncthreads();
        }
    }
}

// lists[dest-major] of the items selected for each rank; counts/offsets (host) in scount/soff
static int multi_select(ghip_ctx *ctx, int n, const unsigned long long *mask, DevBuf &list,
                        int *scount, int *soff, int *total_out)
{
  DDState &D = ctx->dd;
  hipStream_t st = ctx->stream;
  const int P_ = D.nranks;
  const int nblk = cdiv(n > 0 ? n : 1, SELM_BLOCK);
  GCHK(ghip_ensure(ctx, D.selcnt, ((size_t) P_ * nblk + GHIP_MAXRANKS) * 4));
  int *bc = P<int>(D.selcnt), *tot = bc + (size_t) P_ * nblk;
  k_selm_count<<<nblk, 64, 0, st>>>(n, P_, mask, nblk, bc);
  GCHK(ghip_block_offsets(ctx, P_, nblk, bc, tot, st));
  int htot[GHIP_MAXRANKS];
  HIPCHK(hipMemcpyAsync(htot, tot, (size_t) P_ * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  SelOff S;
  int run = 0;
  for(int b = 0; b < GHIP_MAXRANKS; b++)
    {
      S.off[b] = run;
      if(b < P_)
        {
          scount[b] = htot[b];
          soff[b] = run;
          run += htot[b];
        }
    }
  *total_out = run;
  GCHK(ghip_ensure(ctx, list, (size_t) (run > 0 ? run : 1) * 4));
  if(run > 0)
    {
      k_selm_scatter<<<nblk, 64, 0, st>>>(n, P_, mask, nblk, bc, S, P<int>(list));
      HIPCHK(hipGetLastError());
    }
  return GHIP_OK;
}

// element list -> LetRec records
__global__ void k_let_pack(int nrec, const int *__restrict__ list, const int4 *__restrict__ lk,
                           const double4 *__restrict__ xm, const double *__restrict__ aux,
                           const unsigned long long *__restrict__ skey, LetRec *__restrict__ out)
{
  int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nrec)
    return;
  const int e = list[a];
  const int4 k = lk[e];
  const double4 v = xm[e];
  LetRec r;
  r.x = v.x;
  r.y = v.y;
  r.z = v.z;
  r.m = v.w;
  r.aux = aux[e];
  r.pad = 0;
  r.spare = 0;
  if(k.y >= 0)
    {
      r.key = skey[k.y];
      r.level = 0;
    }
  else
    {
      const int L = -k.y - 1;
      const int sh = 63 - 3 * L;
      r.key = (skey[k.z] >> sh) << sh;
      r.level = L;
    }
  out[a] = r;
}

// ---------------------------------------------------------------------------------------------
// which ranks does an item (a gas particle as a ghost, a dust grain) concern?
// ---------------------------------------------------------------------------------------------
// Reach: the distance within which an item of radius h -- or a chunk of items, the largest of radius h --
// concerns a group
struct GhostReach   // a gas particle: it can be a neighbour of a target of the group (r < the group's padded
{                   // search radius), or a target can lie inside ITS smoothing sphere (hydra.c:1266)
  __device__ static double radius(const DDGroup &G, double h) { return G.rmax > h ? G.rmax : h; }
};
struct SphereReach  // a dust grain: every particle of the group lies in its box, and a neighbour of a grain is
{                   // closer than h (u = r / h < 1), so a group farther than h from the sphere's box holds none
  __device__ static double radius(const DDGroup &, double h) { return h; }
};

// does the box (c +- e; e = 0: one item) with radius h come within reach of the group?  (1e-9: rounding slack)
template <class Reach>
__device__ __forceinline__ bool d_group_reached(const DDGroup &G, double cx, double cy, double cz, double ex,
                                                double ey, double ez, double h, const BoxK &b)
{
  if(G.ex < 0)
    return false;
  const double r2 = d_group_box_dist2(G, cx, cy, cz, ex, ey, ez, b);
  const double R = Reach::radius(G, h) * (1.0 + 1.0e-9);
  return r2 < R * R;
}

// Src: where item t of the list comes from -- its mask slot i (the local particle index), position and radius
struct GhostSrc   // local gas particles as indices `src` of the gravity tree; h is padded by the ghost margin,
{                 // and the h a ghost was selected with is kept in h0 (by the chunk's first workgroup)
  const int *src, *perm;
  const double *sx, *sy, *sz, *hsml;
  double margin;
  double *h0;
  __device__ __forceinline__ void load(int t, bool first, int &i, double &x, double &y, double &z, double &h) const
  {
    const int s = src[t];
    i = perm[s];
    x = sx[s];
    y = sy[s];
    z = sz[s];
    const double hi = hsml[i];
    h = hi * margin;
    if(first)
      h0[i] = hi;
  }
};
struct DustSrc   // the grains of a dust pass: list slots `ord` in tree order, local indices `idx`
{
  const int *ord, *idx;
  int n;
  const double *pos, *hsml;
  __device__ __forceinline__ void load(int t, bool, int &i, double &x, double &y, double &z, double &h) const
  {
    i = idx[ord[t]];
    x = pos[i];
    y = pos[(size_t) n + i];
    z = pos[2 * (size_t) n + i];
    h = hsml[i];
  }
};

struct WindSrc   // the listed wind particles: list slots `list`, local indices `idx`, the planes dtj / drmin [nw].
{                // A particle with dt_jump <= 0 takes no part in a pass: radius 0 reaches nothing.  cut = 1: the
                 // sphere is cut to what can still change new_density (r < h_j <= hmax) or lower drmin
                 // (|r - h_j| + h_j / 4 >= r - 3/4 hmax), with the largest h_j of all shards' gas and the drmin of the
                 // own pass, once that found a candidate; cut = 2 (the spread alone): r < hmax
  const int *list, *idx;
  int n, cut;
  const double *pos, *hsml, *dtj, *drmin;
  double hmax;
  __device__ __forceinline__ void load(int t, bool, int &i, double &x, double &y, double &z, double &h) const
  {
    const int a = list[t];
    i = idx[a];
    x = pos[i];
    y = pos[(size_t) n + i];
    z = pos[2 * (size_t) n + i];
    h = hsml[i];
    if(!(dtj[a] > 0.))
      h = 0;
    else if(cut == 2)
      h = h < hmax ? h : hmax;
    else if(cut == 1 && drmin[a] < 1.e40)
      {
        const double far = (drmin[a] + 0.75 * hmax) * (1. + 1.e-9);
        const double c = far > hmax ? far : hmax;
        h = h < c ? h : c;
      }
  }
};

// bounding box of the valid lanes' positions around lane 0's (nearest-image offsets: a chunk is compact,
// the box may straddle the periodic boundary) and their largest radius (h = 0 in the other lanes)
struct ChunkBox
{
  double cx, cy, cz, ex, ey, ez, hmax;
};
__device__ __forceinline__ ChunkBox d_chunk_box(bool valid, double px, double py, double pz, double h,
                                                const BoxK &b)
{
  const double rx = __shfl(px, 0, 64), ry = __shfl(py, 0, 64), rz = __shfl(pz, 0, 64);
  double ox = valid ? px - rx : 0, oy = valid ? py - ry : 0, oz = valid ? pz - rz : 0;
  if(b.periodic)
    {
      ox = d_nearest(ox, b.boxsize, b.boxhalf);
      oy = d_nearest(oy, b.boxsize, b.boxhalf);
      oz = d_nearest(oz, b.boxsize, b.boxhalf);
    }
  double lo[3] = {ox, oy, oz}, hi[4] = {ox, oy, oz, h};
  d_wave_minmax<true>(lo, hi);
  ChunkBox C;
  C.hmax = hi[3];
  C.cx = rx + 0.5 * (lo[0] + hi[0]);
  C.cy = ry + 0.5 * (lo[1] + hi[1]);
  C.cz = rz + 0.5 * (lo[2] + hi[2]);
  C.ex = d_half_extent(lo[0], hi[0], 1e-14);
  C.ey = d_half_extent(lo[1], hi[1], 1e-14);
  C.ez = d_half_extent(lo[2], hi[2], 1e-14);
  return C;
}

// One wavefront per (chunk of 64 items that are neighbours in the gravity tree's (Morton) order,
// destination rank).  The chunk's bounding box is tested against the 64 super-groups of the rank by the
// 64 lanes at once; only for the super-groups it comes near are the 16 groups staged through LDS and
// every lane tests its own item against the near ones.  Interior chunks -- nearly all of them -- cost
// one box test.  mask[] (by local particle index) must be zero on entry for the items; the ranks' bits
// are OR-ed in.
template <class Src, class Reach>
__global__ void __launch_bounds__(64)
k_dd_select(int nitem, Src S, const DDGroup *__restrict__ groups, BoxK bx, int nranks, int me,
            unsigned long long *__restrict__ mask)
{
  __shared__ DDGroup sh[DD_NSUB];
  const int lane = threadIdx.x;
  const int nd = nranks - 1;                     // destinations per chunk
  const int chunk = blockIdx.x / nd;
  int b = blockIdx.x - chunk * nd;
  if(b >= me)
    b++;                                         // skip this rank itself
  const int t = chunk * 64 + lane;
  const bool valid = t < nitem;
  int i = 0;
  double px = 0, py = 0, pz = 0, h = 0;
  if(valid)
    S.load(t, blockIdx.x == chunk * nd, i, px, py, pz, h);
  const ChunkBox C = d_chunk_box(valid, px, py, pz, h, bx);
  const DDGroup *tab = groups + (size_t) b * DD_STRIDE;
  unsigned long long sm = __ballot(d_group_reached<Reach>(tab[lane], C.cx, C.cy, C.cz, C.ex, C.ey, C.ez, C.hmax, bx));
  bool need = false;
  while(sm)
    {
      const int sg = __builtin_ctzll(sm);
      sm &= sm - 1;
      __syncthreads();
      bool near = false;
      if(lane < DD_NSUB)
        {
          const DDGroup G = tab[DD_NSUPER + sg * DD_NSUB + lane];
          sh[lane] = G;
          near = d_group_reached<Reach>(G, C.cx, C.cy, C.cz, C.ex, C.ey, C.ez, C.hmax, bx);
        }
      unsigned long long qm = __ballot(near);
      __syncthreads();
      while(qm)
        {
          const int q = __builtin_ctzll(qm);
          qm &= qm - 1;
          if(valid && !need && d_group_reached<Reach>(sh[q], px, py, pz, 0, 0, 0, h, bx))
            need = true;
        }
      if(__ballot(valid && !need) == 0)
        break;   // every item of the chunk goes there already
    }
  if(need)
    atomicOr(mask + i, 1ULL << b);
}

// ---------------------------------------------------------------------------------------------
// SPH: the ghost records
// ---------------------------------------------------------------------------------------------
// GhostRec of local gas particle i (host order): the two records of the SPH kernels
// (ghip_tree.hip k_gather_gas)
__global__ void k_ghost_pack(int nrec, const int *__restrict__ list, int n, int ngas,
                             const double *__restrict__ pos, const double *__restrict__ mass,
                             const double *__restrict__ velpred, const double *__restrict__ h,
                             const double *__restrict__ pres, const double *__restrict__ rho,
                             const double *__restrict__ dhf, const double *__restrict__ divv,
                             const double *__restrict__ curl, const int *__restrict__ timebin,
                             const int *__restrict__ type, const double *__restrict__ alpha,
                             GhostRec *__restrict__ out)
{
  int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nrec)
    return;
  const int i = list[a];
  GhostRec r;
  r.p[0] = pos[i];
  r.p[1] = pos[(size_t) n + i];
  r.p[2] = pos[2 * (size_t) n + i];
  // (a converted particle of the gas block: nobody's neighbour on any shard, in density() and in hydro_force();
  // a swallowed one travels with its mass 0 and is marked where it arrives, by that shard's rule)
  r.p[3] = type[i] == 0 ? mass[i] : GAS_MARK_CONVERTED;
  r.p[4] = velpred[i];
  r.p[5] = velpred[(size_t) ngas + i];
  r.p[6] = velpred[2 * (size_t) ngas + i];
  r.p[7] = h[i];
  const int tb = timebin[i];
  r.q[0] = pres[i];
  r.q[1] = rho[i];
  r.q[2] = dhf[i];
  r.q[3] = divv[i];
  r.q[4] = curl[i];
  r.q[5] = (double) (tb ? (1 << tb) : 0);   // hydra.c:966
  r.q[6] = alpha ? alpha[i] : 0;   // (ghip_visc_set_alpha: the owner's alpha, in the slot that was spare)
  r.q[7] = 0;
  out[a] = r;
}

static int pack_ghosts(ghip_ctx *ctx, int total)
{
  DDState &D = ctx->dd;
  D.gh_alpha_epoch = ctx->visc_epoch;   // (the alpha these records carry: GHIP_DD_HYDRO asks for the same)
  const int n = ctx->n, ng = ctx->ngas;
  GCHK(ghip_ensure(ctx, D.gh_send, (size_t) (total > 0 ? total : 1) * sizeof(GhostRec)));
  if(total == 0)
    return GHIP_OK;
  k_ghost_pack<<<cdiv(total, 256), 256, 0, ctx->stream>>>(
    total, P<int>(D.gh_list), n, ng, P<double>(ctx->f[GHIP_F_POS]), P<double>(ctx->f[GHIP_F_MASS]),
    P<double>(ctx->f[GHIP_F_VELPRED]), P<double>(ctx->f[GHIP_F_HSML]),
    P<double>(ctx->f[GHIP_F_PRESSURE]), P<double>(ctx->f[GHIP_F_DENSITY]),
    P<double>(ctx->f[GHIP_F_DHSMLFAC]), P<double>(ctx->f[GHIP_F_DIVVEL]),
    P<double>(ctx->f[GHIP_F_CURLVEL]), P<int>(ctx->f[GHIP_F_TIMEBIN]), P<int>(ctx->f[GHIP_F_TYPE]),
    (ctx->visc_alpha.p && ctx->visc_ngas == ng) ? P<double>(ctx->visc_alpha) : nullptr, P<GhostRec>(D.gh_send));
  HIPCHK(hipGetLastError());
  return GHIP_OK;
}

// largest smoothing length any density evaluation of this call used, relative to the one the
// ghosts were selected with: max(right bracket, final h) / h0 over the local gas (host order)
__global__ void k_ghost_growth(int nt, const int *__restrict__ tgt, const int *__restrict__ perm,
                               const double *__restrict__ hcur, const double *__restrict__ right,
                               const double *__restrict__ h0, unsigned long long *__restrict__ out)
{
  int ti = blockIdx.x * blockDim.x + threadIdx.x;
  double r = 0;
  if(ti < nt)
    {
      const int s = tgt[ti];
      const double hm = right[s] > hcur[s] ? right[s] : hcur[s];
      r = hm / h0[perm[s]];
    }
  r = d_wave_max_f64(r);
  if((threadIdx.x & 63) == 0 && r > 0)
    atomicMax(out, (unsigned long long) __double_as_longlong(r));   // positive doubles order like integers
}

// ---------------------------------------------------------------------------------------------
// the dust passes, the wind particles and the friends-of-friends groups: which shards can a sphere reach?
// (ghip_dust.hip, ghip_wind.hip and ghip_fof.hip run the operations)
// ---------------------------------------------------------------------------------------------
// the partners of a pass among this shard's particles: the local Type 0 and Type 2 particles (the candidates of
// both dust passes) / the local Type-0 particles with Mass > 0 (those of both wind passes, virtual_density.c:650-664)
struct DustPartner
{
  const int *type;
  __device__ __forceinline__ bool operator()(int i) const { return type[i] == 0 || type[i] == 2; }
};
struct WindPartner
{
  const int *type;
  const double *mass;
  __device__ __forceinline__ bool operator()(int i) const { return type[i] == 0 && mass[i] > 0; }
};

// ... flagged in curve order, by their indices of the merged gravity tree
template <class Partner>
__global__ void k_flag_partners(int nt, const int *__restrict__ perm, int n, Partner partner, int *__restrict__ flags)
{
  int s = blockIdx.x * blockDim.x + threadIdx.x;
  if(s >= nt)
    return;
  const int i = perm[s];
  flags[s] = (i < n && partner(i)) ? 1 : 0;
}

// this shard's group table over its partners (val: what the groups carry in place of the least OldAcc, which the
// sphere test does not read); the all-gather is left pending
template <class Partner>
static int dd_partner_groups(ghip_ctx *ctx, const Partner &partner, const double *val)
{
  DDState &D = ctx->dd;
  hipStream_t st = ctx->stream;
  const int nt = ctx->gt.n;   // local particles + imported elements of the merged tree
  int nsel = 0;
  GCHK(ghip_ensure(ctx, D.gas_tgt, (size_t) (nt > 0 ? nt : 1) * 4));
  if(nt > 0 && ctx->n > 0)
    {
      GCHK(ghip_ensure(ctx, ctx->dflags, (size_t) nt * 4));
      k_flag_partners<<<cdiv(nt, 256), 256, 0, st>>>(nt, P<int>(ctx->gt.perm), ctx->n, partner, P<int>(ctx->dflags));
      HIPCHK(hipGetLastError());
      int *dnum = &ghip_words(ctx)->dust_partners;
      GCHK(ghip_select_flagged(ctx, nullptr, P<int>(ctx->dflags), P<int>(D.gas_tgt), dnum, nt, st));
      HIPCHK(hipMemcpyAsync(&nsel, dnum, 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
    }
  GCHK(build_groups(ctx, false, P<int>(D.gas_tgt), nsel, val));
  ghip_dd_set_allgather(D, D.grp_own.p, (size_t) DD_STRIDE * sizeof(DDGroup), &D.grp_all);
  return 1;
}

int ghip_dd_dust_groups(ghip_ctx *ctx)
{
  return dd_partner_groups(ctx, DustPartner{P<int>(ctx->f[GHIP_F_TYPE])}, nullptr);
}

// After the all-gather of the group tables: the destinations of the nitem items of S (a Src of k_dd_select) whose
// spheres reach another shard's groups, as per-destination lists of their mask slots in ascending order (list,
// scount / soff) and their total.  mask: u64 [nmask], cleared here
template <class Src>
static int dd_sphere_select(ghip_ctx *ctx, int nitem, const Src &S, double boxsize, int periodic, int nmask,
                            DevBuf &mask, DevBuf &list, int *scount, int *soff, int *total)
{
  DDState &D = ctx->dd;
  hipStream_t st = ctx->stream;
  const int P_ = D.nranks;
  for(int r = 0; r < GHIP_MAXRANKS; r++)
    scount[r] = soff[r] = 0;
  *total = 0;
  GCHK(ghip_ensure(ctx, list, 4));
  if(nitem == 0 || P_ < 2 || nmask == 0)
    return GHIP_OK;
  GCHK(ghip_ensure(ctx, mask, (size_t) nmask * 8));
  HIPCHK(hipMemsetAsync(mask.p, 0, (size_t) nmask * 8, st));
  k_dd_select<Src, SphereReach><<<cdiv(nitem, 64) * (P_ - 1), 64, 0, st>>>(
    nitem, S, P<DDGroup>(D.grp_all), make_box(boxsize, periodic), P_, D.rank, P<unsigned long long>(mask));
  HIPCHK(hipGetLastError());
  return multi_select(ctx, nmask, P<unsigned long long>(mask), list, scount, soff, total);
}

// the destinations of this shard's nd grains (ord: list slots in tree order, idx: local indices, both on the
// device): D.du_list holds their local indices, D.du_scount / du_soff the layout
int ghip_dd_dust_select(ghip_ctx *ctx, const char *what, int nd, const int *ord, const int *idx, double boxsize,
                        int periodic, int *total)
{
  DDState &D = ctx->dd;
  GCHK(check_group_status(ctx, what));
  const DustSrc S = {ord, idx, ctx->n, P<double>(ctx->f[GHIP_F_POS]), P<double>(ctx->f[GHIP_F_HSML])};
  return dd_sphere_select(ctx, nd, S, boxsize, periodic, ctx->n, D.du_mask, D.du_list, D.du_scount, D.du_soff, total);
}

// The wind's group table, and in the status record behind it three words of the wind operation (the largest h_j as
// a double, the dt_jump sum, the list length) and whether this shard has failed already (own_rc != GHIP_OK, its
// message in ctx->err); the all-gather is left pending
int ghip_dd_wind_groups(ghip_ctx *ctx, const double extra[3], int own_rc)
{
  DDState &D = ctx->dd;
  const std::string own_msg = ctx->err;
  const double *mass = P<double>(ctx->f[GHIP_F_MASS]);
  const int rc = dd_partner_groups(ctx, WindPartner{P<int>(ctx->f[GHIP_F_TYPE]), mass}, mass);
  if(rc != 1)
    return rc;
  // (the all-gather is pending, not begun: the status record still gets into grp_own)
  if(own_rc != GHIP_OK)   // (build_groups held its own check, which passed)
    {
      D.held.rc = own_rc;
      D.held.msg = own_msg;
    }
  DDGroup status;
  memset(&status, 0, sizeof(status));
  status.cx = D.held.rc != GHIP_OK ? 1.0 : 0.0;
  status.cy = D.guests_on ? (double) D.guests_held : 0.0;
  status.cz = extra[0];
  status.ex = extra[1];
  status.ey = extra[2];
  // (the resident form: the code too, so that the other shards return what the failing one does)
  status.ez = D.held.rc != GHIP_OK && D.wind.resident ? (double) D.held.rc : 0.0;
  HIPCHK(hipMemcpyAsync(P<DDGroup>(D.grp_own) + DD_TABLE, &status, sizeof(status), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));   // (`status` lives on this frame)
  return 1;
}

// the code the first failed shard published with its status record (the resident form does), GHIP_OK: none
static int wind_failed_code(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  DDGroup rec[GHIP_MAXRANKS];
  HIPCHK(hipMemcpy2DAsync(rec, sizeof(DDGroup), P<DDGroup>(D.grp_all) + DD_TABLE, (size_t) DD_STRIDE * sizeof(DDGroup),
                          sizeof(DDGroup), (size_t) D.nranks, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  for(int r = 0; r < D.nranks; r++)
    if(rec[r].cx != 0)
      return (int) rec[r].ez;
  return GHIP_OK;
}

// after that all-gather: every shard stops here if one has failed; else extra[r][3] of every shard, in rank order
int ghip_dd_wind_status(ghip_ctx *ctx, const char *what, double *extra)
{
  DDState &D = ctx->dd;
  const int rc = check_group_status(ctx, what);
  if(rc != GHIP_OK && D.held.rc == GHIP_OK)   // another shard failed: its code if it said it, under the same message
    {
      const std::string msg = ctx->err;
      const int code = wind_failed_code(ctx);
      return code < 0 ? ghip_fail(ctx, code, "%s", msg.c_str()) : rc;
    }
  GCHK(rc);
  DDGroup rec[GHIP_MAXRANKS];
  HIPCHK(hipMemcpy2DAsync(rec, sizeof(DDGroup), P<DDGroup>(D.grp_all) + DD_TABLE, (size_t) DD_STRIDE * sizeof(DDGroup),
                          sizeof(DDGroup), (size_t) D.nranks, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  for(int r = 0; r < D.nranks; r++)
    {
      extra[3 * r] = rec[r].cz;
      extra[3 * r + 1] = rec[r].ex;
      extra[3 * r + 2] = rec[r].ey;
    }
  return GHIP_OK;
}

// the destinations of the m listed wind particles (list: slots in tree order; idx: local indices; dtj, drmin: planes
// in slot order), where the dust passes leave theirs.  cut, hmax: see WindSrc
int ghip_dd_wind_select(ghip_ctx *ctx, int m, const int *list, const int *idx, const double *dtj, const double *drmin,
                        int cut, double hmax, double boxsize, int periodic, int *total)
{
  DDState &D = ctx->dd;
  const WindSrc S = {list, idx, ctx->n, cut, P<double>(ctx->f[GHIP_F_POS]), P<double>(ctx->f[GHIP_F_HSML]), dtj, drmin, hmax};
  return dd_sphere_select(ctx, m, S, boxsize, periodic, ctx->n, D.du_mask, D.du_list, D.du_scount, D.du_soff, total);
}

// ---------------------------------------------------------------------------------------------
// friends-of-friends groups on shards: whose primary boxes does a sphere reach? (ghip_fof.hip runs the operation)
// ---------------------------------------------------------------------------------------------
struct FofSrc   // items `list` as indices of the merged gravity tree, which are their mask slots too; radius
{               // hs[s] (a settled secondary carries a negative one: radius 0 reaches nothing) or, hs == nullptr, h0
  const int *list;
  const double *sx, *sy, *sz, *hs;
  double h0;
  __device__ __forceinline__ void load(int t, bool, int &i, double &x, double &y, double &z, double &h) const
  {
    const int s = list[t];
    i = s;
    x = sx[s];
    y = sy[s];
    z = sz[s];
    const double hh = hs ? hs[s] : h0;
    h = hh > 0 ? hh : 0;
  }
};

// this shard's group table over its own primaries (tree indices, ascending); the all-gather is left pending
int ghip_dd_fof_groups(ghip_ctx *ctx, const int *plist, int nprim)
{
  DDState &D = ctx->dd;
  // (the groups carry the least mass in place of OldAcc: the sphere test reads neither)
  GCHK(build_groups(ctx, false, plist, nprim, P<double>(ctx->f[GHIP_F_MASS])));
  ghip_dd_set_allgather(D, D.grp_own.p, (size_t) DD_STRIDE * sizeof(DDGroup), &D.grp_all);
  return 1;
}

int ghip_dd_fof_status(ghip_ctx *ctx, const char *what) { return check_group_status(ctx, what); }

// the per-destination lists (ascending tree index) of the nitem items whose spheres reach another shard's primaries;
// mask: u64[ctx->gt.n]
int ghip_dd_fof_select(ghip_ctx *ctx, int nitem, const int *items, const double *hs, double h0, double boxsize,
                       int periodic, DevBuf &mask, DevBuf &list, int *scount, int *soff, int *total)
{
  const FofSrc S = {items, P<double>(ctx->sx), P<double>(ctx->sy), P<double>(ctx->sz), hs, h0};
  return dd_sphere_select(ctx, nitem, S, boxsize, periodic, ctx->gt.n, mask, list, scount, soff, total);
}

// multi_select for the callers outside this file: the items of mask[0 .. n) per rank whose bit is set
int ghip_dd_select_ranks(ghip_ctx *ctx, int n, const unsigned long long *mask, DevBuf &list, int *scount, int *soff,
                         int *total)
{
  return multi_select(ctx, n, mask, list, scount, soff, total);
}

// ---------------------------------------------------------------------------------------------
// the state machine: compute until the next exchange, exchange, continue
// ---------------------------------------------------------------------------------------------
#define set_allgather ghip_dd_set_allgather
#define set_alltoallv ghip_dd_set_alltoallv

// ---- gravity ------------------------------------------------------------------------------
// The guest pass (ghip_dd_set_guests) in place of the range check: which resident particles lie outside this
// shard's pieces of the curve, and their keys listed per host, in the order the shard holds them.
static int find_guests(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  hipStream_t st = ctx->stream;
  const int n = ctx->n;
  for(int r = 0; r < GHIP_MAXRANKS; r++)
    D.guest_scount[r] = D.guest_soff[r] = 0;
  GCHK(ghip_ensure(ctx, D.guest_send, 8));
  if(n == 0)
    return GHIP_OK;
  GCHK(ghip_ensure(ctx, D.guest_mask, (size_t) n * 8));
  GCHK(ghip_ensure(ctx, D.guest_key, (size_t) n * 8));
  const double *x = P<double>(ctx->f[GHIP_F_POS]);
  const double fac = 1.0 / ctx->dlen * (double) (1ULL << GHIP_BITS);
  k_dd_mark_guests<<<cdiv(n, 256), 256, 0, st>>>(
    n, x, x + n, x + 2 * (size_t) n, ctx->corner[0], ctx->corner[1], ctx->corner[2], fac, D.nown,
    P<unsigned long long>(D.ownlo), P<unsigned long long>(D.ownhi), D.nseg, P<unsigned long long>(D.segkey),
    P<int>(D.segowner), P<unsigned long long>(D.guest_key), P<unsigned long long>(D.guest_mask),
    ghip_errword(ctx, GHIP_ERRW_TREE));
  HIPCHK(hipGetLastError());
  int total = 0;
  GCHK(multi_select(ctx, n, P<unsigned long long>(D.guest_mask), D.guest_list, D.guest_scount, D.guest_soff,
                    &total));
  D.guests_held = total;
  if(total > 0)
    {
      GCHK(ghip_ensure(ctx, D.guest_send, (size_t) total * 8));
      k_dd_gather_u64<<<cdiv(total, 256), 256, 0, st>>>(total, P<int>(D.guest_list),
                                                       P<unsigned long long>(D.guest_key),
                                                       P<unsigned long long>(D.guest_send));
      HIPCHK(hipGetLastError());
    }
  return GHIP_OK;
}

// the shard's own tree (moments of the cells it owns), nothing imported
int ghip_dd_own_tree(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  hipStream_t st = ctx->stream;
  GCHK(ghip_join_pair(ctx));
  D.gt_nimp = 0;
  D.gt_is_pot = false;
  D.guests_held = D.guests_hosted = 0;
  D.guest_xchg = false;
  if(D.guests_on)
    GCHK(find_guests(ctx));
  else if(ctx->n > 0)
    {
      const double *x = P<double>(ctx->f[GHIP_F_POS]);
      const double fac = 1.0 / ctx->dlen * (double) (1ULL << GHIP_BITS);
      k_dd_check_range<<<cdiv(ctx->n, 256), 256, 0, st>>>(
        ctx->n, x, x + ctx->n, x + 2 * (size_t) ctx->n, ctx->corner[0], ctx->corner[1],
        ctx->corner[2], fac, D.nown, P<unsigned long long>(D.ownlo), P<unsigned long long>(D.ownhi),
        ghip_errword(ctx, GHIP_ERRW_TREE));
    }
  return ghip_tree_build_impl(ctx);
}

__global__ void k_dd_iota(int n, int *__restrict__ out)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i < n)
    out[i] = i;
}

// the group table of the own tree's targets -- the active gravity targets, or (all) every particle of the
// shard, as compute_potential() has them (potential.c:88-97) -- and its all-gather
int ghip_dd_post_groups(ghip_ctx *ctx, bool all, bool need_oldacc)
{
  DDState &D = ctx->dd;
  if(all)
    {
      const int n = ctx->gt.n;   // (= ctx->n: nothing is imported yet)
      GCHK(ghip_ensure(ctx, D.pot_tgt, (size_t) (n > 0 ? n : 1) * 4));
      if(n > 0)
        {
          k_dd_iota<<<cdiv(n, 256), 256, 0, ctx->stream>>>(n, P<int>(D.pot_tgt));
          HIPCHK(hipGetLastError());
        }
      // (under the Barnes-Hut criterion no test reads amin and OldAcc need not be set: any array serves)
      GCHK(build_groups(ctx, false, P<int>(D.pot_tgt), n,
                        need_oldacc ? nullptr : P<double>(ctx->f[GHIP_F_MASS])));
    }
  else
    {
      GCHK(ghip_build_target_lists(ctx));
      GCHK(build_groups(ctx, false, P<int>(ctx->tg_grav), ctx->nt_grav));
    }
  set_allgather(D, D.grp_own.p, (size_t) DD_STRIDE * sizeof(DDGroup), &D.grp_all);
  return GHIP_OK;
}

// after the all-gather of the group tables: every shard fails if one did (all shards together, see DD_STRIDE);
// does any shard hold a guest?  Then every shard sends the keys of its guests to their hosts, and only there:
// 1, the all-to-all-v is pending.  Nobody holds one (always so with the mode off): 0, nothing is exchanged.
int ghip_dd_post_guests(ghip_ctx *ctx, const char *what)
{
  DDState &D = ctx->dd;
  long long held = 0;
  GCHK(check_group_status(ctx, what, &held));
  if(!D.guests_on || held == 0)
    return 0;
  D.guest_xchg = true;
  set_alltoallv(D, D.guest_send.p, 8, D.guest_scount, D.guest_soff, &D.guest_recv);
  return 1;
}

// the keys of the guests this shard hosts, as the exchange left them, in ascending order
static int sort_hosted_guests(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  const int ng = D.x.rtotal;
  D.guests_hosted = ng;
  if(ng == 0)
    return GHIP_OK;
  GCHK(ghip_ensure(ctx, D.guest_sorted, (size_t) ng * 8));
  const unsigned long long *in = P<unsigned long long>(D.guest_recv);
  unsigned long long *out = P<unsigned long long>(D.guest_sorted);
  return ghip_sort_keys(ctx, in, out, ng, 63, ctx->stream);
}

// after ghip_dd_post_guests (and the exchange it asked for): what can the others need of this tree?
int ghip_dd_post_let(ghip_ctx *ctx, const ghip_grav_params &gp)
{
  DDState &D = ctx->dd;
  hipStream_t st = ctx->stream;
  const int P_ = D.nranks;
  if(D.guest_xchg)
    GCHK(sort_hosted_guests(ctx));
  TreeDev &t = ctx->gt;
  int scount[GHIP_MAXRANKS], soff[GHIP_MAXRANKS], total = 0;
  for(int r = 0; r < GHIP_MAXRANKS; r++)
    scount[r] = soff[r] = 0;
  if(t.nelem > 0 && P_ > 1)
    {
      GCHK(ghip_ensure(ctx, D.reach, (size_t) t.nelem * 8));
      GCHK(ghip_ensure(ctx, D.sendm, (size_t) t.nelem * 8));
      LetK K;
      K.theta2 = gp.ErrTolTheta * gp.ErrTolTheta;
      K.errtol = gp.ErrTolForceAcc;
      K.b = make_box(gp.BoxSize, gp.periodic);
      K.unequal = gp.unequal_softenings || ctx->adaptive_gravsoft;
      K.nranks = P_;
      K.me = D.rank;
      K.nown = D.nown;
      K.ownlo = P<unsigned long long>(D.ownlo);
      K.ownhi = P<unsigned long long>(D.ownhi);
      K.nguest = D.guests_hosted;
      K.guest = P<unsigned long long>(D.guest_sorted);
      unsigned long long all = (P_ >= 64) ? ~0ULL : ((1ULL << P_) - 1ULL);
      all &= ~(1ULL << D.rank);
      unsigned long long *reach = P<unsigned long long>(D.reach),
                         *sendm = P<unsigned long long>(D.sendm);
      k_let_init<<<cdiv(t.nelem, 256), 256, 0, st>>>(t.nelem, all, reach, sendm);
      auto *level_kernel = K.nguest > 0 ? k_let_level<true> : k_let_level<false>;
      for(int L = 0; L <= t.maxlevel; L++)
        level_kernel<<<cdiv(t.nelem, LET_EPW), 64, 0, st>>>(
          t.nelem, L, P<int4>(t.lk), P<double4>(t.xm), P<double4>(t.cl), P<double>(t.aux),
          P<unsigned long long>(t.skey), P<DDGroup>(D.grp_all), K, reach, sendm);
      k_let_single<<<1, 64, 0, st>>>(t.nelem, P<int4>(t.lk), reach, sendm);
      HIPCHK(hipGetLastError());
      GCHK(multi_select(ctx, t.nelem, sendm, D.let_list, scount, soff, &total));
    }
  GCHK(ghip_ensure(ctx, D.let_send, (size_t) (total > 0 ? total : 1) * sizeof(LetRec)));
  if(total > 0)
    {
      k_let_pack<<<cdiv(total, 256), 256, 0, st>>>(total, P<int>(D.let_list), P<int4>(t.lk),
                                                  P<double4>(t.xm), P<double>(t.aux),
                                                  P<unsigned long long>(t.skey),
                                                  P<LetRec>(D.let_send));
      HIPCHK(hipGetLastError());
    }
  D.let_sent = total;
  set_alltoallv(D, D.let_send.p, sizeof(LetRec), scount, soff, &D.let_recv);
  return GHIP_OK;
}

// GHIP_DD_GRAVITY:
//   GROUPS  the shard's own tree and the groups of its active targets          -> all-gather of the groups
//   GUESTS  every shard fails if one did; with ghip_dd_set_guests, when any shard holds a guest: the guests' keys
//           to their hosts (else straight on to LET)                            -> all-to-all-v of u64 keys
//   LET     selection of the locally essential trees, packed                    -> all-to-all-v of LetRec
//   WALK    one tree over the local particles and everything that was imported, then the walks
static int gravity_begin(ghip_ctx *ctx, int, const void *params, int walk)
{
  DDState &D = ctx->dd;
  if(walk < 0 || walk > GHIP_WALK_NEWTON_EWALD)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_begin: unknown walk %d", walk);
  D.gp = *reinterpret_cast<const ghip_grav_params *>(params);
  D.walk = walk;
  return GHIP_OK;
}

static int gravity_step(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  enum { GROUPS, GUESTS, LET, WALK, DONE };
  if(D.phase == GROUPS)
    {
      GCHK(ghip_dd_own_tree(ctx));
      GCHK(ghip_dd_post_groups(ctx, false, true));
      D.phase = GUESTS;
      return 1;
    }
  if(D.phase == GUESTS)
    {
      const int pending = ghip_dd_post_guests(ctx, "gravity");
      D.phase = LET;
      if(pending != 0)
        return pending;
    }
  if(D.phase == LET)
    {
      GCHK(ghip_dd_post_let(ctx, D.gp));
      D.phase = WALK;
      return 1;
    }
  if(D.phase == WALK)
    {
      D.gt_nimp = D.x.rtotal;
      GCHK(ghip_tree_build_impl(ctx));
      D.phase = DONE;
      return ghip_gravity_impl(ctx, &D.gp, D.walk);
    }
  return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_step: gravity has no phase %d", D.phase);
}

// ---- density --------------------------------------------------------------------------------
// the local gas targets in curve order, as indices of the (merged) gravity tree
__global__ void k_flag_gas_targets(int nt, const int *__restrict__ tgt, const int *__restrict__ perm,
                                   int ngas, int *__restrict__ flags)
{
  int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a < nt)
    flags[a] = perm[tgt[a]] < ngas ? 1 : 0;
}

__global__ void k_mask_local_gas(int n, int ngas, const int *__restrict__ perm,
                                 unsigned long long *__restrict__ mask)
{
  int s = blockIdx.x * blockDim.x + threadIdx.x;
  if(s < n)
    mask[s] = perm[s] < ngas ? 1ULL : 0ULL;
}

// GHIP_DD_DENSITY:
//   GROUPS   groups of the gas targets with their padded search radii            -> all-gather of the groups
//   GHOSTS   every shard fails if one did; which local gas particles are ghosts where, packed
//                                                                                 -> all-to-all-v of GhostRec
//   ITERATE  gas tree over the local gas and the ghosts, the h iteration; what it met and the largest growth
//            of a search radius                                                   -> all-gather of the status
//   DECIDE   a radius outgrew the padding: back to GROUPS with a larger one; every shard fails if one did;
//            the ghosts' records as they are after density()                      -> all-to-all-v of GhostRec
//   REFRESH  the ghosts' records unpacked
static int density_begin(ghip_ctx *ctx, int, const void *params, int)
{
  DDState &D = ctx->dd;
  D.dp = *reinterpret_cast<const ghip_dens_params *>(params);
  D.gh_margin_cur = D.gh_margin;   // (grows within the call when a smoothing length outgrows it)
  D.gh_retries = 0;
  return GHIP_OK;
}

static int density_step(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  hipStream_t st = ctx->stream;
  const int P_ = D.nranks;
  const int ng = ctx->ngas;
  enum { GROUPS, GHOSTS, ITERATE, DECIDE, REFRESH, DONE };
  if(D.phase == GROUPS)
    {
      // groups of the gas targets (bounding box, padded search radius) from the curve order of the
      // gravity tree: positions in tree order, smoothing lengths through perm
      // (a density() that no gravity_tree() precedes -- init.c:791 -- orders the shard's own
      // particles itself: the tree of the local particles, nothing imported)
      if(!ctx->gt.built)
        {
          GCHK(ghip_join_pair(ctx));
          D.gt_nimp = 0;
          D.gt_is_pot = false;
          GCHK(ghip_tree_build_impl(ctx));
        }
      GCHK(ghip_build_target_lists(ctx));
      const int nt = ctx->nt_grav;
      int ngt = 0;
      GCHK(ghip_ensure(ctx, D.gas_tgt, (size_t) (nt > 0 ? nt : 1) * 4));
      if(nt > 0 && ng > 0)
        {
          GCHK(ghip_ensure(ctx, ctx->dflags, (size_t) nt * 4));
          k_flag_gas_targets<<<cdiv(nt, 256), 256, 0, st>>>(nt, P<int>(ctx->tg_grav), P<int>(ctx->gt.perm),
                                                           ng, P<int>(ctx->dflags));
          int *dnum = &ghip_words(ctx)->gas_targets;
          GCHK(ghip_select_flagged(ctx, P<int>(ctx->tg_grav), P<int>(ctx->dflags), P<int>(D.gas_tgt), dnum, nt, st));
          HIPCHK(hipMemcpyAsync(&ngt, dnum, 4, hipMemcpyDeviceToHost, st));
          HIPCHK(ghip_stream_sync(ctx, st));
        }
      GCHK(build_groups(ctx, true, P<int>(D.gas_tgt), ngt));
      set_allgather(D, D.grp_own.p, (size_t) DD_STRIDE * sizeof(DDGroup), &D.grp_all);
      D.phase = GHOSTS;
      return 1;
    }
  if(D.phase == GHOSTS)
    {
      GCHK(check_group_status(ctx, "density"));
      // which local gas particles are ghosts where
      int total = 0;
      for(int r = 0; r < GHIP_MAXRANKS; r++)
        D.gh_scount[r] = D.gh_soff[r] = 0;
      GCHK(ghip_ensure(ctx, D.h0, (size_t) (ng > 0 ? ng : 1) * 8));
      if(ng > 0 && P_ > 1)
        {
          GCHK(ghip_ensure(ctx, D.gh_mask, (size_t) ng * 8));
          // the local gas particles in the gravity tree's order (chunks of 64 are compact)
          const int nsrc = ctx->gt.n;
          GCHK(ghip_ensure(ctx, D.sendm, (size_t) nsrc * 8));
          k_mask_local_gas<<<cdiv(nsrc, 256), 256, 0, st>>>(nsrc, ng, P<int>(ctx->gt.perm),
                                                           P<unsigned long long>(D.sendm));
          int c0[GHIP_MAXRANKS], o0[GHIP_MAXRANKS], nfound = 0;
          GCHK(multi_select(ctx, nsrc, P<unsigned long long>(D.sendm), D.gas_src, c0, o0, &nfound));
          if(nfound != ng)
            return ghip_fail(ctx, GHIP_EINVAL, "ghost selection: %d of %d gas particles in the tree",
                             nfound, ng);
          HIPCHK(hipMemsetAsync(D.gh_mask.p, 0, (size_t) ng * 8, st));
          const GhostSrc S = {P<int>(D.gas_src), P<int>(ctx->gt.perm), P<double>(ctx->sx), P<double>(ctx->sy),
                              P<double>(ctx->sz), P<double>(ctx->f[GHIP_F_HSML]), D.gh_margin_cur, P<double>(D.h0)};
          k_dd_select<GhostSrc, GhostReach><<<cdiv(ng, 64) * (P_ - 1), 64, 0, st>>>(
            ng, S, P<DDGroup>(D.grp_all), make_box(D.dp.BoxSize, D.dp.periodic), P_, D.rank,
            P<unsigned long long>(D.gh_mask));
          HIPCHK(hipGetLastError());
          GCHK(multi_select(ctx, ng, P<unsigned long long>(D.gh_mask), D.gh_list, D.gh_scount,
                            D.gh_soff, &total));
        }
      else if(ng > 0)
        HIPCHK(hipMemcpyAsync(D.h0.p, ctx->f[GHIP_F_HSML].p, (size_t) ng * 8, hipMemcpyDeviceToDevice,
                              st));
      D.gh_sent = total;
      GCHK(pack_ghosts(ctx, total));
      set_alltoallv(D, D.gh_send.p, sizeof(GhostRec), D.gh_scount, D.gh_soff, &D.gh_recv);
      D.phase = ITERATE;
      return 1;
    }
  if(D.phase == ITERATE)
    {
      // gas tree over the local gas and the ghosts, the h iteration for the local targets
      D.nghost = D.x.rtotal;
      GCHK(ghip_dd_build_gas_tree(ctx));
      const bool failed = ghip_dd_hold(ctx, ghip_density_impl(ctx, &D.dp));
      // Every search radius used must have stayed inside the padded radius the ghosts were selected
      // with.  The reference re-exports a target at every h iteration, whatever its radius has become
      // (density.c:160-677); here the ghosts are fixed for the call, so a radius that outgrows the
      // padding -- the first density() of a run grows a poor guess by 1.26 per pass -- means: select the
      // ghosts again with a larger padding and repeat the call from the smoothing lengths it started
      // with.  The decision is taken by ALL shards on the all-gathered growth factors, so that they
      // repeat (or fail) together; a rank-local failure of the iteration travels the same way.
      double growth = 0.0;
      if(!failed && ctx->nt_gas > 0)
        {
          unsigned long long *dr = &ghip_words(ctx)->ghost_growth;
          HIPCHK(hipMemsetAsync(dr, 0, 8, st));
          k_ghost_growth<<<cdiv(ctx->nt_gas, 256), 256, 0, st>>>(
            ctx->nt_gas, P<int>(ctx->tg_gas), P<int>(ctx->st.perm), P<double>(ctx->dhcur),
            P<double>(ctx->dright), P<double>(D.h0), dr);
          HIPCHK(hipMemcpyAsync(&growth, dr, 8, hipMemcpyDeviceToHost, st));
          HIPCHK(ghip_stream_sync(ctx, st));
        }
      D.gh_growth = growth;
      GCHK(dd_post_status(ctx, growth, failed));
      D.phase = DECIDE;
      return 1;
    }
  if(D.phase == DECIDE)
    {
      double worst = 0;
      int failed = -1;
      GCHK(dd_read_status(ctx, &worst, &failed));
      if(worst > D.gh_margin_cur && P_ > 1)
        {
          // (a failed iteration of the incomplete attempt -- non-convergence next to missing ghosts --
          // is repeated like everything else)
          if(D.gh_retries >= 40)
            return ghip_fail(ctx, GHIP_ENOCONV, "density: the ghost radius grew %d times without covering "
                             "the smoothing lengths (largest growth %.3g)", D.gh_retries, worst);
          D.gh_retries++;
          D.gh_margin_cur = 1.26 * worst;   // one more pass of the reference's growth factor as head-room
          if(ng > 0)
            HIPCHK(hipMemcpyAsync(ctx->f[GHIP_F_HSML].p, D.h0.p, (size_t) ng * 8, hipMemcpyDeviceToDevice, st));
          D.phase = GROUPS;
          return density_step(ctx);   // groups with the larger padding -> all-gather -> ...
        }
      GCHK(ghip_dd_raise(ctx, failed, "density: the h iteration failed on shard %d (its own message "
                         "says why); every shard stops here", failed));
      // the ghosts' records as they are after density(): hydro_force needs h, rho, P, f, div, curl
      GCHK(pack_ghosts(ctx, D.gh_sent));
      set_alltoallv(D, D.gh_send.p, sizeof(GhostRec), D.gh_scount, D.gh_soff, &D.gh_recv);
      D.phase = REFRESH;
      return 1;
    }
  if(D.phase == REFRESH)
    {
      if(D.x.rtotal != D.nghost)
        return ghip_fail(ctx, GHIP_ECOMM, "ghost refresh: %d records, expected %d", D.x.rtotal, D.nghost);
      GCHK(ghip_dd_refresh_ghosts(ctx));
      D.phase = DONE;
      return GHIP_OK;
    }
  return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_step: density has no phase %d", D.phase);
}

// ---- migration --------------------------------------------------------------------------------
// domain_exchange (domain.c:665-1060): after a drift some particles lie outside their shard's key
// range; each moves to the shard that owns its key, with every resident field.  One record per
// particle: 8-byte slots, the fields in enum order (ints widened), then the shard's DragHeating when it
// holds one (ghip_dust.hip), then alpha and Dtalpha when it holds them (ghip_visc_set_alpha), then the three
// components of Injected_BH_Momentum and of RadAccel when it holds them for its gas count (ghip_wind.hip), slot
// MIG_SLOTS-1 = 1 for gas.  The optional slots have fixed places and travel as zero from a shard
// that does not hold the array.
#define MIG_SLOTS 48
#define MIG_NOPT 5     // optional per-gas arrays: DragHeating, alpha, Dtalpha, Injected_BH_Momentum, RadAccel
#define MIG_XSLOTS 9   // ... and their slots (the last two have three components)
struct MigRec
{
  unsigned long long s[MIG_SLOTS];
};
struct MigField
{
  void *p;
  int ncomp, isint, gas, slot;
};
struct MigTable
{
  int nf;
  MigField f[GHIP_F_COUNT + MIG_NOPT];   // the fields, + the optional arrays
  int xslot;                             // first of the optional slots
};
struct MigSplits
{
  int nseg, me;
  const unsigned long long *key;   // [nseg + 1]
  const int *owner;                // [nseg]
};

// heat: the per-gas DragHeating, or nullptr when the shard holds none; visc: alpha and Dtalpha, or nullptr; wind:
// Injected_BH_Momentum and RadAccel, each or nullptr
static MigTable mig_table(DevBuf *bufs, DevBuf *heat, DevBuf *const *visc, DevBuf *const *wind)
{
  MigTable T;
  T.nf = GHIP_F_COUNT;
  int slot = 0;
  for(int f = 0; f < GHIP_F_COUNT; f++)
    {
      ghip_field_info(f, &T.f[f].gas, &T.f[f].ncomp, &T.f[f].isint);
      T.f[f].p = bufs[f].p;
      T.f[f].slot = slot;
      slot += T.f[f].ncomp;
    }
  T.xslot = slot;
  DevBuf *const opt[MIG_NOPT] = {heat, visc ? visc[0] : nullptr, visc ? visc[1] : nullptr, wind[0], wind[1]};
  for(int k = 0; k < MIG_NOPT; k++)
    {
      const int ncomp = k < 3 ? 1 : 3;
      if(opt[k])
        {
          MigField &F = T.f[T.nf++];
          F.p = opt[k]->p;
          F.ncomp = ncomp;
          F.isint = 0;
          F.gas = 1;
          F.slot = slot;
        }
      slot += ncomp;
    }
  return T;   // T.xslot + MIG_XSLOTS <= MIG_SLOTS - 1 (checked by ghip_dd_begin)
}

__global__ void k_mig_dest(int n, const double *__restrict__ x, const double *__restrict__ y,
                           const double *__restrict__ z, double cx, double cy, double cz, double fac,
                           MigSplits S, unsigned long long *__restrict__ mask)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  // (clamped to the cube: a particle that left it goes to the owner of the boundary cell -- whose range
  // check then refuses it until the host has set a fresh extent, see d_cell21)
  const unsigned long long k = d_peano21(d_cell21(x[i], cx, fac), d_cell21(y[i], cy, fac), d_cell21(z[i], cz, fac));
  int lo = 0, hi = S.nseg - 1;   // largest s with key[s] <= k
  while(lo < hi)
    {
      int mid = (lo + hi + 1) >> 1;
      if(S.key[mid] <= k)
        lo = mid;
      else
        hi = mid - 1;
    }
  const int dest = S.owner[lo];
  mask[i] = (dest == S.me) ? 0ULL : (1ULL << dest);
}

__global__ void k_mig_pack(int nrec, const int *__restrict__ list, int n, int ngas, MigTable T,
                           MigRec *__restrict__ out)
{
  int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nrec)
    return;
  const int i = list[a];
  MigRec &r = out[a];
  const bool isgas = i < ngas;
  for(int k = 0; k < MIG_XSLOTS; k++)   // an optional array this shard does not hold: its slots travel as zero
    r.s[T.xslot + k] = 0;
  for(int f = 0; f < T.nf; f++)
    {
      const MigField F = T.f[f];
      const size_t pitch = F.gas ? ngas : n;
      for(int c = 0; c < F.ncomp; c++)
        {
          unsigned long long v = 0;
          if(!F.gas || isgas)
            {
              if(F.isint)
                v = (unsigned long long) (unsigned int) reinterpret_cast<const int *>(F.p)[c * pitch + i];
              else
                v = reinterpret_cast<const unsigned long long *>(F.p)[c * pitch + i];
            }
          r.s[F.slot + c] = v;
        }
    }
  r.s[MIG_SLOTS - 1] = isgas ? 1ULL : 0ULL;
}

// keep / gas flags packed for ONE scan: low word counts gas, high word counts the other types
__global__ void k_mig_flags_old(int n, int ngas, const unsigned long long *__restrict__ mask,
                                unsigned long long *__restrict__ v)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i < n)
    v[i] = mask[i] ? 0ULL : (i < ngas ? 1ULL : (1ULL << 32));
}

// (a header record -- slot MIG_SLOTS-1 = MIG_HEADER, slot 0 = which tables the sender holds: MIG_HAS_SINKS |
// MIG_HAS_WINDS -- is no particle: counted in headers[0], and per kind in headers[1] and [2], ranked nowhere)
#define MIG_HEADER 2ULL
#define MIG_HAS_SINKS 1ULL
#define MIG_HAS_WINDS 2ULL
__global__ void k_mig_flags_new(int nrecv, const MigRec *__restrict__ rec,
                                unsigned long long *__restrict__ v, unsigned long long *__restrict__ headers)
{
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if(j >= nrecv)
    return;
  const unsigned long long kind = rec[j].s[MIG_SLOTS - 1];
  if(kind == MIG_HEADER)
    {
      v[j] = 0;
      atomicAdd(headers, 1ULL);
      if(rec[j].s[0] & MIG_HAS_SINKS)
        atomicAdd(headers + 1, 1ULL);
      if(rec[j].s[0] & MIG_HAS_WINDS)
        atomicAdd(headers + 2, 1ULL);
    }
  else
    v[j] = kind ? 1ULL : (1ULL << 32);
}

struct MigHeaders
{
  int pos[GHIP_MAXRANKS];   // where the header of each destination goes, -1: none
};
__global__ void k_mig_headers(int nranks, MigHeaders H, unsigned long long tables, MigRec *__restrict__ out)
{
  const int r = blockIdx.x, k = threadIdx.x;
  if(r < nranks && H.pos[r] >= 0 && k < MIG_SLOTS)
    out[H.pos[r]].s[k] = k == MIG_SLOTS - 1 ? MIG_HEADER : (k == 0 ? tables : 0ULL);
}

struct MigCounts
{
  int kg, ko, rg, ro;   // kept gas / other, received gas / other
};

__global__ void k_mig_move_old(int n, int ngas, const unsigned long long *__restrict__ mask,
                               const unsigned long long *__restrict__ rank, MigCounts C, MigTable A,
                               MigTable Bn)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n || mask[i])
    return;
  const bool isgas = i < ngas;
  const int nn = C.kg + C.ko + C.rg + C.ro, ngn = C.kg + C.rg;
  const unsigned long long rk = rank[i];
  const int j = isgas ? (int) (rk & 0xffffffffULL) : ngn + (int) (rk >> 32);
  for(int f = 0; f < A.nf; f++)
    {
      const MigField F = A.f[f], G = Bn.f[f];
      if(F.gas && !isgas)
        continue;
      const size_t po = F.gas ? ngas : n, pn = F.gas ? ngn : nn;
      for(int c = 0; c < F.ncomp; c++)
        {
          if(F.isint)
            reinterpret_cast<int *>(G.p)[c * pn + j] = reinterpret_cast<const int *>(F.p)[c * po + i];
          else
            reinterpret_cast<double *>(G.p)[c * pn + j] =
              reinterpret_cast<const double *>(F.p)[c * po + i];
        }
    }
}

__global__ void k_mig_move_new(int nrecv, const MigRec *__restrict__ rec,
                               const unsigned long long *__restrict__ rank, MigCounts C, MigTable Bn)
{
  int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nrecv)
    return;
  const MigRec &r = rec[a];
  if(r.s[MIG_SLOTS - 1] == MIG_HEADER)
    return;
  const bool isgas = r.s[MIG_SLOTS - 1] != 0;
  const int nn = C.kg + C.ko + C.rg + C.ro, ngn = C.kg + C.rg;
  const unsigned long long rk = rank[a];
  const int j = isgas ? C.kg + (int) (rk & 0xffffffffULL) : ngn + C.ko + (int) (rk >> 32);
  for(int f = 0; f < Bn.nf; f++)
    {
      const MigField G = Bn.f[f];
      if(G.gas && !isgas)
        continue;
      const size_t pn = G.gas ? ngn : nn;
      for(int c = 0; c < G.ncomp; c++)
        {
          const unsigned long long v = r.s[G.slot + c];
          if(G.isint)
            reinterpret_cast<int *>(G.p)[c * pn + j] = (int) (unsigned int) v;
          else
            reinterpret_cast<unsigned long long *>(G.p)[c * pn + j] = v;
        }
    }
}

// GHIP_DD_MIGRATE:
//   SEND   the owner of every local particle's key; those of other shards packed   -> all-to-all-v of MigRec
//   MERGE  kept and received particles into the new layout (gas first), the resident arrays swapped
// and, when the shards hold wind tables (ghip_wind.hip; a header record in the first exchange says who holds what):
//   WROWS        the rows of the Type-3 particles that left, by their place in the run   -> all-to-all-v of row records
//                then: the staying rows re-keyed to the new layout, the arrivals keyed by theirs, sorted again
// and, when the shards hold sink tables (ghip_accretion.hip):
//   ROWS         the rows of the Type-5 particles that left                          -> all-to-all-v of row records
//   ROWS_STATUS  departed rows dropped, arrivals merged, the table sorted again      -> all-gather of the status
//                an ID that stands twice in one table stops all shards
// Exchanges: 1 without tables, 2 with wind tables, 3 with sink tables, 4 with both.
static int migrate_begin(ghip_ctx *ctx, int, const void *, int)
{
  static_assert(sizeof(MigRec) == MIG_SLOTS * 8, "MigRec layout");
  int slots = 0;
  for(int f = 0; f < GHIP_F_COUNT; f++)
    {
      int gas, ncomp, isint;
      ghip_field_info(f, &gas, &ncomp, &isint);
      slots += ncomp;
    }
  slots += MIG_XSLOTS;   // the optional arrays, when the shard holds them
  if(slots > MIG_SLOTS - 1)
    return ghip_fail(ctx, GHIP_EINVAL, "migration record too small for %d field slots", slots);
  return GHIP_OK;
}

static int migrate_step(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  hipStream_t st = ctx->stream;
  const int P_ = D.nranks, n = ctx->n, ng = ctx->ngas;
  // (a DragHeating that no longer matches the gas count -- ghip_set_counts since -- is not carried)
  DevBuf *heat = (ctx->dust_heat.p && ctx->dust_heat.cap >= (size_t) (ng > 0 ? ng : 1) * 8) ? &ctx->dust_heat
                                                                                           : nullptr;
  // (the same for alpha / Dtalpha: carried when they were given for the gas this shard holds)
  DevBuf *const visc_bufs[2] = {&ctx->visc_alpha, &ctx->visc_dtalpha};
  DevBuf *const visc_shadow[2] = {&D.visc_shadow[0], &D.visc_shadow[1]};
  DevBuf *const *visc = (ctx->visc_alpha.p && ctx->visc_dtalpha.p && ctx->visc_ngas == ng) ? visc_bufs : nullptr;
  // (the same for Injected_BH_Momentum and RadAccel: carried when they are held for the gas this shard holds)
  DevBuf *const wind[2] = {(ctx->wind_inj.p && ctx->wind_inj_ngas == ng) ? &ctx->wind_inj : nullptr,
                           (ctx->wind_ra.p && ctx->wind_ra_ngas == ng) ? &ctx->wind_ra : nullptr};
  DevBuf *const wind_shadow[2] = {wind[0] ? &D.wind_shadow[0] : nullptr, wind[1] ? &D.wind_shadow[1] : nullptr};
  enum { SEND, MERGE, DONE, ROWS, ROWS_STATUS, WROWS };
  // after the particles (and the wind rows): the sink rows' exchange, or the end
  auto sink_rows_or_done = [&]() {
    if(!D.mig_tab)
      return (int) GHIP_OK;
    ghip_sinks_mig_post(ctx);   // the rows of the Type-5 particles that left   -> all-to-all-v of row records
    D.phase = ROWS;
    return 1;
  };
  if(D.phase == SEND)
    {
      GHIP_JOIN(ctx);
      int scount[GHIP_MAXRANKS], soff[GHIP_MAXRANKS], total = 0;
      for(int r = 0; r < GHIP_MAXRANKS; r++)
        scount[r] = soff[r] = 0;
      GCHK(ghip_ensure(ctx, D.mig_mask, (size_t) (n > 0 ? n : 1) * 8));
      if(n > 0 && P_ > 1)
        {
          MigSplits S;
          S.nseg = D.nseg;
          S.me = D.rank;
          S.key = P<unsigned long long>(D.segkey);
          S.owner = P<int>(D.segowner);
          const double *x = P<double>(ctx->f[GHIP_F_POS]);
          const double fac = 1.0 / ctx->dlen * (double) (1ULL << GHIP_BITS);
          k_mig_dest<<<cdiv(n, 256), 256, 0, st>>>(n, x, x + n, x + 2 * (size_t) n, ctx->corner[0],
                                                   ctx->corner[1], ctx->corner[2], fac, S,
                                                   P<unsigned long long>(D.mig_mask));
          HIPCHK(hipGetLastError());
          GCHK(multi_select(ctx, n, P<unsigned long long>(D.mig_mask), D.mig_list, scount, soff, &total));
        }
      else if(n > 0)
        HIPCHK(hipMemsetAsync(D.mig_mask.p, 0, (size_t) n * 8, st));
      // A shard that holds a sink table (ghip_accretion.hip) says so to every other shard with one header record in
      // front of that shard's particles, and the rows of its departing Type-5 particles follow in a second exchange:
      // every shard then sees who holds a table, and all of them enter the second exchange or none does.
      // The same for the wind table (ghip_wind.hip), independently: its rows are keyed by particle index, so they are
      // packed by their particle's place in the run of its destination, before anything moves.
      D.mig_tab = ctx->sk.on && !ctx->sk.stale && P_ > 1;
      D.mig_wk = ctx->wk.on && !ctx->wk.stale && P_ > 1;
      const bool headers = D.mig_tab || D.mig_wk;
      GCHK(ghip_ensure(ctx, D.mig_send, (size_t) (headers ? total + P_ : (total > 0 ? total : 1)) * sizeof(MigRec)));
      if(D.mig_wk)
        GCHK(ghip_winds_mig_pack(ctx, total, P<int>(D.mig_list), scount, soff));
      if(D.mig_tab)
        GCHK(ghip_sinks_mig_pack(ctx, total, P<int>(D.mig_list), P<unsigned long long>(D.mig_mask)));
      if(headers)
        {
          const MigTable T = mig_table(ctx->f, heat, visc, wind);
          MigHeaders H;
          int shift = 0;
          for(int r = 0; r < GHIP_MAXRANKS; r++)
            H.pos[r] = -1;
          for(int r = 0; r < P_; r++)
            {
              const int from = soff[r];
              soff[r] += shift;
              if(r == D.rank)
                continue;
              H.pos[r] = soff[r];
              if(scount[r] > 0)
                k_mig_pack<<<cdiv(scount[r], 256), 256, 0, st>>>(scount[r], P<int>(D.mig_list) + from, n, ng, T,
                                                                P<MigRec>(D.mig_send) + soff[r] + 1);
              scount[r]++;
              shift++;
            }
          k_mig_headers<<<P_, 64, 0, st>>>(P_, H, (D.mig_tab ? MIG_HAS_SINKS : 0ULL) | (D.mig_wk ? MIG_HAS_WINDS : 0ULL),
                                           P<MigRec>(D.mig_send));
          HIPCHK(hipGetLastError());
        }
      else if(total > 0)
        {
          k_mig_pack<<<cdiv(total, 256), 256, 0, st>>>(total, P<int>(D.mig_list), n, ng,
                                                      mig_table(ctx->f, heat, visc, wind), P<MigRec>(D.mig_send));
          HIPCHK(hipGetLastError());
        }
      D.mig_out = total;
      set_alltoallv(D, D.mig_send.p, sizeof(MigRec), scount, soff, &D.mig_recv);
      D.phase = MERGE;
      return 1;
    }
  if(D.phase == MERGE)
    {
      const int nrecv = D.x.rtotal;
      D.mig_in = nrecv;
      D.phase = DONE;
      D.wk_plan.moved = false;
      if(nrecv == 0 && D.mig_out == 0 && !D.mig_tab && !D.mig_wk)
        {
          ctx->pot_n = -1;   // (the result of GHIP_DD_POTENTIAL belongs to the particle set before the migration)
          return GHIP_OK;    // nobody left, nobody came: the resident arrays stay as they are
        }
      // new positions: kept gas, received gas, kept others, received others
      GCHK(ghip_ensure(ctx, D.mig_scan, (size_t) (n + nrecv + 2) * 16 + 24));
      unsigned long long *vo = P<unsigned long long>(D.mig_scan), *ro = vo + (n + 1),
                         *vn = ro + (n + 1), *rn = vn + (nrecv + 1), *hw = rn + (nrecv + 1);
      // (layout: flags_old[n+1], rank_old[n+1], flags_new[nrecv+1], rank_new[nrecv+1]; the extra
      // zero entry makes the last rank the total; then the count of header records, of those that say "sink table" and
      // of those that say "wind table")
      HIPCHK(hipMemsetAsync(vo, 0, (size_t) (n + nrecv + 2) * 16 + 24, st));
      if(n > 0)
        k_mig_flags_old<<<cdiv(n, 256), 256, 0, st>>>(n, ng, P<unsigned long long>(D.mig_mask), vo);
      if(nrecv > 0)
        k_mig_flags_new<<<cdiv(nrecv, 256), 256, 0, st>>>(nrecv, P<MigRec>(D.mig_recv), vn, hw);
      HIPCHK(hipGetLastError());
      GCHK(ghip_scan(ctx, vo, ro, n + 1, ctx->stream));
      GCHK(ghip_scan(ctx, vn, rn, nrecv + 1, ctx->stream));
      unsigned long long tot[5];
      HIPCHK(hipMemcpyAsync(&tot[0], ro + n, 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(&tot[1], rn + nrecv, 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(&tot[2], hw, 24, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      // every other shard's header says the same, per kind of table, or no shard holds that kind: all shards see the
      // same picture and stop together, before anything moved
      const int nhdr = (int) tot[2], nsk = (int) tot[3], nwk = (int) tot[4];
      if(nsk != (D.mig_tab ? P_ - 1 : 0))
        return ghip_fail(ctx, GHIP_EINVAL, "GHIP_DD_MIGRATE: %d of the %d other shards hold a sink table and this one "
                         "holds %s: either all shards hold one (an empty one counts) or none does "
                         "(ghip_sinks_set_table / ghip_sinks_clear); every shard stops here, nothing was moved",
                         nsk, P_ - 1, D.mig_tab ? "one" : "none");
      if(nwk != (D.mig_wk ? P_ - 1 : 0))
        return ghip_fail(ctx, GHIP_EINVAL, "GHIP_DD_MIGRATE: %d of the %d other shards hold a wind table and this one "
                         "holds %s: either all shards hold one (an empty one counts) or none does "
                         "(ghip_dd_winds_set_table / ghip_dd_winds_clear); every shard stops here, nothing was moved",
                         nwk, P_ - 1, D.mig_wk ? "one" : "none");
      if(nhdr != (D.mig_tab || D.mig_wk ? P_ - 1 : 0))
        return ghip_fail(ctx, GHIP_ECOMM, "GHIP_DD_MIGRATE: %d header records from %d other shards", nhdr, P_ - 1);
      D.mig_in = nrecv - nhdr;
      ctx->pot_n = -1;   // (the result of GHIP_DD_POTENTIAL belongs to the particle set before the migration)
      if(D.mig_in == 0 && D.mig_out == 0)
        {
          // (only shards with tables come here: the rows' exchanges are collectives)
          if(D.mig_wk)
            {
              ghip_winds_mig_post(ctx);
              D.phase = WROWS;
              return 1;
            }
          return sink_rows_or_done();
        }
      // (a wind field held for another gas count is not carried: it is dropped with the layout it belonged to)
      if(!wind[0])
        ctx->wind_inj_ngas = -1;
      if(!wind[1])
        ctx->wind_ra_ngas = -1;
      MigCounts C;
      C.kg = (int) (tot[0] & 0xffffffffULL);
      C.ko = (int) (tot[0] >> 32);
      C.rg = (int) (tot[1] & 0xffffffffULL);
      C.ro = (int) (tot[1] >> 32);
      const int nn = C.kg + C.ko + C.rg + C.ro, ngn = C.kg + C.rg;
      for(int f = 0; f < GHIP_F_COUNT; f++)
        {
          int gas, ncomp, isint;
          ghip_field_info(f, &gas, &ncomp, &isint);
          size_t bytes = (size_t) (gas ? ngn : nn) * ncomp * (isint ? 4 : 8);
          size_t before = D.fshadow[f].cap;
          GCHK(ghip_ensure(ctx, D.fshadow[f], bytes));
          if(D.fshadow[f].cap != before)
            HIPCHK(hipMemsetAsync(D.fshadow[f].p, 0, D.fshadow[f].cap, st));
        }
      if(heat)
        GCHK(ghip_ensure(ctx, D.heat_shadow, (size_t) (ngn > 0 ? ngn : 1) * 8));
      if(visc)
        for(int k = 0; k < 2; k++)
          GCHK(ghip_ensure(ctx, D.visc_shadow[k], (size_t) (ngn > 0 ? ngn : 1) * 8));
      for(int k = 0; k < 2; k++)
        if(wind[k])
          GCHK(ghip_ensure(ctx, D.wind_shadow[k], 3 * (size_t) (ngn > 0 ? ngn : 1) * 8));
      const MigTable A = mig_table(ctx->f, heat, visc, wind),
                     Bn = mig_table(D.fshadow, heat ? &D.heat_shadow : nullptr, visc ? visc_shadow : nullptr,
                                    wind_shadow);
      if(n > 0)
        k_mig_move_old<<<cdiv(n, 256), 256, 0, st>>>(n, ng, P<unsigned long long>(D.mig_mask), ro, C,
                                                     A, Bn);
      if(nrecv > 0)
        k_mig_move_new<<<cdiv(nrecv, 256), 256, 0, st>>>(nrecv, P<MigRec>(D.mig_recv), rn, C, Bn);
      HIPCHK(hipGetLastError());
      HIPCHK(ghip_stream_sync(ctx, st));
      for(int f = 0; f < GHIP_F_COUNT; f++)
        ctx->f[f].swap(D.fshadow[f]);
      if(heat)
        ctx->dust_heat.swap(D.heat_shadow);
      if(visc)
        {
          ctx->visc_alpha.swap(D.visc_shadow[0]);
          ctx->visc_dtalpha.swap(D.visc_shadow[1]);
        }
      if(wind[0])
        {
          ctx->wind_inj.swap(D.wind_shadow[0]);
          ctx->wind_inj_ngas = ngn;
        }
      if(wind[1])
        {
          ctx->wind_ra.swap(D.wind_shadow[1]);
          ctx->wind_ra_ngas = ngn;
        }
      ctx->visc_ngas = visc ? ngn : -1;
      ctx->visc_epoch++;
      ctx->n = nn;
      ctx->ngas = ngn;
      ctx->gt.built = false;
      ctx->st.built = false;
      D.geom_kept = false;
      ctx->nactive = -1;
      ctx->lists_dirty = ctx->gas_list_dirty = true;
      ctx->gas_types_unknown = true;   // (an arrival may be a converted particle of its old gas block)
      // (SwallowID is per particle and does not travel: no mark of the old layout may be read as one of the new)
      if(ctx->bh_swallow.p)
        HIPCHK(hipMemsetAsync(ctx->bh_swallow.p, 0, ctx->bh_swallow.cap, st));
      // the wind table is keyed by particle index: what MERGE knows of the renumbering stays for its rows (the
      // table counts as stale until they are merged; one that was stale before is not carried)
      if(ctx->wk.on)
        ctx->wk.stale = true;
      if(D.mig_wk)
        {
          WkMigPlan &M = D.wk_plan;
          M.moved = true;
          M.n_old = n;
          M.ng_old = ng;
          M.nrecv = nrecv;
          M.ngn = ngn;
          M.ko = C.ko;
          M.mask = P<unsigned long long>(D.mig_mask);
          M.ro = ro;
          M.vn = vn;
          M.rn = rn;
          for(int r = 0; r < GHIP_MAXRANKS; r++)   // (every other shard sent a header in front of its particles)
            {
              const bool other = r < P_ && r != D.rank;
              M.first[r] = other ? D.x.roff[r] + 1 : 0;
              M.cnt[r] = other ? D.x.rcount[r] - 1 : 0;
            }
          ghip_winds_mig_post(ctx);   // the rows of the Type-3 particles that left   -> all-to-all-v of row records
          D.phase = WROWS;
          return 1;
        }
      return sink_rows_or_done();
    }
  if(D.phase == WROWS)
    {
      GCHK(ghip_winds_mig_merge(ctx));
      D.phase = DONE;
      return sink_rows_or_done();
    }
  if(D.phase == ROWS)
    {
      // the rows that left are dropped, the arrivals merged, the table sorted by ID again; an ID that now stands
      // twice stops all shards (the status round carries it)
      const bool failed = ghip_dd_hold(ctx, ghip_sinks_mig_merge(ctx));
      GCHK(dd_post_status(ctx, failed ? (double) ctx->sk.last_dup : 0.0, failed));
      D.phase = ROWS_STATUS;
      return 1;
    }
  if(D.phase == ROWS_STATUS)
    {
      double id = 0;
      int failed = -1;
      GCHK(dd_read_status(ctx, &id, &failed));
      D.phase = DONE;
      return ghip_dd_raise(ctx, failed, "GHIP_DD_MIGRATE: shard %d could not merge the arriving rows into its sink "
                           "table: the ID %u stands in it twice (its own message says so; that shard holds no table "
                           "now); every shard stops here", failed, (unsigned int) id);
    }
  return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_step: migration has no phase %d", D.phase);
}

// GHIP_DD_HYDRO: one step.  The ghosts' records are current since the end of GHIP_DD_DENSITY: hydro_force is local
static int hydro_begin(ghip_ctx *ctx, int, const void *params, int)
{
  DDState &D = ctx->dd;
  GCHK(ghip_visc_ready(ctx, "GHIP_DD_HYDRO"));
  // the ghosts in place carry their owners' alpha as of the refresh that ended GHIP_DD_DENSITY; the local
  // records take the alpha of this call (k_visc_refresh): a pair across shards must not mix the two
  if(ctx->visc_on && ctx->visc.time_dependent && D.nranks > 1 && D.gh_alpha_epoch != ctx->visc_epoch)
    return ghip_fail(ctx, GHIP_EINVAL, "GHIP_DD_HYDRO: alpha changed (ghip_visc_set_alpha or a kick) since "
                     "the GHIP_DD_DENSITY that packed the ghosts: run GHIP_DD_DENSITY again, on all ranks");
  D.hp = *reinterpret_cast<const ghip_hydro_params *>(params);
  return GHIP_OK;
}

static int hydro_step(ghip_ctx *ctx) { return ghip_hydro_impl(ctx, &ctx->dd.hp); }

// The operations, indexed by GHIP_DD_*.  needs_grav_tree: the operation reads the tree of this step's
// GHIP_DD_GRAVITY and refuses the one GHIP_DD_POTENTIAL leaves behind (selected for other targets).
struct DDOp
{
  const char *name;
  int (*begin)(ghip_ctx *ctx, int op, const void *params, int walk);
  int (*step)(ghip_ctx *ctx);
  bool needs_grav_tree, null_params;
};
static const DDOp dd_ops[] = {
  {nullptr, nullptr, nullptr, false, false},
  {"GHIP_DD_MIGRATE", migrate_begin, migrate_step, false, true},
  {"GHIP_DD_GRAVITY", gravity_begin, gravity_step, false, false},
  {"GHIP_DD_DENSITY", density_begin, density_step, true, false},
  {"GHIP_DD_HYDRO", hydro_begin, hydro_step, false, false},
  {"GHIP_DD_SINK_DENSITY", ghip_dd_sink_begin, ghip_dd_sink_step, true, false},
  {"GHIP_DD_BH_EVALUATE", ghip_dd_sink_begin, ghip_dd_sink_step, true, false},
  {"GHIP_DD_BH_SWALLOW", ghip_dd_sink_begin, ghip_dd_sink_step, true, false},
  {"GHIP_DD_PM", ghip_dd_pm_begin, ghip_dd_pm_step, false, false},
  {"GHIP_DD_DUST_DENSITY", ghip_dd_dust_begin, ghip_dd_dust_step, true, false},
  {"GHIP_DD_DUST_DRAG", ghip_dd_dust_begin, ghip_dd_dust_step, true, false},
  {"GHIP_DD_POTENTIAL", ghip_dd_pot_begin, ghip_dd_pot_step, false, false},
  {"GHIP_DD_GLOBAL_QUANTITIES", ghip_dd_gq_begin, ghip_dd_gq_step, false, false},
  {"GHIP_DD_DECOMPOSE", ghip_dd_decomp_begin, ghip_dd_decomp_step, false, false},
  {"GHIP_DD_PM_REGION", ghip_dd_pmreg_begin, ghip_dd_pmreg_step, false, false},
  {"GHIP_DD_PM_NONPERIODIC", ghip_dd_pmnp_begin, ghip_dd_pmnp_step, false, false},
};
static_assert(sizeof(dd_ops) / sizeof(dd_ops[0]) == DD_NOPS && DD_NOPS == GHIP_DD_PM_NONPERIODIC + 1,
              "one entry of dd_ops per GHIP_DD_* operation");

extern "C" int ghip_dd_begin(ghip_ctx *ctx, int op, const void *params, int walk)
{
  const bool known = op >= 1 && op < DD_NOPS;
  if(!ctx || (!params && !(known && dd_ops[op].null_params)))
    return GHIP_EINVAL;
  DDState &D = ctx->dd;
  if(!D.on)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_begin: call ghip_dd_init first");
  if(!(ctx->dlen > 0))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_begin: call ghip_dd_set_domain first");
  if(ctx->rnd_n > 0)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_begin: not while a table is bound with ghip_set_rnd_table (the cell "
                     "of a pruned node inside a randomised region does not follow from a key range): unbind it");
  if(D.x.kind != 0)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_begin: an exchange is still pending");
  if(!known)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_begin: unknown operation %d", op);
  HIPCHK(hipSetDevice(ctx->device));
  if(dd_ops[op].needs_grav_tree && D.gt_is_pot && ctx->gt.built)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_begin: operation %d needs GHIP_DD_GRAVITY of this step, and the "
                     "tree in place is the one GHIP_DD_POTENTIAL built: run GHIP_DD_GRAVITY first", op);
  D.held.rc = GHIP_OK;
  GCHK(dd_ops[op].begin(ctx, op, params, walk));
  D.op = op;
  D.phase = 0;
  D.bytes_sent[op] = 0;
  return GHIP_OK;
}

// 1: an exchange is pending (ghip_dd_exchange / ghip_dd_exchange_local), 0: the operation is
// complete, < 0: error.  The operation is over when its step returns <= 0, complete or failed, and this is the
// one place that says so: a further ghip_dd_step without a new ghip_dd_begin finds no operation in progress.
extern "C" int ghip_dd_step(ghip_ctx *ctx)
{
  if(!ctx)
    return GHIP_EINVAL;
  DDState &D = ctx->dd;
  if(D.x.kind != 0)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_step: run the pending exchange first");
  HIPCHK(hipSetDevice(ctx->device));
  if(D.op < 1 || D.op >= DD_NOPS)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_step: no operation in progress");
  const int r = dd_ops[D.op].step(ctx);
  if(r <= 0)
    D.op = 0;
  return r;
}

// the whole operation over RCCL (one process per GPU)
extern "C" int ghip_dd_run(ghip_ctx *ctx, int op, const void *params, int walk)
{
  GCHK(ghip_dd_begin(ctx, op, params, walk));
  for(;;)
    {
      int r = ghip_dd_step(ctx);
      if(r <= 0)
        return r;
      GCHK(ghip_dd_exchange(ctx));
    }
}

extern "C" int ghip_dd_get_info(const ghip_ctx *ctx, long long out[16])
{
  if(!ctx || !out)
    return GHIP_EINVAL;
  const DDState &D = ctx->dd;
  for(int i = 0; i < 16; i++)
    out[i] = 0;
  out[0] = D.rank;
  out[1] = D.nranks;
  out[2] = D.gt_nimp;                  // elements imported into the gravity tree
  out[3] = D.let_sent;                 // elements this shard sent
  out[4] = D.nghost;                   // ghost gas particles imported
  out[5] = D.gh_sent;                  // ghosts sent
  out[6] = D.bytes_sent[GHIP_DD_GRAVITY];
  out[7] = D.bytes_sent[GHIP_DD_DENSITY];
  out[8] = (long long) (D.gh_growth * 1.0e6);
  out[9] = ctx->gt.nelem;
  out[10] = ctx->st.nelem;
  out[11] = ctx->n;
  out[12] = ctx->ngas;
  out[13] = D.mig_out;
  out[14] = D.mig_in;
  out[15] = D.bytes_sent[GHIP_DD_MIGRATE];
  return GHIP_OK;
}

extern "C" int ghip_dd_set_guests(ghip_ctx *ctx, int on)
{
  if(!ctx || !ctx->dd.on)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_set_guests: call ghip_dd_init first");
  if(ctx->dd.op != 0)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_set_guests: not while an operation is in progress");
  ctx->dd.guests_on = on != 0;
  return GHIP_OK;
}

extern "C" int ghip_dd_guest_counts(const ghip_ctx *ctx, long long out[2])
{
  if(!ctx || !out)
    return GHIP_EINVAL;
  out[0] = ctx->dd.guests_held;
  out[1] = ctx->dd.guests_hosted;
  return GHIP_OK;
}

extern "C" int ghip_dd_bytes_sent(const ghip_ctx *ctx, int op, long long *bytes)
{
  if(!ctx || !bytes || op < 1 || op >= DD_NOPS)
    return GHIP_EINVAL;
  *bytes = ctx->dd.bytes_sent[op];
  return GHIP_OK;
}

void ghip_dd_release(ghip_ctx *ctx)
{
  if(!ctx)
    return;
  ghip_dd_comm_release(ctx);
  ghip_renew(ctx->dd);
}
