// ghip_decomp.hip -- GHIP_DD_DECOMPOSE: the domain decomposition itself on the resident particles of all
// shards (domain.c:100 domain_Decomposition: domain_findExtent :1972-2014, the cost sum per piece of the
// curve :378-384, domain_findSplit_work_balanced :1075-1113).  It moves no particle; GHIP_DD_MIGRATE does.
//
//   phase 0  k_decomp_extent: one pass over the positions gives xmin[3] / xmax[3] (integer atomic min / max
//            on the order-preserving u64 image of a double: no float atomics), the smallest and largest
//            effective time bin and an error word; with the count they make one block of DC_WORDS u64,
//            all-gathered.
//   phase 1  every rank reads the same bytes in rank order: the cube (the reference's arithmetic, in double,
//            in its order), the level, bmin / bmax, N.  Whatever is wrong is wrong on all ranks alike, so they
//            fail together.  k_decomp_hist: leading key digits = cell -> u64 histogram of integer weights; all-gathered.
//   phase 2  k_decomp_sum adds the histograms; the host converts 8^L words to double, cuts them with
//            ghip_dd_find_split and stores splits and cube.
//
// The reference refines a top-tree until its leaves hold little work and cuts the leaves (domain.c:1738-1960);
// here the leaves are the 8^L cells of one level, as in sharded.decompose.
#include <cfloat>

#include "ghip_keys.h"

#define DC_WORDS 16   // 0-2: images of xmin, 3-5: of xmax, 6: particles, 7: least time bin, 8: largest, 9: errors
#define DC_ERR_POS 1ULL     // a position that is not finite
#define DC_ERR_WORK 2ULL    // a TimeBin outside [0, TIMEBINS] or a negative GravCost
#define DC_ERR_LOCAL 4ULL   // this shard's own pass failed (a HIP error, a pair that did not join): its return code
                            // stays with it, the bit makes every shard stop with it
#define DC_TIMEBINS 29      // TIMEBINS, allvars.h:39: a particle of bin 0 costs (1 + GravCost) / TIMEBASE
#define DC_LDS_LEVEL 4      // up to this level the histogram of a workgroup lives in the LDS (8^4 x 8 B = 32 KB)

// u64 whose unsigned order is the order of the doubles (-0.0 sorts below +0.0: the kernel adds +0.0 first)
static __host__ __device__ __forceinline__ unsigned long long dc_image(double d)
{
  unsigned long long b;
  memcpy(&b, &d, 8);
  return (b >> 63) ? ~b : (b | (1ULL << 63));
}

static inline double dc_unimage(unsigned long long m)
{
  const unsigned long long b = (m >> 63) ? (m & ~(1ULL << 63)) : ~m;
  double d;
  memcpy(&d, &b, 8);
  return d;
}

__global__ void __launch_bounds__(256)
k_decomp_extent(int n, const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                int use_work, const int *__restrict__ cost, const int *__restrict__ tbin,
                unsigned long long *__restrict__ blk)
{
  double mn[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, mx[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
  int bmin = 0x7fffffff, bmax = 0;
  unsigned long long err = 0;
  for(long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x)
    {
      const double p[3] = {x[i] + 0.0, y[i] + 0.0, z[i] + 0.0};
      for(int j = 0; j < 3; j++)
        {
          if(!(fabs(p[j]) <= DBL_MAX))
            err |= DC_ERR_POS;
          else
            {
              mn[j] = p[j] < mn[j] ? p[j] : mn[j];
              mx[j] = p[j] > mx[j] ? p[j] : mx[j];
            }
        }
      if(use_work)
        {
          const int t = tbin[i];
          if(t < 0 || t > DC_TIMEBINS || cost[i] < 0)
            err |= DC_ERR_WORK;
          else
            {
              const int b = t ? t : DC_TIMEBINS;
              bmin = b < bmin ? b : bmin;
              bmax = b > bmax ? b : bmax;
            }
        }
    }
  for(int j = 0; j < 3; j++)
    {
      mn[j] = d_wave_min_f64(mn[j]);
      mx[j] = d_wave_max_f64(mx[j]);
    }
  bmin = d_wave_min_i32(bmin);
  bmax = d_wave_max_i32(bmax);
  err = d_wave_or_u64(err);
  if((threadIdx.x & (GHIP_WAVE - 1)) == 0)
    {
      for(int j = 0; j < 3; j++)
        {
          atomicMin(&blk[j], dc_image(mn[j]));
          atomicMax(&blk[3 + j], dc_image(mx[j]));
        }
      if(use_work)
        {
          atomicMin(&blk[7], (unsigned long long) bmin);
          atomicMax(&blk[8], (unsigned long long) bmax);
        }
      if(err)
        atomicOr(&blk[9], err);
    }
}

// The scatter-add.  The particles of a shard are in curve order after a migration, and clustered ones fall into
// few cells: lanes that hold the same cell as their neighbour form runs, each run is summed inside the
// wavefront (a segmented scan: 6 shuffles) and its last lane issues ONE 64-bit integer atomic add.  LDS = true
// (8^L x 8 B fit into the LDS): the adds go to the workgroup's own histogram, which is flushed once, one
// global atomic per cell the workgroup touched.  Integer sums: the result does not depend on arrival order.
template <bool LDS>
__global__ void __launch_bounds__(256)
k_decomp_hist(int n, const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
              double cx, double cy, double cz, double fac, int level, int ncell, int use_work,
              const int *__restrict__ cost, const int *__restrict__ tbin, int bmax, int wshift,
              unsigned long long *__restrict__ hist)
{
  extern __shared__ unsigned long long s_hist[];
  if(LDS)
    {
      for(int c = threadIdx.x; c < ncell; c += blockDim.x)
        s_hist[c] = 0;
      __syncthreads();
    }
  const int lane = threadIdx.x & (GHIP_WAVE - 1);
  const long long stride = (long long) gridDim.x * blockDim.x;
  // (whole wavefronts go round together: the shuffles below need all 64 lanes)
  for(long long base = (long long) blockIdx.x * blockDim.x + (threadIdx.x - lane); base < n; base += stride)
    {
      const long long i = base + lane;
      unsigned int cell = 0xffffffffu;   // no particle: a run of its own, never added
      unsigned long long w = 0;
      if(i < n)
        {
          // (the leading `level` digits of the key are all the cell needs: 3 * level bits of d_peano21's 63)
          cell = d_peano_top(d_cell21(x[i], cx, fac), d_cell21(y[i], cy, fac), d_cell21(z[i], cz, fac), level);
          w = 1;
          if(use_work)
            {
              const int t = tbin[i];
              const int b = t ? t : DC_TIMEBINS;
              w = ((1ULL + (unsigned long long) (unsigned int) cost[i]) << (bmax - b)) >> wshift;
              w = w ? w : 1;
            }
        }
      const unsigned int before = __shfl_up(cell, 1, GHIP_WAVE), after = __shfl_down(cell, 1, GHIP_WAVE);
      const bool head = lane == 0 || before != cell, tail = lane == GHIP_WAVE - 1 || after != cell;
      const unsigned long long heads = __ballot(head);
      // first lane of this lane's run: the highest head at or below it
      const int first = 63 - __clzll((long long) (heads & (~0ULL >> (63 - lane))));
      const int dist = lane - first;
      for(int off = 1; off < GHIP_WAVE; off <<= 1)
        {
          const unsigned long long o = __shfl_up(w, off, GHIP_WAVE);
          if(dist >= off)
            w += o;
        }
      if(tail && i < n && cell < (unsigned int) ncell)
        {
          if(LDS)
            atomicAdd(&s_hist[cell], w);
          else
            atomicAdd(&hist[cell], w);
        }
    }
  if(LDS)
    {
      __syncthreads();
      for(int c = threadIdx.x; c < ncell; c += blockDim.x)
        {
          const unsigned long long v = s_hist[c];
          if(v)
            atomicAdd(&hist[c], v);
        }
    }
}

__global__ void k_decomp_sum(int ncell, int nranks, const unsigned long long *__restrict__ all,
                             unsigned long long *__restrict__ out)
{
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if(c >= ncell)
    return;
  unsigned long long s = 0;
  for(int r = 0; r < nranks; r++)
    s += all[(size_t) r * ncell + c];
  out[c] = s;
}

// One pass of k_decomp_extent over the resident positions of the context into `own` (shared with the region of
// the non-periodic mesh, ghip_pm.hip).  The block is complete when this returns, also after a failure.
int ghip_extent_pass(ghip_ctx *ctx, DevBuf &own, int use_work)
{
  static_assert(DC_WORDS == EXTENT_WORDS && DC_ERR_POS == EXTENT_ERR_POS && DC_ERR_WORK == EXTENT_ERR_WORK &&
                  DC_ERR_LOCAL == EXTENT_ERR_LOCAL, "the extent block as ghip_internal.h describes it");
  hipStream_t st = ctx->stream;
  const int n = ctx->n;
  const double *x = P<double>(ctx->f[GHIP_F_POS]);
  const int *cost = P<int>(ctx->f[GHIP_F_GRAVCOST]), *tbin = P<int>(ctx->f[GHIP_F_TIMEBIN]);
  unsigned long long blk[DC_WORDS];
  for(int w = 0; w < DC_WORDS; w++)
    blk[w] = 0;
  for(int j = 0; j < 3; j++)   // (an empty shard contributes +MAX / -MAX)
    {
      blk[j] = dc_image(DBL_MAX);
      blk[3 + j] = dc_image(-DBL_MAX);
    }
  blk[6] = (unsigned long long) n;
  blk[7] = 0x7fffffffULL;
  GCHK(ghip_ensure(ctx, own, sizeof(blk)));
  auto pass = [&]() -> int {
    GHIP_JOIN(ctx);
    HIPCHK(hipMemcpyAsync(own.p, blk, sizeof(blk), hipMemcpyHostToDevice, st));
    if(n > 0)
      {
        const int nb = cdiv(n, 256 * 8);
        k_decomp_extent<<<nb < 2048 ? nb : 2048, 256, 0, st>>>(n, x, x + n, x + 2 * (size_t) n, use_work, cost,
                                                                tbin, P<unsigned long long>(own));
        HIPCHK(hipGetLastError());
      }
    HIPCHK(ghip_stream_sync(ctx, st));   // (`blk` lives on this frame)
    return GHIP_OK;
  };
  const int rc = pass();
  if(rc != GHIP_OK)
    {
      const std::string msg = ctx->err;
      blk[9] = DC_ERR_LOCAL;
      HIPCHK(hipMemcpy(own.p, blk, sizeof(blk), hipMemcpyHostToDevice));
      ctx->err = msg;
    }
  return rc;
}

// the same bytes in the same order on every rank: every decision taken on the result is everybody's
unsigned long long ghip_extent_reduce(const unsigned long long *all, int nranks, double xmin[3], double xmax[3],
                                      unsigned long long *ntot, int *bmin, int *bmax, int *bad)
{
  unsigned long long err = 0;
  for(int j = 0; j < 3; j++)
    {
      xmin[j] = DBL_MAX;
      xmax[j] = -DBL_MAX;
    }
  *ntot = 0;
  *bmin = 0x7fffffff;
  *bmax = 0;
  *bad = -1;
  for(int r = 0; r < nranks; r++)
    {
      const unsigned long long *b = &all[(size_t) r * DC_WORDS];
      for(int j = 0; j < 3; j++)
        {
          const double lo = dc_unimage(b[j]), hi = dc_unimage(b[3 + j]);
          xmin[j] = lo < xmin[j] ? lo : xmin[j];
          xmax[j] = hi > xmax[j] ? hi : xmax[j];
        }
      *ntot += b[6];
      *bmin = (int) b[7] < *bmin ? (int) b[7] : *bmin;
      *bmax = (int) b[8] > *bmax ? (int) b[8] : *bmax;
      if(b[9] && *bad < 0)
        *bad = r;
      err |= b[9];
    }
  return err;
}

int ghip_dd_decomp_begin(ghip_ctx *ctx, int op, const void *params, int walk)
{
  DDState &D = ctx->dd;
  // the other thing run() does between two steps shares the operation: `walk` selects the form, as for the dust
  // operations (ghip_sync.hip)
  D.walk = walk;
  if(walk == GHIP_SYNC_POINT_FORM)
    return ghip_dd_sync_begin(ctx, op, params, walk);
  D.dcp = *reinterpret_cast<const ghip_dd_decomp_params *>(params);
  const ghip_dd_decomp_params &p = D.dcp;
  if(p.level < 0 || p.level > 7)
    return ghip_fail(ctx, GHIP_EINVAL, "GHIP_DD_DECOMPOSE: level %d is not 0 (automatic) or 1..7", p.level);
  if(p.level > 0 && (1LL << (3 * p.level)) < D.nranks)
    return ghip_fail(ctx, GHIP_EINVAL, "GHIP_DD_DECOMPOSE: level %d has %lld cells, fewer than the %d ranks",
                     p.level, 1LL << (3 * p.level), D.nranks);
  if((p.use_work != 0 && p.use_work != 1) || (p.find_extent != 0 && p.find_extent != 1) || p.reserved != 0)
    return ghip_fail(ctx, GHIP_EINVAL, "GHIP_DD_DECOMPOSE: use_work and find_extent are 0 or 1, reserved is 0");
  return GHIP_OK;
}

// is x inside the cube as d_cell21 sees it?  ((x - corner) * fac is monotone in x: the extremes decide)
static inline bool dc_inside(double x, double corner, double fac)
{
  const double c = (x - corner) * fac;
  return c >= 0 && c < (double) (1 << GHIP_BITS);
}

// GHIP_DD_DECOMPOSE:
//   EXTENT     this shard's extremes, count, time bins and error bits             -> all-gather of the blocks
//   HISTOGRAM  every shard fails if one did; the cube and the level; this shard's work per cell
//                                                                                 -> all-gather of the histograms
//   CUT        the histograms added, the curve cut into ranges, the ranges (and the cube) put in force
int ghip_dd_decomp_step(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  if(D.walk == GHIP_SYNC_POINT_FORM)
    return ghip_dd_sync_step(ctx);
  hipStream_t st = ctx->stream;
  const ghip_dd_decomp_params &p = D.dcp;
  const int P_ = D.nranks, n = ctx->n;
  const double *x = P<double>(ctx->f[GHIP_F_POS]);
  const int *cost = P<int>(ctx->f[GHIP_F_GRAVCOST]), *tbin = P<int>(ctx->f[GHIP_F_TIMEBIN]);
  enum { EXTENT, HISTOGRAM, CUT };
  if(D.phase == EXTENT)
    {
      // what goes wrong on this shard alone travels in the block too: its peers are inside the same collective
      // and must not be left there (the held failure of the density and the potential, ghip_dd_hold)
      if(ghip_dd_hold(ctx, ghip_extent_pass(ctx, D.dc_own, p.use_work)) && !D.dc_own.p)
        return D.held.rc;   // (without the block there is nothing to send)
      ghip_dd_set_allgather(D, D.dc_own.p, DC_WORDS * 8, &D.dc_all);
      D.phase = HISTOGRAM;
      return 1;
    }
  if(D.phase == HISTOGRAM)
    {
      std::vector<unsigned long long> all((size_t) P_ * DC_WORDS);
      HIPCHK(hipMemcpyAsync(all.data(), D.dc_all.p, all.size() * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      // the same bytes in the same order on every rank: every decision below is everybody's
      double xmin[3], xmax[3];
      unsigned long long ntot = 0;
      int bmin = 0x7fffffff, bmax = 0, bad = -1;
      const unsigned long long err = ghip_extent_reduce(all.data(), P_, xmin, xmax, &ntot, &bmin, &bmax, &bad);
      if(err & DC_ERR_LOCAL)
        return ghip_dd_raise(ctx, bad, "GHIP_DD_DECOMPOSE: the first pass failed on shard %d (its own message "
                             "says why); every shard stops here, nothing was changed", bad);
      if(err & DC_ERR_POS)
        return ghip_fail(ctx, GHIP_EINVAL, "GHIP_DD_DECOMPOSE: a position that is not finite (first on shard %d); "
                         "every shard stops here, nothing was changed", bad);
      if(err & DC_ERR_WORK)
        return ghip_fail(ctx, GHIP_EINVAL, "GHIP_DD_DECOMPOSE: use_work needs 0 <= TimeBin <= %d and GravCost >= 0 "
                         "(first on shard %d); every shard stops here, nothing was changed", DC_TIMEBINS, bad);
      if(ntot == 0)
        return ghip_fail(ctx, GHIP_EINVAL, "GHIP_DD_DECOMPOSE: no shard holds a particle");
      if(ntot > 0x7fffffffULL * GHIP_MAXRANKS)
        return ghip_fail(ctx, GHIP_EINVAL, "GHIP_DD_DECOMPOSE: particle counts do not add up");
      if(p.find_extent)
        {
          // domain_findExtent, domain.c:1996-2011, operation by operation
          double len = 0;
          for(int j = 0; j < 3; j++)
            if(xmax[j] - xmin[j] > len)
              len = xmax[j] - xmin[j];
          len *= 1.001;
          for(int j = 0; j < 3; j++)
            {
              D.dc_center[j] = 0.5 * (xmin[j] + xmax[j]);
              D.dc_corner[j] = 0.5 * (xmin[j] + xmax[j]) - 0.5 * len;
            }
          D.dc_len = len;
          if(!(len > 0) || !(len <= DBL_MAX))
            return ghip_fail(ctx, GHIP_EINVAL, "GHIP_DD_DECOMPOSE: the extent of the particles has length %g", len);
        }
      else
        {
          for(int j = 0; j < 3; j++)
            {
              D.dc_center[j] = ctx->center[j];
              D.dc_corner[j] = ctx->corner[j];
            }
          D.dc_len = ctx->dlen;
        }
      const double fac = 1.0 / D.dc_len * (double) (1ULL << GHIP_BITS);
      for(int j = 0; j < 3; j++)
        if(!dc_inside(xmin[j], D.dc_corner[j], fac) || !dc_inside(xmax[j], D.dc_corner[j], fac))
          return ghip_fail(ctx, GHIP_EINVAL, "GHIP_DD_DECOMPOSE: particles reach [%g, %g] along axis %d, outside the "
                           "domain cube [%g, %g) in force: run with find_extent = 1 (or ghip_dd_set_domain)",
                           xmin[j], xmax[j], j, D.dc_corner[j], D.dc_corner[j] + D.dc_len);
      int level = p.level;
      if(level == 0)   // sharded.histogram_level on the global count
        {
          level = 1;
          while(level < 7 && (1ULL << (3 * level)) * 32 < ntot)
            level++;
          while((1LL << (3 * level)) < P_)
            level++;
        }
      int clog = 0;   // ceil(log2 N)
      while((1ULL << clog) < ntot)
        clog++;
      int shift = 0;
      if(p.use_work)
        {
          shift = (bmax - bmin) + 32 + clog - 63;
          shift = shift > 0 ? shift : 0;
        }
      D.dc_level = level;
      D.dc_bmax = bmax;
      D.dc_shift = shift;
      const int ncell = 1 << (3 * level);
      GCHK(ghip_ensure(ctx, D.dc_hist, (size_t) ncell * 8));
      HIPCHK(hipMemsetAsync(D.dc_hist.p, 0, (size_t) ncell * 8, st));
      if(n > 0)
        {
          // (few, long-lived workgroups: the LDS form pays its flush once per workgroup)
          int nb = cdiv(n, 256 * 16);
          nb = nb < 1024 ? nb : 1024;
          unsigned long long *h = P<unsigned long long>(D.dc_hist);
          if(level <= DC_LDS_LEVEL)
            k_decomp_hist<true><<<nb, 256, (size_t) ncell * 8, st>>>(
              n, x, x + n, x + 2 * (size_t) n, D.dc_corner[0], D.dc_corner[1], D.dc_corner[2], fac, level,
              ncell, p.use_work, cost, tbin, bmax, shift, h);
          else
            k_decomp_hist<false><<<nb, 256, 0, st>>>(
              n, x, x + n, x + 2 * (size_t) n, D.dc_corner[0], D.dc_corner[1], D.dc_corner[2], fac, level,
              ncell, p.use_work, cost, tbin, bmax, shift, h);
          HIPCHK(hipGetLastError());
        }
      ghip_dd_set_allgather(D, D.dc_hist.p, (size_t) ncell * 8, &D.dc_hist_all);
      D.phase = CUT;
      return 1;
    }
  if(D.phase == CUT)
    {
      const int level = D.dc_level, ncell = 1 << (3 * level);
      k_decomp_sum<<<cdiv(ncell, 256), 256, 0, st>>>(ncell, P_, P<unsigned long long>(D.dc_hist_all),
                                                     P<unsigned long long>(D.dc_hist));
      HIPCHK(hipGetLastError());
      std::vector<unsigned long long> sum((size_t) ncell);
      HIPCHK(hipMemcpyAsync(sum.data(), D.dc_hist.p, (size_t) ncell * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      std::vector<double> work((size_t) ncell);
      for(int c = 0; c < ncell; c++)
        work[c] = (double) sum[c];
      std::vector<int> start(P_), end(P_);
      if(ghip_dd_find_split(P_, ncell, work.data(), start.data(), end.data()) != GHIP_OK)
        return ghip_fail(ctx, GHIP_EINVAL, "GHIP_DD_DECOMPOSE: %d cells cannot be cut into %d ranges", ncell, P_);
      unsigned long long splits[GHIP_MAXRANKS + 1];
      for(int r = 0; r < P_; r++)
        splits[r] = (unsigned long long) start[r] << (63 - 3 * level);
      splits[0] = 0;
      splits[P_] = 1ULL << 63;
      GCHK(ghip_dd_set_splits(ctx, splits));
      if(p.find_extent)
        for(int j = 0; j < 3; j++)
          {
            ctx->corner[j] = D.dc_corner[j];
            ctx->center[j] = D.dc_center[j];
          }
      if(p.find_extent)
        ctx->dlen = D.dc_len;
      ctx->gt.built = false;
      ctx->st.built = false;
      D.geom_kept = false;
      ctx->pot_n = -1;
      return 0;
    }
  return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_step: the decomposition has no phase %d", D.phase);
}
