// ghip_sync.hip -- what run() does between two steps, on the resident fields: the next sync point and the
// active list (find_next_sync_point_and_drift, run.c:190-340, without the drift: ghip_drift stays the caller's
// next call), the list in force read back, and the domain cube of one context (domain_findExtent).
//
//   ghip_timebin_hist      TimeBinCount / TimeBinCountSph (k_timebin_histogram, ghip_kick.hip)  -> 64 words read
//   sync_rule              run.c:199-219, 222, 278-293 on the host: integers only
//   k_sync_count           per block of PRIM_BLOCK particles: how many are in an active bin; how many bins lie
//                          outside [0, TIMEBINS)
//   ghip_block_offsets     counts -> offsets, their sum
//   k_sync_scatter         the indices, ascending, into act_next                                -> 2 words read
// and act_next becomes the context's list when nothing was wrong.  The predicate is a shift and a mask on the
// word the pass reads anyway, so no flag array is made for the selections of ghip_prim.hip.  Four launches, a
// 512-byte and an 8-byte clear, two blocking reads.  On shards (GHIP_DD_DECOMPOSE begun with
// walk = GHIP_SYNC_POINT_FORM) the 32 TimeBinCount words of every rank are all-gathered between the histogram
// and the rule, and one status round follows the selection, so that a bad bin on one rank stops all of them
// before any list is replaced.
#include <cfloat>

#include "ghip_prim.h"

#define SYNC_TIMEBINS 29           // TIMEBINS, allvars.h:39
#define SYNC_TIMEBASE (1 << 29)    // TIMEBASE, allvars.h:40

// One wavefront per workgroup, as the selections of ghip_prim.hip: lane l of round j holds particle
// base + 64 j + l, so a ballot is 64 consecutive particles and the popcount below a lane its rank among them.
// (a bin outside [0, TIMEBINS) selects nothing; the shift is masked so that it stays defined)
__device__ __forceinline__ bool d_sync_active(unsigned int mask, int tb)
{
  return (unsigned int) tb < SYNC_TIMEBINS && ((mask >> (tb & 31)) & 1u);
}

__global__ void __launch_bounds__(64) k_sync_count(int n, unsigned int mask, const int *__restrict__ timebin,
                                                   int *__restrict__ blockcnt, int *__restrict__ nbad)
{
  const int base = blockIdx.x * PRIM_BLOCK;
  int c = 0, bad = 0;
  for(int j = 0; j < PRIM_ITEMS; j++)
    {
      const int a = base + j * 64 + threadIdx.x;
      const int tb = a < n ? timebin[a] : 0;
      c += __popcll(__ballot(a < n && d_sync_active(mask, tb)));
      bad += __popcll(__ballot(a < n && (unsigned int) tb >= SYNC_TIMEBINS));
    }
  if(threadIdx.x == 0)
    {
      blockcnt[blockIdx.x] = c;
      if(bad)
        atomicAdd(nbad, bad);
    }
}

__global__ void __launch_bounds__(64) k_sync_scatter(int n, unsigned int mask, const int *__restrict__ timebin,
                                                     const int *__restrict__ blockoff, int *__restrict__ out)
{
  const int base = blockIdx.x * PRIM_BLOCK;
  int off = blockoff[blockIdx.x];
  const unsigned long long below = (1ull << threadIdx.x) - 1ull;
  for(int j = 0; j < PRIM_ITEMS; j++)
    {
      const int a = base + j * 64 + threadIdx.x;
      const bool keep = a < n && d_sync_active(mask, timebin[a]);
      const unsigned long long m = __ballot(keep);
      if(keep)
        out[off + __popcll(m & below)] = a;   // (off + rank < the sum of the counts <= n: act_next holds n)
      off += __popcll(m);
    }
}

// run.c:199-219 (cnt: the populations of all ranks), :222, :278-293; own: this context's populations
static void sync_rule(const ghip_sync_params &p, const long long cnt[32], const long long own[32], ghip_sync_point *o)
{
  int ti_next = SYNC_TIMEBASE;
  long long ntot = 0;
  for(int b = 0; b < SYNC_TIMEBINS; b++)
    {
      ntot += cnt[b];
      if(!cnt[b])
        continue;
      const int dt_bin = b > 0 ? 1 << b : 0;
      const int ti_bin = b > 0 ? (p.Ti_Current / dt_bin) * dt_bin + dt_bin : p.Ti_Current;
      if(ti_bin < ti_next)
        ti_next = ti_bin;
    }
  o->output_due = (ti_next >= p.Ti_nextoutput && p.Ti_nextoutput >= 0) ? 1 : 0;
  o->TimeBinActive = 0;
  o->NumForceUpdate = o->GlobNumForceUpdate = 0;
  o->Flag_FullStep = 0;
  if(o->output_due)
    {
      o->Ti_next = p.Ti_nextoutput;
      return;
    }
  o->Ti_next = ti_next;
  for(int b = 0; b < SYNC_TIMEBINS; b++)
    if(b == 0 || ti_next % (1 << b) == 0)
      {
        o->TimeBinActive |= 1u << b;
        o->NumForceUpdate += own[b];
        o->GlobNumForceUpdate += cnt[b];
      }
  o->Flag_FullStep = o->GlobNumForceUpdate == ntot ? 1 : 0;
}

static int sync_check_params(ghip_ctx *ctx, const ghip_sync_params *p, const char *who)
{
  if(p->Ti_Current < 0 || p->Ti_Current > SYNC_TIMEBASE)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: Ti_Current %d is outside [0, TIMEBASE = %d]", who, p->Ti_Current,
                     SYNC_TIMEBASE);
  if(ctx->n > 0 && (!ctx->f[GHIP_F_TIMEBIN].p || !ctx->f[GHIP_F_TYPE].p))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: the TIMEBIN and TYPE fields are not set", who);
  return GHIP_OK;
}

// this context's populations, recounted: 64 words on the host
static int sync_counts(ghip_ctx *ctx, ghip_sync_point *o)
{
  unsigned long long hist[64];
  GCHK(ghip_timebin_hist(ctx, hist));
  for(int b = 0; b < 32; b++)
    {
      o->TimeBinCount[b] = (long long) hist[b];
      o->TimeBinCountSph[b] = (long long) hist[32 + b];
    }
  return GHIP_OK;
}

// the particles of the bins of `mask` into act_next; sel[0] = their number, sel[1] = TimeBins outside [0, TIMEBINS)
static int sync_select(ghip_ctx *ctx, unsigned int mask, int sel[2])
{
  sel[0] = sel[1] = 0;
  const int n = ctx->n;
  if(n == 0)
    return GHIP_OK;
  hipStream_t st = ctx->stream;
  const int nblk = cdiv(n, PRIM_BLOCK);
  DevBuf &tmp = ghip_prim_scratch(ctx, st);
  GCHK(ghip_ensure(ctx, tmp, (size_t) nblk * 4));
  GCHK(ghip_ensure(ctx, ctx->act_next, (size_t) n * 4));
  int *dsel = ghip_words(ctx)->sync_sel, *boff = P<int>(tmp);
  const int *tb = P<int>(ctx->f[GHIP_F_TIMEBIN]);
  HIPCHK(hipMemsetAsync(dsel, 0, 8, st));
  k_sync_count<<<nblk, 64, 0, st>>>(n, mask, tb, boff, dsel + 1);
  GCHK(ghip_block_offsets(ctx, 1, nblk, boff, dsel, st));
  k_sync_scatter<<<nblk, 64, 0, st>>>(n, mask, tb, boff, P<int>(ctx->act_next));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(sel, dsel, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  if(sel[0] < 0 || sel[0] > n)
    return ghip_fail(ctx, GHIP_EDEVICE, "the selection of the active particles gave %d of %d", sel[0], n);
  return GHIP_OK;
}

// act_next, with `selected` entries, becomes the list in force
static void sync_commit(ghip_ctx *ctx, int selected)
{
  if(selected == ctx->n)
    ctx->nactive = -1;   // everybody: the state of ghip_set_active(ctx, NULL, 0)
  else
    {
      ctx->act_host_idx.swap(ctx->act_next);
      ctx->nactive = selected;
    }
  ctx->lists_dirty = ctx->gas_list_dirty = true;
}

extern "C" int ghip_find_next_sync_point(ghip_ctx *ctx, const ghip_sync_params *p, ghip_sync_point *out)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !p || !out)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_find_next_sync_point: NULL argument");
  const char *who = "ghip_find_next_sync_point";
  if(ctx->dd.on)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: on a multi-GPU shard begin GHIP_DD_DECOMPOSE with walk = "
                     "GHIP_SYNC_POINT_FORM", who);
  GCHK(sync_check_params(ctx, p, who));
  ghip_sync_point o = {};
  GCHK(sync_counts(ctx, &o));
  sync_rule(*p, o.TimeBinCount, o.TimeBinCount, &o);
  // (an output that is due selects nothing; the pass still runs, for the bins it refuses)
  int sel[2];
  GCHK(sync_select(ctx, o.TimeBinActive, sel));
  if(sel[1])
    return ghip_fail(ctx, GHIP_EINVAL, "%s: %d resident TIMEBIN values lie outside [0, %d]; the active list is "
                     "unchanged", who, sel[1], SYNC_TIMEBINS - 1);
  if(!o.output_due)
    {
      if(sel[0] != o.NumForceUpdate)
        return ghip_fail(ctx, GHIP_EDEVICE, "%s: %d particles selected, the bins hold %lld (run.c:332 \"terrible\")",
                         who, sel[0], o.NumForceUpdate);
      sync_commit(ctx, sel[0]);
    }
  *out = o;
  return ghip_check_device_errors(ctx);
}

extern "C" int ghip_get_active(ghip_ctx *ctx, int *idx, int *nactive)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !nactive)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_get_active: NULL argument");
  const int na = ctx->nactive < 0 ? ctx->n : ctx->nactive;
  *nactive = na;
  if(!idx || na == 0)
    return GHIP_OK;
  if(ctx->nactive < 0)
    {
      for(int a = 0; a < na; a++)
        idx[a] = a;
      return GHIP_OK;
    }
  HIPCHK(hipMemcpyAsync(idx, ctx->act_host_idx.p, (size_t) na * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  return GHIP_OK;
}

extern "C" int ghip_find_extent(ghip_ctx *ctx, double corner[3], double center[3], double *len)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !corner || !center || !len)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_find_extent: NULL argument");
  if(ctx->dd.on)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_find_extent: on a multi-GPU shard GHIP_DD_DECOMPOSE with find_extent = 1 "
                     "finds the cube of all ranks");
  if(ctx->n == 0)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_find_extent: no particle");
  if(!ctx->f[GHIP_F_POS].p)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_find_extent: particle field %d not set", (int) GHIP_F_POS);
  GCHK(ghip_extent_pass(ctx, ctx->dd.dc_own, 0));   // (the block of the shard operations: idle here, dd is off)
  unsigned long long blk[EXTENT_WORDS], ntot;
  HIPCHK(hipMemcpyAsync(blk, ctx->dd.dc_own.p, sizeof(blk), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  double xmin[3], xmax[3];
  int bmin, bmax, bad;
  if(ghip_extent_reduce(blk, 1, xmin, xmax, &ntot, &bmin, &bmax, &bad) & EXTENT_ERR_POS)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_find_extent: a position that is not finite");
  // domain_findExtent, domain.c:1996-2011, operation by operation (as GHIP_DD_DECOMPOSE with find_extent = 1)
  double l = 0;
  for(int j = 0; j < 3; j++)
    if(xmax[j] - xmin[j] > l)
      l = xmax[j] - xmin[j];
  l *= 1.001;
  if(!(l > 0) || !(l <= DBL_MAX))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_find_extent: the extent of the particles has length %g", l);
  for(int j = 0; j < 3; j++)
    {
      center[j] = 0.5 * (xmin[j] + xmax[j]);
      corner[j] = 0.5 * (xmin[j] + xmax[j]) - 0.5 * l;
    }
  *len = l;
  return GHIP_OK;
}

// ---- GHIP_DD_DECOMPOSE with walk = GHIP_SYNC_POINT_FORM (ghip_dd_decomp_begin / _step hand over):
//   COUNT   this shard's populations                                     -> all-gather of 32 TimeBinCount words
//   SELECT  the sums, the rule (the same on every rank), this shard's list into act_next
//                                                                        -> the status round {bad bins, failed}
//   COMMIT  every shard fails if one met a bad bin or failed; else act_next becomes the list ----
int ghip_dd_sync_begin(ghip_ctx *ctx, int, const void *params, int)
{
  GHIP_JOIN(ctx);
  ctx->dd.sp = *reinterpret_cast<const ghip_sync_params *>(params);
  return sync_check_params(ctx, &ctx->dd.sp, "GHIP_SYNC_POINT_FORM");
}

int ghip_dd_sync_step(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  hipStream_t st = ctx->stream;
  const char *who = "GHIP_SYNC_POINT_FORM";
  enum { COUNT, SELECT, COMMIT };
  if(D.phase == COUNT)
    {
      D.sp_cur = ghip_sync_point();
      unsigned long long *dhist = ghip_words(ctx)->timebin_hist;
      if(ctx->n == 0)   // (nothing is counted then: the block that travels is cleared here)
        HIPCHK(hipMemsetAsync(dhist, 0, 64 * 8, st));
      // what goes wrong on this shard alone is held: its peers are inside the same collective, the flag travels
      // with the status round
      ghip_dd_hold(ctx, sync_counts(ctx, &D.sp_cur));
      ghip_dd_set_allgather(D, dhist, 32 * 8, &D.sp_all);
      D.phase = SELECT;
      return 1;
    }
  if(D.phase == SELECT)
    {
      int sel[2] = {0, 0};
      if(D.held.rc == GHIP_OK)
        {
          std::vector<unsigned long long> all((size_t) D.nranks * 32);
          long long cnt[32] = {};
          auto pass = [&]() -> int {
            HIPCHK(hipMemcpyAsync(all.data(), D.sp_all.p, all.size() * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(ghip_stream_sync(ctx, st));
            for(int r = 0; r < D.nranks; r++)
              for(int b = 0; b < 32; b++)
                cnt[b] += (long long) all[(size_t) r * 32 + b];
            sync_rule(D.sp, cnt, D.sp_cur.TimeBinCount, &D.sp_cur);
            return sync_select(ctx, D.sp_cur.TimeBinActive, sel);
          };
          ghip_dd_hold(ctx, pass());
        }
      D.sp_selected = sel[0];
      GCHK(dd_post_status(ctx, (double) sel[1], D.held.rc != GHIP_OK));
      D.phase = COMMIT;
      return 1;
    }
  if(D.phase == COMMIT)
    {
      double all[2 * GHIP_MAXRANKS];
      HIPCHK(hipMemcpyAsync(all, D.status_all.p, (size_t) D.nranks * 16, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      long long nbad = 0;
      int first_bad = -1, first_failed = -1;
      for(int r = 0; r < D.nranks; r++)
        {
          nbad += (long long) all[2 * r];
          if(all[2 * r] != 0 && first_bad < 0)
            first_bad = r;
          if(all[2 * r + 1] != 0 && first_failed < 0)
            first_failed = r;
        }
      if(first_failed >= 0)
        return ghip_dd_raise(ctx, first_failed, "%s: shard %d failed (its own message says why); every shard stops "
                             "here, no active list was changed", who, first_failed);
      if(nbad)
        return ghip_fail(ctx, GHIP_EINVAL, "%s: %lld resident TIMEBIN values lie outside [0, %d] (first on shard %d); "
                         "every shard stops here, no active list was changed", who, nbad, SYNC_TIMEBINS - 1, first_bad);
      if(!D.sp_cur.output_due)
        {
          if(D.sp_selected != D.sp_cur.NumForceUpdate)
            return ghip_fail(ctx, GHIP_EDEVICE, "%s: %d particles selected, the bins hold %lld (run.c:332 \"terrible\")",
                             who, D.sp_selected, D.sp_cur.NumForceUpdate);
          sync_commit(ctx, D.sp_selected);
        }
      D.sp_out = D.sp_cur;
      return 0;
    }
  return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_step: the sync point has no phase %d", D.phase);
}

extern "C" int ghip_dd_get_sync_point(const ghip_ctx *ctx, ghip_sync_point *out)
{
  if(!ctx || !out || !ctx->dd.on)
    return GHIP_EINVAL;
  *out = ctx->dd.sp_out;
  return GHIP_OK;
}
