// ghip_prim.hip -- device scans, radix sorts and order-preserving selections, what every pass runs before or after
// its own kernels: the library-backed forms, the one-wavefront forms, the rule that gives each stream its scratch,
// and the diagnostic entry that runs one primitive on host arrays.
#include "ghip_prim.h"

#include <hipcub/hipcub.hpp>

DevBuf &ghip_prim_scratch(ghip_ctx *ctx, hipStream_t st)
{
  return st == ctx->stream ? ctx->cubtmp : (st == ctx->stream3 ? ctx->cubtmp3 : ctx->cubtmp2);
}

// library-backed: run(nullptr, bytes) asks for the scratch size, run(block, bytes) does the work
template <class F> static int lib_call(ghip_ctx *ctx, DevBuf &tmp, F run)
{
  size_t tb = 0;
  HIPCHK(run(nullptr, tb));
  GCHK(ghip_ensure(ctx, tmp, tb + 256));
  HIPCHK(run(tmp.p, tb));
  return GHIP_OK;
}

template <class T> int ghip_scan(ghip_ctx *ctx, const T *in, T *out, int n, hipStream_t st, DevBuf *scratch)
{
  return lib_call(ctx, scratch ? *scratch : ghip_prim_scratch(ctx, st),
                  [&](void *t, size_t &tb) { return hipcub::DeviceScan::ExclusiveSum(t, tb, in, out, n, st); });
}
template int ghip_scan<int>(ghip_ctx *, const int *, int *, int, hipStream_t, DevBuf *);
template int ghip_scan<unsigned long long>(ghip_ctx *, const unsigned long long *, unsigned long long *, int,
                                           hipStream_t, DevBuf *);

// Radix sort of (32-bit key, index) pairs on bits [0, end_bit).  Below 2^20 keys the library picks a
// block sort followed by ~19 merge passes (~125 us at 5e5 keys, all dependent ~5 us launches).  Its
// one-sweep radix sort (GHIP_SORT_ONESWEEP=1) needs fewer launches but was measured slower here:
// a histogram pass, its scan, and per 8-bit digit two clears + one 25 us pass = 157 us.
template <class K, class V>
int ghip_sort_pairs(ghip_ctx *ctx, const K *kin, K *kout, const V *vin, V *vout, int n, int end_bit, hipStream_t st)
{
  if constexpr(sizeof(K) == 4)
    {
      static int onesweep = -1;
      if(onesweep < 0)
        onesweep = (getenv("GHIP_SORT_ONESWEEP") && atoi(getenv("GHIP_SORT_ONESWEEP")) == 1) ? 1 : 0;
      if(onesweep && n > 4096)
        {
          using cfg = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                                 rocprim::default_config, 0>;
          return lib_call(ctx, ghip_prim_scratch(ctx, st), [&](void *t, size_t &tb) {
            return rocprim::radix_sort_pairs<cfg>(t, tb, kin, kout, vin, vout, (size_t) n, 0u,
                                                  (unsigned int) end_bit, st);
          });
        }
    }
  return lib_call(ctx, ghip_prim_scratch(ctx, st), [&](void *t, size_t &tb) {
    return hipcub::DeviceRadixSort::SortPairs(t, tb, kin, kout, vin, vout, n, 0, end_bit, st);
  });
}
#define SORT_PAIRS(K, V) \
  template int ghip_sort_pairs<K, V>(ghip_ctx *, const K *, K *, const V *, V *, int, int, hipStream_t)
SORT_PAIRS(unsigned int, int);
SORT_PAIRS(unsigned long long, int);
SORT_PAIRS(unsigned long long, double);

int ghip_sort_keys(ghip_ctx *ctx, const unsigned long long *kin, unsigned long long *kout, int n, int end_bit,
                   hipStream_t st)
{
  return lib_call(ctx, ghip_prim_scratch(ctx, st), [&](void *t, size_t &tb) {
    return hipcub::DeviceRadixSort::SortKeys(t, tb, kin, kout, n, 0, end_bit, st);
  });
}

// sort key of list slot a: the place of its particle in the gravity tree
__global__ void k_list_order_keys(int n, const int *__restrict__ idx, const int *__restrict__ iperm,
                                  unsigned int *__restrict__ key, int *__restrict__ slot)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= n)
    return;
  key[a] = (unsigned int) iperm[idx[a]];
  slot[a] = a;
}

int ghip_tree_order(ghip_ctx *ctx, int n, const int *idx, unsigned int *key, unsigned int *key2, int *slot, int *ord,
                    hipStream_t st)
{
  k_list_order_keys<<<cdiv(n, 256), 256, 0, st>>>(n, idx, P<int>(ctx->gt.iperm), key, slot);
  HIPCHK(hipGetLastError());
  // (sorted positions of a shard's merged tree run up to its local particles + imported elements)
  const long long nsorted = ctx->gt.n > ctx->n ? ctx->gt.n : ctx->n;
  int end_bit = 1;
  while(end_bit < 32 && (1LL << end_bit) <= nsorted)
    end_bit++;
  return ghip_sort_pairs(ctx, key, key2, slot, ord, n, end_bit, st);
}

__global__ void k_list_slots(int n, const int *__restrict__ idx, int *__restrict__ slot)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a < n)
    slot[idx[a]] = a;
}

int ghip_list_slots(ghip_ctx *ctx, int n, const int *idx, int *slot, hipStream_t st)
{
  k_list_slots<<<cdiv(n, 256), 256, 0, st>>>(n, idx, slot);
  HIPCHK(hipGetLastError());
  return GHIP_OK;
}

int ghip_select_flagged(ghip_ctx *ctx, const int *in, const int *flags, int *out, int *dcount, int n, hipStream_t st)
{
  auto from = [&](auto src) {
    return lib_call(ctx, ghip_prim_scratch(ctx, st), [&](void *t, size_t &tb) {
      return hipcub::DeviceSelect::Flagged(t, tb, src, flags, out, dcount, n, st);
    });
  };
  return in ? from(in) : from(hipcub::CountingInputIterator<int>(0));
}

// One-wavefront forms, for what runs underneath a gravity pair -- the tree build's scans on the main
// stream, the density h-iterations' selection of the targets that are not yet converged.  The library's
// single-pass scan and select use 256-thread workgroups (the select's look-back needs them to make
// progress in order), and a 256-thread workgroup waits, for milliseconds, behind the walks for four free
// wavefront slots on one CU (see ghip_wg).  A workgroup of one wavefront takes the first slot that frees.
// Each form is three small launches over blocks of PRIM_BLOCK items: per-block sums or counts, their
// offsets by one wavefront per row (k_block_offsets), the blocks' local scan or scatter.
__global__ void __launch_bounds__(64) k_wscan_sums(int n, const int *__restrict__ in, int *__restrict__ bsum)
{
  const int base = blockIdx.x * PRIM_BLOCK + threadIdx.x * PRIM_ITEMS;
  int c = 0;
  for(int j = 0; j < PRIM_ITEMS; j++)
    c += (base + j < n) ? in[base + j] : 0;
  for(int o = 32; o > 0; o >>= 1)
    c += __shfl_down(c, o, 64);
  if(threadIdx.x == 0)
    bsum[blockIdx.x] = c;
}

static __device__ int d_wave_inclusive(int c)   // sum of c over the lanes up to and including this one
{
  for(int o = 1; o < 64; o <<= 1)
    {
      const int v = __shfl_up(c, o, 64);
      if((int) threadIdx.x >= o)
        c += v;
    }
  return c;
}

// counts -> exclusive offsets (in place), row blockIdx.x of nblk counts; its sum -> total[row] if asked for
__global__ void __launch_bounds__(64) k_block_offsets(int nblk, int *__restrict__ cnt, int *__restrict__ total)
{
  int *row = cnt + (size_t) blockIdx.x * nblk;
  int run = 0;
  for(int b0 = 0; b0 < nblk; b0 += 64)
    {
      const int b = b0 + threadIdx.x;
      const int c = b < nblk ? row[b] : 0;
      const int incl = d_wave_inclusive(c);
      if(b < nblk)
        row[b] = run + incl - c;
      run += __shfl(incl, 63, 64);
    }
  if(total && threadIdx.x == 0)
    total[blockIdx.x] = run;
}

__global__ void __launch_bounds__(64) k_wscan_apply(int n, const int *__restrict__ in,
                                                    const int *__restrict__ boff, int *__restrict__ out)
{
  const int base = blockIdx.x * PRIM_BLOCK + threadIdx.x * PRIM_ITEMS;
  int v[PRIM_ITEMS], c = 0;
  for(int j = 0; j < PRIM_ITEMS; j++)
    {
      v[j] = (base + j < n) ? in[base + j] : 0;
      c += v[j];
    }
  int run = boff[blockIdx.x] + d_wave_inclusive(c) - c;
  for(int j = 0; j < PRIM_ITEMS; j++)
    {
      if(base + j < n)
        out[base + j] = run;
      run += v[j];
    }
}

__global__ void __launch_bounds__(64) k_sel_count(int n, const int *__restrict__ flags, int *__restrict__ blockcnt)
{
  const int base = blockIdx.x * PRIM_BLOCK;
  int c = 0;
  for(int j = 0; j < PRIM_ITEMS; j++)
    {
      const int a = base + j * 64 + threadIdx.x;
      c += (a < n && flags[a] != 0) ? 1 : 0;
    }
  for(int o = 32; o > 0; o >>= 1)
    c += __shfl_down(c, o, 64);
  if(threadIdx.x == 0)
    blockcnt[blockIdx.x] = c;
}

__global__ void __launch_bounds__(64) k_sel_scatter(int n, const int *__restrict__ in, const int *__restrict__ flags,
                                                    const int *__restrict__ blockoff, int *__restrict__ out)
{
  const int base = blockIdx.x * PRIM_BLOCK;
  int off = blockoff[blockIdx.x];
  const unsigned long long below = (1ull << threadIdx.x) - 1ull;
  for(int j = 0; j < PRIM_ITEMS; j++)
    {
      const int a = base + j * 64 + threadIdx.x;
      const bool keep = a < n && flags[a] != 0;
      const unsigned long long m = __ballot(keep);
      if(keep)
        out[off + __popcll(m & below)] = in[a];
      off += __popcll(m);
    }
}

int ghip_block_offsets(ghip_ctx *ctx, int rows, int nblk, int *cnt, int *total, hipStream_t st)
{
  k_block_offsets<<<rows, 64, 0, st>>>(nblk, cnt, total);
  HIPCHK(hipGetLastError());
  return GHIP_OK;
}

int ghip_wscan_i32(ghip_ctx *ctx, const int *in, int *out, int n, hipStream_t st)
{
  const int nblk = cdiv(n, PRIM_BLOCK);
  DevBuf &tmp = ghip_prim_scratch(ctx, st);
  GCHK(ghip_ensure(ctx, tmp, (size_t) (nblk + 2) * 4));
  int *bsum = P<int>(tmp);
  k_wscan_sums<<<nblk, 64, 0, st>>>(n, in, bsum);
  k_block_offsets<<<1, 64, 0, st>>>(nblk, bsum, nullptr);
  k_wscan_apply<<<nblk, 64, 0, st>>>(n, in, bsum, out);
  HIPCHK(hipGetLastError());
  return GHIP_OK;
}

int ghip_scan_i32_under_pair(ghip_ctx *ctx, const int *in, int *out, int n, hipStream_t st)
{
  return ctx->grav_pending && st == ctx->stream ? ghip_wscan_i32(ctx, in, out, n, st) : ghip_scan(ctx, in, out, n, st);
}

int ghip_wsel_count(ghip_ctx *ctx, int n, const int *flags, int *blockoff, int *total, hipStream_t st)
{
  k_sel_count<<<cdiv(n, PRIM_BLOCK), 64, 0, st>>>(n, flags, blockoff);
  return ghip_block_offsets(ctx, 1, cdiv(n, PRIM_BLOCK), blockoff, total, st);
}

int ghip_wsel_scatter(ghip_ctx *ctx, int n, const int *in, const int *flags, const int *blockoff, int *out,
                      hipStream_t st)
{
  k_sel_scatter<<<cdiv(n, PRIM_BLOCK), 64, 0, st>>>(n, in, flags, blockoff, out);
  HIPCHK(hipGetLastError());
  return GHIP_OK;
}

// ghip_debug_prim: one primitive on host arrays, on the main stream
extern "C" int ghip_debug_prim(ghip_ctx *ctx, int prim, int n, int end_bit, const int *in, const int *flags,
                               int *out, int *count)
{
  if(ctx)
    GHIP_JOIN(ctx);
  const bool sel = prim == GHIP_PRIM_SELECT || prim == GHIP_PRIM_WSELECT;
  if(!ctx || prim < 0 || prim > GHIP_PRIM_SORT_U32 || n < 1 || !out || (!sel && !in) ||
     (sel && (!flags || !count)) || (prim == GHIP_PRIM_SORT_U32 && (end_bit < 1 || end_bit > 32)))
    return GHIP_EINVAL;
  hipStream_t st = ctx->stream;
  const size_t N = (size_t) n, nblk = (size_t) cdiv(n, PRIM_BLOCK);
  // stage: in [n] | flags, or the sorted keys [n] | the indices 0..n-1 [n] | result [n] | block offsets [nblk] | count
  GCHK(ghip_ensure(ctx, ctx->stage, (4 * N + nblk + 1) * 4));
  int *da = P<int>(ctx->stage), *db = da + N, *didx = db + N, *dres = didx + N, *dblk = dres + N, *dcnt = dblk + nblk;
  std::vector<int> h(3 * N);   // (the indices: the sort's values, and what the one-wavefront selection reads for in == NULL)
  for(size_t a = 0; a < N; a++)
    h[a] = in ? in[a] : 0, h[N + a] = sel ? flags[a] : 0, h[2 * N + a] = (int) a;
  HIPCHK(hipMemcpyAsync(da, h.data(), 3 * N * 4, hipMemcpyHostToDevice, st));
  if(prim == GHIP_PRIM_SCAN)
    GCHK(ghip_scan(ctx, da, dres, n, st));
  else if(prim == GHIP_PRIM_WSCAN)
    GCHK(ghip_wscan_i32(ctx, da, dres, n, st));
  else if(prim == GHIP_PRIM_SELECT)
    GCHK(ghip_select_flagged(ctx, in ? da : nullptr, db, dres, dcnt, n, st));
  else if(prim == GHIP_PRIM_WSELECT)
    {
      GCHK(ghip_wsel_count(ctx, n, db, dblk, dcnt, st));
      GCHK(ghip_wsel_scatter(ctx, n, in ? da : didx, db, dblk, dres, st));
    }
  else
    GCHK(ghip_sort_pairs(ctx, reinterpret_cast<unsigned int *>(da), reinterpret_cast<unsigned int *>(db), didx, dres,
                         n, end_bit, st));
  int nout = n;
  if(sel)
    {
      HIPCHK(hipMemcpyAsync(count, dcnt, 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      if((nout = *count) < 0 || nout > n)
        return ghip_fail(ctx, GHIP_EDEVICE, "ghip_debug_prim: %d of %d selected", nout, n);
    }
  if(nout > 0)
    HIPCHK(hipMemcpyAsync(out, dres, (size_t) nout * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  return GHIP_OK;
}
