// ghip_pairs.h -- the ordered "seeker to gas" pair scatter, once: the seekers of a list (dust
// grains, wind particles) find their gas neighbours by a walk of the gas tree, one thread per seeker; the pairs are
// counted, scanned, written as 64-bit keys (gas j << 32 | seeker slot) with their kernel weight, radix sorted, and
// one thread per gas particle applies its run of pairs in slot order.  The slot is the seeker's place in the order
// in which the reference lets a gas particle meet the seekers: the list order for this context's own, behind them
// the imported ones of a shard in receive order.  Which pairs there are and what they weigh is the including file's
// physics, given as a Target; what a gas particle does with its run is the body of that file's apply kernel.
//
// Everything with floating-point arithmetic here is a template or an inline function: it is compiled in the
// including translation unit, under that file's own fp-contract setting (ghip_wind.hip turns contraction off before
// its includes, ghip_dust.hip does not).  The integer-only kernels of a list -- its tree order, its slots by
// particle -- are in ghip_prim.hip (ghip_tree_order, ghip_list_slots).
#ifndef GHIP_PAIRS_H
#define GHIP_PAIRS_H

#include <climits>

#include "ghip_ngb.h"
#include "ghip_prim.h"

#define PAIR_LEAF 16   // a tree node with at most this many particles is swept flat

// The pairs of m targets over the gas tree.  fill == 0: count them into cnt[t]; fill == 1: write
// (j << 32 | slot, W) from off[t] on.  A Target has
//   bool get(t, slot, x, y, z, h, rs)   false: target t has no pairs; else its slot in the keys, its position, its
//                                       radius h and the radius rs <= h of the tree search that meets all its pairs
//   bool pair(j, x, y, z, h, b, W)      whether gas particle j (an index of this context's particles, any value the
//                                       tree holds) and the target are a pair, and the pair's weight
// and holds the arrays of the gas that pair() reads.
template <int fill, class Target>
__global__ void __launch_bounds__(64)
k_pairs(int m, Target T, int nelem, const SphNode *__restrict__ nodes, const int *__restrict__ perm, BoxK b,
        unsigned long long *__restrict__ cnt, const unsigned long long *__restrict__ off, unsigned long long npairs,
        unsigned long long *__restrict__ key, double *__restrict__ wgt)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if(t >= m)
    return;
  int slot;
  double px, py, pz, h, rs;
  unsigned long long c = 0;
  if(T.get(t, slot, px, py, pz, h, rs))
    {
      const unsigned long long o = fill ? off[t] : 0;
      d_ngb_walk_thread<PAIR_LEAF>(GasElems{nodes}, nelem, px, py, pz, rs, b, [&](int p) {
        double W;
        const int j = perm[p];
        if(!T.pair(j, px, py, pz, h, b, W))
          return;
        if(fill)
          {
            if(o + c < npairs)   // (the count of the same walk: never false)
              {
                key[o + c] = ((unsigned long long) j << 32) | (unsigned int) slot;
                wgt[o + c] = W;
              }
          }
        c++;
      });
    }
  if(!fill)
    cnt[t] = c;
}

// the pair buffer for np pairs in a DevBuf of PairBuf::bytes(np): key [np] | key' [np] | W [np] | W' [np]
struct PairBuf
{
  unsigned long long *k0, *k1;
  double *w0, *w1;
  static size_t bytes(size_t np) { return np * 32 + 256; }
  PairBuf(DevBuf &b, size_t np)
  {
    k0 = P<unsigned long long>(b);
    k1 = k0 + np;
    w0 = reinterpret_cast<double *>(k1 + np);
    w1 = w0 + np;
  }
};

// The scatter between the scan and the apply: refuses a pair count outside [0, INT_MAX] (`who` and `what` as in
// "ghip_wind: 5 wind-gas pairs"), makes room in buf, lets fill(PairBuf) launch the k_pairs<1> kernels, and sorts.
// *key, *wgt: the sorted pairs; nullptr where there are none and nothing ran.
template <class Fill>
static int ghip_pairs_fill_sort(ghip_ctx *ctx, DevBuf &buf, long long npairs, const char *who, const char *what,
                                Fill fill, const unsigned long long **key, const double **wgt)
{
  *key = nullptr;
  *wgt = nullptr;
  if(npairs < 0 || npairs > (long long) INT_MAX)
    return ghip_fail(ctx, GHIP_EDEVICE, "%s: %lld %s pairs", who, npairs, what);
  if(npairs == 0)
    return GHIP_OK;
  const size_t np = (size_t) npairs;
  GCHK(ghip_ensure(ctx, buf, PairBuf::bytes(np)));
  const PairBuf pb(buf, np);
  fill(pb);
  HIPCHK(hipGetLastError());
  int end_bit = 33;
  while(end_bit < 64 && (1LL << (end_bit - 32)) <= (long long) ctx->ngas)
    end_bit++;
  GCHK(ghip_sort_pairs(ctx, pb.k0, pb.k1, pb.w0, pb.w1, (int) np, end_bit, ctx->stream));
  *key = pb.k1;
  *wgt = pb.w1;
  return GHIP_OK;
}

// The run of a gas particle in the sorted pairs.  True for the thread whose pair s0 is the first of its gas
// particle j < ngas; that thread then visits its run with d_pair_run: f(slot, W) in slot order.
__device__ __forceinline__ bool d_pair_run_head(long long s0, long long npairs, const unsigned long long *__restrict__ key,
                                                int ngas, unsigned int &j)
{
  if(s0 >= npairs)
    return false;
  j = (unsigned int) (key[s0] >> 32);
  if(s0 > 0 && (unsigned int) (key[s0 - 1] >> 32) == j)
    return false;   // not the first pair of its gas particle
  return j < (unsigned int) ngas;
}

template <class F>
__device__ __forceinline__ void d_pair_run(long long s0, long long npairs, const unsigned long long *__restrict__ key,
                                           const double *__restrict__ wgt, unsigned int j, F &&f)
{
  for(long long s = s0; s < npairs && (unsigned int) (key[s] >> 32) == j; s++)
    f((unsigned int) (key[s] & 0xffffffffULL), wgt[s]);
}

#endif
