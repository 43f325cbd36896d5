// ghip_ngb.h -- the reference's neighbour-search rules, once: the periodic box, the nearest-image
// wrap, the node test of ngb_treefind_*, the gas-tree node record, the cubic-spline kernel and its
// constants, and two walkers over a pre-order element list.  Included by every file that searches
// neighbours (ghip_sph.hip, ghip_sink.hip, ghip_dust.hip, ghip_dd.hip) or needs the constants
// (ghip_sfr.hip).  The walkers serve the passes with few or cheap targets.  The hot SPH kernels use the
// primitives under a loop of their own: k_density and k_hydro share the staged bucket sweep
// d_sph_sweep of ghip_sph.hip (it stays there, next to the LDS staging, the bucket cull and the
// candidate slots it is made of); k_ngb_find is one thread with a per-candidate distance.
#ifndef GHIP_NGB_H
#define GHIP_NGB_H

#include "ghip_internal.h"

// allvars.h:247-253 (the 3D cubic spline)
#define KERNEL_COEFF_1 2.546479089470
#define KERNEL_COEFF_2 15.278874536822
#define KERNEL_COEFF_3 45.836623610466
#define KERNEL_COEFF_4 30.557749073644
#define KERNEL_COEFF_5 5.092958178941
#define KERNEL_COEFF_6 (-15.278874536822)
#define NORM_COEFF 4.188790204786
#define NUMDIMS 3
#define FACT1 0.366025403785  // allvars.h:310
#define GAMMA (7. / 5.)  // allvars.h:64 (this fork: 7/5, not 5/3; token for token as in ghip_timefac.h)
#define GAMMA_MINUS1 (GAMMA - 1)
#define PROTONMASS 1.6726e-24  // allvars.h:89
#define BOLTZMANN 1.3806e-16   // allvars.h:84

struct BoxK
{
  double boxsize, boxhalf;
  int periodic;
};

static inline BoxK make_box(double boxsize, int periodic)
{
  BoxK b = {boxsize, 0.5 * boxsize, periodic};
  return b;
}

// node test of ngb_treefind_* (ngb.c:276-289 / 136-151, blackhole.c:1453-1466, dust.c:1303-1313):
// true if the node (centre c.xyz, side c.w) must be opened for the search sphere `dist` around p
__device__ __forceinline__ bool d_node_overlaps(const double4 c, double dist, double px, double py,
                                                double pz, const BoxK b)
{
  const double len = c.w;
  dist += 0.5 * len;
  double dx = d_ngb_periodic(c.x - px, b.periodic, b.boxsize, b.boxhalf);
  if(dx > dist)
    return false;
  double dy = d_ngb_periodic(c.y - py, b.periodic, b.boxsize, b.boxhalf);
  if(dy > dist)
    return false;
  double dz = d_ngb_periodic(c.z - pz, b.periodic, b.boxsize, b.boxhalf);
  if(dz > dist)
    return false;
  dist += FACT1 * len;
  return !(dx * dx + dy * dy + dz * dz > dist * dist);
}

__device__ __forceinline__ double d_wrap(double d, const BoxK b)
{
  // density.c:838-851 / hydra.c:1251-1264: d > boxhalf -> d - box, d < -boxhalf -> d + box.
  // Written as one compare on |d| and a subtraction of copysign(box, d) under the execution mask
  // (the same IEEE operations; 2 vector instructions per axis in the common no-wrap case, the
  // empty asm keeps the compiler from turning it back into compare+select chains).
  // For |d| < 1.5 * boxsize this is operation for operation the reference's two-`if` form (which
  // could wrap twice only beyond that), and every difference the callers form is between two
  // coordinates inside the box or one box length apart.
  if(b.periodic)
    {
      if(fabs(d) > b.boxhalf)
        {
          d -= copysign(b.boxsize, d);
          asm volatile("" : "+v"(d));
        }
    }
  return d;
}

// the kernel weight W(u = r / h) * hinv3 of density.c:853-871 and its copies (blackhole.c, dust.c)
__device__ __forceinline__ double d_spline_wk(double u, double hinv3)
{
  if(u < 0.5)
    return hinv3 * (KERNEL_COEFF_1 + KERNEL_COEFF_2 * (u - 1) * u * u);
  return hinv3 * KERNEL_COEFF_5 * (1.0 - u) * (1.0 - u) * (1.0 - u);
}

// One element of the gas tree as the SPH walks read it (64 B, one s_load_dwordx16):
//   cx, cy, cz, len | hmax | skip, pidx, pstart, pcount | pad
struct __attribute__((aligned(64))) SphNode
{
  double cx, cy, cz, len;
  double hmax;
  int skip, pidx, pstart, pcount;
  int pad[2];
};
typedef int v16i_s __attribute__((ext_vector_type(16)));

__device__ __forceinline__ double d_f64s(const v16i_s &v, int i)
{
  return __hiloint2double(v[2 * i + 1], v[2 * i]);
}

__device__ __forceinline__ void d_load_sphnode(const SphNode *__restrict__ base, int e, v16i_s &R)
{
  unsigned long long a = reinterpret_cast<unsigned long long>(base + e);
  unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int) a);
  unsigned int hi = __builtin_amdgcn_readfirstlane((unsigned int) (a >> 32));
  const SphNode *p = reinterpret_cast<const SphNode *>(((unsigned long long) hi << 32) | lo);
  asm volatile("s_load_dwordx16 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(R) : "s"(p) : "memory");
}

// ---------------------------------------------------------------------------------------------
// walkers over a pre-order element list.  An accessor E yields for element e
//   link(e)   x = skip (the element after this subtree), y = sorted particle index of a particle
//             element or < 0 for a node, z = first particle of the node, w = their number
//   cell(e)   centre and side of a node (read for nodes only)
// A node the search sphere (p, h) overlaps is descended, or, with at most LEAF particles, swept flat
// (its particles are contiguous in sorted order); the callback applies the exact distance test.
// ---------------------------------------------------------------------------------------------
struct GravElems   // the gravity tree (all particle types): link and cell arrays
{
  const int4 *__restrict__ lk;
  const double4 *__restrict__ cl;
  __device__ __forceinline__ int4 link(int e) const { return lk[e]; }
  __device__ __forceinline__ double4 cell(int e) const { return cl[e]; }
};

struct GasElems   // the gas tree: SphNode records
{
  const SphNode *__restrict__ nodes;
  __device__ __forceinline__ int4 link(int e) const
  {
    const SphNode &N = nodes[e];
    return make_int4(N.skip, N.pidx, N.pstart, N.pcount);
  }
  __device__ __forceinline__ double4 cell(int e) const
  {
    const SphNode &N = nodes[e];
    return make_double4(N.cx, N.cy, N.cz, N.len);
  }
};

// one thread per centre: f(p) for every candidate p (sorted index) the node tests let through
template <int LEAF, class E, class F>
__device__ __forceinline__ void d_ngb_walk_thread(const E el, int nelem, double px, double py, double pz,
                                                  double h, const BoxK b, F &&f)
{
  int e = 0;
  while(e < nelem)
    {
      const int4 k = el.link(e);
      if(k.y >= 0)
        {
          f(k.y);
          e = e + 1;
          continue;
        }
      // a node: skipped when the sphere misses it, descended when it is large, else swept flat
      const bool open = d_node_overlaps(el.cell(e), h, px, py, pz, b);
      if(open && k.w <= LEAF)
        for(int p = k.z; p < k.z + k.w; p++)
          f(p);
      e = (open && k.w > LEAF) ? e + 1 : k.x;
    }
}

// one wavefront (= one workgroup of 64) per centre, wave-uniform element index: f(p, valid) is called
// by all 64 lanes with the lane's own candidate p of a flat 64-wide sweep
template <int LEAF, class E, class F>
__device__ __forceinline__ void d_ngb_walk_wave(const E el, int nelem, double px, double py, double pz,
                                                double h, const BoxK b, F &&f)
{
  const int lane = threadIdx.x;
  int e = 0;
  while(e < nelem)
    {
      const int4 k = el.link(e);
      int first = k.y, count = 1, next = e + 1;   // a particle element
      if(k.y < 0)   // a node: skipped, descended or swept flat as above
        {
          const bool open = d_node_overlaps(el.cell(e), h, px, py, pz, b);
          first = k.z;
          count = (open && k.w <= LEAF) ? k.w : 0;
          next = (open && k.w > LEAF) ? e + 1 : k.x;
        }
      e = next;
      for(int p0 = first; p0 < first + count; p0 += 64)
        f(p0 + lane, p0 + lane < first + count);
    }
}

#endif
