// ghip_wind.hip -- the wind particles of the reference's shipped flag bundle (-DVIRTUAL -DFB_MOMENTUM): the
// propagation loop of momentum_feedback() with its two neighbour passes.  VIRTUAL_FLY_THORUGH_EMPTY_SPACE,
// VARIABLE_PHOTON_SEARCH_RADIUS and RAD_ACCEL are switches of ghip_wind_params.  The creation of wind particles
// (momentum_feedback.c:70-246) is ghip_wind_spawn (ghip_accretion.hip, next to the sinks that emit them).  Not
// built: fb_particles.c, REAL_EOS, NON_GRAY_RAD_TRANSFER.  The resident form (the wind table, ghip_winds_feedback)
// follows ghip_wind_feedback; the loop on domain-decomposed shards is GHIP_DD_WIND, at the end of this file.
//
// Replaces the particle loops of
//   momentum_feedback, the loop and the elimination   momentum_feedback.c:283-568
//   virtual_density / virtual_evaluate_select         virtual_density.c:79-378, 382-625
//   virtual_spread_momentum / _evaluate_onthespot     virtual_spread_momentum.c:58-308, 310-469
//   ngb_treefind_virtual_active                       virtual_density.c:628-748
//
// Wind particles are many and cheap, so a particle is a THREAD, as a grain is (ghip_dust.hip).  The list is
// ordered once per call by the particles' place in the gravity tree (a radix sort of the tree's inverse
// permutation), so that the 64 lanes of a wavefront walk neighbouring parts of the gas tree; the active list of
// every iteration is an order-preserving selection of that order.  It is NOT re-ordered inside the loop: a
// particle moves at most 0.2 Hsml per iteration, which is less than the width of the leaves its lanes share,
// and a re-sort would cost a sort per iteration, about what the density pass costs.
//
// The scatter into the gas is the ordered pair scatter of ghip_pairs.h: the pairs are counted in
// the density pass; this file gives the scatter the wind-gas pair (WindOwn, WindImp) and what a gas particle adds
// from its run (k_wind_apply).  No floating-point atomics; every sum is a per-thread loop in a fixed order: two
// identical calls give identical bits, whatever the launch order of the list.
//
// ONE DELIBERATE DEVIATION from the C text (tests/wind_ref.py takes it too): when the time cap of
// momentum_feedback.c:345-346 sets the jump, dt1 = dt_jump exactly and the particle ends the iteration with
// dt_jump = 0.  The reference recomputes dt1 = dr * U / C * FBV (:348) and subtracts it (:371-372); the residue
// of that round trip is 0 or +-1 ulp, and on its sign hangs one more iteration of length ~1e-17.
//
// no a*b+c -> fma contraction in this file (before the headers, so that their inline functions and the templates
// of ghip_pairs.h follow): every comparison below decides with the C text's own roundings.
#pragma clang fp contract(off)

#include <chrono>

#include "ghip_pairs.h"
#include "ghip_rowtable.h"

#define WIND_C 2.9979e10          // allvars.h:86
#define WIND_THOMPSON 6.65245e-25 // allvars.h:91

// per-particle planes of wind_work ([WIND_NPLANES][nw] doubles, list order)
enum
{
  WP_AGE = 0,   // in      StellarAge
  WP_BIRTH,     // in      BirthPhotonEnergy
  WP_OLD,       // in/out  OldPhotonMomentum
  WP_RHO,       // in/out  NewDensity
  WP_DRMIN,     // in/out  b1.BH_Density
  WP_DT1,       // out
  WP_DT2,       // out
  WP_DTJ,       // out     DtJump
  WP_DMOM,      // out     DeltaPhotonMomentum
  WP_VX,        // Vel [3] of the particle and |Vel| (virtual_spread_momentum.c:391), gathered once per call
  WP_VY,
  WP_VZ,
  WP_VABS,
  WIND_NPLANES
};
#define WIND_NIN (WP_DRMIN + 1)           // planes uploaded by ghip_wind_feedback
#define WIND_NOUT (WP_DMOM - WP_OLD + 1)  // planes read back: WP_OLD .. WP_DMOM

struct WindK
{
  BoxK b;
  double Time, dt_fac, dt_fac_gas, fbv, uvel, udens, ulength, xsec, vmass, vtime, outer;
  double desngb, ogm, softgas, softgasmax, softbulgemax, psr;
  int fly, varsr;
};

// what the host reads once per iteration
struct WindWords
{
  unsigned long long npairs;   // pairs of this iteration's spread pass
  int npos;                    // listed particles with dt_jump > 0: the passes' list
  int nunder;                  // ... with dt_jump > 1e-40: the reference's NextPhoton list (:446)
  int err;                     // a listed particle is not Type 3
  int pad;
  double dt_total;
  unsigned long long hmax;     // bits of the largest Hsml of the gas with Mass > 0 (+inf if one is not > 0 and finite)
};

// The largest h_j of the gas that can be anybody's neighbour, once per call (the gas does not change inside the
// loop).  A pair contributes to a density or receives momentum only where r < h_j <= hmax, so those walks search
// min(Hsml, hmax) instead of the wind particle's own Hsml, which momentum_feedback.c:400 makes three times the
// radius of DesNumNgb neighbours: two orders of magnitude fewer candidates, the same pairs in the same order.
// (The bit patterns of positive doubles order like unsigned integers: an integer atomic, exact.)
__global__ void k_wind_hmax(int ngas, const double *__restrict__ hsml, const double *__restrict__ mass,
                            const int *__restrict__ type, WindWords *words)
{
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long b = 0;
  if(j < ngas && type[j] == 0 && mass[j] > 0)
    {
      const double h = hsml[j];
      b = (h > 0 && h < 1.e300) ? (unsigned long long) __double_as_longlong(h) : 0x7ff0000000000000ULL;
    }
  for(int o = 32; o > 0; o >>= 1)
    {
      const unsigned long long x = __shfl_down(b, o, 64);
      b = x > b ? x : b;
    }
  if((threadIdx.x & 63) == 0 && b)
    atomicMax(&words->hmax, b);
}

// the velocity planes of the list; a particle that is not Type 3 raises words->err
__global__ void k_wind_vel(int nw, const int *__restrict__ idx, int n, const int *__restrict__ type,
                           const double *__restrict__ vel, double *__restrict__ w, WindWords *words)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nw)
    return;
  const int i = idx[a];
  const size_t N = (size_t) n, D = (size_t) nw;
  if(type[i] != 3)
    atomicMax(&words->err, 1);
  const double v0 = vel[i], v1 = vel[N + i], v2 = vel[2 * N + i];
  w[WP_VX * D + a] = v0;
  w[WP_VY * D + a] = v1;
  w[WP_VZ * D + a] = v2;
  w[WP_VABS * D + a] = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
}

// momentum_feedback.c:285-293
__global__ void k_wind_init(int nw, const int *__restrict__ idx, const int *__restrict__ timebin,
                            double *__restrict__ w, int *__restrict__ deleted, double dt_fac)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nw)
    return;
  const size_t D = (size_t) nw;
  const int tb = timebin[idx[a]] & 31;
  w[WP_DTJ * D + a] = (tb ? (double) (1 << tb) : 0.0) * dt_fac;
  w[WP_DT1 * D + a] = 0.;
  w[WP_DT2 * D + a] = 0.;
  w[WP_DMOM * D + a] = 0.;
  deleted[a] = 0;
}

// sum of x[0, nw) in a fixed order: thread t adds x[t], x[t + 1024], ...; then a tree over the threads
__global__ void __launch_bounds__(1024) k_wind_sum(int nw, const double *__restrict__ x, double *__restrict__ out)
{
  __shared__ double s[1024];
  double c = 0;
  for(int a = threadIdx.x; a < nw; a += 1024)
    c += x[a];
  s[threadIdx.x] = c;
  __syncthreads();
  for(unsigned int o = 512; o > 0; o >>= 1)
    {
      if(threadIdx.x < o)
        s[threadIdx.x] += s[threadIdx.x + o];
      __syncthreads();
    }
  if(threadIdx.x == 0)
    *out = s[0];
}

// flags[t] = the t-th particle of the list has dt_jump > 0; counts those above 1e-40 (:446)
__global__ void __launch_bounds__(256) k_wind_flags(int m, const int *__restrict__ list, const double *__restrict__ dtj,
                                                    int *__restrict__ flags, WindWords *words)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  bool under = false;
  if(t < m)
    {
      const double d = dtj[list[t]];
      flags[t] = d > 0.;
      under = d > 1.e-40;
    }
  const unsigned long long bal = __ballot(under);
  if((threadIdx.x & 63) == 0 && bal)
    atomicAdd(&words->nunder, __popcll(bal));
}

__global__ void k_wind_reset(int nw, double *__restrict__ w)   // virtual_density.c:107-127
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nw)
    return;
  w[(size_t) WP_RHO * nw + a] = 0.;
  w[(size_t) WP_DRMIN * nw + a] = 1.e40;
}

// The gas side of a wind-gas pair, and the base of the two targets below.  near(): one candidate of
// ngb_treefind_virtual_active (virtual_density.c:650-664) and the pair geometry of virtual_evaluate_select
// (:495-524): a gas particle of this context with Mass > 0 within the wind particle's own h; r and the gas
// particle's h_j and mass come back.  The nearest image is the text's two comparisons per axis (d_wrap, ghip_ngb.h).
// pair(): the pairs of virtual_evaluate_onthespot (virtual_spread_momentum.c:129-130, 393-419), u = r / h_j < 1,
// with their kernel weight -- what k_pairs (ghip_pairs.h) counts and writes.
struct WindGas
{
  int n, ngas;
  const double *pos, *hsml, *mass;
  const int *type;
  const WindWords *words;
  __device__ __forceinline__ bool near(int j, double px, double py, double pz, double h, const BoxK b, double &r,
                                       double &hj, double &mj) const
  {
    if(j < 0 || j >= ngas || type[j] != 0 || !((mj = mass[j]) > 0))
      return false;
    const double dx = d_wrap(px - pos[j], b), dy = d_wrap(py - pos[(size_t) n + j], b),
                 dz = d_wrap(pz - pos[2 * (size_t) n + j], b);
    const double r2 = dx * dx + dy * dy + dz * dz;
    if(r2 > h * h)
      return false;
    r = sqrt(r2);
    hj = hsml[j];
    return true;
  }
  __device__ __forceinline__ bool pair(int j, double px, double py, double pz, double h, const BoxK b, double &wk) const
  {
    double r, hj, mj;
    if(!near(j, px, py, pz, h, b, r, hj, mj))
      return false;
    const double u = r / hj;
    if(!(u < 1))
      return false;
    const double hinv = 1 / hj;
    wk = d_spline_wk(u, hinv * hinv * hinv);
    return true;
  }
  __device__ __forceinline__ double hmax() const { return __longlong_as_double((long long) words->hmax); }
};

// Where target t of a neighbour pass comes from.  place(): its slot in the pair keys and, where it takes part in a
// density pass, its position and radius.  get(): the same for the spread pass (a Target of k_pairs), which no
// particle with new_density = 0 takes part in; the walk searches min(h, hmax), see k_wind_hmax.  put(): where the
// density pass leaves its two results.
// Own: list slot list[t] of this context's wind particles, position and radius resident at idx[slot], the planes w;
// takes part with dt_jump > 0, and is reset otherwise.
struct WindOwn : WindGas
{
  const int *list, *idx;
  int nw;
  double *w;
  __device__ __forceinline__ bool place(int t, int &slot, double &x, double &y, double &z, double &h) const
  {
    slot = list[t];
    if(!(w[WP_DTJ * (size_t) nw + slot] > 0.))
      return false;
    const int i = idx[slot];
    x = pos[i];
    y = pos[(size_t) n + i];
    z = pos[2 * (size_t) n + i];
    h = hsml[i];
    return true;
  }
  __device__ __forceinline__ bool get(int t, int &slot, double &x, double &y, double &z, double &h, double &rs) const
  {
    if(!(w[WP_RHO * (size_t) nw + list[t]] > 0.) || !place(t, slot, x, y, z, h))
      return false;
    rs = fmin(h, hmax());
    return true;
  }
  __device__ __forceinline__ void put(int, int slot, double rho, double drmin) const
  {
    w[WP_RHO * (size_t) nw + slot] = rho;
    w[WP_DRMIN * (size_t) nw + slot] = drmin;
  }
};

// Imported (GHIP_DD_WIND): record t of another shard's particles, {Pos, Hsml} in rec [4], and for the spread pass
// {NewDensity, DeltaPhotonMomentum, Vel, |Vel|} in srec [6]; its slot in the pair keys is nw + t, behind the own
// ones.  It has dt_jump > 0, or it would not have been sent.  The density pass leaves part[2 t] = the sum,
// part[2 t + 1] = drmin over THIS context's gas.
#define WIND_REC_DENS 4
#define WIND_REC_SPREAD 6
struct WindImp : WindGas
{
  const double *rec, *srec;
  int nw;
  double *part;
  __device__ __forceinline__ bool place(int t, int &slot, double &x, double &y, double &z, double &h) const
  {
    const double *q = rec + WIND_REC_DENS * (size_t) t;
    slot = nw + t;
    x = q[0];
    y = q[1];
    z = q[2];
    h = q[3];
    return true;
  }
  __device__ __forceinline__ bool get(int t, int &slot, double &x, double &y, double &z, double &h, double &rs) const
  {
    if(!(srec[WIND_REC_SPREAD * (size_t) t] > 0.) || !place(t, slot, x, y, z, h))
      return false;
    rs = fmin(h, hmax());
    return true;
  }
  __device__ __forceinline__ void put(int t, int, double rho, double drmin) const
  {
    part[2 * (size_t) t] = rho;
    part[2 * (size_t) t + 1] = drmin;
  }
};

// virtual_evaluate_select for the m targets T (WindOwn or WindImp): those that take part are evaluated, the others
// reset.  cnt != nullptr: cnt[t] = the pairs the spread pass will write for the t-th target (u < 1, and none where
// new_density comes out 0).
template <class Target>
__global__ void __launch_bounds__(64)
k_wind_density(int m, Target T, int nelem, const SphNode *__restrict__ nodes, const int *__restrict__ perm, BoxK b,
               unsigned long long *__restrict__ cnt)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if(t >= m)
    return;
  int slot;
  double px, py, pz, h;
  double rho = 0., drmin = 1.e40;
  unsigned long long c = 0;
  if(T.place(t, slot, px, py, pz, h))
    {
      // every pair with u < 1 has r < h_j <= hmax: this walk meets them all, in the order the walk of the whole
      // sphere h would (its nodes are a subset in the same pre-order)
      const double hmax = T.hmax();
      const double r1 = fmin(h, hmax);
      d_ngb_walk_thread<PAIR_LEAF>(GasElems{nodes}, nelem, px, py, pz, r1, b, [&](int p) {
        double r, hj, mj;
        const int j = perm[p];
        if(!T.near(j, px, py, pz, h, b, r, hj, mj))
          return;
        const double drcheck = fabs(r - hj) + 0.25 * hj;   // :519-520
        if(drcheck < drmin)
          drmin = drcheck;
        const double u = r / hj;
        if(u < 1)
          {
            const double hinv = 1 / hj;
            rho += mj * d_spline_wk(u, hinv * hinv * hinv);
            c++;
          }
      });
      // drmin is a minimum over the whole sphere h.  |r - h_j| + h_j / 4 >= r - 3/4 hmax: beyond
      // r2 = drmin + 3/4 hmax nothing can lower it (a little further, for the roundings of the two sides)
      if(r1 < h)
        {
          const double r2 = fmin(h, (drmin + 0.75 * hmax) * (1. + 1.e-9));
          if(r2 > r1)
            d_ngb_walk_thread<PAIR_LEAF>(GasElems{nodes}, nelem, px, py, pz, r2, b, [&](int p) {
              double r, hj, mj;
              const int j = perm[p];
              if(!T.near(j, px, py, pz, h, b, r, hj, mj))
                return;
              const double drcheck = fabs(r - hj) + 0.25 * hj;
              if(drcheck < drmin)
                drmin = drcheck;
            });
        }
    }
  T.put(t, slot, rho, drmin);
  if(cnt)
    cnt[t] = rho > 0. ? c : 0;
}

// the momentum one gas particle receives from its run of sorted pairs, in slot order: the own wind particles in
// list order, slots [0, nw), from the planes; then the nimp imported ones in receive order, slots nw + t, from
// their spread records (virtual_spread_momentum.c:432, 447-448)
__global__ void k_wind_apply(long long npairs, const unsigned long long *__restrict__ key,
                             const double *__restrict__ wgt, int nw, const double *__restrict__ w, int nimp,
                             const double *__restrict__ srec, const double *__restrict__ mass, int ngas,
                             double *__restrict__ inj)
{
  const long long s0 = (long long) blockIdx.x * blockDim.x + threadIdx.x;
  unsigned int j;
  if(!d_pair_run_head(s0, npairs, key, ngas, j))
    return;
  const size_t D = (size_t) nw, G = (size_t) ngas;
  const double mj = mass[j];
  double i0 = inj[j], i1 = inj[G + j], i2 = inj[2 * G + j];
  d_pair_run(s0, npairs, key, wgt, j, [&](unsigned int a, double wk) {
    if(a >= (unsigned int) nw + (unsigned int) nimp)
      return;
    double rho, dmom, v0, v1, v2, va;
    if(a < (unsigned int) nw)
      {
        rho = w[WP_RHO * D + a];
        dmom = w[WP_DMOM * D + a];
        v0 = w[WP_VX * D + a];
        v1 = w[WP_VY * D + a];
        v2 = w[WP_VZ * D + a];
        va = w[WP_VABS * D + a];
      }
    else
      {
        const double *q = srec + WIND_REC_SPREAD * (size_t) (a - (unsigned int) nw);
        rho = q[0];
        dmom = q[1];
        v0 = q[2];
        v1 = q[3];
        v2 = q[4];
        va = q[5];
      }
    const double ddpm = dmom * mj * wk / rho;
    i0 += ddpm * v0 / va;
    i1 += ddpm * v1 / va;
    i2 += ddpm * v2 / va;
  });
  inj[j] = i0;
  inj[G + j] = i1;
  inj[2 * G + j] = i2;
}

// momentum_feedback.c:312-427 for the m particles of the list (all have dt_jump > 0; the reference's own list
// holds those above 1e-40)
__global__ void k_wind_move(int m, const int *__restrict__ list, const int *__restrict__ idx, int n,
                            double *__restrict__ pos, double *__restrict__ hsml, double *__restrict__ mass, int nw,
                            double *__restrict__ w, WindK K)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if(t >= m)
    return;
  const int a = list[t];
  const size_t D = (size_t) nw, N = (size_t) n;
#define PL(q) w[(size_t) (q) * D + a]
  double dt_bh = PL(WP_DTJ);
  if(!(dt_bh > 1.e-40))
    return;
  const int i = idx[a];
  const double newdens = PL(WP_RHO);
  double h = hsml[i];
  double desired_dr = 0.2 * h;
  if(K.fly)   // :337-340
    {
      const double lim = 0.5 * PL(WP_DRMIN) + 2. * K.softgas;
      if(desired_dr > lim)
        desired_dr = lim;
    }
  const double cap = WIND_C * dt_bh / K.uvel / K.fbv;   // :345-346
  const bool capped = desired_dr > cap;
  if(capped)
    desired_dr = cap;
  // :348, and the deviation: the capped jump takes all the time that is left
  double dt1 = capped ? dt_bh : desired_dr * K.uvel / WIND_C * K.fbv;
  const double dtau_max = 10. * desired_dr / h;
  double dtau = K.xsec * WIND_THOMPSON / PROTONMASS * newdens * desired_dr * K.udens * K.ulength;
  if(dtau > dtau_max)
    dtau = dtau_max;
  double old = PL(WP_OLD);
  const double dmom = old * (1. - exp(-dtau));
  old -= dmom;
  PL(WP_DMOM) = dmom;
  PL(WP_OLD) = old;
  mass[i] = K.vmass * old;
  double x[3];
  for(int k = 0; k < 3; k++)
    {
      x[k] = pos[k * N + i] + dt1 * PL(WP_VX + k);
      pos[k * N + i] = x[k];
    }
  double dtj = capped ? 0. : dt_bh - dt1;
  double dt2 = PL(WP_DT2) + dt1;
  if(K.b.periodic)   // :382-395
    for(int k = 0; k < 3; k++)
      {
        if(x[k] > K.b.boxhalf)
          x[k] -= K.b.boxsize;
        if(x[k] < -K.b.boxhalf)
          x[k] += K.b.boxsize;
      }
  const double r2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
  if(newdens > 0)   // :398-405
    h = 3. * pow((K.desngb * K.ogm / (newdens + 1.e-38)), 0.33333) + K.softgasmax;
  else
    h *= 1.2;
  if(K.varsr)   // :409-410
    {
      const double lim = K.psr * sqrt(r2) + K.softbulgemax;
      if(h > lim)
        h = lim;
    }
  hsml[i] = h;
  if(old < 0.01 * PL(WP_BIRTH) / WIND_C * K.uvel)   // :417-424: hide it
    {
      dt2 += dtj;
      dtj = 0.;
      dt1 = 0.;
    }
  PL(WP_DTJ) = dtj;
  PL(WP_DT2) = dt2;
  PL(WP_DT1) = dt1;
#undef PL
}

// momentum_feedback.c:550-568
__global__ void k_wind_eliminate(int nw, const int *__restrict__ idx, int n, const double *__restrict__ pos,
                                 double *__restrict__ mass, const double *__restrict__ w,
                                 int *__restrict__ deleted, WindK K)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nw)
    return;
  const int i = idx[a];
  const size_t D = (size_t) nw, N = (size_t) n;
  int code = 0;
  if(mass[i] != 0.)
    {
      const double x = pos[i], y = pos[N + i], z = pos[2 * N + i];
      const double r = sqrt(x * x + y * y + z * z);
      if(r > K.outer || K.Time - w[WP_AGE * D + a] > K.vtime)
        code = 1;
      else if(w[WP_OLD * D + a] < 0.01 * w[WP_BIRTH * D + a] / WIND_C * K.uvel)
        code = 2;
      if(code)
        mass[i] = 0.;
    }
  deleted[a] = code;
}

// momentum_feedback.c:497-538 for the active gas
__global__ void k_wind_rad_accel(int nact, const int *__restrict__ act, int ngas, const int *__restrict__ type,
                                 const int *__restrict__ timebin, const double *__restrict__ mass,
                                 double *__restrict__ inj, double *__restrict__ ra, double dt_fac_gas)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if(t >= nact)
    return;
  const int i = act ? act[t] : t;
  if(i < 0 || i >= ngas || type[i] != 0)
    return;
  const size_t G = (size_t) ngas;
  const int tb = timebin[i] & 31;
  const double dt = (tb ? (double) (1 << tb) : 0.0) * dt_fac_gas;
  const double m = mass[i];
  double r[3] = {0., 0., 0.};
  if(dt != 0. && m > 0.)
    {
      for(int k = 0; k < 3; k++)
        r[k] = inj[k * G + i] / dt / m;
      const double ac = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
      const double acmax = 1.e4 / dt;
      if(ac >= acmax)
        for(int k = 0; k < 3; k++)
          r[k] *= (acmax / ac);
    }
  for(int k = 0; k < 3; k++)
    {
      ra[k * G + i] = r[k];
      inj[k * G + i] = 0.;
    }
}

__global__ void k_wind_npairs(const unsigned long long *__restrict__ off, int m, WindWords *words)
{
  if(blockIdx.x == 0 && threadIdx.x == 0)
    words->npairs = off[m];
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static WindK wind_k(const ghip_wind_params *p)
{
  WindK K;
  K.b = make_box(p->BoxSize, p->periodic);
  K.Time = p->Time;
  K.dt_fac = p->dt_fac;
  K.dt_fac_gas = p->dt_fac_gas;
  K.fbv = p->FeedBackVelocity;
  K.uvel = p->UnitVelocity_in_cm_per_s;
  K.udens = p->UnitDensity_in_cgs;
  K.ulength = p->UnitLength_in_cm;
  K.xsec = p->VirtualCrosSection;
  K.vmass = p->VirtualMass;
  K.vtime = p->VirtualTime;
  K.outer = p->OuterBoundary;
  K.desngb = p->DesNumNgb;
  K.ogm = p->OriginalGasMass;
  K.softgas = p->SofteningGas;
  K.softgasmax = p->SofteningGasMaxPhys;
  K.softbulgemax = p->SofteningBulgeMaxPhys;
  K.psr = p->PhotonSearchRadius;
  K.fly = p->fly_through_empty_space != 0;
  K.varsr = p->variable_search_radius != 0;
  return K;
}

// A ghip_set_shard context is refused everywhere.  A ghip_dd_init context is refused by the three passes, which
// run there as GHIP_DD_WIND; the resident gas fields and RAD_ACCEL in the integrator are per-particle and serve it
// (dd_ok).
static int wind_refuse_sharded(ghip_ctx *ctx, const char *who, bool dd_ok = false)
{
  if(ctx->shard_n > 1)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: not available on a sharded context (ghip_set_shard): the wind passes "
                     "are single-rank only", who);
  if(ctx->dd.on && !dd_ok)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: not available on a multi-GPU context (ghip_dd_init): this entry point is "
                     "single-rank, shards run GHIP_DD_WIND with walk = GHIP_WIND_FORM (ghip_dd_begin / ghip_dd_run)", who);
  return GHIP_OK;
}

// the device arrays of a call
struct WindDev
{
  int nw;
  int *idx, *ord, *lista, *listb, *flags, *deleted;
  WindWords *words;
  double *w;
  unsigned long long *cnt, *off;
};

static WindDev wind_dev(ghip_ctx *ctx, int nw)
{
  const size_t D = (size_t) nw;
  WindDev d;
  d.nw = nw;
  // wind_idx: idx | ord | key | key' | slot | list A | list B | flags | deleted   ([nw] each)  | WindWords
  d.idx = P<int>(ctx->wind_idx);
  d.ord = d.idx + D;
  d.lista = d.idx + 5 * D;
  d.listb = d.idx + 6 * D;
  d.flags = d.idx + 7 * D;
  d.deleted = d.idx + 8 * D;
  d.words = reinterpret_cast<WindWords *>(reinterpret_cast<char *>(ctx->wind_idx.p) + ((9 * D * 4 + 63) & ~(size_t) 63));
  // wind_work: planes [WIND_NPLANES][nw] | cnt [nw + 1] | off [nw + 1]   (64-bit)
  d.w = P<double>(ctx->wind_work);
  d.cnt = reinterpret_cast<unsigned long long *>(d.w + WIND_NPLANES * D);
  d.off = d.cnt + D + 1;
  return d;
}

// the tree order of the list d.idx into d.ord (key, key', slot: the three words behind them)
static int wind_tree_order(ghip_ctx *ctx, const WindDev &d, hipStream_t st)
{
  const size_t D = (size_t) d.nw;
  unsigned int *key = reinterpret_cast<unsigned int *>(d.idx + 2 * D);
  return ghip_tree_order(ctx, d.nw, d.idx, key, key + D, d.idx + 4 * D, d.ord, st);
}

// What every entry point asks of the context (wind_begin); then the list to the device, its tree order into
// `ord`, the velocity planes, and words->err raised where an index does not name a Type-3 particle
static int wind_need_trees(ghip_ctx *ctx, const char *who)
{
  if(ctx->ngas > 0)
    GCHK(ghip_finish_gas_tree(ctx));
  if(!ctx->gt.built || (ctx->ngas > 0 && !ctx->st.built))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: call ghip_tree_build first", who);
  return GHIP_OK;
}

// the list of nw particles on the device (host == false: device to device)
static int wind_begin_list(ghip_ctx *ctx, int nw, const int *idx, bool host, WindDev *out)
{
  hipStream_t st = ctx->stream;
  const size_t D = (size_t) nw;
  GCHK(ghip_ensure(ctx, ctx->wind_idx, ((9 * D * 4 + 63) & ~(size_t) 63) + 64));
  GCHK(ghip_ensure(ctx, ctx->wind_work, (WIND_NPLANES * D + 2 * (D + 1)) * 8 + 256));
  const WindDev d = wind_dev(ctx, nw);
  *out = d;
  HIPCHK(hipMemcpyAsync(d.idx, idx, D * 4, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemsetAsync(d.words, 0, sizeof(WindWords), st));
  GCHK(wind_tree_order(ctx, d, st));
  k_wind_vel<<<cdiv(nw, 256), 256, 0, st>>>(nw, d.idx, ctx->n, P<int>(ctx->f[GHIP_F_TYPE]),
                                            P<double>(ctx->f[GHIP_F_VEL]), d.w, d.words);
  if(ctx->ngas > 0)
    k_wind_hmax<<<cdiv(ctx->ngas, 256), 256, 0, st>>>(ctx->ngas, P<double>(ctx->f[GHIP_F_HSML]),
                                                      P<double>(ctx->f[GHIP_F_MASS]), P<int>(ctx->f[GHIP_F_TYPE]),
                                                      d.words);
  HIPCHK(hipGetLastError());
  return GHIP_OK;
}

static int wind_begin(ghip_ctx *ctx, const ghip_wind_params *p, int nw, const int *idx, const char *who, WindDev *out)
{
  GCHK(wind_refuse_sharded(ctx, who));
  if(!p || nw < 0 || (nw > 0 && !idx))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: bad arguments", who);
  out->nw = nw;
  if(nw == 0)
    return GHIP_OK;
  GCHK(wind_need_trees(ctx, who));
  for(int a = 0; a < nw; a++)
    if(idx[a] < 0 || idx[a] >= ctx->n)
      return ghip_fail(ctx, GHIP_EINVAL, "%s: wind particle index %d out of range", who, idx[a]);
  return wind_begin_list(ctx, nw, idx, true, out);
}

static int wind_type_error(ghip_ctx *ctx, const char *who)
{
  return ghip_fail(ctx, GHIP_EINVAL, "%s: wind_idx names a particle that is not Type 3", who);
}

// a resident gas field [3][ngas]: made and zeroed at first use, refused when it holds another gas count
static int wind_gas_field(ghip_ctx *ctx, DevBuf &b, int *held, const char *name, const char *setter, const char *who)
{
  const int ng = ctx->ngas;
  if(*held >= 0 && *held != ng)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: %s is held for %d gas particles, the context has %d (%s again)", who,
                     name, *held, ng, setter);
  if(*held < 0)
    {
      const size_t bytes = 3 * (size_t) (ng > 0 ? ng : 1) * 8;
      GCHK(ghip_ensure(ctx, b, bytes));
      HIPCHK(hipMemsetAsync(b.p, 0, bytes, ctx->stream));
      *held = ng;
    }
  return GHIP_OK;
}

static int wind_injected(ghip_ctx *ctx, const char *who)
{
  return wind_gas_field(ctx, ctx->wind_inj, &ctx->wind_inj_ngas, "Injected_BH_Momentum", "ghip_wind_set_injected", who);
}

static int wind_rad_accel(ghip_ctx *ctx, const char *who)
{
  return wind_gas_field(ctx, ctx->wind_ra, &ctx->wind_ra_ngas, "RadAccel", "ghip_wind_set_rad_accel", who);
}

// the resident fields of the gas as the targets take them, and its tree as the kernels do
static WindGas wind_gas(ghip_ctx *ctx, const WindDev &d)
{
  return WindGas{ctx->n, ctx->ngas, P<double>(ctx->f[GHIP_F_POS]), P<double>(ctx->f[GHIP_F_HSML]),
                 P<double>(ctx->f[GHIP_F_MASS]), P<int>(ctx->f[GHIP_F_TYPE]), d.words};
}
#define WIND_TREE_ARGS ctx->ngas > 0 ? ctx->st.nelem : 0, P<SphNode>(ctx->st.mq), P<int>(ctx->st.perm)

// the particles of `list` (slots of this context's list) / the imported records of GHIP_DD_WIND as targets
static WindOwn wind_own(ghip_ctx *ctx, const WindDev &d, const int *list)
{
  return WindOwn{wind_gas(ctx, d), list, d.idx, d.nw, d.w};
}
static WindImp wind_imp(ghip_ctx *ctx, const WindDev &d, const double *rec, const double *srec, double *part)
{
  return WindImp{wind_gas(ctx, d), rec, srec, d.nw, part};
}

// The scatter of the m particles of `list` (cnt[0, m) counted, cnt[m] = 0, scanned into off; npairs = off[m]):
// fill, sort, apply.  GHIP_DD_WIND: behind them the nimp imported records of `imp`, counted and scanned behind the
// own ones (off[m .. m + nimp], npairs = off[m + nimp])
static int wind_scatter(ghip_ctx *ctx, const WindDev &d, const BoxK &b, int m, const int *list, long long npairs,
                        const unsigned long long *off = nullptr, int nimp = 0, const WindImp *imp = nullptr)
{
  if(!off)
    off = d.off;
  hipStream_t st = ctx->stream;
  const unsigned long long *key;
  const double *wgt;
  GCHK(ghip_pairs_fill_sort(ctx, ctx->wind_pairs, npairs, "ghip_wind", "wind-gas", [&](const PairBuf &pb) {
    if(m > 0)
      k_pairs<1><<<cdiv(m, 64), 64, 0, st>>>(m, wind_own(ctx, d, list), WIND_TREE_ARGS, b, nullptr, off,
                                             (unsigned long long) npairs, pb.k0, pb.w0);
    if(nimp > 0)
      k_pairs<1><<<cdiv(nimp, 64), 64, 0, st>>>(nimp, *imp, WIND_TREE_ARGS, b, nullptr, off + m,
                                                (unsigned long long) npairs, pb.k0, pb.w0);
  }, &key, &wgt));
  if(!key)
    return GHIP_OK;
  k_wind_apply<<<cdiv(npairs, 256), 256, 0, st>>>(npairs, key, wgt, d.nw, d.w, nimp, imp ? imp->srec : nullptr,
                                                  P<double>(ctx->f[GHIP_F_MASS]), ctx->ngas, P<double>(ctx->wind_inj));
  HIPCHK(hipGetLastError());
  return GHIP_OK;
}

// host [m][3] <-> device planes [3][m]
static int wind_upload3(ghip_ctx *ctx, DevBuf &b, const double *h, int m)
{
  GCHK(ghip_ensure(ctx, b, 3 * (size_t) (m > 0 ? m : 1) * 8));
  std::vector<double> t(3 * (size_t) m);
  for(int a = 0; a < m; a++)
    for(int j = 0; j < 3; j++)
      t[(size_t) j * m + a] = h[3 * (size_t) a + j];
  if(m > 0)
    HIPCHK(hipMemcpyAsync(b.p, t.data(), t.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  return GHIP_OK;
}

static int wind_download3(ghip_ctx *ctx, const DevBuf &b, double *h, int m)
{
  std::vector<double> t(3 * (size_t) m);
  if(m > 0)
    HIPCHK(hipMemcpyAsync(t.data(), b.p, t.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  for(int a = 0; a < m; a++)
    for(int j = 0; j < 3; j++)
      h[3 * (size_t) a + j] = t[(size_t) j * m + a];
  return GHIP_OK;
}

extern "C" size_t ghip_wind_params_size(void)
{
  return sizeof(ghip_wind_params);
}

extern "C" int ghip_wind_density(ghip_ctx *ctx, const ghip_wind_params *p, int nwind, const int *wind_idx,
                                 const double *dt_jump, double *new_density, double *drmin)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  static const char *who = "ghip_wind_density";
  if(nwind > 0 && (!dt_jump || !new_density || !drmin))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: bad arguments", who);
  WindDev d;
  GCHK(wind_begin(ctx, p, nwind, wind_idx, who, &d));
  if(nwind == 0)
    return GHIP_OK;
  hipStream_t st = ctx->stream;
  const size_t D = (size_t) nwind;
  HIPCHK(hipMemcpyAsync(d.w + WP_DTJ * D, dt_jump, D * 8, hipMemcpyHostToDevice, st));
  k_wind_density<<<cdiv(nwind, 64), 64, 0, st>>>(nwind, wind_own(ctx, d, d.ord), WIND_TREE_ARGS,
                                                 make_box(p->BoxSize, p->periodic), nullptr);
  HIPCHK(hipGetLastError());
  WindWords h;
  HIPCHK(hipMemcpyAsync(&h, d.words, sizeof(h), hipMemcpyDeviceToHost, st));
  // (WP_RHO and WP_DRMIN are neighbours)
  std::vector<double> o(2 * D);
  HIPCHK(hipMemcpyAsync(o.data(), d.w + WP_RHO * D, 2 * D * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  if(h.err)
    return wind_type_error(ctx, who);
  memcpy(new_density, o.data(), D * 8);
  memcpy(drmin, o.data() + D, D * 8);
  return GHIP_OK;
}

extern "C" int ghip_wind_spread(ghip_ctx *ctx, const ghip_wind_params *p, int nwind, const int *wind_idx,
                                const double *dt_jump, const double *new_density, const double *delta_momentum)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  static const char *who = "ghip_wind_spread";
  if(nwind > 0 && (!dt_jump || !new_density || !delta_momentum))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: bad arguments", who);
  WindDev d;
  GCHK(wind_begin(ctx, p, nwind, wind_idx, who, &d));
  GCHK(wind_injected(ctx, who));
  if(nwind == 0)
    return GHIP_OK;
  hipStream_t st = ctx->stream;
  const size_t D = (size_t) nwind;
  const BoxK b = make_box(p->BoxSize, p->periodic);
  HIPCHK(hipMemcpyAsync(d.w + WP_DTJ * D, dt_jump, D * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d.w + WP_RHO * D, new_density, D * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d.w + WP_DMOM * D, delta_momentum, D * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(d.cnt, 0, (D + 1) * 8, st));
  k_pairs<0><<<cdiv(nwind, 64), 64, 0, st>>>(nwind, wind_own(ctx, d, d.ord), WIND_TREE_ARGS, b, d.cnt, nullptr, 0ULL,
                                             nullptr, nullptr);
  HIPCHK(hipGetLastError());
  GCHK(ghip_scan<unsigned long long>(ctx, d.cnt, d.off, nwind + 1, st));
  k_wind_npairs<<<1, 64, 0, st>>>(d.off, nwind, d.words);
  HIPCHK(hipGetLastError());
  WindWords h;
  HIPCHK(hipMemcpyAsync(&h, d.words, sizeof(h), hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));   // the pair count sizes the sort
  if(h.err)
    return wind_type_error(ctx, who);
  return wind_scatter(ctx, d, b, nwind, d.ord, (long long) h.npairs);
}

// the out planes back to the caller's arrays
static int wind_download_state(ghip_ctx *ctx, const WindDev &d, const ghip_wind_state *s, bool inout)
{
  const size_t D = (size_t) d.nw;
  hipStream_t st = ctx->stream;
  std::vector<double> h(WIND_NOUT * D);
  HIPCHK(hipMemcpyAsync(h.data(), d.w + WP_OLD * D, WIND_NOUT * D * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(s->deleted, d.deleted, D * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  auto plane = [&](int q) { return h.data() + (size_t) (q - WP_OLD) * D; };
  if(inout)
    {
      memcpy(s->old_momentum, plane(WP_OLD), D * 8);
      memcpy(s->new_density, plane(WP_RHO), D * 8);
      memcpy(s->drmin, plane(WP_DRMIN), D * 8);
    }
  memcpy(s->dt1, plane(WP_DT1), D * 8);
  memcpy(s->dt2, plane(WP_DT2), D * 8);
  memcpy(s->dt_jump, plane(WP_DTJ), D * 8);
  memcpy(s->delta_momentum, plane(WP_DMOM), D * 8);
  return GHIP_OK;
}

// The loop for the list and the in planes of `d` (WP_AGE .. WP_DRMIN), which both entry forms have put in place:
// dt_jump, its sum and the first list (:285-302), the density at the start, the iterations, RAD_ACCEL and the
// elimination.  *end says how it ended; the out planes and d.deleted are left on the device.
enum { WIND_FLOOR, WIND_DONE, WIND_NOCONV };
struct WindEnd
{
  int stage = WIND_FLOOR;        // WIND_FLOOR: the sum of dt_jump is at or below the floor (:302), nothing has changed
  int under = 0;                 // WIND_NOCONV: particles still under way
  bool spread_pending = false;   // the last spread's events are not read yet (wind_spread_ms)
};

static int wind_loop(ghip_ctx *ctx, const ghip_wind_params *p, const WindDev &d, const char *who,
                     ghip_wind_result *result, WindEnd *end)
{
  hipStream_t st = ctx->stream;
  const int nw = d.nw;
  const size_t D = (size_t) nw;
  const WindK K = wind_k(p);
  for(int k = 0; k < 6; k++)
    if(!ctx->wind_ev[k])
      HIPCHK(hipEventCreate(&ctx->wind_ev[k]));
  hipEvent_t *ev = ctx->wind_ev;
  // ---- dt_jump, its sum and the first list (:285-302) ----
  k_wind_init<<<cdiv(nw, 256), 256, 0, st>>>(nw, d.idx, P<int>(ctx->f[GHIP_F_TIMEBIN]), d.w, d.deleted, K.dt_fac);
  k_wind_sum<<<1, 1024, 0, st>>>(nw, d.w + WP_DTJ * D, &d.words->dt_total);
  k_wind_flags<<<cdiv(nw, 256), 256, 0, st>>>(nw, d.ord, d.w + WP_DTJ * D, d.flags, d.words);
  HIPCHK(hipGetLastError());
  GCHK(ghip_select_flagged(ctx, d.ord, d.flags, d.lista, &d.words->npos, nw, st));
  WindWords h;
  HIPCHK(hipMemcpyAsync(&h, d.words, sizeof(h), hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  if(h.err)
    return wind_type_error(ctx, who);
  if(h.dt_total <= p->dt_total_floor)
    return GHIP_OK;
  GCHK(wind_injected(ctx, who));
  if(p->rad_accel)
    GCHK(wind_rad_accel(ctx, who));
  ctx->pot_n = -1;   // (positions and masses change)

  // ---- :305: the density at the start ----
  int *cur = d.lista, *nxt = d.listb;
  int m = h.npos;
  if(m < 0 || m > nw)
    return ghip_fail(ctx, GHIP_EDEVICE, "%s: a list of %d of %d particles", who, m, nw);
  k_wind_reset<<<cdiv(nw, 256), 256, 0, st>>>(nw, d.w);
  if(m > 0)
    k_wind_density<<<cdiv(m, 64), 64, 0, st>>>(m, wind_own(ctx, d, cur), WIND_TREE_ARGS, K.b, nullptr);
  HIPCHK(hipGetLastError());

  // ---- :307-490 ----
  int iter = 0, under = h.nunder;
  long long bits = 0;
  bool spread_pending = false;
  double *pos = P<double>(ctx->f[GHIP_F_POS]), *hsml = P<double>(ctx->f[GHIP_F_HSML]), *mass = P<double>(ctx->f[GHIP_F_MASS]);
  auto add_ms = [&](int k, hipEvent_t a, hipEvent_t b) {
    float f = 0;
    if(hipEventElapsedTime(&f, a, b) == hipSuccess)
      ctx->wind_ms[k] += f;
  };
  bool noconv = false;
  while(true)
    {
      iter++;
      bits += (iter == 1) ? m : under;
      HIPCHK(hipEventRecord(ev[0], st));
      HIPCHK(hipMemsetAsync(d.words, 0, 16, st));   // npairs, npos, nunder
      if(m > 0)
        k_wind_move<<<cdiv(m, 256), 256, 0, st>>>(m, cur, d.idx, ctx->n, pos, hsml, mass, nw, d.w, K);
      HIPCHK(hipEventRecord(ev[1], st));
      HIPCHK(hipMemsetAsync(d.cnt + m, 0, 8, st));
      if(m > 0)
        k_wind_density<<<cdiv(m, 64), 64, 0, st>>>(m, wind_own(ctx, d, cur), WIND_TREE_ARGS, K.b, d.cnt);
      HIPCHK(hipGetLastError());
      GCHK(ghip_scan<unsigned long long>(ctx, d.cnt, d.off, m + 1, st));
      k_wind_npairs<<<1, 64, 0, st>>>(d.off, m, d.words);
      HIPCHK(hipEventRecord(ev[2], st));
      if(m > 0)
        {
          k_wind_flags<<<cdiv(m, 256), 256, 0, st>>>(m, cur, d.w + WP_DTJ * D, d.flags, d.words);
          HIPCHK(hipGetLastError());
          GCHK(ghip_select_flagged(ctx, cur, d.flags, nxt, &d.words->npos, m, st));
        }
      HIPCHK(hipEventRecord(ev[3], st));
      HIPCHK(hipMemcpyAsync(&h, d.words, sizeof(h), hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));   // the one read of the iteration: the pair count sizes the sort
      add_ms(0, ev[0], ev[1]);
      add_ms(1, ev[1], ev[2]);
      add_ms(3, ev[2], ev[3]);
      if(spread_pending)
        add_ms(2, ev[4], ev[5]);
      spread_pending = false;
      if(h.npos < 0 || h.npos > m)
        return ghip_fail(ctx, GHIP_EDEVICE, "%s: a list of %d of %d particles", who, h.npos, m);
      if(h.npairs > 0)
        {
          HIPCHK(hipEventRecord(ev[4], st));
          GCHK(wind_scatter(ctx, d, K.b, m, cur, (long long) h.npairs));
          HIPCHK(hipEventRecord(ev[5], st));
          spread_pending = true;
        }
      std::swap(cur, nxt);
      m = h.npos;
      under = h.nunder;
      if(under == 0)
        break;
      if(iter >= p->max_iter)
        {
          noconv = true;
          break;
        }
    }
  result->iterations = iter;
  result->bits = bits;
  if(!noconv)
    {
      if(p->rad_accel)   // :497-538
        {
          const int nact = ctx->nactive < 0 ? ctx->n : ctx->nactive;
          const int *act = ctx->nactive < 0 ? nullptr : P<int>(ctx->act_host_idx);
          if(nact > 0 && ctx->ngas > 0)
            k_wind_rad_accel<<<cdiv(nact, 256), 256, 0, st>>>(nact, act, ctx->ngas, P<int>(ctx->f[GHIP_F_TYPE]),
                                                              P<int>(ctx->f[GHIP_F_TIMEBIN]), mass, P<double>(ctx->wind_inj),
                                                              P<double>(ctx->wind_ra), K.dt_fac_gas);
        }
      k_wind_eliminate<<<cdiv(nw, 256), 256, 0, st>>>(nw, d.idx, ctx->n, pos, mass, d.w, d.deleted, K);
      HIPCHK(hipGetLastError());
    }
  end->stage = noconv ? WIND_NOCONV : WIND_DONE;
  end->under = under;
  end->spread_pending = spread_pending;
  return GHIP_OK;
}

// the last spread's milliseconds, once the caller has waited for the stream
static void wind_spread_ms(ghip_ctx *ctx, const WindEnd &end)
{
  float f = 0;
  if(end.spread_pending && hipEventElapsedTime(&f, ctx->wind_ev[4], ctx->wind_ev[5]) == hipSuccess)
    ctx->wind_ms[2] += f;
}

extern "C" int ghip_wind_feedback(ghip_ctx *ctx, const ghip_wind_params *p, int nwind, const int *wind_idx,
                                  const ghip_wind_state *s, ghip_wind_result *result)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  static const char *who = "ghip_wind_feedback";
  const auto t_begin = std::chrono::steady_clock::now();
  if(result)
    memset(result, 0, sizeof(*result));
  if(!result || !p || (nwind > 0 && (!s || !s->stellar_age || !s->birth_energy || !s->old_momentum ||
                                     !s->new_density || !s->drmin || !s->dt1 || !s->dt2 || !s->dt_jump ||
                                     !s->delta_momentum || !s->deleted)))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: bad arguments", who);
  if(p->max_iter < 1 || !(p->dt_fac >= 0))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: need max_iter >= 1 and dt_fac >= 0", who);
  WindDev d;
  GCHK(wind_begin(ctx, p, nwind, wind_idx, who, &d));
  for(int k = 0; k < 5; k++)
    ctx->wind_ms[k] = 0;
  if(nwind == 0)
    return GHIP_OK;
  hipStream_t st = ctx->stream;
  const int nw = nwind;
  const size_t D = (size_t) nw;

  // ---- the state in ----
  {
    std::vector<double> h(WIND_NIN * D);
    memcpy(h.data() + WP_AGE * D, s->stellar_age, D * 8);
    memcpy(h.data() + WP_BIRTH * D, s->birth_energy, D * 8);
    memcpy(h.data() + WP_OLD * D, s->old_momentum, D * 8);
    memcpy(h.data() + WP_RHO * D, s->new_density, D * 8);
    memcpy(h.data() + WP_DRMIN * D, s->drmin, D * 8);
    HIPCHK(hipMemcpyAsync(d.w, h.data(), h.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ghip_stream_sync(ctx, st));   // (h leaves scope)
  }
  WindEnd end;
  GCHK(wind_loop(ctx, p, d, who, result, &end));
  if(end.stage == WIND_FLOOR)   // :302: the loop is not entered, nothing changes
    return wind_download_state(ctx, d, s, false);
  GCHK(wind_download_state(ctx, d, s, true));
  wind_spread_ms(ctx, end);
  for(int a = 0; a < nw; a++)   // :558-559, in list order
    if(s->deleted[a])
      {
        result->ndeleted++;
        if(s->deleted[a] == 1)
          result->deleted_momentum += s->old_momentum[a];
      }
  ctx->wind_ms[4] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  if(end.stage == WIND_NOCONV)
    return ghip_fail(ctx, GHIP_ENOCONV, "%s: %d wind particles still under way after max_iter = %d iterations", who,
                     end.under, p->max_iter);
  return GHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// the wind particles on the resident state: the wind table and the loop without host arrays
//
// One row of GHIP_WK_COUNT doubles per wind particle in a keyed row table (ghip_rowtable.h), keyed
// by PARTICLE INDEX (DESIGN.md 4.18 says why not by ID).  Sorting, compaction, growth and the table's refusals are
// the row table's; this file says which indices may have a row (k_wk_check_type), where a row goes when the particles
// are reordered (k_wk_map), and what the loop reads and writes (k_wk_flag_list, k_wk_load, k_wk_store).
// ghip_winds_feedback makes its list by a device selection over the active list, gathers the in planes from the
// rows, runs wind_loop and scatters the out planes back.
// ---------------------------------------------------------------------------------------------
#define WK_NC GHIP_WK_COUNT
static_assert(GHIP_WK_STELLAR_AGE == WP_AGE && GHIP_WK_DRMIN == WP_DRMIN && GHIP_WK_DELTA_MOMENTUM == WP_DMOM,
              "the first nine columns of a row are the planes WP_AGE .. WP_DMOM");

// an index of the m unsorted rows whose particle is not Type 3 raises the error words
__global__ void __launch_bounds__(256) k_wk_check_type(int m, const unsigned int *__restrict__ idx, int n,
                                                       const int *__restrict__ type, int *__restrict__ words)
{
  const int r = blockIdx.x * 256 + threadIdx.x;
  if(r >= m)
    return;
  const int i = (int) idx[r];
  if(i < 0 || i >= n || type[i] != 3)
    {
      words[RTW_ERR] = 1;
      atomicMax(words + RTW_ERRKEY, i);
    }
}

// what every entry point of the section refuses.  dd == false: the single-rank family (a plain context or a
// ghip_dd_init context of one rank); dd == true: the shard family ghip_dd_winds_* and the wind forms of GHIP_DD_WIND
// that read the table (a ghip_dd_init context of any rank count)
int ghip_winds_enter(ghip_ctx *ctx, const char *who, bool dd)
{
  if(ctx->shard_n > 1)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: not available on a sharded context (ghip_set_shard): the resident wind "
                     "particles are %s", who, dd ? "for ghip_dd_init contexts" : "single-rank only");
  if(dd && !ctx->dd.on)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: not a multi-GPU context (ghip_dd_init): on a plain context the wind table "
                     "is ghip_winds_set_table / ghip_winds_get_table / ghip_winds_clear and the loop ghip_winds_feedback",
                     who);
  if(!dd && ctx->dd.on && ctx->dd.nranks > 1)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: the shard form is not built into this entry point: on a multi-GPU context "
                     "(ghip_dd_init with %d ranks) the table is ghip_dd_winds_set_table / ghip_dd_winds_get_table / "
                     "ghip_dd_winds_clear and the loop GHIP_DD_WIND with walk = GHIP_WINDS_RESIDENT_FORM", who,
                     ctx->dd.nranks);
  HIPCHK(hipSetDevice(ctx->device));
  return GHIP_OK;
}

// the bodies of the two families (dd: ghip_winds_enter)
static int winds_set_table(ghip_ctx *ctx, const char *who, bool dd, int nwind, const int *idx, const double *rows)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || nwind < 0 || (nwind > 0 && (!idx || !rows)))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: bad arguments", who);
  GCHK(ghip_winds_enter(ctx, who, dd));
  RowTable &T = ctx->wk;
  hipStream_t st = ctx->stream;
  T.on = false;
  T.n = 0;
  T.stale = false;
  for(int r = 0; r < nwind; r++)
    if(idx[r] < 0 || idx[r] >= ctx->n)
      return ghip_fail(ctx, GHIP_EINVAL, "%s: wind particle index %d out of range (the context holds no table now)",
                       who, idx[r]);
  int hw[RTW_WORDS] = {};
  if(nwind > 0)   // (the indices are in [0, n): the same bits as unsigned keys)
    {
      RtWork W;
      GCHK(ghip_rt_work(ctx, T, (size_t) nwind, 0, W, true));
      GCHK(ghip_rt_stage_host(ctx, T, nwind, reinterpret_cast<const unsigned int *>(idx), rows));
      k_wk_check_type<<<cdiv(nwind, 256), 256, 0, st>>>(nwind, P<unsigned int>(T.tmp_key), ctx->n,
                                                       P<int>(ctx->f[GHIP_F_TYPE]), W.words);
      HIPCHK(hipGetLastError());
    }
  const int rc = ghip_rt_install(ctx, T, nwind, who, true, hw);
  if(hw[RTW_ERR])   // (read with the duplicate words, and said first)
    {
      T.on = false;
      T.n = 0;
      return ghip_fail(ctx, GHIP_EINVAL, "%s: index %d names a particle that is not Type 3 (the context holds no "
                       "table now)", who, hw[RTW_ERRKEY]);
    }
  return rc;
}

static int winds_get_table(ghip_ctx *ctx, const char *who, bool dd, int *nwind, int *idx, double *rows)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !nwind)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: bad arguments", who);
  GCHK(ghip_winds_enter(ctx, who, dd));
  GCHK(ghip_rt_need(ctx, ctx->wk, who, true));
  return ghip_rt_get(ctx, ctx->wk, nwind, reinterpret_cast<unsigned int *>(idx), rows);
}

static int winds_clear(ghip_ctx *ctx, const char *who, bool dd)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  GCHK(ghip_winds_enter(ctx, who, dd));
  GCHK(ghip_rt_clear(ctx, ctx->wk));
  (void) ctx->wk_spawn.release();
  (void) ctx->wk_rnd.release();
  return GHIP_OK;
}

extern "C" int ghip_winds_set_table(ghip_ctx *ctx, int nwind, const int *idx, const double *rows)
{
  return winds_set_table(ctx, "ghip_winds_set_table", false, nwind, idx, rows);
}
extern "C" int ghip_winds_get_table(ghip_ctx *ctx, int *nwind, int *idx, double *rows)
{
  return winds_get_table(ctx, "ghip_winds_get_table", false, nwind, idx, rows);
}
extern "C" int ghip_winds_clear(ghip_ctx *ctx) { return winds_clear(ctx, "ghip_winds_clear", false); }
// the table of a shard: local indices, a ghip_dd_init context of any rank count
extern "C" int ghip_dd_winds_set_table(ghip_ctx *ctx, int nwind, const int *idx, const double *rows)
{
  return winds_set_table(ctx, "ghip_dd_winds_set_table", true, nwind, idx, rows);
}
extern "C" int ghip_dd_winds_get_table(ghip_ctx *ctx, int *nwind, int *idx, double *rows)
{
  return winds_get_table(ctx, "ghip_dd_winds_get_table", true, nwind, idx, rows);
}
extern "C" int ghip_dd_winds_clear(ghip_ctx *ctx) { return winds_clear(ctx, "ghip_dd_winds_clear", true); }

// ---- the table through ghip_rearrange / ghip_peano_order ----
// keep[r] = the particle of row r survives; its new index is the row's new key
__global__ void __launch_bounds__(256) k_wk_map(int m, const unsigned int *__restrict__ idx, int n_before,
                                                const int *__restrict__ new_of_old, unsigned int *__restrict__ newidx,
                                                int *__restrict__ keep)
{
  const int r = blockIdx.x * 256 + threadIdx.x;
  if(r >= m)
    return;
  const int i = (int) idx[r];
  const int j = (i >= 0 && i < n_before) ? new_of_old[i] : -1;
  newidx[r] = (unsigned int) j;
  keep[r] = j >= 0;
}

int ghip_winds_remap(ghip_ctx *ctx, const char *who, int n_before, const int *new_of_old)
{
  RowTable &T = ctx->wk;
  if(!T.on || T.n == 0 || n_before <= 0)
    return GHIP_OK;
  const int m = T.n;
  RtWork W;
  GCHK(ghip_rt_work(ctx, T, (size_t) m, 0, W, true));
  unsigned int *newidx = reinterpret_cast<unsigned int *>(W.c);
  k_wk_map<<<cdiv(m, 256), 256, 0, ctx->stream>>>(m, P<unsigned int>(T.key), n_before, new_of_old, newidx, W.a);
  HIPCHK(hipGetLastError());
  int kept = 0;
  GCHK(ghip_rt_compact(ctx, T, who, W, W.a, newidx, 0, &kept));
  // (sorted again without a read: a map sends no two particles to one index)
  return ghip_rt_install(ctx, T, kept, who, true, nullptr);
}

// ---- the table through GHIP_DD_MIGRATE (ghip_dd.hip, migrate_step) ----
// A migration renumbers the shard: kept gas, received gas, kept others, received others (k_mig_move_old / _new).
// A row of a particle that stays is re-keyed to the particle's new index.  A row of a particle that leaves travels in
// an exchange of its own as (the particle's ordinal in the sender's run for that destination, the row): the receiver
// finds the particle at that ordinal behind the sender's receive offset and keys the row by its new index.  A
// departing Type-3 particle without a row departs without one; an arrival without a record stays without a row.
struct WkMigRec
{
  unsigned long long ordinal;
  double c[WK_NC];
};
struct WkMigOff
{
  int v[GHIP_MAXRANKS];
};

// flags[a] = the a-th departing particle is Type 3 and has a row
__global__ void __launch_bounds__(256) k_wkm_count(int total, const int *__restrict__ list, int n,
                                                   const int *__restrict__ type, int nrows,
                                                   const unsigned int *__restrict__ idx, int *__restrict__ flags)
{
  const int a = blockIdx.x * 256 + threadIdx.x;
  if(a >= total)
    return;
  const int i = list[a];
  flags[a] = i >= 0 && i < n && type[i] == 3 && d_rt_find(nrows, idx, (unsigned int) i) >= 0;
}

// cnt[r] = the rows of the run of destination r (pos: the exclusive scan of flags [total + 1])
__global__ void k_wkm_runs(int nranks, WkMigOff start, WkMigOff len, const int *__restrict__ pos, int *__restrict__ cnt)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if(r < nranks)
    cnt[r] = pos[start.v[r] + len.v[r]] - pos[start.v[r]];
}

// the records of the flagged particles, per destination in the order of its run
__global__ void __launch_bounds__(256) k_wkm_pack(int total, const int *__restrict__ list, const int *__restrict__ flags,
                                                  const int *__restrict__ pos, int nranks, WkMigOff start, WkMigOff len,
                                                  WkMigOff out_off, WkMigOff out_len, int nrows,
                                                  const unsigned int *__restrict__ idx, const double *__restrict__ rows,
                                                  WkMigRec *__restrict__ out)
{
  const int a = blockIdx.x * 256 + threadIdx.x;
  if(a >= total || !flags[a])
    return;
  int dest = -1;
  for(int r = 0; r < nranks; r++)
    if(a >= start.v[r] && a < start.v[r] + len.v[r])
      dest = r;
  if(dest < 0)
    return;
  const int k = pos[a] - pos[start.v[dest]];
  const int row = d_rt_find(nrows, idx, (unsigned int) list[a]);
  if(k < 0 || k >= out_len.v[dest] || row < 0)   // (cannot happen: k_wkm_runs counted the same flags)
    return;
  WkMigRec &R = out[out_off.v[dest] + k];
  R.ordinal = (unsigned long long) (a - start.v[dest]);
  for(int c = 0; c < WK_NC; c++)
    R.c[c] = rows[(size_t) row * WK_NC + c];
}

// keep[r] = the particle of row r stays; its new index is the row's new key
__global__ void __launch_bounds__(256) k_wkm_rekey(int m, const unsigned int *__restrict__ idx, WkMigPlan M,
                                                   unsigned int *__restrict__ newidx, int *__restrict__ keep)
{
  const int r = blockIdx.x * 256 + threadIdx.x;
  if(r >= m)
    return;
  const int i = (int) idx[r];
  const bool stays = i >= M.ng_old && i < M.n_old && M.mask[i] == 0;
  newidx[r] = stays ? (unsigned int) (M.ngn + (int) (M.ro[i] >> 32)) : 0u;
  keep[r] = stays;
}

// record a of the arrivals (from: where each sender's records begin, [nranks] and the total behind them) -> the new
// index of the particle it names and its row; a record that names no arriving particle of the block behind the gas
// raises the error words
__global__ void __launch_bounds__(256) k_wkm_unpack(int nrecv, const WkMigRec *__restrict__ rec, int nranks,
                                                    WkMigOff from, WkMigPlan M, unsigned int *__restrict__ newidx,
                                                    double *__restrict__ rows, int *__restrict__ words)
{
  const int a = blockIdx.x * 256 + threadIdx.x;
  if(a >= nrecv)
    return;
  int s = 0;
  for(int r = 1; r < nranks; r++)
    if(a >= from.v[r])
      s = r;
  const unsigned long long o = rec[a].ordinal;
  unsigned int key = 0xffffffffu - (unsigned int) a;   // (an error: no two rows under one key, the words say the rest)
  bool ok = o < (unsigned long long) M.cnt[s];
  if(ok)
    {
      const int q = M.first[s] + (int) o;
      ok = q >= 0 && q < M.nrecv && M.vn[q] == (1ULL << 32);
      if(ok)
        key = (unsigned int) (M.ngn + M.ko + (int) (M.rn[q] >> 32));
    }
  if(!ok)
    {
      words[RTW_ERR] = 1;
      atomicMax(words + RTW_ERRKEY, a);
    }
  newidx[a] = key;
  for(int c = 0; c < WK_NC; c++)
    rows[(size_t) a * WK_NC + c] = rec[a].c[c];
}

int ghip_winds_mig_pack(ghip_ctx *ctx, int total, const int *list, const int *scount, const int *soff)
{
  static_assert(sizeof(WkMigRec) == 8 + 8 * WK_NC, "WkMigRec layout");
  DDState &D = ctx->dd;
  RowTable &T = ctx->wk;
  hipStream_t st = ctx->stream;
  const int m = T.n, P_ = D.nranks;
  WkMigOff start, len, out_off, out_len;
  for(int r = 0; r < GHIP_MAXRANKS; r++)
    {
      start.v[r] = r < P_ ? soff[r] : 0;
      len.v[r] = r < P_ && r != D.rank ? scount[r] : 0;
      out_off.v[r] = out_len.v[r] = D.wk_rscount[r] = D.wk_rsoff[r] = 0;
    }
  int tot = 0;
  if(m > 0 && total > 0)
    {
      const size_t t1 = (size_t) total + 1;
      GCHK(ghip_ensure(ctx, D.wk_flag, (2 * t1 + GHIP_MAXRANKS) * 4));
      int *flags = P<int>(D.wk_flag), *pos = flags + t1, *cnt = pos + t1;
      HIPCHK(hipMemsetAsync(flags, 0, (2 * t1 + GHIP_MAXRANKS) * 4, st));
      k_wkm_count<<<cdiv(total, 256), 256, 0, st>>>(total, list, ctx->n, P<int>(ctx->f[GHIP_F_TYPE]), m,
                                                   P<unsigned int>(T.key), flags);
      HIPCHK(hipGetLastError());
      GCHK(ghip_scan<int>(ctx, flags, pos, total + 1, st));
      k_wkm_runs<<<1, GHIP_MAXRANKS, 0, st>>>(P_, start, len, pos, cnt);
      HIPCHK(hipGetLastError());
      int h[GHIP_MAXRANKS];
      HIPCHK(hipMemcpyAsync(h, cnt, (size_t) P_ * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      for(int r = 0; r < P_; r++)
        if(h[r] < 0 || h[r] > len.v[r] || h[r] > m)
          return ghip_fail(ctx, GHIP_EDEVICE, "GHIP_DD_MIGRATE: %d wind rows in a run of %d particles for rank %d, %d "
                           "rows held", h[r], len.v[r], r, m);
      for(int r = 0; r < P_; r++)
        {
          const int c = h[r];
          out_off.v[r] = D.wk_rsoff[r] = tot;
          out_len.v[r] = D.wk_rscount[r] = c;
          tot += c;
        }
      GCHK(ghip_ensure(ctx, D.wk_rsend, (size_t) (tot > 0 ? tot : 1) * sizeof(WkMigRec)));
      if(tot > 0)
        {
          k_wkm_pack<<<cdiv(total, 256), 256, 0, st>>>(total, list, flags, pos, P_, start, len, out_off, out_len, m,
                                                      P<unsigned int>(T.key), P<double>(T.rows), P<WkMigRec>(D.wk_rsend));
          HIPCHK(hipGetLastError());
        }
    }
  if(tot == 0)
    GCHK(ghip_ensure(ctx, D.wk_rsend, sizeof(WkMigRec)));
  return GHIP_OK;
}

void ghip_winds_mig_post(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  ghip_dd_set_alltoallv(D, D.wk_rsend.p, sizeof(WkMigRec), D.wk_rscount, D.wk_rsoff, &D.wk_rrecv);
}

int ghip_winds_mig_merge(ghip_ctx *ctx)
{
  static const char *who = "GHIP_DD_MIGRATE";
  DDState &D = ctx->dd;
  RowTable &T = ctx->wk;
  hipStream_t st = ctx->stream;
  const WkMigPlan &M = D.wk_plan;
  const int m = T.n, nrecv = D.x.rtotal;
  if(!M.moved)   // (nobody left this shard and nobody came: every key stands, and no record can name a particle)
    {
      if(nrecv > 0)
        return ghip_fail(ctx, GHIP_ECOMM, "%s: %d wind rows came to a shard that received no particle", who, nrecv);
      return GHIP_OK;
    }
  WkMigOff from;
  for(int r = 0; r < GHIP_MAXRANKS; r++)
    from.v[r] = r < D.nranks ? D.x.roff[r] : nrecv;
  RtWork W;
  GCHK(ghip_rt_work(ctx, T, (size_t) (m + nrecv + 1), 0, W, true));
  unsigned int *newidx = reinterpret_cast<unsigned int *>(W.c);
  if(m > 0)
    {
      k_wkm_rekey<<<cdiv(m, 256), 256, 0, st>>>(m, P<unsigned int>(T.key), M, newidx, W.a);
      HIPCHK(hipGetLastError());
    }
  int kept = 0, hw[RTW_WORDS] = {};
  GCHK(ghip_rt_compact(ctx, T, who, W, W.a, newidx, nrecv, &kept));
  if(nrecv > 0)
    {
      k_wkm_unpack<<<cdiv(nrecv, 256), 256, 0, st>>>(nrecv, P<WkMigRec>(D.wk_rrecv), D.nranks, from, M,
                                                    P<unsigned int>(T.tmp_key) + kept,
                                                    P<double>(T.tmp_rows) + (size_t) kept * WK_NC, W.words);
      HIPCHK(hipGetLastError());
    }
  // (sorted again: the kept rows are ascending still, the arrivals lie behind them in the block)
  const int rc = ghip_rt_install(ctx, T, kept + nrecv, who, true, hw);
  if(hw[RTW_ERR])
    {
      T.on = false;
      T.n = 0;
      return ghip_fail(ctx, GHIP_ECOMM, "%s: wind row record %d names no arriving particle behind the gas block (the "
                       "context holds no wind table now)", who, hw[RTW_ERRKEY]);
    }
  return rc;
}

// ---- the loop ----
// flags[a] = the a-th active particle is Type 3 and has a row with StellarAge < Time (:259); an active Type-3
// particle without a row raises the error words
__global__ void __launch_bounds__(256) k_wk_flag_list(int nact, const int *__restrict__ act, int n,
                                                      const int *__restrict__ type, int nrows,
                                                      const unsigned int *__restrict__ idx,
                                                      const double *__restrict__ rows, double Time, int *__restrict__ flags, int *__restrict__ words)
{
  const int a = blockIdx.x * 256 + threadIdx.x;
  if(a >= nact)
    return;
  const int i = act ? act[a] : a;
  int f = 0;
  if(i >= 0 && i < n && type[i] == 3)
    {
      const int r = d_rt_find(nrows, idx, (unsigned int) i);
      if(r < 0)
        {
          words[RTW_ERR] = 1;
          atomicMax(words + RTW_ERRKEY, i);
        }
      else
        f = rows[(size_t) r * WK_NC + GHIP_WK_STELLAR_AGE] < Time;
    }
  flags[a] = f;
}

// the in planes of the list from the rows
__global__ void __launch_bounds__(256) k_wk_load(int nw, const int *__restrict__ list, int nrows,
                                                 const unsigned int *__restrict__ idx,
                                                 const double *__restrict__ rows, double *__restrict__ w)
{
  const int a = blockIdx.x * 256 + threadIdx.x;
  if(a >= nw)
    return;
  const int r = d_rt_find(nrows, idx, (unsigned int) list[a]);
  if(r < 0)
    return;   // (never: the selection listed only particles with a row)
  const double *R = rows + (size_t) r * WK_NC;
  for(int q = WP_AGE; q <= WP_DRMIN; q++)
    w[(size_t) q * nw + a] = R[q];
}

// the out planes WP_OLD .. WP_DMOM back into the rows (all == 0: WP_DT1 .. WP_DMOM only, after a call that did not
// enter the loop), and the code of the elimination
__global__ void __launch_bounds__(256) k_wk_store(int nw, const int *__restrict__ list, int nrows,
                                                  const unsigned int *__restrict__ idx, double *__restrict__ rows,
                                                  const double *__restrict__ w, const int *__restrict__ deleted, int all)
{
  const int a = blockIdx.x * 256 + threadIdx.x;
  if(a >= nw)
    return;
  const int r = d_rt_find(nrows, idx, (unsigned int) list[a]);
  if(r < 0)
    return;
  double *R = rows + (size_t) r * WK_NC;
  for(int q = all ? WP_OLD : WP_DT1; q <= WP_DMOM; q++)
    R[q] = w[(size_t) q * nw + a];
  R[GHIP_WK_DELETED] = (double) deleted[a];
}

// :558-559: one thread, list order (what ghip_wind_feedback adds on the host from its out arrays)
__global__ void k_wk_result(int nw, const int *__restrict__ deleted, const double *__restrict__ old,
                            ghip_wind_result *__restrict__ res)
{
  if(blockIdx.x != 0 || threadIdx.x != 0)
    return;
  int nd = 0;
  double mom = 0;
  for(int a = 0; a < nw; a++)
    if(deleted[a])
      {
        nd++;
        if(deleted[a] == 1)
          mom += old[a];
      }
  res->ndeleted = nd;
  res->deleted_momentum = mom;
}

extern "C" int ghip_winds_feedback(ghip_ctx *ctx, const ghip_wind_params *p, ghip_wind_result *result)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  static const char *who = "ghip_winds_feedback";
  const auto t_begin = std::chrono::steady_clock::now();
  if(result)
    memset(result, 0, sizeof(*result));
  if(!result || !p)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: bad arguments", who);
  if(p->max_iter < 1 || !(p->dt_fac >= 0))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: need max_iter >= 1 and dt_fac >= 0", who);
  GCHK(ghip_winds_enter(ctx, who));
  GCHK(ghip_rt_need(ctx, ctx->wk, who, true));
  RowTable &T = ctx->wk;
  hipStream_t st = ctx->stream;
  for(int k = 0; k < 5; k++)
    ctx->wind_ms[k] = 0;
  // ---- the list: a selection over the active list, its length to the host ----
  const int nact = ctx->nactive < 0 ? ctx->n : ctx->nactive;
  const int *dact = ctx->nactive < 0 ? nullptr : P<int>(ctx->act_host_idx);
  if(nact <= 0)
    return GHIP_OK;
  RtWork W;
  GCHK(ghip_rt_work(ctx, T, (size_t) nact, 0, W, true));
  ghip_wind_result *dres = reinterpret_cast<ghip_wind_result *>(W.report);
  k_wk_flag_list<<<cdiv(nact, 256), 256, 0, st>>>(nact, dact, ctx->n, P<int>(ctx->f[GHIP_F_TYPE]), T.n,
                                                  P<unsigned int>(T.key), P<double>(T.rows), p->Time, W.a, W.words);
  HIPCHK(hipGetLastError());
  GCHK(ghip_select_flagged(ctx, dact, W.a, W.b, W.words + RTW_COUNT, nact, st));
  int w[RTW_WORDS];
  HIPCHK(hipMemcpyAsync(w, W.words, sizeof(w), hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  if(w[RTW_ERR])
    return ghip_fail(ctx, GHIP_EINVAL, "%s: the active Type-3 particle %d has no row in the wind table (%d rows); "
                     "nothing was changed", who, w[RTW_ERRKEY], T.n);
  const int nw = w[RTW_COUNT];
  if(nw < 0 || nw > nact || nw > T.n)
    return ghip_fail(ctx, GHIP_EDEVICE, "%s: a list of %d of %d active particles, %d rows", who, nw, nact, T.n);
  if(nw == 0)
    return GHIP_OK;
  GCHK(wind_need_trees(ctx, who));
  WindDev d;
  GCHK(wind_begin_list(ctx, nw, W.b, false, &d));
  const size_t D = (size_t) nw;
  k_wk_load<<<cdiv(nw, 256), 256, 0, st>>>(nw, d.idx, T.n, P<unsigned int>(T.key), P<double>(T.rows), d.w);
  HIPCHK(hipGetLastError());
  WindEnd end;
  GCHK(wind_loop(ctx, p, d, who, result, &end));
  const bool all = end.stage != WIND_FLOOR;
  k_wk_store<<<cdiv(nw, 256), 256, 0, st>>>(nw, d.idx, T.n, P<unsigned int>(T.key), P<double>(T.rows), d.w, d.deleted,
                                            all);
  HIPCHK(hipGetLastError());
  if(all)
    {
      k_wk_result<<<1, 64, 0, st>>>(nw, d.deleted, d.w + WP_OLD * D, dres);
      HIPCHK(hipGetLastError());
      ghip_wind_result r;
      HIPCHK(hipMemcpyAsync(&r, dres, sizeof(r), hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      result->ndeleted = r.ndeleted;
      result->deleted_momentum = r.deleted_momentum;
      wind_spread_ms(ctx, end);
    }
  else
    HIPCHK(ghip_stream_sync(ctx, st));
  ctx->wind_ms[4] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  if(end.stage == WIND_NOCONV)
    return ghip_fail(ctx, GHIP_ENOCONV, "%s: %d wind particles still under way after max_iter = %d iterations", who,
                     end.under, p->max_iter);
  return GHIP_OK;
}

extern "C" int ghip_wind_get_timing(ghip_ctx *ctx, double ms[5])
{
  if(!ctx || !ms)
    return GHIP_EINVAL;
  for(int k = 0; k < 5; k++)
    ms[k] = ctx->wind_ms[k];
  return GHIP_OK;
}

extern "C" int ghip_wind_get_injected(ghip_ctx *ctx, double *injected)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  GCHK(wind_refuse_sharded(ctx, "ghip_wind_get_injected", true));
  if(!injected)
    return GHIP_OK;
  GCHK(wind_injected(ctx, "ghip_wind_get_injected"));
  return wind_download3(ctx, ctx->wind_inj, injected, ctx->ngas);
}

extern "C" int ghip_wind_set_injected(ghip_ctx *ctx, const double *injected)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  GCHK(wind_refuse_sharded(ctx, "ghip_wind_set_injected", true));
  if(!injected)
    return GHIP_OK;
  GCHK(wind_upload3(ctx, ctx->wind_inj, injected, ctx->ngas));
  ctx->wind_inj_ngas = ctx->ngas;
  return GHIP_OK;
}

extern "C" int ghip_wind_get_rad_accel(ghip_ctx *ctx, double *rad_accel)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  GCHK(wind_refuse_sharded(ctx, "ghip_wind_get_rad_accel", true));
  if(!rad_accel)
    return GHIP_OK;
  GCHK(wind_rad_accel(ctx, "ghip_wind_get_rad_accel"));
  return wind_download3(ctx, ctx->wind_ra, rad_accel, ctx->ngas);
}

extern "C" int ghip_wind_set_rad_accel(ghip_ctx *ctx, const double *rad_accel)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  GCHK(wind_refuse_sharded(ctx, "ghip_wind_set_rad_accel", true));
  if(!rad_accel)
    return GHIP_OK;
  GCHK(wind_upload3(ctx, ctx->wind_ra, rad_accel, ctx->ngas));
  ctx->wind_ra_ngas = ctx->ngas;
  return GHIP_OK;
}

extern "C" int ghip_set_rad_accel(ghip_ctx *ctx, int on)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  if(on)
    GCHK(wind_refuse_sharded(ctx, "ghip_set_rad_accel", true));
  ctx->rad_accel_on = on != 0;
  return GHIP_OK;
}

// RadAccel [3][ngas] for the kick, the PM kick and the drift under ghip_set_rad_accel (made and zeroed at
// first use): *ra = nullptr with the switch off
int ghip_rad_accel_field(ghip_ctx *ctx, const char *who, const double **ra)
{
  *ra = nullptr;
  if(!ctx->rad_accel_on)
    return GHIP_OK;
  GCHK(wind_refuse_sharded(ctx, who, true));
  GCHK(wind_rad_accel(ctx, who));
  *ra = P<double>(ctx->wind_ra);
  return GHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// the loop on multi-GPU shards (GHIP_DD_WIND: GHIP_DD_DUST_DRAG begun with one of the wind forms as `walk`;
// ghip_dd_dust_begin / _step hand over)
//
// The reference runs momentum_feedback() under NTask > 1: dt_total and N_active are all-reduced
// (momentum_feedback.c:301, 469-470), virtual_density() and virtual_spread_momentum() export a particle to the
// tasks its sphere touches and add (virtual_density.c:344) or minimise (:356) what comes back.  Here a wind
// particle stays on its home shard, which moves it; it goes to every other shard whose gas boxes its sphere can
// reach (the all-gathered group boxes of the Type-0 particles with Mass > 0, ghip_dd.hip):
//   GROUPS    list, order, velocities, dt_jump and its sum, the first list; group table -> all-gather, with the
//             shard's hmax, dt_jump sum, list length and failure flag in the status record behind it
//   START     the floor test on the sum of all shards (ascending rank order); the density at the start (:305)
//   per iteration  [move and] own density partial; selection; records {Pos, Hsml}      -> all-to-all-v
//     DENS_IMP   the imported records against this shard's gas; partials {rho, drmin}  -> all-to-all-v (home)
//     DENS_ADD   own + partials in ascending rank order, drmin = min; the new list;
//                {list length, above 1e-40, failed}                                    -> all-gather
//     STATUS     every shard stops if one failed; records {rho, dmom, Vel, |Vel|}       -> all-to-all-v
//     SPREAD     the scatter of the own list and the imported records into this shard's gas; stop or go on
// Four exchanges per iteration: the spread needs the total density (two dependent all-to-all-v), the stop decision
// is the reference's all-reduce, and the spread records need that density.  The importing shard keeps the density
// records, so the spread record carries no position.  DENSITY_FORM ends in DENS_ADD, SPREAD_FORM goes from START
// over the position records (SPREAD_POS) to SPREAD.
// ---------------------------------------------------------------------------------------------
int ghip_dd_wind_groups(ghip_ctx *ctx, const double extra[3], int own_rc);   // ghip_dd.hip
int ghip_dd_wind_status(ghip_ctx *ctx, const char *what, double *extra);
int ghip_dd_wind_select(ghip_ctx *ctx, int m, const int *list, const int *idx, const double *dtj, const double *drmin,
                        int cut, double hmax, double boxsize, int periodic, int *total);

// record r of the send lists: local particle list[r], list slot slot[list[r]].  K = WIND_REC_DENS: {Pos, Hsml};
// K = WIND_REC_SPREAD: {NewDensity, DeltaPhotonMomentum, Vel, |Vel|} from the planes
template <int K>
__global__ void k_wind_pack(int total, const int *__restrict__ list, const int *__restrict__ slot, int n,
                            const double *__restrict__ pos, const double *__restrict__ hsml, int nw,
                            const double *__restrict__ w, double *__restrict__ out)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if(r >= total)
    return;
  const int i = list[r];
  double *o = out + (size_t) K * r;
  if(K == WIND_REC_DENS)
    {
      o[0] = pos[i];
      o[1] = pos[(size_t) n + i];
      o[2] = pos[2 * (size_t) n + i];
      o[3] = hsml[i];
    }
  else
    {
      const int a = slot[i];
      const size_t D = (size_t) nw;
      o[0] = w[WP_RHO * D + a];
      o[1] = w[WP_DMOM * D + a];
      o[2] = w[WP_VX * D + a];
      o[3] = w[WP_VY * D + a];
      o[4] = w[WP_VZ * D + a];
      o[5] = w[WP_VABS * D + a];
    }
}

// the partials {rho, drmin} one shard returned for the cnt particles it was sent: NewDensity += , drmin = min
__global__ void k_wind_add_parts(int cnt, const int *__restrict__ list, const int *__restrict__ slot,
                                 const double *__restrict__ back, int nw, double *__restrict__ w)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if(k >= cnt)
    return;
  const int a = slot[list[k]];
  const size_t D = (size_t) nw;
  w[WP_RHO * D + a] += back[2 * (size_t) k];
  const double dr = back[2 * (size_t) k + 1];
  if(dr < w[WP_DRMIN * D + a])
    w[WP_DRMIN * D + a] = dr;
}

extern "C" size_t ghip_dd_wind_args_size(void)
{
  return sizeof(ghip_dd_wind_args);
}

extern "C" size_t ghip_dd_winds_args_size(void)
{
  return sizeof(ghip_dd_winds_args);
}

enum { WDD_GROUPS, WDD_START, WDD_DENS_IMP, WDD_DENS_ADD, WDD_STATUS, WDD_SPREAD, WDD_SPREAD_POS };

static const char *wind_dd_who(int form, bool resident = false)
{
  if(resident)
    return "ghip_dd winds feedback";
  return form == GHIP_WIND_DENSITY_FORM ? "ghip_dd wind density"
                                        : (form == GHIP_WIND_SPREAD_FORM ? "ghip_dd wind spread" : "ghip_dd wind feedback");
}

int ghip_dd_wind_begin(ghip_ctx *ctx, int, const void *params, int walk)
{
  GHIP_JOIN(ctx);
  if(walk == GHIP_WINDS_SPAWN_FORM)   // (the creation of wind particles, ghip_accretion.hip: it asks for no tree)
    return ghip_dd_spawn_begin(ctx, params);
  const bool resident = walk == GHIP_WINDS_RESIDENT_FORM;
  const char *who = wind_dd_who(walk, resident);
  if(walk != GHIP_WIND_FORM && walk != GHIP_WIND_DENSITY_FORM && walk != GHIP_WIND_SPREAD_FORM && !resident)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd wind: walk = %d is none of GHIP_WIND_FORM, GHIP_WIND_DENSITY_FORM, "
                     "GHIP_WIND_SPREAD_FORM, GHIP_WINDS_RESIDENT_FORM and GHIP_WINDS_SPAWN_FORM", walk);
  GCHK(wind_refuse_sharded(ctx, who, true));
  // the resident form is the whole loop with another source of the list and the planes: its arguments become
  // those of GHIP_WIND_FORM with no list yet (the selection of the first step sets nwind)
  ghip_dd_wind_args a = {};
  if(resident)
    {
      const ghip_dd_winds_args &r = *reinterpret_cast<const ghip_dd_winds_args *>(params);
      a.p = r.p;
      a.result = r.result;
      a.counts = r.counts;
      walk = GHIP_WIND_FORM;
    }
  else
    a = *reinterpret_cast<const ghip_dd_wind_args *>(params);
  const ghip_wind_state *s = a.state;
  bool bad = !a.p || a.nwind < 0 || (a.nwind > 0 && !a.wind_idx);
  if(walk == GHIP_WIND_FORM)
    bad = bad || !a.result || (a.nwind > 0 && (!s || !s->stellar_age || !s->birth_energy || !s->old_momentum ||
                                               !s->new_density || !s->drmin || !s->dt1 || !s->dt2 || !s->dt_jump ||
                                               !s->delta_momentum || !s->deleted));
  else if(walk == GHIP_WIND_DENSITY_FORM)
    bad = bad || (a.nwind > 0 && (!a.dt_jump || !a.new_density || !a.drmin));
  else
    bad = bad || (a.nwind > 0 && (!a.dt_jump || !a.new_density || !a.delta_momentum));
  if(bad)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: bad arguments", who);
  if(walk == GHIP_WIND_FORM && (a.p->max_iter < 1 || !(a.p->dt_fac >= 0)))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: need max_iter >= 1 and dt_fac >= 0", who);
  // (after GHIP_DD_BH_SWALLOW the trees are marked stale for their moments; their geometry still holds)
  if(!ctx->gt.built && !ctx->dd.geom_kept)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: run GHIP_DD_GRAVITY of this step first", who);
  if(!ctx->st.built && !ctx->dd.geom_kept)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: run GHIP_DD_DENSITY of this step first", who);
  for(int k = 0; k < a.nwind; k++)
    if(a.wind_idx[k] < 0 || a.wind_idx[k] >= ctx->n)
      return ghip_fail(ctx, GHIP_EINVAL, "%s: wind particle index %d out of range", who, a.wind_idx[k]);
  WindDD &W = ctx->dd.wind;
  W = WindDD();
  W.a = a;
  W.p = *a.p;
  W.a.p = &W.p;
  W.form = walk;
  W.resident = resident;
  for(int k = 0; k < 5; k++)
    ctx->wind_ms[k] = 0;
  if(a.result)
    memset(a.result, 0, sizeof(*a.result));
  if(a.counts)
    for(int k = 0; k < 6; k++)
      a.counts[k] = 0;
  return GHIP_OK;
}

static void wind_dd_counts(const DDState &D)
{
  const WindDD &W = D.wind;
  if(!W.a.counts)
    return;
  W.a.counts[0] = W.sent;
  W.a.counts[1] = W.recvd;
  W.a.counts[2] = W.imp_pairs;
  W.a.counts[3] = W.exchanges;
  W.a.counts[4] = D.bytes_sent[D.op];
  W.a.counts[5] = W.iter;
}

static int *wind_dd_list(const WindDev &d, const WindDD &W, bool next = false)
{
  if(W.form != GHIP_WIND_FORM)
    return d.ord;
  return (W.cur ^ (next ? 1 : 0)) ? d.listb : d.lista;
}

// Device milliseconds of the operation's phases on this shard, for ghip_wind_get_timing: [0] move, [1] own density,
// [2] spread (count, fill, sort, apply), [3] list, [4] imported density -- summed over the iterations.  An event pair
// is read after the next wait of the host that the operation has anyway.
enum { WT_MOVE = 0, WT_OWN = 1, WT_SPREAD = 2, WT_LIST = 3, WT_IMP = 4 };
static int wind_dd_mark(ghip_ctx *ctx, int k)
{
  if(!ctx->wind_ev[k])
    HIPCHK(hipEventCreate(&ctx->wind_ev[k]));
  HIPCHK(hipEventRecord(ctx->wind_ev[k], ctx->stream));
  return GHIP_OK;
}
static void wind_dd_add_ms(ghip_ctx *ctx, int slot, int k)   // events k, k + 1, both complete
{
  float f = 0;
  if(ctx->wind_ev[k] && ctx->wind_ev[k + 1] && hipEventElapsedTime(&f, ctx->wind_ev[k], ctx->wind_ev[k + 1]) == hipSuccess)
    ctx->wind_ms[slot] += f;
}

// the own density partial of the list, the destinations, the position records on their way
static int wind_dd_density_send(ghip_ctx *ctx, int next_phase)
{
  DDState &D = ctx->dd;
  WindDD &W = D.wind;
  hipStream_t st = ctx->stream;
  const WindDev d = wind_dev(ctx, W.a.nwind > 0 ? W.a.nwind : 1);
  const int nw = W.a.nwind, m = W.m;
  const size_t Dn = (size_t) d.nw;
  const BoxK b = make_box(W.p.BoxSize, W.p.periodic);
  const int *list = wind_dd_list(d, W);
  const bool spread_only = W.form == GHIP_WIND_SPREAD_FORM;
  GCHK(wind_dd_mark(ctx, 2));
  if(m > 0 && !spread_only)
    {
      k_wind_density<<<cdiv(m, 64), 64, 0, st>>>(m, wind_own(ctx, d, list), WIND_TREE_ARGS, b, nullptr);
      HIPCHK(hipGetLastError());
    }
  GCHK(wind_dd_mark(ctx, 3));
  int total = 0;
  // (GHIP_WIND_DD_CUT=0, for measurements: select with the whole sphere Hsml; the results are the same)
  const bool cut = !(getenv("GHIP_WIND_DD_CUT") && atoi(getenv("GHIP_WIND_DD_CUT")) == 0);
  GCHK(ghip_dd_wind_select(ctx, m, list, d.idx, d.w + WP_DTJ * Dn, d.w + WP_DRMIN * Dn, !cut ? 0 : (spread_only ? 2 : 1), W.hmax_all,
                           W.p.BoxSize, W.p.periodic, &total));
  if(D.nranks > 1 && m > 0 && ctx->n > 0)   // (the selection waited for the device)
    {
      wind_dd_add_ms(ctx, WT_OWN, 2);
      if(W.iter > 0)
        wind_dd_add_ms(ctx, WT_MOVE, 0);
    }
  GCHK(ghip_ensure(ctx, D.du_send, (size_t) (total > 0 ? total : 1) * WIND_REC_DENS * 8));
  if(total > 0)
    {
      k_wind_pack<WIND_REC_DENS><<<cdiv(total, 256), 256, 0, st>>>(
        total, P<int>(D.du_list), P<int>(D.du_slot), ctx->n, P<double>(ctx->f[GHIP_F_POS]),
        P<double>(ctx->f[GHIP_F_HSML]), nw, d.w, P<double>(D.du_send));
      HIPCHK(hipGetLastError());
    }
  D.du_sent = total;
  W.sent += total;
  ghip_dd_set_alltoallv(D, D.du_send.p, (size_t) WIND_REC_DENS * 8, D.du_scount, D.du_soff, &D.du_recv);
  W.exchanges++;
  D.phase = next_phase;
  return 1;
}

// one more iteration: the move of the own list, then its density pass
static int wind_dd_iterate(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  WindDD &W = D.wind;
  hipStream_t st = ctx->stream;
  const WindDev d = wind_dev(ctx, W.a.nwind > 0 ? W.a.nwind : 1);
  W.iter++;
  W.bits += (W.iter == 1) ? W.m : W.under;
  GCHK(wind_dd_mark(ctx, 0));
  if(W.m > 0)
    {
      k_wind_move<<<cdiv(W.m, 256), 256, 0, st>>>(W.m, wind_dd_list(d, W), d.idx, ctx->n, P<double>(ctx->f[GHIP_F_POS]),
                                                  P<double>(ctx->f[GHIP_F_HSML]), P<double>(ctx->f[GHIP_F_MASS]), d.nw, d.w,
                                                  wind_k(&W.p));
      HIPCHK(hipGetLastError());
    }
  GCHK(wind_dd_mark(ctx, 1));
  return wind_dd_density_send(ctx, WDD_DENS_IMP);
}

// GHIP_WINDS_RESIDENT_FORM, the front end: this shard's list by the selection of ghip_winds_feedback over its active
// list into d.idx, W.a.nwind = its length (one read).  What the shard cannot do -- no table, a stale one, an active
// Type-3 particle without a row -- comes back as *own_rc with no list: the status record of the first all-gather
// carries it, and every shard stops in the next step.
static int wind_dd_resident_list(ghip_ctx *ctx, const char *who, int *own_rc)
{
  DDState &D = ctx->dd;
  WindDD &W = D.wind;
  RowTable &T = ctx->wk;
  hipStream_t st = ctx->stream;
  W.a.nwind = 0;
  *own_rc = ghip_winds_enter(ctx, who, true);
  if(*own_rc == GHIP_OK)
    *own_rc = ghip_rt_need(ctx, T, who, true);
  if(*own_rc != GHIP_OK)
    {
      const std::string why = ctx->err;
      *own_rc = ghip_fail(ctx, GHIP_EINVAL, "%s (rank %d of %d; either all shards hold a wind table, an empty one "
                          "counts, or the loop is GHIP_WIND_FORM with host arrays: ghip_dd_winds_set_table); nothing "
                          "was changed", why.c_str(), D.rank, D.nranks);
      return GHIP_OK;
    }
  const int nact = ctx->nactive < 0 ? ctx->n : ctx->nactive;
  const int *dact = ctx->nactive < 0 ? nullptr : P<int>(ctx->act_host_idx);
  if(nact <= 0)
    return GHIP_OK;
  RtWork R;
  GCHK(ghip_rt_work(ctx, T, (size_t) nact, 0, R, true));
  k_wk_flag_list<<<cdiv(nact, 256), 256, 0, st>>>(nact, dact, ctx->n, P<int>(ctx->f[GHIP_F_TYPE]), T.n,
                                                  P<unsigned int>(T.key), P<double>(T.rows), W.p.Time, R.a, R.words);
  HIPCHK(hipGetLastError());
  GCHK(ghip_select_flagged(ctx, dact, R.a, R.b, R.words + RTW_COUNT, nact, st));
  int w[RTW_WORDS];
  HIPCHK(hipMemcpyAsync(w, R.words, sizeof(w), hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  const int nw = w[RTW_COUNT];
  if(w[RTW_ERR])
    *own_rc = ghip_fail(ctx, GHIP_EINVAL, "%s: the active Type-3 particle %d of rank %d has no row in the shard's wind "
                        "table (%d rows); nothing was changed", who, w[RTW_ERRKEY], D.rank, T.n);
  else if(nw < 0 || nw > nact || nw > T.n)
    *own_rc = ghip_fail(ctx, GHIP_EDEVICE, "%s: a list of %d of %d active particles, %d rows (rank %d)", who, nw, nact,
                        T.n, D.rank);
  if(*own_rc != GHIP_OK || nw == 0)
    return GHIP_OK;
  const size_t Dn = (size_t) nw;
  GCHK(ghip_ensure(ctx, ctx->wind_idx, ((9 * Dn * 4 + 63) & ~(size_t) 63) + 64));
  HIPCHK(hipMemcpyAsync(ctx->wind_idx.p, R.b, Dn * 4, hipMemcpyDeviceToDevice, st));
  W.a.nwind = nw;
  return GHIP_OK;
}

// ... and the back end: the out planes and the code of the elimination into the rows (all == false: after a call
// that did not enter the loop, as ghip_winds_feedback); res != nullptr: what one thread adds in list order
static int wind_dd_store_rows(ghip_ctx *ctx, const WindDev &d, bool all, ghip_wind_result *res)
{
  RowTable &T = ctx->wk;
  hipStream_t st = ctx->stream;
  const int nw = d.nw;
  k_wk_store<<<cdiv(nw, 256), 256, 0, st>>>(nw, d.idx, T.n, P<unsigned int>(T.key), P<double>(T.rows), d.w, d.deleted,
                                            all);
  HIPCHK(hipGetLastError());
  if(res)
    {
      RtWork R;
      GCHK(ghip_rt_work(ctx, T, 1, 0, R, false));
      ghip_wind_result *dres = reinterpret_cast<ghip_wind_result *>(R.report), r;
      k_wk_result<<<1, 64, 0, st>>>(nw, d.deleted, d.w + WP_OLD * (size_t) nw, dres);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(&r, dres, sizeof(r), hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      res->ndeleted = r.ndeleted;
      res->deleted_momentum = r.deleted_momentum;
    }
  return GHIP_OK;
}

// the end of the loop on this shard: RAD_ACCEL and the elimination (not after max_iter), the state back
static int wind_dd_finish(ghip_ctx *ctx, bool noconv)
{
  DDState &D = ctx->dd;
  WindDD &W = D.wind;
  hipStream_t st = ctx->stream;
  const int nw = W.a.nwind;
  const WindDev d = wind_dev(ctx, nw > 0 ? nw : 1);
  const WindK K = wind_k(&W.p);
  ghip_wind_result *res = W.a.result;
  res->iterations = W.iter;
  res->bits = W.bits;
  if(!noconv)
    {
      if(W.p.rad_accel)
        {
          const int nact = ctx->nactive < 0 ? ctx->n : ctx->nactive;
          const int *act = ctx->nactive < 0 ? nullptr : P<int>(ctx->act_host_idx);
          if(nact > 0 && ctx->ngas > 0)
            k_wind_rad_accel<<<cdiv(nact, 256), 256, 0, st>>>(nact, act, ctx->ngas, P<int>(ctx->f[GHIP_F_TYPE]),
                                                              P<int>(ctx->f[GHIP_F_TIMEBIN]), P<double>(ctx->f[GHIP_F_MASS]),
                                                              P<double>(ctx->wind_inj), P<double>(ctx->wind_ra), K.dt_fac_gas);
        }
      if(nw > 0)
        k_wind_eliminate<<<cdiv(nw, 256), 256, 0, st>>>(nw, d.idx, ctx->n, P<double>(ctx->f[GHIP_F_POS]),
                                                        P<double>(ctx->f[GHIP_F_MASS]), d.w, d.deleted, K);
      HIPCHK(hipGetLastError());
    }
  if(nw > 0 && W.resident)
    GCHK(wind_dd_store_rows(ctx, d, true, res));
  else if(nw > 0)
    {
      const ghip_wind_state *s = W.a.state;
      GCHK(wind_download_state(ctx, d, s, true));
      for(int a = 0; a < nw; a++)   // :558-559, in list order
        if(s->deleted[a])
          {
            res->ndeleted++;
            if(s->deleted[a] == 1)
              res->deleted_momentum += s->old_momentum[a];
          }
    }
  HIPCHK(ghip_stream_sync(ctx, st));
  wind_dd_counts(D);
  if(noconv)
    return ghip_fail(ctx, GHIP_ENOCONV, "%s: %lld wind particles still under way after max_iter = %d iterations",
                     wind_dd_who(W.form, W.resident), W.under_all, W.p.max_iter);
  return 0;
}

int ghip_dd_wind_step(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  WindDD &W = D.wind;
  hipStream_t st = ctx->stream;
  if(W.form == GHIP_WINDS_SPAWN_FORM)
    return ghip_dd_spawn_step(ctx);
  const char *who = wind_dd_who(W.form, W.resident);
  int list_rc = GHIP_OK;
  std::string list_msg;
  if(D.phase == WDD_GROUPS && W.resident)
    {
      GCHK(wind_dd_resident_list(ctx, who, &list_rc));
      list_msg = ctx->err;
    }
  const int nw = W.a.nwind, n = ctx->n;
  const size_t Dn = (size_t) (nw > 0 ? nw : 1);
  const BoxK b = make_box(W.p.BoxSize, W.p.periodic);
  if(D.phase == WDD_GROUPS)
    {
      // the arrays are made for one particle at least: a shard without wind still holds the words
      GCHK(ghip_ensure(ctx, ctx->wind_idx, ((9 * Dn * 4 + 63) & ~(size_t) 63) + 64));
      GCHK(ghip_ensure(ctx, ctx->wind_work, (WIND_NPLANES * Dn + 2 * (Dn + 1)) * 8 + 256));
      GCHK(ghip_ensure(ctx, D.du_slot, (size_t) (n > 0 ? n : 1) * 4));
      const WindDev d = wind_dev(ctx, (int) Dn);
      HIPCHK(hipMemsetAsync(d.words, 0, sizeof(WindWords), st));
      if(nw > 0)
        {
          if(!W.resident)   // (the resident list stands there already)
            HIPCHK(hipMemcpyAsync(d.idx, W.a.wind_idx, Dn * 4, hipMemcpyHostToDevice, st));
          GCHK(wind_tree_order(ctx, d, st));
          k_wind_vel<<<cdiv(nw, 256), 256, 0, st>>>(nw, d.idx, n, P<int>(ctx->f[GHIP_F_TYPE]), P<double>(ctx->f[GHIP_F_VEL]),
                                                    d.w, d.words);
          HIPCHK(hipGetLastError());
          GCHK(ghip_list_slots(ctx, nw, d.idx, P<int>(D.du_slot), st));
        }
      if(ctx->ngas > 0)
        k_wind_hmax<<<cdiv(ctx->ngas, 256), 256, 0, st>>>(ctx->ngas, P<double>(ctx->f[GHIP_F_HSML]),
                                                          P<double>(ctx->f[GHIP_F_MASS]), P<int>(ctx->f[GHIP_F_TYPE]), d.words);
      HIPCHK(hipGetLastError());
      if(nw > 0 && W.form == GHIP_WIND_FORM)
        {
          if(W.resident)
            {
              k_wk_load<<<cdiv(nw, 256), 256, 0, st>>>(nw, d.idx, ctx->wk.n, P<unsigned int>(ctx->wk.key),
                                                       P<double>(ctx->wk.rows), d.w);
              HIPCHK(hipGetLastError());
            }
          else
            {
              const ghip_wind_state *s = W.a.state;
              std::vector<double> h(WIND_NIN * Dn);
              memcpy(h.data() + WP_AGE * Dn, s->stellar_age, Dn * 8);
              memcpy(h.data() + WP_BIRTH * Dn, s->birth_energy, Dn * 8);
              memcpy(h.data() + WP_OLD * Dn, s->old_momentum, Dn * 8);
              memcpy(h.data() + WP_RHO * Dn, s->new_density, Dn * 8);
              memcpy(h.data() + WP_DRMIN * Dn, s->drmin, Dn * 8);
              HIPCHK(hipMemcpyAsync(d.w, h.data(), h.size() * 8, hipMemcpyHostToDevice, st));
              HIPCHK(ghip_stream_sync(ctx, st));   // (h leaves scope)
            }
          k_wind_init<<<cdiv(nw, 256), 256, 0, st>>>(nw, d.idx, P<int>(ctx->f[GHIP_F_TIMEBIN]), d.w, d.deleted, W.p.dt_fac);
          k_wind_sum<<<1, 1024, 0, st>>>(nw, d.w + WP_DTJ * Dn, &d.words->dt_total);
          k_wind_flags<<<cdiv(nw, 256), 256, 0, st>>>(nw, d.ord, d.w + WP_DTJ * Dn, d.flags, d.words);
          HIPCHK(hipGetLastError());
          GCHK(ghip_select_flagged(ctx, d.ord, d.flags, d.lista, &d.words->npos, nw, st));
        }
      else if(nw > 0)
        {
          HIPCHK(hipMemcpyAsync(d.w + WP_DTJ * Dn, W.a.dt_jump, Dn * 8, hipMemcpyHostToDevice, st));
          if(W.form == GHIP_WIND_SPREAD_FORM)
            {
              HIPCHK(hipMemcpyAsync(d.w + WP_RHO * Dn, W.a.new_density, Dn * 8, hipMemcpyHostToDevice, st));
              HIPCHK(hipMemcpyAsync(d.w + WP_DMOM * Dn, W.a.delta_momentum, Dn * 8, hipMemcpyHostToDevice, st));
            }
        }
      WindWords h;
      HIPCHK(hipMemcpyAsync(&h, d.words, sizeof(h), hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      // what this shard met travels with the group tables: every shard stops in the next step (ghip_dd_hold's path)
      int own_rc = list_rc;
      if(own_rc != GHIP_OK)
        ctx->err = list_msg;   // (the selection's own message is the shard's)
      else if(h.err)
        own_rc = wind_type_error(ctx, who);
      else if(W.form == GHIP_WIND_FORM && (h.npos < 0 || h.npos > nw))
        own_rc = ghip_fail(ctx, GHIP_EDEVICE, "%s: a list of %d of %d particles", who, h.npos, nw);
      W.m = W.form == GHIP_WIND_FORM ? h.npos : nw;
      W.under = h.nunder;
      W.cur = 0;
      const double extra[3] = {__builtin_bit_cast(double, h.hmax), h.dt_total, (double) nw};
      D.phase = WDD_START;
      W.exchanges++;
      return ghip_dd_wind_groups(ctx, extra, own_rc);
    }
  const WindDev d = wind_dev(ctx, (int) Dn);
  if(D.phase == WDD_START)
    {
      double extra[3 * GHIP_MAXRANKS];
      // (in the resident form a failing shard's code travels in its status record: the other shards return it too)
      GCHK(ghip_dd_wind_status(ctx, who, extra));
      double hmax = 0, dt_total = 0;
      for(int r = 0; r < D.nranks; r++)   // (the sum in ascending rank order: the same bits on every shard)
        {
          if(extra[3 * r] > hmax)
            hmax = extra[3 * r];
          dt_total += extra[3 * r + 1];
        }
      W.hmax_all = hmax;
      if(W.form == GHIP_WIND_FORM)
        {
          if(dt_total <= W.p.dt_total_floor)   // :302: the loop is not entered, nothing changes on any shard
            {
              if(nw > 0 && W.resident)
                {
                  GCHK(wind_dd_store_rows(ctx, d, false, nullptr));
                  HIPCHK(ghip_stream_sync(ctx, st));
                }
              else if(nw > 0)
                GCHK(wind_download_state(ctx, d, W.a.state, false));
              wind_dd_counts(D);
              return 0;
            }
          GCHK(wind_injected(ctx, who));
          if(W.p.rad_accel)
            GCHK(wind_rad_accel(ctx, who));
          ctx->pot_n = -1;   // (positions and masses change)
        }
      else if(W.form == GHIP_WIND_SPREAD_FORM)
        {
          GCHK(wind_injected(ctx, who));
          return wind_dd_density_send(ctx, WDD_SPREAD_POS);
        }
      if(nw > 0)
        {
          k_wind_reset<<<cdiv(nw, 256), 256, 0, st>>>(nw, d.w);
          HIPCHK(hipGetLastError());
        }
      return wind_dd_density_send(ctx, WDD_DENS_IMP);
    }
  if(D.phase == WDD_DENS_IMP)
    {
      // the imported particles against this shard's gas; the partials go home over the receive layout
      const int nimp = D.x.rtotal;
      W.nimp = nimp;
      W.recvd += nimp;
      GCHK(ghip_ensure(ctx, D.du_part, (size_t) (nimp > 0 ? nimp : 1) * 16));
      GCHK(wind_dd_mark(ctx, 4));
      if(nimp > 0)
        {
          k_wind_density<<<cdiv(nimp, 64), 64, 0, st>>>(
            nimp, wind_imp(ctx, d, P<double>(D.du_recv), nullptr, P<double>(D.du_part)), WIND_TREE_ARGS, b, nullptr);
          HIPCHK(hipGetLastError());
        }
      int sc[GHIP_MAXRANKS], so[GHIP_MAXRANKS];
      for(int r = 0; r < D.nranks; r++)
        {
          sc[r] = D.x.rcount[r];
          so[r] = D.x.roff[r];
        }
      GCHK(wind_dd_mark(ctx, 5));
      ghip_dd_set_alltoallv(D, D.du_part.p, 16, sc, so, &D.du_back);
      W.exchanges++;
      D.phase = WDD_DENS_ADD;
      return 1;
    }
  if(D.phase == WDD_DENS_ADD)
    {
      for(int r = 0; r < D.nranks; r++)
        if(D.x.rcount[r] != (r == D.rank ? 0 : D.du_scount[r]))
          return ghip_fail(ctx, GHIP_ECOMM, "%s: %d partial sums came back from rank %d, %d particles went there", who,
                           D.x.rcount[r], r, D.du_scount[r]);
      for(int r = 0; r < D.nranks; r++)   // own sum first, then the ranks in ascending order (virtual_density.c:344)
        if(r != D.rank && D.du_scount[r] > 0)
          k_wind_add_parts<<<cdiv(D.du_scount[r], 256), 256, 0, st>>>(D.du_scount[r], P<int>(D.du_list) + D.du_soff[r],
                                                                      P<int>(D.du_slot),
                                                                      P<double>(D.du_back) + 2 * (size_t) D.x.roff[r], d.nw, d.w);
      HIPCHK(hipGetLastError());
      if(W.form == GHIP_WIND_DENSITY_FORM)
        {
          if(nw > 0)
            {
              // (WP_RHO and WP_DRMIN are neighbours)
              std::vector<double> o(2 * Dn);
              HIPCHK(hipMemcpyAsync(o.data(), d.w + WP_RHO * Dn, 2 * Dn * 8, hipMemcpyDeviceToHost, st));
              HIPCHK(ghip_stream_sync(ctx, st));
              memcpy(W.a.new_density, o.data(), Dn * 8);
              memcpy(W.a.drmin, o.data() + Dn, Dn * 8);
            }
          HIPCHK(ghip_stream_sync(ctx, st));
          wind_dd_counts(D);
          return 0;
        }
      if(W.iter == 0)   // that was the density at the start
        return wind_dd_iterate(ctx);
      // the new list, and what every shard needs to know of it
      const int m = W.m;
      if(ctx->wind_ev[5])   // (the exchange of the partials lies behind them)
        HIPCHK(hipEventSynchronize(ctx->wind_ev[5]));
      wind_dd_add_ms(ctx, WT_IMP, 4);
      GCHK(wind_dd_mark(ctx, 6));
      HIPCHK(hipMemsetAsync(d.words, 0, 16, st));   // npairs, npos, nunder
      if(m > 0)
        {
          k_wind_flags<<<cdiv(m, 256), 256, 0, st>>>(m, wind_dd_list(d, W), d.w + WP_DTJ * Dn, d.flags, d.words);
          HIPCHK(hipGetLastError());
          GCHK(ghip_select_flagged(ctx, wind_dd_list(d, W), d.flags, wind_dd_list(d, W, true), &d.words->npos, m, st));
        }
      GCHK(wind_dd_mark(ctx, 7));
      WindWords h;
      HIPCHK(hipMemcpyAsync(&h, d.words, sizeof(h), hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      wind_dd_add_ms(ctx, WT_LIST, 6);
      bool failed = false;
      if(h.npos < 0 || h.npos > m)
        failed = ghip_dd_hold(ctx, ghip_fail(ctx, GHIP_EDEVICE, "%s: a list of %d of %d particles", who, h.npos, m));
      else
        ghip_dd_hold(ctx, GHIP_OK);
      W.m_next = failed ? 0 : h.npos;
      W.under_next = failed ? 0 : h.nunder;
      const double mine[4] = {(double) W.m_next, (double) W.under_next, failed ? 1.0 : 0.0, 0.0};
      GCHK(ghip_ensure(ctx, D.status_own, 32));
      HIPCHK(hipMemcpyAsync(D.status_own.p, mine, 32, hipMemcpyHostToDevice, st));
      HIPCHK(ghip_stream_sync(ctx, st));   // (`mine` lives on this frame)
      ghip_dd_set_allgather(D, D.status_own.p, 32, &D.status_all);
      W.exchanges++;
      D.phase = WDD_STATUS;
      return 1;
    }
  if(D.phase == WDD_STATUS)
    {
      double all[4 * GHIP_MAXRANKS];
      HIPCHK(hipMemcpyAsync(all, D.status_all.p, (size_t) D.nranks * 32, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      int first_failed = -1;
      W.under_all = 0;
      for(int r = 0; r < D.nranks; r++)
        {
          if(all[4 * r + 2] != 0 && first_failed < 0)
            first_failed = r;
          W.under_all += (long long) all[4 * r + 1];
        }
      GCHK(ghip_dd_raise(ctx, first_failed, "%s: shard %d reported an error in iteration %d (its own message says what); "
                         "every shard stops here", who, first_failed, W.iter));
    }
  if(D.phase == WDD_STATUS || D.phase == WDD_SPREAD_POS)
    {
      if(D.phase == WDD_SPREAD_POS)
        {
          W.nimp = D.x.rtotal;
          W.recvd += W.nimp;
        }
      // the spread records of the particles that went out, to the same shards in the same order
      const int total = D.du_sent;
      GCHK(ghip_ensure(ctx, D.wd_spread, (size_t) (total > 0 ? total : 1) * WIND_REC_SPREAD * 8));
      if(total > 0)
        {
          k_wind_pack<WIND_REC_SPREAD><<<cdiv(total, 256), 256, 0, st>>>(
            total, P<int>(D.du_list), P<int>(D.du_slot), n, P<double>(ctx->f[GHIP_F_POS]), P<double>(ctx->f[GHIP_F_HSML]),
            d.nw, d.w, P<double>(D.wd_spread));
          HIPCHK(hipGetLastError());
        }
      ghip_dd_set_alltoallv(D, D.wd_spread.p, (size_t) WIND_REC_SPREAD * 8, D.du_scount, D.du_soff, &D.wd_srecv);
      W.exchanges++;
      D.phase = WDD_SPREAD;
      return 1;
    }
  if(D.phase == WDD_SPREAD)
    {
      const int nimp = W.nimp, m = W.m;
      if(D.x.rtotal != nimp)
        return ghip_fail(ctx, GHIP_ECOMM, "%s: %d spread records came for %d imported particles", who, D.x.rtotal, nimp);
      // this shard's particles in list order (slots [0, nw)), then the imported ones in receive order (nw + t)
      const size_t M = (size_t) m + (size_t) nimp;
      GCHK(ghip_ensure(ctx, D.wd_cnt, 2 * (M + 1) * 8));
      unsigned long long *cnt = P<unsigned long long>(D.wd_cnt), *off = cnt + M + 1;
      const WindOwn own = wind_own(ctx, d, wind_dd_list(d, W));
      const WindImp imp = wind_imp(ctx, d, P<double>(D.du_recv), P<double>(D.wd_srecv), nullptr);
      GCHK(wind_dd_mark(ctx, 4));
      HIPCHK(hipMemsetAsync(cnt, 0, (M + 1) * 8, st));
      if(m > 0)
        k_pairs<0><<<cdiv(m, 64), 64, 0, st>>>(m, own, WIND_TREE_ARGS, b, cnt, nullptr, 0ULL, nullptr, nullptr);
      if(nimp > 0)
        k_pairs<0><<<cdiv(nimp, 64), 64, 0, st>>>(nimp, imp, WIND_TREE_ARGS, b, cnt + m, nullptr, 0ULL, nullptr, nullptr);
      HIPCHK(hipGetLastError());
      GCHK(ghip_scan<unsigned long long>(ctx, cnt, off, (int) M + 1, st));
      unsigned long long tot[2];
      HIPCHK(hipMemcpyAsync(&tot[0], off + m, 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(&tot[1], off + M, 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));   // (the pair count sizes the sort)
      W.imp_pairs += (long long) (tot[1] - tot[0]);
      GCHK(wind_scatter(ctx, d, b, m, own.list, (long long) tot[1], off, nimp, &imp));
      GCHK(wind_dd_mark(ctx, 5));
      HIPCHK(hipEventSynchronize(ctx->wind_ev[5]));
      wind_dd_add_ms(ctx, WT_SPREAD, 4);
      if(W.form == GHIP_WIND_SPREAD_FORM)
        {
          HIPCHK(ghip_stream_sync(ctx, st));
          wind_dd_counts(D);
          return 0;
        }
      W.cur ^= 1;
      W.m = W.m_next;
      W.under = W.under_next;
      if(W.under_all == 0)
        return wind_dd_finish(ctx, false);
      if(W.iter >= W.p.max_iter)   // (the global count: all shards stop together)
        return wind_dd_finish(ctx, true);
      return wind_dd_iterate(ctx);
    }
  return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_step: the wind operation has no phase %d", D.phase);
}
