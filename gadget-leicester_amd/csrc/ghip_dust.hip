// ghip_dust.hip -- the dust-gas drag passes of the reference's shipped flag bundle (DUST, DUST_TIMESTEP,
// DUST_POWERLAW, DOUBLEPRECISION, CONSTANT_MEAN_MOLECULAR_WEIGHT), called by compute_accelerations()
// right after blackhole_accretion() (accel.c:194, 198).  The physics switches DUST_GROWTH,
// DUST_REAL_PEBBLE_COLLISIONS, DUST_VAPORIZE, DUST_FE_AND_ICE_GRAINS, DUST_EPSTEIN and
// DUST_NO_FRICTION_HEATING are a run-time setting of the context (ghip_set_dust_model): kernel
// instantiations of their own, the default ones untouched.  Not built: DUST_TWO_POPULATIONS,
// DUST_GROWTH_FIXED_SIZE, DUST_MDUST_GROW, DUST_2ND_POPULATION, DUST_PEBBLES_BORN, DUST_SINK_ON_FLY.
//
// Replaces the particle loops of
//   dust_density / dust_evaluate_density         dust.c:60-261, 748-887
//   dust_drag, the per-grain update              dust.c:263-446 (:449-609 with ghip_set_dust_model)
//   dust_drag / dust_evaluate_select (scatter)   dust.c:889-1029
//   ngb_treefind_dust_active                     dust.c:1235-1333
//
// Grains can be a sizeable fraction of all particles, so a grain is a THREAD, not a wavefront: the
// grains of a launch are ordered by their place in the gravity tree (a radix sort of the tree's
// inverse permutation), which makes the walks of the 64 lanes of a wavefront neighbours in space.
//
// The scatter into the gas is order dependent (the entropy update is multiplicative, with a floor and a
// cap): for each gas particle the reference applies the grains in the order of the active list.  That is the
// ordered pair scatter of ghip_pairs.h; this file gives it the dust-gas pair (DustTarget) and
// what a gas particle does with its run of grains (k_dust_apply).  Every sum is a per-thread loop in a fixed
// order: two identical calls give identical bits.
#include "ghip_pairs.h"

#define DUST_RHO_GRAIN 3.           // rho_dust, dust.c:379

// per-grain planes of the staging buffer ([DUST_NPLANES][nd] doubles)
enum
{
  DP_RHO = 0,   // in   d1.DUST_Density
  DP_ENT,       // in   d2.DUST_Entropy
  DP_GV,        // in   d3.DUST_SurroundingGasVel [3]
  DP_RAD = DP_GV + 3,   // in   DustRadius
  DP_D7,        // in   d7.DUST_particle_density
  DP_D9,        // in/out d9.DUST_particle_velocity [3]
  DP_VCOLL = DP_D9 + 3, // in/out DustVcoll
  DP_DMOM,      // out  DeltaDustMomentum [3]
  DP_DE = DP_DMOM + 3,  // out  DeltaDragEnergy
  DUST_NPLANES
};
#define DUST_NIN (DP_VCOLL + 1)       // planes uploaded
#define DUST_NOUT (DUST_NPLANES - DP_D9)   // planes read back: d9, vcoll, dmom, dE

struct DustK
{
  BoxK b;
  double dt_fac, dt_fac_gas, minegy, meanweight, ulength, umass, udens, uvel;
};

// ghip_set_dust_model: what the k_dust_grain<DustM> instantiation gets beyond DustK.  Wave-uniform: every
// test of a switch is a scalar branch.
#define DUST_A_MIN 0.1     // adust_min, adust_max [cm], dust.c:277
#define DUST_A_MAX 1.e5
struct DustM
{
  int growth, pebble, vaporize, fe_ice, epstein, no_heat;
  int gate;            // All.Time > 0 && All.Time > All.VirtualTime (dust.c:453)
  double vfrag, a_init, uenergy;
  const int *id;       // GHIP_F_ID (fe_ice)
  double *logr;        // LogDustRadius_by_dt [nd] in list order, or nullptr
};

// DUST_REAL_PEBBLE_COLLISIONS in the density pass: the velocities gathered, and where grain a's four sums
// (d7, d9 [3]) go: o[a * sa + c * sc] -- planes for a shard's own list, records of four for imported grains
struct DustVel
{
  const double *vel;
  double *o;
  size_t sa, sc;
};

template <class T>
__device__ __forceinline__ const T &d_only(const T &t)
{
  return t;
}

// the neighbour test and kernel weight of dust_evaluate_density / _select (dust.c:826-847, 971-983):
// r <= h from the tree search, then u = r / h < 1.  Returns false for a non-neighbour.
__device__ __forceinline__ bool d_dust_weight(double px, double py, double pz, double qx, double qy,
                                              double qz, double h, const BoxK b, double &wk)
{
  const double dx = d_wrap(px - qx, b), dy = d_wrap(py - qy, b), dz = d_wrap(pz - qz, b);
  const double r2 = dx * dx + dy * dy + dz * dz;
  if(r2 > h * h)
    return false;
  const double u = sqrt(r2) / h;
  if(!(u < 1))
    return false;
  const double hinv = 1 / h;
  wk = d_spline_wk(u, hinv * hinv * hinv);
  return true;
}

// Where a grain of a launch comes from: this shard's list (a local particle: position and h from the
// resident fields) ...
struct DustGrainLocal
{
  const int *idx;              // list slot -> local particle index
  const double *pos, *hsml;
  int n;
  const double *wi;            // the per-grain value by particle (MASS), or
  const double *wa;            // ... by list slot (the DUST_Density plane)
  __device__ __forceinline__ void get(int a, double &x, double &y, double &z, double &h, double &w) const
  {
    const int i = idx[a];
    x = pos[i];
    y = pos[(size_t) n + i];
    z = pos[2 * (size_t) n + i];
    h = hsml[i];
    w = wi ? wi[i] : wa[a];
  }
};

// ... or a record another shard sent: {x, y, z, h, w, ...}, `stride` doubles each (w: the grain's mass in
// the density pass, its DUST_Density in the drag pass)
struct DustGrainRec
{
  const double *rec;
  int stride;
  __device__ __forceinline__ void get(int a, double &x, double &y, double &z, double &h, double &w) const
  {
    const double *r = rec + (size_t) a * stride;
    x = r[0];
    y = r[1];
    z = r[2];
    h = r[3];
    w = r[4];
  }
};

// dust_evaluate_density (dust.c:748-887): the Type-2 neighbours with Mass > 0 within the grain's h,
// the grain itself included, each weighted with the GRAIN's own mass (dust.c:849: `dustmass` is
// PPP[target].Mass -- a reference quirk kept as it is: the result is m_i * sum_j W_ij, not a density of
// the neighbours' mass; an imported grain brings its mass in the record).  Candidates are this context's
// own particles: imported elements of a shard's merged tree (perm >= n) are skipped.  ord: the launch
// order of the grains (nullptr: as given).  V... is empty for the default kernel (same signature, same code
// as before ghip_set_dust_model existed) and one DustVel for DUST_REAL_PEBBLE_COLLISIONS: d9[k] += m_i W
// Vel_j[k] over the same neighbours (dust.c:851-853), the four sums written through the DustVel
template <class G, class... V>
__global__ void __launch_bounds__(64)
k_dust_density(int nd, const int *__restrict__ ord, G g, int n, const double *__restrict__ pos,
               const double *__restrict__ mass, const int *__restrict__ type, int nelem,
               const int4 *__restrict__ lk, const double4 *__restrict__ cl, const int *__restrict__ perm,
               BoxK b, double *__restrict__ out, V... v)
{
  constexpr bool VELS = sizeof...(V) > 0;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if(t >= nd)
    return;
  const int a = ord ? ord[t] : t;
  double px, py, pz, h, mi;
  g.get(a, px, py, pz, h, mi);
  double rho = 0;
  if constexpr(VELS)
    {
      const DustVel &dv = d_only(v...);
      const double *__restrict__ vel = dv.vel;
      double s0 = 0, s1 = 0, s2 = 0;
      d_ngb_walk_thread<PAIR_LEAF>(GravElems{lk, cl}, nelem, px, py, pz, h, b, [&](int p) {
        const int j = perm[p];
        if(j < 0 || j >= n || type[j] != 2 || !(mass[j] > 0))
          return;
        double wk;
        if(d_dust_weight(px, py, pz, pos[j], pos[(size_t) n + j], pos[2 * (size_t) n + j], h, b, wk))
          {
            const double mw = mi * wk;
            rho += mw;
            s0 += mw * vel[j];
            s1 += mw * vel[(size_t) n + j];
            s2 += mw * vel[2 * (size_t) n + j];
          }
      });
      double *o = dv.o + (size_t) a * dv.sa;
      o[0] = rho;
      o[dv.sc] = s0;
      o[2 * dv.sc] = s1;
      o[3 * dv.sc] = s2;
    }
  else
    {
      d_ngb_walk_thread<PAIR_LEAF>(GravElems{lk, cl}, nelem, px, py, pz, h, b, [&](int p) {
        const int j = perm[p];
        if(j < 0 || j >= n || type[j] != 2 || !(mass[j] > 0))
          return;
        double wk;
        if(d_dust_weight(px, py, pz, pos[j], pos[(size_t) n + j], pos[2 * (size_t) n + j], h, b, wk))
          rho += mi * wk;
      });
      out[a] = rho;
    }
}

// dust_drag, the per-grain part (dust.c:303-446), one thread per grain of the list.  M... is empty for the
// default kernel (same signature, same code as before ghip_set_dust_model existed) and one DustM for the
// instantiation with the switches, which goes on to dust.c:449-609: growth and fragmentation, vaporisation
// of rock and ice, the radius update with its clamps and the latent heat
template <class... M>
__global__ void k_dust_grain(int nd, const int *__restrict__ idx, int n, const int *__restrict__ timebin,
                             const double *__restrict__ mass, const double *__restrict__ grav,
                             double *__restrict__ vel, double *__restrict__ w, DustK K, M... m)
{
  constexpr bool MODEL = sizeof...(M) > 0;
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nd)
    return;
  const int i = idx[a];
  const size_t N = (size_t) n, D = (size_t) nd;
#define PL(q) w[(size_t) (q) * D + a]
  const int tb = timebin[i];
  const double dt = (tb ? (double) (1 << tb) : 0.0) * K.dt_fac;
  const double rho = PL(DP_RHO);
  const double soundspeed = sqrt(8. / M_PI * PL(DP_ENT) * pow(rho, GAMMA_MINUS1));
  double v[3], gv[3], g[3];
  for(int k = 0; k < 3; k++)
    {
      v[k] = vel[k * N + i];
      gv[k] = PL(DP_GV + k);
      g[k] = grav[k * N + i];
    }
  const double delta_vel = sqrt((v[0] - gv[0]) * (v[0] - gv[0]) + (v[1] - gv[1]) * (v[1] - gv[1]) +
                                (v[2] - gv[2]) * (v[2] - gv[2]));
  const double d7 = PL(DP_D7);
  double vcoll = PL(DP_VCOLL);
  for(int k = 0; k < 3; k++)
    PL(DP_DMOM + k) = 0.;
  double de = 0.;
  if(d7 > 0.)   // dust.c:366-376: d9 divided in place
    {
      double d9[3];
      for(int k = 0; k < 3; k++)
        {
          d9[k] = PL(DP_D9 + k) / d7;
          PL(DP_D9 + k) = d9[k];
        }
      const double dpv = sqrt((v[0] - d9[0]) * (v[0] - d9[0]) + (v[1] - d9[1]) * (v[1] - d9[1]) +
                              (v[2] - d9[2]) * (v[2] - d9[2]));
      vcoll = dpv * K.uvel / 1.e2 + 1.e-30;
    }
  if(dt > 0)   // dust.c:385-444
    {
      const double R = PL(DP_RAD);
      const double lambda_h2 = K.meanweight * PROTONMASS / (K.udens * rho) / 1.e-15 / K.ulength;
      const double rey = 6 * delta_vel * R / K.ulength / (lambda_h2 * soundspeed);
      double ts;
      bool epstein = 3. / 2 * lambda_h2 * K.ulength >= R;
      if constexpr(MODEL)
        epstein = epstein || d_only(m...).epstein;   // DUST_EPSTEIN, dust.c:415-416
      if(epstein)   // Epstein
        ts = 1. / (rho * soundspeed / (DUST_RHO_GRAIN * R) * K.umass / K.ulength / K.ulength);
      else if(delta_vel > 0)   // Stokes, C_drag of Weidenschilling 1977
        {
          double C_drag = 0.;
          if(rey >= 800.)
            C_drag = 0.44;
          if(rey < 800. && rey >= 1.)
            C_drag = 24. * pow(rey, -0.6);
          if(rey < 1.)
            C_drag = 24. / rey;
          ts = DUST_RHO_GRAIN * R / (rho * delta_vel) / K.umass * K.ulength * K.ulength;
          ts *= 8. / 3. / C_drag;
        }
      else
        ts = 0.66667 / (rho * soundspeed / (DUST_RHO_GRAIN * R)) / K.umass * K.ulength * R / lambda_h2;
      const double e1 = exp(-dt / ts), e2 = exp(-2. * dt / ts);
      for(int k = 0; k < 3; k++)
        {
          const double vold = v[k];
          const double vsteady = (vold * d7 + gv[k] * rho) / (d7 + rho + 1.e-30);
          const double vnew = vsteady + (vold - vsteady) * e1 + g[k] * ts * (1. - e1);
          const double vnew_nog = vold + g[k] * dt;
          PL(DP_DMOM + k) = 0. - mass[i] * (vnew_nog - vnew);
          if constexpr(MODEL)
            {
              if(!d_only(m...).no_heat)   // DUST_NO_FRICTION_HEATING, dust.c:433-435
                de += mass[i] * ((vnew - vsteady) * (vnew - vsteady)) * (1. - e2) / 2.;
            }
          else
            de += mass[i] * ((vnew - vsteady) * (vnew - vsteady)) * (1. - e2) / 2.;
          vel[k * N + i] = vnew;
        }
      vcoll = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]) * ts * K.uvel / 1.e2;
      vcoll += 0.2;
    }
  if constexpr(MODEL)
    {
      const DustM &mm = d_only(m...);
      if(mm.growth)   // dust.c:451-609 (vaporize needs growth: ghip_set_dust_model)
        {
          const double old_a = PL(DP_RAD);
          double adot = 0.;
          if(mm.gate && d7 > 0.)   // :453, 461: with the FINAL DustVcoll of this call
            {
              const double t_coll = 4. * (DUST_RHO_GRAIN / K.udens) * (old_a / K.ulength) / d7 /
                                    (vcoll * 1.e2 / K.uvel + 1.e-20);
              if(mm.logr)
                mm.logr[a] = t_coll;
              adot = old_a / K.ulength / 3. / t_coll;
              if(mm.pebble)   // growth turns into fragmentation at high collision speeds, :479-490
                {
                  if(mm.vfrag < 0.1)
                    adot = 0.;
                  else
                    {
                      const double xcoll = vcoll / mm.vfrag;
                      adot *= (1 - xcoll * xcoll) / (1 + xcoll * xcoll);
                    }
                }
            }
          double latent = 1.e11;   // rocks, erg/g (:268)
          if(mm.vaporize)
            {
              const bool ice = mm.fe_ice && (mm.id[i] & 1);   // P[].ID % 2, :509
              if(ice)
                latent = 4.e10;
              if(rho > 0.)   // :501
                {
                  const double csu = soundspeed * K.uvel;
                  const double T = M_PI / 8. * (csu * csu) * K.meanweight * PROTONMASS / BOLTZMANN;
                  double pvap;
                  if(!ice)
                    pvap = pow(10., (-24605. / T + 13.176));   // rocks, Podolak et al 1988
                  else if(T <= 600.)
                    pvap = pow(10., (11.6 - 2104. / T));
                  else
                    pvap = 5. + 5.2e-3 * T;
                  adot -= 1. / (DUST_RHO_GRAIN * sqrt(2. * 3.1415)) / soundspeed / K.uvel * pvap / K.uvel;
                }
            }
          double new_a = old_a + (adot * dt) * K.ulength;   // :551
          if(new_a < DUST_A_MIN)   // :566-567, for every grain of the list
            new_a = DUST_A_MIN;
          if(new_a > DUST_A_MAX)
            new_a = DUST_A_MAX;
          PL(DP_RAD) = new_a;
          if(mm.vaporize)   // :533-548, 591-608: takes heat from the gas where grains vaporise
            {
              const double old_l = latent * (old_a - DUST_A_MIN) / (mm.a_init - DUST_A_MIN);
              const double new_l = latent * (new_a - DUST_A_MIN) / (mm.a_init - DUST_A_MIN);
              de += (new_l - old_l) * mass[i] * K.umass / mm.uenergy;
            }
        }
    }
  PL(DP_DE) = de;
  PL(DP_VCOLL) = vcoll;
#undef PL
}

// The dust-gas pair of dust_evaluate_select (dust.c:962-1000) as a Target of k_pairs (ghip_pairs.h): the gas
// neighbours a grain updates are Type 0, Mass > 0, u < 1 with the gas particle's own dt > 0 -- this context's own
// gas only (a shard's ghosts, j >= ngas, are skipped) -- searched at the grain's h ...
struct DustGas
{
  int n, ngas;
  const double *pos, *mass;
  const int *type, *timebin;
  __device__ __forceinline__ bool pair(int j, double px, double py, double pz, double h, const BoxK b, double &wk) const
  {
    if(j < 0 || j >= ngas || type[j] != 0 || !(mass[j] > 0) || timebin[j] == 0)
      return false;
    return d_dust_weight(px, py, pz, pos[j], pos[(size_t) n + j], pos[2 * (size_t) n + j], h, b, wk);
  }
};

// ... and the grain has its DUST_Density > 0.  G: DustGrainLocal, launched in the tree order ord, or DustGrainRec
// (ord == nullptr); grain a takes slot obase + a
template <class G>
struct DustTarget : DustGas
{
  G g;
  const int *ord;
  int obase;
  __device__ __forceinline__ bool get(int t, int &slot, double &x, double &y, double &z, double &h, double &rs) const
  {
    const int a = ord ? ord[t] : t;
    double grho;
    g.get(a, x, y, z, h, grho);
    slot = obase + a;
    rs = h;
    return grho > 0.;
  }
};

#define DUST_REC_DENS 5   // x, y, z, Hsml, Mass
#define DUST_REC_DRAG 9   // x, y, z, Hsml, DUST_Density, DeltaDustMomentum [3], DeltaDragEnergy

// the update of one gas particle by the grains of its run of sorted pairs, in slot order (dust.c:987-996): this
// context's grains, slots [0, nd), from the planes w; then a shard's nimp imported ones, slots nd + t, from their
// drag records
__global__ void k_dust_apply(long long npairs, const unsigned long long *__restrict__ key,
                             const double *__restrict__ wgt, int nd, const double *__restrict__ w, int nimp,
                             const double *__restrict__ rec, int n, int ngas, const double *__restrict__ mass,
                             const int *__restrict__ timebin, double *__restrict__ vel,
                             double *__restrict__ entropy, double *__restrict__ heat, DustK K)
{
  const long long s0 = (long long) blockIdx.x * blockDim.x + threadIdx.x;
  unsigned int j;
  if(!d_pair_run_head(s0, npairs, key, ngas, j))
    return;
  const size_t N = (size_t) n, D = (size_t) nd;
  const int tb = timebin[j];
  const double dt = (tb ? (double) (1 << tb) : 0.0) * K.dt_fac_gas;
  const double mj = mass[j];
  double v0 = vel[j], v1 = vel[N + j], v2 = vel[2 * N + j], A = entropy[j], dh = heat[j];
  d_pair_run(s0, npairs, key, wgt, j, [&](unsigned int a, double wk) {
    if(a >= (unsigned int) nd + (unsigned int) nimp)
      return;
    double density, m0, m1, m2, E;
    if(a < (unsigned int) nd)
      {
        density = w[(size_t) DP_RHO * D + a];
        m0 = w[(size_t) DP_DMOM * D + a];
        m1 = w[(size_t) (DP_DMOM + 1) * D + a];
        m2 = w[(size_t) (DP_DMOM + 2) * D + a];
        E = w[(size_t) DP_DE * D + a];
      }
    else
      {
        const double *q = rec + DUST_REC_DRAG * (size_t) (a - (unsigned int) nd);
        density = q[4];
        m0 = q[5];
        m1 = q[6];
        m2 = q[7];
        E = q[8];
      }
    v0 -= m0 / density * wk;
    v1 -= m1 / density * wk;
    v2 -= m2 / density * wk;
    double u_old = A / GAMMA_MINUS1 * pow(density, GAMMA_MINUS1);
    if(K.minegy > u_old)   // DMAX(All.MinEgySpec, ...), allvars.h:273
      u_old = K.minegy;
    const double u_new = u_old + E * wk / density;
    double u_inc = u_new / u_old;
    if(u_inc > 1.5)
      u_inc = 1.5;
    A *= u_inc;
    dh += 1.e-20 * (E * wk / density * mj / dt);
  });
  vel[j] = v0;
  vel[N + j] = v1;
  vel[2 * N + j] = v2;
  entropy[j] = A;
  heat[j] = dh;
}

// ---------------------------------------------------------------------------------------------
// multi-GPU shards: the grain records that travel (DUST_REC_DENS / DUST_REC_DRAG doubles each)
// ---------------------------------------------------------------------------------------------
// record r of the send lists: local particle list[r], list slot slot[list[r]]; w: the planes (drag)
template <int K>
__global__ void k_dust_pack(int nrec, const int *__restrict__ list, const int *__restrict__ slot, int n,
                            const double *__restrict__ pos, const double *__restrict__ hsml,
                            const double *__restrict__ mass, int nd, const double *__restrict__ w,
                            double *__restrict__ out)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if(r >= nrec)
    return;
  const int i = list[r];
  double *o = out + (size_t) r * K;
  o[0] = pos[i];
  o[1] = pos[(size_t) n + i];
  o[2] = pos[2 * (size_t) n + i];
  o[3] = hsml[i];
  if(K == DUST_REC_DENS)
    o[4] = mass[i];
  else
    {
      const size_t a = (size_t) slot[i], D = (size_t) nd;
      o[4] = w[DP_RHO * D + a];
      for(int k = 0; k < 3; k++)
        o[5 + k] = w[(DP_DMOM + k) * D + a];
      o[8] = w[DP_DE * D + a];
    }
}

// the partial d7 one rank sent back, in the order of this shard's send list for that rank, onto the sums
__global__ void k_dust_add_parts(int cnt, const int *__restrict__ list, const int *__restrict__ slot,
                                 const double *__restrict__ part, double *__restrict__ out)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if(k < cnt)
    out[slot[list[k]]] += part[k];
}

// DUST_REAL_PEBBLE_COLLISIONS: the partial {d7, d9 [3]} records one rank sent back onto the four planes
__global__ void k_dust_add_parts4(int cnt, const int *__restrict__ list, const int *__restrict__ slot,
                                  const double *__restrict__ part, size_t nd, double *__restrict__ out)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if(k >= cnt)
    return;
  const size_t a = (size_t) slot[list[k]];
  for(int c = 0; c < 4; c++)
    out[c * nd + a] += part[4 * (size_t) k + c];
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static DustK dust_k(const ghip_dust_params *p)
{
  DustK K;
  K.b = make_box(p->BoxSize, p->periodic);
  K.dt_fac = p->dt_fac;
  K.dt_fac_gas = p->dt_fac_gas;
  K.minegy = p->MinEgySpec;
  K.meanweight = p->MeanWeight;
  K.ulength = p->UnitLength_in_cm;
  K.umass = p->UnitMass_in_g;
  K.udens = p->UnitDensity_in_cgs;
  K.uvel = p->UnitVelocity_in_cm_per_s;
  return K;
}

// the switches of ghip_set_dust_model as the kernel takes them; logr: the device plane of LogDustRadius_by_dt
static DustM dust_m(ghip_ctx *ctx, double *logr)
{
  const ghip_dust_model &s = ctx->dust_model;
  DustM m;
  m.growth = s.growth != 0;
  m.pebble = s.real_pebble_collisions != 0;
  m.vaporize = s.vaporize != 0;
  m.fe_ice = s.fe_and_ice_grains != 0;
  m.epstein = s.epstein != 0;
  m.no_heat = s.no_friction_heating != 0;
  m.gate = s.Time > 0 && s.Time > s.VirtualTime;
  m.vfrag = s.FragmentationVelocity;
  m.a_init = s.InitialDustRadius;
  m.uenergy = s.UnitEnergy_in_cgs;
  m.id = P<int>(ctx->f[GHIP_F_ID]);
  m.logr = logr;
  return m;
}

static bool dust_pebble(const ghip_ctx *ctx) { return ctx->dust_model_on && ctx->dust_model.real_pebble_collisions; }
static bool dust_growth(const ghip_ctx *ctx) { return ctx->dust_model_on && ctx->dust_model.growth; }

// What a pass asks of the setting before it launches anything.  c.grains: the caller came through
// ghip_dust_grains (the *_grains entry points, GHIP_DUST_GRAINS_FORM on shards) and has arrays for what the switches
// write; c.other names that way for a caller who did not
static int dust_model_ready(ghip_ctx *ctx, const DustCall &c)
{
  if(!ctx->dust_model_on)
    return GHIP_OK;
  const ghip_dust_model &s = ctx->dust_model;
  if(!c.grains && !c.drag && s.real_pebble_collisions)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: real_pebble_collisions is set (ghip_set_dust_model) and this entry "
                     "point has no array for the velocity sums d9: use %s", c.who, c.other);
  if(!c.grains && c.drag && (s.growth || s.vaporize))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: growth / vaporize is set (ghip_set_dust_model) and this entry point "
                     "cannot write the radius: use %s", c.who, c.other);
  if(c.drag && s.fe_and_ice_grains && !ctx->id_given)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: fe_and_ice_grains reads the particles' IDs, and GHIP_F_ID has not "
                     "been given since ghip_set_counts (ghip_set_field)", c.who);
  return GHIP_OK;
}

static int dust_heat_buffer(ghip_ctx *ctx)
{
  const size_t ng = (size_t) (ctx->ngas > 0 ? ctx->ngas : 1);
  const size_t before = ctx->dust_heat.cap;
  GCHK(ghip_ensure(ctx, ctx->dust_heat, ng * 8));
  if(ctx->dust_heat.cap != before)
    HIPCHK(hipMemsetAsync(ctx->dust_heat.p, 0, ctx->dust_heat.cap, ctx->stream));
  return GHIP_OK;
}

// the grain list to the device, ordered by the gravity tree into dust_ord (slot of the t-th thread)
static int dust_upload_list(ghip_ctx *ctx, int nd, const int *idx, const char *who)
{
  for(int a = 0; a < nd; a++)
    if(idx[a] < 0 || idx[a] >= ctx->n)
      return ghip_fail(ctx, GHIP_EINVAL, "%s: grain index %d out of range", who, idx[a]);
  hipStream_t st = ctx->stream;
  const size_t D = (size_t) nd;
  // dust_idx: idx [nd] | ord [nd] | key [nd] | key' [nd] | slot [nd]
  GCHK(ghip_ensure(ctx, ctx->dust_idx, D * 20 + 256));
  int *didx = P<int>(ctx->dust_idx), *dord = didx + D, *dslot = dord + 3 * D;
  unsigned int *dkey = reinterpret_cast<unsigned int *>(dord + D), *dkey2 = dkey + D;
  HIPCHK(hipMemcpyAsync(didx, idx, D * 4, hipMemcpyHostToDevice, st));
  return ghip_tree_order(ctx, nd, didx, dkey, dkey2, dslot, dord, st);
}

// One pass in the record every layer below the entries reads.  g == nullptr (a *_grains entry without its struct)
// becomes a list of -1 grains, which dust_call_check refuses like any other missing argument
static DustCall dust_call(const ghip_dust_params *p, const ghip_dust_grains *g, bool grains, bool drag,
                          const char *who, const char *other)
{
  DustCall c;
  c.p = p;
  if(g)
    c.g = *g;
  else
    c.g.ndust = -1;
  c.grains = grains;
  c.drag = drag;
  c.who = who;
  c.other = other;
  return c;
}

// The argument rules of all four forms, then what the setting asks of this form.  Required with ndust > 0: the
// list and d7; in the drag pass all nine arrays; in the density pass of a grains form d9 when it is written
static int dust_call_check(ghip_ctx *ctx, const DustCall &c)
{
  const ghip_dust_grains &g = c.g;
  bool ok = c.p && g.ndust >= 0;
  if(ok && g.ndust > 0)
    {
      ok = g.dust_idx && g.particle_density;
      if(c.drag)
        ok = ok && g.dust_density && g.dust_entropy && g.dust_gasvel && g.dust_radius && g.particle_velocity &&
             g.delta_momentum && g.delta_energy && g.vcoll;
      else if(c.grains && dust_pebble(ctx))
        ok = ok && g.particle_velocity;
    }
  if(!ok)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: bad arguments", c.who);
  return dust_model_ready(ctx, c);
}

// what every single-rank entry point asks of the context, then the grain list
static int dust_begin(ghip_ctx *ctx, const DustCall &c, bool gas)
{
  const int nd = c.g.ndust;
  const char *who = c.who;
  if(ctx->dd.on && ctx->dd.nranks > 1)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: not available on a multi-GPU context (%d ranks): these entry "
                     "points are single-rank (shards run GHIP_DD_DUST_DENSITY / GHIP_DD_DUST_DRAG)", who,
                     ctx->dd.nranks);
  if(ctx->shard_n > 1)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: not available on a sharded context (ghip_set_shard with %d "
                     "shards): the dust passes are single-rank only", who, ctx->shard_n);
  if(nd == 0)
    return GHIP_OK;
  if(gas)
    GCHK(ghip_finish_gas_tree(ctx));
  if(!ctx->gt.built || (gas && !ctx->st.built))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: call ghip_tree_build first", who);
  return dust_upload_list(ctx, nd, c.g.dust_idx, who);
}

// the per-grain planes of the drag pass, in list order, to dust_work; returns the planes
static int dust_upload_planes(ghip_ctx *ctx, const DustCall &c, std::vector<double> &h)
{
  const ghip_dust_grains &g = c.g;
  const size_t D = (size_t) g.ndust;
  const double *logr = g.log_radius_by_dt;
  h.assign((size_t) DUST_NPLANES * D, 0.0);
  for(size_t a = 0; a < D; a++)
    {
      h[DP_RHO * D + a] = g.dust_density[a];
      h[DP_ENT * D + a] = g.dust_entropy[a];
      h[DP_RAD * D + a] = g.dust_radius[a];
      h[DP_D7 * D + a] = g.particle_density[a];
      h[DP_VCOLL * D + a] = g.vcoll[a];
      for(int k = 0; k < 3; k++)
        {
          h[(DP_GV + k) * D + a] = g.dust_gasvel[3 * a + k];
          h[(DP_D9 + k) * D + a] = g.particle_velocity[3 * a + k];
        }
    }
  // dust_work: planes [DUST_NPLANES][nd] | cnt [nd + 1] | off [nd + 1]   (64-bit)
  //            | LogDustRadius_by_dt [nd] when the model writes it (growth and the caller holds the array)
  const bool lr = logr && dust_growth(ctx);
  GCHK(ghip_ensure(ctx, ctx->dust_work, (DUST_NPLANES * D + 2 * (D + 1) + (lr ? D : 0)) * 8 + 256));
  HIPCHK(hipMemcpyAsync(ctx->dust_work.p, h.data(), DUST_NIN * D * 8, hipMemcpyHostToDevice, ctx->stream));
  if(lr)
    HIPCHK(hipMemcpyAsync(P<double>(ctx->dust_work) + DUST_NPLANES * D + 2 * (D + 1), logr, D * 8,
                          hipMemcpyHostToDevice, ctx->stream));
  return GHIP_OK;
}

// (a LogDustRadius_by_dt array of the caller's was uploaded by dust_upload_planes)
static void dust_run_grains(ghip_ctx *ctx, const DustCall &c)
{
  const int nd = c.g.ndust;
  const DustK K = dust_k(c.p);
  if(ctx->dust_model_on)
    {
      const size_t D = (size_t) nd;
      const bool lr = c.g.log_radius_by_dt && dust_growth(ctx);
      double *dl = lr ? P<double>(ctx->dust_work) + DUST_NPLANES * D + 2 * (D + 1) : nullptr;
      k_dust_grain<DustM><<<cdiv(nd, 256), 256, 0, ctx->stream>>>(
        nd, P<int>(ctx->dust_idx), ctx->n, P<int>(ctx->f[GHIP_F_TIMEBIN]), P<double>(ctx->f[GHIP_F_MASS]),
        P<double>(ctx->f[GHIP_F_GRAVACCEL]), P<double>(ctx->f[GHIP_F_VEL]), P<double>(ctx->dust_work), K,
        dust_m(ctx, dl));
      return;
    }
  k_dust_grain<><<<cdiv(nd, 256), 256, 0, ctx->stream>>>(nd, P<int>(ctx->dust_idx), ctx->n,
                                                         P<int>(ctx->f[GHIP_F_TIMEBIN]),
                                                         P<double>(ctx->f[GHIP_F_MASS]),
                                                         P<double>(ctx->f[GHIP_F_GRAVACCEL]),
                                                         P<double>(ctx->f[GHIP_F_VEL]), P<double>(ctx->dust_work), K);
}

// k_dust_density for ng grains: this context's own list (ord: its tree order) or imported records.  out holds
// d7 [ng], or with real_pebble_collisions d7 and the three velocity sums: sum c of grain a at out[a * sa + c * sc]
template <class G>
static int dust_launch_density(ghip_ctx *ctx, const ghip_dust_params *p, int ng, const int *ord, const G &grain,
                               double *out, size_t sa, size_t sc)
{
  TreeDev &t = ctx->gt;
  const double *pos = P<double>(ctx->f[GHIP_F_POS]), *mass = P<double>(ctx->f[GHIP_F_MASS]);
  const int *type = P<int>(ctx->f[GHIP_F_TYPE]);
  const BoxK b = make_box(p->BoxSize, p->periodic);
  if(dust_pebble(ctx))
    k_dust_density<<<cdiv(ng, 64), 64, 0, ctx->stream>>>(ng, ord, grain, ctx->n, pos, mass, type, t.nelem,
                                                         P<int4>(t.lk), P<double4>(t.cl), P<int>(t.perm), b,
                                                         (double *) nullptr,
                                                         DustVel{P<double>(ctx->f[GHIP_F_VEL]), out, sa, sc});
  else
    k_dust_density<<<cdiv(ng, 64), 64, 0, ctx->stream>>>(ng, ord, grain, ctx->n, pos, mass, type, t.nelem,
                                                         P<int4>(t.lk), P<double4>(t.cl), P<int>(t.perm), b, out);
  HIPCHK(hipGetLastError());
  return GHIP_OK;
}

// the density sums of this context's own list: d7 into dust_work [nd], or with real_pebble_collisions d7 and the
// three velocity sums into its first four planes
static int dust_run_density(ghip_ctx *ctx, const DustCall &c)
{
  const int nd = c.g.ndust;
  const size_t D = (size_t) nd;
  GCHK(ghip_ensure(ctx, ctx->dust_work, (dust_pebble(ctx) ? 4 : 1) * D * 8 + 256));
  const int *didx = P<int>(ctx->dust_idx);
  DustGrainLocal gl = {didx, P<double>(ctx->f[GHIP_F_POS]), P<double>(ctx->f[GHIP_F_HSML]), ctx->n,
                       P<double>(ctx->f[GHIP_F_MASS]), nullptr};
  return dust_launch_density(ctx, c.p, nd, didx + D, gl, P<double>(ctx->dust_work), 1, D);
}

// ... and back to the caller: d7 [nd], and the raw d9 sums [nd][3] with real_pebble_collisions
static int dust_download_density(ghip_ctx *ctx, const DustCall &c)
{
  const size_t D = (size_t) c.g.ndust;
  const double *dout = P<double>(ctx->dust_work);
  std::vector<double> h(dust_pebble(ctx) ? 3 * D : 0);
  HIPCHK(hipMemcpyAsync(c.g.particle_density, dout, D * 8, hipMemcpyDeviceToHost, ctx->stream));
  if(dust_pebble(ctx))
    HIPCHK(hipMemcpyAsync(h.data(), dout + D, 3 * D * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  if(dust_pebble(ctx))
    for(size_t a = 0; a < D; a++)
      for(int k = 0; k < 3; k++)
        c.g.particle_velocity[3 * a + k] = h[k * D + a];
  return GHIP_OK;
}

// The scatter into this context's gas: count, scan, fill, sort, apply (ghip_pairs.h).  Grains [0, nd) are the
// list's (slots in dust_idx, planes w with stride nd, launched in tree order), [nd, nd + nimp) the imported drag
// records rec.  cnt, off: nd + nimp + 1 each.
static int dust_scatter(ghip_ctx *ctx, const DustK &K, int nd, const double *w, int nimp, const double *rec,
                        unsigned long long *dcnt, unsigned long long *doff, long long *npairs_out)
{
  hipStream_t st = ctx->stream;
  const int m = nd + nimp;
  const size_t D = (size_t) nd;
  const int *didx = P<int>(ctx->dust_idx), *dord = didx + D;
  TreeDev &t = ctx->st;
  const SphNode *nodes = P<SphNode>(t.mq);
  const int *perm = P<int>(t.perm);
  const double *pos = P<double>(ctx->f[GHIP_F_POS]), *mass = P<double>(ctx->f[GHIP_F_MASS]);
  const int *tbin = P<int>(ctx->f[GHIP_F_TIMEBIN]);
  const DustGas gas = {ctx->n, ctx->ngas, pos, mass, P<int>(ctx->f[GHIP_F_TYPE]), tbin};
  const DustTarget<DustGrainLocal> own = {
    gas, {didx, pos, P<double>(ctx->f[GHIP_F_HSML]), ctx->n, nullptr, w + DP_RHO * D}, dord, 0};
  const DustTarget<DustGrainRec> imp = {gas, {rec, DUST_REC_DRAG}, nullptr, nd};
  HIPCHK(hipMemsetAsync(dcnt, 0, (size_t) (m + 1) * 8, st));
  if(ctx->ngas > 0 && nd > 0)
    k_pairs<0><<<cdiv(nd, 64), 64, 0, st>>>(nd, own, t.nelem, nodes, perm, K.b, dcnt, nullptr, 0ULL, nullptr, nullptr);
  if(ctx->ngas > 0 && nimp > 0)
    k_pairs<0><<<cdiv(nimp, 64), 64, 0, st>>>(nimp, imp, t.nelem, nodes, perm, K.b, dcnt + D, nullptr, 0ULL, nullptr,
                                              nullptr);
  HIPCHK(hipGetLastError());
  GCHK(ghip_scan<unsigned long long>(ctx, dcnt, doff, m + 1, st));
  unsigned long long npairs = 0;
  if(ctx->ngas > 0)
    HIPCHK(hipMemcpyAsync(&npairs, doff + m, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));   // the pair count sizes the sort
  *npairs_out = (long long) npairs;
  const unsigned long long *key;
  const double *wgt;
  GCHK(ghip_pairs_fill_sort(ctx, ctx->dust_pairs, (long long) npairs, "dust_drag", "dust-gas", [&](const PairBuf &pb) {
    if(nd > 0)
      k_pairs<1><<<cdiv(nd, 64), 64, 0, st>>>(nd, own, t.nelem, nodes, perm, K.b, nullptr, doff, npairs, pb.k0, pb.w0);
    if(nimp > 0)
      k_pairs<1><<<cdiv(nimp, 64), 64, 0, st>>>(nimp, imp, t.nelem, nodes, perm, K.b, nullptr, doff + D, npairs, pb.k0,
                                                pb.w0);
  }, &key, &wgt));
  if(!key)
    return GHIP_OK;
  k_dust_apply<<<cdiv((long long) npairs, 256), 256, 0, st>>>((long long) npairs, key, wgt, nd, w, nimp, rec, ctx->n,
                                                              ctx->ngas, mass, tbin, P<double>(ctx->f[GHIP_F_VEL]),
                                                              P<double>(ctx->f[GHIP_F_ENTROPY]),
                                                              P<double>(ctx->dust_heat), K);
  HIPCHK(hipGetLastError());
  return GHIP_OK;
}

// The grain outputs of the drag pass back to the caller's arrays.  The two planes the model writes under growth
// go back here and nowhere else: the radius to a caller of a grains form, LogDustRadius_by_dt where he holds one
static int dust_download_grains(ghip_ctx *ctx, const DustCall &c, std::vector<double> &h)
{
  const ghip_dust_grains &g = c.g;
  const size_t D = (size_t) g.ndust;
  const double *dw = P<double>(ctx->dust_work);
  HIPCHK(hipMemcpyAsync(h.data() + DP_D9 * D, dw + DP_D9 * D, DUST_NOUT * D * 8, hipMemcpyDeviceToHost,
                        ctx->stream));
  if(dust_growth(ctx) && c.grains)
    HIPCHK(hipMemcpyAsync(g.dust_radius, dw + DP_RAD * D, D * 8, hipMemcpyDeviceToHost, ctx->stream));
  if(dust_growth(ctx) && g.log_radius_by_dt)
    HIPCHK(hipMemcpyAsync(g.log_radius_by_dt, dw + DUST_NPLANES * D + 2 * (D + 1), D * 8, hipMemcpyDeviceToHost,
                          ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  for(size_t a = 0; a < D; a++)
    {
      for(int k = 0; k < 3; k++)
        {
          g.particle_velocity[3 * a + k] = h[(DP_D9 + k) * D + a];
          g.delta_momentum[3 * a + k] = h[(DP_DMOM + k) * D + a];
        }
      g.delta_energy[a] = h[DP_DE * D + a];
      g.vcoll[a] = h[DP_VCOLL * D + a];
    }
  return GHIP_OK;
}

// the two passes on one rank
static int dust_density_impl(ghip_ctx *ctx, const DustCall &c)
{
  GHIP_JOIN(ctx);
  GCHK(dust_call_check(ctx, c));
  GCHK(dust_begin(ctx, c, false));
  if(c.g.ndust == 0)
    return GHIP_OK;
  GCHK(dust_run_density(ctx, c));
  return dust_download_density(ctx, c);
}

static int dust_drag_impl(ghip_ctx *ctx, const DustCall &c)
{
  GHIP_JOIN(ctx);
  GCHK(dust_call_check(ctx, c));
  GCHK(dust_begin(ctx, c, ctx->ngas > 0));
  GCHK(dust_heat_buffer(ctx));
  const int ndust = c.g.ndust;
  if(ndust == 0)
    return GHIP_OK;
  const size_t D = (size_t) ndust;
  std::vector<double> h;
  GCHK(dust_upload_planes(ctx, c, h));
  dust_run_grains(ctx, c);
  HIPCHK(hipGetLastError());
  double *dw = P<double>(ctx->dust_work);
  unsigned long long *dcnt = reinterpret_cast<unsigned long long *>(dw + DUST_NPLANES * D), *doff = dcnt + D + 1;
  long long npairs = 0;
  GCHK(dust_scatter(ctx, dust_k(c.p), ndust, dw, 0, nullptr, dcnt, doff, &npairs));
  return dust_download_grains(ctx, c, h);
}

extern "C" int ghip_dust_density(ghip_ctx *ctx, const ghip_dust_params *p, int ndust, const int *dust_idx,
                                 double *particle_density)
{
  if(!ctx)
    return GHIP_EINVAL;
  ghip_dust_grains g = {};
  g.ndust = ndust;
  g.dust_idx = dust_idx;
  g.particle_density = particle_density;
  return dust_density_impl(ctx, dust_call(p, &g, false, false, "ghip_dust_density", "ghip_dust_density_grains"));
}

extern "C" int ghip_dust_drag(ghip_ctx *ctx, const ghip_dust_params *p, int ndust, const int *dust_idx,
                              const double *dust_density, const double *dust_entropy,
                              const double *dust_gasvel, const double *dust_radius,
                              const double *particle_density, double *particle_velocity,
                              double *delta_momentum, double *delta_energy, double *vcoll)
{
  if(!ctx)
    return GHIP_EINVAL;
  ghip_dust_grains g = {};
  g.ndust = ndust;
  g.dust_idx = dust_idx;
  g.dust_density = dust_density;
  g.dust_entropy = dust_entropy;
  g.dust_gasvel = dust_gasvel;
  g.dust_radius = const_cast<double *>(dust_radius);   // (read only: the switches that write it are refused here)
  g.particle_density = const_cast<double *>(particle_density);
  g.particle_velocity = particle_velocity;
  g.delta_momentum = delta_momentum;
  g.delta_energy = delta_energy;
  g.vcoll = vcoll;
  return dust_drag_impl(ctx, dust_call(p, &g, false, true, "ghip_dust_drag", "ghip_dust_drag_grains"));
}

extern "C" int ghip_dust_density_grains(ghip_ctx *ctx, const ghip_dust_params *p, const ghip_dust_grains *g)
{
  if(!ctx)
    return GHIP_EINVAL;
  return dust_density_impl(ctx, dust_call(p, g, true, false, "ghip_dust_density_grains", ""));
}

extern "C" int ghip_dust_drag_grains(ghip_ctx *ctx, const ghip_dust_params *p, const ghip_dust_grains *g)
{
  if(!ctx)
    return GHIP_EINVAL;
  return dust_drag_impl(ctx, dust_call(p, g, true, true, "ghip_dust_drag_grains", ""));
}

extern "C" int ghip_set_dust_model(ghip_ctx *ctx, const ghip_dust_model *m)
{
  if(!ctx)
    return GHIP_EINVAL;
  if(!m)
    {
      ctx->dust_model_on = false;
      memset(&ctx->dust_model, 0, sizeof(ctx->dust_model));
      return GHIP_OK;
    }
  const double vals[5] = {m->Time, m->VirtualTime, m->FragmentationVelocity, m->InitialDustRadius, m->UnitEnergy_in_cgs};
  static const char *const names[5] = {"Time", "VirtualTime", "FragmentationVelocity", "InitialDustRadius",
                                       "UnitEnergy_in_cgs"};
  for(int k = 0; k < 5; k++)
    if(!std::isfinite(vals[k]))
      return ghip_fail(ctx, GHIP_EINVAL, "ghip_set_dust_model: %s is not finite", names[k]);
  if(m->vaporize && !m->growth)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_set_dust_model: vaporize needs growth (DUST_VAPORIZE does not compile "
                     "without DUST_GROWTH: it uses adust_min)");
  if(m->fe_and_ice_grains && !m->vaporize)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_set_dust_model: fe_and_ice_grains needs vaporize");
  if(m->vaporize && m->InitialDustRadius == DUST_A_MIN)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_set_dust_model: vaporize with InitialDustRadius == %g: the latent heat "
                     "divides by InitialDustRadius - %g", DUST_A_MIN, DUST_A_MIN);
  const bool on = m->growth || m->real_pebble_collisions || m->vaporize || m->fe_and_ice_grains || m->epstein ||
                  m->no_friction_heating;
  if(on && ctx->shard_n > 1)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_set_dust_model: not available on a replicated shard (ghip_set_shard "
                     "with %d ranks); use the ghip_dd_* contexts", ctx->shard_n);
  ctx->dust_model = *m;
  ctx->dust_model_on = on;
  return GHIP_OK;
}

extern "C" size_t ghip_dust_model_size(void) { return sizeof(ghip_dust_model); }
extern "C" size_t ghip_dust_grains_size(void) { return sizeof(ghip_dust_grains); }

extern "C" int ghip_dust_get_drag_heating(ghip_ctx *ctx, double *drag_heating)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  if(ctx->dd.on && !ctx->dust_heat.p)
    {
      // a shard creates its DragHeating in GHIP_DD_DUST_DRAG or ghip_dust_set_drag_heating only: until
      // then it holds none (ghip_sfr_cooling refuses dust = 1), and it reads as zero
      if(drag_heating && ctx->ngas > 0)
        memset(drag_heating, 0, (size_t) ctx->ngas * 8);
      return GHIP_OK;
    }
  GCHK(dust_heat_buffer(ctx));
  if(drag_heating && ctx->ngas > 0)
    HIPCHK(hipMemcpyAsync(drag_heating, ctx->dust_heat.p, (size_t) ctx->ngas * 8, hipMemcpyDeviceToHost,
                          ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  return GHIP_OK;
}

extern "C" int ghip_dust_set_drag_heating(ghip_ctx *ctx, const double *drag_heating)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  GCHK(dust_heat_buffer(ctx));
  if(drag_heating && ctx->ngas > 0)
    HIPCHK(hipMemcpyAsync(ctx->dust_heat.p, drag_heating, (size_t) ctx->ngas * 8, hipMemcpyHostToDevice,
                          ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  return GHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// the passes on a multi-GPU shard (GHIP_DD_DUST_DENSITY / GHIP_DD_DUST_DRAG)
//
// The reference exports a grain to every task whose domain its sphere touches and adds the partial
// results back on the home task (dust.c:60-261, 560-746).  Here a grain goes to every other shard whose
// local Type 0 / Type 2 particles its sphere can reach (the all-gathered group boxes of those
// particles, ghip_dd.hip), once per pass:
//   density  phase 0  own sums; group table -> all-gather
//            phase 1  selection, records {Pos, Hsml, Mass} -> all-to-all-v
//            phase 2  the imported grains against this shard's Type-2 particles; partial d7 back to the
//                     home shards (all-to-all-v with the receive layout as send layout)
//            phase 3  own sum + the partials in ascending rank order (the export table is sorted by
//                     task, dust.c:112-116, and the results are added in that order, :223)
//   drag     phase 0  the per-grain update of this shard's grains; group table -> all-gather
//            phase 1  selection, records {Pos, Hsml, DUST_Density, DeltaDustMomentum, DeltaDragEnergy}
//                     -> all-to-all-v
//            phase 2  the scatter into this shard's gas of its own grains (list order) and the imported
//                     ones (receive order: by sending rank, within a rank by the sender's local particle
//                     index -- the send lists are ascending in it, as DataIndexTable[].Index after the
//                     sort of dust.c:617-621)
// Under NTask > 1 the reference also adds DustDataOut[].DeltaDustMomentum / .DeltaDragEnergy back to
// the exported grains (dust.c:727-728), but dust_evaluate_select never writes DustDataResult
// (dust.c:889-1029): the values it adds are uninitialised memory.  Nothing is added here.
// ---------------------------------------------------------------------------------------------
int ghip_dd_dust_groups(ghip_ctx *ctx);   // ghip_dd.hip
int ghip_dd_dust_select(ghip_ctx *ctx, const char *what, int nd, const int *ord, const int *idx, double boxsize,
                        int periodic, int *total);

// walk = 0: the params of the two operations as the record
static DustCall dust_call_dd_args(const void *params, bool drag, const char *who, const char *other)
{
  // the arrays of ghip_dust_grains but the two that the model writes, with the params inside and a const radius
  const ghip_dd_dust_args &a = *reinterpret_cast<const ghip_dd_dust_args *>(params);
  ghip_dust_grains g = {};
  g.ndust = a.ndust;
  g.dust_idx = a.dust_idx;
  g.particle_density = a.particle_density;
  g.dust_density = a.dust_density;
  g.dust_entropy = a.dust_entropy;
  g.dust_gasvel = a.dust_gasvel;
  g.dust_radius = const_cast<double *>(a.dust_radius);   // (read only: the switches that write it are refused here)
  g.particle_velocity = a.particle_velocity;
  g.delta_momentum = a.delta_momentum;
  g.delta_energy = a.delta_energy;
  g.vcoll = a.vcoll;
  g.counts = a.counts;
  return dust_call(a.p, &g, false, drag, who, other);
}

int ghip_dd_dust_begin(ghip_ctx *ctx, int op, const void *params, int walk)
{
  GHIP_JOIN(ctx);
  ctx->dd.walk = walk;
  // the wind particles share this operation's code and requirements (ghip_wind.hip): their forms hand over
  if(op == GHIP_DD_WIND && ((walk >= GHIP_WIND_FORM && walk <= GHIP_WIND_SPREAD_FORM) || walk == GHIP_WINDS_RESIDENT_FORM || walk == GHIP_WINDS_SPAWN_FORM))
    return ghip_dd_wind_begin(ctx, op, params, walk);
  const bool grains = walk == GHIP_DUST_GRAINS_FORM;
  const bool drag = op == GHIP_DD_DUST_DRAG;
  const char *who = drag ? "ghip_dd dust drag" : "ghip_dd dust density";
  const char *other = "walk = GHIP_DUST_GRAINS_FORM with ghip_dd_dust_grains_args";
  if(walk != 0 && !grains)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: walk = %d is neither 0 nor GHIP_DUST_GRAINS_FORM%s", who, walk,
                     drag ? " nor one of the wind forms GHIP_WIND_FORM, GHIP_WIND_DENSITY_FORM, GHIP_WIND_SPREAD_FORM" : "");
  DustCall &c = ctx->dd.dust;
  if(grains)
    {
      const ghip_dd_dust_grains_args &G = *reinterpret_cast<const ghip_dd_dust_grains_args *>(params);
      c = dust_call(G.p, &G.g, true, drag, who, other);
    }
  else
    c = dust_call_dd_args(params, drag, who, other);
  GCHK(dust_call_check(ctx, c));
  // (after GHIP_DD_BH_SWALLOW the trees are marked stale for their moments; their geometry still holds)
  if(!ctx->gt.built && !ctx->dd.geom_kept)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: run GHIP_DD_GRAVITY of this step first", who);
  if(drag && !ctx->st.built && !ctx->dd.geom_kept)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: run GHIP_DD_DENSITY of this step first", who);
  if(c.g.counts)
    for(int k = 0; k < 4; k++)
      c.g.counts[k] = 0;
  ctx->dd.du_sent = ctx->dd.du_recvd = 0;
  return GHIP_OK;
}

// what the operation sent, received and paired, when it ends
static void dust_write_counts(const DDState &D, long long npairs)
{
  long long *counts = D.dust.g.counts;
  if(!counts)
    return;
  counts[0] = D.du_sent;
  counts[1] = D.du_recvd;
  if(D.dust.drag)
    counts[2] = npairs;
  counts[3] = D.bytes_sent[D.op];
}

int ghip_dd_dust_step(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  if(D.op == GHIP_DD_WIND && D.walk >= GHIP_WIND_FORM)
    return ghip_dd_wind_step(ctx);
  const DustCall &c = D.dust;
  const ghip_dust_params *p = c.p;
  hipStream_t st = ctx->stream;
  const bool drag = c.drag;
  const bool vels = !drag && dust_pebble(ctx);   // (the density pass carries d7 and the three velocity sums)
  const int npart = vels ? 4 : 1;                // doubles of a partial sum that goes home
  const char *who = c.who;
  const int nd = c.g.ndust, n = ctx->n;
  const size_t Dn = (size_t) nd;
  const int *didx = P<int>(ctx->dust_idx), *dord = didx + Dn;
  const double *pos = P<double>(ctx->f[GHIP_F_POS]), *hsml = P<double>(ctx->f[GHIP_F_HSML]),
               *mass = P<double>(ctx->f[GHIP_F_MASS]);
  const int recd = drag ? DUST_REC_DRAG : DUST_REC_DENS;
  enum { OWN, SELECT, IMPORTED, ADD };   // (the phases 0 .. 3 of the comment above; drag ends in IMPORTED)
  if(D.phase == OWN)
    {
      if(drag)
        GCHK(dust_heat_buffer(ctx));   // (this shard holds DragHeating from now on)
      if(nd > 0)
        {
          GCHK(dust_upload_list(ctx, nd, c.g.dust_idx, who));
          didx = P<int>(ctx->dust_idx);
          dord = didx + Dn;
          if(drag)
            {
              std::vector<double> h;
              GCHK(dust_upload_planes(ctx, c, h));
              dust_run_grains(ctx, c);
            }
          else
            GCHK(dust_run_density(ctx, c));
          HIPCHK(hipGetLastError());
          GCHK(ghip_ensure(ctx, D.du_slot, (size_t) (n > 0 ? n : 1) * 4));
          GCHK(ghip_list_slots(ctx, nd, didx, P<int>(D.du_slot), st));
        }
      D.phase = SELECT;
      return ghip_dd_dust_groups(ctx);
    }
  if(D.phase == SELECT)
    {
      int total = 0;
      GCHK(ghip_dd_dust_select(ctx, who, nd, dord, didx, p->BoxSize, p->periodic, &total));
      GCHK(ghip_ensure(ctx, D.du_send, (size_t) (total > 0 ? total : 1) * recd * 8));
      if(total > 0)
        {
          if(drag)
            k_dust_pack<DUST_REC_DRAG><<<cdiv(total, 256), 256, 0, st>>>(
              total, P<int>(D.du_list), P<int>(D.du_slot), n, pos, hsml, mass, nd, P<double>(ctx->dust_work),
              P<double>(D.du_send));
          else
            k_dust_pack<DUST_REC_DENS><<<cdiv(total, 256), 256, 0, st>>>(
              total, P<int>(D.du_list), P<int>(D.du_slot), n, pos, hsml, mass, nd, nullptr, P<double>(D.du_send));
          HIPCHK(hipGetLastError());
        }
      D.du_sent = total;
      ghip_dd_set_alltoallv(D, D.du_send.p, (size_t) recd * 8, D.du_scount, D.du_soff, &D.du_recv);
      D.phase = IMPORTED;
      return 1;
    }
  if(D.phase == IMPORTED && !drag)
    {
      // the imported grains against this shard's Type-2 particles; the partial sums go home
      const int nimp = D.x.rtotal;
      D.du_recvd = nimp;
      GCHK(ghip_ensure(ctx, D.du_part, (size_t) (nimp > 0 ? nimp : 1) * npart * 8));
      if(nimp > 0)
        GCHK(dust_launch_density(ctx, p, nimp, nullptr, DustGrainRec{P<double>(D.du_recv), DUST_REC_DENS},
                                 P<double>(D.du_part), 4, 1));
      int sc[GHIP_MAXRANKS], so[GHIP_MAXRANKS];
      for(int r = 0; r < D.nranks; r++)
        {
          sc[r] = D.x.rcount[r];
          so[r] = D.x.roff[r];
        }
      ghip_dd_set_alltoallv(D, D.du_part.p, (size_t) npart * 8, sc, so, &D.du_back);
      D.phase = ADD;
      return 1;
    }
  if(D.phase == ADD && !drag)
    {
      for(int r = 0; r < D.nranks; r++)
        if(D.x.rcount[r] != (r == D.rank ? 0 : D.du_scount[r]))
          return ghip_fail(ctx, GHIP_ECOMM, "%s: %d partial sums came back from rank %d, %d grains went there",
                           who, D.x.rcount[r], r, D.du_scount[r]);
      if(nd > 0)
        {
          double *dout = P<double>(ctx->dust_work);
          for(int r = 0; r < D.nranks; r++)   // own sum first, then the ranks in ascending order
            if(r != D.rank && D.du_scount[r] > 0)
              {
                if(vels)
                  k_dust_add_parts4<<<cdiv(D.du_scount[r], 256), 256, 0, st>>>(
                    D.du_scount[r], P<int>(D.du_list) + D.du_soff[r], P<int>(D.du_slot),
                    P<double>(D.du_back) + 4 * (size_t) D.x.roff[r], Dn, dout);
                else
                  k_dust_add_parts<<<cdiv(D.du_scount[r], 256), 256, 0, st>>>(
                    D.du_scount[r], P<int>(D.du_list) + D.du_soff[r], P<int>(D.du_slot),
                    P<double>(D.du_back) + D.x.roff[r], dout);
              }
          HIPCHK(hipGetLastError());
          GCHK(dust_download_density(ctx, c));
        }
      HIPCHK(ghip_stream_sync(ctx, st));
      dust_write_counts(D, 0);
      return 0;
    }
  if(D.phase == IMPORTED && drag)
    {
      // this shard's grains in list order, then the imported ones in receive order
      const int nimp = D.x.rtotal;
      D.du_recvd = nimp;
      const size_t M = (size_t) nd + (size_t) nimp;
      // du_part: cnt [M + 1] | off [M + 1]   (64-bit)
      GCHK(ghip_ensure(ctx, D.du_part, 2 * (M + 1) * 8 + 256));
      unsigned long long *dcnt = P<unsigned long long>(D.du_part), *doff = dcnt + M + 1;
      const double *rec = nimp > 0 ? P<double>(D.du_recv) : nullptr;
      long long npairs = 0;
      GCHK(dust_scatter(ctx, dust_k(p), nd, P<double>(ctx->dust_work), nimp, rec, dcnt, doff, &npairs));
      if(nd > 0)
        {
          std::vector<double> h((size_t) DUST_NPLANES * Dn);
          GCHK(dust_download_grains(ctx, c, h));
        }
      HIPCHK(ghip_stream_sync(ctx, st));
      dust_write_counts(D, npairs);
      return 0;
    }
  return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_step: the dust passes have no phase %d", D.phase);
}
