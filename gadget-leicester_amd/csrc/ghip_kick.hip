// ghip_kick.hip -- "next" row N1: timestep criterion + kick on the resident
// particles, so that P/SphP need not leave HBM between force evaluations.
//
// Replaces the loop of advance_and_find_timesteps() (timestep.c:142-260) with get_timestep()
// (timestep.c:607-1123; flag == 0, TypeOfTimestepCriterion 0) and do_the_kick()
// (timestep.c:364-605) for the minimal periodic flag set -- no PMGRID long-range kick, no
// MAGNETIC terms -- and the per-type sums of find_dt_displacement_constraint()
// (timestep.c:1125-1224).  The shipped bundle's rules (DUST, DUST_TIMESTEP, BLACK_HOLES +
// ACCRETION_RADIUS, VIRTUAL: grains, sinks, virtual particles, DragAccel) are the
// k_advance_timesteps<true> instantiation, chosen by ghip_set_integration_flags; the default
// instantiation is the minimal set's kernel, instruction for instruction.  DoDynamicUpdate / force_kick_node
// (forcetree.c:1474-1651) has no counterpart: the device tree is rebuilt every step.  The host
// keeps the linked lists of the time bins (FirstInTimeBin...) -- it rebuilds them from the
// returned TimeBin[] as reconstruct_timebins() does.
// One thread per active particle, SoA planes: a streaming, HBM-bound kernel (per collisionless
// particle 60 B in + 32 B out, per gas particle 156 B in + 96 B out).
#include "ghip_internal.h"

// no a*b+c -> fma contraction in this file: the kick is rounding-for-rounding the host's
// arithmetic (sqrt and division are correctly rounded on the device), so velocities, entropies and
// the integer timeline come out identical to the CPU path; only pow() (MinEgySpec floor) may differ
// in the last bits.  A streaming kernel: the extra instructions are free.
#pragma clang fp contract(off)

#include "ghip_timefac.h"
#include <type_traits>

#define GHIP_TIMEBINS 29                   // allvars.h:39
#define GHIP_TIMEBASE (1 << GHIP_TIMEBINS) // allvars.h:41
#define GAMMA_MINUS1 (GAMMA - 1)

struct KickK
{
  int ti_current;
  double timebase;
  int comoving;
  double time, hubble_a, fac1, fac2, fac3, a3inv, atime;   // timestep.c:52-63
  double errtol, courant, maxdt, mindt, dtdisp;
  double soft[6];
  int adaptive_hsml;
  int pmgrid;            // PMGRID: GravPM enters the criterion and VelPred (timestep.c:648-652, 511-513)
  double dt_gravkickB;   // timestep.c:66-72
  double minegy;
  unsigned int active;
  DriftK tab;   // gravkick / hydrokick tables (comoving)
};

// the shipped bundle's rules (ghip_set_integration_flags); the default kernel has none of them
struct KickB
{
  int dust, dust_timestep, black_holes, accretion_radius, virt;
  double dt_abs;     // Type 3: min(0.03 OuterBoundary / C UnitVelocity FeedBackVelocity, dt_ff = 1)
  double dt_accr0;   // Type 5: 0.03 (OuterBoundary / 100)
  double acc_dt, smbh_mass, inner, sink;
  const double *mass;        // [n]
  double *drag;              // [3][ngas] or null (zero)
  const double *ddm;         // [3][ngas] or null (zero)
};

// ghip_set_viscosity with time_dependent: the alpha update of do_the_kick (timestep.c:529-534).  The pack
// of k_advance_timesteps is then one KickV (minimal flag set) or one KickBV (the bundle's rules, which
// still find their KickB in it).
struct KickV
{
  double *alpha;           // [ngas]
  const double *dtalpha;   // [ngas]
  double alpha_max, alpha_min;   // All.ArtBulkViscConst, All.AlphaMin
};
struct KickBV : KickB
{
  KickV v;
};
__device__ __forceinline__ const KickV &d_kickv(const KickV &v) { return v; }
__device__ __forceinline__ const KickV &d_kickv(const KickBV &x) { return x.v; }

// ghip_set_rad_accel: RAD_ACCEL in get_timestep and do_the_kick (timestep.c:668-671, 497-500).  A KickR stands
// FIRST in the pack of k_advance_timesteps, in front of what the pack would hold without it
struct KickR
{
  const double *ra;   // SphP[].ra.RadAccel [3][ngas]
};
template <class T>
__device__ __forceinline__ const KickV &d_kickv(const KickR &, const T &t) { return d_kickv(t); }
template <class... T>
__device__ __forceinline__ const KickR &d_kickr(const KickR &r, const T &...) { return r; }
__device__ __forceinline__ const KickB &d_kickb(const KickB &x) { return x; }
__device__ __forceinline__ const KickB &d_kickb(const KickR &, const KickB &x) { return x; }

// X... is empty for the default kernel (the minimal flag set: same signature, same code as before the
// bundle existed) and one KickB for the bundle's rules; every rule sits in an `if constexpr`
template <bool BUNDLE, class... X>
__global__ void k_advance_timesteps(int nact, const int *__restrict__ act, int n, int ngas, KickK k,
                                    const int *__restrict__ type, double *__restrict__ vel,
                                    const double *__restrict__ gravaccel,
                                    const double *__restrict__ gravpm,
                                    const double *__restrict__ hydroaccel,
                                    double *__restrict__ velpred, double *__restrict__ entropy,
                                    double *__restrict__ dtentropy,
                                    const double *__restrict__ density,
                                    const double *__restrict__ hsml,
                                    const double *__restrict__ maxsignalvel,
                                    int *__restrict__ timebin, int *__restrict__ ti_begstep,
                                    int *__restrict__ err, int *errw, double *__restrict__ kick_dv,
                                    int *__restrict__ kick_flag, X... xs)
{
// (errw: asynchronous mode, the pinned word the next synchronising call checks)
#define D_RAISE(code)                   \
  do                                    \
    {                                   \
      atomicMax(err, (code));           \
      if(errw)                          \
        *(volatile int *) errw = (code); \
    }                                   \
  while(0)
  int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nact)
    return;
  const int i = act ? act[a] : a;
  const int ty = type[i];
  const bool gas = (ty == 0) && (i < ngas);
  double g[3], hy[3] = {0, 0, 0};
  for(int j = 0; j < 3; j++)
    g[j] = gravaccel[(size_t) j * n + i];
  if(gas)
    for(int j = 0; j < 3; j++)
      hy[j] = hydroaccel[(size_t) j * ngas + i];

  // ---- get_timestep, timestep.c:636-700, 947-1123 ----
  double ax = k.fac1 * g[0], ay = k.fac1 * g[1], az = k.fac1 * g[2];
  double pm[3] = {0, 0, 0};
  if(k.pmgrid)   // timestep.c:648-652
    {
      for(int j = 0; j < 3; j++)
        pm[j] = gravpm[(size_t) j * n + i];
      ax += k.fac1 * pm[0];
      ay += k.fac1 * pm[1];
      az += k.fac1 * pm[2];
    }
  if(ty == 0)
    {
      ax += k.fac2 * hy[0];
      ay += k.fac2 * hy[1];
      az += k.fac2 * hy[2];
      if constexpr((... || std::is_same_v<X, KickR>))   // timestep.c:668-671
        {
          if(gas)
            {
              const double *ra = d_kickr(xs...).ra;
              ax += k.fac2 * ra[i];
              ay += k.fac2 * ra[(size_t) ngas + i];
              az += k.fac2 * ra[2 * (size_t) ngas + i];
            }
        }
      if constexpr(BUNDLE)
        {
          const KickB &x = d_kickb(xs...);
          if(x.dust && gas && x.drag)   // timestep.c:673-677
            {
              ax += k.fac2 * x.drag[i];
              ay += k.fac2 * x.drag[(size_t) ngas + i];
              az += k.fac2 * x.drag[2 * (size_t) ngas + i];
            }
        }
    }
  double ac = sqrt(ax * ax + ay * ay + az * az);
  if(ac == 0)
    ac = 1.0e-30;
  double dt = sqrt(2 * k.errtol * k.atime * k.soft[ty] / ac);
  if constexpr(BUNDLE)
    {
      const KickB &x = d_kickb(xs...);
      if(x.dust_timestep && ty == 0 && x.mass[i] > 0)   // timestep.c:710-722
        {
          const double m = x.mass[i];
          double d[3] = {0, 0, 0};
          if(gas && x.ddm)
            for(int j = 0; j < 3; j++)
              d[j] = x.ddm[(size_t) j * ngas + i];
          ax += d[0] / m / dt;
          ay += d[1] / m / dt;
          az += d[2] / m / dt;
          ac = sqrt(ax * ax + ay * ay + az * az);   // (the overwrite below reads this ac)
          if(ac > 0)   // (ac == 0: the reference compares an uninitialised dt_new; dt stays)
            {
              double dt_new = sqrt(2 * k.errtol * k.atime * k.soft[ty] / ac);
              if(dt_new < dt)
                dt = dt_new;
            }
        }
      if(x.dust && ty == 2)   // timestep.c:725-726
        dt = dt / 2;
    }
  if(k.adaptive_hsml && ty == 0)   // timestep.c:740-743
    dt = sqrt(2 * k.errtol * k.atime * hsml[i] / 2.8 / ac);
  if(gas)
    {
      double dt_courant;
      if(k.comoving)
        dt_courant = 2 * k.courant * k.time * hsml[i] / (k.fac3 * maxsignalvel[i]);
      else
        dt_courant = 2 * k.courant * hsml[i] / maxsignalvel[i];
      if(dt_courant < dt)
        dt = dt_courant;
    }
  if constexpr(BUNDLE)
    {
      const KickB &x = d_kickb(xs...);
      if(x.virt && ty == 3)   // timestep.c:887-897
        {
          if(dt > x.dt_abs)
            dt = x.dt_abs;
        }
      if(x.black_holes && ty == 5)   // timestep.c:908-947
        {
          double dt_accr = x.dt_accr0;
          if(x.accretion_radius)
            {
              const double m = x.mass[i];
              double dt_a = 1.e10;
              if(m >= 0.45 * x.smbh_mass && x.inner > 0)
                dt_a = x.acc_dt * pow((x.inner + 0.5 * hsml[i]), 1.5) / pow(m, 0.5);
              if(m < 0.45 * x.smbh_mass && x.sink > 0)
                dt_a = x.acc_dt * pow((x.sink + 0.5 * hsml[i]), 1.5) / pow(m, 0.5);
              if(dt_accr > dt_a)
                dt_accr = dt_a;
            }
          if(dt_accr < dt)
            dt = dt_accr;
        }
    }
  dt *= k.hubble_a;
  if(dt >= k.maxdt)
    dt = k.maxdt;
  if(dt >= k.dtdisp)
    dt = k.dtdisp;
  if(dt < k.mindt)
    {
      D_RAISE(888);   // timestep.c:1082
      return;
    }
  int ti_step = (int) (dt / k.timebase);
  if(!(ti_step > 0 && ti_step < GHIP_TIMEBASE))
    {
      D_RAISE(818);   // timestep.c:1119
      return;
    }
  // ---- advance_and_find_timesteps, timestep.c:146-175: power-of-two step, bin, synchronisation
  int ti_min = GHIP_TIMEBASE;
  while(ti_min > ti_step)
    ti_min >>= 1;
  ti_step = ti_min;
  if(ti_step == 1)
    {
      D_RAISE(112313);   // get_timestep_bin, timestep.c:1233
      return;
    }
  int bin = ti_step ? 31 - __clz(ti_step) : 0;
  const int binold = timebin[i];
  if(bin > binold && ((k.active >> bin) & 1u) == 0)
    {
      bin = binold;   // leave at old step if not synchronised
      ti_step = bin ? (1 << bin) : 0;
    }
  if(k.ti_current >= GHIP_TIMEBASE)
    {
      ti_step = 0;
      bin = 0;
    }
  if((GHIP_TIMEBASE - k.ti_current) < ti_step)
    {
      D_RAISE(888);   // timestep.c:171
      return;
    }
  timebin[i] = bin;
  const int ti_step_old = binold ? (1 << binold) : 0;
  const int tb0 = ti_begstep[i];
  const int tstart = tb0 + ti_step_old / 2;           // midpoint of old step
  const int tend = tb0 + ti_step_old + ti_step / 2;   // midpoint of new step
  const int tcurrent = tb0 + ti_step_old;
  ti_begstep[i] = tcurrent;
  bool grain = false;   // timestep.c:410-418: dv = 0, dust_drag has integrated the grain's velocity
  if constexpr(BUNDLE)
    {
      const KickB &x = d_kickb(xs...);
      if(x.virt && ty == 3)
        return;   // timestep.c:375-377: no kick, no force_kick_node
      grain = x.dust && ty == 2;
    }

  // ---- do_the_kick, timestep.c:378-395 ----
  double dt_entr, dt_gravkick, dt_hydrokick, dt_gravkick2, dt_hydrokick2;
  if(k.comoving)
    {
      dt_entr = (tend - tstart) * k.timebase;
      dt_gravkick = d_table_factor(k.tab.gravkick, tstart, tend, k.tab);
      dt_hydrokick = d_table_factor(k.tab.hydrokick, tstart, tend, k.tab);
      dt_gravkick2 = d_table_factor(k.tab.gravkick, tcurrent, tend, k.tab);
      dt_hydrokick2 = d_table_factor(k.tab.hydrokick, tcurrent, tend, k.tab);
    }
  else
    {
      dt_entr = dt_gravkick = dt_hydrokick = (tend - tstart) * k.timebase;
      dt_gravkick2 = dt_hydrokick2 = (tend - tcurrent) * k.timebase;
    }
  double v[3];
  if constexpr(BUNDLE)
    {
      for(int j = 0; j < 3; j++)
        v[j] = vel[(size_t) j * n + i] + (grain ? 0.0 : g[j] * dt_gravkick);
    }
  else
    for(int j = 0; j < 3; j++)
      v[j] = vel[(size_t) j * n + i] + g[j] * dt_gravkick;   // timestep.c:413-424
  if(gas)
    {
      for(int j = 0; j < 3; j++)
        {
          v[j] += hy[j] * dt_hydrokick;   // timestep.c:491-494
          double vp = v[j] - dt_gravkick2 * g[j] - dt_hydrokick2 * hy[j];
          if constexpr((... || std::is_same_v<X, KickR>))   // timestep.c:497-500: VelPred is SET, as the text has it
            {
              const double ra = d_kickr(xs...).ra[(size_t) j * ngas + i];
              v[j] += ra * dt_hydrokick;
              vp = v[j] - dt_hydrokick2 * ra;
            }
          if(k.pmgrid)
            vp += pm[j] * k.dt_gravkickB;   // timestep.c:511-513
          velpred[(size_t) j * ngas + i] = vp;
          if constexpr(BUNDLE)
            {
              const KickB &x = d_kickb(xs...);
              if(x.dust && x.drag)
                x.drag[(size_t) j * ngas + i] = 0.;   // timestep.c:508
            }
        }
      if constexpr((... || (std::is_same_v<X, KickV> || std::is_same_v<X, KickBV>)))   // timestep.c:530-533
        {
          const KickV &w = d_kickv(xs...);
          double al = w.alpha[i];
          al += w.dtalpha[i] * dt_entr;
          al = al < w.alpha_max ? al : w.alpha_max;   // DMIN
          if(al < w.alpha_min)
            al = w.alpha_min;
          w.alpha[i] = al;
        }
      double A = entropy[i], dA = dtentropy[i];
      if(dA * dt_entr > -0.5 * A)   // timestep.c:553-557
        A += dA * dt_entr;
      else
        A *= 0.5;
      if(k.minegy != 0)   // timestep.c:574-583
        {
          double minentropy = k.minegy * GAMMA_MINUS1 / pow(density[i] * k.a3inv, GAMMA_MINUS1);
          if(A < minentropy)
            {
              A = minentropy;
              dA = 0;
            }
        }
      dt_entr = (bin ? (1 << bin) : 0) / 2 * k.timebase;   // timestep.c:590-593
      if(A + dA * dt_entr < 0.5 * A)
        dA = -0.5 * A / dt_entr;
      entropy[i] = A;
      dtentropy[i] = dA;
    }
  // a kept tree (ghip_set_dynamic_tree): what force_kick_node(i, dv) receives, timestep.c:584-588
  if(kick_dv)
    {
      if constexpr(BUNDLE)
        {
          for(int j = 0; j < 3; j++)
            kick_dv[(size_t) j * n + i] =
              (grain ? 0.0 : g[j] * dt_gravkick) + (gas ? hy[j] * dt_hydrokick : 0.0);
        }
      else
        for(int j = 0; j < 3; j++)
          kick_dv[(size_t) j * n + i] = g[j] * dt_gravkick + (gas ? hy[j] * dt_hydrokick : 0.0);
      if constexpr((... || std::is_same_v<X, KickR>))   // timestep.c:498
        {
          if(gas)
            for(int j = 0; j < 3; j++)
              kick_dv[(size_t) j * n + i] += d_kickr(xs...).ra[(size_t) j * ngas + i] * dt_hydrokick;
        }
      kick_flag[i] = 1;
    }
  for(int j = 0; j < 3; j++)
    vel[(size_t) j * n + i] = v[j];
}

#undef D_RAISE

// TimeBinCount[] / TimeBinCountSph[] (allvars.h:337-338) recounted over all particles
__global__ void k_timebin_histogram(int n, const int *__restrict__ type,
                                    const int *__restrict__ timebin,
                                    unsigned long long *__restrict__ out)
{
  __shared__ unsigned int h[64];
  if(threadIdx.x < 64)
    h[threadIdx.x] = 0;
  __syncthreads();
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i < n)
    {
      int b = timebin[i] & 31;
      atomicAdd(&h[b], 1u);
      if(type[i] == 0)
        atomicAdd(&h[32 + b], 1u);
    }
  __syncthreads();
  if(threadIdx.x < 64 && h[threadIdx.x])
    atomicAdd(out + threadIdx.x, (unsigned long long) h[threadIdx.x]);
}

int ghip_timebin_hist(ghip_ctx *ctx, unsigned long long hist[64])
{
  memset(hist, 0, 64 * 8);
  const int n = ctx->n;
  if(n == 0)
    return GHIP_OK;
  hipStream_t st = ctx->stream;
  unsigned long long *dhist = ghip_words(ctx)->timebin_hist;
  HIPCHK(hipMemsetAsync(dhist, 0, 64 * 8, st));
  k_timebin_histogram<<<cdiv(n, 256), 256, 0, st>>>(n, P<int>(ctx->f[GHIP_F_TYPE]),
                                                    P<int>(ctx->f[GHIP_F_TIMEBIN]), dhist);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(hist, dhist, 64 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  return GHIP_OK;
}

extern "C" int ghip_timebin_counts(ghip_ctx *ctx, long long *TimeBinCount, long long *TimeBinCountSph)
{
  if(!ctx)
    return GHIP_EINVAL;
  if(TimeBinCount)
    memset(TimeBinCount, 0, 32 * sizeof(long long));
  if(TimeBinCountSph)
    memset(TimeBinCountSph, 0, 32 * sizeof(long long));
  if(ctx->n == 0)
    return GHIP_OK;
  unsigned long long hist[64];
  GCHK(ghip_timebin_hist(ctx, hist));
  for(int b = 0; b < 32; b++)
    {
      if(TimeBinCount)
        TimeBinCount[b] = (long long) hist[b];
      if(TimeBinCountSph)
        TimeBinCountSph[b] = (long long) hist[32 + b];
    }
  return ghip_check_device_errors(ctx);
}

// ---- the shipped bundle's rules: switches and the resident per-particle inputs ----
#define GHIP_C_LIGHT 2.9979e10   // allvars.h:86

static bool kick_sharded(const ghip_ctx *ctx)
{
  return ctx->shard_n > 1 || (ctx->dd.on && ctx->dd.nranks > 1);
}

// the arguments of k_advance_timesteps<true>; fails when fields were set for other particle counts
static int kick_bundle_args(ghip_ctx *ctx, KickB *x, const char *who)
{
  memset(x, 0, sizeof(*x));
  if(!ctx->iflags_on)
    return GHIP_OK;
  const ghip_integration_flags &f = ctx->iflags;
  x->dust = f.dust;
  x->dust_timestep = f.dust_timestep;
  x->black_holes = f.black_holes;
  x->accretion_radius = f.accretion_radius;
  x->virt = f.virtual_particles;
  // timestep.c:891-894, left to right as the host evaluates it; dt_ff = 1
  double dt_abs = 0.03 * f.OuterBoundary / GHIP_C_LIGHT * f.UnitVelocity_in_cm_per_s * f.FeedBackVelocity;
  double dt_ff = 1.;
  if(dt_abs > dt_ff)
    dt_abs = dt_ff;
  x->dt_abs = dt_abs;
  x->dt_accr0 = 0.03 * (f.OuterBoundary / 100.);   // timestep.c:910
  x->acc_dt = f.AccDtBlackHole;
  x->smbh_mass = f.SMBHmass;
  x->inner = f.InnerBoundary;
  x->sink = f.SinkBoundary;
  x->mass = P<double>(ctx->f[GHIP_F_MASS]);
  if((ctx->has_drag || ctx->has_ddm) && ctx->kick_fields_ngas != ctx->ngas)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: DragAccel / DeltaDustMomentum were set for %d gas particles, "
                     "the context has %d (ghip_kick_set_fields again)", who, ctx->kick_fields_ngas, ctx->ngas);
  x->drag = ctx->has_drag ? P<double>(ctx->kick_drag) : nullptr;
  x->ddm = ctx->has_ddm ? P<double>(ctx->kick_ddm) : nullptr;
  return GHIP_OK;
}

extern "C" int ghip_set_integration_flags(ghip_ctx *ctx, const ghip_integration_flags *f)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  ctx->iflags_on = f != nullptr;
  if(f)
    ctx->iflags = *f;
  else
    memset(&ctx->iflags, 0, sizeof(ctx->iflags));
  return GHIP_OK;
}

// host [m][3] -> device planes [3][m]
static int upload_planes(ghip_ctx *ctx, DevBuf &b, const double *h, int m)
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

extern "C" int ghip_kick_set_fields(ghip_ctx *ctx, const double *drag_accel, const double *gas_dust_momentum,
                                    const double *new_density)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  if((drag_accel || gas_dust_momentum || new_density) && kick_sharded(ctx))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_kick_set_fields: DragAccel / DeltaDustMomentum / NewDensity "
                     "are kept on single-rank contexts only (this one is sharded or multi-GPU)");
  const int n = ctx->n, ng = ctx->ngas;
  ctx->has_drag = ctx->has_ddm = ctx->has_newdens = false;
  if(drag_accel)
    GCHK(upload_planes(ctx, ctx->kick_drag, drag_accel, ng));
  if(gas_dust_momentum)
    GCHK(upload_planes(ctx, ctx->kick_ddm, gas_dust_momentum, ng));
  if(new_density)
    {
      GCHK(ghip_ensure(ctx, ctx->kick_newdens, (size_t) (n > 0 ? n : 1) * 8));
      if(n > 0)
        HIPCHK(hipMemcpyAsync(ctx->kick_newdens.p, new_density, (size_t) n * 8, hipMemcpyHostToDevice,
                              ctx->stream));
      HIPCHK(ghip_stream_sync(ctx, ctx->stream));
    }
  ctx->has_drag = drag_accel != nullptr;
  ctx->has_ddm = gas_dust_momentum != nullptr;
  ctx->has_newdens = new_density != nullptr;
  ctx->kick_fields_n = n;
  ctx->kick_fields_ngas = ng;
  return GHIP_OK;
}

extern "C" int ghip_kick_get_drag_accel(ghip_ctx *ctx, double *drag_accel)
{
  if(!ctx || !drag_accel)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  const int ng = ctx->ngas;
  if(!ctx->has_drag)
    {
      memset(drag_accel, 0, 3 * (size_t) ng * 8);
      return GHIP_OK;
    }
  if(ctx->kick_fields_ngas != ng)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_kick_get_drag_accel: DragAccel was set for %d gas particles, "
                     "the context has %d", ctx->kick_fields_ngas, ng);
  std::vector<double> t(3 * (size_t) ng);
  if(ng > 0)
    HIPCHK(hipMemcpyAsync(t.data(), ctx->kick_drag.p, t.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  for(int a = 0; a < ng; a++)
    for(int j = 0; j < 3; j++)
      drag_accel[3 * (size_t) a + j] = t[(size_t) j * ng + a];
  return ghip_check_device_errors(ctx);
}

// device planes [3][m] -> host [m][3]
static int download_planes(ghip_ctx *ctx, const DevBuf &b, double *h, int m)
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

extern "C" int ghip_kick_get_fields(ghip_ctx *ctx, double *drag_accel, double *gas_dust_momentum,
                                    double *new_density, int held[3])
{
  if(!ctx || !held)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  const int n = ctx->n, ng = ctx->ngas;
  const bool ok = ctx->kick_fields_n == n && ctx->kick_fields_ngas == ng;
  held[0] = ok && ctx->has_drag;
  held[1] = ok && ctx->has_ddm;
  held[2] = ok && ctx->has_newdens;
  if(drag_accel && held[0])
    GCHK(download_planes(ctx, ctx->kick_drag, drag_accel, ng));
  if(gas_dust_momentum && held[1])
    GCHK(download_planes(ctx, ctx->kick_ddm, gas_dust_momentum, ng));
  if(new_density && held[2] && n > 0)
    {
      HIPCHK(hipMemcpyAsync(new_density, ctx->kick_newdens.p, (size_t) n * 8, hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ghip_stream_sync(ctx, ctx->stream));
    }
  return GHIP_OK;
}

extern "C" int ghip_advance_timesteps(ghip_ctx *ctx, const ghip_kick_params *p,
                                      long long *TimeBinCount, long long *TimeBinCountSph)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !p)
    return GHIP_EINVAL;
  if(p->ComovingIntegrationOn && (!p->GravKickTable || !p->HydroKickTable))
    return ghip_fail(ctx, GHIP_EINVAL,
                     "ghip_advance_timesteps: comoving kicks need the factor tables");
  if(!(p->Timebase_interval > 0))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_advance_timesteps: Timebase_interval must be > 0");
  GCHK(ghip_visc_ready(ctx, "ghip_advance_timesteps"));
  int n = ctx->n, ng = ctx->ngas;
  if(TimeBinCount)
    memset(TimeBinCount, 0, 32 * sizeof(long long));
  if(TimeBinCountSph)
    memset(TimeBinCountSph, 0, 32 * sizeof(long long));
  if(n == 0)
    return GHIP_OK;
  hipStream_t st = ctx->stream;
  KickK k;
  memset(&k, 0, sizeof(k));
  k.ti_current = p->Ti_Current;
  k.timebase = p->Timebase_interval;
  k.comoving = p->ComovingIntegrationOn;
  k.time = p->Time;
  if(k.comoving)
    {
      // timestep.c:52-60, evaluated on the host exactly as the reference does
      k.fac1 = 1 / (p->Time * p->Time);
      k.fac2 = 1 / pow(p->Time, 3 * GAMMA - 2);
      k.fac3 = pow(p->Time, 3 * (1 - GAMMA) / 2.0);
      k.hubble_a = p->hubble_a;
      k.a3inv = 1 / (p->Time * p->Time * p->Time);
      k.atime = p->Time;
    }
  else
    k.fac1 = k.fac2 = k.fac3 = k.hubble_a = k.a3inv = k.atime = 1;
  k.errtol = p->ErrTolIntAccuracy;
  k.courant = p->CourantFac;
  k.maxdt = p->MaxSizeTimestep;
  k.mindt = p->MinSizeTimestep;
  k.dtdisp = p->dt_displacement;
  for(int t = 0; t < 6; t++)
    k.soft[t] = p->SofteningTable[t];
  k.adaptive_hsml = p->AdaptiveGravsoftForGasHsml;
  k.pmgrid = p->pmgrid;
  k.dt_gravkickB = p->dt_gravkickB;
  k.minegy = p->MinEgySpec;
  k.active = p->TimeBinActive;
  k.tab.timebase = p->Timebase_interval;
  k.tab.logTimeBegin = p->logTimeBegin;
  k.tab.logTimeMax = p->logTimeMax;
  int *derr = &ghip_words(ctx)->step_err;
  HIPCHK(hipMemsetAsync(derr, 0, 4, st));
  GCHK(ghip_ensure(ctx, ctx->stage, (2 * DRIFT_TABLE_LENGTH + 64) * 8));
  double *d = P<double>(ctx->stage);
  if(k.comoving)
    {
      HIPCHK(hipMemcpyAsync(d, p->GravKickTable, DRIFT_TABLE_LENGTH * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(d + DRIFT_TABLE_LENGTH, p->HydroKickTable, DRIFT_TABLE_LENGTH * 8,
                            hipMemcpyHostToDevice, st));
      k.tab.gravkick = d;
      k.tab.hydrokick = d + DRIFT_TABLE_LENGTH;
    }
  const int nact = ctx->nactive < 0 ? n : ctx->nactive;
  const int *act = ctx->nactive < 0 ? nullptr : P<int>(ctx->act_host_idx);
  HIPCHK(hipEventRecord(ctx->evp[12], st));
  // with a kept tree the kicks are recorded and handed to the nodes (force_kick_node inside
  // do_the_kick, force_finish_kick_nodes at the end of advance_and_find_timesteps, timestep.c:256-263)
  const bool record = ctx->dyn_on && ctx->dyn_valid && ctx->dyn.tree.n == n;
  if(record)
    {
      GCHK(ghip_ensure(ctx, ctx->dyn.kick_dv, 4 * (size_t) n * 8));
      GCHK(ghip_ensure(ctx, ctx->dyn.kick_flag, (size_t) n * 4));
      HIPCHK(hipMemsetAsync(ctx->dyn.kick_flag.p, 0, (size_t) n * 4, st));
    }
  KickB x;
  GCHK(kick_bundle_args(ctx, &x, "ghip_advance_timesteps"));
  KickR r = {nullptr};   // ghip_set_rad_accel: the instantiations with RadAccel, else the kernels as they were
  GCHK(ghip_rad_accel_field(ctx, "ghip_advance_timesteps", &r.ra));
  // the arguments every instantiation takes, before its pack
#define KICK_ARGS                                                                                          \
  nact, act, n, ng, k, P<int>(ctx->f[GHIP_F_TYPE]), P<double>(ctx->f[GHIP_F_VEL]),                         \
    P<double>(ctx->f[GHIP_F_GRAVACCEL]), P<double>(ctx->f[GHIP_F_GRAVPM]),                                 \
    P<double>(ctx->f[GHIP_F_HYDROACCEL]), P<double>(ctx->f[GHIP_F_VELPRED]),                               \
    P<double>(ctx->f[GHIP_F_ENTROPY]), P<double>(ctx->f[GHIP_F_DTENTROPY]),                                \
    P<double>(ctx->f[GHIP_F_DENSITY]), P<double>(ctx->f[GHIP_F_HSML]),                                     \
    P<double>(ctx->f[GHIP_F_MAXSIGNALVEL]), P<int>(ctx->f[GHIP_F_TIMEBIN]),                                \
    P<int>(ctx->f[GHIP_F_TI_BEGSTEP]), derr, ctx->async ? ghip_errword(ctx, GHIP_ERRW_TIMESTEP) : nullptr, \
    record ? P<double>(ctx->dyn.kick_dv) : nullptr, record ? P<int>(ctx->dyn.kick_flag) : nullptr
  if(nact > 0 && r.ra && ctx->visc_on && ctx->visc.time_dependent)
    {
      const KickV w = {P<double>(ctx->visc_alpha), P<double>(ctx->visc_dtalpha), ctx->visc.ArtBulkViscConst,
                       ctx->visc.AlphaMin};
      if(ctx->iflags_on)
        {
          KickBV xw;
          static_cast<KickB &>(xw) = x;
          xw.v = w;
          k_advance_timesteps<true><<<cdiv(nact, 256), 256, 0, st>>>(KICK_ARGS, r, xw);
        }
      else
        k_advance_timesteps<false><<<cdiv(nact, 256), 256, 0, st>>>(KICK_ARGS, r, w);
      ctx->visc_epoch++;
    }
  else if(nact > 0 && r.ra && ctx->iflags_on)
    k_advance_timesteps<true><<<cdiv(nact, 256), 256, 0, st>>>(KICK_ARGS, r, x);
  else if(nact > 0 && r.ra)
    k_advance_timesteps<false><<<cdiv(nact, 256), 256, 0, st>>>(KICK_ARGS, r);
  else if(nact > 0 && ctx->visc_on && ctx->visc.time_dependent)
    {
      const KickV w = {P<double>(ctx->visc_alpha), P<double>(ctx->visc_dtalpha), ctx->visc.ArtBulkViscConst,
                       ctx->visc.AlphaMin};
      if(ctx->iflags_on)
        {
          KickBV xw;
          static_cast<KickB &>(xw) = x;
          xw.v = w;
          k_advance_timesteps<true><<<cdiv(nact, 256), 256, 0, st>>>(KICK_ARGS, xw);
        }
      else
        k_advance_timesteps<false><<<cdiv(nact, 256), 256, 0, st>>>(KICK_ARGS, w);
      ctx->visc_epoch++;   // (alpha changed: ghosts packed before this carry the old one)
    }
  else if(nact > 0 && ctx->iflags_on)
    k_advance_timesteps<true><<<cdiv(nact, 256), 256, 0, st>>>(KICK_ARGS, x);
  else if(nact > 0)
    k_advance_timesteps<false><<<cdiv(nact, 256), 256, 0, st>>>(KICK_ARGS);
#undef KICK_ARGS
  if(record && nact > 0)
    GCHK(ghip_dyn_kick_recorded(ctx));
  HIPCHK(hipEventRecord(ctx->evp[13], st));
  HIPCHK(hipGetLastError());
  const bool want_counts = TimeBinCount || TimeBinCountSph;
  if(ctx->async && !want_counts)
    return GHIP_OK;   // (a failed criterion is reported by the next call that synchronises)
  int herr = 0;
  HIPCHK(hipMemcpyAsync(&herr, derr, 4, hipMemcpyDeviceToHost, st));
  if(want_counts)
    {
      int rc = ghip_timebin_counts(ctx, TimeBinCount, TimeBinCountSph);   // (synchronises)
      if(rc != GHIP_OK && rc != GHIP_ETIMESTEP)
        return rc;
    }
  else
    HIPCHK(ghip_stream_sync(ctx, st));
  if(herr)
    {
      ghip_fail(ctx, GHIP_ETIMESTEP,
                "ghip_advance_timesteps: the reference stops here with endrun(%d) "
                "(timestep.c:171/1082: 888, :1119: 818, :1233: 112313)",
                herr);
      ctx->timestep_endrun = herr;
      *ghip_errword(ctx, GHIP_ERRW_TIMESTEP) = 0;
      return GHIP_ETIMESTEP;
    }
  ctx->timestep_endrun = 0;
  return GHIP_OK;
}

extern "C" int ghip_timestep_endrun_code(const ghip_ctx *ctx)
{
  return ctx ? ctx->timestep_endrun : 0;
}

// ---- per-type sums of find_dt_displacement_constraint (timestep.c:1140-1156) -----------------
// stage 1: one partial per block and type (fixed tree order inside the block); stage 2: the
// partials of a type are added in block order by one thread -- deterministic.
__global__ void k_vel_moments(int n, const int *__restrict__ type, const double *__restrict__ vel,
                              const double *__restrict__ mass, double *__restrict__ pv2,
                              double *__restrict__ pmin, unsigned int *__restrict__ pcnt)
{
  __shared__ double sv[256], sm[256];
  __shared__ unsigned int sc[256];
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int ty = -1;
  double v2 = 0, m = 1.0e30;
  if(i < n)
    {
      ty = type[i];
      double a = vel[i], b = vel[(size_t) n + i], c = vel[2 * (size_t) n + i];
      v2 = a * a + b * b + c * c;
      double mi = mass[i];
      if(mi > 0)
        m = mi;
    }
  for(int t = 0; t < 6; t++)
    {
      sv[threadIdx.x] = (ty == t) ? v2 : 0.0;
      sm[threadIdx.x] = (ty == t) ? m : 1.0e30;
      sc[threadIdx.x] = (ty == t) ? 1u : 0u;
      __syncthreads();
      for(unsigned int s = 128; s > 0; s >>= 1)
        {
          if(threadIdx.x < s)
            {
              sv[threadIdx.x] += sv[threadIdx.x + s];
              sm[threadIdx.x] = fmin(sm[threadIdx.x], sm[threadIdx.x + s]);
              sc[threadIdx.x] += sc[threadIdx.x + s];
            }
          __syncthreads();
        }
      if(threadIdx.x == 0)
        {
          pv2[(size_t) t * gridDim.x + blockIdx.x] = sv[0];
          pmin[(size_t) t * gridDim.x + blockIdx.x] = sm[0];
          pcnt[(size_t) t * gridDim.x + blockIdx.x] = sc[0];
        }
      __syncthreads();
    }
}

__global__ void k_vel_moments_final(int nblocks, const double *__restrict__ pv2,
                                    const double *__restrict__ pmin,
                                    const unsigned int *__restrict__ pcnt, double *__restrict__ out)
{
  int t = threadIdx.x;
  if(t >= 6)
    return;
  double v = 0, m = 1.0e30;
  unsigned long long c = 0;
  for(int b = 0; b < nblocks; b++)
    {
      v += pv2[(size_t) t * nblocks + b];
      m = fmin(m, pmin[(size_t) t * nblocks + b]);
      c += pcnt[(size_t) t * nblocks + b];
    }
  out[t] = v;
  out[6 + t] = m;
  out[12 + t] = (double) c;
}

extern "C" int ghip_velocity_moments(ghip_ctx *ctx, double v2sum[6], double min_mass[6],
                                     long long count[6])
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !v2sum || !min_mass || !count)
    return GHIP_EINVAL;
  int n = ctx->n;
  for(int t = 0; t < 6; t++)
    {
      v2sum[t] = 0;
      min_mass[t] = 1.0e30;
      count[t] = 0;
    }
  if(n == 0)
    return GHIP_OK;
  hipStream_t st = ctx->stream;
  int nb = cdiv(n, 256);
  GCHK(ghip_ensure(ctx, ctx->stage, (size_t) nb * 6 * (8 + 8 + 4) + 64 * 8));
  double *pv2 = P<double>(ctx->stage), *pmin = pv2 + (size_t) 6 * nb, *out = pmin + (size_t) 6 * nb;
  unsigned int *pcnt = reinterpret_cast<unsigned int *>(out + 24);
  k_vel_moments<<<nb, 256, 0, st>>>(n, P<int>(ctx->f[GHIP_F_TYPE]), P<double>(ctx->f[GHIP_F_VEL]),
                                    P<double>(ctx->f[GHIP_F_MASS]), pv2, pmin, pcnt);
  k_vel_moments_final<<<1, 64, 0, st>>>(nb, pv2, pmin, pcnt, out);
  HIPCHK(hipGetLastError());
  double h[18];
  HIPCHK(hipMemcpyAsync(h, out, sizeof(h), hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  for(int t = 0; t < 6; t++)
    {
      v2sum[t] = h[t];
      min_mass[t] = h[6 + t];
      count[t] = (long long) h[12 + t];
    }
  return GHIP_OK;
}

// The long-range kick at the end of a PM step (timestep.c:269-345): every particle gets
// Vel += GravPM * dt_gravkick; the predicted velocity of every gas particle is rebuilt from the new
// Vel at the current time (its own step's mid-point kicks + the new PM half-step dt_gravkickB).
// X... is empty for the kernel as it was and one KickR under ghip_set_rad_accel (timestep.c:337-339)
template <class... X>
__global__ void k_pm_kick(int n, int ngas, int ti_current, DriftK tab, double dt_gravkick,
                          double dt_gravkickB, const int *__restrict__ type,
                          const int *__restrict__ timebin, const int *__restrict__ ti_begstep,
                          double *__restrict__ vel, const double *__restrict__ gravaccel,
                          const double *__restrict__ gravpm, const double *__restrict__ hydroaccel,
                          double *__restrict__ velpred, X... xs)
{
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  double pm[3], v[3];
  for(int j = 0; j < 3; j++)
    {
      pm[j] = gravpm[(size_t) j * n + i];
      v[j] = vel[(size_t) j * n + i] + pm[j] * dt_gravkick;   // timestep.c:313
      vel[(size_t) j * n + i] = v[j];
    }
  if(type[i] == 0 && i < ngas)
    {
      const int tb = timebin[i];
      const int dt_step = tb ? (1 << tb) : 0;   // timestep.c:317
      const int t0 = ti_begstep[i];
      double dt_gravkickA, dt_hydrokick;
      if(tab.comoving)   // timestep.c:319-325
        {
          dt_gravkickA = d_table_factor(tab.gravkick, t0, ti_current, tab) -
                         d_table_factor(tab.gravkick, t0, t0 + dt_step / 2, tab);
          dt_hydrokick = d_table_factor(tab.hydrokick, t0, ti_current, tab) -
                         d_table_factor(tab.hydrokick, t0, t0 + dt_step / 2, tab);
        }
      else
        dt_gravkickA = dt_hydrokick = (ti_current - (t0 + dt_step / 2)) * tab.timebase;
      for(int j = 0; j < 3; j++)   // timestep.c:330-333
        velpred[(size_t) j * ngas + i] = v[j] + gravaccel[(size_t) j * n + i] * dt_gravkickA +
                                         hydroaccel[(size_t) j * ngas + i] * dt_hydrokick +
                                         pm[j] * dt_gravkickB;
      if constexpr(sizeof...(X) > 0)   // timestep.c:337-339: VelPred is SET
        for(int j = 0; j < 3; j++)
          velpred[(size_t) j * ngas + i] = v[j] + d_kickr(xs...).ra[(size_t) j * ngas + i] * dt_hydrokick;
    }
}

extern "C" int ghip_pm_kick(ghip_ctx *ctx, const ghip_pmkick_params *p)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !p)
    return GHIP_EINVAL;
  if(p->ComovingIntegrationOn && (!p->GravKickTable || !p->HydroKickTable))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_pm_kick: comoving integration needs the kick tables");
  const int n = ctx->n, ng = ctx->ngas;
  if(n == 0)
    return GHIP_OK;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DriftK tab;
  memset(&tab, 0, sizeof(tab));
  tab.timebase = p->Timebase_interval;
  tab.comoving = p->ComovingIntegrationOn;
  tab.logTimeBegin = p->logTimeBegin;
  tab.logTimeMax = p->logTimeMax;
  if(p->ComovingIntegrationOn)
    {
      GCHK(ghip_ensure(ctx, ctx->stage, 3 * DRIFT_TABLE_LENGTH * 8));
      double *d = P<double>(ctx->stage);
      HIPCHK(hipMemcpyAsync(d + DRIFT_TABLE_LENGTH, p->GravKickTable, DRIFT_TABLE_LENGTH * 8,
                            hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(d + 2 * DRIFT_TABLE_LENGTH, p->HydroKickTable, DRIFT_TABLE_LENGTH * 8,
                            hipMemcpyHostToDevice, st));
      tab.gravkick = d + DRIFT_TABLE_LENGTH;
      tab.hydrokick = d + 2 * DRIFT_TABLE_LENGTH;
    }
  KickR r = {nullptr};
  GCHK(ghip_rad_accel_field(ctx, "ghip_pm_kick", &r.ra));
#define PMKICK_ARGS                                                                                    \
  n, ng, p->Ti_Current, tab, p->dt_gravkick, p->dt_gravkickB, P<int>(ctx->f[GHIP_F_TYPE]),             \
    P<int>(ctx->f[GHIP_F_TIMEBIN]), P<int>(ctx->f[GHIP_F_TI_BEGSTEP]), P<double>(ctx->f[GHIP_F_VEL]),  \
    P<double>(ctx->f[GHIP_F_GRAVACCEL]), P<double>(ctx->f[GHIP_F_GRAVPM]),                             \
    P<double>(ctx->f[GHIP_F_HYDROACCEL]), P<double>(ctx->f[GHIP_F_VELPRED])
  if(r.ra)
    k_pm_kick<<<cdiv(n, 256), 256, 0, st>>>(PMKICK_ARGS, r);
  else
    k_pm_kick<<<cdiv(n, 256), 256, 0, st>>>(PMKICK_ARGS);
#undef PMKICK_ARGS
  HIPCHK(hipGetLastError());
  return GHIP_OK;
}
