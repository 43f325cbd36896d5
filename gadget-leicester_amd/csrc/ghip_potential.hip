// ghip_potential.hip -- compute_potential() (potential.c:22-325) and the per-type sums of
// compute_global_quantities_of_system() (global.c:18-238) on gfx950.
//
// The potential walk is a kernel of its own, not a mode of k_grav_walk (ghip_walk.h): it is a
// diagnostic that runs every TimeBetStatistics, and the tuned force walk stays as it is.  It reads
// the same 64-byte element records (WalkHot / WalkCold) of the tree the gravity walks would use at
// this moment (the tree of the current positions, or the kept tree of ghip_set_dynamic_tree).
//
// Mapping: one lane per target, ALL particles of the context are targets (potential.c:88-97), in
// tree (curve) order so that the lanes of a wavefront walk similar paths.  Each lane follows the
// pre-order list with its own cursor: e + 1 opens a node or steps past a particle, the node's skip
// index accepts it -- the reference's nextnode / sibling order, so every lane adds its terms in the
// reference's order.  Plain loads (the records are wave-divergent here), no inline assembly.
//
// Floating-point contraction is off in this file: the opening decisions and the sums are the
// reference's operations one by one, so a restatement in numpy reproduces them.
#pragma clang fp contract(off)

#include <cmath>

#include "ghip_internal.h"
#include "ghip_walkrec.h"
#include "ghip_timefac.h"

#define GHIP_POT_ORIGIN 2.8372975   // potcorr[0][0][0] and the comoving self term (forcetree.c:4479,
                                    // potential.c:253)

struct PotK
{
  double theta, errtol;
  double boxsize, boxhalf;
  double rcut, asmthfac;   // short-range walk (forcetree.c:3805-3812)
  double fac_intp;         // 2 EN / BoxSize (forcetree.c:4517)
};

// ewald_pot_corr (forcetree.c:4633-4684) on the (EN+1)^3 table of psi / BoxSize
__device__ __forceinline__ double d_ewald_pot_corr(const double *__restrict__ tab, double fac_intp,
                                                   double dx, double dy, double dz)
{
  const int E1 = GHIP_EN + 1;
  if(dx < 0)
    dx = -dx;
  if(dy < 0)
    dy = -dy;
  if(dz < 0)
    dz = -dz;
  double u = dx * fac_intp;
  int i = (int) u;
  if(i >= GHIP_EN)
    i = GHIP_EN - 1;
  u -= i;
  double v = dy * fac_intp;
  int j = (int) v;
  if(j >= GHIP_EN)
    j = GHIP_EN - 1;
  v -= j;
  double w = dz * fac_intp;
  int k = (int) w;
  if(k >= GHIP_EN)
    k = GHIP_EN - 1;
  w -= k;
  const double f1 = (1 - u) * (1 - v) * (1 - w), f2 = (1 - u) * (1 - v) * (w);
  const double f3 = (1 - u) * (v) * (1 - w), f4 = (1 - u) * (v) * (w);
  const double f5 = (u) * (1 - v) * (1 - w), f6 = (u) * (1 - v) * (w);
  const double f7 = (u) * (v) * (1 - w), f8 = (u) * (v) * (w);
  const double *t00 = tab + ((size_t) i * E1 + j) * E1 + k;   // [i][j][k]
  const double *t01 = t00 + E1;                                 // [i][j+1][k]
  const double *t10 = t00 + (size_t) E1 * E1;                   // [i+1][j][k]
  const double *t11 = t10 + E1;                                 // [i+1][j+1][k]
  return t00[0] * f1 + t00[1] * f2 + t01[0] * f3 + t01[1] * f4 + t10[0] * f5 + t10[1] * f6 +
         t11[0] * f7 + t11[1] * f8;
}

// the spline potential of forcetree.c:3496-3510 (times mass / h); -mass / r outside h
__device__ __forceinline__ double d_pot_term(double mass, double r, double h)
{
  if(r >= h)
    return -mass / r;
  const double h_inv = 1.0 / h;
  const double u = r * h_inv;
  double wp;
  if(u < 0.5)
    wp = -2.8 + u * u * (5.333333333333 + u * u * (6.4 * u - 9.6));
  else
    wp = -3.2 + 0.066666666667 / u +
         u * u * (10.666666666667 + u * (-16.0 + u * (9.6 - 2.133333333333 * u)));
  return mass * h_inv * wp;
}

// force_treeevaluate_potential (forcetree.c:3217-3530; PERIODIC: NEAREST and the Ewald potential
// correction with every interaction) and force_treeevaluate_potential_shortrange (:3752-4115, SHORT).
// UNEQUAL: the softening rules of UNEQUALSOFTENINGS, with ADAPTIVE_GRAVSOFT_FORGAS folded into the
// records (a particle's aux is its softening -- Hsml for gas --, a node's aux is its largest
// softening, negative when the node opens for every target inside it: mixed softenings, or always
// with adaptive softening).
// SHARD (GHIP_DD_POTENTIAL): the tree is the merged one of a multi-GPU shard.  Its n sources are the shard's
// own particles (perm < nlocal) and what was imported, particles and pruned nodes (perm >= nlocal): sources,
// never targets.  A lane that has to open an imported pruned node (a node whose skip link is e + 1) reports
// it through errw, as the force walk does (ghip_walk.h).
template <bool PERIODIC, bool SHORT, bool UNEQUAL, bool REL, bool SHARD>
__global__ void __launch_bounds__(256)
  k_pot_walk(const TreeSizes *__restrict__ ts, int n, const WalkHot *__restrict__ hot,
             const WalkCold *__restrict__ cold, const double *__restrict__ tx,
             const double *__restrict__ ty, const double *__restrict__ tz,
             const double *__restrict__ tsoft, const double *__restrict__ toldacc,
             const int *__restrict__ perm, const double *__restrict__ potcorr,
             const float *__restrict__ srpot, PotK k, double *__restrict__ pot_out,
             unsigned long long *__restrict__ nint_out, int nlocal, int *errw)
{
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if(s >= n)
    return;
  if(SHARD && perm[s] >= nlocal)
    return;
  const int nelem = ts->nelem;
  const double px = tx[s], py = ty[s], pz = tz[s];
  const double hi = tsoft[s];
  const double aold = REL ? k.errtol * toldacc[s] : 0.0;
  double pot = 0;
  unsigned int nint = 0;
  int e = 0;
  while(e < nelem)
    {
      const WalkHot H = hot[e];
      double dx = H.x - px, dy = H.y - py, dz = H.z - pz;
      if(PERIODIC)
        {
          dx = d_nearest(dx, k.boxsize, k.boxhalf);
          dy = d_nearest(dy, k.boxsize, k.boxhalf);
          dz = d_nearest(dz, k.boxsize, k.boxhalf);
        }
      const double r2 = dx * dx + dy * dy + dz * dz;
      double h = hi;
      int next;
      if(H.pidx >= 0)
        {
          if(UNEQUAL && h < H.aux)
            h = H.aux;
          next = e + 1;
        }
      else
        {
          if(SHORT)
            {
              // the whole cell beyond the cut-off: drop the branch (forcetree.c:3900-3929)
              const WalkCold C = cold[e];
              const double eff = k.rcut + 0.5 * C.len;
              double dxx = C.cx - px, dyy = C.cy - py, dzz = C.cz - pz;
              if(PERIODIC)
                {
                  dxx = d_nearest(dxx, k.boxsize, k.boxhalf);
                  dyy = d_nearest(dyy, k.boxsize, k.boxhalf);
                  dzz = d_nearest(dzz, k.boxsize, k.boxhalf);
                }
              if(dxx < -eff || dxx > eff || dyy < -eff || dyy > eff || dzz < -eff || dzz > eff)
                {
                  e = H.skip;
                  continue;
                }
            }
          bool open;
          if(REL)
            {
              open = H.mlen2 > r2 * r2 * aold;
              if(!open)
                {
                  // the 0.6 len box test against the unwrapped centre - pos (forcetree.c:3439-3450)
                  const WalkCold C = cold[e];
                  open = fabs(C.cx - px) < C.len06 && fabs(C.cy - py) < C.len06 &&
                         fabs(C.cz - pz) < C.len06;
                }
            }
          else
            open = H.len2 > r2 * k.theta * k.theta;
          if(!open && UNEQUAL)
            {
              const double ms = fabs(H.aux);
              if(h < ms)
                {
                  h = ms;
                  if(H.aux < 0 && r2 < h * h)
                    open = true;
                }
            }
          if(open)
            {
              if(SHARD && H.skip == e + 1)
                *(volatile int *) errw = 1;
              e = e + 1;
              continue;
            }
          next = H.skip;
        }
      const double r = sqrt(r2);
      if(SHORT)
        {
          const int tabindex = (int) (r * k.asmthfac);
          if(tabindex < GHIP_NTAB)
            {
              // (-fac * mass / r and fac * mass * h_inv * wp: the product fac * mass first, as :4082-4096)
              const double fac = srpot[tabindex];
              pot += d_pot_term(fac * H.m, r, h);
              nint++;
            }
        }
      else
        {
          pot += d_pot_term(H.m, r, h);
          if(PERIODIC)
            pot += H.m * d_ewald_pot_corr(potcorr, k.fac_intp, dx, dy, dz);
          nint++;
        }
      e = next;
    }
  pot_out[perm[s]] = pot;
  if(nint_out)
    nint_out[perm[s]] = nint;
}

// potcorr of ewald_init (forcetree.c:4466-4481, 4518-4525): psi(x) / BoxSize at x = 0.5 (i,j,k) / EN,
// 2.8372975 / BoxSize at the origin; ewald_psi is forcetree.c:4686-4720
__global__ void k_ewald_pot_table(double boxsize, double *__restrict__ tab)
{
  const int E1 = GHIP_EN + 1;
  const int nidx = blockIdx.x * blockDim.x + threadIdx.x;
  if(nidx >= E1 * E1 * E1)
    return;
  const int i = nidx / (E1 * E1), j = (nidx / E1) % E1, kk = nidx % E1;
  double psi;
  if(i + j + kk == 0)
    psi = GHIP_POT_ORIGIN;
  else
    {
      const double alpha = 2.0;
      const double x0 = 0.5 * ((double) i) / GHIP_EN, x1 = 0.5 * ((double) j) / GHIP_EN,
                   x2 = 0.5 * ((double) kk) / GHIP_EN;
      double sum1 = 0;
      for(int n0 = -4; n0 <= 4; n0++)
        for(int n1 = -4; n1 <= 4; n1++)
          for(int n2 = -4; n2 <= 4; n2++)
            {
              const double d0 = x0 - n0, d1 = x1 - n1, d2 = x2 - n2;
              const double r = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
              sum1 += erfc(alpha * r) / r;
            }
      double sum2 = 0;
      for(int h0 = -4; h0 <= 4; h0++)
        for(int h1 = -4; h1 <= 4; h1++)
          for(int h2i = -4; h2i <= 4; h2i++)
            {
              const double hdotx = x0 * h0 + x1 * h1 + x2 * h2i;
              const int h2 = h0 * h0 + h1 * h1 + h2i * h2i;
              if(h2 > 0)
                sum2 += 1 / (M_PI * h2) * exp(-M_PI * M_PI * h2 / (alpha * alpha)) *
                        cos(2 * M_PI * hdotx);
            }
      const double r = sqrt(x0 * x0 + x1 * x1 + x2 * x2);
      psi = M_PI / (alpha * alpha) - sum1 - sum2 + 1 / r;
    }
  tab[nidx] = psi / boxsize;
}

// potential.c:245-259: the self term, the comoving periodic background term, the factor G
__global__ void k_pot_finish(int n, const double *__restrict__ mass, const int *__restrict__ type,
                             double soft0, double soft1, double soft2, double soft3, double soft4,
                             double soft5, double bgfac, double G, double *__restrict__ pot)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  const int t = type[i];
  const double st = t == 0 ? soft0 : t == 1 ? soft1 : t == 2 ? soft2 : t == 3 ? soft3 : t == 4 ? soft4 : soft5;
  double p = pot[i];
  const double m = mass[i];
  p += m / st;
  if(bgfac != 0)
    p -= GHIP_POT_ORIGIN * pow(m, 2.0 / 3) * bgfac;
  pot[i] = p * G;
}

// potential.c:303-325: fac * r^2 with fac = -1/2 Omega0 H^2 (comoving, not periodic) or
// -1/2 OmegaLambda H^2 (physical)
__global__ void k_pot_quadratic(int n, const double *__restrict__ pos, double fac,
                                double *__restrict__ pot)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  double r2 = 0;
  for(int k = 0; k < 3; k++)
    r2 += pos[(size_t) k * n + i] * pos[(size_t) k * n + i];
  pot[i] += fac * r2;
}

static int ensure_pot_table(ghip_ctx *ctx, double BoxSize)
{
  if(ctx->potcorr_box == BoxSize)
    return GHIP_OK;
  const int E1 = GHIP_EN + 1;
  const int nt = E1 * E1 * E1;
  GCHK(ghip_ensure(ctx, ctx->potcorr, (size_t) nt * sizeof(double)));
  k_ewald_pot_table<<<cdiv(nt, 64), 64, 0, ctx->stream>>>(BoxSize, P<double>(ctx->potcorr));
  HIPCHK(hipGetLastError());
  ctx->potcorr_box = BoxSize;
  return GHIP_OK;
}

static int ensure_srpot_table(ghip_ctx *ctx)
{
  if(ctx->srpot.p)
    return GHIP_OK;
  // forcetree.c:4195-4202: shortrange_table_potential[i] = erfc(u), a float table as in the reference
  float tab[GHIP_NTAB];
  for(int i = 0; i < GHIP_NTAB; i++)
    {
      const double u = 3.0 / GHIP_NTAB * (i + 0.5);
      tab[i] = (float) erfc(u);
    }
  GCHK(ghip_ensure(ctx, ctx->srpot, sizeof(tab)));
  HIPCHK(hipMemcpyAsync(ctx->srpot.p, tab, sizeof(tab), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  return GHIP_OK;
}

extern "C" int ghip_ewald_get_pot_table(ghip_ctx *ctx, double BoxSize, double *host)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !host || !(BoxSize > 0))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_ewald_get_pot_table: need BoxSize > 0 and an output");
  GCHK(ensure_pot_table(ctx, BoxSize));
  const int E1 = GHIP_EN + 1;
  HIPCHK(hipMemcpyAsync(host, ctx->potcorr.p, (size_t) E1 * E1 * E1 * sizeof(double),
                        hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  return GHIP_OK;
}

// the argument rules of ghip_potential (and of GHIP_DD_POTENTIAL): everything is checked here, before
// anything is launched
static int pot_check(ghip_ctx *ctx, const ghip_pot_params *p, const char *who)
{
  const ghip_grav_params &g = p->grav;
  if(p->pm.pmgrid != 0)
    GCHK(ghip_pm_pot_check(ctx, p, who));
  if(g.periodic && !(g.BoxSize > 0))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: periodic needs BoxSize > 0", who);
  for(int t = 0; t < 6; t++)
    if(!(p->SofteningTable[t] > 0))
      return ghip_fail(ctx, GHIP_EINVAL, "%s: SofteningTable[%d] must be > 0", who, t);
  const bool rel = g.ErrTolTheta == 0;   // (only the relative criterion reads OldAcc)
  for(int f : {GHIP_F_POS, GHIP_F_MASS, GHIP_F_TYPE, GHIP_F_OLDACC})
    if(ctx->n > 0 && !ctx->f[f].p && (f != GHIP_F_OLDACC || rel))
      return ghip_fail(ctx, GHIP_EINVAL, "%s: particle field %d not set", who, f);
  return GHIP_OK;
}

// the walk of the gravity tree in place for the context's own particles and potential.c:245-259 (self term,
// comoving periodic background, * G).  shard: the tree is the merged tree of a multi-GPU shard.
static int pot_walk_and_finish(ghip_ctx *ctx, const ghip_pot_params *p, bool shard)
{
  const ghip_grav_params &g = p->grav;
  const int pmgrid = p->pm.pmgrid;
  const bool rel = g.ErrTolTheta == 0;
  const int n = ctx->n;
  const int nt = shard ? ctx->gt.n : n;   // lanes: the sources of the tree, own particles and imports
  hipStream_t st = ctx->stream;
  const bool shortrange = pmgrid > 0;
  const bool periodic = g.periodic != 0;
  const bool ewald = periodic && !shortrange;
  const bool unequal = g.unequal_softenings || ctx->adaptive_gravsoft;
  if(ewald)
    GCHK(ensure_pot_table(ctx, g.BoxSize));
  if(shortrange)
    GCHK(ensure_srpot_table(ctx));
  PotK k;
  k.theta = g.ErrTolTheta;
  k.errtol = g.ErrTolForceAcc;
  k.boxsize = g.BoxSize;
  k.boxhalf = 0.5 * g.BoxSize;
  k.rcut = g.Rcut;
  k.asmthfac = shortrange ? 0.5 / g.Asmth * (GHIP_NTAB / 3.0) : 0.0;
  k.fac_intp = periodic ? 2 * GHIP_EN / g.BoxSize : 0.0;
  // OldAcc of every particle in tree order (the relative criterion of potential.c reads P[].OldAcc)
  if(rel)
    GCHK(ghip_gather_f64_lim(ctx, ctx->gt.n, P<int>(ctx->gt.perm), P<double>(ctx->f[GHIP_F_OLDACC]), n,
                             P<double>(ctx->soldacc)));
  const TreeDev &t = (ctx->dyn_use && !shard) ? ctx->dyn.tree : ctx->gt;
#define POT_ARGS                                                                                   \
  P<TreeSizes>(t.dsz), nt, P<WalkHot>(t.mq), P<WalkCold>(t.mq2), P<double>(ctx->sx),               \
    P<double>(ctx->sy), P<double>(ctx->sz), P<double>(ctx->ssoft),                                  \
    rel ? P<double>(ctx->soldacc) : nullptr,                                                        \
    P<int>(ctx->gt.perm), ewald ? P<double>(ctx->potcorr) : nullptr,                                \
    shortrange ? P<float>(ctx->srpot) : nullptr, k, P<double>(ctx->pot),                            \
    P<unsigned long long>(ctx->pot_nint), n, ghip_errword(ctx, GHIP_ERRW_LET)
#define POT_LAUNCH(PER, SR, UNEQ, REL, SH)                                                         \
  k_pot_walk<PER, SR, UNEQ, REL, SH><<<cdiv(nt, 256), 256, 0, st>>>(POT_ARGS)
#define POT_LAUNCH_S(PER, SR, UNEQ, REL)                                                           \
  do                                                                                               \
    {                                                                                              \
      if(shard)                                                                                    \
        POT_LAUNCH(PER, SR, UNEQ, REL, true);                                                      \
      else                                                                                         \
        POT_LAUNCH(PER, SR, UNEQ, REL, false);                                                     \
    }                                                                                              \
  while(0)
#define POT_LAUNCH_R(PER, SR, UNEQ)                                                                \
  do                                                                                               \
    {                                                                                              \
      if(rel)                                                                                      \
        POT_LAUNCH_S(PER, SR, UNEQ, true);                                                         \
      else                                                                                         \
        POT_LAUNCH_S(PER, SR, UNEQ, false);                                                        \
    }                                                                                              \
  while(0)
#define POT_LAUNCH_U(PER, SR)                                                                      \
  do                                                                                               \
    {                                                                                              \
      if(unequal)                                                                                  \
        POT_LAUNCH_R(PER, SR, true);                                                               \
      else                                                                                         \
        POT_LAUNCH_R(PER, SR, false);                                                              \
    }                                                                                              \
  while(0)
  if(periodic)
    {
      if(shortrange)
        POT_LAUNCH_U(true, true);
      else
        POT_LAUNCH_U(true, false);
    }
  else
    {
      if(shortrange)
        POT_LAUNCH_U(false, true);
      else
        POT_LAUNCH_U(false, false);
    }
#undef POT_LAUNCH_U
#undef POT_LAUNCH_R
#undef POT_LAUNCH_S
#undef POT_LAUNCH
#undef POT_ARGS
  HIPCHK(hipGetLastError());
  // potential.c:245-259
  double bgfac = 0;
  if(p->comoving && periodic)
    bgfac = pow(p->Omega0 * 3 * p->Hubble * p->Hubble / (8 * M_PI * p->G), 1.0 / 3);
  const double *S = p->SofteningTable;
  k_pot_finish<<<cdiv(n, 256), 256, 0, st>>>(n, P<double>(ctx->f[GHIP_F_MASS]), P<int>(ctx->f[GHIP_F_TYPE]),
                                             S[0], S[1], S[2], S[3], S[4], S[5], bgfac, p->G,
                                             P<double>(ctx->pot));
  HIPCHK(hipGetLastError());
  return GHIP_OK;
}

// potential.c:301-325
static int pot_quadratic(ghip_ctx *ctx, const ghip_pot_params *p)
{
  const int n = ctx->n;
  double qfac = 0;
  if(p->comoving)
    {
      if(!p->grav.periodic)
        qfac = -0.5 * p->Omega0 * p->Hubble * p->Hubble;
    }
  else
    qfac = -0.5 * p->OmegaLambda * p->Hubble * p->Hubble;
  if(qfac != 0 && n > 0)
    {
      k_pot_quadratic<<<cdiv(n, 256), 256, 0, ctx->stream>>>(n, P<double>(ctx->f[GHIP_F_POS]), qfac,
                                                             P<double>(ctx->pot));
      HIPCHK(hipGetLastError());
    }
  return GHIP_OK;
}

static int pot_ensure_result(ghip_ctx *ctx)
{
  const int n = ctx->n;
  GCHK(ghip_ensure(ctx, ctx->pot, (size_t) (n > 0 ? n : 1) * sizeof(double)));
  GCHK(ghip_ensure(ctx, ctx->pot_nint, (size_t) (n > 0 ? n : 1) * sizeof(unsigned long long)));
  ctx->pot_n = -1;
  return GHIP_OK;
}

extern "C" int ghip_potential(ghip_ctx *ctx, const ghip_pot_params *p)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !p)
    return GHIP_EINVAL;
  if(ctx->dd.on)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_potential: on a multi-GPU shard (ghip_dd_init) run the collective "
                     "GHIP_DD_POTENTIAL through ghip_dd_begin / ghip_dd_run");
  if(ctx->shard_n > 1)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_potential: not on a multi-GPU shard");
  if(!ctx->gt.built)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_potential: call ghip_tree_build first");
  GCHK(pot_check(ctx, p, "ghip_potential"));
  GCHK(ghip_tree_verify(ctx));
  const int n = ctx->n;
  GCHK(pot_ensure_result(ctx));
  if(n == 0)
    {
      ctx->pot_n = 0;
      return GHIP_OK;
    }
  // potential.c:262-270: pmpotential_periodic / pmpotential_nonperiodic(0).  The deposit comes first: the open
  // mesh checks with it that every particle lies inside its region, GHIP_EREGION before any potential is written
  const bool mesh = p->pm.pmgrid > 0;
  if(mesh)
    {
      PmBlock b;
      GCHK(ghip_pm_pot_deposit(ctx, p, &b));
      if(b.outside)
        return ghip_fail(ctx, GHIP_EREGION, "ghip_potential: a particle lies outside the allowed region of the mesh; "
                         "no potential was written.  Find the region again (ghip_pm_find_region) and repeat the call");
    }
  GCHK(pot_walk_and_finish(ctx, p, false));
  if(mesh)
    GCHK(ghip_pm_pot_solve(ctx, p, 1, nullptr, P<double>(ctx->pot)));
  GCHK(pot_quadratic(ctx, p));
  ctx->pot_n = n;
  return GHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// GHIP_DD_POTENTIAL (ghip_dd_begin / ghip_dd_step): compute_potential() on a domain-decomposed shard.
//   GROUPS   the shard's own tree, target groups over ALL its particles (the locally essential tree of the
//            step's GHIP_DD_GRAVITY was selected against the active targets only)  -> all-gather of the groups
//   GUESTS   with ghip_dd_set_guests, when any shard holds a guest: the guests' keys to their hosts
//            (else straight on to LET)                                            -> all-to-all-v of u64 keys
//   LET      selection of the locally essential trees under the opening rules of k_pot_walk, packed
//                                                                                 -> all-to-all-v of LetRec
//   WALK     the merged tree, the walk for the shard's own particles, the finish; what the walk met
//                                                                                 -> all-gather of the status
//   DEPOSIT  every shard fails if one did; no mesh: the r^2 term, done.  Mesh: deposit -> all-gather of meshes
//   SOLVE    the meshes added in rank order, solved, read out at the own particles; the r^2 term
// ---------------------------------------------------------------------------------------------
int ghip_dd_pot_begin(ghip_ctx *ctx, int, const void *params, int)
{
  GHIP_JOIN(ctx);
  ctx->dd.pot = *reinterpret_cast<const ghip_pot_params *>(params);
  return pot_check(ctx, &ctx->dd.pot, "GHIP_DD_POTENTIAL");
}

int ghip_dd_pot_step(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  const ghip_pot_params *p = &D.pot;
  hipStream_t st = ctx->stream;
  const int n = ctx->n;
  const bool mesh = p->pm.pmgrid > 0;
  enum { GROUPS, GUESTS, LET, WALK, DEPOSIT, SOLVE };
  if(D.phase == GROUPS)
    {
      ctx->pot_n = -1;
      GCHK(ghip_dd_own_tree(ctx));
      GCHK(ghip_dd_post_groups(ctx, true, p->grav.ErrTolTheta == 0));
      D.phase = GUESTS;
      return 1;
    }
  if(D.phase == GUESTS)
    {
      const int pending = ghip_dd_post_guests(ctx, "potential");
      D.phase = LET;
      if(pending != 0)
        return pending;
    }
  if(D.phase == LET)
    {
      GCHK(ghip_dd_post_let(ctx, p->grav));
      D.phase = WALK;
      return 1;
    }
  if(D.phase == WALK)
    {
      D.gt_nimp = D.x.rtotal;
      GCHK(ghip_tree_build_impl(ctx));
      D.gt_is_pot = true;
      int rc = pot_ensure_result(ctx);
      if(rc == GHIP_OK && n > 0)
        rc = pot_walk_and_finish(ctx, p, true);
      // did a target have to open a pruned node?  Every shard learns it from every shard's status
      HIPCHK(ghip_stream_sync(ctx, st));
      if(rc == GHIP_OK)
        rc = ghip_check_device_errors(ctx);
      GCHK(dd_post_status(ctx, 0.0, ghip_dd_hold(ctx, rc)));
      D.phase = DEPOSIT;
      return 1;
    }
  if(D.phase == DEPOSIT)
    {
      double worst;
      int failed;
      GCHK(dd_read_status(ctx, &worst, &failed));
      GCHK(ghip_dd_raise(ctx, failed, "potential: the walk failed on shard %d (its own message says "
                         "why); every shard stops here", failed));
      if(mesh)
        {
          // (the open mesh's block carries its status word: a particle outside the region on any shard ends the
          // call on all of them in SOLVE)
          PmBlock b;
          GCHK(ghip_pm_pot_deposit(ctx, p, &b));
          ghip_dd_set_allgather(D, b.p, b.bytes, &D.pm_all);
          D.phase = SOLVE;
          return 1;
        }
      GCHK(pot_quadratic(ctx, p));
      ctx->pot_n = n;
      return 0;
    }
  if(D.phase == SOLVE)
    {
      GCHK(ghip_pm_pot_solve(ctx, p, D.nranks, P<double>(D.pm_all), P<double>(ctx->pot)));
      GCHK(pot_quadratic(ctx, p));
      ctx->pot_n = n;
      return 0;
    }
  return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_step: the potential has no phase %d", D.phase);
}

extern "C" int ghip_get_potential(ghip_ctx *ctx, double *host)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !host)
    return GHIP_EINVAL;
  if(ctx->pot_n != ctx->n)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_get_potential: call ghip_potential first");
  if(ctx->n > 0)
    HIPCHK(hipMemcpyAsync(host, ctx->pot.p, (size_t) ctx->n * sizeof(double), hipMemcpyDeviceToHost,
                          ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  return ghip_check_device_errors(ctx);
}

// interactions per target of the last ghip_potential (sum and maximum)
extern "C" int ghip_potential_interactions(ghip_ctx *ctx, long long *sum, long long *maxval)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || ctx->pot_n != ctx->n)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_potential_interactions: call ghip_potential first");
  std::vector<unsigned long long> v((size_t) ctx->n);
  if(ctx->n > 0)
    HIPCHK(hipMemcpyAsync(v.data(), ctx->pot_nint.p, v.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  long long s = 0, m = 0;
  for(unsigned long long x : v)
    {
      s += (long long) x;
      m = (long long) x > m ? (long long) x : m;
    }
  if(sum)
    *sum = s;
  if(maxval)
    *maxval = m;
  return GHIP_OK;
}

// ... and per target, host order
extern "C" int ghip_get_potential_interactions(ghip_ctx *ctx, long long *host)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !host)
    return GHIP_EINVAL;
  if(ctx->pot_n != ctx->n)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_get_potential_interactions: call ghip_potential first");
  static_assert(sizeof(long long) == sizeof(unsigned long long), "counts are copied as they are");
  if(ctx->n > 0)
    HIPCHK(hipMemcpyAsync(host, ctx->pot_nint.p, (size_t) ctx->n * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ghip_stream_sync(ctx, ctx->stream));
  return GHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// compute_global_quantities_of_system (global.c:18-238): per particle the 14 contributions, per
// block and type fixed-order partial sums, the blocks added on the host in block order.  No atomics:
// two calls on the same state give the same bits.
// ---------------------------------------------------------------------------------------------
#define GQ_NQ 14          // mass, pot, kin, int, mom[3], com[3], angmom[3], rad
#define GQ_PER_THREAD 8
#define GQ_BLOCK 256

struct GqK
{
  int n, ngas;
  int Ti_Current;
  int comoving;
  double a1, a2, a3;
  int pmgrid;
  double dt_gravkick_pm;   // the PM kick factor, the same for every particle
  double rad_fac;          // C / UnitVelocity_in_cm_per_s
  DriftK dk;               // kick tables (comoving)
};

__device__ __forceinline__ void d_gq_particle(int i, const GqK &k, const double *__restrict__ pos,
                                              const double *__restrict__ vel, const double *__restrict__ mass,
                                              const int *__restrict__ type, const int *__restrict__ timebin,
                                              const int *__restrict__ ti_begstep,
                                              const double *__restrict__ gacc, const double *__restrict__ gravpm,
                                              const double *__restrict__ hacc, const double *__restrict__ entropy,
                                              const double *__restrict__ dtentropy,
                                              const double *__restrict__ density,
                                              const double *__restrict__ pot,
                                              const double *__restrict__ photon, double q[GQ_NQ])
{
  const int n = k.n, ng = k.ngas;
  const int t = type[i];
  const double m = mass[i];
  q[13] = (photon && t == 3 && m != 0.) ? photon[i] * k.rad_fac : 0.0;
  q[0] = m;
  q[1] = pot ? 0.5 * m * pot[i] / k.a1 : 0.0;
  const int dt_step = timebin[i] ? (1 << timebin[i]) : 0;
  const int tb = ti_begstep[i];
  double dt_entr, dt_gravkick, dt_hydrokick;
  if(k.comoving)
    {
      dt_entr = (k.Ti_Current - (tb + dt_step / 2)) * k.dk.timebase;
      dt_gravkick = d_table_factor(k.dk.gravkick, tb, k.Ti_Current, k.dk) -
                    d_table_factor(k.dk.gravkick, tb, tb + dt_step / 2, k.dk);
      dt_hydrokick = d_table_factor(k.dk.hydrokick, tb, k.Ti_Current, k.dk) -
                     d_table_factor(k.dk.hydrokick, tb, tb + dt_step / 2, k.dk);
    }
  else
    dt_entr = dt_gravkick = dt_hydrokick = (k.Ti_Current - (tb + dt_step / 2)) * k.dk.timebase;
  const bool gas = t == 0 && i < ng;
  double v[3];
  for(int j = 0; j < 3; j++)
    {
      v[j] = vel[(size_t) j * n + i] + gacc[(size_t) j * n + i] * dt_gravkick;
      if(gas)
        v[j] += hacc[(size_t) j * ng + i] * dt_hydrokick;
    }
  double entr = 0;
  if(gas)
    entr = entropy[i] + dtentropy[i] * dt_entr;
  if(k.pmgrid)
    for(int j = 0; j < 3; j++)
      v[j] += gravpm[(size_t) j * n + i] * k.dt_gravkick_pm;
  q[2] = 0.5 * m * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) / k.a2;
  q[3] = gas ? m * (entr / (GAMMA - 1) * pow(density[i] / k.a3, GAMMA - 1)) : 0.0;
  const double x0 = pos[i], x1 = pos[(size_t) n + i], x2 = pos[2 * (size_t) n + i];
  for(int j = 0; j < 3; j++)
    {
      q[4 + j] = m * v[j];
      q[7 + j] = m * pos[(size_t) j * n + i];
    }
  q[10] = m * (x1 * v[2] - x2 * v[1]);
  q[11] = m * (x2 * v[0] - x0 * v[2]);
  q[12] = m * (x0 * v[1] - x1 * v[0]);
}

// out[block][type][q]
__global__ void __launch_bounds__(GQ_BLOCK)
  k_global_quantities(GqK k, const double *__restrict__ pos, const double *__restrict__ vel,
                      const double *__restrict__ mass, const int *__restrict__ type,
                      const int *__restrict__ timebin, const int *__restrict__ ti_begstep,
                      const double *__restrict__ gacc, const double *__restrict__ gravpm,
                      const double *__restrict__ hacc, const double *__restrict__ entropy,
                      const double *__restrict__ dtentropy, const double *__restrict__ density,
                      const double *__restrict__ pot, const double *__restrict__ photon,
                      double *__restrict__ out)
{
  __shared__ double red[GQ_BLOCK];
  double acc[6][GQ_NQ];
  for(int t = 0; t < 6; t++)
    for(int q = 0; q < GQ_NQ; q++)
      acc[t][q] = 0;
  const int base = blockIdx.x * GQ_BLOCK * GQ_PER_THREAD;
  for(int c = 0; c < GQ_PER_THREAD; c++)
    {
      const int i = base + c * GQ_BLOCK + threadIdx.x;
      if(i < k.n)
        {
          double q[GQ_NQ];
          d_gq_particle(i, k, pos, vel, mass, type, timebin, ti_begstep, gacc, gravpm, hacc, entropy,
                        dtentropy, density, pot, photon, q);
          const int t = type[i];
          for(int tt = 0; tt < 6; tt++)
            if(tt == t)
              for(int qq = 0; qq < GQ_NQ; qq++)
                acc[tt][qq] += q[qq];
        }
    }
  // fixed-order tree reduction of each of the 6 x 14 sums
  for(int t = 0; t < 6; t++)
    for(int q = 0; q < GQ_NQ; q++)
      {
        red[threadIdx.x] = acc[t][q];
        __syncthreads();
        for(int w = GQ_BLOCK / 2; w > 0; w >>= 1)
          {
            if((int) threadIdx.x < w)
              red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
          }
        if(threadIdx.x == 0)
          out[((size_t) blockIdx.x * 6 + t) * GQ_NQ + q] = red[0];
        __syncthreads();
      }
}

// the arguments and the resident fields the sums read
static int gq_check(ghip_ctx *ctx, const ghip_global_params *p, const char *who)
{
  if(p->ComovingIntegrationOn && (!p->GravKickTable || !p->HydroKickTable))
    return ghip_fail(ctx, GHIP_EINVAL, "%s: comoving runs need the kick tables", who);
  if(ctx->n == 0)
    return GHIP_OK;
  for(int f : {GHIP_F_POS, GHIP_F_VEL, GHIP_F_MASS, GHIP_F_TYPE, GHIP_F_TIMEBIN, GHIP_F_TI_BEGSTEP,
               GHIP_F_GRAVACCEL})
    if(!ctx->f[f].p)
      return ghip_fail(ctx, GHIP_EINVAL, "%s: particle field %d not set", who, f);
  if(p->pmgrid && !ctx->f[GHIP_F_GRAVPM].p)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: PMGRID needs GRAVPM", who);
  if(ctx->ngas > 0)
    for(int f : {GHIP_F_HYDROACCEL, GHIP_F_ENTROPY, GHIP_F_DTENTROPY, GHIP_F_DENSITY})
      if(!ctx->f[f].p)
        return ghip_fail(ctx, GHIP_EINVAL, "%s: gas field %d not set", who, f);
  return GHIP_OK;
}

static int gq_local(ghip_ctx *ctx, const ghip_global_params *p, ghip_global_sums *out);

extern "C" int ghip_global_quantities(ghip_ctx *ctx, const ghip_global_params *p, ghip_global_sums *out)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !p || !out)
    return GHIP_EINVAL;
  if(ctx->dd.on)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_global_quantities: on a multi-GPU shard (ghip_dd_init) run the "
                     "collective GHIP_DD_GLOBAL_QUANTITIES through ghip_dd_begin / ghip_dd_run");
  if(ctx->shard_n > 1)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_global_quantities: not on a multi-GPU shard");
  return gq_local(ctx, p, out);
}

// the sums over the particles of this context
static int gq_local(ghip_ctx *ctx, const ghip_global_params *p, ghip_global_sums *out)
{
  if(p->ComovingIntegrationOn && (!p->GravKickTable || !p->HydroKickTable))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_global_quantities: comoving runs need the kick tables");
  memset(out, 0, sizeof(*out));
  const int n = ctx->n, ng = ctx->ngas;
  if(n == 0)
    return GHIP_OK;
  hipStream_t st = ctx->stream;
  GqK k;
  k.n = n;
  k.ngas = ng;
  k.Ti_Current = p->Ti_Current;
  k.comoving = p->ComovingIntegrationOn;
  k.a1 = k.a2 = k.a3 = 1;
  if(k.comoving)
    {
      k.a1 = p->Time;
      k.a2 = p->Time * p->Time;
      k.a3 = p->Time * p->Time * p->Time;
    }
  k.pmgrid = p->pmgrid;
  k.dt_gravkick_pm = p->dt_gravkick_pm;
  k.rad_fac = p->rad_fac;
  k.dk = DriftK();
  k.dk.timebase = p->Timebase_interval;
  k.dk.comoving = k.comoving;
  k.dk.logTimeBegin = p->logTimeBegin;
  k.dk.logTimeMax = p->logTimeMax;
  // upload order: kick tables, photon momenta; then the partial sums come back through the same buffer
  const int nb = cdiv(n, GQ_BLOCK * GQ_PER_THREAD);
  const size_t npart = (size_t) nb * 6 * GQ_NQ;
  const size_t ntab = k.comoving ? 2 * DRIFT_TABLE_LENGTH : 0;
  const size_t nph = p->OldPhotonMomentum ? (size_t) n : 0;
  const size_t npot = p->Potential ? (size_t) n : 0;
  GCHK(ghip_ensure(ctx, ctx->gq_work, (npart + ntab + nph + npot + 1) * sizeof(double)));
  double *w = P<double>(ctx->gq_work);
  double *tabs = w + npart, *ph = w + npart + ntab, *hpot = ph + nph;
  if(k.comoving)
    {
      HIPCHK(hipMemcpyAsync(tabs, p->GravKickTable, DRIFT_TABLE_LENGTH * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(tabs + DRIFT_TABLE_LENGTH, p->HydroKickTable, DRIFT_TABLE_LENGTH * 8,
                            hipMemcpyHostToDevice, st));
      k.dk.gravkick = tabs;
      k.dk.hydrokick = tabs + DRIFT_TABLE_LENGTH;
    }
  if(nph)
    HIPCHK(hipMemcpyAsync(ph, p->OldPhotonMomentum, nph * 8, hipMemcpyHostToDevice, st));
  if(npot)
    HIPCHK(hipMemcpyAsync(hpot, p->Potential, npot * 8, hipMemcpyHostToDevice, st));
  const bool gas = ng > 0;
  for(int f : {GHIP_F_POS, GHIP_F_VEL, GHIP_F_MASS, GHIP_F_TYPE, GHIP_F_TIMEBIN, GHIP_F_TI_BEGSTEP,
               GHIP_F_GRAVACCEL})
    if(!ctx->f[f].p)
      return ghip_fail(ctx, GHIP_EINVAL, "ghip_global_quantities: particle field %d not set", f);
  if(p->pmgrid && !ctx->f[GHIP_F_GRAVPM].p)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_global_quantities: PMGRID needs GRAVPM");
  if(gas)
    for(int f : {GHIP_F_HYDROACCEL, GHIP_F_ENTROPY, GHIP_F_DTENTROPY, GHIP_F_DENSITY})
      if(!ctx->f[f].p)
        return ghip_fail(ctx, GHIP_EINVAL, "ghip_global_quantities: gas field %d not set", f);
  k_global_quantities<<<nb, GQ_BLOCK, 0, st>>>(
    k, P<double>(ctx->f[GHIP_F_POS]), P<double>(ctx->f[GHIP_F_VEL]), P<double>(ctx->f[GHIP_F_MASS]),
    P<int>(ctx->f[GHIP_F_TYPE]), P<int>(ctx->f[GHIP_F_TIMEBIN]), P<int>(ctx->f[GHIP_F_TI_BEGSTEP]),
    P<double>(ctx->f[GHIP_F_GRAVACCEL]), p->pmgrid ? P<double>(ctx->f[GHIP_F_GRAVPM]) : nullptr,
    gas ? P<double>(ctx->f[GHIP_F_HYDROACCEL]) : nullptr, gas ? P<double>(ctx->f[GHIP_F_ENTROPY]) : nullptr,
    gas ? P<double>(ctx->f[GHIP_F_DTENTROPY]) : nullptr, gas ? P<double>(ctx->f[GHIP_F_DENSITY]) : nullptr,
    npot ? hpot : ctx->pot_n == n ? P<double>(ctx->pot) : nullptr, nph ? ph : nullptr, w);
  HIPCHK(hipGetLastError());
  std::vector<double> h(npart);
  HIPCHK(hipMemcpyAsync(h.data(), w, npart * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  GCHK(ghip_check_device_errors(ctx));
  // the blocks in block order
  double s[6][GQ_NQ] = {};
  for(int b = 0; b < nb; b++)
    for(int t = 0; t < 6; t++)
      for(int q = 0; q < GQ_NQ; q++)
        s[t][q] += h[((size_t) b * 6 + t) * GQ_NQ + q];
  for(int t = 0; t < 6; t++)
    {
      out->MassComp[t] = s[t][0];
      out->EnergyPotComp[t] = s[t][1];
      out->EnergyKinComp[t] = s[t][2];
      out->EnergyIntComp[t] = s[t][3];
      for(int j = 0; j < 3; j++)
        {
          out->MomentumComp[t][j] = s[t][4 + j];
          out->CenterOfMassComp[t][j] = s[t][7 + j];
          out->AngMomentumComp[t][j] = s[t][10 + j];
        }
      out->EnergyRadComp += s[t][13];
    }
  return GHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// GHIP_DD_GLOBAL_QUANTITIES: phase 0 sums the shard's own particles (k_global_quantities, blocks in block
// order) and posts the all-gather of its ghip_global_sums; phase 1 adds the shards' sums in rank order --
// the same additions on every shard, so `out` holds the same bytes everywhere.  (The reference reduces to
// rank 0 and broadcasts, global.c:146-237.)
// ---------------------------------------------------------------------------------------------
#define GQ_SUM_DOUBLES (sizeof(ghip_global_sums) / sizeof(double))
static_assert(sizeof(ghip_global_sums) % sizeof(double) == 0, "ghip_global_sums is an array of doubles");

// Begun with walk = GHIP_FOF_FORM the operation is the group finder of all shards (ghip_fof.hip), whose catalogue
// has this operation's contract: the same bytes on all shards, sums added in rank order, no atomics.
int ghip_dd_gq_begin(ghip_ctx *ctx, int op, const void *params, int walk)
{
  ctx->dd.gq_form = walk == GHIP_FOF_FORM ? GHIP_FOF_FORM : 0;
  if(ctx->dd.gq_form == GHIP_FOF_FORM)
    return ghip_dd_fof_begin(ctx, op, params, walk);
  GHIP_JOIN(ctx);
  DDState &D = ctx->dd;
  D.gq = *reinterpret_cast<const ghip_dd_global_args *>(params);
  if(!D.gq.p || !D.gq.out)
    return ghip_fail(ctx, GHIP_EINVAL, "GHIP_DD_GLOBAL_QUANTITIES: params needs p and out");
  D.gq_p = *D.gq.p;
  return gq_check(ctx, &D.gq_p, "GHIP_DD_GLOBAL_QUANTITIES");
}

int ghip_dd_gq_step(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  if(D.gq_form == GHIP_FOF_FORM)
    return ghip_dd_fof_step(ctx);
  hipStream_t st = ctx->stream;
  enum { OWN_SUMS, ADD };
  if(D.phase == OWN_SUMS)
    {
      ghip_global_sums mine;
      GCHK(gq_local(ctx, &D.gq_p, &mine));
      GCHK(ghip_ensure(ctx, D.gq_send, sizeof(mine)));
      HIPCHK(hipMemcpyAsync(D.gq_send.p, &mine, sizeof(mine), hipMemcpyHostToDevice, st));
      HIPCHK(ghip_stream_sync(ctx, st));   // (`mine` lives on this frame)
      ghip_dd_set_allgather(D, D.gq_send.p, sizeof(mine), &D.gq_all);
      D.phase = ADD;
      return 1;
    }
  if(D.phase == ADD)
    {
      std::vector<double> all((size_t) D.nranks * GQ_SUM_DOUBLES);
      HIPCHK(hipMemcpyAsync(all.data(), D.gq_all.p, all.size() * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      double s[GQ_SUM_DOUBLES];
      for(size_t q = 0; q < GQ_SUM_DOUBLES; q++)
        s[q] = 0;
      for(int r = 0; r < D.nranks; r++)   // in rank order
        for(size_t q = 0; q < GQ_SUM_DOUBLES; q++)
          s[q] += all[(size_t) r * GQ_SUM_DOUBLES + q];
      memcpy(D.gq.out, s, sizeof(ghip_global_sums));
      return 0;
    }
  return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_step: the global quantities have no phase %d", D.phase);
}
