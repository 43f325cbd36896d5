// ghip_sfr.hip -- cooling_and_starformation with the cooling function and the dust drag heating, for
// the reference's shipped flag bundle (COOLING, SFR, DUST, BH_FORM, FIND_SMBH, EVAPORATION_RADIAL,
// CONSTANT_MEAN_MOLECULAR_WEIGHT, BLACK_HOLES + BH_THERMALFEEDBACK) and the sibling closed forms of
// DoCooling (ISOTHERM, EVAPORATION, BETA_COOLING [+ BETA_COOLING_TAPPER_OFF]).
//
// Replaces the particle loops of
//   cooling_and_starformation, the deterministic part   sfr_eff.c:183-597
//   DoCooling, the closed forms                         cooling.c:82-300
//   FindQuasars, the SMBH position                      blackhole.c:1481-1530
//
// One lane per active particle, fp64, streaming the resident fields once: nothing is shared between
// particles, so the pass is bound by HBM bandwidth (about 100 bytes per gas particle).  The sink
// candidates are compacted in active-list order without atomics: the pass leaves one 64-bit ballot
// mask and its population count per wavefront, an exclusive scan of the counts gives every wavefront
// its first slot, and a scatter writes each candidate at its slot plus the number of candidates below
// it in the mask.  The host reads two ints and the ncand candidates, never an [ngas] array.  The list itself
// stays on the device (ctx->sfr_cand) for ghip_sfr_form_sinks, which converts exactly those particles.
#include "ghip_ngb.h"   // the reference's constants
#include "ghip_prim.h"

#define SFR_TAPPER_RHO 1.e-10      // rho_crit of BETA_COOLING_TAPPER_OFF, cooling.c:219

struct SfrK
{
  int cooling, tapper, comoving, pad;
  double timebase, a3inv, time, time_hubble_a;
  double critdens, minegy, grain_floor, u_to_temp;
  double eqtemp, betacool, cool_ind, rho_cool_ind, evap_dens, udens;
  double xbh, ybh, zbh;
};

// DoCooling(u_old, rho, dt, &ne, r2) for the closed forms (cooling.c:82-300): rho is the proper
// density, dt the comoving-corrected step dtime
__device__ __forceinline__ double sfr_do_cooling(const SfrK &K, double u_old, double rho, double dt,
                                                 double r2)
{
  switch(K.cooling)
    {
      case GHIP_COOL_ISOTHERM:   // :170-173
        return K.eqtemp / K.u_to_temp;
      case GHIP_COOL_EVAPORATION:   // :175-183
        {
          const double u_eq = K.eqtemp / K.u_to_temp;
          double tcool = K.betacool;
          tcool *= (1. + pow(rho * K.udens / K.evap_dens, 5.));
          return (u_old + u_eq * dt / tcool) / (1. + dt / tcool);
        }
      case GHIP_COOL_EVAPORATION_RADIAL:   // :185-192
        {
          const double u_eq = K.eqtemp / K.u_to_temp / (pow(sqrt(r2), K.cool_ind) + 1e-10);
          double tcool = K.betacool;
          tcool *= (1. + pow(rho * K.udens / K.evap_dens, K.rho_cool_ind));
          return (u_old + u_eq * dt / tcool) / (1. + dt / tcool);
        }
      case GHIP_COOL_BETA:   // :196-198, 218-222, 282
        {
          const double r = sqrt(r2);
          const double u_eq = K.eqtemp / K.u_to_temp / (pow(r, 0.5) + 1.e-10);
          double tcool = K.betacool * pow(r, 1.5);
          if(K.tapper)
            tcool *= (1. + pow(rho * K.udens / SFR_TAPPER_RHO, 2.));
          return (u_old + u_eq * dt / tcool) / (1. + dt / tcool);
        }
      default:
        return u_old;
    }
}

// One lane per active-list position a.  Every lane reaches the two ballots at the end (no early
// return), so that each wavefront of the grid writes its mask and count.
__global__ __launch_bounds__(256) void k_sfr_cooling(
  int nact, const int *__restrict__ act, int n, int ngas, const double *__restrict__ pos,
  double *__restrict__ mass, const int *__restrict__ type, const int *__restrict__ timebin,
  const double *__restrict__ density, const double *__restrict__ entropy, double *__restrict__ dtentropy,
  double *__restrict__ injected, double *__restrict__ dragheat, SfrK K,
  unsigned long long *__restrict__ candmask, int *__restrict__ candcnt, int *__restrict__ nfloor)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  bool cand = false, floored = false;
  if(a < nact)
    {
      const int i = act ? act[a] : a;
      if(i >= 0 && i < n)
        {
          const int ty = type[i];
          if(ty == 2)
            {
              // remove dust particles of very small mass (:185-187)
              const double m = mass[i];
              if(m <= K.grain_floor && m != 0)
                {
                  mass[i] = 0.;
                  floored = true;
                }
            }
          else if(ty == 0 && i < ngas)
            {
              const int tb = timebin[i];
              const double dt = (tb ? (double) (1 << tb) : 0.0) * K.timebase;
              const double dtime = K.comoving ? K.time * dt / K.time_hubble_a : dt;
              const double m = mass[i];
              const double rho = density[i];
              int flag = 1;   // sink candidate (:226-229, 459-462)
              if(rho >= K.critdens)
                flag = 0;
              if(m == 0)
                flag = 1;
              cand = !flag;
              if(flag == 1)
                {
                  const double A = entropy[i];
                  const double prho = rho * K.a3inv;
                  const double pw = pow(prho, GAMMA_MINUS1);   // the reference evaluates it twice
                  double unew = (A + dtentropy[i] * dt) / GAMMA_MINUS1 * pw;   // :486-488
                  if(unew < K.minegy)
                    unew = K.minegy;
                  if(dragheat)   // :481-499: neither spent nor cleared when Mass == 0
                    {
                      const double dh = dragheat[i];
                      if(dh && m != 0)
                        {
                          unew += dh / m * dt;
                          dragheat[i] = 0.;
                        }
                    }
                  const double inj = injected[i];   // :502-524
                  if(inj)
                    {
                      if(m != 0)
                        unew += inj / m;
                      if(K.u_to_temp * unew > 5.0e9)
                        unew = 5.0e9 / K.u_to_temp;
                      injected[i] = 0.;
                    }
                  double r2 = 0;   // to the SMBH, not wrapped (:215-224)
                  if(K.cooling >= GHIP_COOL_EVAPORATION_RADIAL)
                    {
                      const double dx = pos[i] - K.xbh;   // POS is SoA with pitch n on the device
                      const double dy = pos[(size_t) n + i] - K.ybh;
                      const double dz = pos[2 * (size_t) n + i] - K.zbh;
                      r2 = dx * dx + dy * dy + dz * dz;
                    }
                  unew = sfr_do_cooling(K, unew, prho, dtime, r2);
                  if(tb && dt > 0)   // :572-595
                    {
                      double d = (unew * GAMMA_MINUS1 / pw - A) / dt;
                      if(d < -0.5 * A / dt)
                        d = -0.5 * A / dt;
                      dtentropy[i] = d;
                    }
                }
            }
        }
    }
  const unsigned long long cm = __ballot(cand);
  const unsigned long long fm = __ballot(floored);
  if((threadIdx.x & (GHIP_WAVE - 1)) == 0)
    {
      const int w = a / GHIP_WAVE;
      candmask[w] = cm;
      candcnt[w] = __popcll(cm);
      if(fm)
        atomicAdd(nfloor, __popcll(fm));   // a count: the grains whose mass became 0
    }
}

// cand_idx[off[w] + (candidates below this lane in the wavefront's mask)] = the particle index
__global__ __launch_bounds__(256) void k_sfr_scatter(int nact, const int *__restrict__ act,
                                                     const unsigned long long *__restrict__ candmask,
                                                     const int *__restrict__ off, int *__restrict__ cand_idx)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nact)
    return;
  const unsigned long long m = candmask[a / GHIP_WAVE];
  const int lane = a & (GHIP_WAVE - 1);
  if((m >> lane) & 1ull)
    cand_idx[off[a / GHIP_WAVE] + __popcll(m & ((1ull << lane) - 1ull))] = act ? act[a] : a;
}

extern "C" int ghip_sfr_cooling(ghip_ctx *ctx, const ghip_sfr_params *p, int *ncand, int *cand_idx)
{
  if(!ctx)
    return GHIP_EINVAL;
  if(!p || !ncand)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_sfr_cooling: bad arguments");
  if(p->cooling < GHIP_COOL_NONE || p->cooling > GHIP_COOL_BETA)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_sfr_cooling: unknown cooling variant %d", p->cooling);
  // (a multi-GPU shard holds DragHeating once GHIP_DD_DUST_DRAG or ghip_dust_set_drag_heating created it)
  if(p->dust && ctx->dd.on && ctx->dd.nranks > 1 && !ctx->dust_heat.p)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_sfr_cooling: dust = 1 on a multi-GPU context (%d ranks) that "
                     "holds no DragHeating: it exists on single-rank contexts, and on shards after "
                     "GHIP_DD_DUST_DRAG or ghip_dust_set_drag_heating", ctx->dd.nranks);
  if(p->dust && ctx->shard_n > 1)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_sfr_cooling: dust = 1 on a sharded context (%d shards): "
                     "DragHeating exists on single-rank contexts only", ctx->shard_n);
  if(p->comoving && !(p->Time > 0 && p->hubble_a > 0))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_sfr_cooling: comoving needs Time > 0 and hubble_a > 0");
  GHIP_JOIN(ctx);
  *ncand = 0;
  ctx->sfr_ncand = -1;
  GCHK(ghip_sink_buffers(ctx));
  double *dragheat = nullptr;
  if(p->dust && ctx->dust_heat.p)   // never set: zero everywhere, and it stays unallocated
    {
      if(ctx->dust_heat.cap < (size_t) ctx->ngas * 8)
        return ghip_fail(ctx, GHIP_EINVAL, "ghip_sfr_cooling: the resident DragHeating holds fewer than "
                         "ngas = %d values (set it again after ghip_set_counts)", ctx->ngas);
      dragheat = P<double>(ctx->dust_heat);
    }
  const int nact = ctx->nactive < 0 ? ctx->n : ctx->nactive;
  if(nact <= 0)
    {
      ctx->sfr_ncand = 0;
      return GHIP_OK;
    }
  SfrK K;
  K.cooling = p->cooling;
  K.tapper = p->beta_tapper_off;
  K.comoving = p->comoving;
  K.pad = 0;
  K.timebase = p->Timebase_interval;
  if(p->comoving)   // sfr_eff.c:145-156
    {
      K.a3inv = 1 / (p->Time * p->Time * p->Time);
      K.time = p->Time;
      K.time_hubble_a = p->Time * p->hubble_a;
    }
  else
    K.a3inv = K.time = K.time_hubble_a = 1;
  K.critdens = p->CritPhysDensity_code;
  K.minegy = p->MinEgySpec;
  K.grain_floor = 1.e-5 * p->OriginalGasMass;
  // cooling.c:104-105 and sfr_eff.c:127 (CONSTANT_MEAN_MOLECULAR_WEIGHT): the same factor
  K.u_to_temp = p->MeanWeight * PROTONMASS / BOLTZMANN * GAMMA_MINUS1 * p->UnitEnergy_in_cgs /
                p->UnitMass_in_g;
  K.eqtemp = p->EqTemp;
  K.betacool = p->BetaCool;
  K.cool_ind = p->Cool_ind;
  K.rho_cool_ind = p->rho_cool_ind;
  K.evap_dens = p->Evap_dens;
  K.udens = p->UnitDensity_in_cgs;
  K.xbh = p->smbh_pos[0];
  K.ybh = p->smbh_pos[1];
  K.zbh = p->smbh_pos[2];

  hipStream_t st = ctx->stream;
  const int nb = cdiv(nact, 256);
  const size_t nw = (size_t) nb * (256 / GHIP_WAVE);
  // sfr_work: mask u64[nw] | cnt i32[nw + 1] | off i32[nw + 1] | nfloor i32
  GCHK(ghip_ensure(ctx, ctx->sfr_work, nw * 8 + (2 * nw + 3) * 4 + 64));
  unsigned long long *dmask = P<unsigned long long>(ctx->sfr_work);
  int *dcnt = reinterpret_cast<int *>(dmask + nw), *doff = dcnt + nw + 1, *dnfloor = doff + nw + 1;
  // the candidates stay on the device for ghip_sfr_form_sinks (ghip_accretion.hip)
  ctx->sfr_ncand = -1;
  GCHK(ghip_ensure(ctx, ctx->sfr_cand, (size_t) nact * 4));
  int *dcand = P<int>(ctx->sfr_cand);
  HIPCHK(hipMemsetAsync(dcnt + nw, 0, 4, st));
  HIPCHK(hipMemsetAsync(dnfloor, 0, 4, st));
  const int *dact = ctx->nactive < 0 ? nullptr : P<int>(ctx->act_host_idx);
  k_sfr_cooling<<<nb, 256, 0, st>>>(nact, dact, ctx->n, ctx->ngas, P<double>(ctx->f[GHIP_F_POS]),
                                    P<double>(ctx->f[GHIP_F_MASS]), P<int>(ctx->f[GHIP_F_TYPE]),
                                    P<int>(ctx->f[GHIP_F_TIMEBIN]), P<double>(ctx->f[GHIP_F_DENSITY]),
                                    P<double>(ctx->f[GHIP_F_ENTROPY]), P<double>(ctx->f[GHIP_F_DTENTROPY]),
                                    P<double>(ctx->bh_injected), dragheat, K, dmask, dcnt, dnfloor);
  HIPCHK(hipGetLastError());
  GCHK(ghip_scan(ctx, dcnt, doff, (int) nw + 1, st));
  k_sfr_scatter<<<nb, 256, 0, st>>>(nact, dact, dmask, doff, dcand);
  HIPCHK(hipGetLastError());
  int tot[2] = {0, 0};   // candidates, floored grains
  HIPCHK(hipMemcpyAsync(tot, doff + nw, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  if(tot[0] < 0 || tot[0] > nact)
    return ghip_fail(ctx, GHIP_EDEVICE, "ghip_sfr_cooling: %d candidates of %d active", tot[0], nact);
  *ncand = tot[0];
  ctx->sfr_ncand = tot[0];
  if(cand_idx && tot[0] > 0)
    {
      HIPCHK(hipMemcpyAsync(cand_idx, dcand, (size_t) tot[0] * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
    }
  if(tot[1] > 0)
    ctx->gt.built = false;   // grain masses changed: the gravity tree's moments are stale
  return GHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// FindQuasars (blackhole.c:1481-1530), the position part: the last active Type-5 particle with
// Mass > 0.9 SMBHmass in active-list order, and how many there are
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_find_smbh(int nact, const int *__restrict__ act, int n,
                                                   const int *__restrict__ type,
                                                   const double *__restrict__ mass, double thresh,
                                                   int *__restrict__ res)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nact)
    return;
  const int i = act ? act[a] : a;
  if(i < 0 || i >= n)
    return;
  if(type[i] == 5 && mass[i] > thresh)
    {
      atomicAdd(&res[0], 1);
      atomicMax(&res[1], a + 1);   // 1 + the last list position
    }
}

__global__ void k_smbh_pos(int n, const int *__restrict__ act, const double *__restrict__ pos,
                           int *__restrict__ res)
{
  if(blockIdx.x != 0 || threadIdx.x != 0)
    return;
  double *out = reinterpret_cast<double *>(res + 2);
  const int l = res[1];
  if(l > 0)
    {
      const size_t i = (size_t) (act ? act[l - 1] : l - 1);
      out[0] = pos[i];   // SoA with pitch n
      out[1] = pos[(size_t) n + i];
      out[2] = pos[2 * (size_t) n + i];
    }
  else
    out[0] = out[1] = out[2] = 0.0;
}

extern "C" int ghip_find_smbh(ghip_ctx *ctx, double SMBHmass, double pos[3], int *count)
{
  if(!ctx)
    return GHIP_EINVAL;
  if(!pos || !count)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_find_smbh: bad arguments");
  GHIP_JOIN(ctx);
  pos[0] = pos[1] = pos[2] = 0.0;
  *count = 0;
  const int nact = ctx->nactive < 0 ? ctx->n : ctx->nactive;
  if(nact <= 0)
    return GHIP_OK;
  hipStream_t st = ctx->stream;
  // res: count i32 | 1 + last position i32 | pos f64[3]
  GCHK(ghip_ensure(ctx, ctx->sfr_work, 64));
  int *dres = P<int>(ctx->sfr_work);
  const int *dact = ctx->nactive < 0 ? nullptr : P<int>(ctx->act_host_idx);
  HIPCHK(hipMemsetAsync(dres, 0, 8, st));
  k_find_smbh<<<cdiv(nact, 256), 256, 0, st>>>(nact, dact, ctx->n, P<int>(ctx->f[GHIP_F_TYPE]),
                                                P<double>(ctx->f[GHIP_F_MASS]), 0.9 * SMBHmass, dres);
  k_smbh_pos<<<1, 64, 0, st>>>(ctx->n, dact, P<double>(ctx->f[GHIP_F_POS]), dres);
  HIPCHK(hipGetLastError());
  struct
  {
    int count, last;
    double pos[3];
  } r;
  HIPCHK(hipMemcpyAsync(&r, dres, sizeof(r), hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  *count = r.count;
  pos[0] = r.pos[0];
  pos[1] = r.pos[1];
  pos[2] = r.pos[2];
  return GHIP_OK;
}
