// ghip_accretion.hip -- the sinks on the resident state: the sink table, blackhole_accretion() as a whole and the
// BH_FORM conversion, for the shipped flags BLACK_HOLES, BH_FORM, SWALLOWGAS, ACCRETION_RADIUS, BH_MASS_REAL,
// LIMITED_ACCRETION_AND_FEEDBACK (and their siblings ACCRETION_AT_EDDINGTON_RATE, ENFORCE_EDDINGTON_LIMIT).
//
// Replaces, for a host with a resident run,
//   blackhole_accretion()                         blackhole.c:70-791 without the log files
//     the Mdot loop                               :119-286   -> k_acc_begin
//     blackhole_evaluate / _evaluate_swallow      the kernels of ghip_sink.hip, unchanged (ghip_bh_launch_*)
//     the finish and the per-bin sums             :679-735   -> k_acc_finish, k_acc_report
//   the BH_FORM branch of cooling_and_starformation   sfr_eff.c:602-629   -> k_form_rows, k_form_apply
//   density() for Type-5 targets                  ghip_sink_density's kernel and h iteration (ghip_sinks_density)
//   momentum_feedback(), the sinks' emission      momentum_feedback.c:70-246   -> ghip_wind_spawn, the end of this file
//
// The per-sink state lives in a keyed row table (ghip_rowtable.h) of GHIP_SK_COUNT doubles per
// Type-5 particle, keyed by P[].ID: a pass selects the active Type-5 particles on the device, in active-list order,
// and finds each one's row by d_rt_find.  Nothing here is keyed by particle index, so no reordering of the particles
// moves the table.  Sorting, compaction, growth and the table's refusals are the row table's; this file says which
// rows (k_sk_mark_dead, k_sk_flag_sinks, k_sk_rows, the k_skm_* kernels) and what is in them.
// Sinks are few (hundreds): everything below but the two neighbour passes is one thread per sink, and the sums
// that have an order (the report) are added by a single thread in active-list order.
//
// On a multi-GPU shard the table holds the rows of the shard's own Type-5 particles: GHIP_DD_MIGRATE carries a row
// with its particle, and the two passes are collectives (GHIP_DD_SINK_DENSITY / GHIP_DD_BH_SWALLOW begun with
// walk = GHIP_SINKS_RESIDENT_FORM) -- the second half of this file.
//
// ghip_blackhole_accretion waits for the device once, for its report.  The number of active sinks is not known
// on the host before that: the passes are launched for as many records as the table has rows, and a record
// beyond the active sinks is inert (mass 0: marks nothing; its own mark set: sweeps nothing).
//
// no a*b+c -> fma contraction in this file (before the headers, as in ghip_wind.hip): every result equals the
// op-by-op IEEE evaluation of the C text, which the tests restate in numpy.
#pragma clang fp contract(off)

#include "ghip_rowtable.h"

#define SK_NC GHIP_SK_COUNT

struct AccK
{
  int limited, at_edd, enforce, mass_real, dust;
  double medd_fac, tvisc, eddf, dt_fac;
};

// what every entry point of the section refuses
static int sk_enter(ghip_ctx *ctx, const char *who, bool need_table)
{
  if(ctx->shard_n > 1)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: not available on a replicated shard (ghip_set_shard with %d ranks)",
                     who, ctx->shard_n);
  HIPCHK(hipSetDevice(ctx->device));
  if(!ctx->id_given)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: the sink table is keyed by P[].ID, and GHIP_F_ID has not been given "
                     "since ghip_set_counts (ghip_set_field)", who);
  return need_table ? ghip_rt_need(ctx, ctx->sk, who, true) : GHIP_OK;
}

// the two passes that one GPU runs alone are collectives on a multi-GPU shard, where the table holds the rows of
// the shard's own Type-5 particles
static int sk_one_gpu(ghip_ctx *ctx, const char *who, const char *op)
{
  if(ctx->dd.on && ctx->dd.nranks > 1)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: on a multi-GPU shard (%d ranks) use %s with walk = "
                     "GHIP_SINKS_RESIDENT_FORM (ghip_dd_sinks_args)", who, ctx->dd.nranks, op);
  return GHIP_OK;
}

extern "C" int ghip_sinks_set_table(ghip_ctx *ctx, int nsink, const unsigned int *id, const double *rows)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || nsink < 0 || (nsink > 0 && (!id || !rows)))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_sinks_set_table: bad arguments");
  GCHK(sk_enter(ctx, "ghip_sinks_set_table", false));
  int hw[RTW_WORDS];
  GCHK(ghip_rt_stage_host(ctx, ctx->sk, nsink, id, rows));
  return ghip_rt_install(ctx, ctx->sk, nsink, "ghip_sinks_set_table", false, hw);
}

extern "C" int ghip_sinks_get_table(ghip_ctx *ctx, int *nsink, unsigned int *id, double *rows)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !nsink)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_sinks_get_table: bad arguments");
  GCHK(sk_enter(ctx, "ghip_sinks_get_table", true));
  return ghip_rt_get(ctx, ctx->sk, nsink, id, rows);
}

extern "C" int ghip_sinks_clear(ghip_ctx *ctx)
{
  if(!ctx)
    return GHIP_EINVAL;
  GHIP_JOIN(ctx);
  return ghip_rt_clear(ctx, ctx->sk);
}

// keep[row] = 0 for the row of every Type-5 particle that the map eliminates
__global__ void k_sk_mark_dead(int n, const int *__restrict__ type, const int *__restrict__ idf,
                               const int *__restrict__ new_of_old, int nrows, const unsigned int *__restrict__ ids,
                               int *__restrict__ keep)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if(i < n && type[i] == 5 && new_of_old[i] < 0)
    {
      const int r = d_rt_find(nrows, ids, (unsigned int) idf[i]);
      if(r >= 0)
        keep[r] = 0;
    }
}

int ghip_sinks_drop_eliminated(ghip_ctx *ctx, int n_before, const int *new_of_old)
{
  RowTable &T = ctx->sk;
  if(!T.on || T.n == 0 || n_before <= 0 || !ctx->id_given)
    return GHIP_OK;
  hipStream_t st = ctx->stream;
  const int m = T.n;
  RtWork W;
  GCHK(ghip_rt_work(ctx, T, (size_t) m, 0, W, true));
  HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(W.a), 1, (size_t) m, st));
  k_sk_mark_dead<<<cdiv(n_before, 256), 256, 0, st>>>(n_before, P<int>(ctx->f[GHIP_F_TYPE]), P<int>(ctx->f[GHIP_F_ID]),
                                                     new_of_old, m, P<unsigned int>(T.key), W.a);
  HIPCHK(hipGetLastError());
  int kept = 0;   // (in place: the selection keeps the order, nothing is sorted)
  return ghip_rt_compact(ctx, T, "ghip_rearrange", W, W.a, nullptr, 0, &kept);
}

// ---------------------------------------------------------------------------------------------
// the active Type-5 particles, in active-list order, and their rows
// ---------------------------------------------------------------------------------------------
__global__ void k_sk_flag_sinks(int nact, const int *__restrict__ act, int n, const int *__restrict__ type,
                                int *__restrict__ flags)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nact)
    return;
  const int i = act ? act[a] : a;
  flags[a] = (i >= 0 && i < n && type[i] == 5) ? 1 : 0;
}

// row[a] of the a-th selected particle, a < min(count, G); whoever has none is an error.  (More selected particles
// than rows: one of them has none, or two carry the same ID -- SK_BAD covers both.)
#define SK_BAD(words, G) ((words)[RTW_ERR] != 0 || (words)[RTW_COUNT] > (G))
__global__ void k_sk_rows(int nact, const int *__restrict__ sel, const int *__restrict__ idf, int nrows,
                          const unsigned int *__restrict__ ids, int G, int *__restrict__ row, int *__restrict__ words)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nact || a >= words[RTW_COUNT])
    return;
  const unsigned int id = (unsigned int) idf[sel[a]];
  const int r = d_rt_find(nrows, ids, id);
  if(r < 0)
    {
      words[RTW_ERR] = 1;
      atomicMax(reinterpret_cast<unsigned int *>(words + RTW_ERRKEY), id);
    }
  else if(a < G)
    row[a] = r;
}

// selection + rows, everything left on the device: W.b = the particles, W.row = their rows, W.words
static int sk_select(ghip_ctx *ctx, int G, RtWork &W, int *nact_out)
{
  RowTable &T = ctx->sk;
  hipStream_t st = ctx->stream;
  const int nact = ctx->nactive < 0 ? ctx->n : ctx->nactive;
  *nact_out = nact;
  GCHK(ghip_rt_work(ctx, T, (size_t) (nact > 0 ? nact : 1), (size_t) (G > 0 ? G : 1), W, true));
  if(nact <= 0)
    return GHIP_OK;
  const int *dact = ctx->nactive < 0 ? nullptr : P<int>(ctx->act_host_idx);
  k_sk_flag_sinks<<<cdiv(nact, 256), 256, 0, st>>>(nact, dact, ctx->n, P<int>(ctx->f[GHIP_F_TYPE]), W.a);
  HIPCHK(hipGetLastError());
  GCHK(ghip_select_flagged(ctx, dact, W.a, W.b, W.words + RTW_COUNT, nact, st));
  k_sk_rows<<<cdiv(nact, 256), 256, 0, st>>>(nact, W.b, P<int>(ctx->f[GHIP_F_ID]), T.n, P<unsigned int>(T.key), G,
                                             W.row, W.words);
  HIPCHK(hipGetLastError());
  return GHIP_OK;
}

// The G sink records of a pass.  Record a < min(count, G) is the a-th active sink: its state from the fields and
// its row, after the Mdot step (blackhole.c:119-286) when do_mdot.  Every other record -- and every record once a
// row is missing -- is inert: mass 0 (marks nothing), its own mark set (sweeps nothing).
__global__ void k_acc_begin(int G, const int *__restrict__ words, const int *__restrict__ sel,
                            const int *__restrict__ row, int n, const double *__restrict__ pos,
                            const double *__restrict__ vel, const double *__restrict__ mass,
                            const double *__restrict__ hsml, const int *__restrict__ timebin,
                            const int *__restrict__ idf, double *__restrict__ rows, AccK K, int do_mdot,
                            SinkRec *__restrict__ recs, double *__restrict__ dh)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= G)
    return;
  const int cnt = words[RTW_COUNT] < G ? words[RTW_COUNT] : G;
  SinkRec S;
  if(a >= cnt || SK_BAD(words, G))
    {
      S.x = S.y = S.z = S.vx = S.vy = S.vz = S.mass = S.h = S.mdot = 0;
      S.rho = 1.0;
      S.id = 0;
      S.timebin = 0;
      S.index = 0;
      S.mark = 1;
      recs[a] = S;
      if(dh)
        dh[a] = 0;
      return;
    }
  const int i = sel[a];
  double *R = rows + (size_t) row[a] * SK_NC;
  const int tb = timebin[i];
  const double m = mass[i];
  if(do_mdot)
    {
      const double dt = (tb ? (double) (1 << tb) : 0.0) * K.dt_fac;
      const double meddington = K.medd_fac * (K.mass_real ? m : R[GHIP_SK_BH_MASS]);
      double mdot = 0;
      if(K.limited)
        {
          if(!K.at_edd)
            {
              mdot = R[GHIP_SK_ACCDISC_MASS] / (dt + K.tvisc);
              if(K.enforce && mdot > K.eddf * meddington)
                mdot = K.eddf * meddington;
              R[GHIP_SK_ACCDISC_MASS] -= mdot * dt;
              R[GHIP_SK_BH_MASS] += mdot * dt;
            }
          else
            {
              mdot = K.eddf * meddington;
              R[GHIP_SK_BH_MASS] += mdot * dt;
            }
        }
      else if(K.enforce && mdot > K.eddf * meddington)
        mdot = K.eddf * meddington;
      R[GHIP_SK_BH_MDOT] = mdot;
    }
  S.x = pos[i];
  S.y = pos[(size_t) n + i];
  S.z = pos[2 * (size_t) n + i];
  S.vx = vel[i];
  S.vy = vel[(size_t) n + i];
  S.vz = vel[2 * (size_t) n + i];
  S.mass = m;
  S.h = hsml[i];
  S.mdot = R[GHIP_SK_BH_MDOT];
  S.rho = R[GHIP_SK_BH_DENSITY];
  S.id = (unsigned int) idf[i];
  S.timebin = tb;
  S.index = i;
  S.mark = 0;
  recs[a] = S;
  if(dh)
    dh[a] = S.h;
}

// ---------------------------------------------------------------------------------------------
// density() for the active sinks
// ---------------------------------------------------------------------------------------------
// res: h | numngb | rho | entropy [ns] | gasvel [ns][3]
__global__ void k_sk_store_density(int ns, const int *__restrict__ sel, const int *__restrict__ row,
                                   const double *__restrict__ res, double *__restrict__ hsml,
                                   double *__restrict__ rows)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= ns)
    return;
  double *R = rows + (size_t) row[a] * SK_NC;
  hsml[sel[a]] = res[a];
  R[GHIP_SK_NUMNGB] = res[(size_t) ns + a];
  R[GHIP_SK_BH_DENSITY] = res[2 * (size_t) ns + a];
  R[GHIP_SK_BH_ENTROPY] = res[3 * (size_t) ns + a];
  for(int k = 0; k < 3; k++)
    R[GHIP_SK_GASVEL + k] = res[4 * (size_t) ns + 3 * (size_t) a + k];
}

extern "C" int ghip_sinks_density(ghip_ctx *ctx, const ghip_dens_params *p, double ngb_factor, int *iterations)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !p)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_sinks_density: bad arguments");
  if(iterations)
    *iterations = 0;
  GCHK(sk_one_gpu(ctx, "ghip_sinks_density", "GHIP_DD_SINK_DENSITY"));
  GCHK(sk_enter(ctx, "ghip_sinks_density", true));
  GCHK(ghip_finish_gas_tree(ctx));
  if(!ctx->st.built)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_sinks_density: call ghip_tree_build first");
  RowTable &T = ctx->sk;
  hipStream_t st = ctx->stream;
  RtWork W;
  int nact = 0;
  GCHK(sk_select(ctx, T.n, W, &nact));
  int w[RTW_WORDS];
  HIPCHK(hipMemcpyAsync(w, W.words, sizeof(w), hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  if(w[RTW_ERR])
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_sinks_density: the active Type-5 particle with ID %u has no row in "
                     "the sink table (%d rows, %d active sinks)", (unsigned int) w[RTW_ERRKEY], T.n, w[RTW_COUNT]);
  const int ns = w[RTW_COUNT];
  if(ns > T.n)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_sinks_density: %d active Type-5 particles for %d rows of the sink "
                     "table: two of them carry the same ID", ns, T.n);
  if(ns <= 0)
    return GHIP_OK;
  // staging: SinkRec[ns] | h[ns] | out[6][ns] | slot[ns], as ghip_sink_density
  GCHK(ghip_ensure(ctx, ctx->stage, (size_t) ns * (sizeof(SinkRec) + 8 + 48 + 4) + 256));
  SinkRec *drecs = P<SinkRec>(ctx->stage);
  double *dh = reinterpret_cast<double *>(drecs + ns), *dout = dh + ns;
  int *dslot = reinterpret_cast<int *>(dout + 6 * (size_t) ns);
  AccK K = {};
  k_acc_begin<<<cdiv(ns, 64), 64, 0, st>>>(ns, W.words, W.b, W.row, ctx->n, P<double>(ctx->f[GHIP_F_POS]),
                                           P<double>(ctx->f[GHIP_F_VEL]), P<double>(ctx->f[GHIP_F_MASS]),
                                           P<double>(ctx->f[GHIP_F_HSML]), P<int>(ctx->f[GHIP_F_TIMEBIN]),
                                           P<int>(ctx->f[GHIP_F_ID]), P<double>(T.rows), K, 0, drecs, dh);
  HIPCHK(hipGetLastError());
  SinkIter I;
  sink_iter_init(I, ns);
  HIPCHK(hipMemcpyAsync(I.h.data(), dh, (size_t) ns * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  std::vector<double> hout((size_t) ns * 7);
  const int maxiter = p->MaxIter > 0 ? p->MaxIter : 150;
  int ncur = ns, iter = 0;
  while(ncur > 0)
    {
      GCHK(sink_density_pass(ctx, p, ns, drecs, dh, dslot, dout, I, ncur, 0));
      HIPCHK(hipMemcpyAsync(hout.data(), dout, (size_t) ns * 48, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      ncur = sink_iterate(p, ngb_factor, ns, hout.data(), ncur, I);
      if(ncur > 0)
        {
          iter++;
          if(iter > maxiter)
            return ghip_fail(ctx, GHIP_ENOCONV, "sink density: %d sinks not converged after %d h-iterations "
                             "(reference: endrun(1155))", ncur, maxiter);
        }
    }
  // the results go back as one block (dh | dout hold 7 planes) and from there into HSML and the rows
  for(int a = 0; a < ns; a++)
    {
      hout[a] = I.h[a];
      hout[(size_t) ns + a] = I.numngb[a];
      hout[2 * (size_t) ns + a] = I.rho[a];
      hout[3 * (size_t) ns + a] = I.entropy[a];
      for(int k = 0; k < 3; k++)
        hout[4 * (size_t) ns + 3 * (size_t) a + k] = I.gasvel[3 * (size_t) a + k];
    }
  HIPCHK(hipMemcpyAsync(dh, hout.data(), (size_t) ns * 56, hipMemcpyHostToDevice, st));
  k_sk_store_density<<<cdiv(ns, 64), 64, 0, st>>>(ns, W.b, W.row, dh, P<double>(ctx->f[GHIP_F_HSML]),
                                                  P<double>(T.rows));
  HIPCHK(hipGetLastError());
  HIPCHK(ghip_stream_sync(ctx, st));   // (hout goes out of scope)
  if(iterations)
    *iterations = iter;
  return GHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// blackhole_accretion()
// ---------------------------------------------------------------------------------------------
// before the swallow pass: each sink's own SwallowID as the marking pass left it, and BH_Mass by particle
__global__ void k_acc_marks(int G, const int *__restrict__ words, const int *__restrict__ row,
                            const unsigned int *__restrict__ swallow, const double *__restrict__ rows,
                            SinkRec *__restrict__ recs, double *__restrict__ dpbh)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  const int cnt = words[RTW_COUNT] < G ? words[RTW_COUNT] : G;
  if(a >= cnt || SK_BAD(words, G))
    return;
  const int i = recs[a].index;
  recs[a].mark = swallow[i];
  dpbh[i] = rows[(size_t) row[a] * SK_NC + GHIP_SK_BH_MASS];
}

// blackhole.c:679-714 for sink a; out: the [9][G] planes of k_bh_swallow
__global__ void k_acc_finish(int G, const int *__restrict__ words, const int *__restrict__ row,
                             const SinkRec *__restrict__ recs, const double *__restrict__ out,
                             const int *__restrict__ victim, int n, double *__restrict__ vel,
                             double *__restrict__ mass, double *__restrict__ rows, AccK K,
                             const unsigned long long *__restrict__ gate)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  const int cnt = words[RTW_COUNT] < G ? words[RTW_COUNT] : G;
  if(a >= cnt || SK_BAD(words, G) || (gate && *gate))   // gate: the shards' common verdict, not 0 = the call fails
    return;
  const int i = recs[a].index;
  double *R = rows + (size_t) row[a] * SK_NC;
  const double am = out[a], ab = out[(size_t) G + a], ad = out[2 * (size_t) G + a];
  if(victim[i])
    R[GHIP_SK_BH_MASS] = 0;   // P[j].BH_Mass = 0 of a swallowed sink (blackhole.c:1274)
  R[GHIP_SK_ACC_MASS] = am;
  R[GHIP_SK_ACC_BHMASS] = ab;
  R[GHIP_SK_ACC_DUSTMASS] = ad;
  for(int k = 0; k < 3; k++)
    R[GHIP_SK_ACC_MOMENTUM + k] = out[(size_t) (3 + k) * G + a];
  if(am > 0)
    {
      const double m = mass[i];
      for(int k = 0; k < 3; k++)
        {
          const double v = vel[(size_t) k * n + i];
          vel[(size_t) k * n + i] = (v * m + out[(size_t) (3 + k) * G + a]) / (m + am);
        }
      double mnew = m + am;
      R[GHIP_SK_BH_MASS] += ab;
      if(K.dust)
        R[GHIP_SK_DUST_MASS] += ad;
      if(K.limited)
        {
          R[GHIP_SK_ACCDISC_MASS] += am;
          if(K.at_edd)
            mnew = R[GHIP_SK_BH_MASS];
        }
      if(K.dust)
        R[GHIP_SK_TOTAL_MASS] += am;
      mass[i] = mnew;
    }
}

// blackhole.c:715-719 and the counts: one thread, active-list order
__global__ void k_acc_report(int G, const int *__restrict__ words, const int *__restrict__ row,
                             const SinkRec *__restrict__ recs, const double *__restrict__ out,
                             const double *__restrict__ mass, const double *__restrict__ rows,
                             ghip_bh_accretion_report *__restrict__ rep)
{
  if(blockIdx.x != 0 || threadIdx.x != 0)
    return;
  for(int b = 0; b < 32; b++)
    rep->TimeBin_BH_mass[b] = rep->TimeBin_BH_dynamicalmass[b] = rep->TimeBin_BH_Mdot[b] = 0;
  rep->swallowed[0] = rep->swallowed[1] = rep->swallowed[2] = 0;
  rep->nactive_sinks = words[RTW_COUNT];
  rep->missing = words[RTW_ERR] ? 1 : (words[RTW_COUNT] > G ? 2 : 0);
  rep->missing_id = (unsigned int) words[RTW_ERRKEY];
  rep->pad = 0;
  if(rep->missing)
    return;
  const int cnt = words[RTW_COUNT] < G ? words[RTW_COUNT] : G;
  for(int a = 0; a < cnt; a++)
    {
      const double *R = rows + (size_t) row[a] * SK_NC;
      const int bin = recs[a].timebin;
      if(bin >= 0 && bin < 32)
        {
          rep->TimeBin_BH_mass[bin] += R[GHIP_SK_BH_MASS];
          rep->TimeBin_BH_dynamicalmass[bin] += mass[recs[a].index];
          rep->TimeBin_BH_Mdot[bin] += R[GHIP_SK_BH_MDOT];
        }
      for(int k = 0; k < 3; k++)
        rep->swallowed[k] += (long long) (out[(size_t) (6 + k) * G + a] + 0.5);
    }
}

static AccK acc_kparams(const ghip_bh_params *bh, const ghip_bh_accretion_params *p)
{
  AccK K;
  K.limited = p->limited_accretion != 0;
  K.at_edd = p->accretion_at_eddington_rate != 0;
  K.enforce = p->enforce_eddington_limit != 0;
  K.mass_real = p->bh_mass_real != 0;
  K.dust = bh->dust != 0;
  K.medd_fac = p->medd_fac;
  K.tvisc = p->tvisc;
  K.eddf = p->EddingtonFactor;
  K.dt_fac = bh->dt_fac;
  return K;
}

extern "C" int ghip_blackhole_accretion(ghip_ctx *ctx, const ghip_bh_params *bh, const ghip_bh_accretion_params *p,
                                        ghip_bh_accretion_report *report)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !bh || !p || !report)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_blackhole_accretion: bad arguments");
  memset(report, 0, sizeof(*report));
  GCHK(sk_one_gpu(ctx, "ghip_blackhole_accretion", "GHIP_DD_BH_SWALLOW"));
  GCHK(sk_enter(ctx, "ghip_blackhole_accretion", true));
  if(!ctx->gt.built)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_blackhole_accretion: call ghip_tree_build first");
  GCHK(ghip_sink_buffers(ctx));
  RowTable &T = ctx->sk;
  hipStream_t st = ctx->stream;
  const int G = T.n;
  const size_t n = (size_t) ctx->n;
  const AccK K = acc_kparams(bh, p);
  // staging: SinkRec[G] | out [9][G] ; particle-indexed: bh mass [n], victim [n]
  const size_t g1 = (size_t) (G > 0 ? G : 1), n1 = n > 0 ? n : 1;
  GCHK(ghip_ensure(ctx, ctx->stage, g1 * (sizeof(SinkRec) + 72) + n1 * 12 + 512));
  SinkRec *drecs = P<SinkRec>(ctx->stage);
  double *dout = reinterpret_cast<double *>(drecs + g1), *dpbh = dout + 9 * g1;
  int *dvict = reinterpret_cast<int *>(dpbh + n1);
  RtWork W;
  int nact = 0;
  GCHK(sk_select(ctx, G, W, &nact));
  ghip_bh_accretion_report *drep = reinterpret_cast<ghip_bh_accretion_report *>(W.report);
  // P[].SwallowID = 0, Injected_BH_Energy = 0 (blackhole.c: the start of blackhole_accretion)
  HIPCHK(hipMemsetAsync(ctx->bh_swallow.p, 0, ctx->bh_swallow.cap, st));
  HIPCHK(hipMemsetAsync(ctx->bh_injected.p, 0, ctx->bh_injected.cap, st));
  if(G > 0 && nact > 0 && n > 0)
    {
      const int nb = cdiv(G, 64);
      HIPCHK(hipMemsetAsync(dpbh, 0, n * 12, st));
      k_acc_begin<<<nb, 64, 0, st>>>(G, W.words, W.b, W.row, ctx->n, P<double>(ctx->f[GHIP_F_POS]),
                                     P<double>(ctx->f[GHIP_F_VEL]), P<double>(ctx->f[GHIP_F_MASS]),
                                     P<double>(ctx->f[GHIP_F_HSML]), P<int>(ctx->f[GHIP_F_TIMEBIN]),
                                     P<int>(ctx->f[GHIP_F_ID]), P<double>(T.rows), K, 1, drecs, nullptr);
      HIPCHK(hipGetLastError());
      GCHK(ghip_bh_launch_evaluate(ctx, bh, G, drecs));
      k_acc_marks<<<nb, 64, 0, st>>>(G, W.words, W.row, P<unsigned int>(ctx->bh_swallow), P<double>(T.rows), drecs,
                                     dpbh);
      HIPCHK(hipGetLastError());
      GCHK(ghip_bh_launch_swallow(ctx, bh, G, drecs, dpbh, dvict, dout));
      k_acc_finish<<<nb, 64, 0, st>>>(G, W.words, W.row, drecs, dout, dvict, ctx->n, P<double>(ctx->f[GHIP_F_VEL]),
                                      P<double>(ctx->f[GHIP_F_MASS]), P<double>(T.rows), K, nullptr);
      HIPCHK(hipGetLastError());
    }
  k_acc_report<<<1, 64, 0, st>>>(G, W.words, W.row, drecs, dout,
                                 P<double>(ctx->f[GHIP_F_MASS]), P<double>(T.rows), drep);
  HIPCHK(hipGetLastError());
  // the one blocking read of the call
  HIPCHK(hipMemcpyAsync(report, drep, sizeof(*report), hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  if(report->missing == 1)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_blackhole_accretion: the active Type-5 particle with ID %u has no row "
                     "in the sink table (%d rows, %d active sinks); nothing but the marks was changed",
                     report->missing_id, T.n, report->nactive_sinks);
  if(report->missing)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_blackhole_accretion: %d active Type-5 particles for %d rows of the sink "
                     "table: two of them carry the same ID; nothing but the marks was changed",
                     report->nactive_sinks, T.n);
  ctx->gt.built = false;   // masses changed: the trees' moments are stale
  ctx->st.built = false;
  return GHIP_OK;
}

// ---------------------------------------------------------------------------------------------
// BH_FORM: a flagged gas particle becomes a sink (sfr_eff.c:602-629)
// ---------------------------------------------------------------------------------------------
// the new rows and masses of the candidates; no field is written yet
__global__ void k_form_rows(int ncand, const int *__restrict__ cand, const double *__restrict__ u01, int n,
                            const double *__restrict__ mass, const int *__restrict__ idf, int limited,
                            unsigned int *__restrict__ new_id, double *__restrict__ new_rows,
                            double *__restrict__ mold, double *__restrict__ mnew)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if(k >= ncand)
    return;
  const int i = cand[k];
  const bool ok = i >= 0 && i < n;
  const double m = ok ? mass[i] : 0.0;
  const double mm = m * (0.995 + 0.005 * u01[k]);
  mold[k] = m;
  mnew[k] = mm;
  new_id[k] = ok ? (unsigned int) idf[i] : 0u;
  double *R = new_rows + (size_t) k * SK_NC;
  for(int c = 0; c < SK_NC; c++)
    R[c] = 0;
  if(limited)
    R[GHIP_SK_ACCDISC_MASS] = mm;
  else
    R[GHIP_SK_BH_MASS] = mm;
}

__global__ void k_form_apply(int ncand, const int *__restrict__ cand, const double *__restrict__ mnew, int n,
                             double *__restrict__ mass, int *__restrict__ type)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if(k >= ncand)
    return;
  const int i = cand[k];
  if(i >= 0 && i < n)
    {
      type[i] = 5;
      mass[i] = mnew[k];
    }
}

// one thread, list order
__global__ void k_form_report(int ncand, const int *__restrict__ cand, const double *__restrict__ mold, int n,
                              const int *__restrict__ timebin, ghip_sfr_form_report *__restrict__ rep)
{
  if(blockIdx.x != 0 || threadIdx.x != 0)
    return;
  rep->stars_converted = ncand;
  rep->pad = 0;
  rep->sum_mass_stars = 0;
  for(int b = 0; b < 32; b++)
    rep->converted_in_bin[b] = 0;
  for(int k = 0; k < ncand; k++)
    {
      rep->sum_mass_stars += mold[k];
      const int i = cand[k];
      const int bin = (i >= 0 && i < n) ? timebin[i] : -1;
      if(bin >= 0 && bin < 32)
        rep->converted_in_bin[bin]++;
    }
}

extern "C" int ghip_sfr_form_sinks(ghip_ctx *ctx, int ncand, const double *u01, int limited_accretion,
                                   ghip_sfr_form_report *report)
{
  if(ctx)
    GHIP_JOIN(ctx);
  if(!ctx || !report || ncand < 0 || (ncand > 0 && !u01))
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_sfr_form_sinks: bad arguments");
  GCHK(sk_enter(ctx, "ghip_sfr_form_sinks", false));
  RowTable &T = ctx->sk;
  GCHK(ghip_rt_need(ctx, T, "ghip_sfr_form_sinks", false));
  if(ctx->sfr_ncand < 0)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_sfr_form_sinks: no candidates in place: ghip_sfr_cooling has not run "
                     "since the particles were last reordered, recounted or converted");
  if(ncand != ctx->sfr_ncand)
    return ghip_fail(ctx, GHIP_EINVAL, "ghip_sfr_form_sinks: ncand = %d, the last ghip_sfr_cooling found %d", ncand,
                     ctx->sfr_ncand);
  memset(report, 0, sizeof(*report));
  ctx->sfr_ncand = -1;   // consumed
  ghip_rt_open_empty(T);
  if(ncand == 0)
    return GHIP_OK;
  hipStream_t st = ctx->stream;
  const int old = T.n, m = old + ncand;
  GCHK(ghip_rt_stage(ctx, T, m, true));   // the old rows in front, the new ones behind
  // staging: u01 | mass before | mass after [ncand]
  GCHK(ghip_ensure(ctx, ctx->stage, (size_t) ncand * 24 + 256));
  double *du = P<double>(ctx->stage), *dmold = du + ncand, *dmnew = dmold + ncand;
  const int *dcand = P<int>(ctx->sfr_cand);
  HIPCHK(hipMemcpyAsync(du, u01, (size_t) ncand * 8, hipMemcpyHostToDevice, st));
  k_form_rows<<<cdiv(ncand, 256), 256, 0, st>>>(ncand, dcand, du, ctx->n, P<double>(ctx->f[GHIP_F_MASS]),
                                                P<int>(ctx->f[GHIP_F_ID]), limited_accretion != 0,
                                                P<unsigned int>(T.tmp_key) + old,
                                                P<double>(T.tmp_rows) + (size_t) old * SK_NC, dmold, dmnew);
  HIPCHK(hipGetLastError());
  // (sorts, and waits: a duplicate ID is refused before any field changes)
  int hw[RTW_WORDS];
  RtWork W;
  GCHK(ghip_rt_install(ctx, T, m, "ghip_sfr_form_sinks", false, hw));
  GCHK(ghip_rt_work(ctx, T, (size_t) m, 0, W, false));
  ghip_sfr_form_report *drep = reinterpret_cast<ghip_sfr_form_report *>(W.report);
  k_form_report<<<1, 64, 0, st>>>(ncand, dcand, dmold, ctx->n, P<int>(ctx->f[GHIP_F_TIMEBIN]), drep);
  k_form_apply<<<cdiv(ncand, 256), 256, 0, st>>>(ncand, dcand, dmnew, ctx->n, P<double>(ctx->f[GHIP_F_MASS]),
                                                 P<int>(ctx->f[GHIP_F_TYPE]));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(report, drep, sizeof(*report), hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  // as after ghip_set_field of TYPE and MASS
  ctx->pot_n = -1;
  ctx->gt.built = false;
  ctx->st.built = false;
  ctx->dd.geom_kept = false;
  return ghip_check_gas_types(ctx);
}

extern "C" size_t ghip_dd_sinks_args_size(void) { return sizeof(ghip_dd_sinks_args); }

// ---------------------------------------------------------------------------------------------
// the rows in GHIP_DD_MIGRATE: a departing Type-5 particle takes its row to the shard that receives it, in a
// second all-to-all-v of (ID, SK_NC doubles) records beside the particles' own (ghip_dd.hip, migrate_step)
// ---------------------------------------------------------------------------------------------
struct SkMigRec
{
  unsigned long long id;
  double c[SK_NC];
};
struct SkMigOff
{
  int v[GHIP_MAXRANKS];
};

// rows per destination; keep[row] = 0 for a row that departs.  (A departing Type-5 particle without a row departs
// without one: the next pass says so.)
__global__ void k_skm_count(int total, const int *__restrict__ list, const unsigned long long *__restrict__ mask,
                            const int *__restrict__ type, const int *__restrict__ idf, int nrows,
                            const unsigned int *__restrict__ ids, int *__restrict__ keep, int *__restrict__ cnt)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= total)
    return;
  const int i = list[a];
  if(type[i] != 5 || mask[i] == 0)
    return;
  const int r = d_rt_find(nrows, ids, (unsigned int) idf[i]);
  if(r < 0)
    return;
  keep[r] = 0;
  atomicAdd(cnt + (__ffsll((long long) mask[i]) - 1), 1);
}

// (the order within a destination is that of the atomics: the receiver sorts by ID)
__global__ void k_skm_pack(int total, const int *__restrict__ list, const unsigned long long *__restrict__ mask,
                           const int *__restrict__ type, const int *__restrict__ idf, int nrows,
                           const unsigned int *__restrict__ ids, const double *__restrict__ rows, SkMigOff off,
                           SkMigOff lim, int *__restrict__ cur, SkMigRec *__restrict__ out)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= total)
    return;
  const int i = list[a];
  if(type[i] != 5 || mask[i] == 0)
    return;
  const unsigned int id = (unsigned int) idf[i];
  const int r = d_rt_find(nrows, ids, id);
  if(r < 0)
    return;
  const int dest = __ffsll((long long) mask[i]) - 1;
  const int k = atomicAdd(cur + dest, 1);
  if(k >= lim.v[dest])   // (cannot happen: k_skm_count counted the same records)
    return;
  SkMigRec &R = out[off.v[dest] + k];
  R.id = id;
  for(int c = 0; c < SK_NC; c++)
    R.c[c] = rows[(size_t) r * SK_NC + c];
}

__global__ void k_skm_unpack(int nrecv, const SkMigRec *__restrict__ rec, unsigned int *__restrict__ id,
                             double *__restrict__ rows)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= nrecv)
    return;
  id[a] = (unsigned int) rec[a].id;
  for(int c = 0; c < SK_NC; c++)
    rows[(size_t) a * SK_NC + c] = rec[a].c[c];
}

int ghip_sinks_mig_pack(ghip_ctx *ctx, int total, const int *list, const unsigned long long *mask)
{
  static_assert(sizeof(SkMigRec) == 8 + 8 * SK_NC, "SkMigRec layout");
  DDState &D = ctx->dd;
  RowTable &T = ctx->sk;
  hipStream_t st = ctx->stream;
  const int m = T.n, P_ = D.nranks;
  GCHK(ghip_ensure(ctx, D.sk_keep, (size_t) (m > 0 ? m : 1) * 4));
  GCHK(ghip_ensure(ctx, D.sk_rcnt, (size_t) 2 * GHIP_MAXRANKS * 4));
  HIPCHK(hipMemsetAsync(D.sk_rcnt.p, 0, (size_t) 2 * GHIP_MAXRANKS * 4, st));
  int cnt[GHIP_MAXRANKS];
  for(int r = 0; r < GHIP_MAXRANKS; r++)
    cnt[r] = D.sk_rscount[r] = D.sk_rsoff[r] = 0;
  if(m > 0)
    HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(D.sk_keep.p), 1, (size_t) m, st));
  const bool any = m > 0 && total > 0 && ctx->id_given;
  if(any)
    {
      k_skm_count<<<cdiv(total, 256), 256, 0, st>>>(total, list, mask, P<int>(ctx->f[GHIP_F_TYPE]),
                                                   P<int>(ctx->f[GHIP_F_ID]), m, P<unsigned int>(T.key),
                                                   P<int>(D.sk_keep), P<int>(D.sk_rcnt));
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(cnt, D.sk_rcnt.p, (size_t) P_ * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
    }
  HIPCHK(hipGetLastError());
  SkMigOff off, lim;
  int tot = 0;
  for(int r = 0; r < GHIP_MAXRANKS; r++)
    {
      const int c = (r < P_ && cnt[r] > 0 && cnt[r] <= m) ? cnt[r] : 0;
      off.v[r] = tot;
      lim.v[r] = c;
      D.sk_rscount[r] = c;
      D.sk_rsoff[r] = tot;
      tot += c;
    }
  GCHK(ghip_ensure(ctx, D.sk_rsend, (size_t) (tot > 0 ? tot : 1) * sizeof(SkMigRec)));
  if(tot > 0)
    {
      k_skm_pack<<<cdiv(total, 256), 256, 0, st>>>(total, list, mask, P<int>(ctx->f[GHIP_F_TYPE]),
                                                  P<int>(ctx->f[GHIP_F_ID]), m, P<unsigned int>(T.key),
                                                  P<double>(T.rows), off, lim, P<int>(D.sk_rcnt) + GHIP_MAXRANKS,
                                                  P<SkMigRec>(D.sk_rsend));
      HIPCHK(hipGetLastError());
    }
  return GHIP_OK;
}

void ghip_sinks_mig_post(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  ghip_dd_set_alltoallv(D, D.sk_rsend.p, sizeof(SkMigRec), D.sk_rscount, D.sk_rsoff, &D.sk_rrecv);
}

// after the second exchange: the rows that left are dropped, the arrivals join, the table is sorted again
int ghip_sinks_mig_merge(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  RowTable &T = ctx->sk;
  hipStream_t st = ctx->stream;
  const int m = T.n, nrecv = D.x.rtotal;
  int sent = 0;
  for(int r = 0; r < D.nranks; r++)
    sent += D.sk_rscount[r];
  if(sent == 0 && nrecv == 0)
    return GHIP_OK;
  RtWork W;
  GCHK(ghip_rt_work(ctx, T, (size_t) (m + nrecv + 1), 0, W, true));
  int kept = 0, hw[RTW_WORDS];
  GCHK(ghip_rt_compact(ctx, T, "GHIP_DD_MIGRATE", W, P<int>(D.sk_keep), nullptr, nrecv, &kept));
  if(nrecv == 0)
    return GHIP_OK;   // (nothing arrived: compacted in place, ascending still)
  k_skm_unpack<<<cdiv(nrecv, 256), 256, 0, st>>>(nrecv, P<SkMigRec>(D.sk_rrecv), P<unsigned int>(T.tmp_key) + kept,
                                                P<double>(T.tmp_rows) + (size_t) kept * SK_NC);
  HIPCHK(hipGetLastError());
  return ghip_rt_install(ctx, T, kept + nrecv, "GHIP_DD_MIGRATE", false, hw);
}

// ---------------------------------------------------------------------------------------------
// ghip_sinks_density and ghip_blackhole_accretion on shards: GHIP_DD_SINK_DENSITY / GHIP_DD_BH_SWALLOW begun with
// walk = GHIP_SINKS_RESIDENT_FORM.  The exchanges are those of the per-pass forms (ghip_sink.hip); what differs is
// where a shard's sinks come from (the device selection and the table) and where the results go (the fields and
// the rows).  A shard that cannot post its sinks -- no table, an active Type-5 particle without a row -- posts ONE
// failure record instead (index -1: timebin = the kind, id, x = its rank) and holds its error (ghip_dd_hold).
// Every shard reads the same gathered records, so k_skd_check gives every shard the same verdict without another
// exchange: kind << 40 | rank << 32 | id, the largest, 0 = fine.  When it is not 0 the gathered records are made
// inert (mass 0: marks nothing; mark set: sweeps nothing), the rows are put back as they were before the Mdot step,
// the finish is gated, every exchange still takes place, and all shards fail together at the end.
// ---------------------------------------------------------------------------------------------
enum { SKD_NOROW = 1, SKD_LOCALDUP, SKD_NOTABLE, SKD_DUP };
#define SKD_WORD(kind, rank, id) \
  (((unsigned long long) (kind) << 40) | ((unsigned long long) ((rank) & 0xff) << 32) | (unsigned long long) (id))

__global__ void k_skd_check(int ns, const SinkRec *__restrict__ recs, unsigned long long *__restrict__ gw)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a >= ns)
    return;
  const int idx = recs[a].index;
  const unsigned int id = recs[a].id;
  if(idx < 0)
    {
      atomicMax(gw, SKD_WORD(recs[a].timebin, (int) recs[a].x, id));
      return;
    }
  for(int b = a + 1; b < ns; b++)   // (hundreds of sinks)
    if(recs[b].index >= 0 && recs[b].id == id)
      {
        atomicMax(gw, SKD_WORD(SKD_DUP, 0xff, id));
        break;
      }
}

__global__ void k_skd_inert(int ns, SinkRec *__restrict__ recs, const unsigned long long *__restrict__ gw)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a < ns && *gw)
    {
      recs[a].mass = 0;
      recs[a].mark = 1;
    }
}

__global__ void k_skd_restore(long long m, const double *__restrict__ snap, double *__restrict__ rows,
                              const unsigned long long *__restrict__ gw)
{
  const long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x;
  if(e < m && *gw)
    rows[e] = snap[e];
}

__global__ void k_skd_h(int ns, const SinkRec *__restrict__ recs, double *__restrict__ h)
{
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if(a < ns)
    h[a] = recs[a].h;
}

// the all-gathered partial planes [nranks][9][ns] of this shard's own sinks [off, off + cnt), added in ascending rank
// order from 0.0 with plain adds: the bits of the per-pass form's host loop (dd_sink_sum_parts).  out: [9][cnt]
__global__ void k_skd_sum_own(int nranks, int ns, int off, int cnt, const double *__restrict__ parts,
                              double *__restrict__ out)
{
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if(e >= 9 * cnt)
    return;
  const int plane = e / cnt, a = e % cnt;
  double s = 0.0;
  for(int r = 0; r < nranks; r++)
    s += parts[((size_t) r * 9 + plane) * ns + off + a];
  out[e] = s;
}

// the report on a shard: the counts are those of THIS shard's particles (its own partial planes, all sinks), and
// a failed call reports its verdict and no sums
__global__ void k_skd_report(int ns, const double *__restrict__ part, const unsigned long long *__restrict__ gw,
                             ghip_bh_accretion_report *__restrict__ rep)
{
  if(blockIdx.x != 0 || threadIdx.x != 0)
    return;
  for(int k = 0; k < 3; k++)
    {
      long long c = 0;
      for(int g = 0; g < ns; g++)
        c += (long long) (part[(size_t) (6 + k) * ns + g] + 0.5);
      rep->swallowed[k] = c;
    }
  const unsigned long long w = *gw;
  if(w)
    {
      for(int b = 0; b < 32; b++)
        rep->TimeBin_BH_mass[b] = rep->TimeBin_BH_dynamicalmass[b] = rep->TimeBin_BH_Mdot[b] = 0;
      rep->missing = (int) (w >> 40);
      rep->missing_id = (unsigned int) w;
    }
}

static int skd_w(ghip_ctx *ctx, RtWork &W)
{
  return ghip_rt_work(ctx, ctx->sk, ctx->dd.sk_na, ctx->dd.sk_nrow, W, false);
}

// all shards stop together: the shard that posted the failure record with its own message, the others with the
// verdict they all read
static int skd_fail(ghip_ctx *ctx, unsigned long long w, const char *who)
{
  if(ctx->dd.held.rc != GHIP_OK)
    return ghip_fail(ctx, ctx->dd.held.rc, "%s", ctx->dd.held.msg.c_str());
  const int kind = (int) (w >> 40), rank = (int) ((w >> 32) & 0xff);
  const unsigned int id = (unsigned int) w;
  const char *tail = "every shard stops here; nothing but the marks was changed";
  switch(kind)
    {
    case SKD_NOROW:
      return ghip_fail(ctx, GHIP_EINVAL, "%s: on shard %d the active Type-5 particle with ID %u has no row in the "
                       "sink table; %s", who, rank, id, tail);
    case SKD_LOCALDUP:
      return ghip_fail(ctx, GHIP_EINVAL, "%s: shard %d has more active Type-5 particles than rows in its sink table: "
                       "two of them carry the same ID; %s", who, rank, tail);
    case SKD_NOTABLE:
      return ghip_fail(ctx, GHIP_EINVAL, "%s: shard %d holds no sink table (or has not been given GHIP_F_ID): either "
                       "all shards hold one (an empty one counts) or none does; %s", who, rank, tail);
    default:
      return ghip_fail(ctx, GHIP_EINVAL, "%s: two active Type-5 particles of the run carry the ID %u; %s", who, id,
                       tail);
    }
}

int ghip_dd_sinks_begin(ghip_ctx *ctx, int op, const void *params)
{
  DDState &D = ctx->dd;
  const char *who = op == GHIP_DD_SINK_DENSITY ? "GHIP_DD_SINK_DENSITY" : "GHIP_DD_BH_SWALLOW";
  D.sinks = *reinterpret_cast<const ghip_dd_sinks_args *>(params);
  const ghip_dd_sinks_args &A = D.sinks;
  if(ctx->shard_n > 1)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: not available on a replicated shard (ghip_set_shard with %d ranks)", who,
                     ctx->shard_n);
  if(op == GHIP_DD_SINK_DENSITY)
    {
      if(!A.dens)
        return ghip_fail(ctx, GHIP_EINVAL, "%s (resident form): bad arguments", who);
      if(A.iterations)
        *A.iterations = 0;
      if(!ctx->st.built)
        return ghip_fail(ctx, GHIP_EINVAL, "%s: run GHIP_DD_DENSITY of this step first", who);
    }
  else
    {
      if(!A.bh || !A.acc || !A.report)
        return ghip_fail(ctx, GHIP_EINVAL, "%s (resident form): bad arguments", who);
      memset(A.report, 0, sizeof(*A.report));
      if(!ctx->gt.built)
        return ghip_fail(ctx, GHIP_EINVAL, "%s: run GHIP_DD_GRAVITY of this step first", who);
    }
  D.sink = ghip_dd_sink_args();   // (what the shared passes of ghip_sink.hip read)
  D.sink.dens = A.dens;
  D.sink.ngb_factor = A.ngb_factor;
  D.sink.bh = A.bh;
  D.sk_form = GHIP_SINKS_RESIDENT_FORM;
  return GHIP_OK;
}

// POST: this shard's active sinks, found in its table, to every shard
static int skd_post(ghip_ctx *ctx, bool swallow, const char *who)
{
  DDState &D = ctx->dd;
  RowTable &T = ctx->sk;
  hipStream_t st = ctx->stream;
  const ghip_dd_sinks_args &A = D.sinks;
  GCHK(ghip_sink_buffers(ctx));
  if(swallow)
    {
      // P[].SwallowID = 0, Injected_BH_Energy = 0 on every shard (ghip_sink_reset)
      HIPCHK(hipMemsetAsync(ctx->bh_swallow.p, 0, ctx->bh_swallow.cap, st));
      HIPCHK(hipMemsetAsync(ctx->bh_injected.p, 0, ctx->bh_injected.cap, st));
    }
  GCHK(ghip_ensure(ctx, D.sk_gw, 64));
  HIPCHK(hipMemsetAsync(D.sk_gw.p, 0, 64, st));
  int kind = 0, cnt = 0;
  unsigned int errid = 0;
  RtWork W;
  D.sk_na = D.sk_nrow = 1;
  if(!ctx->id_given || !T.on || T.stale)
    {
      kind = SKD_NOTABLE;
      GCHK(ghip_rt_work(ctx, T, D.sk_na, D.sk_nrow, W, true));
      if(!ctx->id_given)
        ghip_dd_hold(ctx, ghip_fail(ctx, GHIP_EINVAL, "%s: the sink table is keyed by P[].ID, and GHIP_F_ID has not "
                                    "been given since ghip_set_counts (ghip_set_field)", who));
      else if(T.on)
        ghip_dd_hold(ctx, ghip_rt_need(ctx, T, who, true));   // (stale)
      else
        ghip_dd_hold(ctx, ghip_fail(ctx, GHIP_EINVAL, "%s: this shard holds no sink table (ghip_sinks_set_table; "
                                    "either all shards hold one or none does)", who));
    }
  else
    {
      int nact = 0, w[RTW_WORDS];
      GCHK(sk_select(ctx, T.n, W, &nact));
      D.sk_na = (size_t) (nact > 0 ? nact : 1);
      D.sk_nrow = (size_t) (T.n > 0 ? T.n : 1);
      // (the first of the two blocking reads: the exchange needs the count)
      HIPCHK(hipMemcpyAsync(w, W.words, sizeof(w), hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      if(w[RTW_ERR])
        {
          kind = SKD_NOROW;
          errid = (unsigned int) w[RTW_ERRKEY];
          ghip_dd_hold(ctx, ghip_fail(ctx, GHIP_EINVAL, "%s: the active Type-5 particle with ID %u has no row in this "
                                      "shard's sink table (%d rows, %d active sinks); nothing but the marks was "
                                      "changed", who, errid, T.n, w[RTW_COUNT]));
        }
      else if(w[RTW_COUNT] > T.n)
        {
          kind = SKD_LOCALDUP;
          ghip_dd_hold(ctx, ghip_fail(ctx, GHIP_EINVAL, "%s: %d active Type-5 particles for %d rows of this shard's "
                                      "sink table: two of them carry the same ID; nothing but the marks was changed",
                                      who, w[RTW_COUNT], T.n));
        }
      else
        cnt = w[RTW_COUNT] > 0 ? w[RTW_COUNT] : 0;
    }
  D.sk_cnt = cnt;
  const int nsend = kind ? 1 : cnt;
  GCHK(ghip_ensure(ctx, D.sk_send, (size_t) (nsend > 0 ? nsend : 1) * sizeof(SinkRec)));
  if(kind)
    {
      SinkRec E;
      memset(&E, 0, sizeof(E));
      E.x = (double) D.rank;
      E.rho = 1.0;
      E.id = errid;
      E.timebin = kind;
      E.index = -1;
      E.mark = 1;
      HIPCHK(hipMemcpyAsync(D.sk_send.p, &E, sizeof(E), hipMemcpyHostToDevice, st));
      HIPCHK(ghip_stream_sync(ctx, st));   // (`E` lives on this frame)
    }
  else if(cnt > 0)
    {
      AccK K = {};
      if(swallow)
        {
          K = acc_kparams(A.bh, A.acc);
          GCHK(ghip_ensure(ctx, D.sk_snap, (size_t) T.n * SK_NC * 8));
          HIPCHK(hipMemcpyAsync(D.sk_snap.p, T.rows.p, (size_t) T.n * SK_NC * 8, hipMemcpyDeviceToDevice, st));
        }
      k_acc_begin<<<cdiv(cnt, 64), 64, 0, st>>>(cnt, W.words, W.b, W.row, ctx->n, P<double>(ctx->f[GHIP_F_POS]),
                                                P<double>(ctx->f[GHIP_F_VEL]), P<double>(ctx->f[GHIP_F_MASS]),
                                                P<double>(ctx->f[GHIP_F_HSML]), P<int>(ctx->f[GHIP_F_TIMEBIN]),
                                                P<int>(ctx->f[GHIP_F_ID]), P<double>(T.rows), K, swallow ? 1 : 0,
                                                P<SinkRec>(D.sk_send), nullptr);
      HIPCHK(hipGetLastError());
    }
  int scount[GHIP_MAXRANKS], soff[GHIP_MAXRANKS];
  for(int r = 0; r < D.nranks; r++)
    {
      scount[r] = nsend;
      soff[r] = 0;
    }
  ghip_dd_set_alltoallv(D, D.sk_send.p, sizeof(SinkRec), scount, soff, &D.sk_all);
  return 1;
}

int ghip_dd_sinks_step(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  RowTable &T = ctx->sk;
  hipStream_t st = ctx->stream;
  const ghip_dd_sinks_args &A = D.sinks;
  const bool swallow = D.op == GHIP_DD_BH_SWALLOW;
  const char *who = swallow ? "GHIP_DD_BH_SWALLOW" : "GHIP_DD_SINK_DENSITY";
  enum { POST, EVALUATE, SWALLOW, FINISH };   // (the density's third phase is COLLECT of ghip_sink.hip)
  const int cnt = D.sk_cnt;
  const size_t n = (size_t) ctx->n;
  unsigned long long *gw = P<unsigned long long>(D.sk_gw);
  if(D.phase == POST)
    {
      D.phase = EVALUATE;
      return skd_post(ctx, swallow, who);
    }
  if(D.phase == EVALUATE)
    {
      D.sk_total = D.x.rtotal;
      D.sk_off = D.x.roff[D.rank];
      const int ns = D.sk_total;
      if(D.x.rcount[D.rank] != (D.held.rc != GHIP_OK ? 1 : cnt))
        return ghip_fail(ctx, GHIP_ECOMM, "%s: the exchange lost this shard's own records", who);
      if(ns == 0)
        return 0;   // no active sink anywhere (the report is zero)
      SinkRec *all = P<SinkRec>(D.sk_all);
      k_skd_check<<<cdiv(ns, 64), 64, 0, st>>>(ns, all, gw);
      HIPCHK(hipGetLastError());
      if(!swallow)
        {
          // the h iteration is the host's: it starts from every sink's h, and it can stop here
          GCHK(ghip_ensure(ctx, D.sk_part, (size_t) ns * 48));
          k_skd_h<<<cdiv(ns, 64), 64, 0, st>>>(ns, all, P<double>(D.sk_part));
          HIPCHK(hipGetLastError());
          unsigned long long w = 0;
          sink_iter_init(D.sk_it, ns);
          HIPCHK(hipMemcpyAsync(D.sk_it.h.data(), D.sk_part.p, (size_t) ns * 8, hipMemcpyDeviceToHost, st));
          HIPCHK(hipMemcpyAsync(&w, gw, 8, hipMemcpyDeviceToHost, st));
          HIPCHK(ghip_stream_sync(ctx, st));
          if(w)
            return skd_fail(ctx, w, who);
          D.sk_ncur = ns;
          D.sk_iter = 0;
          D.phase = 2;   // COLLECT
          return dd_sink_density_pass(ctx);
        }
      k_skd_inert<<<cdiv(ns, 64), 64, 0, st>>>(ns, all, gw);
      if(cnt > 0)
        k_skd_restore<<<cdiv((long long) T.n * SK_NC, 256), 256, 0, st>>>((long long) T.n * SK_NC, P<double>(D.sk_snap),
                                                                         P<double>(T.rows), gw);
      HIPCHK(hipGetLastError());
      GCHK(ghip_bh_launch_evaluate(ctx, A.bh, ns, all));
      // each sink's own SwallowID as the marking pass left it goes into its record (the particle is local: its
      // mark saw every claim), BH_Mass by particle stays here; the records are posted again
      GCHK(ghip_ensure(ctx, D.sk_work, (n > 0 ? n : 1) * 12 + 64));
      double *dpbh = P<double>(D.sk_work);
      if(n > 0)
        HIPCHK(hipMemsetAsync(dpbh, 0, n * 12, st));
      if(cnt > 0)
        {
          RtWork W;
          GCHK(skd_w(ctx, W));
          k_acc_marks<<<cdiv(cnt, 64), 64, 0, st>>>(cnt, W.words, W.row, P<unsigned int>(ctx->bh_swallow),
                                                    P<double>(T.rows), P<SinkRec>(D.sk_send), dpbh);
          HIPCHK(hipGetLastError());
        }
      D.x.kind = 2;   // (the same send buffer, counts and offsets as the first time)
      D.phase = SWALLOW;
      return 1;
    }
  const int ns = D.sk_total;
  double *dpbh = P<double>(D.sk_work);
  int *dvict = reinterpret_cast<int *>(dpbh + n);
  if(D.phase == SWALLOW)
    {
      if(D.x.rtotal != ns)
        return ghip_fail(ctx, GHIP_ECOMM, "%s: %d records came back, %d went", who, D.x.rtotal, ns);
      SinkRec *all = P<SinkRec>(D.sk_all);
      k_skd_inert<<<cdiv(ns, 64), 64, 0, st>>>(ns, all, gw);
      HIPCHK(hipGetLastError());
      GCHK(ghip_ensure(ctx, D.sk_part, (size_t) ns * 72));
      GCHK(ghip_bh_launch_swallow(ctx, A.bh, ns, all, dpbh, dvict, P<double>(D.sk_part)));
      ghip_dd_set_allgather(D, D.sk_part.p, (size_t) ns * 72, &D.sk_parts);
      D.phase = FINISH;
      return 1;
    }
  if(D.phase == FINISH)
    {
      RtWork W;
      GCHK(skd_w(ctx, W));
      GCHK(ghip_ensure(ctx, D.sk_own, (size_t) (cnt > 0 ? cnt : 1) * 72));
      ghip_bh_accretion_report *drep = reinterpret_cast<ghip_bh_accretion_report *>(W.report);
      if(cnt > 0)
        {
          k_skd_sum_own<<<cdiv(9 * cnt, 64), 64, 0, st>>>(D.nranks, ns, D.sk_off, cnt, P<double>(D.sk_parts),
                                                         P<double>(D.sk_own));
          k_acc_finish<<<cdiv(cnt, 64), 64, 0, st>>>(cnt, W.words, W.row, P<SinkRec>(D.sk_send), P<double>(D.sk_own),
                                                     dvict, ctx->n, P<double>(ctx->f[GHIP_F_VEL]),
                                                     P<double>(ctx->f[GHIP_F_MASS]), P<double>(T.rows),
                                                     acc_kparams(A.bh, A.acc), gw);
          HIPCHK(hipGetLastError());
        }
      k_acc_report<<<1, 64, 0, st>>>(cnt, W.words, W.row, P<SinkRec>(D.sk_send), P<double>(D.sk_own),
                                     P<double>(ctx->f[GHIP_F_MASS]), P<double>(T.rows), drep);
      k_skd_report<<<1, 64, 0, st>>>(ns, P<double>(D.sk_part), gw, drep);
      HIPCHK(hipGetLastError());
      // the second blocking read: the report, and the verdict with it
      unsigned long long w = 0;
      HIPCHK(hipMemcpyAsync(A.report, drep, sizeof(*A.report), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(&w, gw, 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      if(w)
        return skd_fail(ctx, w, who);
      ctx->gt.built = false;   // masses changed: the trees' moments are stale
      ctx->st.built = false;
      D.geom_kept = true;      // (their geometry is not: the dust passes may still use them)
      return 0;
    }
  return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_step: the resident sink passes have no phase %d", D.phase);
}

// the end of GHIP_DD_SINK_DENSITY in its resident form: the converged values of this shard's own sinks
int ghip_dd_sinks_store_density(ghip_ctx *ctx)
{
  DDState &D = ctx->dd;
  hipStream_t st = ctx->stream;
  const int cnt = D.sk_cnt, off = D.sk_off;
  const SinkIter &I = D.sk_it;
  if(cnt > 0)
    {
      std::vector<double> hout((size_t) cnt * 7);
      for(int a = 0; a < cnt; a++)
        {
          const int g = off + a;
          hout[a] = I.h[g];
          hout[(size_t) cnt + a] = I.numngb[g];
          hout[2 * (size_t) cnt + a] = I.rho[g];
          hout[3 * (size_t) cnt + a] = I.entropy[g];
          for(int k = 0; k < 3; k++)
            hout[4 * (size_t) cnt + 3 * (size_t) a + k] = I.gasvel[3 * (size_t) g + k];
        }
      RtWork W;
      GCHK(skd_w(ctx, W));
      GCHK(ghip_ensure(ctx, D.sk_own, (size_t) cnt * 72));
      HIPCHK(hipMemcpyAsync(D.sk_own.p, hout.data(), (size_t) cnt * 56, hipMemcpyHostToDevice, st));
      k_sk_store_density<<<cdiv(cnt, 64), 64, 0, st>>>(cnt, W.b, W.row, P<double>(D.sk_own),
                                                       P<double>(ctx->f[GHIP_F_HSML]), P<double>(ctx->sk.rows));
      HIPCHK(hipGetLastError());
      HIPCHK(ghip_stream_sync(ctx, st));   // (hout goes out of scope)
    }
  if(D.sinks.iterations)
    *D.sinks.iterations = D.sk_iter;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// ghip_wind_spawn: the massive sinks create wind particles (momentum_feedback.c:70-246)
//
//   count   one thread per active sink (sk_select: active-list order), new_wind and correction_wind   :75-133
//   scan    exclusive scan of the counts; the total is the one blocking read; NumPart + total <= MaxPart  :149-156
//   grow    old_of_new[j] = j (j < n), = the parent sink of the appended j; the planes move as in ghip_rearrange  :158
//   fill    one thread per new particle: its sink by a search in the scanned counts, `bits` its rank there  :159-228
// The counts are of the order of the sinks: one 64-lane wavefront per workgroup; the map and the fill run over
// particles: 256 threads per workgroup.  Every store is a plain vector store.
// ---------------------------------------------------------------------------------------------
#define SPAWN_C 2.9979e10          // allvars.h:86
#define SPAWN_GRAVITY 6.672e-8     // allvars.h:79
#define SPAWN_THOMPSON 6.65245e-25 // allvars.h:91
#define SPAWN_PROTONMASS 1.6726e-24 // allvars.h:89
#define SPAWN_MAX_PER_SINK (1ULL << 30)

struct SpawnK
{
  double Time, dt_fac, smbh, vstart, vfb, vmass, fbv, uvel, soft, inner;
  double ledd;   // L_Edd_dimensionless (:36-37)
  double ewm;    // energy_wind_min (:39)
  double cu;     // C / UnitVelocity_in_cm_per_s
  int step, frac_ledd, at_edd, startup, isotropic, acc_radius, fly;
};

// what the host reads
struct SpawnWords
{
  unsigned long long total;
  int nactive, emitting, missing;
  unsigned int missing_id;
  double exact_sum;
};

struct SpawnDev
{
  SpawnWords *words;
  unsigned long long *cnt, *off;   // [G + 1]
  double *exact, *corr, *dt, *drm; // [G]
  int *qual;                       // [G]: the sink counts (:75)
};

static int spawn_dev(ghip_ctx *ctx, int G, SpawnDev &S)
{
  const size_t g1 = (size_t) G + 1;
  GCHK(ghip_ensure(ctx, ctx->wk_spawn, 64 + g1 * (2 * 8 + 4 * 8 + 4) + 64));
  char *base = P<char>(ctx->wk_spawn);
  S.words = reinterpret_cast<SpawnWords *>(base);
  S.cnt = reinterpret_cast<unsigned long long *>(base + 64);
  S.off = S.cnt + g1;
  S.exact = reinterpret_cast<double *>(S.off + g1);
  S.corr = S.exact + g1;
  S.dt = S.corr + g1;
  S.drm = S.dt + g1;
  S.qual = reinterpret_cast<int *>(S.drm + g1);
  return GHIP_OK;
}
static_assert(sizeof(SpawnWords) <= 64, "the words block of ghip_ctx::wk_spawn");

// :75-133 for record a < G; record G holds the zero behind the counts
__global__ void __launch_bounds__(64) k_spawn_count(int G, const int *__restrict__ words, const int *__restrict__ sel,
                                                    const int *__restrict__ row, const double *__restrict__ mass,
                                                    const int *__restrict__ timebin, const double *__restrict__ rows,
                                                    SpawnK K, SpawnDev S)
{
  const int a = blockIdx.x * 64 + threadIdx.x;
  if(a > G)
    return;
  if(a == G)
    {
      S.cnt[G] = 0;
      return;
    }
  const int c = words[RTW_COUNT] < G ? words[RTW_COUNT] : G;
  unsigned long long new_wind = 0;
  double exact = 0, corr = 1., dt = 0, drm = 0;
  int qual = 0;
  if(a < c && !SK_BAD(words, G))
    {
      const int i = sel[a];
      const double *R = rows + (size_t) row[a] * SK_NC;
      const double m = mass[i];
      if(m > 0.5 * K.smbh && K.Time > K.vstart)
        {
          qual = 1;
          const int tb = timebin[i];
          dt = (tb ? (double) (1 << tb) : 0.0) * K.dt_fac;
          drm = R[GHIP_SK_BH_DENSITY];
          if(K.frac_ledd)
            exact = K.vfb * K.ledd * (K.at_edd ? R[GHIP_SK_BH_MASS] : m) * dt / K.ewm;   // :85, :88
          else
            {
              const double cc = K.cu * K.cu;   // pow(C / U, 2)
              double lum = K.vfb * 0.1 * R[GHIP_SK_BH_MDOT] * cc;   // :100
              if(lum > K.ledd * m)
                lum = K.ledd * m;
              exact = K.vfb * lum * dt / K.ewm;   // :105
            }
          if(K.startup ? exact > 1.e-4 : exact > 0.)
            {
              // (int) new_wind_exact + 1; a count that no MaxPart can hold stands for itself
              new_wind = exact < (double) SPAWN_MAX_PER_SINK ? (unsigned long long) (int) exact + 1ULL : SPAWN_MAX_PER_SINK;
              corr = exact / (double) new_wind;
            }
        }
    }
  S.cnt[a] = new_wind;
  S.exact[a] = exact;
  S.corr[a] = corr;
  S.dt[a] = dt;
  S.drm[a] = drm;
  S.qual[a] = qual;
}

// one thread, active-list order
__global__ void k_spawn_words(int G, const int *__restrict__ words, SpawnDev S)
{
  if(blockIdx.x != 0 || threadIdx.x != 0)
    return;
  SpawnWords w;
  w.total = S.off[G];
  w.nactive = words[RTW_COUNT];
  w.missing = words[RTW_ERR] ? 1 : (words[RTW_COUNT] > G ? 2 : 0);
  w.missing_id = (unsigned int) words[RTW_ERRKEY];
  w.emitting = 0;
  w.exact_sum = 0;
  for(int a = 0; a < G; a++)
    if(S.cnt[a] > 0)
      {
        w.emitting++;
        w.exact_sum += S.exact[a];
      }
  *S.words = w;
}

// :89: P[i].Mass = P[i].BH_Mass of every counting sink
__global__ void __launch_bounds__(64) k_spawn_edd_mass(int G, const int *__restrict__ sel, const int *__restrict__ row,
                                                       const double *__restrict__ rows, const int *__restrict__ qual,
                                                       double *__restrict__ mass)
{
  const int a = blockIdx.x * 64 + threadIdx.x;
  if(a < G && qual[a])
    mass[sel[a]] = rows[(size_t) row[a] * SK_NC + GHIP_SK_BH_MASS];
}

// the sink of the t-th new particle: the last a with off[a] <= t (off[G] = total > t, so its count is not 0)
__device__ __forceinline__ int d_spawn_sink(int G, const unsigned long long *__restrict__ off, unsigned long long t)
{
  int lo = 0, hi = G;   // off[lo] <= t < off[hi]
  while(hi - lo > 1)
    {
      const int mid = (lo + hi) >> 1;
      if(off[mid] <= t)
        lo = mid;
      else
        hi = mid;
    }
  return lo;
}

__global__ void __launch_bounds__(256) k_spawn_map(int n, int nn, int G, const unsigned long long *__restrict__ off,
                                                   const int *__restrict__ sel, int *__restrict__ old_of_new)
{
  const int j = blockIdx.x * 256 + threadIdx.x;
  if(j >= nn)
    return;
  old_of_new[j] = j < n ? j : sel[d_spawn_sink(G, off, (unsigned long long) (j - n))];
}

// :159-228 for the new particle j = n + t, whose record is a copy of its sink's
__global__ void __launch_bounds__(256) k_spawn_fill(int total, int n, int nn, int G, SpawnDev S,
                                                    const int *__restrict__ sel, SpawnK K, int nrnd,
                                                    const double *__restrict__ rnd, int *__restrict__ type,
                                                    double *__restrict__ hsml, double *__restrict__ vel,
                                                    double *__restrict__ mass, int *__restrict__ idf,
                                                    double *__restrict__ kick_newdens, int *__restrict__ act_tail,
                                                    unsigned int *__restrict__ tab_idx, double *__restrict__ tab_rows)
{
  const int t = blockIdx.x * 256 + threadIdx.x;
  if(t >= total)
    return;
  const int a = d_spawn_sink(G, S.off, (unsigned long long) t);
  const unsigned int bits = (unsigned int) ((unsigned long long) t - S.off[a]);
  const int j = n + t;
  const size_t N = (size_t) nn;
  type[j] = 3;
  double h = hsml[j];
  h += K.soft;
  if(K.acc_radius)
    h += K.inner;
  hsml[j] = h;
  const unsigned int id = (unsigned int) idf[sel[a]], m = (unsigned int) nrnd;
  const double r1 = rnd[(id + 2u + bits + (unsigned int) K.step) % m];
  const double r2 = rnd[(id + 3u + bits + (unsigned int) K.step) % m];
  const double theta = K.isotropic ? acos(2. * r1 - 1.) : acos(0.5 * r1 + 0.5);
  const double phi = 2 * M_PI * (r2 + K.Time);
  const double dir[3] = {sin(theta) * cos(phi), sin(theta) * sin(phi), cos(theta)};
  for(int k = 0; k < 3; k++)
    vel[(size_t) k * N + j] = K.cu * dir[k] / K.fbv;   // :191
  idf[j] = (int) (id + (unsigned int) j);   // :215
  const double corr = S.corr[a];
  const double old = K.ewm / SPAWN_C * K.uvel * corr, birth = K.ewm * corr;   // :225-226
  mass[j] = K.vmass * old;
  if(kick_newdens)
    kick_newdens[j] = 0.;
  if(act_tail)
    act_tail[t] = j;
  tab_idx[t] = (unsigned int) j;
  double *R = tab_rows + (size_t) t * GHIP_WK_COUNT;
  for(int c = 0; c < GHIP_WK_COUNT; c++)
    R[c] = 0;
  R[GHIP_WK_STELLAR_AGE] = K.Time;
  R[GHIP_WK_BIRTH_ENERGY] = birth;
  R[GHIP_WK_OLD_MOMENTUM] = old;
  R[GHIP_WK_DRMIN] = K.fly ? 0. : S.drm[a];
  R[GHIP_WK_DT1] = S.dt[a];
}

extern "C" size_t ghip_wind_spawn_params_size(void)
{
  return sizeof(ghip_wind_spawn_params);
}

extern "C" size_t ghip_wind_spawn_report_size(void)
{
  return sizeof(ghip_wind_spawn_report);
}

// One call in three parts, so that the shard form (GHIP_WINDS_SPAWN_FORM, below) can put an exchange between the
// second and the third: the count and the scan with the one blocking read; what the words refuse; grow and fill.
struct SpawnRun
{
  SpawnK K;
  SpawnWords h;
  int G, n;
  size_t na, nrow;   // the sizes the selection asked of the sink table's work: the same block later
  int counted;       // 0: no active particle, nothing was counted and nothing is to do
};

static SpawnK spawn_k(const ghip_wind_spawn_params *p)
{
  SpawnK K;
  K.Time = p->Time;
  K.dt_fac = p->dt_fac;
  K.smbh = p->SMBHmass;
  K.vstart = p->VirtualStart;
  K.vfb = p->VirtualFeedBack;
  K.vmass = p->VirtualMass;
  K.fbv = p->FeedBackVelocity;
  K.uvel = p->UnitVelocity_in_cm_per_s;
  K.soft = p->SofteningBndryMaxPhys;
  K.inner = p->InnerBoundary;
  // :36-37; pow(x, 2) is x * x
  K.ledd = (4 * M_PI * SPAWN_GRAVITY * SPAWN_C * SPAWN_PROTONMASS / SPAWN_THOMPSON) / (K.uvel * K.uvel) * p->UnitTime_in_s;
  K.ewm = p->VirtualMomentum * SPAWN_C / K.uvel;
  K.cu = SPAWN_C / K.uvel;
  K.step = p->NumCurrentTiStep;
  K.frac_ledd = p->fraction_of_ledd_feedback != 0;
  K.at_edd = K.frac_ledd && p->accretion_at_eddington_rate != 0;
  K.startup = p->startup_luminosity != 0;
  K.isotropic = p->isotropic != 0;
  K.acc_radius = p->accretion_radius != 0;
  K.fly = p->fly_through_empty_space != 0;
  return K;
}

// ---- count, scan, the one blocking read ----
static int spawn_scan(ghip_ctx *ctx, const ghip_wind_spawn_params *p, SpawnRun &R)
{
  RowTable &T = ctx->sk;
  hipStream_t st = ctx->stream;
  memset(&R, 0, sizeof(R));
  R.K = spawn_k(p);
  R.G = T.n;
  R.n = ctx->n;
  const int G = R.G;
  RtWork W;
  int nact = 0;
  GCHK(sk_select(ctx, G, W, &nact));
  R.na = (size_t) (nact > 0 ? nact : 1);
  R.nrow = (size_t) (G > 0 ? G : 1);
  if(nact <= 0 || R.n == 0)
    return GHIP_OK;
  SpawnDev S;
  GCHK(spawn_dev(ctx, G, S));
  k_spawn_count<<<cdiv(G + 1, 64), 64, 0, st>>>(G, W.words, W.b, W.row, P<double>(ctx->f[GHIP_F_MASS]),
                                               P<int>(ctx->f[GHIP_F_TIMEBIN]), P<double>(T.rows), R.K, S);
  HIPCHK(hipGetLastError());
  GCHK(ghip_scan<unsigned long long>(ctx, S.cnt, S.off, G + 1, st));
  k_spawn_words<<<1, 64, 0, st>>>(G, W.words, S);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&R.h, S.words, sizeof(R.h), hipMemcpyDeviceToHost, st));
  HIPCHK(ghip_stream_sync(ctx, st));
  R.counted = 1;
  return GHIP_OK;
}

// what the words refuse; nothing has changed
static int spawn_verdict(ghip_ctx *ctx, const ghip_wind_spawn_params *p, const char *who, const SpawnRun &R)
{
  const SpawnWords &h = R.h;
  if(!R.counted)
    return GHIP_OK;
  if(h.missing == 1)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: the active Type-5 particle with ID %u has no row in the sink table (%d "
                     "rows, %d active sinks); nothing was changed", who, h.missing_id, ctx->sk.n, h.nactive);
  if(h.missing)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: %d active Type-5 particles for %d rows of the sink table: two of them "
                     "carry the same ID; nothing was changed", who, h.nactive, ctx->sk.n);
  if((unsigned long long) R.n + h.total > (unsigned long long) p->MaxPart)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: NumPart = %d and %llu new wind particles do not fit MaxPart = %d (the "
                     "reference's endrun(8888)); nothing was changed", who, R.n, h.total, p->MaxPart);
  return GHIP_OK;
}

// :89, then grow and fill
static int spawn_grow(ghip_ctx *ctx, const ghip_wind_spawn_params *p, const SpawnRun &R,
                      ghip_wind_spawn_report *report)
{
  if(!R.counted)
    return GHIP_OK;
  RowTable &T = ctx->sk;
  hipStream_t st = ctx->stream;
  const SpawnK &K = R.K;
  const SpawnWords &h = R.h;
  const int G = R.G, n = R.n;
  // The selection of spawn_scan again: the same sizes give the same block of ctx->sk.work, not cleared.  On shards an
  // exchange lies between the two parts; the invariant is that NOTHING uses the sink table's work block between
  // phase 0 and phase 1 of ghip_dd_spawn_step -- the all-gather of the status record touches status_own / status_all
  // only, and no other entry point may run on the context while the operation is in progress (ghip_dd_begin).
  RtWork W;
  GCHK(ghip_rt_work(ctx, T, R.na, R.nrow, W, false));
  SpawnDev S;
  GCHK(spawn_dev(ctx, G, S));
  const int total = (int) h.total, nn = n + total;
  report->spawned = total;
  report->nsinks_emitting = h.emitting;
  report->new_wind_exact_sum = h.exact_sum;
  report->gsl_draws = 3LL * total;
  if(K.at_edd && G > 0)
    {
      k_spawn_edd_mass<<<cdiv(G, 64), 64, 0, st>>>(G, W.b, W.row, P<double>(T.rows), S.qual, P<double>(ctx->f[GHIP_F_MASS]));
      HIPCHK(hipGetLastError());
    }
  if(total == 0)
    return GHIP_OK;

  // ---- grow ----
  const double *rnd = P<double>(ctx->rnd_table);
  int nrnd = ctx->rnd_n;
  if(p->rnd_table && p->nrnd > 0)
    {
      nrnd = p->nrnd;
      GCHK(ghip_ensure(ctx, ctx->wk_rnd, (size_t) nrnd * 8));
      HIPCHK(hipMemcpyAsync(ctx->wk_rnd.p, p->rnd_table, (size_t) nrnd * 8, hipMemcpyHostToDevice, st));
      rnd = P<double>(ctx->wk_rnd);
    }
  unsigned int *tab_idx = nullptr;
  int *act_tail = nullptr, *old_of_new = nullptr;
  double *tab_rows = nullptr;
  GCHK(ghip_rt_reserve(ctx, ctx->wk, total, &tab_idx, &tab_rows));
  const int old_nact = ctx->nactive;
  if(old_nact >= 0)   // the list in force, and the new particles behind it (:202-204)
    {
      GCHK(ghip_ensure(ctx, ctx->act_next, (size_t) (old_nact + total) * 4));
      if(old_nact > 0)
        HIPCHK(hipMemcpyAsync(ctx->act_next.p, ctx->act_host_idx.p, (size_t) old_nact * 4, hipMemcpyDeviceToDevice, st));
      act_tail = P<int>(ctx->act_next) + old_nact;
    }
  GCHK(ghip_seq_grow_begin(ctx, nn, &old_of_new));
  k_spawn_map<<<cdiv(nn, 256), 256, 0, st>>>(n, nn, G, S.off, W.b, old_of_new);
  HIPCHK(hipGetLastError());
  // (k_seq_move takes this map, which is not a permutation, and nn > n: see ghip_seq_grow_apply)
  GCHK(ghip_seq_grow_apply(ctx, nn));

  // ---- fill (the fields are the new layout's now) ----
  const bool nd = ctx->has_newdens && ctx->kick_fields_n == nn;
  k_spawn_fill<<<cdiv(total, 256), 256, 0, st>>>(total, n, nn, G, S, W.b, K, nrnd, rnd, P<int>(ctx->f[GHIP_F_TYPE]),
                                                 P<double>(ctx->f[GHIP_F_HSML]), P<double>(ctx->f[GHIP_F_VEL]),
                                                 P<double>(ctx->f[GHIP_F_MASS]), P<int>(ctx->f[GHIP_F_ID]),
                                                 nd ? P<double>(ctx->kick_newdens) : nullptr, act_tail, tab_idx, tab_rows);
  HIPCHK(hipGetLastError());
  HIPCHK(ghip_stream_sync(ctx, st));   // (the caller's rnd_table has been read)
  ghip_rt_appended(ctx->wk, total);
  if(old_nact >= 0)
    {
      ctx->act_host_idx.swap(ctx->act_next);
      ctx->nactive = old_nact + total;
    }
  return GHIP_OK;
}

extern "C" int ghip_wind_spawn(ghip_ctx *ctx, const ghip_wind_spawn_params *p, ghip_wind_spawn_report *report)
{
  if(ctx)
    GHIP_JOIN(ctx);
  static const char *who = "ghip_wind_spawn";
  if(!ctx || !p || !report)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: bad arguments", who);
  memset(report, 0, sizeof(*report));
  if(ctx->dd.on && ctx->dd.nranks > 1 && ctx->shard_n <= 1)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: the shard form is not built into this entry point: on a multi-GPU context "
                     "(ghip_dd_init with %d ranks) wind particles are created by GHIP_DD_WIND with walk = "
                     "GHIP_WINDS_SPAWN_FORM (ghip_dd_winds_args)", who, ctx->dd.nranks);
  GCHK(ghip_winds_enter(ctx, who));
  GCHK(sk_enter(ctx, who, true));
  GCHK(ghip_rt_need(ctx, ctx->wk, who, false));   // (no wind table yet: the first wind particles open one)
  if(!(p->rnd_table && p->nrnd > 0) && ctx->rnd_n <= 0)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: no RndTable: neither rnd_table / nrnd nor a table bound with "
                     "ghip_set_rnd_table", who);
  if(p->MaxPart < ctx->n)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: MaxPart = %d is below NumPart = %d", who, p->MaxPart, ctx->n);
  report->first_index = ctx->n;
  SpawnRun R;
  GCHK(spawn_scan(ctx, p, R));
  GCHK(spawn_verdict(ctx, p, who, R));
  return spawn_grow(ctx, p, R, report);
}

// ---------------------------------------------------------------------------------------------
// ghip_wind_spawn on shards: GHIP_DD_WIND begun with walk = GHIP_WINDS_SPAWN_FORM (ghip_dd_wind_begin / _step hand
// over).  The reference's creation is local per task (momentum_feedback.c:70-246): the new particle is P[NumPart +
// stars_spawned] of the TASK, its ID the sink's plus that local index, only tot_spawned is all-reduced (:240), and
// endrun(8888) on any task ends all.  So every shard runs the three parts of ghip_wind_spawn on its own sinks, with
// one all-gather of {spawned, sinks emitting, new_wind_exact sum, failed} between the verdict and the growth: a
// shard that cannot go on (no sink or wind table, no RndTable in the params, an active Type-5 particle without a
// row, NumPart + total > MaxPart) holds its message, every shard takes the exchange, and then all return GHIP_EINVAL
// naming the shard, no byte changed anywhere.  Otherwise each shard grows and fills locally; a shard that spawns
// nothing changes nothing.
// ---------------------------------------------------------------------------------------------
int ghip_dd_spawn_begin(ghip_ctx *ctx, const void *params)
{
  static const char *who = "ghip_dd wind spawn";
  const ghip_dd_winds_args &a = *reinterpret_cast<const ghip_dd_winds_args *>(params);
  if(!a.spawn || !a.report || !a.tot_spawned)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: bad arguments (spawn, report and tot_spawned of ghip_dd_winds_args)", who);
  if(ctx->shard_n > 1)
    return ghip_fail(ctx, GHIP_EINVAL, "%s: not available on a sharded context (ghip_set_shard)", who);
  WindDD &W = ctx->dd.wind;
  W = WindDD();
  W.form = GHIP_WINDS_SPAWN_FORM;
  W.spawn_args = a;
  W.spawn_p = *a.spawn;
  memset(a.report, 0, sizeof(*a.report));
  *a.tot_spawned = 0;
  return GHIP_OK;
}

int ghip_dd_spawn_step(ghip_ctx *ctx)
{
  static const char *who = "ghip_dd wind spawn";
  static_assert(sizeof(SpawnRun) <= sizeof(WindDD::spawn_run), "WindDD::spawn_run holds a SpawnRun");
  DDState &D = ctx->dd;
  WindDD &W = D.wind;
  hipStream_t st = ctx->stream;
  const ghip_wind_spawn_params *p = &W.spawn_p;
  SpawnRun R;
  if(D.phase == 0)
    {
      GHIP_JOIN(ctx);
      memset(&R, 0, sizeof(R));
      // (what fails here is held, not returned: every shard takes the exchange)
      int rc = ghip_winds_enter(ctx, who, true);
      if(rc == GHIP_OK)
        rc = sk_enter(ctx, who, true);
      if(rc == GHIP_OK)
        rc = ghip_rt_need(ctx, ctx->wk, who, true);
      if(rc == GHIP_OK && !(p->rnd_table && p->nrnd > 0))
        rc = ghip_fail(ctx, GHIP_EINVAL, "%s: no RndTable: rnd_table / nrnd must come in the params (ghip_dd_begin "
                       "refuses a table bound with ghip_set_rnd_table)", who);
      if(rc == GHIP_OK && p->MaxPart < ctx->n)
        rc = ghip_fail(ctx, GHIP_EINVAL, "%s: MaxPart = %d is below NumPart = %d", who, p->MaxPart, ctx->n);
      if(rc == GHIP_OK)
        rc = spawn_scan(ctx, p, R);
      if(rc == GHIP_OK)
        rc = spawn_verdict(ctx, p, who, R);
      if(rc != GHIP_OK)
        {
          const std::string why = ctx->err;
          rc = ghip_fail(ctx, GHIP_EINVAL, "%s (rank %d of %d); no shard has changed anything", why.c_str(), D.rank,
                         D.nranks);
          R.counted = 0;
        }
      const bool failed = ghip_dd_hold(ctx, rc);
      memcpy(W.spawn_run, &R, sizeof(R));
      const double mine[4] = {failed ? 0.0 : (double) R.h.total, failed ? 0.0 : (double) R.h.emitting,
                              failed ? 0.0 : R.h.exact_sum, failed ? 1.0 : 0.0};
      GCHK(ghip_ensure(ctx, D.status_own, 32));
      HIPCHK(hipMemcpyAsync(D.status_own.p, mine, 32, hipMemcpyHostToDevice, st));
      HIPCHK(ghip_stream_sync(ctx, st));   // (`mine` lives on this frame)
      ghip_dd_set_allgather(D, D.status_own.p, 32, &D.status_all);
      D.phase = 1;
      return 1;
    }
  if(D.phase == 1)
    {
      memcpy(&R, W.spawn_run, sizeof(R));
      double all[4 * GHIP_MAXRANKS];
      HIPCHK(hipMemcpyAsync(all, D.status_all.p, (size_t) D.nranks * 32, hipMemcpyDeviceToHost, st));
      HIPCHK(ghip_stream_sync(ctx, st));
      int first_failed = -1;
      long long tot = 0;
      for(int r = 0; r < D.nranks; r++)
        {
          if(all[4 * r + 3] != 0 && first_failed < 0)
            first_failed = r;
          tot += (long long) all[4 * r];
        }
      if(first_failed >= 0)   // (GHIP_EINVAL on every shard: what a shard holds back here is an argument error)
        {
          if(D.held.rc != GHIP_OK)
            return ghip_fail(ctx, D.held.rc, "%s", D.held.msg.c_str());
          return ghip_fail(ctx, GHIP_EINVAL, "%s: shard %d cannot create its wind particles (its own message says "
                           "why); every shard stops here, no shard has changed anything", who, first_failed);
        }
      *W.spawn_args.tot_spawned = tot;
      W.spawn_args.report->first_index = R.n;
      GCHK(spawn_grow(ctx, p, R, W.spawn_args.report));
      HIPCHK(ghip_stream_sync(ctx, st));
      return 0;
    }
  return ghip_fail(ctx, GHIP_EINVAL, "ghip_dd_step: the wind spawn has no phase %d", D.phase);
}
