/*
 * ghip.h -- C-ABI of libghip.so: the MI355X (gfx950) force path of GADGET-3 (Leicester fork).
 *
 * Plain C, no C++/torch types.  One ghip_ctx per process / GPU / MPI rank (the reference is
 * single-threaded per rank, SURVEY.md 8b "Threading").  Every entry point returns 0 on success
 * or a negative GHIP_E* code and never calls exit(); the host glue maps a failure to the
 * reference's endrun(code) convention (endrun.c:23-38) -- see INTEGRATION.md.
 *
 * What each group replaces in the reference:
 *   ghip_upload_aos / ghip_download_aos   the lazy reads/writes of P[] / SphP[] inside the walks
 *                                         (allvars.h:1131-1377, 1384-1639)
 *   ghip_tree_build                       force_treebuild()            forcetree.c:67-872
 *   ghip_gravity                          the active-list loop over force_treeevaluate*()
 *                                         gravtree.c:130-168 + forcetree.c:1797, 2330, 2873
 *   ghip_ewald_init                       ewald_init()                 forcetree.c:4402-4527
 *   ghip_density                          density() incl. h iteration  density.c:89-704, 711-1029
 *   ghip_update_hmax                      force_update_hmax()          forcetree.c:1661-1786
 *   ghip_hydro                            hydro_force()                hydra.c:145-813, 822-1995
 *   ghip_peano_hilbert_keys               peano_hilbert_key()          peano.c:300-316
 *   ghip_gravity_finish / _vacuum_energy  OldAcc, *G, Lambda term      gravtree.c:381-403, 470-483
 *   ghip_set_adaptive_gravsoft            -DADAPTIVE_GRAVSOFT_FORGAS   forcetree.c:705-726, 2038-2139
 *   ghip_drift                            drift_particle()             predict.c:129-259
 *   ghip_advance_timesteps / ghip_pm_kick get_timestep, do_the_kick, long-range kick
 *                                                                      timestep.c:29-605
 *   ghip_tree_export                      Nodes[] / Extnodes[] / Nextnode[] / Father[] as
 *                                         force_treebuild leaves them  allvars.h:1847-1916
 *   ghip_pm_periodic                      pmforce_periodic()           pm_periodic.c:199-800
 *   ghip_pm_nonperiodic                   pmforce_nonperiodic(0)       pm_nonperiodic.c:576-1175
 *   ghip_potential                        compute_potential()          potential.c:22-325
 *   ghip_global_quantities                compute_global_quantities_of_system()  global.c:18-238
 *   ghip_find_next_sync_point             find_next_sync_point_and_drift() without its drift  run.c:190-340
 *   ghip_find_extent                      domain_findExtent() of one context   domain.c:1972-2014
 *   ghip_fof                              fof_fof() without group files / SUBFIND   fof.c:94-333
 *   ghip_rearrange                        rearrange_particle_sequence() sfr_eff.c:1018-1129
 *   ghip_peano_order                      peano_hilbert_order()        peano.c:25-185
 * The host-side mirror with the reference's own names (gravity_tree(), density(), hydro_force(),
 * force_treeevaluate(), ...) is include/gadget_force.h.
 */
#ifndef GHIP_H
#define GHIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ghip_ctx ghip_ctx;

/* error codes */
#define GHIP_OK 0
#define GHIP_EHIP (-90001)       /* a HIP runtime call failed (message in ghip_last_error) */
#define GHIP_EINVAL (-90002)     /* bad argument / call order */
#define GHIP_ENOMEM (-90003)     /* device or host allocation failed */
#define GHIP_ENOCONV (-90004)    /* density h-iteration did not converge (reference: endrun(1155)) */
#define GHIP_ENODEVICE (-90005)  /* no usable gfx950 device */
#define GHIP_EDEVICE (-90008)    /* an internal invariant broke on the device (plan overflow, a pruned
                                  * node of an imported tree that a target had to open, ...); results
                                  * of the step must not be used */
#define GHIP_ECOMM (-90009)      /* an RCCL call of the multi-GPU exchange failed */
#define GHIP_EREGION (-90010)    /* non-periodic mesh: a particle lies outside the allowed region; nothing was
                                  * written.  Run ghip_pm_find_region (GHIP_DD_PM_REGION) and call again */
#define GHIP_ETIMESTEP (-90006)  /* timestep criterion failed (reference: endrun(888|818|112313));
                                  * the code is returned by ghip_timestep_endrun_code */

/* particle fields held on the device in the host's particle order.  3-vectors are [n][3]
 * doubles on the host side; ints are 32-bit. */
enum ghip_field
{
  GHIP_F_POS = 0,        /* P[].Pos           [n][3] f64 in  */
  GHIP_F_VEL,            /* P[].Vel           [n][3] f64 in  (node vs/vmax only) */
  GHIP_F_MASS,           /* P[].Mass          [n]    f64 in  */
  GHIP_F_TYPE,           /* P[].Type          [n]    i32 in  */
  GHIP_F_OLDACC,         /* P[].OldAcc        [n]    f64 in/out */
  GHIP_F_HSML,           /* PPP[].Hsml        [n]    f64 in/out (gas entries used) */
  GHIP_F_TIMEBIN,        /* P[].TimeBin       [n]    i32 in  */
  GHIP_F_TI_BEGSTEP,     /* P[].Ti_begstep    [n]    i32 in  */
  GHIP_F_VELPRED,        /* SphP[].VelPred    [ngas][3] f64 in */
  GHIP_F_ENTROPY,        /* SphP[].Entropy    [ngas] f64 in  */
  GHIP_F_DTENTROPY,      /* SphP[].e.DtEntropy [ngas] f64 in (pressure prediction) / out (hydro) */
  GHIP_F_GRAVACCEL,      /* P[].g.GravAccel   [n][3] f64 out */
  GHIP_F_GRAVCOST,       /* P[].GravCost      [n]    i32 out (ninteractions) */
  GHIP_F_NUMNGB,         /* PPP[].n.NumNgb    [ngas] f64 out */
  GHIP_F_DENSITY,        /* SphP[].d.Density  [ngas] f64 in/out */
  GHIP_F_DHSMLFAC,       /* SphP[].h.DhsmlDensityFactor [ngas] f64 in/out */
  GHIP_F_DIVVEL,         /* SphP[].v.DivVel   [ngas] f64 in/out */
  GHIP_F_CURLVEL,        /* SphP[].r.CurlVel  [ngas] f64 in/out */
  GHIP_F_PRESSURE,       /* SphP[].Pressure   [ngas] f64 in/out */
  GHIP_F_HYDROACCEL,     /* SphP[].a.HydroAccel [ngas][3] f64 out */
  GHIP_F_MAXSIGNALVEL,   /* SphP[].MaxSignalVel [ngas] f64 out */
  GHIP_F_TI_CURRENT,     /* P[].Ti_current    [n]    i32 in/out (ghip_drift) */
  GHIP_F_GRAVPM,         /* P[].GravPM        [n][3] f64 out (ghip_pm_periodic; PMGRID builds) */
  GHIP_F_ID,             /* P[].ID            [n]    i32 in  (carried along by the multi-GPU
                          *                                   migration; no kernel reads it) */
  GHIP_F_COUNT
};

/* Byte layout of the host's AoS records (struct particle_data / sph_particle_data are
 * compile-flag dependent, allvars.h:1131-1639; offsets come from a probe TU).
 * An offset of -1 means "field absent".  Hsml/NumNgb live in P when BLACK_HOLES||DUST, else in
 * SphP (the PPP macro, allvars.h:266-270): set exactly one of the two pairs. */
typedef struct
{
  int p_stride, p_pos, p_vel, p_mass, p_gravaccel, p_oldacc, p_gravcost /* f32 */;
  int p_ti_begstep /* i32 */, p_type /* i16 */, p_timebin /* i16 */;
  int p_hsml, p_numngb; /* when PPP == P, else -1 */
  int s_stride, s_entropy, s_pressure, s_velpred, s_maxsignalvel, s_density, s_dtentropy;
  int s_hydroaccel, s_dhsmlfac, s_divvel, s_curlvel;
  int s_hsml, s_numngb; /* when PPP == SphP, else -1 */
  int p_ti_current;     /* i32 */
  int p_gravpm;         /* P[].GravPM (PMGRID builds, allvars.h:1180-1183): uploaded with the records
                           and written back with the gravity results; -1 otherwise */
} ghip_layout;

typedef struct
{
  double ErrTolTheta;        /* All.ErrTolTheta: != 0 Barnes-Hut, == 0 relative criterion */
  double ErrTolForceAcc;     /* All.ErrTolForceAcc */
  double ForceSoftening[6];  /* All.ForceSoftening[] = 2.8 * SofteningTable[] (gravtree.c:881) */
  double BoxSize;            /* All.BoxSize */
  int periodic;              /* built with PERIODIC */
  int unequal_softenings;    /* built with UNEQUALSOFTENINGS */
  double Rcut, Asmth;        /* All.Rcut[0], All.Asmth[0] (PMGRID short-range walk only) */
} ghip_grav_params;

#define GHIP_WALK_NEWTON 0      /* force_treeevaluate                   forcetree.c:1797 */
#define GHIP_WALK_SHORTRANGE 1  /* force_treeevaluate_shortrange        forcetree.c:2330 */
#define GHIP_WALK_EWALD 2       /* force_treeevaluate_ewald_correction  forcetree.c:2873 (adds) */
#define GHIP_WALK_NEWTON_EWALD 3 /* both of gravity_tree's passes of a PERIODIC && !PMGRID build
                                  * (gravtree.c:130-168) in one call: same results as 0 then 2, but
                                  * the two walks share the device (one is bound by fp64 issue, the
                                  * other by the table gathers) */

typedef struct
{
  double DesNumNgb, MaxNumNgbDeviation, MinGasHsml;  /* All.* (density.c:559-646) */
  double BoxSize;
  int periodic;
  int Ti_Current;            /* All.Ti_Current */
  double Timebase_interval;  /* All.Timebase_interval */
  int MaxIter;               /* MAXITER (150) */
} ghip_dens_params;

typedef struct
{
  double ArtBulkViscConst;   /* All.ArtBulkViscConst */
  double BoxSize;
  int periodic;
  int ComovingIntegrationOn;
  double hubble_a2, fac_mu, fac_vsic_fix; /* hydra.c:192-208 (1 when not comoving) */
  double Timebase_interval;
  int raw_dtentropy;         /* 1: leave DtEntropy as hydro_evaluate's raw sum (hydra.c:1934), skip
                              * hydro_force's conversion to dA/dt (hydra.c:583) */
} ghip_hydro_params;

/* drift_particle() for every particle + optional do_box_wrapping() (predict.c:129-259, 282-310) */
typedef struct
{
  int time1;                 /* All.Ti_Current to drift to */
  double Timebase_interval;
  int ComovingIntegrationOn;
  double logTimeBegin, logTimeMax;                          /* driftfac.c:20 */
  const double *DriftTable, *GravKickTable, *HydroKickTable; /* host, 1000 entries each */
  double MinGasHsml;
  int box_wrap;              /* also apply do_box_wrapping() with BoxSize */
  double BoxSize;
  int pmgrid;                /* PMGRID: VelPred += (GravAccel + GravPM) * dt_gravkick (predict.c:181-184) */
} ghip_drift_params;

/* "next" row N1: timestep criterion + kick for the active particles
 * (advance_and_find_timesteps timestep.c:29-362, get_timestep :607-1123 with
 * TypeOfTimestepCriterion 0, do_the_kick :364-605; minimal flag set) */
typedef struct
{
  int Ti_Current;            /* All.Ti_Current */
  double Timebase_interval;
  int ComovingIntegrationOn;
  double Time;               /* All.Time */
  double hubble_a;           /* hubble_function(All.Time) (timestep.c:56); ignored when not comoving */
  double ErrTolIntAccuracy, CourantFac, MaxSizeTimestep, MinSizeTimestep;
  double dt_displacement;    /* find_dt_displacement_constraint (timestep.c:1125) */
  double SofteningTable[6];  /* All.SofteningTable (set_softenings, gravtree.c:839) */
  double MinEgySpec;
  unsigned int TimeBinActive; /* bit b set <=> TimeBinActive[b] (timestep.c:163) */
  double logTimeBegin, logTimeMax;                /* driftfac.c:20 */
  const double *GravKickTable, *HydroKickTable;   /* host, 1000 entries each; comoving only */
  int AdaptiveGravsoftForGasHsml; /* ADAPTIVE_GRAVSOFT_FORGAS + _HSML: the gravity criterion of a
                                     gas particle uses Hsml/2.8 as its softening (timestep.c:740-743) */
  int pmgrid;                /* PMGRID: GRAVPM is added to the acceleration of the gravity criterion
                                (timestep.c:648-652) and VelPred += GravPM * dt_gravkickB (:511-513) */
  double dt_gravkickB;       /* timestep.c:66-72, from All.PM_Ti_begstep / PM_Ti_endstep */
} ghip_kick_params;

/* the long-range kick that ends a PM step (timestep.c:269-345).  The integer-timeline bookkeeping
 * (new PM step, All.PM_Ti_begstep/endstep, :273-300) stays with the host, which passes the two kick
 * factors: dt_gravkick over [mid-point of the old PM step, mid-point of the new one] and the new
 * dt_gravkickB (:296-300).  In/out VEL, VELPRED; in GRAVPM, GRAVACCEL, HYDROACCEL, TIMEBIN,
 * TI_BEGSTEP, TYPE.  ALL particles are kicked, not the active list. */
typedef struct
{
  int Ti_Current;
  double Timebase_interval;
  int ComovingIntegrationOn;
  double logTimeBegin, logTimeMax;
  const double *GravKickTable, *HydroKickTable;   /* host, 1000 entries each; comoving only */
  double dt_gravkick, dt_gravkickB;
} ghip_pmkick_params;

/* "next" row N2: byte offsets of struct NODE / struct extNODE (allvars.h:1847-1916) as the host
 * was compiled; -1 = member absent / not wanted.  Vectors are 3 consecutive doubles. */
typedef struct
{
  int node_stride, n_len, n_center, n_s, n_mass, n_bitflags, n_sibling, n_nextnode, n_father,
    n_ti_current;
  int ext_stride, e_dp, e_vs, e_vmax, e_divvmax, e_hmax, e_ti_lastkicked, e_flag;
  int n_maxsoft;   /* NODE.maxsoft (allvars.h:1857-1860, ADAPTIVE_GRAVSOFT_FORGAS builds only) */
} ghip_node_layout;

/* "next" row N3: periodic particle-mesh long-range force (pmforce_periodic, pm_periodic.c:199) */
typedef struct
{
  int pmgrid;        /* PMGRID (even) */
  double BoxSize;
  double G;          /* All.G: GravPM comes out with G applied, as in the reference (:224) */
  double Asmth;      /* All.Asmth[0] = ASMTH * BoxSize / PMGRID (pm_periodic.c:83) */
} ghip_pm_params;

/* work counters of the last phase, counted exactly as the reference counts them
 * (SURVEY.md 8d): used for roofline.achieved */
typedef struct
{
  long long grav_interactions;   /* sum of ninteractions over targets (forcetree.c:2214) */
  long long grav_targets;
  long long ewald_interactions;  /* sum of cost (forcetree.c:3170) */
  long long dens_neighbours;     /* neighbours with r2 < h2, summed over h-iterations (density.c:856) */
  long long dens_target_evals;   /* target evaluations summed over h-iterations */
  int dens_iterations;
  long long hydro_pairs;         /* pairs passing hydra.c:1266-1269 with r > 0 */
  long long hydro_targets;
  int tree_nodes, gastree_nodes;
  /* device time of the last call of each phase, ms, measured with hipEvents on the ctx stream */
  float ms_tree, ms_grav, ms_ewald, ms_dens, ms_hmax, ms_hydro;
  /* walk efficiency: elements visited summed over wavefronts (64 targets share each visit) */
  long long grav_wave_steps, ewald_wave_steps;
  float ms_kick;                 /* k_advance_timesteps of the last ghip_advance_timesteps */
  float ms_pm;                   /* the last ghip_pm_periodic / ghip_pm_nonperiodic (deposit .. interpolation) */
} ghip_stats;

/* ---- lifetime ---- */
int ghip_create(int device, ghip_ctx **out);
void ghip_destroy(ghip_ctx *ctx);
const char *ghip_last_error(const ghip_ctx *ctx);
const char *ghip_version(void);
/* bytes of device memory the library's contexts of this process hold at the moment (every device
 * allocation of the library is counted): back at its earlier value once a context is destroyed */
long long ghip_device_bytes_in_use(void);

/* ---- particle data ---- */
/* declare particle counts (gas = indices [0,ngas), allvars.h:1384); (re)allocates device arrays.
 *
 * A context is made once and lives through many particle sets (tests/test_gpu_context_reuse.py drives
 * one through changing counts, geometries, walk kinds, meshes and switches and holds every result to a
 * context made for that problem alone).  What a call with CHANGED counts does to the state it finds:
 *   discarded   both trees and the kept geometry of the shards (the next walk or SPH pass needs
 *               ghip_tree_build); the active list (everybody is active again) and the target lists; the
 *               potential of ghip_potential; "GHIP_F_ID has been given" (a bound RndTable needs the IDs of
 *               the new particles before the next build)
 *   refused     values that were given per gas particle or per particle for the old counts -- alpha /
 *   until       Dtalpha (ghip_visc_set_alpha), DragAccel / DeltaDustMomentum (ghip_kick_set_fields, read
 *   given       under integration flags only), DragHeating, Injected_BH_Momentum / RadAccel, the sink
 *   again       marks, the sink table (ghip_sinks_set_table), the wind table (ghip_winds_set_table)
 *               and the candidates of ghip_sfr_cooling:
 *               the pass that reads them fails with GHIP_EINVAL and a message instead of reading
 *               them at another pitch; ghip_tree_substep and ghip_tree_kick_nodes refuse a kept tree
 *               (ghip_set_dynamic_tree) of another particle number until a full build has captured the
 *               new one
 *   undefined   the contents of all 24 fields: a field is [ncomp][count] with pitch count, so the old
 *               bytes mean nothing at the new counts (a buffer that had to grow is zeroed, one that did
 *               not keeps its bytes).  Inputs are set again; an output field holds values only for the
 *               targets of the pass that wrote it since.  The region of ghip_pm_find_region belongs to
 *               the particles it was found for: find or set it again.
 *   kept        every switch and what it was given -- ghip_set_massless_gas_rule,
 *               ghip_set_adaptive_gravsoft, ghip_set_dynamic_tree, ghip_set_rnd_table,
 *               ghip_set_viscosity, ghip_set_dust_model, ghip_set_integration_flags, ghip_set_async,
 *               ghip_set_hydro_release, the shard set-up (ghip_set_shard, ghip_dd_init and the domain,
 *               splits or segments, which a new decomposition sets again); the tables and plans, each
 *               keyed by the one parameter it depends on and remade when a call brings another value
 *               (Ewald force and potential tables: BoxSize; FFT plans and Green's functions: PMGRID; the
 *               short-range tables: none); capacities (buffers only grow), the sort width a clustered
 *               build switched to, the walk plan history and the pair balance -- these change speed and,
 *               for gravity accelerations, the order of a target's partial sums, nothing else.
 * A call with the SAME counts keeps everything, the active list and the trees included (the fields are
 * set again by ghip_set_field, which invalidates the trees where they depend on the field). */
int ghip_set_counts(ghip_ctx *ctx, int numpart, int ngas);
/* copy one field host->device / device->host, host arrays in the plain layouts listed above */
int ghip_set_field(ghip_ctx *ctx, int field, const void *host);
int ghip_get_field(ghip_ctx *ctx, int field, void *host);
/* whole-record path: H2D of the raw P[]/SphP[] blocks + device-side unpack, and the reverse
 * (results are packed into the device image of the records, then one D2H per block) */
int ghip_upload_aos(ghip_ctx *ctx, const void *P, const void *SphP, const ghip_layout *lay,
                    int numpart, int ngas);
/* The same in two calls, for a host that starts the gravity walks before the gas data are across:
 * ghip_upload_aos_particles moves the P[] block (all the gravity tree and its walks read, unless
 * ADAPTIVE_GRAVSOFT_FORGAS needs smoothing lengths that live in SphP[]: refused then), and
 * ghip_upload_aos_gas the SphP[] block -- it does not wait for a GHIP_WALK_NEWTON_EWALD pair in
 * flight and must precede the first SPH call of the step. */
int ghip_upload_aos_particles(ghip_ctx *ctx, const void *P, const ghip_layout *lay, int numpart, int ngas);
int ghip_upload_aos_gas(ghip_ctx *ctx, const void *SphP, const ghip_layout *lay);
int ghip_download_aos(ghip_ctx *ctx, void *P, void *SphP, const ghip_layout *lay,
                      int want_gravity, int want_density, int want_hydro);
/* ghip_download_aos without the wait at its end: the packing kernels and the copies are queued on the
 * library's stream; the arrays are complete after the next synchronising call (ghip_sync). */
int ghip_download_aos_async(ghip_ctx *ctx, void *P, void *SphP, const ghip_layout *lay,
                            int want_gravity, int want_density, int want_hydro);
/* gravity_tree()'s post-pass (ghip_gravity_finish_ex with these arguments) and the gravity fields of
 * the P[] block (ghip_download_aos(..., 1, 0, 0)) in one call that, with a GHIP_WALK_NEWTON_EWALD pair
 * in flight, is ordered after the pair ONLY -- not behind SPH kernels queued underneath it, whose tail
 * the copy then overlaps.  Returns with P[] complete. */
int ghip_gravity_to_records(ghip_ctx *ctx, double G, int pmgrid, double comoving_fac, void *P,
                            const ghip_layout *lay);
/* After ghip_upload_aos / ghip_upload_aos_particles: 1 when a record of the gas block [0, ngas) has a
 * Type other than 0 (a particle converted since the last rearrange_particle_sequence(); the block is
 * gas by allvars.h:1384), else 0.  Lets a host skip its own pass over P[].Type. */
int ghip_gas_block_mixed(ghip_ctx *ctx);
/* Page-lock a host array the record copies go through (the reference allocates P[] / SphP[] once
 * for All.MaxPart, allocate.c:30-60): the copies then run at the link's rate instead of through
 * the runtime's staging buffers.  Optional; a range that cannot be locked is left as it is
 * (returns GHIP_OK, ghip_last_error tells).  ghip_unpin_host before the array is freed;
 * ghip_destroy releases what is left. */
int ghip_pin_host(ghip_ctx *ctx, void *ptr, size_t bytes);
int ghip_unpin_host(ghip_ctx *ctx, void *ptr);

/* ---- active list (FirstActiveParticle/NextActiveParticle, run.c:300-320) ---- */
/* host indices of the active particles; NULL or n == numpart with idx NULL: all active */
int ghip_set_active(ghip_ctx *ctx, const int *idx, int nactive);
/* the list in force, after ghip_set_active and ghip_find_next_sync_point alike: *nactive always, the
 * indices (ascending where the library made the list) if idx != NULL.  With everybody active: numpart
 * and 0 .. numpart-1.  Synchronises. */
int ghip_get_active(ghip_ctx *ctx, int *idx /* may be NULL */, int *nactive);

/* ---- find_next_sync_point_and_drift() without the drift (run.c:190-340), on the resident TIMEBIN ----
 * The bins are recounted on the device (TimeBinCount / TimeBinCountSph, reconstruct_timebins).  For every
 * populated bin n > 0 the next kick is (Ti_Current / 2^n) * 2^n + 2^n, for bin 0 it is Ti_Current; Ti_next is
 * the least of them (run.c:199-219), TIMEBASE = 1 << 29 when no bin is populated.
 *   output_due (run.c:222: Ti_next >= Ti_nextoutput >= 0): the call reports Ti_next = Ti_nextoutput,
 *       TimeBinActive = 0 and both force counts 0, and leaves the active list as it was.  The caller drifts
 *       there with ghip_drift, writes its output (run.c:222-251 stays host code), picks its next output time
 *       and calls again with the same Ti_Current.
 *   otherwise bin 0 is active and bin n > 0 is active when 2^n divides Ti_next (run.c:278-289); the active list
 *       of the context becomes { i : TimeBinActive[TIMEBIN[i]] } in ASCENDING PARTICLE INDEX, for every consumer
 *       of ghip_set_active (target lists, kick, sfr, sink).  The reference chains the list bin-major
 *       (run.c:300-320); no device pass depends on the order of the list -- the target lists are sorted along
 *       the curve, the kick and the cooling act per particle --, only the order in which ghip_sfr_cooling and
 *       ghip_find_smbh report follows it.  When every particle is active the context is in the state of
 *       ghip_set_active(ctx, NULL, 0).
 * The call does not drift: ghip_drift(time1 = out->Ti_next) stays the caller's next call.
 * GHIP_EINVAL, the active list unchanged: NULL arguments; Ti_Current outside [0, TIMEBASE]; a resident
 * TIMEBIN outside [0, 28] (the message names how many; they are not folded into the 32 counters).
 * Host traffic: one blocking read of the 64 counters, one of the list length (with the count of bad bins).
 * On a multi-GPU shard (ghip_dd_init): GHIP_SYNC_POINT_FORM below; a context of ghip_set_shard holds every
 * particle and calls this.  The host mirror libgadget_force.so keeps its own FirstActiveParticle chain. ---- */
typedef struct
{
  int Ti_Current;     /* the sync point just completed: All.Ti_Current on entry of run.c:190 */
  int Ti_nextoutput;  /* All.Ti_nextoutput; < 0: none */
} ghip_sync_params;
typedef struct
{
  int Ti_next;                 /* ti_next_kick_global (run.c:199-219); Ti_nextoutput when output_due */
  int output_due;              /* run.c:222: ti_next_kick_global >= Ti_nextoutput >= 0 */
  unsigned int TimeBinActive;  /* bit b <=> TimeBinActive[b], b in [0, 28] (run.c:278-289); bits 29..31 zero */
  long long NumForceUpdate;    /* this context's active particles */
  long long GlobNumForceUpdate;/* all ranks' (equal to NumForceUpdate on one context) */
  int Flag_FullStep;           /* GlobNumForceUpdate == total particle count (run.c:293) */
  long long TimeBinCount[32], TimeBinCountSph[32];  /* this context's populations */
} ghip_sync_point;
int ghip_find_next_sync_point(ghip_ctx *ctx, const ghip_sync_params *p, ghip_sync_point *out);
/* domain_findExtent (domain.c:1972-2014) over the resident POS of a single context: len = 1.001 *
 * max_j(max_j - min_j), center_j = (min_j + max_j) / 2, corner_j = center_j - len / 2 -- what ghip_tree_build
 * takes, in the operation order of GHIP_DD_DECOMPOSE with find_extent = 1.  GHIP_EINVAL: a coordinate that is
 * not finite, no particle, len == 0; a multi-GPU shard (GHIP_DD_DECOMPOSE finds the cube of all ranks). */
int ghip_find_extent(ghip_ctx *ctx, double corner[3], double center[3], double *len);
/* restrict evaluation to shard `rank` of `nranks` equal-count slices of the space-filling-curve
 * ordered active list (multi-GPU data parallelism; results of other slices are left untouched) */
int ghip_set_shard(ghip_ctx *ctx, int rank, int nranks);

/* shard exchange (multi-GPU; replaces the MPI export rounds gravtree.c:175-339,
 * density.c:193-389, hydra.c:274-526).  group 0 = gravity (width 4), 1 = density (width 7),
 * 2 = hydro (width 5).  ghip_shard_count: padded slice length `per` and this rank's count.
 * ghip_shard_pack writes this rank's finished results as [width][per] doubles into DEVICE memory;
 * the caller all-gathers the equal-sized blocks (RCCL) into [nranks][width][per];
 * ghip_shard_unpack fills in the other ranks' slices. */
int ghip_shard_count(ghip_ctx *ctx, int gas, int *per, int *mine);
int ghip_shard_pack(ghip_ctx *ctx, int group, void *dev_buf);
int ghip_shard_unpack(ghip_ctx *ctx, int group, const void *dev_buf_all, int nranks);

/* ---- multi-GPU: Peano-Hilbert domain decomposition with tree-node / ghost exchange ----
 * One process (or, for tests, one context) per GPU; each holds the particles of ONE contiguous
 * Peano-Hilbert key range (domain.c:100 domain_Decomposition; ranges cut by cumulative work,
 * domain.c:378-384, 1075-1113 -- by the library itself from the resident particles of all ranks:
 * GHIP_DD_DECOMPOSE below, then GHIP_DD_MIGRATE; a host that has all keys in one place may still
 * cut them itself and call ghip_dd_set_splits).  Replaces the top-tree pseudo-particles of force_treebuild
 * (forcetree.c:384-450, 879-1075) and the export rounds of gravity_tree / density / hydro_force
 * (gravtree.c:175-339, density.c:193-389, hydra.c:274-526):
 *   gravity  every shard receives, once per call, the part of every other shard's tree that its
 *            targets can possibly open (a locally essential tree: particles + pruned nodes with
 *            their moments), builds ONE tree over its particles and the imports and walks it --
 *            per target the opening decisions, hence GravCost, equal the single-rank tree's;
 *   SPH      gas particles within the padded search radius of another shard's targets (or whose own
 *            smoothing sphere reaches them) are imported as ghosts before density(); their records
 *            are refreshed once between density() and hydro_force().
 * Results of a shard cover its own (active) particles only; nothing is replicated.
 *
 * An operation is a small state machine, so that the same code serves RCCL (one rank per process)
 * and several logical shards in one process (parity tests on one GPU):
 *   ghip_dd_begin(op)   then   while(ghip_dd_step() == 1) <exchange>
 * where <exchange> is ghip_dd_exchange (this rank's part of a collective over RCCL: ncclAllGather,
 * or ncclAllGather of counts + grouped ncclSend/ncclRecv) or ghip_dd_exchange_local (all shards of
 * one process at once, device-to-device copies).  ghip_dd_run = the whole loop over RCCL. */
#define GHIP_DD_MIGRATE 1    /* params: NULL.  Particles that drifted out of their shard's key range
                              * move to the shard that owns them, with every resident field
                              * (domain_exchange, domain.c:665-1060); numpart / ngas of the
                              * contexts change, gas stays in front.  Run after ghip_drift. */
#define GHIP_DD_GRAVITY 2    /* params: ghip_grav_params, walk: GHIP_WALK_*; tree build included */
#define GHIP_DD_DENSITY 3    /* params: ghip_dens_params; needs the gravity tree of this step */
#define GHIP_DD_HYDRO 4      /* params: ghip_hydro_params; after GHIP_DD_DENSITY + ghip_update_hmax */
int ghip_dd_init(ghip_ctx *ctx, int rank, int nranks);
/* the global domain cube (identical on all ranks: the all-reduced extent of domain_findExtent,
 * domain.c:1972-2014) and All.ForceSoftening -- what ghip_tree_build takes in a single-GPU run */
int ghip_dd_set_domain(ghip_ctx *ctx, const double DomainCorner[3], const double DomainCenter[3],
                       double DomainLen, const double ForceSoftening[6]);
/* nranks+1 Peano-Hilbert keys (21 bits per dimension): rank r owns [splits[r], splits[r+1]);
 * splits[0] = 0, splits[nranks] = 2^63.  Every resident particle must lie in its rank's range
 * (unless ghip_dd_set_guests allows guests). */
int ghip_dd_set_splits(ghip_ctx *ctx, const unsigned long long *splits);
/* The general form, for decompositions in which a rank owns several pieces of the curve
 * (-DMULTIPLEDOMAINS > 1, domain.c:482-494, 1158-1215: DomainTask[] per top-leaf): nseg segments
 * [keys[s], keys[s+1]) in key order with owner[s]; keys[0] = 0, keys[nseg] = 2^63.  Neighbouring
 * segments of one owner are merged.  A tree cell is "wholly this rank's" when it lies inside ONE of
 * its pieces; everything else works as for one range per rank (the target groups of a rank then
 * span its pieces, which only makes their boxes less compact). */
int ghip_dd_set_segments(ghip_ctx *ctx, int nseg, const unsigned long long *keys, const int *owner);
/* Peano-Hilbert keys of the resident particles (host array of numpart entries) */
int ghip_dd_keys(ghip_ctx *ctx, unsigned long long *keys_host);
/* domain_findSplit_work_balanced (domain.c:1075-1113, equal speed factors): cut ndomain
 * curve-ordered pieces of work into ncpu contiguous ranges [start[i], end[i]].  Host arithmetic. */
int ghip_dd_find_split(int ncpu, int ndomain, const double *domainWork, int *start, int *end);
/* search radii are padded by this factor when ghosts are first selected in a density() (default
 * 1.3).  Only a performance knob: when the h iteration takes a smoothing length beyond the padded
 * radius on any shard, all shards restore their starting Hsml, select ghosts again with
 * 1.26 x the worst growth seen and repeat the iteration (a collective decision). */
int ghip_dd_set_ghost_margin(ghip_ctx *ctx, double margin);
/* Guests.  A resident particle whose key lies outside every piece of the curve its shard owns is a GUEST of
 * that shard; the shard that owns the key is its HOST.  A run that does not migrate before every force
 * computation has them: the reference decomposes only every TreeDomainUpdateFrequency * TotNumPart force
 * computations (domain.c:115-135) and in between a particle stays in the memory of the rank that holds it.
 *   on = 0 (default)  every resident particle must lie in its shard's pieces: one that does not ends
 *          GHIP_DD_GRAVITY and GHIP_DD_POTENTIAL on all shards (device invariant 2, value 5) -- the host
 *          runs GHIP_DD_MIGRATE (or its own domain_exchange) before every call.
 *   on = 1 guests are legal in GHIP_DD_GRAVITY and GHIP_DD_POTENTIAL, and so in the SPH, sink and dust
 *          operations that follow them: results equal the single global tree of the current positions,
 *          interaction and neighbour counts bit for bit.  The rule: a host may send a cell as ONE pruned
 *          element only if its local moments are the cell's global moments, so a cell whose key range holds
 *          the key of a guest held elsewhere is descended like a cell shared between shards.  Every shard
 *          counts its guests (the count travels in the status record behind its group table); when any shard
 *          holds one, one more exchange precedes the selection -- an all-to-all-v of 8-byte keys, each guest's
 *          key to its host only; when nobody holds one, nothing more is exchanged than with on = 0.
 * Set the same value on every rank (a collective setting, like the key ranges).  Invalidates nothing.
 * A particle outside the domain cube stays an error (6).  GHIP_DD_MIGRATE and GHIP_DD_DECOMPOSE are
 * unchanged: guests are what they exist to move. */
int ghip_dd_set_guests(ghip_ctx *ctx, int on);
/* out[0]: guests resident on this shard in its last GHIP_DD_GRAVITY / GHIP_DD_POTENTIAL, out[1]: guest keys
 * it received as their host (both 0 with the mode off) */
int ghip_dd_guest_counts(const ghip_ctx *ctx, long long out[2]);
/* RCCL: rank 0 creates the id (128 bytes) and the host broadcasts it (MPI_Bcast in the reference's
 * world); every rank then connects.  The library binds the librccl that sits next to the HIP
 * runtime the process uses (ghip_dd_rccl_library tells which). */
int ghip_dd_rccl_unique_id(void *id128);
int ghip_dd_rccl_connect(ghip_ctx *ctx, const void *id128);
const char *ghip_dd_rccl_library(void);
int ghip_dd_begin(ghip_ctx *ctx, int op, const void *params, int walk);
/* 1: exchange pending, 0: done, < 0: error.  A step that returns <= 0 ends the operation, complete or failed:
 * a further ghip_dd_step without a new ghip_dd_begin fails with "no operation in progress". */
int ghip_dd_step(ghip_ctx *ctx);
int ghip_dd_exchange(ghip_ctx *ctx);             /* RCCL */
int ghip_dd_exchange_local(ghip_ctx **ctxs, int nranks);
/* the pending exchange staged through host memory and the CALLER's all-gather of equal-sized
 * blocks (recv = [nranks][bytes]; return 0) -- MPI_Allgather for a host whose ranks have no RCCL
 * between them; also the only way to rehearse several ranks on ONE GPU.  Slow by construction. */
int ghip_dd_exchange_host(ghip_ctx *ctx,
                          int (*allgather)(void *user, const void *send, size_t bytes, void *recv),
                          void *user);
int ghip_dd_run(ghip_ctx *ctx, int op, const void *params, int walk);
/* out[0..10]: rank, nranks, elements imported into the gravity tree, elements sent, ghosts
 * imported, ghosts sent, bytes sent by the last gravity / density operation, largest Hsml growth
 * of the last density (x 1e6), elements of the gravity / gas tree */
int ghip_dd_get_info(const ghip_ctx *ctx, long long out[16]);

/* ---- pre-condition of the path: drift the resident particles (replaces the lazy
 * drift_particle() calls inside the walks, forcetree.c:1911, ngb.c:57) ---- */
int ghip_drift(ghip_ctx *ctx, const ghip_drift_params *p);

/* ---- "next" row N1: timestep + kick on the resident fields.  Works on the active list of
 * ghip_set_active.  In/out: VEL, VELPRED, ENTROPY, DTENTROPY, TIMEBIN, TI_BEGSTEP; in: GRAVACCEL
 * (final, xG), HYDROACCEL, HSML, MAXSIGNALVEL, DENSITY, TYPE.  TimeBinCount/TimeBinCountSph
 * (32 entries each, may be NULL) receive the recounted bin populations (allvars.h:337-338).
 * Returns GHIP_ETIMESTEP where the reference calls endrun(); ghip_timestep_endrun_code gives the
 * reference's code (888, 818, 112313).  With both arrays NULL the bins are not recounted
 * (ghip_timebin_counts does it on demand) and, under ghip_set_async, the call does not wait. ---- */
int ghip_advance_timesteps(ghip_ctx *ctx, const ghip_kick_params *p, long long *TimeBinCount,
                           long long *TimeBinCountSph);
int ghip_timestep_endrun_code(const ghip_ctx *ctx);
/* ---- the integrator of the shipped flag bundle (-DDUST -DDUST_TIMESTEP -DBLACK_HOLES
 * -DACCRETION_RADIUS -DVIRTUAL): the type rules of get_timestep, do_the_kick and drift_particle
 * (timestep.c:364-947, predict.c:129-259), for ghip_advance_timesteps and ghip_drift alike.
 *   gas     criterion + fac2 DragAccel (timestep.c:673-677); dust_timestep: DeltaDustMomentum /
 *           Mass / dt joins the acceleration and dt = min(dt, dt_new) (:710-722, nothing when the
 *           new acceleration is 0); the kick sets DragAccel = 0 (:508); the drift adds
 *           DragAccel dt_hydrokick to VelPred (predict.c:195-198)
 *   Type 2  half the gravity step (:725-726), no gravity kick (:410-418; dust_drag has integrated
 *           the grain's velocity); a kept tree still gets its (zero) kick
 *   Type 3  step <= min(0.03 OuterBoundary / C UnitVelocity_in_cm_per_s FeedBackVelocity, 1)
 *           (:887-897, C = 2.9979e10); no kick, no drift (:375-377, predict.c:134-136) -- TimeBin and
 *           Ti_begstep advance
 *   Type 5  step <= 0.03 OuterBoundary / 100, and with accretion_radius
 *           <= AccDtBlackHole (InnerBoundary | SinkBoundary + Hsml / 2)^1.5 / Mass^0.5 (:908-947);
 *           Hsml is the resident HSML at the sink's index (ghip_sink_density writes it there)
 * Switches that are 0 take no part; f == NULL restores the minimal flag set (the default kernels).
 * Works on every kind of context (single, ghip_set_shard, ghip_dd_*). ---- */
typedef struct
{
  int dust, dust_timestep, black_holes, accretion_radius, virtual_particles;
  double OuterBoundary, AccDtBlackHole, SMBHmass, InnerBoundary, SinkBoundary;
  double FeedBackVelocity, UnitVelocity_in_cm_per_s;
} ghip_integration_flags;
int ghip_set_integration_flags(ghip_ctx *ctx, const ghip_integration_flags *f);
/* the per-particle inputs of those rules, resident next to the GHIP_F_* fields and zero until set:
 * gas SphP[].da.DragAccel [ngas][3] (in/out: the kick resets it), gas P[].DeltaDustMomentum
 * [ngas][3], P[].NewDensity [n] (kept; with VIRTUAL the reference reads it only to divide by an
 * uninitialised rho, the device takes dt_ff = 1 -- DESIGN 4.6).  NULL = zero.  Values set for one
 * ngas are refused after ghip_set_counts changes it.  Single-rank contexts only: a non-NULL field
 * on a sharded or multi-GPU context is GHIP_EINVAL. */
int ghip_kick_set_fields(ghip_ctx *ctx, const double *drag_accel, const double *gas_dust_momentum,
                         const double *new_density);
int ghip_kick_get_drag_accel(ghip_ctx *ctx, double *drag_accel);
/* the three arrays of ghip_kick_set_fields as the context holds them: held[k] = 1 when array k is held for the
 * current counts (it then lands in its host array, layouts as above; NULL = skip), else 0 and nothing is written */
int ghip_kick_get_fields(ghip_ctx *ctx, double *drag_accel, double *gas_dust_momentum, double *new_density,
                         int held[3]);
/* the bin populations after the last ghip_advance_timesteps, recounted over all particles
 * (reconstruct_timebins, predict.c:14-127); synchronises */
int ghip_timebin_counts(ghip_ctx *ctx, long long *TimeBinCount, long long *TimeBinCountSph);
int ghip_pm_kick(ghip_ctx *ctx, const ghip_pmkick_params *p);
/* per-type sums of find_dt_displacement_constraint (timestep.c:1140-1156): sum of |v|^2, smallest
 * positive mass (1e30 if none), particle count -- 6 entries each */
int ghip_velocity_moments(ghip_ctx *ctx, double v2sum[6], double min_mass[6], long long count[6]);
/* pack the kick's results (Vel, TimeBin, Ti_begstep; VelPred, Entropy, DtEntropy) into the device
 * image of the records and copy the blocks to the host */
int ghip_download_aos_kick(ghip_ctx *ctx, void *P, void *SphP, const ghip_layout *lay);

/* ---- "next" row N2: export the device-built gravity tree in the reference's representation
 * (what force_treebuild + force_update_node_recursive leave behind, forcetree.c:67-872): record k
 * of Nodes_base / Extnodes_base is node MaxPart + k (the root is node MaxPart), Nextnode[] and
 * Father[] are filled for the particles [0, numpart).  Needs a built tree and the VEL, HSML,
 * DIVVEL, TYPE fields (for vs, vmax, hmax, divVmax).  Single-rank semantics: no TOPLEVEL /
 * pseudo-particle entries. ---- */
int ghip_tree_export(ghip_ctx *ctx, const ghip_node_layout *lay, int MaxPart, int Ti_Current,
                     int unequal_softenings, void *Nodes_base, void *Extnodes_base, int *Nextnode,
                     int *Father, int max_nodes, int *numnodes);

/* ---- "next" row N3: P[].GravPM = long-range force of all particles on a PMGRID^3 periodic mesh
 * (replaces long_range_force() -> pmforce_periodic(), longrange.c / pm_periodic.c:199-800; the
 * field is zeroed first as long_range_force does).  Pairs with GHIP_WALK_SHORTRANGE. ---- */
int ghip_pm_periodic(ghip_ctx *ctx, const ghip_pm_params *p);

/* ---- the non-periodic particle-mesh force of TreePM with open boundaries (PMGRID without PERIODIC:
 * pm_nonperiodic.c, mesh 0; no PLACEHIGHRESREGION, SCALARFIELD, ENLARGEREGION; GRIDBOOST 2).  The FFT mesh
 * is GRID^3 = (2 PMGRID)^3, zero padded; the particles occupy cells [2, GRID/2 - 2) of its lower octant.
 *
 * The region (pm_init_regionsize, :91-212): the extremes of the resident positions are reduced on the device,
 * the arithmetic of :123-159 runs on the host in double, operation for operation, and the result is stored
 * in the context.  ghip_pm_find_region returns GHIP_EINVAL, nothing stored, for: no particle, a position that
 * is not finite, an extent of zero (one particle, or all coincident), an odd pmgrid or one outside [8, 512].
 * Not on a multi-GPU shard (GHIP_EINVAL): there GHIP_DD_PM_REGION (below) gives every rank the same bytes.
 * ghip_pm_set_region stores a region the host kept (All.Xmintot, All.Corner ... of a restart) after checking
 * that it places [Xmintot, Xmaxtot] into cells [2, GRID/2 - 2); ghip_pm_get_region returns the region in
 * force (GHIP_EINVAL: none).  The walk's Asmth / Rcut are the region's.  The Green's function table
 * (pm_setup_nonperiodic_kernel, :371-558) is built on the device by the first call that needs it; it depends
 * on PMGRID only, so a new region of the same pmgrid keeps it. ---- */
typedef struct
{
  int pmgrid;                       /* PMGRID; the FFT mesh is (2 PMGRID)^3 */
  double Xmintot[3], Xmaxtot[3];    /* allowed region, symmetrised (:130-135) */
  double TotalMeshSize;             /* :144 */
  double Corner[3], UpperCorner[3]; /* :152-153 */
  double Asmth, Rcut;               /* ASMTH * TotalMeshSize / GRID, RCUT * Asmth (:158-159), ASMTH 1.25, RCUT 4.5 */
} ghip_pm_region;
int ghip_pm_find_region(ghip_ctx *ctx, int pmgrid, ghip_pm_region *out);   /* out may be NULL */
int ghip_pm_set_region(ghip_ctx *ctx, const ghip_pm_region *r);
int ghip_pm_get_region(const ghip_ctx *ctx, ghip_pm_region *out);
/* P[].GravPM = pmforce_nonperiodic(0) (:576-1175) and the tail of long_range_force (longrange.c:117-138:
 * comoving: += 0.5 Hubble^2 Omega0 Pos, else += OmegaLambda Hubble^2 Pos), the field zeroed first.  Needs a
 * region of the same pmgrid (GHIP_EINVAL otherwise).  A particle outside [Xmintot, Xmaxtot] -- or with a
 * coordinate that is not a number -- makes the call return GHIP_EREGION and write NOTHING, not even the zeros
 * (the reference returns 1, :646): run ghip_pm_find_region and call again, as long_range_force does (:88-96),
 * and build the tree again afterwards as the reference does (:1170).  The range check is one device pass into
 * an error word; no position is read on the host.  It allows 4 DBL_EPSILON max(|Xmintot|, |Xmaxtot|) along each
 * axis: the symmetrisation of :133-134 can round a bound one unit in the last place inside the particle that
 * defines the extent, which the reference then refuses for good (endrun(68687)).  Cells of the force mesh that the reference leaves unwritten
 * (outside [2, GRID/2 - 2)) are zero.  fp64 atomic adds in the mass assignment: reproducible to rounding, not
 * bitwise.  ms_pm of ghip_get_stats reports the call.  Pairs with GHIP_WALK_SHORTRANGE at periodic = 0, Rcut
 * and Asmth from the region.  Not on a multi-GPU shard: GHIP_DD_PM_NONPERIODIC.  n = 0: GHIP_OK. */
typedef struct
{
  int pmgrid;
  double G;          /* All.G */
  int comoving;      /* All.ComovingIntegrationOn */
  double Omega0, OmegaLambda, Hubble;
} ghip_pmnp_params;
int ghip_pm_nonperiodic(ghip_ctx *ctx, const ghip_pmnp_params *p);

/* ---- compute_potential() (potential.c:22-325): the potential of EVERY particle of the context from a
 * walk of the tree the gravity walks would use now (the tree of the last ghip_tree_build, or the kept
 * tree after ghip_tree_substep when ghip_set_dynamic_tree is on; the caller drifts first), then the
 * reference's finish: + Mass / SofteningTable[type] (the self term, which adaptive gas softening does
 * not cancel), comoving periodic runs - 2.8372975 m^(2/3) (Omega0 3 H^2 / (8 pi G))^(1/3), * G,
 * pm.pmgrid > 0: + the periodic PM potential (pmpotential_periodic, pm_periodic.c:808-1195; the walk is
 * then the short-range one, grav.Rcut / Asmth), and -1/2 Omega0 H^2 r^2 (comoving, not periodic) or
 * -1/2 OmegaLambda H^2 r^2 (physical).  grav.periodic without a mesh adds the Ewald potential
 * correction to every interaction (forcetree.c:3514).  Reads POS, MASS, TYPE, OLDACC (relative
 * criterion) and, with adaptive softening, the HSML the tree was built with.  The result stays in a
 * per-context buffer (ghip_get_potential); no GHIP_F_* field changes.  Not on a multi-GPU shard
 * (GHIP_EINVAL): domain-decomposed shards run the collective GHIP_DD_POTENTIAL (below).  pm.G is the mesh part's G (All.G, as for ghip_pm_periodic); pm.BoxSize must equal
 * grav.BoxSize.  grav.periodic == 0 with pm.pmgrid > 0: the short-range walk without nearest images plus the
 * NON-PERIODIC mesh potential (pmpotential_nonperiodic(0), pm_nonperiodic.c:1354-1750, with the fac of :1378
 * applied): a region must be set (ghip_pm_find_region), pm.pmgrid == region.pmgrid, grav.Asmth == pm.Asmth ==
 * region.Asmth, grav.Rcut == region.Rcut; pm.BoxSize is not read.  A particle outside the region: GHIP_EREGION,
 * no potential written.  Every argument is checked before anything runs. ---- */
typedef struct
{
  ghip_grav_params grav;     /* opening criterion, softenings, BoxSize, periodic, Rcut / Asmth */
  ghip_pm_params pm;         /* pm.pmgrid = 0: no mesh */
  double G;                  /* All.G */
  double SofteningTable[6];  /* All.SofteningTable (the self term) */
  int comoving;              /* All.ComovingIntegrationOn */
  double Omega0, OmegaLambda, Hubble;
} ghip_pot_params;
int ghip_potential(ghip_ctx *ctx, const ghip_pot_params *p);
/* P[].p.Potential [n] f64, host order */
int ghip_get_potential(ghip_ctx *ctx, double *host);
/* interactions of the last walk: summed over the targets and the largest per target */
int ghip_potential_interactions(ghip_ctx *ctx, long long *sum, long long *maxval);
/* ... and per target [n], host order (a single context, or a shard after GHIP_DD_POTENTIAL) */
int ghip_get_potential_interactions(ghip_ctx *ctx, long long *host);
/* potcorr[65][65][65] of ewald_init, already divided by BoxSize (tests) */
int ghip_ewald_get_pot_table(ghip_ctx *ctx, double BoxSize, double *host);

/* ---- compute_global_quantities_of_system() (global.c:18-238), the per-type sums before the
 * MPI_Reduce: velocities predicted to Ti_Current with the grav / hydro kick factors (+ HydroAccel of gas,
 * + GravPM dt_gravkick_pm under PMGRID), entropies with DtEntropy, EnergyPotComp from the potential of
 * the last ghip_potential (0 when there is none for the current particle set).  Reads POS, VEL, MASS,
 * TYPE, TIMEBIN, TI_BEGSTEP, GRAVACCEL, (PMGRID) GRAVPM, (gas) HYDROACCEL, ENTROPY, DTENTROPY, DENSITY.
 * The potential is p->Potential when given, else that of the last ghip_potential -- which holds only
 * while POS, MASS, TYPE and the particle counts are unchanged since (ghip_set_field, ghip_set_counts, the
 * uploads and ghip_drift discard it): call ghip_potential on the current state first.
 * Domain-decomposed shards run the collective GHIP_DD_GLOBAL_QUANTITIES (below); this call returns
 * GHIP_EINVAL there.
 * Deterministic: fixed-order partial sums, no atomics.  The totals (sys.EnergyKin = sum of the
 * components, ...) are the host's. ---- */
typedef struct
{
  int Ti_Current;
  double Timebase_interval;
  int ComovingIntegrationOn;
  double Time;                                    /* All.Time (a1, a2, a3 of global.c:26-36) */
  double logTimeBegin, logTimeMax;                /* driftfac.c:20 */
  const double *GravKickTable, *HydroKickTable;   /* host, 1000 entries each; comoving only */
  int pmgrid;                                     /* PMGRID build: vel += GravPM dt_gravkick_pm */
  double dt_gravkick_pm;                          /* global.c:96-103, from All.PM_Ti_begstep / endstep */
  const double *OldPhotonMomentum;                /* VIRTUAL: P[].OldPhotonMomentum [n], host; NULL = absent */
  double rad_fac;                                 /* C / All.UnitVelocity_in_cm_per_s */
  const double *Potential;                        /* P[].p.Potential [n], host; NULL = the result of the last
                                                     ghip_potential */
} ghip_global_params;
typedef struct
{
  double MassComp[6], EnergyKinComp[6], EnergyPotComp[6], EnergyIntComp[6];
  double MomentumComp[6][4], AngMomentumComp[6][4], CenterOfMassComp[6][4];   /* [3] stays 0 */
  double EnergyRadComp;                           /* VIRTUAL: Type 3, Mass != 0 */
} ghip_global_sums;
int ghip_global_quantities(ghip_ctx *ctx, const ghip_global_params *p, ghip_global_sums *out);

/* ---- "next" row N4: sink (black-hole) neighbour passes and the per-particle part of
 * cooling_and_starformation, for the reference's shipped flag bundle (BLACK_HOLES, SWALLOWGAS,
 * ACCRETION_RADIUS, ACCRETION_DENSITY, ACCRETION_OF_DUST_ONLY, BH_MERGERS_WITHIN_H,
 * BH_THERMALFEEDBACK + TMP_FEEDBACK, DUST, COOLING, SFR, BH_FORM).  The sinks are given by their
 * particle indices; their per-sink state (ID, Mdot, BH_Density, BH_Mass ...) travels in small host
 * arrays, the victims' marks (P[].SwallowID, SphP[].i.Injected_BH_Energy) are resident.  A host
 * with a resident run keeps the per-sink state in the resident sink table instead ("the sinks on the
 * resident state" below): ghip_sinks_density, ghip_blackhole_accretion (the whole of
 * blackhole_accretion(), blackhole.c:70-791, scalar bookkeeping included) and ghip_sfr_form_sinks (the
 * conversion of a flagged gas particle into a sink, sfr_eff.c:602-629; only the GSL stream stays with
 * the host) then need no per-sink host array.  The cooling
 * function (DoCooling, cooling.c) runs on the device in ghip_sfr_cooling below.  On a multi-GPU shard the neighbour passes run through GHIP_DD_SINK_DENSITY /
 * GHIP_DD_BH_EVALUATE / GHIP_DD_BH_SWALLOW below. ---- */
typedef struct
{
  double BoxSize;
  int periodic;
  double ascale;            /* All.Time when comoving, else 1 (blackhole.c:89-95) */
  double dt_fac;            /* All.Timebase_interval / hubble_a (:822) */
  double SMBHmass, InnerBoundary, SinkBoundary, SofteningBndry;   /* All.* */
  double CritDensity;       /* All.CritOverDensity * UnitLength_in_cm^3 / UnitMass_in_g (:1099) */
  double FeedbackCoeff;     /* All.BlackHoleFeedbackFactor * 6.67e-8 * pow(4.*3.1415/3.*5., 0.3333)
                               / All.UnitEnergy_in_cgs (:1138-1139) */
  double UnitMass_in_g;
  int dust;                   /* -DDUST */
  int accretion_of_dust_only; /* -DACCRETION_OF_DUST_ONLY */
  int accretion_density;      /* -DACCRETION_DENSITY */
} ghip_bh_params;
/* density() for Type-5 targets (density.c BLACK_HOLES branches): h iteration against the gas tree
 * for DesNumNgb * ngb_factor (All.BlackHoleNgbFactor) neighbours.  hsml [nsink] in/out (also
 * written to the resident HSML field); numngb, bh_density, bh_entropy [nsink], bh_gasvel
 * [nsink][3].  Needs the tree of this step. */
int ghip_sink_density(ghip_ctx *ctx, const ghip_dens_params *p, double ngb_factor, int nsink,
                      const int *sink_idx, double *hsml, double *numngb, double *bh_density,
                      double *bh_entropy, double *bh_gasvel, int *iterations);
/* P[].SwallowID = 0, Injected_BH_Energy = 0 for all particles (start of blackhole_accretion) */
int ghip_sink_reset(ghip_ctx *ctx);
/* blackhole_evaluate (blackhole.c:794-1190): marks the victims (SwallowID = ID of the sink; a
 * victim claimed by several sinks goes to the largest ID) and spreads the feedback energy.
 * Reads POS, VEL, MASS, HSML, TIMEBIN, TYPE and the gas DENSITY from the resident fields. */
int ghip_blackhole_evaluate(ghip_ctx *ctx, const ghip_bh_params *p, int nsink, const int *sink_idx,
                            const unsigned int *sink_id, const double *bh_mdot,
                            const double *bh_density);
/* blackhole_evaluate_swallow (blackhole.c:1201-1346): per sink the accreted mass, BH mass, dust
 * mass [nsink] and momentum [nsink][3]; the victims' resident MASS becomes 0 (a tree built before
 * is stale afterwards), sink_bh_mass [nsink] (P[].BH_Mass of the sinks, in/out) becomes 0 for a
 * swallowed sink; counts = gas / sinks / dust swallowed.
 * blackhole_accretion() runs this pass only for a sink that nobody claimed in the marking pass
 * (blackhole.c:528-532: `if(P[i].Type == 5) if(P[i].SwallowID == 0) blackhole_evaluate_swallow(i, ...)`).
 * So a sink whose own resident SwallowID is not 0 swallows nothing here: the particles marked with
 * its ID keep their mass, and its five sums are 0 (what they hold in the reference after :713).
 * "Swallowed" therefore means: marked by a sink that is itself unmarked. */
int ghip_blackhole_swallow(ghip_ctx *ctx, const ghip_bh_params *p, int nsink, const int *sink_idx,
                           const unsigned int *sink_id, double *sink_bh_mass, double *acc_mass,
                           double *acc_bhmass, double *acc_dustmass, double *acc_momentum,
                           long long counts[3]);
/* the resident marks: SwallowID [numpart] (u32), Injected_BH_Energy [ngas]; NULL = skip */
int ghip_sink_get_marks(ghip_ctx *ctx, unsigned int *swallow_id, double *injected_energy);
int ghip_sink_set_marks(ghip_ctx *ctx, const unsigned int *swallow_id, const double *injected_energy);
/* cooling_and_starformation (sfr_eff.c:82-947), per active gas particle (ghip_set_active), with the
 * cooling function as identity (kept as it is; ghip_sfr_cooling below is the complete pass):
 * flag_sink_host [ngas] = 1 where the particle qualifies for
 * conversion into a sink (:226-229), else the isochoric update of DTENTROPY incl. the injected
 * black-hole energy (:486-531, 582-594).  Non-comoving. */
int ghip_cooling_and_starformation(ghip_ctx *ctx, double Timebase_interval,
                                   double CritPhysDensity_code, double MinEgySpec,
                                   double u_to_temp_fac, int *flag_sink_host);

/* ---- cooling_and_starformation with the cooling function and the dust drag heating
 * (sfr_eff.c:183-597 + DoCooling, cooling.c:82-300), per active particle in active-list order
 * (ghip_set_active), for the shipped bundle (COOLING, SFR, DUST, BH_FORM, FIND_SMBH,
 * EVAPORATION_RADIAL, CONSTANT_MEAN_MOLECULAR_WEIGHT) and its sibling closed forms.  The TREECOOL
 * network (cooling.c:459-567) is compiled out under CONSTANT_MEAN_MOLECULAR_WEIGHT and not built. ---- */
enum
{
  GHIP_COOL_NONE = 0,            /* u returned unchanged (also -DADIABATIC without sub-flags) */
  GHIP_COOL_ISOTHERM,            /* u = EqTemp / u_to_temp_fac (cooling.c:170-173) */
  GHIP_COOL_EVAPORATION,         /* tcool = BetaCool (1 + (rho / Evap_dens)^5) (:175-183) */
  GHIP_COOL_EVAPORATION_RADIAL,  /* u_eq / (r^Cool_ind + 1e-10), (rho / Evap_dens)^rho_cool_ind (:185-192; shipped) */
  GHIP_COOL_BETA                 /* u_eq / (r^0.5 + 1e-10), tcool = BetaCool r^1.5 (:196-198, 282);
                                    beta_tapper_off: tcool *= 1 + (rho / 1e-10)^2 (:218-222) */
};
typedef struct
{
  int cooling;              /* GHIP_COOL_* */
  int beta_tapper_off;      /* -DBETA_COOLING_TAPPER_OFF (GHIP_COOL_BETA only) */
  int dust;                 /* -DDUST: spend the resident DragHeating (sfr_eff.c:481-499) */
  int comoving;             /* All.ComovingIntegrationOn */
  double Timebase_interval; /* All.Timebase_interval */
  double Time, hubble_a;    /* All.Time, hubble_function(All.Time) (comoving only): a3inv = 1 / Time^3,
                               dtime = Time dt / (Time hubble_a) (sfr_eff.c:145-156, 191-196) */
  double CritPhysDensity_code;  /* All.CritPhysDensity * UnitLength_in_cm^3 / UnitMass_in_g (:226-229) */
  double MinEgySpec, OriginalGasMass;
  double MeanWeight, UnitEnergy_in_cgs, UnitMass_in_g, UnitDensity_in_cgs;
  double EqTemp, BetaCool, Cool_ind, rho_cool_ind, Evap_dens;   /* All.* of cooling.c */
  double smbh_pos[3];       /* All.xbh, ybh, zbh (ghip_find_smbh); the origin when FIND_SMBH is off */
} ghip_sfr_params;
/* For each active particle, in active-list order: an active Type-2 grain with Mass <= 1e-5
 * OriginalGasMass gets Mass = 0 in the resident MASS (:185-187); an active gas particle is a sink
 * candidate when Density >= CritPhysDensity_code and Mass != 0 (:226-229, 459-462), else
 *   unew = max(MinEgySpec, (A + dA/dt dt) / (gamma-1) (rho a3inv)^(gamma-1))       (:486-488)
 *        + DragHeating / Mass dt, DragHeating = 0 (dust; neither when Mass == 0)  (:481-499)
 *        + Injected_BH_Energy / Mass, 5e9 K ceiling, the injection consumed       (:502-524)
 *   unew = DoCooling(unew, rho a3inv, dtime, r2)  with r2 = |Pos - smbh_pos|^2 (not wrapped)
 *   dA/dt = (unew (gamma-1) / (rho a3inv)^(gamma-1) - A) / dt, floor -A / (2 dt)  (:572-595)
 * Reads POS, MASS, TYPE, TIMEBIN, DENSITY, ENTROPY, DTENTROPY, the resident Injected_BH_Energy and
 * (dust) DragHeating -- zero when it was never set.  Writes DTENTROPY, MASS (grains), the two marks.
 * *ncand = the number of candidates; cand_idx [*ncand] (NULL: count only) their particle indices in
 * active-list order (a stable device compaction: the host reads ncand ints, not ngas).  NULL params or
 * an unknown cooling: GHIP_EINVAL; so is dust = 1 on a replicated shard (ghip_set_shard) and on a
 * multi-GPU shard that holds no DragHeating (neither GHIP_DD_DUST_DRAG nor ghip_dust_set_drag_heating
 * has created it there).  Otherwise a shard runs the pass on its own particles. */
int ghip_sfr_cooling(ghip_ctx *ctx, const ghip_sfr_params *p, int *ncand, int *cand_idx);
/* the position part of FindQuasars (blackhole.c:1481-1530): over the active particles, pos = the
 * position of the LAST one in active-list order with Type 5 and Mass > 0.9 SMBHmass (the origin if
 * none), *count = how many there are.  Across ranks the host adds pos and count (MPI_Allreduce SUM,
 * as the reference does). */
int ghip_find_smbh(ghip_ctx *ctx, double SMBHmass, double pos[3], int *count);

/* ---- the sinks on the resident state: the sink table, blackhole_accretion() as a whole
 * (blackhole.c:70-791 without the log files) and the BH_FORM conversion (sfr_eff.c:602-629), for the
 * shipped flags BLACK_HOLES, BH_FORM, SWALLOWGAS, ACCRETION_RADIUS, BH_MASS_REAL,
 * LIMITED_ACCRETION_AND_FEEDBACK.  Every entry point of this section returns GHIP_EINVAL on a replicated
 * shard (ghip_set_shard).  On a multi-GPU shard (ghip_dd_init with more than one rank) the table holds the
 * rows of the Type-5 particles resident on that shard and travels with GHIP_DD_MIGRATE; ghip_sinks_density
 * and ghip_blackhole_accretion return GHIP_EINVAL there and name the collective to use instead
 * (GHIP_DD_SINK_DENSITY / GHIP_DD_BH_SWALLOW with walk = GHIP_SINKS_RESIDENT_FORM, ghip_dd_sinks_args).
 *
 * The table holds one row per Type-5 particle, keyed by P[].ID (GHIP_F_ID must have been given since the
 * counts last changed: GHIP_EINVAL otherwise) and kept in ascending ID order in device memory owned by the
 * context.  Because it is keyed by ID, ghip_rearrange and ghip_peano_order do not move it; ghip_rearrange
 * drops the rows of the Type-5 particles it eliminates.  A pass finds its sinks by a device selection of
 * the active Type-5 particles (in active-list order) and a search of each one's ID in the table: no host
 * index array enters.  An active Type-5 particle without a row: GHIP_EINVAL, the message names its ID, and
 * nothing but the marks (reset) has changed.  After ghip_set_counts with CHANGED counts the table is
 * refused until it is given again.  Mass, Vel, Hsml, TimeBin and Type stay in the GHIP_F_* fields. ---- */
enum
{
  GHIP_SK_BH_MASS = 0,       /* P[].BH_Mass */
  GHIP_SK_ACCDISC_MASS,      /* P[].AccDisc_Mass */
  GHIP_SK_BH_MDOT,           /* P[].BH_Mdot */
  GHIP_SK_DUST_MASS,         /* P[].Dust_Mass */
  GHIP_SK_TOTAL_MASS,        /* P[].Total_Mass */
  GHIP_SK_BH_DENSITY,        /* P[].b1.BH_Density */
  GHIP_SK_BH_ENTROPY,        /* P[].b2.BH_Entropy */
  GHIP_SK_GASVEL,            /* P[].b3.BH_SurroundingGasVel[3]: three columns */
  GHIP_SK_NUMNGB = GHIP_SK_GASVEL + 3,   /* PPP[].n.NumNgb */
  GHIP_SK_ACC_MASS,          /* the last ghip_blackhole_accretion's BH_accreted_Mass (before the reset of :713) */
  GHIP_SK_ACC_BHMASS,        /* ... BH_accreted_BHMass */
  GHIP_SK_ACC_DUSTMASS,      /* ... BH_accreted_DustMass */
  GHIP_SK_ACC_MOMENTUM,      /* ... BH_accreted_momentum[3]: three columns */
  GHIP_SK_COUNT = GHIP_SK_ACC_MOMENTUM + 3
};
/* id [nsink], rows [nsink][GHIP_SK_COUNT] in any order (sorted on the device).  Two rows with the same ID:
 * GHIP_EINVAL (the message names the ID) and the context holds no table.  nsink = 0: an empty table. */
int ghip_sinks_set_table(ghip_ctx *ctx, int nsink, const unsigned int *id, const double *rows);
/* *nsink rows in ascending ID order; id and rows NULL: the count only */
int ghip_sinks_get_table(ghip_ctx *ctx, int *nsink, unsigned int *id, double *rows);
int ghip_sinks_clear(ghip_ctx *ctx);   /* no table; its device memory is given back */
/* The resident form of ghip_sink_density: the same kernels and the same h iteration, for the active Type-5
 * particles in active-list order (ghip_set_active / ghip_find_next_sync_point).  Hsml is read from and
 * written to GHIP_F_HSML; NumNgb, BH_Density, BH_Entropy and BH_SurroundingGasVel go into the rows.
 * *iterations (may be NULL) = the iteration count.  The h update itself is the host's (its pow() decides
 * the bisection, bit for bit as in ghip_sink_density): per pass the six kernel sums of the sinks come to
 * the host, the results do not. */
int ghip_sinks_density(ghip_ctx *ctx, const ghip_dens_params *p, double ngb_factor, int *iterations);
typedef struct
{
  int limited_accretion;            /* -DLIMITED_ACCRETION_AND_FEEDBACK with -DACCRETION_RADIUS (shipped: 1) */
  int accretion_at_eddington_rate;  /* -DACCRETION_AT_EDDINGTON_RATE (read under limited_accretion only) */
  int enforce_eddington_limit;      /* -DENFORCE_EDDINGTON_LIMIT */
  int bh_mass_real;                 /* -DBH_MASS_REAL: meddington from P[].Mass, else from P[].BH_Mass */
  double medd_fac;   /* (4 M_PI GRAVITY C PROTONMASS / (0.1 C C THOMPSON)) * All.UnitTime_in_s
                        (blackhole.c:149-159): meddington = medd_fac * mass */
  double tvisc;      /* All.ViscousTimescale / All.UnitTime_in_s (:196) */
  double EddingtonFactor;   /* All.BlackHoleEddingtonFactor */
} ghip_bh_accretion_params;
typedef struct
{
  double TimeBin_BH_mass[32], TimeBin_BH_dynamicalmass[32], TimeBin_BH_Mdot[32];   /* this call's active sinks,
                                       added in active-list order by one thread (blackhole.c:715-719) */
  long long swallowed[3];           /* gas / sinks / dust swallowed */
  int nactive_sinks;
  int missing;                      /* the call fails -- 1: an active Type-5 particle has no row; 2: there are more
                                       of them than rows, so two of them carry the same ID */
  unsigned int missing_id;          /* ... the largest such ID */
  int pad;
} ghip_bh_accretion_report;
/* blackhole_accretion() for the active Type-5 particles in active-list order (a sink of Mass == 0 that an
 * earlier step swallowed included, as in the reference).  Needs the gravity tree of this step.
 *   Mdot (blackhole.c:119-286), one thread per sink: dt = (TimeBin ? 1 << TimeBin : 0) * bh->dt_fac;
 *     limited_accretion: mdot = AccDisc_Mass / (dt + tvisc), clamped to EddingtonFactor * meddington under
 *     enforce_eddington_limit, AccDisc_Mass -= mdot dt, BH_Mass += mdot dt (:196-202); with
 *     accretion_at_eddington_rate mdot = EddingtonFactor * meddington, BH_Mass += mdot dt (:205-206);
 *     without limited_accretion mdot = 0 (BONDI is not built) under the clamp of :218-219.  BH_Mdot = mdot.
 *   the marks are reset; blackhole_evaluate and blackhole_evaluate_swallow are the kernels of
 *     ghip_blackhole_evaluate / ghip_blackhole_swallow, reading mdot, BH_Density, the IDs and BH_Mass from
 *     device memory; only a sink whose own SwallowID is 0 swallows; BH_Mass of a swallowed sink becomes 0
 *   finish (:679-735), one thread per sink: if BH_accreted_Mass > 0, Vel = (Vel Mass + momentum) / (Mass +
 *     accreted_Mass), Mass += accreted_Mass, BH_Mass += accreted_BHMass, Dust_Mass += accreted_DustMass and
 *     Total_Mass += accreted_Mass (bh->dust), AccDisc_Mass += accreted_Mass (limited_accretion; at the
 *     Eddington rate then Mass = BH_Mass), written into GHIP_F_VEL, GHIP_F_MASS and the rows.
 * All of this arithmetic is compiled without contraction: it equals the op-by-op IEEE evaluation.
 * One device-to-host copy of the report is the only blocking read of the call.  Afterwards, as after
 * ghip_blackhole_swallow: victims have mass 0 and the trees are stale in mass only. */
int ghip_blackhole_accretion(ghip_ctx *ctx, const ghip_bh_params *bh, const ghip_bh_accretion_params *p,
                             ghip_bh_accretion_report *report);
typedef struct
{
  int stars_converted;
  int pad;
  double sum_mass_stars;            /* the masses before the change, added in list order (sfr_eff.c:607) */
  int converted_in_bin[32];         /* per TimeBin: what the host subtracts from TimeBinCountSph (:628) */
} ghip_sfr_form_report;
/* sfr_eff.c:602-629 for the candidates the last ghip_sfr_cooling found (kept on the device; ncand must be
 * the count it returned, and the particles must not have been reordered since: GHIP_EINVAL otherwise, and
 * nothing changes).  Candidate k in active-list order: Type = 5, Mass *= 0.995 + 0.005 * u01[k], and a new
 * row with its ID, all zero except BH_Mass = Mass -- with limited_accretion AccDisc_Mass = Mass and
 * BH_Mass = 0.  u01 [ncand]: the host's gsl_rng_uniform draws, one per conversion, in order.  A context
 * without a table gets one.  The candidates are consumed.  Afterwards the state is as after any change of
 * TYPE (the gas block is mixed until ghip_rearrange takes the records out of it; both trees are stale). */
int ghip_sfr_form_sinks(ghip_ctx *ctx, int ncand, const double *u01, int limited_accretion,
                        ghip_sfr_form_report *report);

/* ---- the dust-gas drag passes of the shipped flag bundle (DUST, DUST_TIMESTEP, DUST_POWERLAW,
 * CONSTANT_MEAN_MOLECULAR_WEIGHT): dust_density() and dust_drag() (dust.c:60-1029, called at accel.c:194,
 * 198).  The sub-flags DUST_GROWTH, DUST_REAL_PEBBLE_COLLISIONS, DUST_VAPORIZE, DUST_FE_AND_ICE_GRAINS,
 * DUST_EPSTEIN and DUST_NO_FRICTION_HEATING are a setting of the context (ghip_set_dust_model, below); not
 * built: DUST_TWO_POPULATIONS, DUST_GROWTH_FIXED_SIZE, DUST_MDUST_GROW, DUST_2ND_POPULATION,
 * DUST_PEBBLES_BORN, DUST_SINK_ON_FLY, DUST_ENERGY_CONSERVATION, DUST_OPACITY_FIT.
 * The grains are given by their particle
 * indices (the active Type-2 particles in active-list order); their per-grain state travels in host
 * arrays in list order.  Read from the resident fields: POS, MASS, TYPE, HSML, TIMEBIN, GRAVACCEL
 * (the finished value gravity_tree() leaves), VEL and the gas ENTROPY.  Needs the trees of this step;
 * the trees stay valid (no position or mass changes).  These two entry points are single-rank: on a
 * sharded or multi-GPU context both return GHIP_EINVAL; multi-GPU shards run GHIP_DD_DUST_DENSITY /
 * GHIP_DD_DUST_DRAG (below). ---- */
typedef struct
{
  int periodic;
  double BoxSize;
  double dt_fac;        /* grains: All.Timebase_interval / hubble_a (dust.c:348) */
  double dt_fac_gas;    /* gas: All.Timebase_interval, / (All.Time * hubble_a) when comoving (:984-987) */
  double MinEgySpec;
  double MeanWeight;    /* All.MeanWeight (CONSTANT_MEAN_MOLECULAR_WEIGHT) */
  double UnitLength_in_cm, UnitMass_in_g, UnitDensity_in_cgs, UnitVelocity_in_cm_per_s;
} ghip_dust_params;
/* dust_evaluate_density (dust.c:748-887): particle_density [ndust] = P[].d7.DUST_particle_density,
 * the sum over the Type-2 neighbours with Mass > 0 within the grain's Hsml (itself included) of
 * m_i * W(r, h_i) -- the GRAIN's mass m_i, as the reference has it (dust.c:849). */
int ghip_dust_density(ghip_ctx *ctx, const ghip_dust_params *p, int ndust, const int *dust_idx,
                      double *particle_density);
/* dust_drag (dust.c:263-746 + dust_evaluate_select :889-1029).  In [ndust]: dust_density (d1),
 * dust_entropy (d2), dust_gasvel [ndust][3] (d3), dust_radius, particle_density (d7).  In/out:
 * particle_velocity [ndust][3] (d9: divided by d7 where d7 > 0), vcoll (DustVcoll: kept where
 * d7 <= 0 and dt == 0).  Out: delta_momentum [ndust][3], delta_energy.  The grains' resident VEL,
 * the gas's VEL and ENTROPY and the resident DragHeating are updated; each gas particle receives the
 * grains in list order, as the reference's serial loop applies them (the entropy update is capped
 * and floored, so the order matters).  Deterministic. */
int ghip_dust_drag(ghip_ctx *ctx, const ghip_dust_params *p, int ndust, const int *dust_idx,
                   const double *dust_density, const double *dust_entropy, const double *dust_gasvel,
                   const double *dust_radius, const double *particle_density, double *particle_velocity,
                   double *delta_momentum, double *delta_energy, double *vcoll);
/* the resident SphP[].dh.DragHeating [ngas] (zero when first used); NULL = skip.  On a multi-GPU shard
 * (ghip_dd_init) the buffer exists once GHIP_DD_DUST_DRAG or ghip_dust_set_drag_heating has created it;
 * it then travels with its gas particles in GHIP_DD_MIGRATE.  Before that, get reads zeros and creates
 * nothing. */
int ghip_dust_get_drag_heating(ghip_ctx *ctx, double *drag_heating);
int ghip_dust_set_drag_heating(ghip_ctx *ctx, const double *drag_heating);

/* ---- the physics switches of the dust passes that the reference's Makefile lists next to -DDUST:
 * grain growth, fragmentation, vaporisation (dust.c:449-609).  A setting of the context, for
 * ghip_dust_density / ghip_dust_drag, the two *_grains entry points below and both forms of the GHIP_DD_DUST_*
 * operations alike.  p == NULL or all six switches 0: the default kernels, nothing allocated.  The setter only copies
 * the struct (a host sets Time every step).
 *   real_pebble_collisions   the density pass also sums d9[k] += m_i W(r, h_i) Vel_j[k] over the neighbours
 *              of d7, with the same weight (dust.c:851-853); the drag pass divides by d7 as it always has.
 *              In the growth rule: adot = 0 if FragmentationVelocity < 0.1, else
 *              adot *= (1 - x^2) / (1 + x^2), x = DustVcoll / FragmentationVelocity (:479-490)
 *   epstein    ts is always the Epstein expression (:415-416)
 *   no_friction_heating   the friction term of DeltaDragEnergy is dropped (:433-435)
 *   growth     behind the gate Time > 0 && Time > VirtualTime, for d7 > 0 (:453-494):
 *              t_coll = 4 (rho_grain / UnitDensity) (a / UnitLength) / d7 / (DustVcoll 1e2 / UnitVelocity
 *              + 1e-20) with the FINAL DustVcoll of the call -- the value of :374 is overwritten at
 *              :437-444 whenever dt > 0, a quirk kept --, LogDustRadius_by_dt = t_coll, adot = a / UnitLength
 *              / 3 / t_coll.  DustRadius += adot dt UnitLength_in_cm (:551), then clamped to [0.1, 1e5] cm
 *              (:566-567) -- for EVERY grain of the list, also with dt == 0 or behind a closed gate
 *   vaporize   for DUST_Density > 0, whatever the gate (:501-529): T = pi / 8 (c_s UnitVelocity)^2 MeanWeight
 *              m_p / k_B, pvap = 10^(-24605 / T + 13.176), adot -= 1 / (rho_grain sqrt(2 * 3.1415)) / c_s
 *              / UnitVelocity * pvap / UnitVelocity (the literal is 3.1415).  The latent heat 1e11 (a - 0.1) /
 *              (InitialDustRadius - 0.1) is taken before and after the radius update; the difference times
 *              Mass UnitMass_in_g / UnitEnergy_in_cgs is added to DeltaDragEnergy (:533-608), so the
 *              scatter cools or heats the gas by it
 *   fe_and_ice_grains   grains with an odd ID (the resident GHIP_F_ID) are water ice: pvap = 10^(11.6 -
 *              2104 / T) for T <= 600, 5 + 5.2e-3 T above; latent constant 4e10 (:509-547, 596-605)
 * GHIP_EINVAL from the setter, before anything is launched: a value that is not finite; vaporize without
 * growth; fe_and_ice_grains without vaporize; vaporize with InitialDustRadius == 0.1 (the denominator of the
 * latent heat); a context of ghip_set_shard (use the ghip_dd_* contexts).  A drag pass with
 * fe_and_ice_grains returns GHIP_EINVAL when GHIP_F_ID was never given (ghip_set_field).
 * On ghip_dd_* contexts the setting must be the same on all ranks (the caller's duty: nothing checks it). ---- */
typedef struct
{
  int growth;                   /* DUST_GROWTH */
  int real_pebble_collisions;   /* DUST_REAL_PEBBLE_COLLISIONS */
  int vaporize;                 /* DUST_VAPORIZE (needs growth) */
  int fe_and_ice_grains;        /* DUST_FE_AND_ICE_GRAINS (needs vaporize) */
  int epstein;                  /* DUST_EPSTEIN */
  int no_friction_heating;      /* DUST_NO_FRICTION_HEATING */
  double Time, VirtualTime;     /* All.Time, All.VirtualTime: the gate of growth */
  double FragmentationVelocity; /* All.FragmentationVelocity, in the units of DustVcoll (m/s) */
  double InitialDustRadius;     /* All.InitialDustRadius [cm] */
  double UnitEnergy_in_cgs;
} ghip_dust_model;
int ghip_set_dust_model(ghip_ctx *ctx, const ghip_dust_model *m);   /* NULL: everything off (the default path) */
size_t ghip_dust_model_size(void);    /* sizeof(ghip_dust_model) of the library, for bindings to check */
/* The arrays of a grain list, in list order: the members of ghip_dust_density / ghip_dust_drag plus the two
 * that the model writes.  Members a pass does not use may be NULL. */
typedef struct
{
  int ndust;
  const int *dust_idx;            /* local particle indices, in active-list order */
  double *particle_density;       /* [ndust] d7: density out, drag in */
  const double *dust_density, *dust_entropy, *dust_gasvel;   /* drag in (d1, d2, d3 [ndust][3]) */
  double *dust_radius;            /* drag in/out [ndust] (written with growth only) */
  double *particle_velocity;      /* [ndust][3] d9: density out -- the raw sums, written with
                                     real_pebble_collisions only --, drag in/out (divided by d7 where d7 > 0) */
  double *delta_momentum, *delta_energy;   /* drag out ([ndust][3], [ndust]) */
  double *vcoll;                  /* drag in/out [ndust] */
  double *log_radius_by_dt;       /* drag in/out [ndust], may be NULL: t_coll where dust.c:465 writes it (growth,
                                     the gate open, d7 > 0), the caller's value elsewhere */
  long long *counts;              /* shards only, out [4] (may be NULL): as ghip_dd_dust_args.counts */
} ghip_dust_grains;
size_t ghip_dust_grains_size(void);
/* ghip_dust_density / ghip_dust_drag for every setting of ghip_set_dust_model (single-rank, like them).  The
 * two old entry points keep their signatures and honour epstein / no_friction_heating; ghip_dust_density with
 * real_pebble_collisions set, and ghip_dust_drag with growth or vaporize set, return GHIP_EINVAL: they have
 * no array for what those switches write. */
int ghip_dust_density_grains(ghip_ctx *ctx, const ghip_dust_params *p, const ghip_dust_grains *g);
int ghip_dust_drag_grains(ghip_ctx *ctx, const ghip_dust_params *p, const ghip_dust_grains *g);

/* ---- wind particles of the shipped flag bundle (-DVIRTUAL -DFB_MOMENTUM, with VIRTUAL_FLY_THORUGH_EMPTY_SPACE,
 * VARIABLE_PHOTON_SEARCH_RADIUS and RAD_ACCEL as run-time switches): the propagation loop of momentum_feedback()
 * (momentum_feedback.c:251-591) with its two neighbour passes virtual_density() and virtual_spread_momentum().
 * ghip_set_integration_flags gives a Type-3 particle its step limit and neither kick nor drift; THIS is where
 * it moves.  The creation of wind particles (:70-246) is ghip_wind_spawn, below.  Not built:
 * fb_particles.c (PHOTONS, VIRTUAL_HEATING, re-emission), REAL_EOS, NON_GRAY_RAD_TRANSFER.
 * The wind particles are given by their particle indices: the active Type-3 particles with StellarAge < Time
 * and WindOrPhoton == 0, in active-list order (:253-278); their per-particle state travels in host arrays in
 * list order.  Resident fields read: TYPE, TIMEBIN, VEL, and of the gas POS, HSML, MASS; written at the wind
 * indices by ghip_wind_feedback: POS, HSML, MASS.  Needs the trees of this step (GHIP_EINVAL "call
 * ghip_tree_build first" otherwise); the gas tree stays valid, the gas does not move.  The gravity tree keeps
 * the wind particles where they were when it was built, as the reference's does.  ghip_wind_density,
 * ghip_wind_spread and ghip_wind_feedback are single-rank: on a ghip_dd_init context they return GHIP_EINVAL and
 * name GHIP_DD_WIND, the operation that runs them on shards (below); on a ghip_set_shard context every entry
 * point below returns GHIP_EINVAL.  An index that does not name a Type-3 particle is GHIP_EINVAL. ---- */
typedef struct
{
  int periodic;
  double BoxSize;
  double Time;
  double dt_fac;        /* wind particles: All.Timebase_interval / hubble_a (momentum_feedback.c:288) */
  double dt_fac_gas;    /* gas (rad_accel): All.Timebase_interval, / time_hubble_a when comoving (:502-505) */
  double FeedBackVelocity, UnitVelocity_in_cm_per_s, UnitDensity_in_cgs, UnitLength_in_cm;
  double VirtualCrosSection, VirtualMass, VirtualTime, OuterBoundary;
  double DesNumNgb, OriginalGasMass, SofteningGas, SofteningGasMaxPhys, SofteningBulgeMaxPhys;
  double PhotonSearchRadius;
  double dt_total_floor;   /* 1e-15 * All.VirtualTime * (All.MaxPart * NTask), :302.  GHIP_DD_WIND: the GLOBAL floor,
                            * with NTask in it, the same on every shard: it is compared with the sum over all shards */
  int fly_through_empty_space;   /* VIRTUAL_FLY_THORUGH_EMPTY_SPACE: the drmin step limit of :337-340 */
  int variable_search_radius;    /* VARIABLE_PHOTON_SEARCH_RADIUS: the Hsml cap of :409-410 */
  int rad_accel;                 /* RAD_ACCEL: :497-538 at the end of ghip_wind_feedback */
  int max_iter;                  /* a guard the reference lacks: GHIP_ENOCONV after this many iterations */
} ghip_wind_params;
size_t ghip_wind_params_size(void);
/* one virtual_density() (virtual_density.c:79-748).  In [nwind]: dt_jump.  Out [nwind]: new_density
 * (P[].NewDensity) and drmin (b1.BH_Density).  Every listed particle gets new_density = 0 and drmin = 1e40
 * (:107-127); those with dt_jump > 0 are evaluated: over the gas neighbours j with Mass > 0 within the
 * particle's own resident HSML, drmin = min(drmin, |r - h_j| + 0.25 h_j) (:519-520) and, where r / h_j < 1,
 * new_density += m_j W(r, h_j) with the GAS particle's h_j (:524-539).  Read-only on the resident fields. */
int ghip_wind_density(ghip_ctx *ctx, const ghip_wind_params *p, int nwind, const int *wind_idx,
                      const double *dt_jump, double *new_density, double *drmin);
/* one virtual_spread_momentum() (virtual_spread_momentum.c:58-469).  In [nwind]: dt_jump, new_density,
 * delta_momentum (DeltaPhotonMomentum).  For the listed particles with new_density > 0 && dt_jump > 0
 * (:129-130) every gas neighbour found as above with u < 1 receives delta_momentum m_j W / new_density
 * Vel[k] / |Vel| (:432, 448) into the resident SphP[].i.Injected_BH_Momentum.  Each gas particle receives its
 * wind particles in list order and every sum runs in a fixed order: two identical calls give identical
 * bits. */
int ghip_wind_spread(ghip_ctx *ctx, const ghip_wind_params *p, int nwind, const int *wind_idx,
                     const double *dt_jump, const double *new_density, const double *delta_momentum);
/* the per-particle state of ghip_wind_feedback, host arrays [nwind] in list order, none may be NULL */
typedef struct
{
  const double *stellar_age;     /* in      P[].StellarAge */
  const double *birth_energy;    /* in      P[].BirthPhotonEnergy */
  double *old_momentum;          /* in/out  P[].OldPhotonMomentum */
  double *new_density;           /* in/out  P[].NewDensity */
  double *drmin;                 /* in/out  P[].b1.BH_Density */
  double *dt1, *dt2, *dt_jump;   /* out     P[].dt1, P[].dt2, P[].DtJump */
  double *delta_momentum;        /* out     P[].DeltaPhotonMomentum (kept 0 for a particle that never moved) */
  int *deleted;                  /* out     0 = kept, 1 = left OuterBoundary or older than VirtualTime, 2 = depleted */
} ghip_wind_state;
typedef struct
{
  int iterations;              /* N_iter */
  long long bits;              /* basic steps of all particles (:324) */
  int ndeleted;                /* count_deleted_photon */
  double deleted_momentum;     /* OldPhotonMomentum of the deleted of the first kind, summed in list order (:559) */
} ghip_wind_result;
/* momentum_feedback.c:283-568 without the prints and the diagnostic files.  dt_jump from the time bin, dt2 = 0;
 * if the sum of dt_jump is at or below dt_total_floor the call returns having changed nothing (the out arrays
 * are filled: dt_jump, zeros).  Otherwise one density pass, then per iteration the move of every particle with
 * dt_jump > 0 (:312-427), a density pass, a spread pass and the new list (dt_jump > 1e-40), until the list is
 * empty; with rad_accel :497-538 for the active gas (ghip_set_active); then the elimination (:550-568: Mass = 0
 * and the code in `deleted`).  The per-particle state crosses the link once in and once out; inside the loop
 * one 40-byte read per iteration (pair and list counts) reaches the host.  The neighbour walks search
 * min(Hsml, the largest h_j of the gas) for the sums and the pairs, and as far beyond as drmin needs: the pairs
 * and their order are those of the whole sphere.
 * ONE DELIBERATE DEVIATION: when the time cap of :345-346 sets the jump, dt1 = dt_jump exactly and the particle
 * ends the iteration with dt_jump = 0.  The reference recomputes dt1 = dr * U / C * FBV (:348) and subtracts it
 * (:371-372); the residue of that round trip is 0 or +-1 ulp, and on its sign hangs one more iteration of
 * length ~1e-17.
 * max_iter reached with particles under way: GHIP_ENOCONV, the state as it stands (no rad_accel, no
 * elimination), ghip_last_error says how many were under way. */
int ghip_wind_feedback(ghip_ctx *ctx, const ghip_wind_params *p, int nwind, const int *wind_idx,
                       const ghip_wind_state *state, ghip_wind_result *result);
/* the resident gas fields SphP[].i.Injected_BH_Momentum [ngas][3] and SphP[].ra.RadAccel [ngas][3], zero when
 * first used; NULL = skip.  Values held for one ngas are refused after ghip_set_counts changes it (set them
 * again), as ghip_kick_set_fields does.  On a ghip_dd_init context they are the fields of the shard's own gas
 * and travel with their particle in GHIP_DD_MIGRATE (a field held for another gas count is not carried). */
int ghip_wind_get_injected(ghip_ctx *ctx, double *injected);
int ghip_wind_set_injected(ghip_ctx *ctx, const double *injected);
int ghip_wind_get_rad_accel(ghip_ctx *ctx, double *rad_accel);
int ghip_wind_set_rad_accel(ghip_ctx *ctx, const double *rad_accel);
/* RAD_ACCEL in the integrator: the timestep criterion adds fac2 RadAccel (timestep.c:668-671); the kick adds
 * RadAccel dt_hydrokick to Vel and then SETS VelPred = Vel - dt_hydrokick2 RadAccel (:497-500, overwriting the
 * line above it, as the C text does; the PMGRID term of :512 still follows); ghip_pm_kick sets VelPred = Vel +
 * RadAccel dt_hydrokick (:337-339); ghip_drift adds RadAccel dt_hydrokick to VelPred (predict.c:190-192).
 * Kernel instantiations of their own: with the switch off (the default) the existing kernels run and a
 * resident RadAccel is not read.  Per-particle arithmetic: a ghip_dd_init shard reads its own RadAccel; not on
 * a ghip_set_shard context. */
int ghip_set_rad_accel(ghip_ctx *ctx, int on);
/* milliseconds of the last ghip_wind_feedback from events around its phases, summed over the iterations:
 * move, density, spread, list, and the whole call; synchronises.  After GHIP_DD_WIND: this shard's move, own
 * density, spread, list, and in ms[4] the density of the imported particles */
int ghip_wind_get_timing(ghip_ctx *ctx, double ms[5]);

/* ---- the wind particles on the resident state: the wind table, the propagation loop without host arrays and
 * the creation of wind particles by the massive sinks (momentum_feedback.c:70-246).  With them the wind cycle
 * closes on the device: the sinks accrete (ghip_blackhole_accretion), emit (ghip_wind_spawn), the wind
 * propagates (ghip_winds_feedback) and what is spent leaves with ghip_rearrange; no per-particle host array and
 * no pass through the host is involved.  There are two families.  The entry points of THIS section are for one
 * GPU: a plain context or a ghip_dd_init context of a single rank; on a ghip_dd_init context with more than one
 * rank each of them returns GHIP_EINVAL, says that the shard form is not built into it and names the shard family.
 * The shard family is for a ghip_dd_init context of any rank count: the table ghip_dd_winds_set_table /
 * _get_table / _clear (local indices), which GHIP_DD_MIGRATE carries, and the loop as the collective GHIP_DD_WIND
 * with walk = GHIP_WINDS_RESIDENT_FORM (both below, with the other wind forms); on a plain context they return
 * GHIP_EINVAL and name the single-rank function.  On a ghip_set_shard context every entry point of both families
 * returns GHIP_EINVAL.  ghip_wind_spawn on more than one rank is GHIP_DD_WIND with walk = GHIP_WINDS_SPAWN_FORM.
 * Not built: force_add_star_to_tree (a spawn discards the trees), fb_particles.c / PHOTONS, SPH_EMIT, and the P[i].dt1 the
 * reference writes into the sink's own record (:80).
 *
 * The table holds one row of GHIP_WK_COUNT doubles per wind particle, keyed by PARTICLE INDEX and kept in
 * ascending index order in device memory owned by the context.  It cannot be keyed by P[].ID as the sink table
 * is: :215 sets ID = the sink's ID + (NumPart + stars_spawned), and NumPart shrinks when
 * rearrange_particle_sequence() eliminates particles, so two live wind particles can carry the same ID (the
 * shipped -DIGNORE_NON_UNIQUE tolerates it).  Because it is keyed by index, ghip_rearrange and ghip_peano_order
 * carry it: every index goes through their new_of_old, the rows of eliminated particles are dropped, and the
 * rows are put back in ascending order.  After ghip_set_counts with CHANGED counts the table is refused until
 * it is given again. ---- */
enum
{
  GHIP_WK_STELLAR_AGE = 0,   /* P[].StellarAge */
  GHIP_WK_BIRTH_ENERGY,      /* P[].BirthPhotonEnergy */
  GHIP_WK_OLD_MOMENTUM,      /* P[].OldPhotonMomentum */
  GHIP_WK_NEW_DENSITY,       /* P[].NewDensity */
  GHIP_WK_DRMIN,             /* P[].b1.BH_Density */
  GHIP_WK_DT1,               /* P[].dt1 */
  GHIP_WK_DT2,               /* P[].dt2 */
  GHIP_WK_DT_JUMP,           /* P[].DtJump */
  GHIP_WK_DELTA_MOMENTUM,    /* P[].DeltaPhotonMomentum */
  GHIP_WK_DELETED,           /* the code of ghip_wind_state.deleted of the last ghip_winds_feedback: 0.0, 1.0 or 2.0 */
  GHIP_WK_COUNT
};
/* idx [nwind], rows [nwind][GHIP_WK_COUNT] in any order (sorted on the device).  GHIP_EINVAL, and the context
 * holds no table: an index out of range, an index that names a particle that is not Type 3, an index given
 * twice (the message names the index).  nwind = 0: an empty table. */
int ghip_winds_set_table(ghip_ctx *ctx, int nwind, const int *idx, const double *rows);
/* *nwind rows in ascending index order; idx and rows NULL: the count only */
int ghip_winds_get_table(ghip_ctx *ctx, int *nwind, int *idx, double *rows);
int ghip_winds_clear(ghip_ctx *ctx);   /* no table; its device memory is given back */
/* The resident form of ghip_wind_feedback: the same kernels and the same loop, no wind_idx, no ghip_wind_state.
 * The list is a device selection: the active Type-3 particles (ghip_set_active / ghip_find_next_sync_point)
 * that have a row with StellarAge < Time (:259), in active-list order.  An active Type-3 particle without a
 * row: GHIP_EINVAL, the message names its index, and nothing has changed.  The state of the listed particles is
 * gathered from the rows, and after the loop and the elimination every column but StellarAge and BirthEnergy
 * is written back (GHIP_WK_DELETED with the code); a row that is not listed is not touched.  The host reads
 * the length of the list (8 bytes) where ghip_wind_feedback uploads the state, then as there the 40 bytes per
 * iteration, and the result, which one thread adds in list order.  Everything else is as ghip_wind_feedback
 * says, the deviation and GHIP_ENOCONV included; the values equal, bit for bit, those of ghip_wind_feedback
 * called with the same list and the rows' state. */
int ghip_winds_feedback(ghip_ctx *ctx, const ghip_wind_params *p, ghip_wind_result *result);
typedef struct
{
  double Time;
  double dt_fac;                 /* All.Timebase_interval / hubble_a (:79) */
  double SMBHmass, VirtualStart, VirtualFeedBack, VirtualMomentum, VirtualMass, FeedBackVelocity;
  double UnitVelocity_in_cm_per_s, UnitTime_in_s;
  double SofteningBndryMaxPhys;
  double InnerBoundary;          /* added to Hsml behind the softening under accretion_radius (:182) */
  int NumCurrentTiStep;
  int MaxPart;
  int fraction_of_ledd_feedback;     /* -DFRACTION_OF_LEDD_FEEDBACK: :85, else :100-105 */
  int accretion_at_eddington_rate;   /* -DACCRETION_AT_EDDINGTON_RATE (read under fraction_of_ledd_feedback): :88-89 */
  int startup_luminosity;            /* -DSTARTUP_LUMINOSITY: emit above 1e-4, else above 0 (:114-118) */
  int isotropic;                     /* -DISOTROPIC: :169, else :171 */
  int accretion_radius;              /* -DACCRETION_RADIUS: :182 */
  int fly_through_empty_space;       /* -DVIRTUAL_FLY_THORUGH_EMPTY_SPACE: the new row's drmin = 0 (:198), else the
                                        sink's b1.BH_Density, which :158 copies */
  const double *rnd_table;           /* the host's RndTable [nrnd], copied by the call; NULL: the table bound with */
  int nrnd;                          /* ghip_set_rnd_table.  Neither: GHIP_EINVAL */
  int pad;
} ghip_wind_spawn_params;
typedef struct
{
  int spawned;                /* stars_spawned */
  int nsinks_emitting;        /* sinks with new_wind > 0 */
  int first_index;            /* index of the first new particle: NumPart before the call */
  int pad;
  double new_wind_exact_sum;  /* new_wind_exact of the emitting sinks, added in list order by one thread */
  long long gsl_draws;        /* 3 * spawned: the draws of :193 (multiplied by 0. there), which the host takes from its
                                 own random_generator to keep its stream where the reference's would be */
} ghip_wind_spawn_report;
size_t ghip_wind_spawn_params_size(void);
size_t ghip_wind_spawn_report_size(void);
/* momentum_feedback.c:70-246 on the device.  Needs the sink table (ghip_sinks_set_table: BH_Mdot and BH_Mass are
 * read from the rows; an active Type-5 particle without a row is GHIP_EINVAL as in the sink passes) and a wind
 * table; a context without a wind table gets an empty one.
 *   count   one thread per active Type-5 particle, in active-list order.  A sink counts when Mass > 0.5 SMBHmass
 *           && Time > VirtualStart (:75).  dt = (TimeBin ? 1 << TimeBin : 0) * dt_fac; new_wind_exact from :85-88
 *           under the switches or :100-105; new_wind = (int) new_wind_exact + 1 above the threshold, else 0;
 *           correction_wind = new_wind_exact / new_wind (:126-133).  Compiled without contraction.
 *   scan    an exclusive scan of the counts and the one blocking read of the call, the total.  NumPart + total >
 *           MaxPart: GHIP_EINVAL (the reference's endrun(8888); the message has both numbers), nothing has changed.
 *   grow    the state goes from n to n + total particles: every GHIP_F_* field and every optional per-particle
 *           array (SwallowID, the kick's NewDensity) of an appended particle is its sink's, P[NumPart +
 *           stars_spawned] = P[i] (:158).  Arrays per gas particle do not change: ngas does not.
 *   fill    one thread per new particle j, the bits-th of its sink: Type = 3; Hsml += SofteningBndryMaxPhys (+=
 *           InnerBoundary); theta and phi from RndTable[(ID + 2 + bits + NumCurrentTiStep) % nrnd] and [(ID + 3 +
 *           ...) % nrnd] in unsigned 32-bit arithmetic (:168-173); Vel = C / UnitVelocity * dir / FeedBackVelocity
 *           (:191); Pos stays the sink's (the term of :193 is multiplied by 0.); ID += j in unsigned arithmetic
 *           (:215); OldMomentum = VirtualMomentum-energy / C * UnitVelocity * correction, BirthEnergy = energy *
 *           correction (:225-226); Mass = VirtualMass * OldMomentum (:228); the kick's NewDensity = 0; the row is
 *           StellarAge = Time, dt1 = dt (:80, copied by :158), drmin as above, everything else 0, appended to
 *           the table (the new particles have the largest indices: it stays sorted).
 * Under accretion_at_eddington_rate a counting sink's Mass = BH_Mass (:89), whether it emits or not.
 * Afterwards the new particles stand at the end of the active list in force (everybody active: still
 * everybody, :202-204); the bin counts are recounted by the next ghip_find_next_sync_point; both trees and the
 * kept tree of ghip_set_dynamic_tree are discarded (force_add_star_to_tree is not built): ghip_tree_build comes
 * next.  The sink table is untouched: its key is the ID, and no sink moved.  spawned == 0 leaves every byte of
 * the state, the lists and the trees as they were.
 * CALL ORDER.  A particle born at Time is not propagated until StellarAge < Time (:259), and propagation does
 * not touch the sinks: ghip_wind_spawn may run AFTER ghip_winds_feedback and the other neighbour passes of the
 * step, so that they use the trees of the step, with the same result as the reference's order.  That is the
 * intended order: ghip_blackhole_accretion, ghip_winds_feedback, ghip_wind_spawn, the kick. */
int ghip_wind_spawn(ghip_ctx *ctx, const ghip_wind_spawn_params *p, ghip_wind_spawn_report *report);

/* The dust passes on a multi-GPU shard (GHIP_DD_DUST_DENSITY / GHIP_DD_DUST_DRAG through ghip_dd_begin /
 * ghip_dd_run): the reference's export of the grains (dust.c:60-261, 560-746).  Each grain goes to every
 * other shard whose local Type 0 / Type 2 particles its sphere (Pos, Hsml) can reach (a sphere test
 * against the all-gathered group boxes of those particles).
 *   DUST_DENSITY  every shard sums its own Type-2 neighbours for its own and the imported grains (the
 *                 grain's own mass, dust.c:849); the partial d7 of an imported grain goes back to its
 *                 home shard, which adds them to its own sum in ascending rank order (dust.c:223).
 *   DUST_DRAG     the per-grain update runs on the home shard; the grain's Pos, Hsml, DUST_Density,
 *                 DeltaDustMomentum and DeltaDragEnergy go to the same shards, and every shard
 *                 scatters into its own gas.  A gas particle receives this shard's grains in list
 *                 order, then the imported ones by sending rank and, within a rank, by the sender's
 *                 local particle index (the reference's order with one export round).
 * Arrays describe the grains resident on THIS shard, as ghip_dust_density / ghip_dust_drag take them;
 * the drag pass creates the shard's resident DragHeating.  Members an operation does not use may be
 * NULL. */
typedef struct
{
  const ghip_dust_params *p;
  int ndust;                      /* active grains resident on this shard */
  const int *dust_idx;            /* their local particle indices, in active-list order */
  double *particle_density;       /* [ndust] d7: DUST_DENSITY out, DUST_DRAG in */
  const double *dust_density, *dust_entropy, *dust_gasvel, *dust_radius;   /* DUST_DRAG in (d1, d2, d3 [ndust][3]) */
  double *particle_velocity;      /* DUST_DRAG in/out [ndust][3] (d9) */
  double *delta_momentum, *delta_energy;   /* DUST_DRAG out ([ndust][3], [ndust]) */
  double *vcoll;                  /* DUST_DRAG in/out [ndust] */
  long long *counts;              /* out [4] (may be NULL): grain records this shard sent, records it
                                     received, (gas, grain) pairs of its scatter (DUST_DRAG), bytes sent */
} ghip_dd_dust_args;

/* The sink passes on a multi-GPU shard (GHIP_DD_SINK_DENSITY / _BH_EVALUATE / _BH_SWALLOW through
 * ghip_dd_begin / ghip_dd_run): the sinks of every shard are made known to all shards (a few hundred
 * 96-byte records), each shard evaluates ALL sinks against ITS OWN particles, and the partial sums
 * (density: 6 doubles per sink and h iteration; swallow: 9) are all-gathered and added in rank order
 * -- the reference's export of the few sink targets (blackhole.c:310-600) instead of an import of
 * their neighbourhoods.  A victim is local to exactly one shard, which sees every sink's claim, so
 * the marks equal the single-GPU ones.  Arrays of this struct describe the sinks resident on THIS
 * shard; members an operation does not use may be NULL. */
typedef struct
{
  const ghip_dens_params *dens;   /* SINK_DENSITY */
  double ngb_factor;              /* All.BlackHoleNgbFactor */
  const ghip_bh_params *bh;       /* BH_EVALUATE, BH_SWALLOW */
  int nsink;                      /* sinks resident on this shard */
  const int *sink_idx;            /* their local particle indices */
  const unsigned int *sink_id;    /* P[].ID */
  double *hsml;                   /* [nsink] SINK_DENSITY in/out */
  double *numngb, *bh_density, *bh_entropy, *bh_gasvel;   /* SINK_DENSITY out ([nsink], gasvel [nsink][3]) */
  const double *bh_mdot;          /* BH_EVALUATE in */
  const double *bh_density_in;    /* BH_EVALUATE in */
  double *sink_bh_mass;           /* BH_SWALLOW in/out */
  double *acc_mass, *acc_bhmass, *acc_dustmass, *acc_momentum;   /* BH_SWALLOW out */
  long long *counts;              /* BH_SWALLOW out [3]: gas / sinks / dust swallowed ON THIS SHARD */
} ghip_dd_sink_args;
#define GHIP_DD_SINK_DENSITY 5   /* needs GHIP_DD_DENSITY of this step (the shard's gas tree) */
#define GHIP_DD_BH_EVALUATE 6    /* needs GHIP_DD_GRAVITY of this step (the shard's gravity tree) */
#define GHIP_DD_BH_SWALLOW 7     /* a sink whose own SwallowID is set swallows nothing (blackhole.c:528-532, see
                                    ghip_blackhole_swallow): its mark travels to the other shards in its record */
/* The sinks on the resident state of shards and ranks: GHIP_DD_SINK_DENSITY and GHIP_DD_BH_SWALLOW begun with
 * walk = GHIP_SINKS_RESIDENT_FORM take a ghip_dd_sinks_args and no host array.  Every shard holds the rows
 * of the Type-5 particles resident on it (ghip_sinks_set_table / _get_table / _clear / ghip_sfr_form_sinks act
 * on those rows); either all shards hold a table (an empty one counts) or none does.  GHIP_DD_MIGRATE carries
 * the row of a departing Type-5 particle to the shard that receives the particle, as a second all-to-all-v
 * of (ID, GHIP_SK_COUNT doubles) records that runs only when the shards hold tables; a departing Type-5
 * particle without a row departs without one; an ID that arrives where it already has a row fails the
 * migration on all shards.  One shard with a table beside one without: GHIP_DD_MIGRATE and both forms below
 * fail on all shards, nothing moved.
 *   GHIP_DD_SINK_DENSITY  ghip_sinks_density for the active Type-5 particles of all shards: each shard selects
 *     its own in active-list order and finds their rows; the exchanges are those of the walk = 0 form (the
 *     96-byte records to everybody, 6 partial sums per sink and h pass all-gathered, the h update on every
 *     shard's host).  The home shard writes h into GHIP_F_HSML and NumNgb, BH_Density, BH_Entropy and
 *     BH_SurroundingGasVel into the rows.  *iterations (may be NULL): the iteration count.
 *   GHIP_DD_BH_SWALLOW    ghip_blackhole_accretion as ONE collective: the Mdot loop into the rows and the reset
 *     of the marks; the records to everybody; blackhole_evaluate for all sinks over each shard's particles;
 *     the records again, now with each sink's own SwallowID as the marking pass left it (BH_Mass stays at
 *     home: a swallowed sink's BH_Mass is read on the shard that holds it); the sweep and the all-gather of
 *     its 9 partial planes; their sum in ascending rank order from 0.0 on the device (the bits of the
 *     walk = 0 form's host loop); the finish into GHIP_F_VEL, GHIP_F_MASS and the rows of this shard's sinks.
 *     *report: this shard's sinks (the per-bin sums, nactive_sinks) and the particles of THIS shard that
 *     were swallowed -- the per-task values of the reference, which the host adds (blackhole.c:659-661,
 *     749-751).  Blocking reads: the selection's words and the report.  Afterwards as after the walk = 0
 *     form: the trees are stale in mass only.
 * GHIP_DD_BH_EVALUATE has no such form (any walk but 0: GHIP_EINVAL).  An active Type-5 particle without a
 * row on its home shard, a shard without a table, two active sinks of the run with one ID: GHIP_EINVAL on
 * all shards, the message names the ID, and nothing but the marks (reset) has changed.  A sink swallowed
 * while inactive does not add its BH_Mass (as on one GPU). */
typedef struct
{
  const ghip_dens_params *dens; double ngb_factor; int *iterations;        /* GHIP_DD_SINK_DENSITY */
  const ghip_bh_params *bh; const ghip_bh_accretion_params *acc;
  ghip_bh_accretion_report *report;                                        /* GHIP_DD_BH_SWALLOW */
} ghip_dd_sinks_args;
size_t ghip_dd_sinks_args_size(void);
#define GHIP_SINKS_RESIDENT_FORM 1   /* `walk` of ghip_dd_begin / ghip_dd_run for the two operations above */
/* pmforce_periodic on shards (params: ghip_pm_params): every shard deposits ITS particles on the full
 * PMGRID^3 mesh, the meshes are all-gathered and added in rank order (8 PMGRID^3 bytes per shard:
 * 16.8 MB at PMGRID = 128), then every shard transforms the identical mesh and interpolates the
 * force for its own particles -- the reference's slab exchange (pm_periodic.c:263-450) with the
 * transform replicated instead of distributed.  Pairs with GHIP_WALK_SHORTRANGE of GHIP_DD_GRAVITY. */
#define GHIP_DD_PM 8
/* the dust passes (params: ghip_dd_dust_args, see above) */
#define GHIP_DD_DUST_DENSITY 9   /* needs GHIP_DD_GRAVITY of this step */
#define GHIP_DD_DUST_DRAG 10     /* needs GHIP_DD_GRAVITY and GHIP_DD_DENSITY of this step */
/* The dust passes with the arrays of ghip_dust_grains, for every setting of ghip_set_dust_model: the same two
 * operations and the same exchanges, GHIP_DD_DUST_DENSITY / GHIP_DD_DUST_DRAG begun with walk =
 * GHIP_DUST_GRAINS_FORM and params a ghip_dd_dust_grains_args (ghip_dd_begin's `walk` selects the form of an
 * operation; the operation codes stay below 16 and none moves).  walk = 0 is the form above.  With
 * real_pebble_collisions the partial an importing shard returns per grain record is d7 and the three velocity
 * sums (32 bytes, not 8), added on the home shard rank by rank in ascending order; without it not a byte more
 * travels.  The per-grain update (growth, vaporisation) runs on the home shard only and the 72-byte drag record
 * is unchanged: DeltaDragEnergy already holds the latent heat.  Radius and LogDustRadius_by_dt are host-held
 * per-grain arrays and need no migration slot.  With walk = 0 the two operations refuse the switches that
 * ghip_dust_density / ghip_dust_drag refuse; any other walk is GHIP_EINVAL. */
typedef struct
{
  const ghip_dust_params *p;
  ghip_dust_grains g;
} ghip_dd_dust_grains_args;
#define GHIP_DUST_GRAINS_FORM 1   /* `walk` of ghip_dd_begin / ghip_dd_run for the two dust operations */
/* compute_potential() on shards (params: ghip_pot_params, the argument rules of ghip_potential, checked
 * by ghip_dd_begin before anything is launched or posted).  The targets are ALL particles of every shard,
 * so the locally essential trees of the step's GHIP_DD_GRAVITY -- selected against the active targets
 * only -- do not serve: the operation builds the shard's tree, forms target groups over all its own
 * particles (with their least OldAcc), all-gathers them, selects / packs / exchanges the tree elements as
 * GHIP_DD_GRAVITY does, builds the merged tree and walks it for its own particles.  pm.pmgrid > 0: every
 * shard deposits its own particles, the meshes are all-gathered and added in rank order as in GHIP_DD_PM,
 * every shard solves and reads out at its own particles.  Afterwards ghip_get_potential /
 * ghip_get_potential_interactions give the shard's own particles in host order, and
 * GHIP_DD_GLOBAL_QUANTITIES reads the result; it is discarded where ghip_potential's is, and by
 * GHIP_DD_MIGRATE.  The gravity tree the operation leaves behind is NOT the one of the step's
 * GHIP_DD_GRAVITY: the operations that need that one return GHIP_EINVAL until the next GHIP_DD_GRAVITY.
 * A target that would have to open an imported pruned node makes every shard return GHIP_EDEVICE. */
#define GHIP_DD_POTENTIAL 11
/* compute_global_quantities_of_system() on shards (params: ghip_dd_global_args): every shard sums its own
 * particles as ghip_global_quantities does (the potential: p->Potential, else the shard's last
 * GHIP_DD_POTENTIAL), the sums are all-gathered and added in rank order on every shard: `out` holds the
 * same bytes on all shards, on a repeat and for every transport.  No atomics. */
#define GHIP_DD_GLOBAL_QUANTITIES 12
typedef struct
{
  const ghip_global_params *p;
  ghip_global_sums *out;
} ghip_dd_global_args;
/* ... begun with walk = GHIP_FOF_FORM and params a ghip_dd_fof_args: the friends-of-friends groups of ALL shards
 * (fof_fof on NTask > 1, fof.c; "friends-of-friends groups" below says what the collective form does).  The
 * traffic counter of GHIP_DD_GLOBAL_QUANTITIES (ghip_dd_bytes_sent) serves whichever form ran last. */
#define GHIP_FOF_FORM 1
/* domain_Decomposition on shards (params: ghip_dd_decomp_params): the ranges of ghip_dd_set_splits, and on
 * request the cube of ghip_dd_set_domain, are computed from the RESIDENT particles of all shards; no rank
 * ever holds another rank's keys.  Three steps, two all-gathers:
 *   1. every shard reduces its positions to xmin[3] / xmax[3] (integer atomic min / max on the
 *      order-preserving u64 image of a double), its count and its smallest / largest time bin; one 128-byte
 *      block per rank is all-gathered.  find_extent: DomainLen = 1.001 max_j(xmax_j - xmin_j), DomainCenter_j =
 *      0.5 (xmin_j + xmax_j), DomainCorner_j = DomainCenter_j - 0.5 DomainLen (domain.c:1972-2014);
 *   2. every shard adds the INTEGER weight of each of its particles into a u64 histogram over the 8^level
 *      cells of the Peano-Hilbert curve in that cube; the histograms are all-gathered (8^level x 8 bytes per
 *      rank).  use_work = 0: w = 1.  use_work = 1: domain_particle_costfactor (domain.c:378-384) times
 *      2^bmax, w = ((1 + GravCost) << (bmax - b)) >> s, at least 1, with b = TimeBin ? TimeBin : 29, bmin /
 *      bmax the smallest / largest b of the run and s = max(0, (bmax - bmin) + 32 + ceil(log2 N) - 63) so that
 *      no sum leaves 64 bits.  A common power of two does not move a cut, and integer sums do not depend on
 *      the order in which they are formed;
 *   3. the histograms are added, converted to double and cut by ghip_dd_find_split; splits[r] = first cell of
 *      rank r << (63 - 3 level).
 * Afterwards every rank holds the same splits (one range per rank: a ghip_dd_set_segments layout is replaced)
 * and the same cube (ForceSoftening is kept); the trees, a kept geometry and the result of GHIP_DD_POTENTIAL
 * are discarded as ghip_dd_set_splits / ghip_dd_set_domain / GHIP_DD_MIGRATE discard them.  No particle
 * moves: run GHIP_DD_MIGRATE next, as after a drift.  A position that is not finite, a TimeBin outside
 * [0, 29] or a negative GravCost under use_work, no particle at all, an extent of length 0, or (find_extent =
 * 0) a particle outside the kept cube make ALL ranks return GHIP_EINVAL with the same message after the first
 * all-gather; nothing is changed then.  So does a failure of one rank's own first pass (that rank returns its
 * own code and message, the others GHIP_EDEVICE naming it).
 * Precondition, as for every ghip_dd_begin: ghip_dd_set_domain has been called once, also when find_extent = 1
 * -- ForceSoftening reaches the context only there; the cube given may be any (it is replaced). */
#define GHIP_DD_DECOMPOSE 13
typedef struct
{
  int level;        /* histogram level L: the curve is cut on 8^L cells.  0: about 32 particles of the whole
                     * run per cell (L = 1..7), raised until 8^L >= nranks.  Otherwise 1..7; GHIP_EINVAL if
                     * 8^L < nranks */
  int use_work;     /* 0: every particle weighs 1.  1: domain_particle_costfactor */
  int find_extent;  /* 0: keep the cube of ghip_dd_set_domain (periodic runs).  1: domain_findExtent over all
                     * ranks first */
  int reserved;
} ghip_dd_decomp_params;
/* pm_init_regionsize on shards (params: const int *pmgrid): every shard reduces its own positions, one
 * 128-byte block per rank (the six extremes, the count, the status) is all-gathered and every rank evaluates
 * the same blocks in rank order -- the reference's MPI_Allreduce (:118-119) -- and stores the same region,
 * bit for bit the one ghip_pm_find_region gives for all particles in one context.  An empty shard contributes
 * +MAX / -MAX.  The refusals of ghip_pm_find_region are GHIP_EINVAL with the same message on every rank. */
#define GHIP_DD_PM_REGION 14
/* pmforce_nonperiodic on shards (params: ghip_pmnp_params): every shard checks its own particles against the
 * region and deposits them into the COMPACT lower octant, PMGRID^3 doubles; the octants and one 8-byte status
 * word each are all-gathered (8 PMGRID^3 + 8 bytes per shard, not the padded mesh), added in rank order,
 * scattered into the zeroed padded mesh and solved on every shard, which reads out its own particles.  A
 * particle outside the region on ANY shard makes EVERY shard return GHIP_EREGION, nothing written anywhere. */
#define GHIP_DD_PM_NONPERIODIC 15
/* The wind particles on multi-GPU shards (GHIP_DD_WIND begun with one of the three wind forms as `walk`, through
 * ghip_dd_begin / ghip_dd_run): the loop of
 * momentum_feedback() under NTask > 1 (momentum_feedback.c:301, 469-470 all-reduce dt_total and N_active;
 * virtual_density.c:236-361 and virtual_spread_momentum.c export a particle to the tasks its sphere touches).
 * No operation code is added: the codes stay 1..15 and 16 stays unknown to ghip_dd_begin, as the friends-of-friends
 * groups and the sync point took a form of an existing operation.  GHIP_DD_WIND is the operation whose requirements
 * the wind shares, GHIP_DD_DUST_DRAG, and `walk` selects the form (its traffic counter serves whichever form ran
 * last):
 *   GHIP_WIND_FORM           the whole loop (:283-568), as ghip_wind_feedback
 *   GHIP_WIND_DENSITY_FORM   one virtual_density():         in dt_jump, out new_density, drmin
 *   GHIP_WIND_SPREAD_FORM    one virtual_spread_momentum(): in dt_jump, new_density, delta_momentum
 * (GHIP_WIND_FORM + 0, 1, 2; walk = 0 and GHIP_DUST_GRAINS_FORM stay the dust drag's, any other walk is GHIP_EINVAL).
 * Needs GHIP_DD_GRAVITY and GHIP_DD_DENSITY of this step: the list is ordered by
 * the gravity tree and the walks run on the shard's gas tree.  Arrays describe the wind particles resident on
 * THIS shard; a wind particle stays resident on its home shard for the whole call, wherever it flies, and the gas
 * neither moves nor changes mass.  Every shard takes every exchange, with or without wind or gas of its own.
 *   begin     one all-gather: the group boxes of the shard's Type-0 particles with Mass > 0, its largest h_j,
 *             its dt_jump sum and its list length.  The dt_jump sums are added in ascending rank order and
 *             compared with p->dt_total_floor, the GLOBAL floor: at or below it every shard returns having
 *             changed nothing.
 *   per iteration, four exchanges:
 *     1. the move of the own list and the own density partial over the shard's own gas; then {Pos, Hsml} of the
 *        listed particles with dt_jump > 0 go to every other shard whose gas boxes their sphere can reach (the
 *        radius is cut to what can still change new_density or drmin once the own pass found a candidate);
 *     2. every shard evaluates what it imported against its own gas; {new_density, drmin} partials go home,
 *        where new_density = own + partials in ascending rank order (virtual_density.c:344) and drmin = the
 *        minimum of all;
 *     3. the new list (dt_jump > 0); {list length, particles above 1e-40, failure} of every shard are
 *        all-gathered: the loop ends when no shard has a particle above 1e-40 (:470-472), and max_iter counts
 *        the global iterations, so all shards stop together (GHIP_ENOCONV);
 *     4. {new_density, DeltaPhotonMomentum, Vel, |Vel|} of the exported particles go to the same shards, and
 *        every shard scatters into its own Injected_BH_Momentum: a gas particle takes this shard's wind
 *        particles in list order, then the imported ones by sending rank ascending and within a rank by the
 *        sender's local particle index ascending (the dust drag's rule).  No floating-point atomics.
 *   end       RAD_ACCEL for the shard's active gas (ghip_set_active) and the elimination, locally.
 * result->iterations is the global count; bits, ndeleted and deleted_momentum are THIS shard's: the host adds
 * them in rank order where the reference all-reduces (:572-573).  A failure on one shard (an index that is not
 * Type 3, a list length that makes no sense) ends the operation on all shards in the same step.  Afterwards a
 * wind particle may lie outside its shard's key ranges or outside the domain cube: the operation reads no keys
 * and does not mind; the host runs GHIP_DD_DECOMPOSE / GHIP_DD_MIGRATE next, or accepts guests
 * (ghip_dd_set_guests). */
typedef struct
{
  const ghip_wind_params *p;
  int nwind;                       /* wind particles resident on this shard */
  const int *wind_idx;             /* their local particle indices, in active-list order */
  const ghip_wind_state *state;    /* WIND_FORM: as ghip_wind_feedback takes it */
  const double *dt_jump;           /* the single passes, in [nwind] */
  double *new_density;             /* DENSITY_FORM out, SPREAD_FORM in [nwind] */
  double *drmin;                   /* DENSITY_FORM out [nwind] */
  const double *delta_momentum;    /* SPREAD_FORM in [nwind] */
  ghip_wind_result *result;        /* WIND_FORM */
  long long *counts;               /* out [6] (may be NULL): records this shard sent, records it received, pairs it
                                      scattered for imported particles, exchanges run, bytes sent, iterations */
} ghip_dd_wind_args;
size_t ghip_dd_wind_args_size(void);
#define GHIP_DD_WIND GHIP_DD_DUST_DRAG   /* with one of the following as `walk` */
#define GHIP_WIND_FORM 16           /* `walk` of ghip_dd_begin / ghip_dd_run for GHIP_DD_WIND: the whole loop */
#define GHIP_WIND_DENSITY_FORM 17
#define GHIP_WIND_SPREAD_FORM 18
/* The resident wind particles on shards ("Resident, on shards").  The wind table of a shard:
 * ghip_dd_winds_set_table / _get_table / _clear for a ghip_dd_init context of ANY rank count; idx holds LOCAL particle
 * indices of the shard.  The refusals are those of the single-rank functions (an index out of range, not Type 3,
 * given twice: no table; stale after ghip_set_counts with changed counts); on a plain context they are GHIP_EINVAL
 * and name the single-rank function, on a ghip_set_shard context GHIP_EINVAL.  ghip_rearrange and ghip_peano_order,
 * which are local on a ghip_dd_init context, carry the table as on one GPU.
 * GHIP_DD_MIGRATE carries it too.  A migration renumbers the shard (kept gas, received gas, kept others, received
 * others), so a row of a particle that stays is re-keyed to its particle's new index, and a row of a Type-3 particle
 * that leaves travels, in one more all-to-all-v after the particles', as its particle's ordinal in the sender's run
 * for that destination plus the GHIP_WK_COUNT doubles (88 bytes); the receiver keys it by the new index of the
 * particle at that ordinal, and the table is sorted again.  A departing Type-3 particle without a row departs
 * without one; an arrival without a record has no row.  The header record of the particles' exchange says which
 * tables the sender holds: either all shards hold a wind table (an empty one counts) or none does, else every shard
 * returns GHIP_EINVAL before anything moved -- independently of the same rule for the sink tables.  Exchanges of a
 * migration: 1 without tables, 2 with wind tables, 3 with sink tables, 4 with both.  A stale table is not carried
 * and stays refused. */
int ghip_dd_winds_set_table(ghip_ctx *ctx, int nwind, const int *idx, const double *rows);
int ghip_dd_winds_get_table(ghip_ctx *ctx, int *nwind, int *idx, double *rows);
int ghip_dd_winds_clear(ghip_ctx *ctx);
/* ghip_winds_feedback as a collective: GHIP_DD_WIND begun with walk = GHIP_WINDS_RESIDENT_FORM and params a
 * ghip_dd_winds_args.  Everything GHIP_WIND_FORM says holds -- the same kernels, the four exchanges per iteration,
 * the selection cut, the rank-order sums, the end --; only the source of the list and of the planes differs.  The
 * list is the device selection of ghip_winds_feedback over the shard's active list: Type 3, a row, StellarAge <
 * Time, in active-list order.  The in planes are gathered from the rows; at the end the out planes and the code of
 * the elimination are scattered back; a row that is not listed is not touched.  An active Type-3 particle without
 * a row on its shard, a shard without a table, or one with a stale table: GHIP_EINVAL on ALL shards in the same
 * step (the status record of the first all-gather carries it; the failing shard's message names the index and the
 * rank), every exchange up to there is taken, nothing has changed.  Blocking reads per shard: the words of the
 * selection with the list length replace the upload of the state; the rest is as GHIP_WIND_FORM.  The values are
 * bit for bit those of GHIP_WIND_FORM given the same lists and the rows' state. */
/* ghip_wind_spawn as a collective: GHIP_DD_WIND begun with walk = GHIP_WINDS_SPAWN_FORM and the spawn members of
 * the same struct (p, result and counts are not read).  The reference's creation is local per task
 * (momentum_feedback.c:70-246): the new particle is P[NumPart + stars_spawned] of the TASK, its ID the sink's ID +
 * that LOCAL index, only tot_spawned is all-reduced (:240), and endrun(8888) on any task ends all tasks.  So every
 * shard does what ghip_wind_spawn does, on its own sinks from its own sink table, with ONE all-gather of {spawned,
 * sinks emitting, new_wind_exact sum, failed} between the scan and the growth.  spawn->rnd_table / nrnd MUST be
 * given: ghip_dd_begin refuses a context with a table bound by ghip_set_rnd_table.  A shard without a sink table or
 * without a wind table (ghip_dd_winds_set_table; an empty one counts), with an active Type-5 particle without a
 * row, or with NumPart + spawned > MaxPart makes EVERY shard return GHIP_EINVAL in the same step -- the failing
 * shard's message says why and names its rank, the others name the shard -- and no shard has changed a byte.
 * Otherwise each shard grows and fills locally: *report is the shard's own (first_index: its NumPart before),
 * *tot_spawned the sum over all shards, the same on all of them, for All.TotNumPart.  A shard that spawns nothing
 * changes nothing but takes the exchange.  The form does not ask for the trees of the step; on a shard that
 * spawned, both trees are gone afterwards, as on one GPU.  A new particle stands where its sink stands, inside the
 * shard's key range: no migration is implied. */
typedef struct
{
  const ghip_wind_params *p;       /* RESIDENT_FORM */
  ghip_wind_result *result;        /* RESIDENT_FORM: this shard's, as GHIP_WIND_FORM leaves it */
  long long *counts;               /* RESIDENT_FORM: out [6] (may be NULL), as ghip_dd_wind_args.counts */
  const ghip_wind_spawn_params *spawn;   /* SPAWN_FORM, with rnd_table / nrnd */
  ghip_wind_spawn_report *report;        /* SPAWN_FORM: this shard's */
  long long *tot_spawned;                /* SPAWN_FORM: the sum over all shards */
} ghip_dd_winds_args;
size_t ghip_dd_winds_args_size(void);
#define GHIP_WINDS_RESIDENT_FORM 32 /* `walk` for GHIP_DD_WIND: the whole loop from the shard's wind table */
#define GHIP_WINDS_SPAWN_FORM 33    /* ... the creation of wind particles by the shard's massive sinks */
/* ghip_find_next_sync_point on shards: GHIP_DD_DECOMPOSE begun with walk = GHIP_SYNC_POINT_FORM and params a
 * ghip_sync_params (the result: ghip_dd_get_sync_point) -- the two things run() does between two steps share one
 * operation, as the two forms of the dust operations do; no operation code is added.  Every
 * shard recounts its own bins and all-gathers its 32 TimeBinCount words (256 bytes); the sums give every rank
 * the same Ti_next -- the MPI_Allreduce(MIN) of run.c:219: a rank that holds none of the earliest bin still
 * gets the global value --, the same mask, GlobNumForceUpdate and Flag_FullStep.  Each shard then selects its
 * own local indices, and one status round (16 bytes per rank) carries what it met: a TIMEBIN outside [0, 28]
 * on one shard makes every shard return GHIP_EINVAL, and no shard's list changes.  Ti_Current is checked by
 * ghip_dd_begin; nothing of the decomposition (ranges, cube, trees) is touched. */
#define GHIP_SYNC_POINT_FORM 1   /* `walk` of ghip_dd_begin / ghip_dd_run for GHIP_DD_DECOMPOSE */
int ghip_dd_get_sync_point(const ghip_ctx *ctx, ghip_sync_point *out);   /* of the last completed one */
/* the ranges (nranks+1 keys) and the cube in force: what ghip_dd_set_splits / ghip_dd_set_domain /
 * GHIP_DD_DECOMPOSE stored last.  ghip_dd_get_splits returns GHIP_EINVAL while a ghip_dd_set_segments layout is
 * in force (several pieces per rank are not nranks+1 keys). */
int ghip_dd_get_splits(const ghip_ctx *ctx, unsigned long long *splits);
int ghip_dd_get_domain(const ghip_ctx *ctx, double corner[3], double center[3], double *len);
/* bytes this shard sent over links in its last operation `op` (GHIP_DD_*), its own block excluded */
int ghip_dd_bytes_sent(const ghip_ctx *ctx, int op, long long *bytes);

/* ---- the path ---- */
int ghip_tree_build(ghip_ctx *ctx, const double DomainCorner[3], const double DomainCenter[3],
                    double DomainLen, const double ForceSoftening[6]);
/* ---- sub-steps on the tree of the last full build (the reference's dynamic tree update,
 * forcetree.c:1356-1651: force_drift_node, force_kick_node, force_finish_kick_nodes) ----
 * Without this, every ghip_tree_build builds the tree of the CURRENT positions -- a valid Barnes-Hut
 * tree, but not the one the reference walks on a sub-step (TreeReconstructFlag == 0): there the cells
 * are those of the last full build, a node's centre of mass has moved with its mass-weighted velocity
 * vs, its side length has grown by 2 vmax dt and the momentum of the kicked particles is folded into
 * vs.  With ghip_set_dynamic_tree(ctx, 1):
 *   ghip_tree_build        = a full build (force_treebuild); a copy of the gravity tree is kept with
 *                            vs and vmax per node
 *   ghip_advance_timesteps   records the velocity change of every particle it kicks and hands Mass dv
 *                            and max|Vel| to all ancestors (force_kick_node); a host that kicks itself
 *                            calls ghip_tree_kick_nodes(ctx, n, idx, dv[n][3]) after it has stored the
 *                            new velocities (ghip_set_field VEL)
 *   ghip_tree_substep(ctx, dt_drift)
 *                          = what gravity_tree() does with TreeReconstructFlag == 0: every node of the
 *                            kept tree goes from the previous sync point to this one (pending kicks
 *                            into vs, s += vs dt_drift, len += 2 vmax dt_drift; dt_drift = (Ti_Current
 *                            - Ti_previous) * Timebase_interval, or get_drift_factor in comoving runs)
 *                            and its particle elements take the resident POS / MASS (drift the
 *                            particles first: ghip_drift, without box wrapping -- the reference wraps
 *                            at domain decompositions only); the tree of the current positions is
 *                            rebuilt as well, for the target order and the gas tree (SPH neighbour sets
 *                            are geometric: they do not depend on the tree that finds them).
 *                            The gravity walks read the kept tree until the next ghip_tree_build.
 * All nodes move at once; the reference moves a node when a walk or a kick first meets it, which is
 * the same state up to the rounding of s += vs dt in one piece or several.  Not on a multi-GPU shard
 * and not with ADAPTIVE_GRAVSOFT_FORGAS. */
int ghip_set_dynamic_tree(ghip_ctx *ctx, int on);
int ghip_tree_substep(ghip_ctx *ctx, double dt_drift);
int ghip_tree_kick_nodes(ghip_ctx *ctx, int nkicked, const int *idx, const double *dv3);
/* the same when the resident VEL is not the kicked one yet: vmax[k] = max_j |P[idx[k]].Vel[j]| of the
 * new velocity travels with the kick (what force_kick_node computes itself, forcetree.c:1478-1480).
 * A particle listed twice hands up the sum of its kicks. */
int ghip_tree_kick_nodes_vmax(ghip_ctx *ctx, int nkicked, const int *idx, const double *dv3,
                              const double *vmax);
/* the kept tree in pre-order (tests): xm = (s or pos, mass), cl = (centre, len), ev = (vs, vmax),
 * lk = links; NULL = skip */
int ghip_tree_dump_dynamic(ghip_ctx *ctx, int *nelem, double *xm4, double *cl4, double *ev4, int *lk4);
/* ADAPTIVE_GRAVSOFT_FORGAS (the shipped Makefile bundle): on != 0 makes the gravitational softening
 * of a gas particle its Hsml instead of ForceSoftening[0], as a target (forcetree.c:1851-1856), as
 * a source (:2038-2058) and in the nodes' maxsoft (:705-726, 845-846), which then opens a node
 * whenever the target lies inside it (:2125-2139).  Implies UNEQUALSOFTENINGS.  The softenings are
 * captured by ghip_tree_build: call this before it (it invalidates a built tree). */
int ghip_set_adaptive_gravsoft(ghip_ctx *ctx, int on);
int ghip_ewald_init(ghip_ctx *ctx, double BoxSize);
/* host copy of the ewald table [3][65][65][65] already scaled by 1/BoxSize^2 */
int ghip_ewald_get_table(ghip_ctx *ctx, double *host);
/* walk kind: GHIP_WALK_*.  Results: GRAVACCEL (G-less, as gravtree.c:381-393 expects) and
 * GRAVCOST of the active particles.  The EWALD walk adds to both. */
int ghip_gravity(ghip_ctx *ctx, const ghip_grav_params *p, int walk);
/* external targets (the mode==1 gravdata_in record, allvars.h:1690-1703): coordinates, type,
 * OldAcc in; Acc[3], Ninteractions out; all host arrays */
int ghip_gravity_ext(ghip_ctx *ctx, const ghip_grav_params *p, int walk, int nt,
                     const double *pos, const int *type, const double *oldacc, double *acc,
                     int *ninteractions);
/* the post-pass of gravity_tree() over the active particles, in the reference's order
 * (gravtree.c:362-403):
 *   comoving_fac != 0 : GravAccel += comoving_fac * Pos, with comoving_fac = 0.5 * Hubble^2 *
 *                       Omega0 / G -- the term of comoving runs built without PERIODIC and PMGRID
 *                       (:362-373); pass 0 otherwise
 *   OldAcc = |GravAccel|; pmgrid != 0: |GravAccel + GRAVPM / G| (:375-391, the relative opening
 *                       criterion of a TreePM run sees the total acceleration)
 *   GravAccel *= G      (:398-403)
 * all_shards != 0: every active target regardless of ghip_set_shard (replicated multi-GPU mode,
 * after the all-gather). */
int ghip_gravity_finish_ex(ghip_ctx *ctx, double G, int pmgrid, double comoving_fac,
                           int all_shards);
/* = ghip_gravity_finish_ex(ctx, G, 0, 0, 0) / (ctx, G, 0, 0, 1): builds without PMGRID that are
 * periodic or not comoving */
int ghip_gravity_finish(ghip_ctx *ctx, double G);
int ghip_gravity_finish_all(ghip_ctx *ctx, double G);
/* GravAccel += fac * Pos for all active particles, fac = OmegaLambda * Hubble^2: the vacuum-energy
 * term of runs in physical coordinates (gravtree.c:470-483, !PERIODIC && !PMGRID &&
 * ComovingIntegrationOn == 0); call it after ghip_gravity_finish */
int ghip_gravity_vacuum_energy(ghip_ctx *ctx, double fac);
/* the same with gravdata_in.Soft (allvars.h:1695, gravtree.c:214-220): soft[a] = Hsml of a gas
 * target, used when ghip_set_adaptive_gravsoft is on; NULL = ghip_gravity_ext */
int ghip_gravity_ext_soft(ghip_ctx *ctx, const ghip_grav_params *p, int walk, int nt,
                          const double *pos, const int *type, const double *soft,
                          const double *oldacc, double *acc, int *ninteractions);
/* softened direct summation over all particles for the active targets (accuracy oracle on
 * device, formula of forcetree.c:4273-4336); writes GRAVACCEL */
int ghip_gravity_direct(ghip_ctx *ctx, const ghip_grav_params *p);
int ghip_density(ghip_ctx *ctx, const ghip_dens_params *p);
int ghip_update_hmax(ghip_ctx *ctx);
int ghip_hydro(ghip_ctx *ctx, const ghip_hydro_params *p);
/* -DBLACK_HOLES / -DDUST builds: a gas particle of mass 0 (swallowed, waiting for the next
 * rearrange_particle_sequence) is skipped by the neighbour loop of density() (rule 1: -DDUST or
 * -DBLACK_HOLES, density.c:831-834) and also by hydro_force()'s (rule 3: -DBLACK_HOLES,
 * hydra.c:1235-1238); it stays a target.  0 (default): the builds without these flags sum it with
 * weight 0 but count it in NumNgb.  Independent of this switch a record of the gas block whose Type is
 * not 0 is never a target or a neighbour, as in the reference's loops. */
int ghip_set_massless_gas_rule(ghip_ctx *ctx, int rule);
/* When ghip_hydro is called underneath a GHIP_WALK_NEWTON_EWALD pair in flight, its kernel is held
 * back on the device until the Ewald walk drains (fastest step for resident data).  early != 0: it
 * starts at once -- the step's kernels take 0.2 ms longer at c2, but a host that downloads the SPH
 * results gets them across while the walks still run. */
int ghip_set_hydro_release(ghip_ctx *ctx, int early);
/* ---- the artificial viscosity of the pair loop beyond the constant All.ArtBulkViscConst of
 * ghip_hydro_params: -DTIME_DEP_ART_VISC (Morris & Monaghan: every gas particle has its own alpha with a
 * source in compressions and a decay elsewhere) and the three uniform switches of hydra.c:1512-1595.  A
 * setting of the context, for ghip_hydro, GHIP_DD_HYDRO and ghip_advance_timesteps alike:
 *   ghip_hydro   BulkVisc_ij = (alpha_i + alpha_j) / 2 (hydra.c:1541-1545); under `conventional` the
 *                mu_ij of :1516-1518 also enters vsig (:1520), so MAXSIGNALVEL changes with it; the
 *                post-pass writes Dtalpha of the call's targets (hydra.c:735-744, evaluated with
 *                v.DivVel / r.CurlVel: the u.s.* members the reference names exist only under
 *                -DNAVIERSTOKES), non-targets keep theirs
 *   ghip_advance_timesteps   alpha += Dtalpha dt_entr, clamped to [AlphaMin, ArtBulkViscConst]
 *                (timestep.c:530-533), for the active Type 0 records of the gas block; ghip_pm_kick
 *                leaves alpha alone
 * The alpha a hydro call uses is the one held when it is called, also on a tree kept across kicks
 * (ghip_set_dynamic_tree).  p == NULL or all four switches 0: the default kernels, nothing allocated.
 * Not built: -DALTVISCOSITY, -DALTERNATIVE_VISCOUS_TIMESTEP, -DNAVIERSTOKES, -DHIGH_ART_VISC_START (the
 * host sets its initial alpha itself).
 * GHIP_EINVAL, before anything is launched: a value that is not finite; AlphaMin < 0 or
 * > ArtBulkViscConst; a context of ghip_set_shard (use the ghip_dd_* contexts); ghip_hydro /
 * GHIP_DD_HYDRO / ghip_advance_timesteps with time_dependent set and no alpha given since
 * ghip_set_counts last changed the counts; ghip_visc_get without alpha.
 * On ghip_dd_* contexts the setting must be the same on all ranks (the caller's duty: nothing checks it);
 * a ghost carries its owner's alpha as of the GHIP_DD_DENSITY before, in the record it has always had --
 * no byte more on the links -- so alpha is set before GHIP_DD_DENSITY: a GHIP_DD_HYDRO on more than one
 * rank after alpha changed since (ghip_visc_set_alpha, a kick) is GHIP_EINVAL, not a pair of two epochs;
 * every shard computes Dtalpha for its own targets. ---- */
typedef struct
{
  int time_dependent;     /* TIME_DEP_ART_VISC: BulkVisc_ij = (alpha_i + alpha_j) / 2  (hydra.c:1541-1545) */
  int conventional;       /* CONVENTIONAL_VISCOSITY: mu_ij, visc of hydra.c:1516-1518, 1549-1551 */
  int no_limiter;         /* NOVISCOSITYLIMITER: skip hydra.c:1583-1595 */
  int no_shear_limiter;   /* NO_SHEAR_VISCOSITY_LIMITER: f1 = f2 = 1 (hydra.c:1538-1540) */
  double ArtBulkViscConst;/* upper clamp of alpha in the kick (timestep.c:531) */
  double AlphaMin, ViscSource, DecayTime;   /* All.* after begrun.c:132-133 */
  double dtalpha_comoving_div;  /* hubble_a * All.Time^2 (hydra.c:742-743); read only when the hydro call is comoving */
} ghip_visc_params;
int ghip_set_viscosity(ghip_ctx *ctx, const ghip_visc_params *p);     /* NULL: everything off (the default path) */
/* SphP[].alpha / SphP[].Dtalpha of the resident gas, [ngas] in host order (a shard's own gas in its
 * order); dtalpha NULL: zeros.  Resident next to the GHIP_F_* fields from the first call on. */
int ghip_visc_set_alpha(ghip_ctx *ctx, const double *alpha, const double *dtalpha);
int ghip_visc_get(ghip_ctx *ctx, double *alpha, double *dtalpha);     /* either may be NULL; synchronises */
/* All.ViscSource = ViscSource0 / log((GAMMA + 1) / (GAMMA - 1)), All.DecayTime = 1 / DecayLength *
 * sqrt((GAMMA - 1) / 2 * GAMMA): begrun.c:132-133 as written, GAMMA = 7 / 5.  Host arithmetic. */
void ghip_visc_derive(double ViscSource0, double DecayLength, double *ViscSource, double *DecayTime);
size_t ghip_visc_params_size(void);   /* sizeof(ghip_visc_params) of the library, for bindings to check */

/* ---- Randomised subnodes for (near-)coincident particles: the reference without -DNOTREERND
 * (forcetree.c:219-232, 303-316; system.c:161-172).  In a node whose side is below
 * 1.0e-3 * ForceSoftening[Type] a particle's subnode is not taken from its position but is
 *   min(7, (int) (8.0 * table[((ID + d) % (ntable + (d & 3))) % ntable]))
 * with d the depth of the node (the root: 0) and ID + d in unsigned 32-bit arithmetic; below level 21 a
 * position is compared with the node's centre (forcetree.c:208-217).  The table is copied to the device by
 * this call (the host refills its RndTable every step: call it before every ghip_tree_build); IDs are the
 * GHIP_F_ID field; the thresholds are the ForceSoftening of ghip_tree_build, also with
 * ghip_set_adaptive_gravsoft.  Both trees follow the rule.  A particle's path through the tree then has
 * GHIP_TREE_MAXLEVEL digits: node levels 0 .. GHIP_TREE_MAXLEVEL - 1.  Two sources that share every one of
 * them make the build fail with GHIP_EDEVICE ("tree error"); the context stays usable.
 * table == NULL (or ntable == 0) unbinds: identical Morton keys become one level-21 leaf, and every launch and
 * result is that of a library without this call.  Entries must lie in [0, 1).
 * Not on domain-decomposed shards: ghip_dd_begin is GHIP_EINVAL while a table is bound. ---- */
#define GHIP_TREE_MAXLEVEL 42
int ghip_set_rnd_table(ghip_ctx *ctx, const double *table, int ntable);
int ghip_tree_max_level(void);   /* GHIP_TREE_MAXLEVEL of the library */

/* one fixed-h evaluation for a single target (density_evaluate mode 0, density.c:711):
 * out7 = rho, numngb, dhsmlrho, divv, rot[3] (raw sums, before finalisation) */
int ghip_density_evaluate(ghip_ctx *ctx, const ghip_dens_params *p, int target, double h,
                          double out7[7]);
/* neighbour lists for one search centre (ngb_treefind_variable / _pairs, ngb.c:169, 32):
 * writes up to cap host indices, returns the count in *nfound */
int ghip_ngb_treefind(ghip_ctx *ctx, const double center[3], double hsml, int pairs,
                      int periodic, double boxsize, int *ngblist, int cap, int *nfound);
/* diagnostic: one device primitive on n >= 1 host ints, on the main stream; out holds n ints.  prim:
 *   0, 1  out = exclusive sums of in (the scan library's form, the one-wavefront form)
 *   2, 3  out = the in[a] with flags[a] != 0, in order (in == NULL: the indices a), *count = their number (same two forms)
 *   4     out = the permutation that sorts the keys in (unsigned, below 2^end_bit) stably */
enum { GHIP_PRIM_SCAN, GHIP_PRIM_WSCAN, GHIP_PRIM_SELECT, GHIP_PRIM_WSELECT, GHIP_PRIM_SORT_U32 };
int ghip_debug_prim(ghip_ctx *ctx, int prim, int n, int end_bit, const int *in, const int *flags,
                    int *out, int *count);

/* ---- keys (peano.c:300-358), device evaluation of n integer triplets ---- */
int ghip_peano_hilbert_keys(ghip_ctx *ctx, int n, const int *x, const int *y, const int *z,
                            int bits, unsigned long long *keys);
int ghip_morton_keys(ghip_ctx *ctx, int n, const int *x, const int *y, const int *z, int bits,
                     unsigned long long *keys);

/* ---- a resident step loop that never waits for the device (run.c:40-155 with P / SphP in HBM) ----
 * ghip_set_async(ctx, 1): ghip_drift and ghip_advance_timesteps (called with NULL count arrays)
 * return without waiting; what they would have reported -- the reference's endrun(12) of a particle
 * ahead of the drift target, endrun(888|818|112313) of a failed timestep criterion -- is reported
 * with the same codes by the next entry point that synchronises (ghip_sync, ghip_get_field, the
 * h iteration of ghip_density, ...).  ghip_tree_build needs no switch: whenever the particle number
 * equals the previous build's it is enqueued without waiting for the node counts, and the counts
 * are verified before anything persistent is modified on their basis (a build that overflowed its
 * buffers is repeated and the gravity calls made since are replayed: same results, later).
 * With both, the host enqueues a step while the device still works on the previous one; the only
 * wait left in a step with gas is the h iteration's unconverged count, which is read underneath
 * the gravity walks. */
int ghip_set_async(ghip_ctx *ctx, int on);

/* statistics of a run of steps without a host synchronisation per step: the library keeps one set
 * of phase events per step and sums its device counters on the device.
 *   ghip_run_begin(ctx, max_steps);  { ghip_step_begin(ctx); <the calls of a step>; ghip_step_end(ctx); } ...
 *   ghip_run_end(ctx, &stats)        -- synchronises once */
typedef struct
{
  long long steps;             /* ghip_step_end calls */
  long long steps_timed;       /* of them, with events kept (the last max_steps) */
  long long launches;          /* kernel launches issued by the library (its own and rocPRIM's) */
  long long blocking_syncs;    /* host waits for the device inside the library */
  long long grav_interactions, ewald_interactions, dens_neighbours, hydro_pairs;
  long long grav_wave_steps, ewald_wave_steps, dens_extra_iterations;
  double ms_tree, ms_grav, ms_ewald, ms_dens, ms_hmax, ms_hydro, ms_kick;   /* summed device spans */
  double ms_steps_device;      /* sum over steps of (step begin mark -> step end mark), device clock */
  double ms_between_steps;     /* sum of (end mark of step k -> begin mark of step k+1): the device
                                * waiting for the host between steps */
  double ms_first_to_last;     /* begin mark of the first timed step -> end mark of the last */
} ghip_run_stats;
int ghip_run_begin(ghip_ctx *ctx, int max_steps);
int ghip_step_begin(ghip_ctx *ctx);
int ghip_step_end(ghip_ctx *ctx);
int ghip_run_end(ghip_ctx *ctx, ghip_run_stats *out);

/* ---- friends-of-friends groups (fof_fof, fof.c:94-333; ghip_fof.hip) ----
 * ghip_fof finds the FOF groups of the resident state on the gravity tree of the current positions
 * (ghip_tree_build; no tree is built here):
 *   linking      two particles of a primary type are linked when their nearest-image distance satisfies
 *                r2 <= LinkL^2 (ngb_treefind_fof_primary, ngb.c:351-368: equality links); the groups are the
 *                connected components (fof_find_groups, fof.c:337-706), labelled with their smallest ID
 *   secondaries  a particle of a secondary type (and of no primary type) takes the label of the nearest primary
 *                with r2 < h^2; h starts at Hsml for gas and at 0.1 LinkL otherwise and is doubled while nothing
 *                is found, at most MaxIter times (GHIP_ENOCONV then: endrun(1159)); fof.c:1434-1776.  Equally
 *                distant primaries: the one with the smaller ID (the reference keeps the first in traversal order)
 *   catalogue    a group is the set of all particles with one label (a particle of neither kind is a group of
 *                its own, as in the reference); kept with Len >= group_min_len, ordered by Len descending, then
 *                MinID ascending; GrNr = 0 .. Ngroups-1, Offset the running sum of Len (fof.c:710-974, 1081-1119).
 *                CM: periodic, the mass-weighted nearest images about the member that carries MinID, wrapped into
 *                [0, BoxSize); else the mass-weighted mean.  MaxDens / index_maxdens: the gas member (Type 0)
 *                of largest GHIP_F_DENSITY > 0, ties to the smaller particle index; -1 without one.
 * Sums are taken in a fixed order without floating-point atomics: two calls on one state give identical bytes.
 * Sfr, BH_Mass and BH_Mdot are no resident fields: they stay with the host, which has the member list.
 * GHIP_EINVAL: no tree built, GHIP_F_ID never set, no particle of a primary type, a domain decomposition on
 * (groups that span shards are found by the collective form below).  Duplicate IDs are outside the contract, as under the reference's
 * IGNORE_NON_UNIQUE.  The getters return what the last successful ghip_fof of this context found. */
typedef struct {
  double LinkL;          /* > 0: taken as is.  <= 0: LINKLENGTH rule of fof.c:112-124, computed on the device:
                            linklength * pow(masstot / ndmtot / rhodm, 1/3) over the primary types */
  double linklength;     /* LINKLENGTH (0.2), used when LinkL <= 0 */
  double rhodm;          /* (Omega0 - OmegaBaryon) * 3 H^2 / (8 pi G), host-computed, used when LinkL <= 0 */
  int primary_types;     /* FOF_PRIMARY_LINK_TYPES, bit mask of 1 << Type */
  int secondary_types;   /* FOF_SECONDARY_LINK_TYPES; 0 = none */
  int group_min_len;     /* GROUP_MIN_LEN (32) */
  double BoxSize; int periodic;
  int MaxIter;           /* MAXITER (150) of the nearest-primary search */
} ghip_fof_params;

typedef struct { int Ngroups; long long Nids; int largest; double LinkL; int nearest_iterations; } ghip_fof_result;

typedef struct {          /* struct group_properties, fof.h:26-60, the members the resident state can fill */
  int Len, Offset, MinID, GrNr, LenType[6];
  double MassType[6], Mass, CM[3], Vel[3];
  double MaxDens; int index_maxdens;      /* densest gas member (fof.c:950-961); -1 = no gas member */
} ghip_fof_group;

int ghip_fof(ghip_ctx *ctx, const ghip_fof_params *p, ghip_fof_result *out);
int ghip_fof_get_groups(ghip_ctx *ctx, ghip_fof_group *groups /* [Ngroups] */);
int ghip_fof_get_ids(ghip_ctx *ctx, int *ids /* [Nids], sorted by (GrNr, ID): fof_compare_ID_list_GrNrID */);
int ghip_fof_get_labels(ghip_ctx *ctx, int *minid /* [n] */, int *grnr /* [n]; -1 = in no kept group */);
size_t ghip_fof_params_size(void);
size_t ghip_fof_group_size(void);   /* for the bindings' ABI check */
/* device milliseconds of the last ghip_fof: linking, flattening + labels, secondary rounds, catalogue */
int ghip_fof_get_timing(ghip_ctx *ctx, double ms[4]);

/* On domain-decomposed shards ghip_fof is refused; the groups of the WHOLE system are found by the collective
 *   ghip_dd_begin / ghip_dd_run(ctx, GHIP_DD_GLOBAL_QUANTITIES, &ghip_dd_fof_args, GHIP_FOF_FORM)
 * on the merged gravity tree of this step's GHIP_DD_GRAVITY (GHIP_EINVAL without it, or with the tree that
 * GHIP_DD_POTENTIAL leaves behind); no tree is built, no resident field changed.  Own primaries are linked on the
 * merged tree; primaries within LinkL of another shard's primary boxes travel there once as (x, y, z, label), are
 * linked against that shard's tree by the same pair test, and labels (MinID, MinIDTask) are exchanged along the
 * same lists until none falls (fof.c:416-583).  A secondary asks every shard whose primaries its sphere reaches
 * and takes the smallest (r2, ID) (fof.c:1434-1776).  Partial group records go to MinIDTask, are added there in
 * rank order (fof.c:977-1119), and the kept groups are gathered and ordered on every shard.  Afterwards, on every
 * shard: ghip_fof_get_groups -> the complete catalogue, identical bytes everywhere (index_maxdens: the local index
 * on the shard ghip_fof_get_maxdens_task names; ties of MaxDens to the lower rank, then the smaller index);
 * ghip_fof_get_labels -> MinID and global GrNr of the shard's own particles; ghip_fof_get_ids -> the IDs of its own
 * members of kept groups by (GrNr, ID), counts[0] of them; ghip_fof_get_timing -> this shard's device time,
 * exchanges excluded.  No floating-point atomics: two runs give identical bytes.  Errors every shard sees alike
 * (NULL members, the parameter rules of ghip_fof, GHIP_F_ID never set) come from ghip_dd_begin; "no primary on any
 * shard" (GHIP_EINVAL), more than MaxIter doublings (GHIP_ENOCONV) and labels that do not settle (GHIP_EDEVICE)
 * stop all shards together, which stay usable. */
typedef struct {
  const ghip_fof_params *p;   /* the same values on every rank */
  ghip_fof_result *out;       /* Ngroups, Nids, largest: of the WHOLE system; LinkL; nearest_iterations: rounds of the
                                 collective search.  The same bytes on every rank */
  long long *counts;          /* may be NULL; [8]: own members of kept groups (= entries of ghip_fof_get_ids), primaries
                                 sent, primaries received, label rounds, secondary queries sent (all rounds),
                                 partial group records sent, bytes sent, kept groups this rank owns (MinIDTask) */
} ghip_dd_fof_args;
/* the shard whose local index index_maxdens is (task_maxdens, fof.h:46); without a decomposition 0 where
 * index_maxdens >= 0 */
int ghip_fof_get_maxdens_task(ghip_ctx *ctx, int *task /* [Ngroups]; -1 = no gas member */);
size_t ghip_dd_fof_args_size(void);

/* ---- the particle sequence: rearrange_particle_sequence() and peano_hilbert_order() on the device ----
 * What domain_Decomposition() runs around its cut (domain.c:120-135, 281-285), for a resident run whose passes
 * leave Mass == 0 records (ghip_blackhole_swallow, the wind loop) and Type != 0 records inside the gas block
 * (ghip_sfr_cooling, sinks formed from ghip_fof groups).
 *
 * ghip_rearrange (sfr_eff.c:1018-1129) is an ORDER-PRESERVING compaction.  The new layout: the gas survivors in
 * their old order, then (fix_converted) the records of the old gas block whose Type is not 0, in their old
 * order, then the other survivors in their old order; eliminate_massless drops every record with Mass == 0,
 * whatever its type.  With both set the gas block afterwards is exactly {Type == 0, Mass != 0} of the old gas
 * block.  A converted record keeps its per-particle fields and drops its per-gas ones.  This is the -DDUST
 * build's behaviour, the only one built: without -DDUST the reference counts a massless record that is not gas
 * and leaves it in place.  The reference's serial swap-from-the-end leaves another order; peano_hilbert_order()
 * follows it at domain.c:285 and its merge sort is stable, so after ghip_peano_order the two sequences differ
 * inside runs of equal keys at most.  count_gaselim counts eliminated Type 0 records, count_dustelim Type 2;
 * `converted` is counted on the device (there is no Stars_converted to pass, hence no endrun(181170)).
 *
 * ghip_peano_order (peano.c:25-185) sorts the gas block [0, ngas) and the block behind it separately, each
 * stably, by the key of ghip_dd_keys (domain.c's Key[i]: 21 bits per dimension in the cube DomainCorner,
 * DomainLen).  DomainCorner == NULL: on a ghip_dd_init context the domain of ghip_dd_set_domain /
 * GHIP_DD_DECOMPOSE (DomainLen is ignored), on any other context GHIP_EINVAL.  A position that is not finite or
 * lies outside [corner, corner + len) in a dimension: GHIP_EINVAL, nothing moved.  It sorts whatever types the
 * blocks hold (a mixed gas block is legal).
 *
 * With a record travel, bit for bit, in both calls: every GHIP_F_* field and every optional resident array held
 * for the current counts -- DragHeating, alpha and Dtalpha, Injected_BH_Momentum, RadAccel, SwallowID and
 * Injected_BH_Energy, DragAccel, DeltaDustMomentum and NewDensity of ghip_kick_set_fields.  An array held for
 * other counts is dropped, as by GHIP_DD_MIGRATE.  The wind table (ghip_winds_set_table), which is keyed by
 * particle index, follows: every index goes through new_of_old, the rows of eliminated particles are dropped and
 * the rows are put back in ascending index order.  A call that moved something leaves the rest of the state as
 * a migration does: both trees are gone, a kept tree (ghip_set_dynamic_tree) is refused until a full build, the
 * target lists and the active list are gone (everybody is active; ghip_find_next_sync_point makes the next list,
 * as reconstruct_timebins() at domain.c:305), the potential and the FOF labels are stale and refused.  Every
 * switch is kept.  A call that moved nothing (changed == 0) invalidates nothing.  Both calls wait for the
 * context's streams first; both are local on a ghip_dd_init context (no exchange) and GHIP_EINVAL on a
 * replicated shard (ghip_set_shard with nranks > 1).  The host mirror (gadget_force.h) has neither: a host that
 * owns P[] keeps its own functions. */
typedef struct {
  int fix_converted;        /* the -DSFR part, sfr_eff.c:1030-1053 */
  int eliminate_massless;   /* the -DBLACK_HOLES part with -DDUST, sfr_eff.c:1055-1095 */
} ghip_rearrange_params;
typedef struct {
  int numpart, ngas;        /* after the call */
  int converted;            /* records that left the gas block and survive */
  int count_elim, count_gaselim, count_dustelim;   /* this context's; a caller with shards adds them up */
  int changed;              /* 0: no record moved */
} ghip_rearrange_result;
int ghip_rearrange(ghip_ctx *ctx, const ghip_rearrange_params *p, ghip_rearrange_result *out);
int ghip_peano_order(ghip_ctx *ctx, const double DomainCorner[3], double DomainLen, int *changed);
/* the permutation of the last of the two calls (the identity when it moved nothing): new_of_old[n before the
 * call], -1 for an eliminated record; old_of_new[n after it].  Either may be NULL */
int ghip_sequence_get_map(ghip_ctx *ctx, int *new_of_old, int *old_of_new);
/* of the same call: {n before, n after (-1, -1: no call yet), bytes its move read and wrote, planes it moved} */
int ghip_sequence_get_info(ghip_ctx *ctx, long long out[4]);

/* ---- introspection ---- */
int ghip_get_stats(const ghip_ctx *ctx, ghip_stats *out);
/* tree dump for parity tests: the pre-order element list of the gravity tree (which = 0) or the
 * gas tree (which = 1): xm4 = (x,y,z,mass), cl4 = (centre, len), lk4 = (skip, particle index in
 * tree order or -(level+1), first particle, count), aux, and perm = tree order -> host index.
 * Pass NULL arrays to query *nelem only. */
int ghip_tree_dump(ghip_ctx *ctx, int which, int *nelem, double *xm4, double *cl4, int *lk4,
                   double *aux, int *perm);
/* device stream (hipStream_t) the kernels run on, for callers that time with HIP events */
void *ghip_stream(ghip_ctx *ctx);
int ghip_sync(ghip_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
