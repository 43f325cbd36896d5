/*
 * gadget_force.h -- host-side mirror of the reference's call surface for the force path.
 *
 * The reference host is plain C on global AoS arrays (allvars.h, proto.h, forcetree.h).  This
 * header restates exactly the part of that interface the force path touches, with the same
 * names, argument meaning and error behaviour, so that
 *   (a) accel.c (accel.c:27-313) can call gravity_tree() / density() / force_update_hmax() /
 *       hydro_force() unchanged, and
 *   (b) the parity tests read like tests of the reference's own functions.
 * Everything computes on the GPU through include/ghip.h; there is no CPU fallback.
 *
 * Struct layout: the MINIMAL periodic flag set of BASELINE.md (-DPERIODIC -DPEANOHILBERT
 * -DDOUBLEPRECISION ...: sizeof(particle_data) = 112, sizeof(sph_particle_data) = 184,
 * SURVEY.md 8b).  A host built with another -D set keeps its own allvars.h and passes its own
 * offsets through ghip_layout; nothing in libghip.so depends on this struct.
 *
 * Reference interfaces replaced (file:line):
 *   gravity_tree            gravtree.c:27        set_softenings        gravtree.c:835
 *   force_treebuild         forcetree.c:67       force_update_hmax     forcetree.c:1661
 *   force_treeevaluate      forcetree.c:1797     ..._shortrange        forcetree.c:2330
 *   ..._ewald_correction    forcetree.c:2873     ewald_init            forcetree.c:4402
 *   density                 density.c:89         density_evaluate      density.c:711
 *   density_isactive        density.c:1035       hydro_force           hydra.c:145
 *   hydro_evaluate          hydra.c:822          ngb_treefind_variable ngb.c:169
 *   ngb_treefind_pairs      ngb.c:32             peano_hilbert_key     peano.c:300
 *   morton_key              peano.c:320          domain_findExtent     domain.c:1972
 *   endrun                  endrun.c:23
 */
#ifndef GADGET_FORCE_H
#define GADGET_FORCE_H

#include "ghip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef double MyFloat;       /* DOUBLEPRECISION, allvars.h:154-165 */
typedef double MyDouble;
typedef double MyLongDouble;  /* no FLTROUNDOFFREDUCTION, allvars.h:191-202 */
typedef unsigned long long peanokey; /* allvars.h:55 */

#define BITS_PER_DIMENSION 21 /* allvars.h:58 */
#define NODELISTLENGTH 8
#define GAMMA (7. / 5.)       /* allvars.h:64 */
#define GAMMA_MINUS1 (GAMMA - 1)

/* allvars.h:1131-1377, minimal flag set: 112 bytes */
struct particle_data
{
  MyDouble Pos[3];
  MyDouble Vel[3];
  MyDouble Mass;
  unsigned int ID;
  union
  {
    MyFloat GravAccel[3];
    MyLongDouble dGravAccel[3];
  } g;
  MyFloat OldAcc;
  float GravCost;
  int Ti_begstep;
  int Ti_current;
  short int Type;
  short int TimeBin;
};

/* allvars.h:1384-1639, minimal flag set (+BH_THERMALFEEDBACK's `i`): 184 bytes */
struct sph_particle_data
{
  MyDouble Entropy;
  MyFloat Pressure;
  MyDouble VelPred[3];
  MyFloat MaxSignalVel;
  union
  {
    MyFloat Density;
    MyLongDouble dDensity;
  } d;
  union
  {
    MyFloat DtEntropy;
    MyLongDouble dDtEntropy;
  } e;
  union
  {
    MyFloat HydroAccel[3];
    MyLongDouble dHydroAccel[3];
  } a;
  union
  {
    MyFloat DhsmlDensityFactor;
    MyLongDouble dDhsmlDensityFactor;
  } h;
  union
  {
    MyFloat DivVel;
    MyLongDouble dDivVel;
  } v;
  union
  {
    MyFloat CurlVel;
    MyFloat Rot[3];
    MyLongDouble dRot[3];
  } r;
  MyFloat Hsml;   /* PPP == SphP when !BLACK_HOLES && !DUST, allvars.h:266-270 */
  MyFloat Left, Right;
  union
  {
    MyFloat NumNgb;
    MyLongDouble dNumNgb;
  } n;
  union
  {
    MyFloat Injected_BH_Energy;
    MyLongDouble dInjected_BH_Energy;
  } i;
  MyFloat pad_[2];
};

#define PPP SphP /* allvars.h:266-270 */

/* the members of `All` (struct global_data_all_processes, allvars.h:530-1123) the path uses */
struct global_data_all_processes
{
  int MaxPart;
  double G;
  double ErrTolTheta, ErrTolForceAcc;
  int TypeOfOpeningCriterion;
  double BoxSize;
  double DesNumNgb, MaxNumNgbDeviation;
  double MinGasHsmlFractional, MinGasHsml;
  double ArtBulkViscConst;
  int Ti_Current;
  double Timebase_interval;
  double Time;
  int ComovingIntegrationOn;
  double Hubble, Omega0, OmegaLambda; /* hubble_function(), darkenergy.c:389 (no DARKENERGY) */
  double SofteningGas, SofteningHalo, SofteningDisk, SofteningBulge, SofteningStars, SofteningBndry;
  double SofteningGasMaxPhys, SofteningHaloMaxPhys, SofteningDiskMaxPhys, SofteningBulgeMaxPhys,
    SofteningStarsMaxPhys, SofteningBndryMaxPhys;
  double SofteningTable[6], ForceSoftening[6];
  double Rcut[2], Asmth[2];           /* PMGRID */
  long long TotNumOfForces;
  int BunchSize;
  double BufferSize;
  /* "next" row N1: timestep criterion + kick (timestep.c) */
  double ErrTolIntAccuracy, CourantFac, MaxSizeTimestep, MinSizeTimestep, MaxRMSDisplacementFac;
  double OmegaBaryon, MinEgySpec;
  int TypeOfTimestepCriterion, StarformationOn;
  /* "next" row N4: the sink passes (blackhole.c, density.c BLACK_HOLES / DUST branches) */
  double BlackHoleNgbFactor, BlackHoleFeedbackFactor;
  double SMBHmass, InnerBoundary, SinkBoundary, CritOverDensity;
  double UnitLength_in_cm, UnitMass_in_g, UnitEnergy_in_cgs;
};

/* A host whose `All` is the reference's full struct (allvars.h:530-1123, ~300 members whose
 * layout depends on the -D flags) cannot share the subset above.  Like P[]/SphP[] (ghip_layout) it
 * hands over BYTE OFFSETS instead: gadget_force_bind_all(&All_of_the_host, &offsets) makes every
 * entry point of this library read the members below from the host's struct and write back the ones
 * the path changes (ErrTolTheta gravtree.c:396-397, TotNumOfForces :783, SofteningTable /
 * ForceSoftening / MinGasHsml :835-884).  One int per member, in the order of GADGET_FORCE_ALL_MEMBERS;
 * -1 = the host's build has no such member (the library keeps its own value, 0 unless set).
 * A probe TU fills the table with offsetof(struct global_data_all_processes, member), INTEGRATION.md. */
#define GADGET_FORCE_ALL_MEMBERS(X)                                                               \
  X(MaxPart) X(G) X(ErrTolTheta) X(ErrTolForceAcc) X(TypeOfOpeningCriterion) X(BoxSize)          \
  X(DesNumNgb) X(MaxNumNgbDeviation) X(MinGasHsmlFractional) X(MinGasHsml) X(ArtBulkViscConst)   \
  X(Ti_Current) X(Timebase_interval) X(Time) X(ComovingIntegrationOn) X(Hubble) X(Omega0)        \
  X(OmegaLambda) X(SofteningGas) X(SofteningHalo) X(SofteningDisk) X(SofteningBulge)              \
  X(SofteningStars) X(SofteningBndry) X(SofteningGasMaxPhys) X(SofteningHaloMaxPhys)             \
  X(SofteningDiskMaxPhys) X(SofteningBulgeMaxPhys) X(SofteningStarsMaxPhys)                       \
  X(SofteningBndryMaxPhys) X(SofteningTable) X(ForceSoftening) X(Rcut) X(Asmth)                   \
  X(TotNumOfForces) X(BunchSize) X(BufferSize) X(ErrTolIntAccuracy) X(CourantFac)                 \
  X(MaxSizeTimestep) X(MinSizeTimestep) X(MaxRMSDisplacementFac) X(OmegaBaryon) X(MinEgySpec)     \
  X(TypeOfTimestepCriterion) X(StarformationOn) X(BlackHoleNgbFactor) X(BlackHoleFeedbackFactor)  \
  X(SMBHmass) X(InnerBoundary) X(SinkBoundary) X(CritOverDensity) X(UnitLength_in_cm)             \
  X(UnitMass_in_g) X(UnitEnergy_in_cgs)
struct gadget_force_all_layout
{
#define GADGET_FORCE_X(m) int m;
  GADGET_FORCE_ALL_MEMBERS(GADGET_FORCE_X)
#undef GADGET_FORCE_X
};
/* host_All == NULL unbinds (the library's own `All` is the state again).  The member types must be
 * the reference's (int / double / long long, MyFloat == double: DOUBLEPRECISION builds). */
void gadget_force_bind_all(void *host_All, const struct gadget_force_all_layout *offsets);
int gadget_force_all_layout_count(void);   /* number of ints in the table (ABI check for bindings) */

/* A host built with another -D set keeps its own struct particle_data / sph_particle_data -- the
 * shipped bundle's are 536 / 264 bytes, with Hsml and NumNgb in P (the PPP macro) and the
 * BLACK_HOLES / DUST unions -- and binds its arrays by BYTE OFFSETS: every driver of this library then
 * reads and writes the host's records through the tables (P / SphP below stay unused).  `lay` as for
 * ghip_upload_aos; `bh` (may be NULL) names the members the sink passes touch, -1 = absent:
 *   P[].ID, SwallowID (unsigned int), BH_Mass, BH_Mdot, b1.BH_Density, b2.BH_Entropy,
 *   b3.BH_SurroundingGasVel[3], b4.BH_accreted_Mass, b5.BH_accreted_BHMass, b5.BH_accreted_DustMass,
 *   b6.BH_accreted_momentum[3], d1.DUST_Density, d2.DUST_Entropy, d3.DUST_SurroundingGasVel[3],
 *   Dust_Mass (allvars.h:1206-1330), SphP[].i.Injected_BH_Energy (allvars.h:1580-1584).
 * A probe TU fills both tables with offsetof() under the host's flags. */
struct gadget_force_bh_layout
{
  int p_id, p_swallowid, p_bh_mass, p_bh_mdot, p_bh_density, p_bh_entropy, p_bh_gasvel;
  int p_bh_accreted_mass, p_bh_accreted_bhmass, p_bh_accreted_dustmass, p_bh_accreted_momentum;
  int p_dust_density, p_dust_entropy, p_dust_gasvel, p_dust_mass;
  int s_injected_bh_energy;
};
void gadget_force_bind_records(void *host_P, void *host_SphP, const ghip_layout *lay,
                               const struct gadget_force_bh_layout *bh);   /* host_P == NULL unbinds */

/* allvars.h:1673-1684: export bookkeeping record other translation units sort with the two
 * functions below (blackhole.c:366, dust.c:114, density.c:186 ...) */
struct data_index
{
  int Task;
  int Index;
  int IndexGet;
};

/* gravdata_in / gravdata_out, allvars.h:1690-1716 (mode == 1 records) */
struct gravdata_in
{
  MyFloat Pos[3];
  int Type;
  MyFloat OldAcc;
  int NodeList[NODELISTLENGTH];
};
struct gravdata_out
{
  MyLongDouble Acc[3];
  int Ninteractions;
};

/* struct NODE / struct extNODE (allvars.h:1847-1916) of the minimal flag set: 88 / 80 bytes */
struct NODE
{
  MyFloat len;
  MyFloat center[3];
  union
  {
    int suns[8];
    struct
    {
      MyFloat s[3];
      MyFloat mass;
      unsigned int bitflags;
      int sibling;
      int nextnode;
      int father;
    } d;
  } u;
  int Ti_current;
};
struct extNODE
{
  MyLongDouble dp[3];
  MyFloat vs[3];
  MyFloat vmax;
  MyFloat divVmax;
  MyFloat hmax;
  int Ti_lastkicked;
  int Flag;
};

/* compile-time switches of the reference that this library takes at run time */
struct gadget_force_config
{
  int periodic;            /* -DPERIODIC */
  int pmgrid;              /* -DPMGRID=n (0: off): gravity_tree uses the short-range walk */
  int unequal_softenings;  /* -DUNEQUALSOFTENINGS */
  int device;              /* GPU ordinal of this rank */
  int black_holes;         /* -DBLACK_HOLES (without NO_BH_ACCRETION): Type 5 is a density target
                              (density.c:1035-1041) */
  int dust;                /* -DDUST: Type 2 is a density target (density.c:1043-1046) */
  int accretion_of_dust_only;   /* -DACCRETION_OF_DUST_ONLY (blackhole.c:1003) */
  int accretion_density;        /* -DACCRETION_DENSITY (blackhole.c:1094) */
  int overlap_sph;         /* 1: on a step with gas, gravity_tree() returns with its walks still in
                              flight and density() / force_update_hmax() / hydro_force() run underneath
                              them on the device; the gravity results (GravAccel, OldAcc, GravCost) and
                              density()'s (one download of the SphP[] block per step instead of two)
                              reach the records when hydro_force() returns -- or gadget_force_flush().  Valid
                              for accel.c's sequence (accel.c:61-106: nothing reads P[].g.GravAccel
                              between the four calls); 0 (default): every driver returns with its own
                              results in P[] / SphP[] */
  int dynamic_tree;        /* All.DoDynamicUpdate: 1 = a gravity_tree() with TreeReconstructFlag == 0 walks
                              the tree of the last force_treebuild(), its nodes drifted and kicked as
                              force_drift_node / force_kick_node / force_finish_kick_nodes do
                              (forcetree.c:1356-1651; ghip_tree_substep), instead of a tree of the
                              current positions.  force_kick_node() and force_finish_kick_nodes() below
                              are then the reference's (timestep.c:261, 588); the library's own
                              advance_and_find_timesteps() hands its kicks to the nodes itself.
                              Comoving runs need gadget_force_set_drift_table(); 0 (default): every
                              gravity_tree() rebuilds */
  int pin_records;         /* 1: page-lock the first NumPart / N_gas records of P[] / SphP[] when they
                              are first uploaded (again when the arrays move or grow), so the record
                              copies run at the link's rate; released by gadget_force_finalize().  The
                              reference allocates both arrays once for All.MaxPart (allocate.c:30-60) */
  int accept_guests;       /* NTask > 1.  0 (default): every record of a rank must lie inside the rank's
                              DomainTask[] pieces of the curve when a driver is called, i.e. the host runs
                              domain_Decomposition() before EVERY gravity_tree() / compute_potential(): a
                              record that has drifted across a split ends the call on all ranks in endrun
                              (the library's device invariant 2, value 5).  1: the drivers accept such
                              records (ghip_dd_set_guests, include/ghip.h) -- the reference's own rule:
                              between two decompositions (domain.c:115-135, TreeDomainUpdateFrequency) a
                              particle stays in the memory of the rank that holds it.  gravity_tree(),
                              density(), force_update_hmax(), hydro_force(), compute_potential() and the
                              sink and dust collectives then give the single global tree's results for the
                              current positions.  The same value on every rank.  (Last member: a host built
                              against the shorter struct must zero-fill it -- `= {0}` does.) */
};

/* ---- globals with the reference's names (allvars.c) ---- */
extern struct particle_data *P;
extern struct sph_particle_data *SphP;
extern struct global_data_all_processes All;
extern int NumPart, N_gas;
extern int FirstActiveParticle, *NextActiveParticle;
extern int TreeReconstructFlag;
extern double DomainCorner[3], DomainCenter[3], DomainLen, DomainFac;
extern int *Ngblist;
extern struct gravdata_in *GravDataGet;
extern struct gravdata_out *GravDataResult;
extern int ThisTask, NTask;
extern double CPU_Step_Treewalk, CPU_Step_Treebuild, CPU_Step_Density, CPU_Step_Hydro,
  CPU_Step_Hmaxupdate; /* the CPU_Step[] buckets the path fills (allvars.h:205-238) */

/* the host's tree arrays (allvars.h:1880-1916, forcetree.c:4560-4600 force_treeallocate).  When
 * Nodes_base is set, force_treebuild() also exports the device-built tree into them ("next" row
 * N2): Nodes = Nodes_base - All.MaxPart as in the reference, Numnodestree = number of nodes. */
extern struct NODE *Nodes_base, *Nodes;
extern struct extNODE *Extnodes_base, *Extnodes;
extern int *Nextnode, *Father;
extern int MaxNodes, Numnodestree;

/* time bins (allvars.h:337-346) and the step flag of run.c; TIMEBINS = 29 */
#define TIMEBINS 29
#define TIMEBASE (1 << TIMEBINS)
extern int TimeBinCount[TIMEBINS], TimeBinCountSph[TIMEBINS], TimeBinActive[TIMEBINS];
extern int FirstInTimeBin[TIMEBINS], LastInTimeBin[TIMEBINS];
extern int *NextInTimeBin, *PrevInTimeBin; /* sized MaxPart by the host */
extern int Flag_FullStep;

/* ---- library management (no counterpart in the reference) ---- */
int gadget_force_init(const struct gadget_force_config *cfg);  /* 0 or a GHIP_E* code */
void gadget_force_finalize(void);
const char *gadget_force_last_error(void);
ghip_ctx *gadget_force_ctx(void);
void gadget_force_layout(ghip_layout *lay);   /* offsets of the structs above */
/* endrun(code) handler: default prints "task %d: endrun called with an error level of %d" and
 * abort()s like MPI_Abort would; tests install a recording handler. */
void gadget_force_set_endrun(void (*handler)(int code));
/* the comoving kick-factor tables of driftfac.c (GravKickTable / HydroKickTable, 1000 entries each,
 * built by the host's init_drift_table) and their log(a) range; needed when
 * All.ComovingIntegrationOn is set */
/* the host's DriftTable[DRIFT_TABLE_LENGTH] (driftfac.c:26-60): cfg.dynamic_tree in comoving runs takes
 * force_drift_node's dt_drift from it (get_drift_factor, driftfac.c:123-163; logTimeBegin / logTimeMax
 * as given to gadget_force_set_kick_tables); without it a comoving sub-step rebuilds */
void gadget_force_set_drift_table(const double *drifttable);
void gadget_force_set_kick_tables(const double *gravkick, const double *hydrokick,
                                  double logTimeBegin, double logTimeMax);
/* tell the glue that the host changed P/SphP outside the four drivers */
void gadget_force_mark_dirty(void);
/* overlap_sph: complete a gravity_tree() whose results are still on the device (no-op otherwise) */
void gadget_force_flush(void);

/* ---- compute_potential() / compute_global_quantities_of_system() (potential.c:22-325, global.c:18-238;
 * -DCOMPUTE_POTENTIAL_ENERGY, -DOUTPUTPOTENTIAL).  Where the results go, as BYTE OFFSETS (-1 = the
 * host's build has no such member; a probe TU fills them with offsetof):
 *   p_potential            P[].p.Potential (double), written by compute_potential() and read by
 *                          compute_global_quantities_of_system()
 *   p_old_photon_momentum  P[].OldPhotonMomentum (VIRTUAL): EnergyRadComp of Type 3
 *   sys_*                  the members of the host's struct state_of_system (allvars.h:1646-1667) that
 *                          global.c writes; sys_EnergyRadAdded / sys_EnergyRadDeleted are listed for a
 *                          complete probe and never written (global.c does not write them)
 *   a_pm_ti_begstep / a_pm_ti_endstep   All.PM_Ti_begstep / PM_Ti_endstep in the host's `All` bound
 *                          with gadget_force_bind_all (PMGRID builds: the GravPM kick, global.c:96-103)
 *   rad_fac                C / All.UnitVelocity_in_cm_per_s (VIRTUAL; not an offset)
 * NTask > 1 with a transport bound (gadget_force_connect or gadget_force_set_allgather): both functions
 * are collectives that EVERY rank enters, as gravity_tree() is.  compute_potential() uploads this rank's
 * records, drifts what is behind Ti_Current on the device, runs GHIP_DD_POTENTIAL and writes
 * P[].p.Potential of this rank's records only; compute_global_quantities_of_system() runs
 * GHIP_DD_GLOBAL_QUANTITIES and fills the bound SysState on every rank with the same bytes (the reference
 * reduces to rank 0 and broadcasts the struct, global.c:146-237).  NTask > 1 without a transport: both
 * call endrun(90012) and write nothing.  cfg.dynamic_tree is not supported on ranks.  A missing binding
 * the build needs (p_potential, the SysState, the PM step or the comoving tables) is endrun(90013). */
struct gadget_force_potential_layout
{
  int p_potential, p_old_photon_momentum;
  int sys_Mass, sys_EnergyRadComp, sys_EnergyRadAdded, sys_EnergyRadDeleted, sys_EnergyKin, sys_EnergyPot,
    sys_EnergyInt, sys_EnergyTot, sys_Momentum, sys_AngMomentum, sys_CenterOfMass, sys_MassComp,
    sys_EnergyKinComp, sys_EnergyPotComp, sys_EnergyIntComp, sys_EnergyTotComp, sys_MomentumComp,
    sys_AngMomentumComp, sys_CenterOfMassComp;
  int a_pm_ti_begstep, a_pm_ti_endstep;
  double rad_fac;
};
/* host_SysState: the host's SysState (what energy_statistics() prints); lay == NULL unbinds */
void gadget_force_bind_potential(void *host_SysState, const struct gadget_force_potential_layout *lay);
/* potential.c:22-325: every particle behind All.Ti_Current is drifted on the device (potential.c:74-78;
 * the host's records keep their state), the tree is the one gravity_tree() would walk now (a fresh build,
 * or the kept tree with cfg.dynamic_tree), and ONLY P[].p.Potential is written */
void compute_potential(void);
/* global.c:18-238: SysState from the host's records (P[].p.Potential as compute_potential left it) */
void compute_global_quantities_of_system(void);

/* ---- the reference's call surface ---- */
/* ---- fof_fof() (fof.c:94-333; accel.c:176-189 calls fof_fof(-1) between hydro_force() and blackhole_accretion()
 * under -DFOF -DBLACK_HOLES): the group catalogue of this rank's records by ghip_fof, and for num < 0 the new
 * sink seeds of fof_make_black_holes() (fof.c:1783-1886).  One table of ints:
 *   a_*    byte offsets of doubles in `host_All`: Omega0, OmegaBaryon, Hubble, G, Time (-1: the mirror's own
 *          `All` / gadget_force_bind_all), MinFoFMassForNewSeed, SeedBlackHoleMass, MassTable[1], massDMpart
 *          (-1: 0; the seeds need the first two and one of the last two)
 *   primary_types, secondary_types, group_min_len   FOF_PRIMARY_LINK_TYPES (2), FOF_SECONDARY_LINK_TYPES,
 *          GROUP_MIN_LEN (32) as VALUES (<= 0 for the last: 32)
 *   p_bh_mass, p_bh_mdot, p_stellar_age   byte offsets of P[].BH_Mass, P[].BH_Mdot (doubles; -1: p_bh_mass /
 *          p_bh_mdot of the bh table of gadget_force_bind_records, if bound) and P[].StellarAge (-1: absent)
 * fof_fof(num) uploads the records if the device copy is stale, uploads P[].ID (p_id of the bh table; without one
 * the ID is the index), builds the tree if none of the current records is in place (fof.c:149-150), runs ghip_fof
 * with LinkL from the LINKLENGTH rule (fof.c:112-124) and fills Ngroups, TotNgroups, TotNids and Group[], which
 * the mirror owns and which stay valid until the next call.  Group[] is left sorted by MinID (fof.c:1117);
 * FirstPos is the position of the member that carries MinID; Sfr, BH_Mass and BH_Mdot of a group are summed from
 * the records where their members are bound (Sfr is not), else 0; task_maxdens = ThisTask where index_maxdens >= 0.
 * num < 0: every group with LenType[1] * massDMpart >= (Omega0 - OmegaBaryon) / Omega0 * MinFoFMassForNewSeed,
 * no Type-5 member and a gas member gets a seed at index_maxdens: endrun(7772) if that record is not gas, else
 * Type = 5, StellarAge = All.Time, BH_Mass = SeedBlackHoleMass, BH_Mdot = 0; Stars_converted grows by their
 * number, which gadget_force_fof_new_seeds() also returns (All.TotBHs += / All.TotN_gas -= stay the host's).
 * The device copy is marked stale then.  num >= 0 computes the same catalogue and returns: the group files are the
 * host's I/O, SUBFIND is not built.
 * NTask > 1: endrun(90016) -- groups that span ranks need an exchange of labels that is not built.  No table
 * bound: endrun(90013).  The nearest-primary search did not converge: endrun(1159), as fof.c:1651. */
struct gadget_force_fof_layout
{
  int a_omega0, a_omega_baryon, a_hubble, a_g, a_time;
  int a_min_fof_mass_for_new_seed, a_seed_black_hole_mass, a_mass_table_1, a_mass_dm_part;
  int primary_types, secondary_types, group_min_len;
  int p_bh_mass, p_bh_mdot, p_stellar_age;
};
void gadget_force_bind_fof(void *host_All, const struct gadget_force_fof_layout *lay);   /* lay == NULL unbinds */
int gadget_force_fof_layout_count(void);   /* number of ints in the table (ABI check for bindings) */
int gadget_force_fof_new_seeds(void);      /* seeds the last fof_fof(num < 0) made */
struct gadget_force_group                  /* struct group_properties, fof.h:26-47 (-DSFR -DBLACK_HOLES) */
{
  int Len;
  int Offset;
  int MinID;
  int MinIDTask;
  int GrNr;
  int LenType[6];
  double MassType[6];
  double Mass;
  double CM[3];
  double Vel[3];
  double FirstPos[3];
  double Sfr;
  double BH_Mass;
  double BH_Mdot;
  double MaxDens;
  int index_maxdens, task_maxdens;
};
extern int Ngroups, TotNgroups;
extern long long TotNids;
extern struct gadget_force_group *Group;
extern int Stars_converted;
void fof_fof(int num);

void endrun(int ierr);
void set_softenings(void);
/* gravtree.c:892-907 (order by Task, then Index) and :909-963 (a stable sort of data_index records
 * with that interface; they live in gravtree.c, which this library replaces) */
int data_index_compare(const void *a, const void *b);
void mysort_dataindex(void *b, size_t n, size_t s, int (*cmp)(const void *, const void *));
void domain_findExtent(void);
int force_treebuild(int npart, void *mp);
/* forcetree.c:1455, 1522 (cfg.dynamic_tree): the momentum a kicked particle hands to its ancestors;
 * collected per call and applied to the kept tree by force_finish_kick_nodes() */
void force_kick_node(int i, MyFloat *dv);
void force_finish_kick_nodes(void);
void ewald_init(void);
void gravity_tree(void);
void density(void);
int density_isactive(int n);
void force_update_hmax(void);
void hydro_force(void);
/* "next" row N1 (timestep.c:29, 1125, 1226): the particle loop runs on the device */
void advance_and_find_timesteps(void);
void find_dt_displacement_constraint(double hfac);
int get_timestep_bin(int ti_step);

int force_treeevaluate(int target, int mode, int *nexport, int *nsend_local);
int force_treeevaluate_shortrange(int target, int mode, int *nexport, int *nsend_local);
int force_treeevaluate_ewald_correction(int target, int mode, int *nexport, int *nsend_local);
int density_evaluate(int target, int mode, int *nexport, int *nsend_local);
int hydro_evaluate(int target, int mode, int *nexport, int *nsend_local);
int ngb_treefind_variable(MyDouble searchcenter[3], MyFloat hsml, int target, int *startnode,
                          int mode, int *nexport, int *nsend_local);
int ngb_treefind_pairs(MyDouble searchcenter[3], MyFloat hsml, int target, int *startnode,
                       int mode, int *nexport, int *nsend_local);

/* "next" row N4, BLACK_HOLES builds with bound records (gadget_force_bind_records with a bh table):
 * the two per-sink neighbour passes with the reference's signatures (proto.h:110-111; mode 0 = a
 * local sink, index into P[]) -- a batch of one on the device -- and the neighbour-pass core of
 * blackhole_accretion() (blackhole.c:70): for ALL active sinks, SwallowID / Injected_BH_Energy reset
 * (:300-305 via the marks), blackhole_evaluate (:346-353), blackhole_evaluate_swallow (:545-551), the
 * accreted sums added to the sinks' records (:648-660), the victims' Mass zeroed, and the swallow
 * counts (N_gas_swallowed, N_BH_swallowed, N_dust_swallowed).  The per-sink scalar bookkeeping
 * around it (Mdot, Eddington limit, logs: blackhole.c:133-290, 690-800) stays the host's. */
int blackhole_evaluate(int target, int mode, int *nexport, int *nsend_local);
int blackhole_evaluate_swallow(int target, int mode, int *nexport, int *nsend_local);
void blackhole_accretion_neighbour_passes(void);
extern int N_gas_swallowed, N_BH_swallowed, N_dust_swallowed;

/* DUST builds with bound records: the dust-gas drag passes with the reference's names (dust.c:60, 263;
 * called at accel.c:194, 198), for the active Type-2 particles in FirstActiveParticle order.  They read
 * d1.DUST_Density / d2.DUST_Entropy / d3.DUST_SurroundingGasVel through the bh table of
 * gadget_force_bind_records, and the members below through this table (byte offsets, -1 = absent):
 *   P[]     d7.DUST_particle_density, d9.DUST_particle_velocity[3], DeltaDustMomentum[3],
 *           NewDragAcc[3], DeltaDragEnergy, DustRadius, DustVcoll   (allvars.h:1201-1319)
 *   SphP[]  dh.DragHeating                                         (allvars.h:1440)
 *   All     MeanWeight, UnitDensity_in_cgs, UnitVelocity_in_cm_per_s, read from `host_All` (the host's
 *           own `All`; the other members come from the library's `All` or gadget_force_bind_all)
 * dust_density() writes d7 of the grains; dust_drag() writes the grains' Vel, d9, DeltaDustMomentum,
 * NewDragAcc (zero), DeltaDragEnergy and DustVcoll, and the gas's Vel, Entropy and dh.DragHeating (in/out:
 * the records' value plus this step's heating); nothing else.  With NTask > 1 and a transport bound
 * (gadget_force_connect / gadget_force_set_allgather) both are collectives over all ranks, after
 * gravity_tree() and density() of the same step (GHIP_DD_DUST_DENSITY / GHIP_DD_DUST_DRAG); without one
 * they call endrun(90010).  lay == NULL unbinds. */
struct gadget_force_dust_layout
{
  int p_particle_density, p_particle_velocity, p_delta_momentum, p_new_drag_acc, p_delta_energy,
    p_radius, p_vcoll;
  int s_drag_heating;
  int a_mean_weight, a_unit_density, a_unit_velocity;
};
void gadget_force_bind_dust(void *host_All, const struct gadget_force_dust_layout *lay);
/* The physics switches the reference's Makefile lists next to -DDUST (ghip_set_dust_model, include/ghip.h) on
 * bound records: the six switches as ints (> 0: defined), byte offsets of All.VirtualTime,
 * All.FragmentationVelocity, All.InitialDustRadius and All.UnitEnergy_in_cgs (doubles) in the host's All, and of
 * P[].LogDustRadius_by_dt (double) in the bound P records; -1 = absent.  All.Time is the mirror's own, P[].ID the
 * p_id of the bh table of gadget_force_bind_records (fe_and_ice_grains needs it).  growth needs a_virtual_time,
 * real_pebble_collisions a_fragmentation_velocity, vaporize a_initial_dust_radius and a_unit_energy: endrun(90002)
 * otherwise.  Once bound, every dust pass sets the model with the All.Time of the call; dust_density() also writes
 * the raw d9 sums (real_pebble_collisions), dust_drag() also writes DustRadius and, where dust.c:465 does,
 * LogDustRadius_by_dt (growth).  lay == NULL unbinds.
 * Single rank for growth, real_pebble_collisions and vaporize: with NTask > 1 both functions call endrun(90015)
 * and write nothing -- ranks drive GHIP_DD_DUST_DENSITY / GHIP_DD_DUST_DRAG in the GHIP_DUST_GRAINS_FORM with
 * ghip_set_dust_model themselves.  epstein and no_friction_heating alone also serve ranks. */
struct gadget_force_dust_model_layout
{
  int growth, real_pebble_collisions, vaporize, fe_and_ice_grains, epstein, no_friction_heating;
  int a_virtual_time, a_fragmentation_velocity, a_initial_dust_radius, a_unit_energy;
  int p_log_radius_by_dt;
};
void gadget_force_bind_dust_model(void *host_All, const struct gadget_force_dust_model_layout *lay);

/* -DTIME_DEP_ART_VISC and the uniform viscosity switches of hydro_evaluate (hydra.c:1512-1595) on bound
 * records (ghip_set_viscosity, include/ghip.h).  Byte offsets of All.AlphaMin / All.ViscSource /
 * All.DecayTime (doubles, as begrun.c:132-133 left them) in the host's All, of SphP[].alpha and
 * SphP[].Dtalpha (doubles) in the bound SphP records, and the four compile-time switches as ints
 * (> 0: defined).  -1 = absent; time_dependent needs all five offsets.  Once bound, hydro_force()
 * gathers alpha and Dtalpha from the records, runs, and writes both back once the SPH results have
 * arrived (also with cfg.overlap_sph): Dtalpha of the active gas is new.
 * advance_and_find_timesteps() gathers them again, applies timestep.c:530-533 and writes both back:
 * alpha of the kicked gas is new.  All.ArtBulkViscConst is the mirror's own.  lay == NULL unbinds.
 * Single rank: with NTask > 1 a bound table makes hydro_force() and advance_and_find_timesteps()
 * call endrun(90014) and write nothing -- ranks drive GHIP_DD_HYDRO with ghip_set_viscosity /
 * ghip_visc_set_alpha themselves. */
struct gadget_force_visc_layout
{
  int a_alpha_min, a_visc_source, a_decay_time;
  int s_alpha, s_dtalpha;
  int time_dependent, conventional, no_limiter, no_shear_limiter;
};
void gadget_force_bind_viscosity(void *host_All, const struct gadget_force_visc_layout *lay);
/* The reference built without -DNOTREERND (the shipped flags): RndTable[n] (system.c:161-172; RNDTABLE = 262144),
 * which run.c:620 refills every step, chooses the subnodes of particles in cells smaller than 1e-3 of their
 * softening (forcetree.c:219-232).  While a table is bound every force_treebuild() uploads it together with
 * P[].ID (p_id of the bh table of gadget_force_bind_records; without one the ID is the index) and the device
 * builds the reference's tree for coincident particles too (ghip_set_rnd_table, include/ghip.h).
 * RndTable == NULL unbinds: identical keys become one level-21 leaf again.  Single rank only. */
void gadget_force_bind_rndtable(const double *RndTable, int n);
void dust_density(void);
void dust_drag(void);

/* The integrator of the shipped flag bundle (-DDUST_TIMESTEP -DACCRETION_RADIUS -DVIRTUAL -DSFR with
 * the configuration's dust / black_holes): once bound, advance_and_find_timesteps() applies the type
 * rules of get_timestep / do_the_kick (ghip_set_integration_flags, include/ghip.h), keeps the bound
 * per-bin sums as timestep.c:183-210 does -- incrementally, in FirstActiveParticle order, where a
 * particle's bin changed -- and find_dt_displacement_constraint() merges types 0/4/5
 * (timestep.c:1160-1172, 1190-1194).  Byte offsets, -1 = absent:
 *   P[]     NewDensity, Total_Mass, DeltaDustMomentum[3]   (allvars.h:1201-1222; Dust_Mass comes from
 *           the bh table of gadget_force_bind_records)
 *   SphP[]  Sfr, da.DragAccel[3]                          (allvars.h:1435, 1514)
 *   All     OuterBoundary, AccDtBlackHole, FeedBackVelocity, UnitVelocity_in_cm_per_s, read from
 *           `host_All` (All.SMBHmass, InnerBoundary and SinkBoundary come from the library's `All`)
 * DragAccel is read before the kick and written back (zero for the kicked gas); the gas's
 * DeltaDustMomentum is read.  NewDensity is not (the kick takes dt_ff = 1 whatever it holds).  These three are kept on a single GPU: with NTask > 1 a
 * table naming any of them calls endrun(90011) (a shipped multi-rank host passes -1: its build never
 * makes them non-zero).  The sums: TimeBinSfr[] (sfr) and, with black_holes and dust,
 * TimeBin_BH_mass / _dynamicalmass / _Mdot from Dust_Mass / Total_Mass / Mass; NULL = not kept.
 * lay == NULL unbinds. */
struct gadget_force_integration_layout
{
  int dust_timestep, accretion_radius, virtual_particles, sfr;   /* flags */
  int p_new_density, p_total_mass, p_delta_dust_momentum, s_sfr, s_drag_accel;
  int a_outer_boundary, a_acc_dt_black_hole, a_feedback_velocity, a_unit_velocity;
};
void gadget_force_bind_integration(void *host_All, const struct gadget_force_integration_layout *lay,
                                   double *TimeBinSfr, double *TimeBin_BH_mass,
                                   double *TimeBin_BH_dynamicalmass, double *TimeBin_BH_Mdot);

/* ---- more than one rank (NTask > 1): the drivers above become collectives ----
 * The host has decomposed the domain (domain_Decomposition, domain.c:100) and every rank holds the
 * particles of its key range in P[0, NumPart).  With NTask > 1 gravity_tree() / density() /
 * force_update_hmax() / hydro_force() take the ranks' key ranges from the host's own top-tree
 *   splits[r] = TopNodes[<the leaf DomainStartList[r]>].StartKey          (domain.c:1075-1113, 1495)
 * and run the domain-decomposed device path (ghip_dd_*: locally essential trees and SPH ghosts in
 * place of the export loops gravtree.c:175-339, density.c:193-389, hydra.c:274-526 and of the
 * pseudo-particle exchange forcetree.c:879-1016, 1722-1747).  MULTIPLEDOMAINS must be 1.
 * Exchanges go over RCCL (gadget_force_connect: every rank passes the 128-byte id that rank 0
 * obtained from gadget_force_unique_id and broadcast over the host's MPI), or -- a host without
 * RCCL, several ranks on one GPU -- through the host's own all-gather (gadget_force_set_allgather:
 * `allgather(user, send, bytes, recv)` = MPI_Allgather(send, bytes, MPI_BYTE, recv, bytes, MPI_BYTE)). */
struct topnode_data   /* allvars.h:437-447 */
{
  peanokey Size;
  peanokey StartKey;
  long long Count;
  MyFloat GravCost;
  int Daughter;
  int Pstart;
  int Blocks;
  int Leaf;
};
extern struct topnode_data *TopNodes;
extern int NTopnodes, NTopleaves;
extern int *DomainStartList, *DomainEndList;
extern int *DomainTask;   /* allvars.h:429: the rank of every top-leaf.  When set (-DMULTIPLEDOMAINS > 1: a rank
                             owns several pieces of the curve, domain.c:1158-1215) the drivers take the
                             ownership of the curve from it, leaf by leaf, instead of from DomainStartList */
int gadget_force_unique_id(void *id128);
int gadget_force_connect(const void *id128);
void gadget_force_set_allgather(int (*allgather)(void *user, const void *send, size_t bytes, void *recv),
                                void *user);

peanokey peano_hilbert_key(int x, int y, int z, int bits);
peanokey morton_key(int x, int y, int z, int bits);
double hubble_function(double a);

#ifdef __cplusplus
}
#endif
#endif
