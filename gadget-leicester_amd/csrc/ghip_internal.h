// ghip_internal.h -- shared declarations of the gfx950 force-path library (not installed).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/ghip.h"
#include "ghip_count.h"

#define GHIP_BITS 21       // BITS_PER_DIMENSION, allvars.h:58
#define GHIP_EN 64         // EN, forcetree.c:51
// A second copy of the Ewald table is brick-tiled: one 128-byte line holds the values of 2 (first
// index) x 2 (second index) rows x 4 consecutive values of the last index, and consecutive bricks
// along the last index OVERLAP by one value (3 cells per brick), so that the pair (k, k+1) of a cell
// never straddles two lines.  Value (i, j, v) sits in brick (i>>1, j>>1, v/3) at
// ((i&1)*2 + (j&1))*4 + v%3 -- and, for v%3 == 0 and v > 0, also in slot 3 of brick v/3 - 1.
#define GHIP_EW_NB ((GHIP_EN >> 1) + 1)   // bricks along the first and the second index (values 0..EN)
#define GHIP_EW_NKB (GHIP_EN / 3 + 1)     // bricks along the last index: 3 cells each
#define GHIP_EW_DOUBLES (GHIP_EW_NB * GHIP_EW_NB * GHIP_EW_NKB * 16)
static inline __host__ __device__ unsigned int ghip_ew_offset(int i, int j, int kb, int t)
{
  return (unsigned int) ((((i >> 1) * GHIP_EW_NB + (j >> 1)) * GHIP_EW_NKB + kb) * 16 +
                         ((i & 1) * 2 + (j & 1)) * 4 + t);
}
#define GHIP_NTAB 1000     // NTAB, forcetree.c:28
#define GHIP_WAVE 64
#define GHIP_BLOCK 256
#define GHIP_MAXRANKS 64      // shards of a multi-GPU run (u64 rank masks)

// ---------------------------------------------------------------------------------------------
// host-side helpers
// ---------------------------------------------------------------------------------------------
// A block of device memory and its owner: a device allocation of the library is a DevBuf member of
// the context (or of one of its sub-objects) and is freed with it -- there is no list to add it to.
// Sized by ghip_ensure; the bytes all DevBufs of the process hold are counted
// (ghip_device_bytes_in_use).
struct DevBuf
{
  void *p = nullptr;
  size_t cap = 0;  // bytes
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { (void) release(); }
  hipError_t alloc(size_t bytes);   // of an empty DevBuf (ghip_api.hip)
  hipError_t release();             // back to empty; what hipFree said
  void swap(DevBuf &o)              // the two exchange their blocks
  {
    void *tp = p;
    size_t tc = cap;
    p = o.p;
    cap = o.cap;
    o.p = tp;
    o.cap = tc;
  }
};

// Gives back everything a sub-object of the context owns: it is destroyed and a fresh one made in
// its place, so that its DevBuf members free themselves and its other members start over.
template <class T> static inline void ghip_renew(T &x)
{
  x.~T();
  new(&x) T();
}

// Sizes of a tree as the DEVICE knows them: written by k_tree_info at the end of the counting stage
// of a build, into device memory (the build's later kernels and every hot-path consumer read them
// there) and into a pinned host mirror (the host learns them without a copy at its next
// verification point, ghip_tree_verify).  The host therefore enqueues a whole build, and the walks
// behind it, without waiting for the node count.
struct TreeSizes
{
  int nelem;      // n + nnodes; 0 while the tree is unusable (bad != 0): every consumer then does nothing
  int nnodes;
  int maxlevel;
  int bad;        // 1: more nodes than the element buffers hold; 2: key runs too long for the 32-bit sort;
                  // 3: paths deeper than GHIP_TREE_MAXLEVEL (ghip_set_rnd_table)
  int n;          // sources
  int gen;        // build generation (host counter): tells a fresh mirror from a stale one
  int longrun;
  int pad;
};

struct TreeDev
{
  int n = 0;        // particles in this tree
  int nnodes = 0;   // (host copies: exact after a synchronous build or after ghip_tree_verify)
  int nelem = 0;    // n + nnodes
  int maxlevel = GHIP_BITS;  // deepest node level
  // sort
  DevBuf key, skey, idx, perm, iperm;  // u64[n], u64[n], i32[n], i32[n] (sorted->host index), i32[nhost]
  DevBuf skey2, rnd_long;              // u64[n]: second word of the paths; long runs of the re-sort (ghip_set_rnd_table)
  bool rnd = false;                    // this build's paths have two words (a table is bound)
  DevBuf cpl, cnt, nb;                 // i32[n]: common prefix levels, node counts, exclusive scan
  DevBuf phkey, phorder;               // u64[n], i32[n]: tree-order indices in Peano-Hilbert order
  // pre-order element list
  DevBuf xm, cl, lk, aux;              // double4[nelem], double4[nelem], int4[nelem], f64[nelem]
  // walk segments (ghip_walk.h): start[ns+1], nanc[ns], anc[ns][GHIP_MAXANC]
  DevBuf seg_start, seg_nanc, seg_anc;
  int ns = 1;            // segments of the fine table
  int seg_ns[3] = {1, 1, 1}, seg_soff[3] = {0, 0, 0}, seg_noff[3] = {0, 0, 0};   // fine / mid / coarse
  DevBuf mq, mq2;                      // WalkHot[nelem], WalkCold[nelem]: walk records (gravity tree)
  DevBuf slvl;                         // i32[n]: level of an imported pruned node in sorted order, 0: particle
  DevBuf father, arrived;              // moment pass: per-level lists of the chunk-crossing nodes, their counts
  DevBuf dsz;                          // TreeSizes on the device
  TreeSizes *hsz = nullptr;            // its pinned host mirror
  int cap_nodes = 0;                   // nodes the element buffers are sized for
  int last_n = -1, last_nnodes = 0;    // the last verified build: sources, nodes
  bool built = false;
};

// ---------------------------------------------------------------------------------------------
// multi-GPU domain decomposition (ghip_dd.hip, ghip_comm.hip)
// ---------------------------------------------------------------------------------------------
// Target groups of a shard, two levels: DD_NSUPER super-groups of DD_NSUB groups of consecutive
// targets along the space-filling curve.  A group is (bounding box, the least OldAcc of its
// targets, the largest search radius); other shards test their tree nodes / gas particles against
// these boxes to decide what this shard can possibly need (ghip_dd.hip).
#define DD_NSUPER 64   // = lanes of a wavefront: one test of a node against all super-groups of a rank
#define DD_NSUB 16
#define DD_NGROUPS (DD_NSUPER * DD_NSUB)
#define DD_TABLE (DD_NSUPER + DD_NGROUPS)   // records per shard: super-groups first
// ... and one status record behind them (cx != 0: this shard met an error while it prepared the
// table -- a particle outside its key range, a device invariant): every shard reads every status after
// the all-gather and all of them fail TOGETHER, instead of one returning while its peers wait for it
// inside the next collective.  cy: the guests this shard holds (ghip_dd_set_guests; 0 with the mode off):
// after the all-gather every shard knows whether anybody holds one
#define DD_STRIDE (DD_TABLE + 1)
struct __attribute__((aligned(64))) DDGroup
{
  double cx, cy, cz;   // box centre
  double ex, ey, ez;   // half extents; ex < 0: empty group
  double amin;         // gravity: least OldAcc of the targets; SPH: unused
  double rmax;         // SPH: largest search radius (Hsml * margin) of the targets; gravity: unused
};

// one element of a locally essential tree as it crosses a link (64 B)
struct __attribute__((aligned(64))) LetRec
{
  double x, y, z, m;          // particle: position, mass; pruned node: centre of mass, mass
  unsigned long long key;     // Morton key (node: the cell's prefix, zero padded)
  double aux;                 // particle: its softening; node: max softening below, negative = mixed
  int level;                  // 0: particle; L > 0: node of level L that no target of the receiver opens
  int pad;
  double spare;
};

// a ghost gas particle as it crosses a link: the two 64-byte records of the SPH kernels
struct __attribute__((aligned(64))) GhostRec
{
  double p[8];   // x, y, z, m, vx, vy, vz, h
  double q[8];   // pressure, density, dhsmlfac, divvel, curlvel, timestep, 0, 0
};

// a pending exchange of the state machine (ghip_dd_step): executed over RCCL by ghip_dd_exchange
// or, for several shards living in one process, by ghip_dd_exchange_local
struct DDXchg
{
  int kind = 0;                 // 0 none, 1 all-gather of fixed-size blocks, 2 all-to-all-v of records
  const void *send = nullptr;   // device
  size_t bytes = 0;             // kind 1: bytes per rank; kind 2: bytes per record
  DevBuf *recv = nullptr;       // kind 1: [nranks][bytes]; kind 2: records, source-rank major
  int scount[GHIP_MAXRANKS], soff[GHIP_MAXRANKS];   // kind 2, in records (soff into `send`)
  int rcount[GHIP_MAXRANKS], roff[GHIP_MAXRANKS];   // filled by the exchange
  int rtotal = 0;
};

// state of the h iteration of a set of sinks (ghip_sink.hip)
struct SinkIter
{
  std::vector<double> h, left, right, numngb, rho, entropy, gasvel;
  std::vector<int> todo;
};

// what a sink pass needs of its sink (ghip_sink.hip: the host fills it from the resident fields' values;
// ghip_accretion.hip: a kernel does, from the fields and the resident sink table)
struct SinkRec
{
  double x, y, z, vx, vy, vz, mass, h, mdot, rho;
  unsigned int id;
  int timebin, index;
  unsigned int mark;   // the sink's own resident SwallowID (the swallow pass; 0 in the other passes)
};

// A keyed row table on the device (ghip_rowtable.h): an ascending 32-bit key column and one row of
// `nc` doubles per key.  The resident sink table is one, keyed by P[].ID, so that no reordering of the particles
// moves it; the resident wind table is one, keyed by PARTICLE INDEX (two live wind particles can carry the same ID),
// so that ghip_rearrange and ghip_peano_order send it through their maps and ghip_wind_spawn appends to it.
struct RowTable
{
  DevBuf key, rows;           // u32[n] ascending, f64[n][nc]
  DevBuf tmp_key, tmp_rows;   // the image: rows in any order that a new table is sorted from, or grows into
  DevBuf work;                // status words, a report, the int arrays of selections and sorts (RtWork)
  int n = 0;
  const int nc;
  const char *const what, *const key_what, *const setter;   // in messages: "sink", "ID", "ghip_sinks_set_table"
  bool on = false;            // a table was given (possibly of 0 rows)
  bool stale = false;         // ghip_set_counts changed the counts since: refused until given again
  unsigned int last_dup = 0;  // the key that the last refused installation found twice
  RowTable(int nc_, const char *what_, const char *key_what_, const char *setter_)
      : nc(nc_), what(what_), key_what(key_what_), setter(setter_)
  {
  }
};

// One dust pass as ghip_dust.hip runs it: each of the four entry forms (positional, *_grains, GHIP_DD_DUST_* with
// walk = 0 or GHIP_DUST_GRAINS_FORM) fills this once, and everything below the entry reads only it
struct DustCall
{
  const ghip_dust_params *p = nullptr;
  ghip_dust_grains g = {};
  bool grains = false;            // the caller has arrays for what the model writes (d9 sums, radius)
  bool drag = false;
  const char *who = "", *other = "";   // the entry in messages; the form that dust_model_ready points to
};

// The renumbering of a migration as the wind rows need it (ghip_dd.hip, migrate_step, fills it in MERGE; mig_scan and
// mig_mask hold the arrays until the next migration): the new layout is kept gas, received gas, kept others, received
// others.  A kept particle i that is not gas goes to ngn + (ro[i] >> 32); the particle at receive position q, not gas
// (vn[q] == 1 << 32), to ngn + ko + (rn[q] >> 32).
struct WkMigPlan
{
  bool moved = false;             // the layout changed (else: nobody left or came, every key stands)
  int n_old = 0, ng_old = 0, nrecv = 0, ngn = 0, ko = 0;
  const unsigned long long *mask = nullptr, *ro = nullptr, *vn = nullptr, *rn = nullptr;
  int first[GHIP_MAXRANKS], cnt[GHIP_MAXRANKS];   // per sender: receive position of its first particle, its particles
};

#define DD_NOPS (GHIP_DD_PM_NONPERIODIC + 1)   // operations of ghip_dd_begin, 0 = none (dd_ops[] in ghip_dd.hip)

// GHIP_DD_WIND in progress (ghip_wind.hip): copies of the arguments, the form, and where the loop stands
struct WindDD
{
  ghip_dd_wind_args a = {};
  ghip_wind_params p = {};
  int form = 0;            // GHIP_WIND_FORM, _DENSITY_FORM or _SPREAD_FORM
  bool resident = false;   // GHIP_WINDS_RESIDENT_FORM: form = GHIP_WIND_FORM, the list and the planes from the wind table
  // GHIP_WINDS_SPAWN_FORM (ghip_accretion.hip): the arguments, a copy of the params, and what the count found (a SpawnRun)
  ghip_dd_winds_args spawn_args = {};
  ghip_wind_spawn_params spawn_p = {};
  alignas(8) char spawn_run[256] = {};
  int iter = 0;            // global iterations begun (0: the density at the start)
  int m = 0, under = 0;    // this shard's list; its particles above 1e-40
  int m_next = 0, under_next = 0;
  long long under_all = 0; // ... of all shards, as of the last status round
  double hmax_all = 0;     // the largest h_j of any shard's gas
  int cur = 0;             // which of the two list buffers holds the list
  int nimp = 0;            // density records imported this iteration (kept for the spread pass)
  long long bits = 0, sent = 0, recvd = 0, imp_pairs = 0, exchanges = 0;
  bool entered = false;    // the loop was entered (the floor was passed)
};

struct DDState
{
  bool on = false;
  int rank = 0, nranks = 1;
  unsigned long long splits[GHIP_MAXRANKS + 1];   // Peano-Hilbert key range of rank r: [splits[r], splits[r+1])
  // The general form (MULTIPLEDOMAINS > 1: a rank owns several pieces of the curve, domain.c:482-494,
  // 1158-1215): nseg segments [segkey[s], segkey[s+1]) with their owners, adjacent segments of one
  // owner merged; ownlo/ownhi = this rank's own pieces.  Device copies for the three kernels that ask
  // "whose is this key" (range check, shared-cell test of the LET selection, migration).
  int nseg = 0, nown = 0;
  bool seg_layout = false;        // the layout in force came from ghip_dd_set_segments (splits[] does not describe it)
  DevBuf segkey, segowner, ownlo, ownhi;
  void *nccl = nullptr;                           // ncclComm_t (ghip_comm.hip)
  // state machine
  int op = 0, phase = 0, walk = 0;
  ghip_grav_params gp;
  ghip_dens_params dp;
  ghip_hydro_params hp;
  DDXchg x;
  DevBuf xstage;                  // device staging of the count all-gather
  // target-group tables: own, and everybody's after the all-gather
  DevBuf grp_own, grp_all;        // DDGroup[DD_TABLE], DDGroup[nranks][DD_TABLE]
  // gravity: locally essential trees
  DevBuf reach, sendm;            // u64[nelem]: ranks whose targets reach / are sent this element
  DevBuf selcnt;                  // i32[nranks][nblocks] block counts / offsets of the packing
  DevBuf let_list;                // i32: per destination, the elements of this tree it is sent
  DevBuf let_send, let_recv;      // LetRec[]
  int let_sent = 0, gh_sent = 0;
  double gh_growth = 0;
  DevBuf gas_tgt;                 // i32: the local gas targets in curve order (gravity-tree indices)
  DevBuf gas_src;                 // i32: all local gas particles in gravity-tree order
  int gt_nimp = 0;                // imported elements the next gravity-tree build includes
  DevBuf src_x, src_y, src_z, src_m, src_aux, src_key, src_lvl;   // sources = local particles + imports
  // SPH: ghost gas particles
  DevBuf gh_mask;                 // u64[ngas]: ranks this gas particle is a ghost on
  DevBuf gh_list;                 // i32: per destination, the local gas-tree indices sent (fixed for the step)
  int gh_scount[GHIP_MAXRANKS], gh_soff[GHIP_MAXRANKS];
  DevBuf gh_send, gh_recv;        // GhostRec[]
  int nghost = 0;
  double gh_margin = 1.3;         // search radii are padded by this factor when ghosts are selected
  double gh_margin_cur = 1.3;     // ... in the density call in progress: grows when an h outgrew it (see density_step)
  int gh_retries = 0;             // re-selections of the density call in progress
  DevBuf status_own, status_all;  // f64[2] per shard: {a value, error flag} (dd_post_status / dd_read_status)
  // guests (ghip_dd_set_guests): resident particles whose keys lie outside this shard's pieces of the curve.
  // The gravity tree's guest pass (ghip_dd_own_tree) finds them and lists their keys per host (the shard
  // that owns the key); when any shard holds one, the keys go to their hosts before the selection of the
  // locally essential trees, which then descends every cell that contains one (k_let_level).
  bool guests_on = false;
  bool guest_xchg = false;        // the operation in progress exchanged guest keys (their sorted list is in place)
  int guests_held = 0;            // guests resident here in the last GHIP_DD_GRAVITY / GHIP_DD_POTENTIAL
  int guests_hosted = 0;          // guest keys received for this shard's pieces of the curve
  DevBuf guest_mask, guest_key;   // u64[n]: 1 << host of a guest, else 0; u64[n]: the Peano-Hilbert keys
  DevBuf guest_list;              // i32: per host, the local indices of its guests (ascending)
  DevBuf guest_send, guest_recv;  // u64: the guests' keys, host-major / the keys received, source-rank major
  DevBuf guest_sorted;            // u64[guests_hosted]: the received keys in ascending order
  int guest_scount[GHIP_MAXRANKS], guest_soff[GHIP_MAXRANKS];
  // what this shard itself met just before a collective decision, kept while its flag travels and raised as its
  // own error when all shards stop (ghip_dd_hold / ghip_dd_raise); consumed in the next phase: one slot is enough
  struct { int rc = 0; std::string msg; } held;
  DevBuf gsx, gsy, gsz, gsm, gsh; // gas sources = local gas + ghosts (tree build input)
  DevBuf h0;                      // f64[ngas]: smoothing lengths the ghost selection was made with
  // migration (domain_exchange): destination masks, send lists, records, shadow field arrays
  DevBuf mig_mask, mig_list, mig_send, mig_recv, mig_scan;
  DevBuf fshadow[GHIP_F_COUNT];
  int mig_out = 0, mig_in = 0;
  // sinks on shards (ghip_sink.hip): every shard's sinks are made known to all, each shard
  // evaluates all of them against its own particles, the partial sums are all-gathered
  ghip_dd_sink_args sink;         // arguments of the operation in progress
  DevBuf sk_send, sk_all;         // SinkRec[] of this shard / of all shards (rank order)
  DevBuf sk_part, sk_parts;       // partial sums of this shard [k][nsink_total] / of all shards
  DevBuf sk_work;                 // per pass: h[total] | slots[total]; swallow: BH masses [n] | victims [n]
  int sk_total = 0, sk_off = 0, sk_iter = 0, sk_ncur = 0;
  SinkIter sk_it;                 // h iteration state of ALL sinks (identical on all ranks)
  // ... in their resident form (walk = GHIP_SINKS_RESIDENT_FORM, ghip_accretion.hip): no host array, this shard's
  // sinks are selected on the device and found in its sink table
  ghip_dd_sinks_args sinks = {};  // arguments of the operation in progress
  int sk_form = 0;                // 0: the per-pass form; GHIP_SINKS_RESIDENT_FORM
  int sk_cnt = 0;                 // this shard's active sinks (0 on a shard that posted a failure record)
  size_t sk_na = 1, sk_nrow = 1;  // the sizes its selection asked of the sink table's work: the same block every phase
  DevBuf sk_gw;                   // u64: the verdict on the gathered records (0: fine), the same on all shards
  DevBuf sk_snap;                 // f64: this shard's rows before the Mdot step, put back when the call fails
  DevBuf sk_own;                  // f64[9][sk_cnt]: the rank-ordered sums of this shard's own sinks
  // the rows of the sink table in GHIP_DD_MIGRATE
  bool mig_tab = false;           // this shard holds a table: its records carry a header, the rows follow
  DevBuf sk_keep, sk_rcnt;        // i32[rows]: 0 = the row departs; i32: rows per destination, pack cursors
  DevBuf sk_rsend, sk_rrecv;      // (ID, GHIP_SK_COUNT doubles) records out / in
  int sk_rscount[GHIP_MAXRANKS], sk_rsoff[GHIP_MAXRANKS];
  // the rows of the wind table in GHIP_DD_MIGRATE (ghip_wind.hip): keyed by particle index, so they are re-keyed
  bool mig_wk = false;            // this shard holds a wind table: the header says so, the rows follow
  DevBuf wk_flag;                 // i32: departing particle has a row [total + 1] | its scan [total + 1] | rows per run
  DevBuf wk_rsend, wk_rrecv;      // (ordinal in the sender's run, GHIP_WK_COUNT doubles) records out / in
  int wk_rscount[GHIP_MAXRANKS], wk_rsoff[GHIP_MAXRANKS];
  WkMigPlan wk_plan;              // what MERGE knew of the renumbering, kept for the rows
  // the dust passes on shards (ghip_dust.hip): this shard's grains go to the shards their spheres reach,
  // partial d7 come back (density), drag records are scattered into every shard's own gas (drag)
  DustCall dust;                  // the operation in progress
  DevBuf du_mask;                 // u64[n]: ranks each local grain goes to (by local particle index)
  DevBuf du_slot;                 // i32[n]: list slot of each local grain (read where du_mask is set)
  DevBuf du_list;                 // i32: per destination, the local particle indices sent (ascending)
  DevBuf du_send, du_recv;        // grain records [DUST_REC doubles] out / in (source-rank major)
  DevBuf du_part, du_back;        // f64: partial d7 of the imported grains / of this shard's exported ones
  DevBuf heat_shadow;             // DragHeating of the migration's new layout
  DevBuf visc_shadow[2];          // ... and alpha / Dtalpha (ghip_visc_set_alpha)
  long long gh_alpha_epoch = -1;  // ctx->visc_epoch when the ghost records in place were packed
  int du_scount[GHIP_MAXRANKS], du_soff[GHIP_MAXRANKS];
  int du_sent = 0, du_recvd = 0;
  // the wind particles on shards (ghip_wind.hip) use the dust passes' selection and record buffers, and:
  WindDD wind;                    // the operation in progress
  DevBuf wd_spread, wd_srecv;     // spread records out / in; the density records in du_recv stay for the spread pass
  DevBuf wd_cnt;                  // u64: pair counts and offsets of the combined scatter (own list | imported)
  DevBuf wind_shadow[2];          // Injected_BH_Momentum / RadAccel of the migration's new layout
  // The trees of this step after GHIP_DD_BH_SWALLOW: only masses changed (the victims' are 0), so their
  // geometry still serves the dust passes, which read the resident masses.  Cleared wherever particles
  // move or a tree is built.
  bool geom_kept = false;
  // traffic of the last operation (bytes this rank sent over links, excluding its own block)
  long long bytes_sent[DD_NOPS] = {};
  ghip_pm_params pm;              // GHIP_DD_PM
  DevBuf pm_all;                  // the density meshes of all shards
  // GHIP_DD_PM_REGION / GHIP_DD_PM_NONPERIODIC (ghip_pm.hip): the extent blocks travel in dc_own / dc_all, the
  // compact octants with their status word in pm_all
  int pmreg_grid = 0;             // PMGRID of the GHIP_DD_PM_REGION in progress
  ghip_pmnp_params pmnp;          // arguments of the GHIP_DD_PM_NONPERIODIC in progress
  // GHIP_DD_POTENTIAL / GHIP_DD_GLOBAL_QUANTITIES (ghip_potential.hip)
  ghip_pot_params pot;            // arguments of the operation in progress
  DevBuf pot_tgt;                 // i32[n]: 0 .. n-1, the target list "all particles of the shard's own tree"
  bool gt_is_pot = false;         // the gravity tree in place is the merged tree GHIP_DD_POTENTIAL built
                                  // (selected for all particles as targets), not the step's GHIP_DD_GRAVITY's
  ghip_dd_global_args gq;         // GHIP_DD_GLOBAL_QUANTITIES: arguments, a copy of *gq.p
  ghip_global_params gq_p;
  int gq_form = 0;                // 0: the energy sums; GHIP_FOF_FORM: the group finder (ghip_fof.hip, state in ctx->fof)
  DevBuf gq_send, gq_all;         // ghip_global_sums of this shard / of all shards (rank order)
  // GHIP_DD_DECOMPOSE (ghip_decomp.hip)
  ghip_dd_decomp_params dcp;      // arguments of the operation in progress
  DevBuf dc_own, dc_all;          // u64[DC_WORDS]: extent images, count, time bins, error word / of all shards
  DevBuf dc_hist, dc_hist_all;    // u64[8^level]: this shard's histogram, later the sum / of all shards
  int dc_level = 0, dc_bmax = 0, dc_shift = 0;
  double dc_corner[3] = {0, 0, 0}, dc_center[3] = {0, 0, 0}, dc_len = 0;   // the cube the keys are formed in
  // GHIP_DD_DECOMPOSE begun with walk = GHIP_SYNC_POINT_FORM (ghip_sync.hip)
  ghip_sync_params sp = {};       // arguments of the operation in progress
  ghip_sync_point sp_out = {};    // the result of the last completed one (ghip_dd_get_sync_point)
  ghip_sync_point sp_cur = {};    // ... of the one in progress
  int sp_selected = 0;            // entries of its list, waiting in act_next for every shard's status
  DevBuf sp_all;                  // u64[nranks][32]: the TimeBinCount of all shards (this shard's: DevWords::timebin_hist)
};

// the pending exchange of a state-machine step (ghip_dd.hip, ghip_sink.hip)
static inline void ghip_dd_set_allgather(DDState &D, const void *send, size_t bytes, DevBuf *recv)
{
  D.x.kind = 1;
  D.x.send = send;
  D.x.bytes = bytes;
  D.x.recv = recv;
}

static inline void ghip_dd_set_alltoallv(DDState &D, const void *send, size_t recbytes,
                                         const int *scount, const int *soff, DevBuf *recv)
{
  D.x.kind = 2;
  D.x.send = send;
  D.x.bytes = recbytes;
  D.x.recv = recv;
  for(int r = 0; r < D.nranks; r++)
    {
      D.x.scount[r] = scount[r];
      D.x.soff[r] = soff[r];
    }
}

// Named scratch words of a context in device memory (ctx->words, made and zeroed by ghip_create):
// one field per use, so that no two uses share a word by accident.  ghip_words(ctx) -> the block.
struct DevWords
{
  // own line: the main stream polls it (ghip_hydro_impl) while kernels of other streams write the rest
  alignas(128) unsigned int pair_started;   // the pair's Ewald walk has dispatched its last workgroup
  alignas(128) unsigned long long ghost_growth;   // density on shards: largest h growth (bits of a double)
  unsigned long long timebin_hist[64];      // ghip_timebin_counts: all particles [0, 32), gas [32, 64)
  int list_count;      // make_list (ghip_tree.hip): targets selected
  int dust_partners;   // ghip_dd_dust_groups: local Type 0 / Type 2 particles selected
  int gas_targets;     // density on shards: gas targets selected
  int step_err;        // ghip_drift / ghip_advance_timesteps: what the kernel met
  int pm_err;          // non-periodic mesh (ghip_pm.hip): a particle outside the allowed region (the range check)
  int tree_info[2][2]; // count_nodes, per tree (gravity, gas): {deepest level, longest key run the
                       // 32-bit sort left unsorted}; k_tree_info reads them and leaves them zeroed
  int rnd_info[2][2];  // rnd_order (ghip_tree.hip), two sets used in turn: {crowded sources, long runs}
  int sync_sel[2];     // ghip_find_next_sync_point: {particles selected, TimeBins outside [0, TIMEBINS)}
};

// ... and in pinned, device-visible host memory (ctx->pinned): kernels write, the host reads after a wait
struct alignas(64) PinnedWords
{
  TreeSizes sizes[2];   // host mirrors of the trees' sizes (gt.hsz, st.hsz)
  int gas_mixed;        // the record unpack met a record of the gas block [0, ngas) that is not Type 0
  int sel_left;         // ghip_density_impl: targets left after an h iteration, written by ghip_wsel_count (a
                        // copy to the host would be one more kernel of the runtime's that waits behind the pair)
};

// the gravity tree between two full builds with what moves it (ghip_set_dynamic_tree, ghip_export.hip)
struct DynTree
{
  TreeDev tree;
  DevBuf ev, dp;             // double4[nelem]: (vs, vmax) / (dp, kicked) per element
  DevBuf eh, cnt, fa;        // scratch of the moment pass (export's kernels)
  DevBuf kick;               // double4[nelem]: a kick pass's per-element sums
  DevBuf kick_dv, kick_flag; // f64[3][n], i32[n]: velocity changes of the last ghip_advance_timesteps
};

// One real 3-d transform of the particle-mesh force (ghip_pm.hip, pm_fft_prepare): hipFFT plans for n^3 on the
// context's stream, the mesh and its transform.  Owns the plans: they are destroyed with it, here alone.
struct PmFft
{
  int n = 0;                             // side the plans and buffers are made for
  void *fwd = nullptr, *inv = nullptr;   // hipfftHandle
  DevBuf rho, k;
  PmFft() = default;
  PmFft(const PmFft &) = delete;
  PmFft &operator=(const PmFft &) = delete;
  ~PmFft();
};

// particle-mesh force (ghip_pm.hip): the periodic mesh PMGRID^3 with its force components
struct PmMesh
{
  PmFft fft;
  DevBuf force;
  // The non-periodic mesh (ghip_pm.hip, "non-periodic mesh"): the padded mesh GRID^3 = (2 PMGRID)^3, the Green's
  // function table, the force components and the density of the lower octant PMGRID^3 (+ one status word).
  // Renewed as a whole, alone (ghip_renew(open)) or with the mesh that owns it.
  struct Open
  {
    PmFft fft;
    int table_n = 0;   // PMGRID `table` is filled for (0: not filled)
    DevBuf table, force, oct;
  } open;
};

// friends-of-friends groups (ghip_fof.hip): work arrays of the last call and its catalogue.  s* arrays are in
// the gravity tree's sorted order, the others in host order or per group.
struct FofState
{
  DevBuf sid, sflag, parent, rootmin, slabel;   // i32[n]: IDs, kind (1 primary, 2 secondary), union-find, min ID per root, labels
  DevBuf plist, slist;                          // i32: sorted indices of the primaries / the secondaries
  DevBuf hcur;                                  // f64[nsec]: search radius of each secondary
  DevBuf words;                                 // FofWords: counters and the link length
  DevBuf part;                                  // f64: block sums of the LINKLENGTH rule
  DevBuf label, key, skey, val, sval;           // i32[n] labels (host order); (label, ID) keys and members, sorted
  DevBuf head, segof, segstart, gkey, gskey, gval, gorder, glen, goff, grnr;   // segments = candidate groups
  DevBuf pgrnr, ids;                            // i32[n] GrNr per particle; i32[Nids] the ID list
  DevBuf groups;                                // ghip_fof_group[Ngroups]
  int n = -1, ngroups = 0;                      // particle count of the last successful call (-1: none)
  long long nids = 0;                           // entries of `ids` (the collective form: this shard's own members)
  double ms[4] = {0, 0, 0, 0};
  hipEvent_t ev[5] = {};
  // ---- the collective form on shards (GHIP_DD_GLOBAL_QUANTITIES begun with walk = GHIP_FOF_FORM; ghip_dd_fof_step).
  // Tree order means the merged tree of GHIP_DD_GRAVITY: nt = own particles + imports; the union-find has the
  // nimp imported primaries behind them.  A label word is (MinID ^ sign bit) << 32 | MinIDTask.
  bool dd = false;                              // the catalogue in place came from the collective form
  ghip_dd_fof_args a = {};                      // arguments of the operation in progress, a copy of *a.p
  ghip_fof_params p = {};
  int nt = 0, nprim = 0, nsec = 0, nimp = 0, nexp = 0, nseg = 0, nown = 0, nkept = 0, iter = 0, rounds = 0;
  long long totprim = 0, totsec = 0, queries = 0, parts_sent = 0;
  double linkl = 0;
  DevBuf stat_own, stat_all;                    // f64[4]: mass and number of the primaries, secondaries, error flag
  DevBuf word_own, word_all;                    // u64: the one-word all-gathers (labels fell / secondaries left)
  DevBuf rlab, plab, plabh;                     // u64: label word per root [nt + nimp], per particle [nt], host order [n]
  DevBuf xmask, xlist, xsend, xrecv;            // border primaries: destinations, lists (tree indices), (x, y, z, label)
  DevBuf lsend, lrecv;                          // u64: the labels of a round, along the same lists
  DevBuf parent2;                               // the union-find while it grows by the imports
  DevBuf hs, cr2, cid, clab;                    // secondaries, by tree index: radius (< 0 settled), best r2 / ID / label
  DevBuf qlist, qsend, qrecv, asend, arecv;     // their queries (x, y, z, h) and the answers (r2, ID, label)
  DevBuf smask, seglist, psend, precv;          // catalogue: owner of each local segment, partial records out / in
  DevBuf rqsend, rqrecv, rpsend, rprecv;        // ... "about which position": the labels asked / FirstPos answered
  DevBuf pkey, pskey, pval, psval, phead, psegof, psegstart;   // the partials an owner received, by (MinID, source)
  DevBuf own, keep, klist, ksend, kall;         // owned groups, who is kept, the kept records of this shard / of all
  DevBuf mkey, msk, mval, msv;                  // kept groups by MinID, for the look-up of GrNr
  DevBuf key2, skey2;                           // (GrNr, ID) of the own members
  DevBuf task;                                  // i32[Ngroups]: the shard index_maxdens counts on
  int x_scount[GHIP_MAXRANKS] = {}, x_soff[GHIP_MAXRANKS] = {}, x_rcount[GHIP_MAXRANKS] = {};
  int q_scount[GHIP_MAXRANKS] = {}, q_soff[GHIP_MAXRANKS] = {};
  int p_scount[GHIP_MAXRANKS] = {}, p_soff[GHIP_MAXRANKS] = {};
  ~FofState()
  {
    for(int i = 0; i < 5; i++)
      if(ev[i])
        (void) hipEventDestroy(ev[i]);
  }
};

// The Newtonian walk of a Newton + Ewald pair is held to W one-wavefront workgroups per SIMD (4 W per
// CU) by unused dynamic LDS: the largest allocation of which 4 W fit into a CU's 160 KB, a whole
// number of 2 KB allocation granules.  W = 4: 10 KB (16 per CU), W = 5: 8 KB (20), W = 6: 6 KB (24 fit;
// the next granule, 8 KB, admits 20 again -- the granules leave nothing in between).
#define GHIP_LDS_PER_CU 163840
#define GHIP_LDS_GRANULE 2048
#define GHIP_PAIR_LDS(W) ((GHIP_LDS_PER_CU / (4 * (W))) / GHIP_LDS_GRANULE * GHIP_LDS_GRANULE)
#define GHIP_PAIR_NSET 3   // settings the balance chooses from: W = 6, 5, 4
static_assert(GHIP_PAIR_LDS(4) == 10240 && GHIP_PAIR_LDS(5) == 8192 && GHIP_PAIR_LDS(6) == 6144,
              "dynamic-LDS caps of the pair");

// ghip_rearrange / ghip_peano_order (ghip_sequence.hip): the maps of the last call, its work arrays, and the
// shadows of the optional resident arrays (the GHIP_F_* fields use DDState::fshadow, as the migration does)
#define SEQ_NOPT 10
struct SeqState
{
  DevBuf new_of_old, old_of_new;   // i32[n before] (-1: eliminated), i32[n after]
  int n_before = -1, n_after = -1; // -1: no call yet
  long long bytes_moved = 0;       // read + written by the move of the last call (0: nothing moved), its planes
  int planes = 0;
  DevBuf flags, rank;              // u64[n + 1]: survivor flags (gas low word, others high word), their exclusive scan
  DevBuf key, skey, idx, sidx;     // u64[n], u64[n], i32[n], i32[n]: the stable pair sort of the two blocks
  DevBuf words;                    // i32[8]: counters and flags of a call
  DevBuf xshadow[SEQ_NOPT];        // new layout of DragHeating, alpha, Dtalpha, Injected_BH_Momentum, RadAccel,
                                   // SwallowID, Injected_BH_Energy, DragAccel, DeltaDustMomentum, NewDensity
};

struct ghip_ctx
{
  ghip_ctx() = default;
  ghip_ctx(const ghip_ctx &) = delete;
  ghip_ctx &operator=(const ghip_ctx &) = delete;
  // waits for the streams, then destroys every handle that was made (all start as nullptr); the
  // members free their device memory afterwards
  ~ghip_ctx();

  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;

  int n = 0, ngas = 0;
  // host-order fields
  DevBuf f[GHIP_F_COUNT];
  // staging for host<->device transfers / AoS images
  DevBuf stage, aosP, aosS;
  PinnedWords *pinned = nullptr;   // hipHostMalloc

  // domain
  double corner[3] = {0, 0, 0}, center[3] = {0, 0, 0}, dlen = 0;
  double soft[6] = {0, 0, 0, 0, 0, 0};

  TreeDev gt;  // gravity tree: all particles
  TreeDev st;  // gas tree
  // sorted gravity-source side arrays (targets read these): x,y,z,soft,oldacc  [n]
  DevBuf sx, sy, sz, ssoft, soldacc;
  // gas records in gas-tree order
  DevBuf gp;  // 8 doubles: x,y,z,m,vx,vy,vz,h
  DevBuf gq;  // 8 doubles: pressure, density, dhsmlfac, divvel, curlvel, timestep, 0, 0
  // density work arrays (gas-tree order)
  DevBuf dleft, dright, drho, dnumngb, ddhsml, ddivv, drot, dflags, dtgt_a, dtgt_b, dhcur;
  DevBuf hpart;  // hydro partial sums

  // active lists
  DevBuf act_host_idx;  // i32[nactive] host indices (uploaded)
  int nactive = -1;     // -1: all
  DevBuf act_next;      // i32[n]: the list ghip_find_next_sync_point is writing; swapped in when the call succeeds
  bool gas_mixed = false;        // a record of the gas block [0, ngas) has Type != 0 (ghip_check_gas_types)
  int skip_massless = 0;         // a gas particle of mass 0 is nobody's neighbour: 1 in density() (-DDUST or
                                 // -DBLACK_HOLES), 3 in density() and hydro_force() (-DBLACK_HOLES)
  bool massless_marked = false;  // the gas records carry the mark of the massless rule
  bool gas_types_unknown = false;  // ... not known since a migration: checked before the next gas tree
  bool lists_dirty = true;       // gravity target list
  bool gas_list_dirty = true;    // gas target list (made once the deferred gas tree exists)
  DevBuf tg_grav, tg_gas;  // sorted-order target lists
  int nt_grav = 0, nt_gas = 0;
  int shard_rank = 0, shard_n = 1;

  // walk outputs in target order
  DevBuf tax, tay, taz, tcost;
  // second set (slot 1) for the Ewald walk of an overlapped Newton+Ewald pair
  DevBuf tax2, tay2, taz2, tcost2, plan_nsub2, plan_woff2, plan_wave2, cubtmp2;
  hipStream_t stream2 = nullptr;   // the pair's Ewald walk runs here
  hipStream_t stream3 = nullptr;   // ... and its Newtonian walk here, so the main stream stays free
  bool adaptive_gravsoft = false;   // ADAPTIVE_GRAVSOFT_FORGAS: gas softening = Hsml (ghip_set_adaptive_gravsoft)
  bool grav_pending = false;       // a pair is in flight; evx[2] marks its end (see ghip_join)
  unsigned int *pair_started = nullptr;   // &DevWords::pair_started once a pair has run
  // the second half of the gas tree build (elements, moments, SphNode records, gas records) is
  // deferred to the first call that needs it, so that it runs underneath a gravity pair
  bool gas_pending = false;
  bool gas_wait_upload = false;   // ghip_upload_aos_particles done, ghip_upload_aos_gas not yet: the
                                   // deferred gas-tree work must not run on stale SphP fields
  hipEvent_t evx[4] = {};          // pair ordering: inputs ready / Newton combined / Ewald combined /
                                   // Ewald walk kernel done (ghip_hydro waits for it)
  hipEvent_t evt[2] = {};          // tree build: fork after the tree-order gather / join (curve_order
                                   // runs on stream2 next to the element emission on the main stream)
  // adaptive wavefront plan of the gravity walks (ghip_walk.h): per walk kind the elements
  // visited per bucket in the previous call (double-buffered) and the scratch plan arrays
  DevBuf plan_steps[3][2], plan_nsub, plan_woff, plan_wave;
  int plan_nb[3] = {-1, -1, -1}, plan_ns[3] = {-1, -1, -1}, plan_cur[3] = {0, 0, 0};
  hipStream_t plan_writer[3] = {nullptr, nullptr, nullptr};   // stream of the last walk of each kind: its
                                                               // per-bucket counts feed the next plan
  DevBuf cubtmp3;                                              // scan space of a plan built on stream3

  // ewald
  DevBuf ewtab;   // double[(EN+1)^3]: fcorrx scaled by 1/Box^2 (y, z by symmetry)
  DevBuf ewbrick; // the same values brick-tiled (GHIP_EW_DOUBLES), for the Ewald walk outside a pair
  double ew_box = 0;
  DevBuf srtab;   // float[NTAB]
  bool srtab_ready = false;

  // scan/sort temp
  DevBuf cubtmp;
  PmMesh pm;
  ghip_pm_region pm_region = {};   // the allowed region of the non-periodic mesh (ghip_pm_find_region / _set_region)
  bool pm_region_set = false;
  DevBuf words;   // DevWords
  // work counters of the walks and the SPH kernels, 64 slots per kind (ghip_count.h): of the current
  // calls (each call of a kind clears its own) and of the run (ghip_run_begin clears)
  DevBuf cslots, rslots;
  ghip_stats stats;
  hipEvent_t ev[16] = {};
  DDState dd;                // multi-GPU domain decomposition (ghip_dd.hip)
  DevBuf bh_swallow, bh_injected;   // "next" row N4 (ghip_sink.hip): P[].SwallowID u32[n],
                                    // SphP[].i.Injected_BH_Energy f64[ngas]
  DevBuf dust_heat;                 // dust_drag (ghip_dust.hip): SphP[].dh.DragHeating f64[ngas]
  DevBuf dust_idx, dust_work, dust_pairs;   // ... its grain list, per-grain planes, sorted pairs
  DevBuf sfr_work;                  // ghip_sfr_cooling (ghip_sfr.hip): candidate flags, offsets, counts
  int timestep_endrun = 0;   // endrun code of the last ghip_advance_timesteps failure
  // the shipped bundle's integrator (ghip_set_integration_flags, ghip_kick.hip / ghip_drift.hip)
  bool iflags_on = false;
  ghip_integration_flags iflags = {};
  DevBuf kick_drag, kick_ddm, kick_newdens;   // f64[3][ngas], f64[3][ngas], f64[n]
  bool has_drag = false, has_ddm = false, has_newdens = false;
  int kick_fields_n = -1, kick_fields_ngas = -1;   // counts the fields were set for
  // wind particles (ghip_wind.hip): the list and its orders, per-particle planes, sorted pairs; the resident gas
  // fields Injected_BH_Momentum and RadAccel f64[3][ngas] with the gas count they hold (-1: not made yet)
  DevBuf wind_idx, wind_work, wind_pairs, wind_inj, wind_ra;
  int wind_inj_ngas = -1, wind_ra_ngas = -1;
  bool rad_accel_on = false;        // ghip_set_rad_accel: kick, PM kick and drift read RadAccel
  hipEvent_t wind_ev[8] = {};       // phase marks of ghip_wind_feedback (made by its first call)
  double wind_ms[5] = {0, 0, 0, 0, 0};
  RowTable wk{GHIP_WK_COUNT, "wind", "index", "ghip_winds_set_table"};   // the resident wind table
  DevBuf wk_spawn, wk_rnd;          // ghip_wind_spawn: per-sink counts, offsets and records; its copy of a RndTable

  // the physics switches of the dust passes (ghip_set_dust_model, ghip_dust.hip)
  bool dust_model_on = false;          // any switch set: the k_dust_grain<DustM> / k_dust_density<G, DustVel> instantiations run
  ghip_dust_model dust_model = {};
  bool id_given = false;               // GHIP_F_ID has been set since the counts last changed
  // the viscosity of the pair loop (ghip_set_viscosity, ghip_sph.hip / ghip_kick.hip)
  bool visc_on = false;                // any switch set: the k_hydro<TG, HydV> instantiations run
  ghip_visc_params visc = {};
  DevBuf visc_alpha, visc_dtalpha;     // f64[ngas] host order: SphP[].alpha, SphP[].Dtalpha (made on demand)
  int visc_ngas = -1;                  // gas count alpha was given for (-1: none since the counts changed)
  long long visc_epoch = 0;            // counts every change of alpha (ghip_visc_set_alpha, the kick)

  // ---- randomised subnodes (ghip_set_rnd_table, ghip_tree.hip) ----
  DevBuf rnd_table;                // f64[rnd_n]: the host's RndTable
  int rnd_n = 0;                   // 0: no table bound (the level-GHIP_BITS leaf of identical keys)
  unsigned int rnd_gen = 0;        // picks the set of DevWords::rnd_info a build counts in

  // ---- asynchronous tree build (ghip_tree.hip) ----
  // A build whose particle number equals the previous build's is enqueued without the host waiting
  // for the node counts: buffers are sized by capacity, every kernel reads the sizes on the device
  // (TreeSizes).  The counts are VERIFIED -- the host waits for ev_sizes only, recorded right after the
  // counting stage, not for the walks -- before anything persistent is modified on their basis
  // (ghip_tree_verify: entry of ghip_density and of everything that joins).  A build that turns out
  // bad (more nodes than the buffers hold, key runs too long for the 32-bit sort) left nelem = 0 on
  // the device, so whatever ran on it did nothing; it is then repeated synchronously and the gravity
  // calls made since are replayed from grav_log.
  bool async = false;              // ghip_set_async: drift / kick report their errors at the next sync
  bool tree_unverified = false;
  bool tree_async_ok = true;       // GHIP_TREE_SYNC=1 switches the asynchronous build off
  hipEvent_t ev_sizes = nullptr, ev_sizes_gas = nullptr;
  bool gas_unverified = false;     // the same for the gas tree, whose whole build is deferred (ghip_finish_gas_tree)
  bool gas_async = false;          // ... and follows the gravity tree's mode
  int build_gen = 0;
  bool sort_wide = false;          // sticky: a build met key runs too long for the 32-bit sort
  bool in_recover = false;
  struct GravCall
  {
    ghip_grav_params p;
    int walk;
  };
  std::vector<GravCall> grav_log;  // gravity calls since the last tree build
  std::vector<void *> host_pins;   // ranges page-locked by ghip_pin_host
  bool hydro_early = false;        // ghip_set_hydro_release
  // ---- the gravity tree between two full builds (ghip_set_dynamic_tree, ghip_export.hip): a copy of
  // the last full build's element list whose nodes are drifted and kicked as forcetree.c:1356-1520
  // does; the gravity walks of a sub-step read it instead of the tree of the current positions ----
  bool dyn_on = false, dyn_valid = false, dyn_use = false;
  DynTree dyn;
  // balance of a Newton + Ewald pair (ghip_gravity.hip, pair_balance): dynamic LDS per Newtonian
  // workgroup in use, and a ring of the last pairs' start / end events with the cap they ran under.
  // A fresh context starts with 5 Newtonian wavefronts per SIMD: 5 * 56 + 112 + 112 registers host
  // the Ewald walk and a density wavefront next to them.
  int pair_lds = GHIP_PAIR_LDS(5);
  hipEvent_t pc_ev[4][4] = {};         // made by the first pair
  int pc_cap[4] = {0, 0, 0, 0};        // 0: slot empty or already read
  int pc_hyd[4] = {0, 0, 0, 0};        // the hydro kernel was queued underneath that pair
  int pc_head = 0;
  float pc_cost[GHIP_PAIR_NSET] = {-1.f, -1.f, -1.f};   // last measured cost of a pair under setting k
  int pc_age[GHIP_PAIR_NSET] = {0, 0, 0};               // pairs launched since that measurement
  hipEvent_t ev_side = nullptr;    // end of ghip_gravity_to_records' work on the pair's stream

  // ---- run statistics without a host synchronisation per step (ghip_run_begin / ghip_step_begin /
  // ghip_step_end / ghip_get_run_stats): a ring of event sets, the run's counter slots (rslots) ----
  std::vector<hipEvent_t> ev_ring;     // [slots][GHIP_NEV + 2]: phase events + step begin / end marks
  int ring_slots = 0, ring_cur = -1;   // ring_cur < 0: the fixed set ev[] is in use
  hipEvent_t *evp = nullptr;           // the event set in use (ev[] or a ring slot)
  long long run_steps = 0, run_syncs0 = 0, run_launches0 = 0, run_dens_iter = 0;
  long long n_syncs = 0;               // blocking host waits inside the library since creation
  // ---- ghip_potential / ghip_global_quantities (ghip_potential.hip) ----
  DevBuf pot;                      // f64[n]: P[].p.Potential of the last ghip_potential, host order
  DevBuf pot_nint;                 // u64[n]: its interactions per target, host order
  int pot_n = -1;                  // particle count of that call (-1: none)
  DevBuf potcorr;                  // f64[(EN+1)^3]: potcorr / BoxSize (forcetree.c:4466-4525)
  double potcorr_box = 0;
  DevBuf srpot;                    // float[NTAB]: shortrange_table_potential (forcetree.c:4201)
  DevBuf gq_work;                  // partial sums, kick tables and photon momenta of ghip_global_quantities
  FofState fof;                    // ghip_fof (ghip_fof.hip)
  SeqState seq;                    // ghip_rearrange / ghip_peano_order (ghip_sequence.hip)
  RowTable sk{GHIP_SK_COUNT, "sink", "ID", "ghip_sinks_set_table"};   // the resident sink table (ghip_accretion.hip)
  DevBuf sfr_cand;                 // i32: the candidates of the last ghip_sfr_cooling, in active-list order
  int sfr_ncand = -1;              // their number (-1: none in place; ghip_sfr_form_sinks consumes them)
};
#define GHIP_NEV 16

// every blocking wait of the host goes through these two (they are counted: ghip_run_stats)
static inline hipError_t ghip_stream_sync(ghip_ctx *ctx, hipStream_t st)
{
  ctx->n_syncs++;
  return hipStreamSynchronize(st);
}
static inline hipError_t ghip_event_sync(ghip_ctx *ctx, hipEvent_t e)
{
  ctx->n_syncs++;
  return hipEventSynchronize(e);
}
long long ghip_launch_count(void);   // kernel launches issued through this library so far (ghip_api.hip)
int ghip_tree_verify(ghip_ctx *ctx);  // tree.hip
int ghip_gas_verify(ghip_ctx *ctx);

int ghip_fail(ghip_ctx *ctx, int code, const char *fmt, ...);
// Device error words: ints in pinned, device-visible host memory that kernels set when an internal
// invariant breaks.  Every synchronising entry point (ghip_sync, ghip_get_field, the AoS downloads,
// ghip_get_stats) calls ghip_check_device_errors after its stream sync and fails with GHIP_EDEVICE.
#define GHIP_ERRW_PLAN 0     // wavefront plan of a gravity walk exceeded its grid (ghip_walk.h)
#define GHIP_ERRW_LET 1      // a target wanted to open a pruned node of another shard's tree
#define GHIP_ERRW_TREE 2     // tree emission wrote outside the element list / malformed import
#define GHIP_ERRW_PM 3       // non-periodic mesh: a mesh index outside the lower octant was refused (ghip_pm.hip)
#define GHIP_ERRW_DRIFT 4    // a particle was ahead of the drift target (reference: endrun(12), predict.c:148)
#define GHIP_ERRW_TIMESTEP 5 // the endrun code of a failed timestep criterion (888, 818, 112313)
#define GHIP_ERRW_COUNT 8
// (one block per process, shared by its contexts: an error raised by a kernel of one logical shard
// is seen by whichever context synchronises next.  Made once, by the first ghip_create.)
int *ghip_errwords(void);
static inline int *ghip_errword(ghip_ctx *, int which) { return ghip_errwords() + which; }
int ghip_check_device_errors(ghip_ctx *ctx);
// ghip_kick.hip: TimeBinCount[32] | TimeBinCountSph[32] recounted over all particles (k_timebin_histogram), on the
// host when this returns: the one 64-word blocking read of ghip_timebin_counts and ghip_find_next_sync_point
int ghip_timebin_hist(ghip_ctx *ctx, unsigned long long hist[64]);
// The overlapped Newton+Ewald pair returns with its walks still running on their own streams, so
// that the SPH phases -- which read and write nothing the walks touch -- can be enqueued on the
// main stream underneath them.  Every other entry point first makes the main stream wait for the
// pair (GHIP_JOIN at its top).
int ghip_join(ghip_ctx *ctx);        // wait for a pair in flight AND complete a deferred gas tree
// Workgroup size of the short kernels that may run underneath a gravity pair: the walks use
// one-wavefront workgroups, and a 256-thread workgroup -- which needs four free wavefront slots in
// one CU at the same moment -- would starve behind them however high its stream's priority.
static inline int ghip_wg(const ghip_ctx *ctx) { return ctx->grav_pending ? 64 : 256; }
// The same for a device-to-device copy of 32-bit words on the main stream: hipMemcpyAsync becomes the
// runtime's copy kernel, whose large workgroups wait for milliseconds behind a pair that fills every
// register of the SIMDs (3.4 and 1.6 ms for the two 1 MB target lists in front of the density loop
// at c2).  One-wavefront workgroups of a dozen registers take the first slot that frees (ghip_tree.hip).
int ghip_copy_i32(ghip_ctx *ctx, int *dst, const int *src, size_t n);
// pinned word the record unpack sets when a record of the gas block [0, ngas) is not Type 0
static inline int *ghip_gas_mixed_word(ghip_ctx *ctx) { return &ctx->pinned->gas_mixed; }
static inline DevWords *ghip_words(ghip_ctx *ctx) { return reinterpret_cast<DevWords *>(ctx->words.p); }
static inline unsigned long long *ghip_cslot(ghip_ctx *ctx, int kind)
{
  return reinterpret_cast<unsigned long long *>(ctx->cslots.p) + (size_t) kind * GHIP_CKIND_U64;
}
static inline unsigned long long *ghip_rslot(ghip_ctx *ctx, int kind)
{
  return reinterpret_cast<unsigned long long *>(ctx->rslots.p) + (size_t) kind * GHIP_CKIND_U64;
}
// host copy of a slot buffer added up: out[kind][which], which = 0, 1
int ghip_read_slots(ghip_ctx *ctx, DevBuf &buf, unsigned long long out[GHIP_CK_COUNT][2]);
// the marks in the mass of a gas record, gp[8 s + 3] (k_mark_converted in ghip_tree.hip says who sets and who
// removes them): a record that no neighbour loop sums.  The loops test mass < 0.
#define GAS_MARK_CONVERTED (-1.0)   // Type != 0; a ghost carries it from its owner (k_ghost_pack); never removed
#define GAS_MARK_MASSLESS (-2.0)    // Mass == 0 under ghip_set_massless_gas_rule; off for hydro_force() under rule 1
int ghip_mark_converted_gas(ghip_ctx *ctx);
int ghip_sink_buffers(ghip_ctx *ctx);        // SwallowID / Injected_BH_Energy, zeroed when first made
// ghip_sink.hip, for the resident forms of ghip_accretion.hip: the h iteration of the sinks and one pass of its
// kernel sums; the marking pass and the swallow pass (with the victims' masses zeroed) for ns records on the device
void sink_iter_init(SinkIter &I, int ns);
int sink_iterate(const ghip_dens_params *p, double ngb_factor, int ns, const double *sums, int ncur, SinkIter &I);
int sink_density_pass(ghip_ctx *ctx, const ghip_dens_params *p, int ns, const SinkRec *drecs, double *dh,
                      int *dslot, double *dout, const SinkIter &I, int ncur, int local_only);
int ghip_bh_launch_evaluate(ghip_ctx *ctx, const ghip_bh_params *p, int ns, const SinkRec *drecs);
int ghip_bh_launch_swallow(ghip_ctx *ctx, const ghip_bh_params *p, int ns, const SinkRec *drecs,
                           const double *dpbh, int *dvict, double *dout);
// ghip_accretion.hip: ghip_rearrange drops the rows of the Type-5 particles it eliminates (a table exists)
int ghip_sinks_drop_eliminated(ghip_ctx *ctx, int n_before, const int *new_of_old);
// ghip_wind.hip: the wind table through a reordering (every index through new_of_old, the rows of eliminated
// particles dropped, ascending order restored); what every entry point of the resident wind section refuses
int ghip_winds_remap(ghip_ctx *ctx, const char *who, int n_before, const int *new_of_old);
int ghip_winds_enter(ghip_ctx *ctx, const char *who, bool dd = false);
// the wind rows in GHIP_DD_MIGRATE: before anything moves, the rows of the departing Type-3 particles (list: the runs
// of the destinations, scount / soff as multi_select left them); the exchange left pending; after it the table
// re-keyed to the new layout and merged with the arrivals
int ghip_winds_mig_pack(ghip_ctx *ctx, int total, const int *list, const int *scount, const int *soff);
void ghip_winds_mig_post(ghip_ctx *ctx);
int ghip_winds_mig_merge(ghip_ctx *ctx);
// ghip_sequence.hip, for ghip_wind_spawn: the state grows from n to nn particles.  _begin gives the map to fill,
// old_of_new [nn] on the device (the source record of every record of the new layout); _apply moves every plane
// along it and leaves the state as after ghip_rearrange, the maps of ghip_sequence_get_map included
int ghip_seq_grow_begin(ghip_ctx *ctx, int nn, int **old_of_new);
int ghip_seq_grow_apply(ghip_ctx *ctx, int nn);
// the rows in GHIP_DD_MIGRATE (ghip_accretion.hip): the rows of the departing Type-5 particles `list` (destination
// 1 << r in mask[]) packed per destination; the second exchange posted; departed rows out, arrivals in, sorted
int ghip_sinks_mig_pack(ghip_ctx *ctx, int total, const int *list, const unsigned long long *mask);
void ghip_sinks_mig_post(ghip_ctx *ctx);
int ghip_sinks_mig_merge(ghip_ctx *ctx);
// the resident form of the sink operations on shards (ghip_accretion.hip), called by ghip_dd_sink_begin / _step
int ghip_dd_sinks_begin(ghip_ctx *ctx, int op, const void *params);
int ghip_dd_sinks_step(ghip_ctx *ctx);
int ghip_dd_sinks_store_density(ghip_ctx *ctx);
int dd_sink_density_pass(ghip_ctx *ctx);
int ghip_unmark_massless_for_hydro(ghip_ctx *ctx);
int ghip_remark_massless_for_density(ghip_ctx *ctx);
int ghip_check_gas_types(ghip_ctx *ctx);   // after TYPE changed: recount, sets ctx->gas_mixed (synchronises)
// kField[] of ghip_api.hip, for the migration (ghip_dd.hip) and the record members (ghip_records.hip)
void ghip_field_info(int f, int *gas, int *ncomp, int *isint);
int ghip_dyn_capture(ghip_ctx *ctx);                 // after a full build: copy the gravity tree, vs / vmax per node
int ghip_dyn_kick_recorded(ghip_ctx *ctx);           // force_kick_node for what ghip_advance_timesteps recorded
void ghip_dyn_release(ghip_ctx *ctx);
int ghip_fill_walk_records(ghip_ctx *ctx, TreeDev &t);
int ghip_gravity_finish_on(ghip_ctx *ctx, double G, int pmgrid, double comoving_fac, int all_shards,
                           hipStream_t st);
int ghip_join_pair(ghip_ctx *ctx);   // wait for a pair in flight only (entry of the gravity walks)
int ghip_finish_gas_tree(ghip_ctx *ctx);   // complete a deferred gas tree (entry of the SPH phases)
// ghip_wind.hip: SphP[].ra.RadAccel [3][ngas] for the kick, the PM kick and the drift (nullptr: ghip_set_rad_accel off)
int ghip_rad_accel_field(ghip_ctx *ctx, const char *who, const double **ra);
#define GHIP_JOIN(ctx)                          \
  do                                            \
    {                                           \
      int j_ = ghip_join(ctx);                  \
      if(j_ != GHIP_OK)                         \
        return j_;                              \
    }                                           \
  while(0)
void ghip_pm_release(ghip_ctx *ctx);
// The mesh part of the potential (ghip_pm.hip), for pot.pm.pmgrid != 0: pmpotential_periodic with
// pot.grav.periodic, else pmpotential_nonperiodic(0) -- decided there.  _check: the argument rules of ghip_potential.
// _deposit: this context's particles onto its (zeroed) mesh; *b is the block a shard all-gathers (the periodic mesh;
// the open mesh's octant and its status word), outside = 1 when a particle lies outside the open mesh's region
// (nothing deposited then; always 0 for the periodic mesh).  _solve: all != nullptr: the mesh is the sum of the
// nranks gathered blocks in rank order, GHIP_EREGION if a status word says so, before anything is written; else
// pot[i] += the mesh potential at particle i.
struct PmBlock
{
  const void *p;
  size_t bytes;
  int outside;
};
int ghip_pm_pot_check(ghip_ctx *ctx, const ghip_pot_params *p, const char *who);
int ghip_pm_pot_deposit(ghip_ctx *ctx, const ghip_pot_params *p, PmBlock *b);
int ghip_pm_pot_solve(ghip_ctx *ctx, const ghip_pot_params *p, int nranks, const double *all, double *pot);
// ghip_decomp.hip: one pass of k_decomp_extent over the resident positions into the block `own` (EXTENT_WORDS
// u64: images of xmin[3], xmax[3], the count, time bins, the error word; an empty context contributes +MAX / -MAX).
// A failure of the pass itself is returned AND marked in the block, so that peers of a collective stop with it.
#define EXTENT_WORDS 16
int ghip_extent_pass(ghip_ctx *ctx, DevBuf &own, int use_work);
// ... and the blocks of nranks contexts evaluated in rank order (host copies): 0, or the error bits met
// (first on rank *bad)
unsigned long long ghip_extent_reduce(const unsigned long long *all, int nranks, double xmin[3], double xmax[3],
                                      unsigned long long *ntot, int *bmin, int *bmax, int *bad);
#define EXTENT_ERR_POS 1ULL     // a position that is not finite
#define EXTENT_ERR_WORK 2ULL    // a TimeBin outside [0, TIMEBINS] or a negative GravCost
#define EXTENT_ERR_LOCAL 4ULL   // the pass itself failed on that rank

#define HIPCHK(call)                                                                         \
  do                                                                                         \
    {                                                                                        \
      hipError_t e_ = (call);                                                                \
      if(e_ != hipSuccess)                                                                   \
        return ghip_fail(ctx, GHIP_EHIP, "%s:%d %s -> %s", __FILE__, __LINE__, #call,        \
                         hipGetErrorString(e_));                                             \
    }                                                                                        \
  while(0)

#define GCHK(call)            \
  do                          \
    {                         \
      int r_ = (call);        \
      if(r_ != GHIP_OK)       \
        return r_;            \
    }                         \
  while(0)

int ghip_ensure(ghip_ctx *ctx, DevBuf &b, size_t bytes);
static inline int cdiv(long long a, int b) { return (int) ((a + b - 1) / b); }

template <class T> static inline T *P(DevBuf &b) { return reinterpret_cast<T *>(b.p); }
template <class T> static inline const T *P(const DevBuf &b) { return reinterpret_cast<const T *>(b.p); }

// Target sharding (multi-GPU).  The curve-ordered target list is cut into buckets of 64; rank r
// owns buckets r, r+N, r+2N, ... (every rank samples the whole volume, so per-rank cost is
// balanced without a cost model).  The list is stored rank-major, so a rank's targets are the
// contiguous range [lo, lo+cnt); `per` is the padded common slice length of the all-gathers.
static inline void ghip_shard_range(int nt, int nranks, int rank, int *lo, int *cnt, int *per)
{
  int nb = (nt + 63) / 64;
  int lastsize = nt - (nb - 1) * 64;
  int acc = 0, mine = 0, mylo = 0;
  for(int r = 0; r < nranks; r++)
    {
      int cb = (r < nb) ? (nb - r + nranks - 1) / nranks : 0;
      int c = cb * 64;
      if(cb > 0 && (nb - 1) % nranks == r)
        c -= 64 - lastsize;
      if(r == rank)
        {
          mylo = acc;
          mine = c;
        }
      acc += c;
    }
  *lo = mylo;
  *cnt = mine;
  *per = ((nb + nranks - 1) / nranks) * 64;
}

// tree.hip
int ghip_tree_build_impl(ghip_ctx *ctx);
int ghip_build_target_lists(ghip_ctx *ctx);
int ghip_gastree_refresh_hmax(ghip_ctx *ctx);
int ghip_gather_f64(ghip_ctx *ctx, int n, const int *perm, const double *src, double *dst);
int ghip_gather_f64_lim(ghip_ctx *ctx, int n, const int *perm, const double *src, int limit,
                        double *dst);
// gravity.hip
int ghip_gravity_impl(ghip_ctx *ctx, const ghip_grav_params *p, int walk);
int ghip_build_segments(ghip_ctx *ctx, TreeDev &t, bool walk_records);
// sph.hip
int ghip_density_impl(ghip_ctx *ctx, const ghip_dens_params *p);
int ghip_hydro_impl(ghip_ctx *ctx, const ghip_hydro_params *p);
int ghip_sph_fill_nodes(ghip_ctx *ctx, bool hmax_only);
int ghip_visc_buffers(ghip_ctx *ctx);                   // alpha / Dtalpha for the current gas count
int ghip_visc_ready(ghip_ctx *ctx, const char *who);   // the refusals of ghip_set_viscosity's mode
// dd.hip
void ghip_dd_release(ghip_ctx *ctx);
// the pieces of the gravity operation that GHIP_DD_POTENTIAL shares (ghip_potential.hip):
// the shard's own tree (nothing imported) after the key-range check; the group table over `nt` targets
// `tgt` of that tree (all = true: every particle of the shard) with its all-gather left pending; after it,
// the selection of the locally essential trees under the opening rules of gp, packed, the all-to-all-v
// left pending
int ghip_dd_own_tree(ghip_ctx *ctx);
int ghip_dd_post_groups(ghip_ctx *ctx, bool all, bool need_oldacc);
int ghip_dd_post_guests(ghip_ctx *ctx, const char *what);   // 1: the guest keys' exchange is pending, 0: no guests
int ghip_dd_post_let(ghip_ctx *ctx, const ghip_grav_params &gp);
// the operations of dd_ops[] (ghip_dd.hip; gravity, density, hydro and migration are static there): begin copies
// its own params into DDState and makes its own checks, step returns what ghip_dd_step returns
int ghip_dd_sink_begin(ghip_ctx *ctx, int op, const void *params, int walk);     // sink.hip: the three sink ops
int ghip_dd_sink_step(ghip_ctx *ctx);
int ghip_dd_pm_begin(ghip_ctx *ctx, int op, const void *params, int walk);       // pm.hip: GHIP_DD_PM
int ghip_dd_pm_step(ghip_ctx *ctx);
int ghip_dd_pmreg_begin(ghip_ctx *ctx, int op, const void *params, int walk);    // ... GHIP_DD_PM_REGION
int ghip_dd_pmreg_step(ghip_ctx *ctx);
int ghip_dd_pmnp_begin(ghip_ctx *ctx, int op, const void *params, int walk);     // ... GHIP_DD_PM_NONPERIODIC
int ghip_dd_pmnp_step(ghip_ctx *ctx);
int ghip_dd_dust_begin(ghip_ctx *ctx, int op, const void *params, int walk);     // dust.hip: the two dust ops
int ghip_dd_dust_step(ghip_ctx *ctx);
int ghip_dd_pot_begin(ghip_ctx *ctx, int op, const void *params, int walk);      // potential.hip
int ghip_dd_pot_step(ghip_ctx *ctx);
int ghip_dd_gq_begin(ghip_ctx *ctx, int op, const void *params, int walk);
int ghip_dd_gq_step(ghip_ctx *ctx);
int ghip_dd_fof_begin(ghip_ctx *ctx, int op, const void *params, int walk);      // fof.hip: GHIP_FOF_FORM of the above
int ghip_dd_fof_step(ghip_ctx *ctx);
int ghip_dd_decomp_begin(ghip_ctx *ctx, int op, const void *params, int walk);   // decomp.hip
int ghip_dd_decomp_step(ghip_ctx *ctx);
int ghip_dd_sync_begin(ghip_ctx *ctx, int op, const void *params, int walk);     // sync.hip: GHIP_SYNC_POINT_FORM
int ghip_dd_sync_step(ghip_ctx *ctx);
int ghip_dd_wind_begin(ghip_ctx *ctx, int op, const void *params, int walk);     // wind.hip: the wind forms of GHIP_DD_DUST_DRAG
int ghip_dd_wind_step(ghip_ctx *ctx);
int ghip_dd_spawn_begin(ghip_ctx *ctx, const void *params);                      // accretion.hip: GHIP_WINDS_SPAWN_FORM
int ghip_dd_spawn_step(ghip_ctx *ctx);
// all shards stop together: hold keeps rc (with ctx->err if it is a failure) and says whether it failed, the flag
// travels with the next exchange; raise(r = first rank whose flag is set, < 0: none, GHIP_OK) then fails with this
// shard's own code and message if it holds one, else with the formatted message and GHIP_EDEVICE
bool ghip_dd_hold(ghip_ctx *ctx, int rc);
int ghip_dd_raise(ghip_ctx *ctx, int failed_rank, const char *fmt, ...);
// the status round: {value, failed} uploaded, its all-gather left pending; then the largest value, the first failed rank
int dd_post_status(ghip_ctx *ctx, double value, bool failed);
int dd_read_status(ghip_ctx *ctx, double *worst, int *first_failed);

// ---------------------------------------------------------------------------------------------
// walk segments: the element list of a tree is cut into `ns` contiguous segments and `nsub`
// wavefronts share one bucket of 64 targets (wavefront `sub` takes segments sub, sub+nsub, ...);
// see ghip_walk.h "Load balance"
// ---------------------------------------------------------------------------------------------
#define GHIP_MAXANC 48      // >= GHIP_TREE_MAXLEVEL: a segment may start below a chain of that many nodes
#define GHIP_MAXSUB 8
struct WalkSeg
{
  int ns;                          // number of segments
  int nsub;                        // wavefronts per bucket
  const int *__restrict__ start;   // [ns+1] first element of each segment
  const int *__restrict__ nanc;    // [ns]
  const int *__restrict__ anc;     // [ns][GHIP_MAXANC] ancestors of start[k], root first
};

int ghip_walk_layout(const TreeDev &t, WalkSeg &sg, int table);   // returns nsub

// ---------------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------------
// 64-lane reductions, fixed order.  The butterflies leave the result in every lane.
#define GHIP_WAVE_REDUCE(name, T, expr)                    \
  __device__ __forceinline__ T name(T v)                   \
  {                                                        \
    for(int off = 32; off > 0; off >>= 1)                  \
      {                                                    \
        T o = __shfl_xor(v, off, 64);                      \
        v = expr;                                          \
      }                                                    \
    return v;                                              \
  }
GHIP_WAVE_REDUCE(d_wave_min_i32, int, o < v ? o : v)
GHIP_WAVE_REDUCE(d_wave_max_i32, int, o > v ? o : v)
GHIP_WAVE_REDUCE(d_wave_min_f64, double, o < v ? o : v)
GHIP_WAVE_REDUCE(d_wave_max_f64, double, o > v ? o : v)
GHIP_WAVE_REDUCE(d_wave_sum_f64, double, v + o)
GHIP_WAVE_REDUCE(d_wave_or_u64, unsigned long long, v | o)
#undef GHIP_WAVE_REDUCE

// element link record: x = skip (element index after this subtree), y = sorted particle index
// for a particle element or -(level+1) for a node, z = first particle of the node, w = count
#define LK_IS_PARTICLE(lk) ((lk).y >= 0)

__device__ __forceinline__ double d_nearest(double x, double boxsize, double boxhalf)
{
  // forcetree.c:49 NEAREST
  return (x > boxhalf) ? (x - boxsize) : ((x < -boxhalf) ? (x + boxsize) : x);
}

__device__ __forceinline__ double d_ngb_periodic(double x, int periodic, double boxsize,
                                                 double boxhalf)
{
  // allvars.h:300-308 NGB_PERIODIC_LONG_*
  double xt = fabs(x);
  return (periodic && xt > boxhalf) ? (boxsize - xt) : xt;
}

// (a shift-down sum: valid in lane 0 only)
__device__ __forceinline__ unsigned long long d_wave_sum_u64(unsigned long long v)
{
  for(int off = 32; off > 0; off >>= 1)
    v += __shfl_down(v, off, 64);
  return v;
}
