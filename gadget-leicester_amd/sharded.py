"""Force steps sharded over the GPUs of a node (one process per GPU).

Two modes:

* DOMAIN DECOMPOSITION (default; `decompose`, `DomainShards`, `DomainRank` below): every shard
  owns the particles of one Peano-Hilbert key range; tree nodes (locally essential trees) and
  ghost gas particles cross the links, in C over RCCL (ghip_dd_* in include/ghip.h).  This module
  only cuts the curve (`decompose`, calling the library's restatement of
  domain_findSplit_work_balanced) and drives the per-operation state machine.

* REPLICATED SOURCES (`ShardedForceStep`, the round-1 design, kept selectable): every rank holds
  all particles, targets are dealt out in buckets, results are all-gathered by torch.distributed.

----- replicated mode -----
One force step sharded over the GPUs of a node (one process per GPU, torch.distributed).

Replaces the reference's MPI export/import rounds (gravtree.c:175-339, density.c:193-389,
hydra.c:274-526).  Design ("Multi-GPU"): every rank holds all particles and builds
the same tree -- 288 GB of HBM makes replication cheap -- and evaluates one contiguous slice of
the space-filling-curve ordered target list; finished per-target results are exchanged with ONE
fixed-size all-gather per phase (RCCL over xGMI when the backend is "nccl"; gloo on CPU in the
tests).  No partial sums cross a link, so results are bit-identical to the single-GPU run.

The `engine` argument is duck-typed: gadget-leicester_amd.bindings.ForcePath on a GPU, or a CPU
stand-in with the same methods in tests/test_shard_gloo.py.
"""
GROUP_GRAVITY, GROUP_DENSITY, GROUP_HYDRO = 0, 1, 2
WIDTH = {GROUP_GRAVITY: 4, GROUP_DENSITY: 7, GROUP_HYDRO: 5}


class ShardedForceStep:
    def __init__(self, engine, rank, world, dist=None, device=None):
        self.e = engine
        self.rank = int(rank)
        self.world = int(world)
        self.dist = dist
        self.device = device
        self._buf = {}
        engine.set_shard(self.rank, self.world)

    def _buffers(self, group, per):
        import torch
        key = (group, per)
        if key not in self._buf:
            w = WIDTH[group]
            mine = torch.zeros(w * per, dtype=torch.float64, device=self.device)
            allb = torch.zeros(self.world * w * per, dtype=torch.float64, device=self.device)
            self._buf[key] = (mine, allb)
        return self._buf[key]

    def exchange_begin(self, group):
        """pack this rank's slice and start the all-gather of one phase; returns a handle for
        exchange_end (None for a single rank).  With the RCCL backend the collective runs
        asynchronously on its own stream, so it overlaps whatever is launched before
        exchange_end."""
        if self.world == 1:
            return None
        per, _ = self.e.shard_count(group != GROUP_GRAVITY)
        if per == 0:
            return None
        mine, allb = self._buffers(group, per)
        self.e.shard_pack(group, mine.data_ptr())      # synchronises the library's stream
        on_gpu = self.device is not None and str(self.device).startswith("cuda")
        work = None
        if on_gpu and self.dist.get_backend() == "gloo":
            # self-test configuration (several ranks sharing one GPU): stage through the host
            host_all = allb.cpu()
            self.dist.all_gather_into_tensor(host_all, mine.cpu())
            allb.copy_(host_all)
        elif on_gpu:
            work = self.dist.all_gather_into_tensor(allb, mine, async_op=True)
        else:
            self.dist.all_gather_into_tensor(allb, mine)
        return (group, allb, work, on_gpu)

    def exchange_end(self, handle):
        if handle is None:
            return
        group, allb, work, on_gpu = handle
        if work is not None:
            work.wait()          # orders torch's current stream behind the collective
        if on_gpu:
            # wait for that stream only: a device-wide synchronize would also wait for a gravity
            # pair still in flight on the library's own streams and undo the overlap
            import torch
            done = torch.cuda.Event()
            done.record()
            done.synchronize()
        self.e.shard_unpack(group, allb.data_ptr(), self.world)

    def exchange(self, group):
        """all-gather this phase's per-target results; no-op for a single rank."""
        self.exchange_end(self.exchange_begin(group))

    def step(self, tree_args, grav_params, dens_params, hydro_params, G, walks, has_gas=True):
        """tree build -> gravity walks -> density -> hmax -> hydro, with the three exchanges.
        Nothing in the SPH phases reads the gravity results: with the paired walk
        (GHIP_WALK_NEWTON_EWALD) the gravity kernels are still running on their own streams when
        the SPH phases are enqueued, and the gravity exchange comes last."""
        e = self.e
        e.tree_build(*tree_args)
        pair = getattr(e, "WALK_PAIR", None)
        if pair is not None and list(walks) == [pair[0], pair[1]]:
            e.gravity(grav_params, pair[2])     # both walks in one call, returns with them in flight
        else:
            for w in walks:
                e.gravity(grav_params, w)
        if has_gas:
            e.density(dens_params)
            self.exchange(GROUP_DENSITY)
            e.update_hmax()
            e.hydro(hydro_params)
            self.exchange(GROUP_HYDRO)
        self.exchange(GROUP_GRAVITY)
        if hasattr(e, "gravity_finish_all"):
            e.gravity_finish_all(G)    # OldAcc / G scaling for every particle, on every rank
        else:
            e.set_shard(0, 1)
            e.gravity_finish(G)
            e.set_shard(self.rank, self.world)


# ================================================================================================
# domain decomposition
# ================================================================================================
import importlib as _importlib

import numpy as _np


def _bindings():
    return _importlib.import_module(__package__ + ".bindings")


def histogram_level(n):
    """Level of the key histogram the curve is cut on: about 32 particles per cell, 8^level cells,
    level in 1..7 (the reference refines its top-tree until a leaf holds few particles,
    domain.c:1738-1960; a fixed level is enough for the sizes of BASELINE's configs)."""
    level = 1
    while level < 7 and 8 ** level * 32 < n:
        level += 1
    return level


def decompose(keys, nranks, work=None, level=None):
    """Cut the Peano-Hilbert curve into `nranks` contiguous ranges of about equal work.
    keys: uint64 Peano-Hilbert keys (21 bits per dimension) of ALL particles; work: per-particle
    cost, the reference's (1 + GravCost) / 2^TimeBin (domain.c:378-384), default 1.
    The work is summed per level-`level` cell and the cells are cut by the library's
    ghip_dd_find_split = domain_findSplit_work_balanced (domain.c:1075-1113).
    Returns (splits[nranks+1] uint64, owner[n] int)."""
    keys = _np.ascontiguousarray(keys, _np.uint64)
    n = len(keys)
    if level is None:
        level = histogram_level(n)
    while 8 ** level < nranks:
        level += 1
    shift = _np.uint64(63 - 3 * level)
    cell = (keys >> shift).astype(_np.int64)
    w = _np.ones(n) if work is None else _np.asarray(work, _np.float64)
    hist = _np.bincount(cell, weights=w, minlength=8 ** level)
    start, end = _bindings().dd_find_split(nranks, hist)
    splits = _np.zeros(nranks + 1, _np.uint64)
    for r in range(nranks):
        splits[r] = _np.uint64(int(start[r])) << shift
    splits[0] = 0
    splits[nranks] = _np.uint64(1) << _np.uint64(63)
    owner = _np.searchsorted(splits[1:nranks], keys, side="right").astype(_np.int32)
    return splits, owner


def find_guests(keys, holder, splits=None, segments=None):
    """The guests of a layout: particles whose Peano-Hilbert key lies outside every piece of the curve that
    the rank holding them owns (ghip_dd_set_guests).  keys: uint64 keys; holder: the rank that holds each
    particle; the layout as `splits` (nranks+1 keys, rank r owns [splits[r], splits[r+1])) or as
    `segments` = (keys[nseg+1], owner[nseg]) (ghip_dd_set_segments).  A key equal to a boundary belongs to
    the piece above it; an empty piece owns nothing.  Returns (guest_indices ascending, host_of_guest): the
    host is the rank that owns the guest's key."""
    keys = _np.ascontiguousarray(keys, _np.uint64)
    holder = _np.asarray(holder, _np.int64)
    if (splits is None) == (segments is None):
        raise ValueError("find_guests: give the layout as splits or as segments")
    if segments is not None:
        bounds = _np.ascontiguousarray(segments[0], _np.uint64)
        owner = _np.asarray(segments[1], _np.int64)
    else:
        bounds = _np.ascontiguousarray(splits, _np.uint64)
        owner = _np.arange(len(bounds) - 1, dtype=_np.int64)
    if len(bounds) != len(owner) + 1:
        raise ValueError("find_guests: nseg + 1 keys for nseg owners")
    # the last piece that starts at or before the key: empty pieces share their start with the next one,
    # which side="right" steps over
    piece = _np.searchsorted(bounds[:-1], keys, side="right") - 1
    host = owner[piece]
    guests = _np.nonzero(host != holder)[0]
    return guests, host[guests].astype(_np.int32)


def _empty_wind_state():
    z = _np.zeros(0)
    return dict(stellar_age=z, birth_energy=z, old_momentum=z, new_density=z, drmin=z)


def _fof_result(path, keep):
    out = path.fof_adopt(keep)
    out.counts = keep["counts"]
    return out


def _rearrange(path, how):
    if how is True:
        return path.rearrange()
    return path.rearrange(bool(how.fix_converted), bool(how.eliminate_massless))


def _elim_counts(res):
    return (int(res.count_elim), int(res.count_gaselim), int(res.count_dustelim))


def _redistributed(results, counts, ordered):
    tot = [sum(c[k] for c in counts) for k in range(3)]
    return dict(results=results, tot_elim=tot[0], tot_gaselim=tot[1], tot_dustelim=tot[2], ordered=ordered)


class DomainShards:
    """All shards of a run as contexts of THIS process (one after the other on one GPU, or one per
    visible GPU): the parity-test and rehearsal form of the multi-GPU path.  Exchanges are
    device-to-device copies (ghip_dd_exchange_local); everything else is the code the RCCL path
    runs."""

    def __init__(self, paths):
        self.paths = list(paths)
        self.B = _bindings()

    def run(self, op, params, walk=0):
        prm = params if isinstance(params, (list, tuple)) else [params] * len(self.paths)
        self.B.dd_run_local(self.paths, op, prm, walk)

    def gravity(self, params, walk):
        self.run(self.B.DD_GRAVITY, params, walk)

    def density(self, params):
        self.run(self.B.DD_DENSITY, params)

    def hydro(self, params):
        self.run(self.B.DD_HYDRO, params)

    def migrate(self):
        self.run(self.B.DD_MIGRATE, None)

    def accept_guests(self, on=True):
        """ghip_dd_set_guests on every shard: gravity and potential accept resident particles that left
        their shard's pieces of the curve since the last migration"""
        for p in self.paths:
            p.dd_set_guests(on)

    def set_viscosity(self, params=None):
        """ghip_set_viscosity on every shard (the setting must be the same on all of them)"""
        for p in self.paths:
            p.set_viscosity(params)

    def set_dust_model(self, model=None):
        """ghip_set_dust_model on every shard (the setting must be the same on all of them)"""
        for p in self.paths:
            p.set_dust_model(model)

    def visc_set_alpha(self, alpha, dtalpha=None):
        """per shard: alpha (and Dtalpha or None) of its own gas, in its order.  Before density(): a ghost
        carries its owner's alpha as of the ghost refresh that ends GHIP_DD_DENSITY."""
        for r, p in enumerate(self.paths):
            p.visc_set_alpha(alpha[r], None if dtalpha is None else dtalpha[r])

    def visc_get(self):
        """[(alpha, Dtalpha)] per shard"""
        return [p.visc_get() for p in self.paths]

    def decompose(self, params=None):
        """GHIP_DD_DECOMPOSE(DecompParams; None = automatic level, unit weights, the cube kept): new key
        ranges (and on request a new cube) from the resident particles of all shards.  Moves nothing."""
        self.run(self.B.DD_DECOMPOSE, params if params is not None else self.B.DecompParams())

    def redistribute(self, params=None, rearrange=None, peano_order=False):
        """decompose, then migrate: afterwards every particle sits on the shard its key names.  As
        domain_Decomposition() does (domain.c:120-135, 281-285): with rearrange = a RearrangeParams (or True: both
        of its switches) every shard first runs ghip_rearrange, and with peano_order every shard ends with
        ghip_peano_order in the domain in force.  Returns None with the defaults, else a dict: results (one
        RearrangeResult per shard, or None), tot_elim / tot_gaselim / tot_dustelim (their sums), ordered (per
        shard: whether the order moved a record)."""
        if rearrange is None and not peano_order:
            self.decompose(params)
            self.migrate()
            return None
        results = None
        if rearrange is not None:
            results = [_rearrange(p, rearrange) for p in self.paths]
        self.decompose(params)
        self.migrate()
        ordered = [p.peano_order() for p in self.paths] if peano_order else None
        return _redistributed(results, [_elim_counts(r) for r in results] if results else [], ordered)

    def pm_region(self, pmgrid):
        """GHIP_DD_PM_REGION: the region of the non-periodic mesh from the resident particles of all shards,
        stored on every shard (the same bytes); returns it (PmRegion)"""
        import ctypes as C
        self.run(self.B.DD_PM_REGION, C.c_int(int(pmgrid)))
        return self.paths[0].pm_get_region()

    def pm_nonperiodic(self, params):
        """GHIP_DD_PM_NONPERIODIC(PmnpParams): every shard's F_GRAVPM; GhipError with GHIP_EREGION when a
        particle of any shard left the region: pm_region(), then call again"""
        self.run(self.B.DD_PM_NONPERIODIC, params)

    def sync_point(self, ti_current, ti_nextoutput=-1):
        """GHIP_DD_DECOMPOSE in its SYNC_POINT_FORM: the next sync point of ALL shards' particles and every shard's own active list
        (get_active()) -> [SyncPoint] in shard order; Ti_next, TimeBinActive, GlobNumForceUpdate and
        Flag_FullStep are the same on all of them.  A TIMEBIN outside [0, 28] on one shard: GhipError on all,
        no list changed."""
        self.run(self.B.DD_DECOMPOSE, self.B.SyncParams(int(ti_current), int(ti_nextoutput)), self.B.SYNC_POINT_FORM)
        return [p.dd_get_sync_point() for p in self.paths]

    def potential(self, params):
        """GHIP_DD_POTENTIAL(PotParams): afterwards every path's get_potential() / get_potential_interactions()
        give its own particles"""
        self.run(self.B.DD_POTENTIAL, params)

    def global_quantities(self, params, tables=None, per_shard=None):
        """GHIP_DD_GLOBAL_QUANTITIES(GlobalParams): the sums of the whole system as every shard holds them, a
        list of dicts (GlobalSums.asdict) in shard order.  tables: dict(grav_kick_table=, hydro_kick_table=);
        per_shard: one dict per shard of its own old_photon_momentum / potential arrays."""
        built = [self.B.dd_global_args(params, p.n, **(tables or {}), **((per_shard or [{}] * len(self.paths))[r]))
                 for r, p in enumerate(self.paths)]
        self.run(self.B.DD_GLOBAL_QUANTITIES, [b[0] for b in built])
        return [b[1]["out"].asdict() for b in built]

    def fof(self, **params):
        """GHIP_DD_GLOBAL_QUANTITIES begun with walk = FOF_FORM (params: those of ForcePath.fof, the same for all):
        the friends-of-friends groups of the whole system on the merged trees of this step's gravity().  Returns
        the FofResult per shard (with .counts: int64[8], bindings.FOF_COUNTS); afterwards every path's fof_groups()
        / fof_maxdens_task() give the complete catalogue, fof_labels() / fof_ids() its own particles."""
        built = [self.B.dd_fof_args(**params) for _ in self.paths]
        self.run(self.B.DD_GLOBAL_QUANTITIES, [b[0] for b in built], self.B.FOF_FORM)
        return [_fof_result(p, b[1]) for p, b in zip(self.paths, built)]

    def wind_feedback(self, params, wind, state):
        """GHIP_DD_WIND in its WIND_FORM, the whole loop (momentum_feedback.c:283-568): wind[r] are shard r's local indices in list
        order, state[r] its dict(stellar_age, birth_energy, old_momentum, new_density, drmin) or None where the
        shard has no wind.  params.dt_total_floor is the GLOBAL floor.  Returns one dict per shard as
        ForcePath.wind_feedback does: iterations is the global count, bits / ndeleted / deleted_momentum are the
        shard's own (add them in rank order); counts: int64[6] (bindings.WIND_COUNTS).  Afterwards wind particles
        may lie outside their shard's key ranges: redistribute(), or accept_guests()."""
        built = [self.B.dd_wind_args(params, wind[r], state=state[r] if len(wind[r]) else _empty_wind_state())
                 for r in range(len(self.paths))]
        self.run(self.B.WIND_OP, [b[0] for b in built], self.B.WIND_FORM)
        return [self.B.dd_wind_result(b[1]) for b in built]

    def winds_feedback(self, params):
        """GHIP_DD_WIND in its WINDS_RESIDENT_FORM: ForcePath.winds_feedback as one collective.  Every shard lists
        its active Type-3 particles that have a row with StellarAge < Time in its wind table (dd_winds_set_table),
        takes the state from the rows and writes it back.  Returns one dict per shard: iterations (global), the
        shard's bits / ndeleted / deleted_momentum, counts.  An active Type-3 particle without a row, or a shard
        without a table: GhipError on all shards, nothing changed."""
        built = [self.B.dd_winds_args(params) for _ in self.paths]
        self.run(self.B.WIND_OP, [b[0] for b in built], self.B.WINDS_RESIDENT_FORM)
        return [self.B.dd_wind_result(b[1]) for b in built]

    def wind_spawn(self, params, rnd):
        """GHIP_DD_WIND in its WINDS_SPAWN_FORM: ForcePath.wind_spawn as one collective.  Every shard's massive active
        sinks (found in its sink table) create wind particles behind its own particles and rows in its wind table;
        rnd is the host's RndTable, which must be given.  Returns one dict per shard as ForcePath.wind_spawn does,
        with tot_spawned, the sum over all shards; every path's .n follows.  One shard that cannot (no table, a
        missing row, MaxPart): GhipError on all shards, nothing changed anywhere."""
        built = [self.B.dd_winds_args(spawn=params, rnd_table=rnd) for _ in self.paths]
        self.run(self.B.WIND_OP, [b[0] for b in built], self.B.WINDS_SPAWN_FORM)
        for p in self.paths:
            p.counts()
        return [self.B.dd_winds_spawn_report(b[1]) for b in built]

    def sinks_density(self, params, ngb_factor):
        """GHIP_DD_SINK_DENSITY in its SINKS_RESIDENT_FORM: ForcePath.sinks_density for the active Type-5 particles
        of all shards, each found in its shard's sink table -> the iteration count (the same on all shards)"""
        built = [self.B.dd_sinks_args(dens=params, ngb_factor=ngb_factor) for _ in self.paths]
        self.run(self.B.DD_SINK_DENSITY, [b[0] for b in built], self.B.SINKS_RESIDENT_FORM)
        return built[0][1]["iterations"].value

    def blackhole_accretion(self, bh_params, acc_params):
        """GHIP_DD_BH_SWALLOW in its SINKS_RESIDENT_FORM: blackhole_accretion() as one collective -> one dict per
        shard as ForcePath.blackhole_accretion returns it: the per-bin sums and nactive are those of the shard's
        own sinks, counts the particles of that shard that were swallowed (add them in rank order)"""
        built = [self.B.dd_sinks_args(bh=bh_params, acc=acc_params) for _ in self.paths]
        self.run(self.B.DD_BH_SWALLOW, [b[0] for b in built], self.B.SINKS_RESIDENT_FORM)
        return [self.B.dd_sinks_report(b[1]) for b in built]

    def wind_density(self, params, wind, dt_jump):
        """GHIP_DD_WIND in its WIND_DENSITY_FORM: one virtual_density() -> [(new_density, drmin, counts)] per shard"""
        built = [self.B.dd_wind_args(params, wind[r], dt_jump=dt_jump[r]) for r in range(len(self.paths))]
        self.run(self.B.WIND_OP, [b[0] for b in built], self.B.WIND_DENSITY_FORM)
        return [(b[1]["new_density"], b[1]["drmin"], b[1]["counts"].copy()) for b in built]

    def wind_spread(self, params, wind, dt_jump, new_density, delta_momentum):
        """GHIP_DD_WIND in its WIND_SPREAD_FORM: one virtual_spread_momentum() into every shard's resident
        Injected_BH_Momentum -> [counts] per shard"""
        built = [self.B.dd_wind_args(params, wind[r], dt_jump=dt_jump[r], new_density=new_density[r],
                                     delta_momentum=delta_momentum[r]) for r in range(len(self.paths))]
        self.run(self.B.WIND_OP, [b[0] for b in built], self.B.WIND_SPREAD_FORM)
        return [b[1]["counts"].copy() for b in built]


class DomainRank:
    """One shard per process.  transport "rccl": the exchanges run in C over RCCL; `bcast(obj)` is
    the host's broadcast from rank 0 (MPI_Bcast in the reference's world,
    torch.distributed.broadcast_object_list in bench.py) and carries the 128-byte RCCL id once.
    transport "host": every exchange is staged through host memory and `allgather(bytes) -> bytes`
    (ghip_dd_exchange_host) -- the rehearsal form for several ranks on one GPU."""

    def __init__(self, path, rank, nranks, bcast=None, transport="rccl", allgather=None):
        self.p, self.rank, self.nranks = path, int(rank), int(nranks)
        self.B = _bindings()
        self.transport, self.allgather = transport, allgather
        path.dd_init(rank, nranks)
        if transport == "rccl":
            uid = self.B.dd_rccl_unique_id() if rank == 0 else None
            uid = bcast(uid)
            path.dd_rccl_connect(uid)

    def _run(self, op, params, walk=0):
        if self.transport == "rccl":
            self.p.dd_run(op, params, walk)
        else:
            self.p.dd_run_host(op, params, self.allgather, walk)

    def timed(self, op, params, walk=0):
        """The operation phase by phase with the device drained in between (measurement only):
        returns ([compute ms per phase], [exchange ms per exchange])."""
        import time
        p = self.p
        p.dd_begin(op, params, walk)
        comp, exch = [], []
        cb = None
        if self.transport != "rccl":
            cb = p.allgather_callback(self.allgather)
        while True:
            p.sync()
            t0 = time.perf_counter()
            rc = p.dd_step()
            p.sync()
            comp.append(1e3 * (time.perf_counter() - t0))
            if rc == 0:
                break
            t0 = time.perf_counter()
            if cb is None:
                p.dd_exchange()
            else:
                p.dd_exchange_host(cb)
            p.sync()
            exch.append(1e3 * (time.perf_counter() - t0))
        if op == self.B.DD_MIGRATE:
            p.counts()
        return comp, exch

    def gravity(self, params, walk):
        self._run(self.B.DD_GRAVITY, params, walk)

    def density(self, params):
        self._run(self.B.DD_DENSITY, params)

    def hydro(self, params):
        self._run(self.B.DD_HYDRO, params)

    def migrate(self):
        self._run(self.B.DD_MIGRATE, None)

    def accept_guests(self, on=True):
        """ghip_dd_set_guests on this rank; the caller gives every rank the same setting"""
        self.p.dd_set_guests(on)

    def set_viscosity(self, params=None):
        """ghip_set_viscosity on this rank; the caller gives every rank the same setting"""
        self.p.set_viscosity(params)

    def set_dust_model(self, model=None):
        """ghip_set_dust_model on this rank; the caller gives every rank the same setting"""
        self.p.set_dust_model(model)

    def visc_set_alpha(self, alpha, dtalpha=None):
        """alpha (and Dtalpha or None) of this rank's own gas, before density()"""
        self.p.visc_set_alpha(alpha, dtalpha)

    def visc_get(self):
        return self.p.visc_get()

    def decompose(self, params=None):
        """GHIP_DD_DECOMPOSE(DecompParams; None = automatic level, unit weights, the cube kept), a collective:
        new key ranges (and on request a new cube) from the resident particles of all ranks -- this rank
        contributes one 128-byte block and one histogram, never its keys.  Moves nothing."""
        self._run(self.B.DD_DECOMPOSE, params if params is not None else self.B.DecompParams())

    def redistribute(self, params=None, rearrange=None, peano_order=False):
        """decompose, then migrate: afterwards every particle sits on the rank its key names.  With rearrange (a
        RearrangeParams, or True: both switches) this rank first runs ghip_rearrange, with peano_order it ends with
        ghip_peano_order in the domain in force (domain.c:120-135, 281-285); both are local.  Returns None with
        the defaults, else a dict as DomainShards.redistribute: results = [this rank's RearrangeResult], the
        totals summed over all ranks through the host all-gather of transport "host" (with "rccl" the caller's
        MPI adds them: the totals are then this rank's own and `local_totals` says so)."""
        if rearrange is None and not peano_order:
            self.decompose(params)
            self.migrate()
            return None
        res = _rearrange(self.p, rearrange) if rearrange is not None else None
        self.decompose(params)
        self.migrate()
        ordered = [self.p.peano_order()] if peano_order else None
        mine = _elim_counts(res) if res is not None else (0, 0, 0)
        counts, local = [mine], self.nranks > 1
        if res is not None and self.allgather is not None:
            got = _np.frombuffer(self.allgather(_np.array(mine, _np.int64).tobytes()), _np.int64)
            counts, local = [tuple(int(v) for v in row) for row in got.reshape(self.nranks, 3)], False
        out = _redistributed([res] if res is not None else None, counts if res is not None else [], ordered)
        out["local_totals"] = bool(local and res is not None)
        return out

    def pm_region(self, pmgrid):
        """GHIP_DD_PM_REGION, a collective: the region of the non-periodic mesh from the resident particles of
        all ranks (this rank contributes one 128-byte block), stored on every rank; returns it (PmRegion)"""
        import ctypes as C
        self._run(self.B.DD_PM_REGION, C.c_int(int(pmgrid)))
        return self.p.pm_get_region()

    def pm_nonperiodic(self, params):
        """GHIP_DD_PM_NONPERIODIC(PmnpParams), a collective: this rank's F_GRAVPM; GhipError with GHIP_EREGION
        on every rank when a particle of any rank left the region: pm_region(), then call again"""
        self._run(self.B.DD_PM_NONPERIODIC, params)

    def sync_point(self, ti_current, ti_nextoutput=-1):
        """GHIP_DD_DECOMPOSE in its SYNC_POINT_FORM, a collective: the next sync point of all ranks' particles (this rank contributes
        its 32 bin populations, 256 bytes, and one status record) and this rank's own active list
        (self.p.get_active()) -> SyncPoint"""
        self._run(self.B.DD_DECOMPOSE, self.B.SyncParams(int(ti_current), int(ti_nextoutput)), self.B.SYNC_POINT_FORM)
        return self.p.dd_get_sync_point()

    def potential(self, params):
        """GHIP_DD_POTENTIAL(PotParams), a collective: afterwards the path's get_potential() gives its own
        particles"""
        self._run(self.B.DD_POTENTIAL, params)

    def global_quantities(self, params, grav_kick_table=None, hydro_kick_table=None, old_photon_momentum=None,
                          potential=None):
        """GHIP_DD_GLOBAL_QUANTITIES(GlobalParams), a collective: the sums of the whole system (the same bytes
        on every rank) as a dict (GlobalSums.asdict)"""
        args, keep = self.B.dd_global_args(params, self.p.n, grav_kick_table, hydro_kick_table,
                                           old_photon_momentum, potential)
        self._run(self.B.DD_GLOBAL_QUANTITIES, args)
        return keep["out"].asdict()

    def fof(self, **params):
        """GHIP_DD_GLOBAL_QUANTITIES begun with walk = FOF_FORM, a collective (params: those of ForcePath.fof, the
        same on every rank): the FofResult of the whole system (the same bytes on every rank, with .counts);
        afterwards the path's fof_groups() / fof_maxdens_task() / fof_labels() / fof_ids() answer"""
        args, keep = self.B.dd_fof_args(**params)
        self._run(self.B.DD_GLOBAL_QUANTITIES, args, self.B.FOF_FORM)
        return _fof_result(self.p, keep)

    def wind_feedback(self, params, wind, state=None):
        """GHIP_DD_WIND in its WIND_FORM, a collective: the whole loop of momentum_feedback.c:283-568 for this rank's wind particles
        (local indices in list order; state: dict(stellar_age, birth_energy, old_momentum, new_density, drmin)).
        params.dt_total_floor is the GLOBAL floor.  Returns a dict as ForcePath.wind_feedback does: iterations is
        the global count, bits / ndeleted / deleted_momentum are this rank's own; counts: bindings.WIND_COUNTS"""
        args, keep = self.B.dd_wind_args(params, wind, state=state if len(wind) else _empty_wind_state())
        self._run(self.B.WIND_OP, args, self.B.WIND_FORM)
        return self.B.dd_wind_result(keep)

    def winds_feedback(self, params):
        """GHIP_DD_WIND in its WINDS_RESIDENT_FORM, a collective: ForcePath.winds_feedback for this rank's active
        Type-3 particles with a row in its wind table (dd_winds_set_table) -> a dict: iterations (global), this
        rank's bits / ndeleted / deleted_momentum, counts"""
        args, keep = self.B.dd_winds_args(params)
        self._run(self.B.WIND_OP, args, self.B.WINDS_RESIDENT_FORM)
        return self.B.dd_wind_result(keep)

    def wind_spawn(self, params, rnd):
        """GHIP_DD_WIND in its WINDS_SPAWN_FORM, a collective: ForcePath.wind_spawn for this rank's own sinks -> a
        dict as there, with tot_spawned, the sum over all ranks; the path's .n follows"""
        args, keep = self.B.dd_winds_args(spawn=params, rnd_table=rnd)
        self._run(self.B.WIND_OP, args, self.B.WINDS_SPAWN_FORM)
        self.p.counts()
        return self.B.dd_winds_spawn_report(keep)

    def sinks_density(self, params, ngb_factor):
        """GHIP_DD_SINK_DENSITY in its SINKS_RESIDENT_FORM, a collective: ForcePath.sinks_density for the active
        Type-5 particles of all ranks, this rank's found in its own sink table -> the iteration count"""
        args, keep = self.B.dd_sinks_args(dens=params, ngb_factor=ngb_factor)
        self._run(self.B.DD_SINK_DENSITY, args, self.B.SINKS_RESIDENT_FORM)
        return keep["iterations"].value

    def blackhole_accretion(self, bh_params, acc_params):
        """GHIP_DD_BH_SWALLOW in its SINKS_RESIDENT_FORM, a collective: blackhole_accretion() -> a dict as
        ForcePath.blackhole_accretion returns it, of this rank's own sinks and swallowed particles (the host adds
        the ranks' values, blackhole.c:659-661, 749-751)"""
        args, keep = self.B.dd_sinks_args(bh=bh_params, acc=acc_params)
        self._run(self.B.DD_BH_SWALLOW, args, self.B.SINKS_RESIDENT_FORM)
        return self.B.dd_sinks_report(keep)

    def wind_density(self, params, wind, dt_jump):
        """GHIP_DD_WIND in its WIND_DENSITY_FORM, a collective -> (new_density, drmin, counts) of this rank's list"""
        args, keep = self.B.dd_wind_args(params, wind, dt_jump=dt_jump)
        self._run(self.B.WIND_OP, args, self.B.WIND_DENSITY_FORM)
        return keep["new_density"], keep["drmin"], keep["counts"].copy()

    def wind_spread(self, params, wind, dt_jump, new_density, delta_momentum):
        """GHIP_DD_WIND in its WIND_SPREAD_FORM, a collective, into this rank's Injected_BH_Momentum -> counts"""
        args, keep = self.B.dd_wind_args(params, wind, dt_jump=dt_jump, new_density=new_density,
                                         delta_momentum=delta_momentum)
        self._run(self.B.WIND_OP, args, self.B.WIND_SPREAD_FORM)
        return keep["counts"].copy()
