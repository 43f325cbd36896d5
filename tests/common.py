"""Shared test plumbing: seeded problems, the oracle side and the device side of one step.

The oracle (oracle/) is imported here and ONLY in tests/, smoke() and bench.py's cpu_baseline.
"""
import importlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import oracle as O  # noqa: E402

pkg = importlib.import_module("gadget-leicester_amd")
ics = importlib.import_module("gadget-leicester_amd.ics")


def bindings():
    return importlib.import_module("gadget-leicester_amd.bindings")


class Problem:
    """A seeded particle set plus the run-time parameters of the BASELINE configs."""

    def __init__(self, ng=12, gas=True, periodic=True, seed=12345, clustered=True, soft_frac=0.04,
                 unequal=False, des_ngb=33.0, ic=None):
        self.ic = ic if ic is not None else ics.make_ics(ng, gas=gas, seed=seed,
                                                        clustered=clustered)
        ic = self.ic
        self.n = len(ic["pos"])
        self.ngas = int(ic["ngas"])
        self.periodic = int(periodic)
        self.box = float(ic["boxsize"])
        eps = soft_frac * ic["spacing"]
        table = np.full(6, eps)
        if unequal:
            table[0] = 0.5 * eps
            table[1] = 2.0 * eps
        self.unequal = int(unequal)
        self.force_soft = 2.8 * table          # All.ForceSoftening, gravtree.c:881
        self.min_gas_hsml = 0.0 * self.force_soft[0]
        self.ErrTolForceAcc = 0.005
        self.theta = 0.5
        self.des_ngb = des_ngb
        self.max_dev = 2.0
        self.visc = 0.8
        self.G = 1.0
        self.extent = O.domain_extent(ic["pos"])
        # SPH state: entropy from u (init.c:540-548 needs rho; use a flat entropy instead), first
        # smoothing-length guess from the mean inter-particle spacing
        ng_ = self.ngas
        self.hsml0 = np.zeros(self.n)
        if ng_:
            self.hsml0[:ng_] = 1.2 * (3.0 * des_ngb / (4 * np.pi * ng_)) ** (1.0 / 3.0) * self.box
        rng = np.random.default_rng(seed + 1)
        self.entropy = 0.05 * (1 + 0.2 * rng.random(ng_))
        self.dtentropy = 1e-3 * rng.standard_normal(ng_)
        self.timebin = rng.integers(1, 4, self.n).astype(np.int32)
        self.ti_begstep = np.zeros(self.n, np.int32)
        self.ti_current = 2
        self.timebase = 1e-3
        self.velpred = ic["vel"][:ng_] + 0.01 * rng.standard_normal((ng_, 3))

    # ---- parameter structs for both sides ----
    def o_grav(self, theta, kind="newton", rcut=0.0, asmth=0.0):
        return O.GravParams(theta, self.ErrTolForceAcc, self.box, self.periodic, self.unequal,
                            rcut, asmth)

    def o_dens(self):
        return O.DensParams(self.des_ngb, self.max_dev, self.min_gas_hsml, self.box,
                            self.periodic, self.ti_current, self.timebase, 150)

    def o_hydro(self, comoving=0, hubble_a2=1.0, fac_mu=1.0, fac_vsic_fix=1.0):
        return O.HydroParams(self.visc, self.box, self.periodic, comoving, hubble_a2, fac_mu,
                             fac_vsic_fix, self.timebase)

    def g_grav(self, theta, rcut=0.0, asmth=0.0):
        B = bindings()
        p = B.GravParams()
        p.ErrTolTheta = theta
        p.ErrTolForceAcc = self.ErrTolForceAcc
        for i in range(6):
            p.ForceSoftening[i] = self.force_soft[i]
        p.BoxSize = self.box
        p.periodic = self.periodic
        p.unequal_softenings = self.unequal
        p.Rcut = rcut
        p.Asmth = asmth
        return p

    def g_dens(self):
        B = bindings()
        return B.DensParams(self.des_ngb, self.max_dev, self.min_gas_hsml, self.box,
                            self.periodic, self.ti_current, self.timebase, 150)

    def g_hydro(self, comoving=0, hubble_a2=1.0, fac_mu=1.0, fac_vsic_fix=1.0):
        B = bindings()
        return B.HydroParams(self.visc, self.box, self.periodic, comoving, hubble_a2, fac_mu,
                             fac_vsic_fix, self.timebase, 0)

    # ---- oracle side ----
    def oracle_tree(self, hsml=None, toplevels=0):
        ic = self.ic
        return O.Tree(ic["pos"], ic["vel"], ic["mass"], ic["type"], self.force_soft,
                      hsml=(self.hsml0 if hsml is None else hsml), extent=self.extent,
                      toplevels=toplevels)

    # ---- device side ----
    def device(self, dev=0):
        return self.load(bindings().ForcePath(dev))

    def load(self, fp):
        """This problem into the context `fp`, which may have held another one: the counts and the fields a
        fresh context is given, nothing else -- OLDACC, GRAVPM, ID and the output fields stay as the problem
        before left them (a caller sets them where a fresh-context test would)."""
        B = bindings()
        ic = self.ic
        fp.set_counts(self.n, self.ngas)
        fp.set_field(B.F_POS, ic["pos"])
        fp.set_field(B.F_VEL, ic["vel"])
        fp.set_field(B.F_MASS, ic["mass"])
        fp.set_field(B.F_TYPE, ic["type"])
        fp.set_field(B.F_HSML, self.hsml0)
        fp.set_field(B.F_TIMEBIN, self.timebin)
        fp.set_field(B.F_TI_BEGSTEP, self.ti_begstep)
        if self.ngas:
            fp.set_field(B.F_VELPRED, self.velpred)
            fp.set_field(B.F_ENTROPY, self.entropy)
            fp.set_field(B.F_DTENTROPY, self.dtentropy)
        return fp

    def device_tree(self, fp):
        fp.tree_build(self.extent[0], self.extent[1], self.extent[2], self.force_soft)


def box_edge_particles(box, pmgrid, on_the_edge=True, n=64, seed=21):
    """Particles for the cell rule of the periodic mesh (pm_periodic.c:318-325) as an ics dict: for each axis one
    in the last cell (box (N - 0.5) / N: its +1 corner wraps), one at the origin, random interior ones, and, with
    on_the_edge, for each axis one whose coordinate there equals the box size (the clamp: last cell, offset 1) and
    one with all three.  Without on_the_edge the set is the same one less those four."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.05 * box, 0.95 * box, (n, 3))
    mass = rng.uniform(0.5, 1.5, n) / n
    for j in range(3):
        pos[j, j] = box
        pos[4 + j, j] = box * (pmgrid - 0.5) / pmgrid
    pos[3] = box
    pos[7] = 0.0
    keep = np.arange(n) if on_the_edge else np.r_[4:n]
    pos, mass = np.ascontiguousarray(pos[keep]), np.ascontiguousarray(mass[keep])
    k = len(keep)
    return dict(pos=pos, vel=np.zeros((k, 3)), mass=mass, type=np.ones(k, np.int32), ngas=0, boxsize=float(box),
                spacing=box / 4.0, id=np.arange(1, k + 1, dtype=np.uint32), u=np.zeros(0))


def sampled_hydro_check(pr, T, get_field, act, tol=1e-11, hparams=None):
    """hydro_force() of a big configuration against the oracle on the gas targets `act`: the oracle's
    hydro_evaluate for those targets on the DEVICE's density results of all gas particles (smoothing
    lengths, densities, pressures, f, div v, curl v -- themselves checked against the oracle's
    density() on the sample), after force_update_hmax() with the same values.  Checks HydroAccel,
    DtEntropy and MaxSignalVel of the sample; returns the oracle's pair count for them."""
    B = bindings()
    n, ng = pr.n, pr.ngas

    def gas(field):
        a = np.zeros(n)
        a[:ng] = get_field(field)[:ng]
        return a
    hs = np.asarray(get_field(B.F_HSML), np.float64).copy()
    dens, pres, dhf = gas(B.F_DENSITY), gas(B.F_PRESSURE), gas(B.F_DHSMLFAC)
    divv, curl = gas(B.F_DIVVEL), gas(B.F_CURLVEL)
    allgas = np.arange(ng, dtype=np.int32)
    T.update_hmax(allgas, hs, divv)
    oh = T.hydro(hparams if hparams is not None else pr.o_hydro(), act, pr.velpred, hs, dens, pres, dhf,
                 divv, curl, pr.timebin)
    ha = get_field(B.F_HYDROACCEL)
    scale = np.abs(oh["hydroaccel"][act]).max()
    assert np.abs(ha[act] - oh["hydroaccel"][act]).max() < tol * scale, "HydroAccel of the sample"
    de = get_field(B.F_DTENTROPY)
    assert np.abs(de[act] - oh["dtentropy"][act]).max() < tol * max(np.abs(oh["dtentropy"][act]).max(), 1e-300)
    ms = get_field(B.F_MAXSIGNALVEL)
    assert relerr(ms[act], oh["maxsignalvel"][act]) < tol, "MaxSignalVel of the sample"
    return oh["npairs"]


def relerr(a, b):
    """max_i |a_i - b_i| / |b_i| over vectors (rows)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    if a.ndim == 1:
        den = np.maximum(np.abs(b), 1e-300)
        return float(np.max(np.abs(a - b) / den)) if len(a) else 0.0
    den = np.maximum(np.linalg.norm(b, axis=1), 1e-300)
    return float(np.max(np.linalg.norm(a - b, axis=1) / den)) if len(a) else 0.0


class ShardSet:
    """A Problem cut into `nshards` Peano-Hilbert key ranges, each resident in a device context of
    its own (several logical shards on one GPU): the multi-GPU path as the parity tests drive it.
    Local particle order of a shard: its gas particles first (allvars.h:1384), global order kept."""

    def __init__(self, pr, nshards, work=None, dev=0, fields=None, domains=1, contexts=None):
        """contexts: `nshards` existing contexts (of an earlier ShardSet) to load instead of new ones: they are
        given the counts, the fields, the domain and the splits or segments of this problem, as a decomposition
        of a running code reloads its shards; whatever else they hold stays."""
        B = bindings()
        sh = importlib.import_module("gadget-leicester_amd.sharded")
        self.pr, self.P, self.B = pr, nshards, B
        assert contexts is None or len(contexts) == nshards
        ic = pr.ic
        # keys from the device (ghip_dd_keys), checked against the oracle's table-driven curve
        probe = B.ForcePath(dev)
        probe.set_counts(pr.n, 0)
        probe.set_field(B.F_POS, ic["pos"])
        probe.dd_init(0, 1)
        probe.dd_set_domain(pr.extent[0], pr.extent[1], pr.extent[2], pr.force_soft)
        self.keys = probe.dd_keys()
        probe.close()
        fac = (1 << 21) / pr.extent[2]
        ip = ((ic["pos"] - pr.extent[0]) * fac).astype(np.int64)
        sample = np.arange(0, pr.n, max(1, pr.n // 512))
        want = np.array([O.peano_hilbert_key(*ip[i]) for i in sample], dtype=np.uint64)
        assert np.array_equal(self.keys[sample], want), "device Peano-Hilbert keys differ"
        self.segments = None
        if domains > 1:
            # -DMULTIPLEDOMAINS=domains (the shipped Makefile: 16): the curve is cut into
            # nshards * domains pieces and every shard owns `domains` of them -- here dealt out in
            # turn, so that no two neighbouring pieces share an owner (domain.c:1158-1215 assigns them
            # by load; any assignment is a valid decomposition)
            pieces, piece_of = sh.decompose(self.keys, nshards * domains, work)
            seg_owner = (np.arange(nshards * domains) * 7 + 3) % nshards if nshards % 7 else \
                np.arange(nshards * domains) % nshards
            seg_owner = seg_owner.astype(np.int32)
            self.segments = (pieces, seg_owner)
            self.splits = None
            self.owner = seg_owner[piece_of].astype(np.int32)
        else:
            self.splits, self.owner = sh.decompose(self.keys, nshards, work)
        self.gid, self.ngas, self.fp = [], [], []
        extra = fields or {}
        for r in range(nshards):
            mine = np.where(self.owner == r)[0]
            g = np.concatenate([mine[mine < pr.ngas], mine[mine >= pr.ngas]]).astype(np.int64)
            ngl = int((mine < pr.ngas).sum())
            self.gid.append(g)
            self.ngas.append(ngl)
            fp = B.ForcePath(dev) if contexts is None else contexts[r]
            fp.set_counts(len(g), ngl)
            if len(g):
                fp.set_field(B.F_POS, ic["pos"][g])
                fp.set_field(B.F_VEL, ic["vel"][g])
                fp.set_field(B.F_MASS, ic["mass"][g])
                fp.set_field(B.F_TYPE, ic["type"][g])
                fp.set_field(B.F_HSML, extra.get("hsml", pr.hsml0)[g])
                fp.set_field(B.F_TIMEBIN, pr.timebin[g])
                fp.set_field(B.F_TI_BEGSTEP, pr.ti_begstep[g])
                fp.set_field(B.F_OLDACC, extra.get("oldacc", np.zeros(pr.n))[g])
                fp.set_field(B.F_ID, g.astype(np.int32))      # global index, follows the particle
            if ngl:
                gg = g[:ngl]
                fp.set_field(B.F_VELPRED, pr.velpred[gg])
                fp.set_field(B.F_ENTROPY, pr.entropy[gg])
                fp.set_field(B.F_DTENTROPY, pr.dtentropy[gg])
            if contexts is None:
                fp.dd_init(r, nshards)
            fp.dd_set_domain(pr.extent[0], pr.extent[1], pr.extent[2], pr.force_soft)
            if self.segments is not None:
                fp.dd_set_segments(*self.segments)
            else:
                fp.dd_set_splits(self.splits)
            self.fp.append(fp)
        self.run = sh.DomainShards(self.fp)

    def set_field(self, field, glob):
        gas = self.B._FIELD_INFO[field][0]
        for r, fp in enumerate(self.fp):
            g = self.gid[r][:self.ngas[r]] if gas else self.gid[r]
            if len(g):
                fp.set_field(field, np.asarray(glob)[g])

    def get_field(self, field):
        B = self.B
        gas, ncomp, isint = B._FIELD_INFO[field]
        nglob = self.pr.ngas if gas else self.pr.n
        shape = (nglob, 3) if ncomp == 3 else (nglob,)
        out = np.zeros(shape, np.int32 if isint else np.float64)
        for r, fp in enumerate(self.fp):
            g = self.gid[r][:self.ngas[r]] if gas else self.gid[r]
            if len(g):
                out[g] = fp.get_field(field)
        return out

    def migrate(self):
        """GHIP_DD_MIGRATE on all shards, then re-read who holds what from the ID field"""
        self.run.run(self.B.DD_MIGRATE, None)
        for r, fp in enumerate(self.fp):
            n, ngl = fp.counts()
            self.gid[r] = fp.get_field(self.B.F_ID).astype(np.int64) if n else np.zeros(0, np.int64)
            self.ngas[r] = ngl
            self.owner[self.gid[r]] = r

    def each(self, fn):
        return [fn(fp) for fp in self.fp]

    def locate(self, glob):
        """per shard: (local indices of the particles `glob` it holds, their positions in `glob`)"""
        glob = np.asarray(glob, np.int64)
        shard = np.full(self.pr.n, -1, np.int32)
        local = np.zeros(self.pr.n, np.int32)
        for r, g in enumerate(self.gid):
            shard[g] = r
            local[g] = np.arange(len(g), dtype=np.int32)
        out = []
        for r in range(self.P):
            pos = np.where(shard[glob] == r)[0]
            out.append((local[glob[pos]].astype(np.int32), pos.astype(np.int64)))
        return out

    def close(self):
        for fp in self.fp:
            fp.close()


def failing_collective(paths, op, params, walk=0):
    """`op` on all shards of this process, expected to fail: the GhipError of every shard, in shard order.
    All shards must fail in the same step (no shard is left inside the collective), and the failed step ends
    the operation on every one of them: a further ghip_dd_step finds no operation in progress."""
    import pytest
    B = bindings()
    prm = params if isinstance(params, (list, tuple)) else [params] * len(paths)
    for fp, q in zip(paths, prm):
        fp.dd_begin(op, q, walk)
    while True:
        rcs, errs = [], []
        for fp in paths:
            try:
                rcs.append(fp.dd_step())
            except B.GhipError as e:
                errs.append(e)
        if errs:
            break
        assert rcs == [1] * len(paths), "the operation did not fail: %r" % (rcs,)
        B.dd_exchange_local(paths)
    assert len(errs) == len(paths), "%d of %d shards failed, the others returned %r" % (len(errs), len(paths), rcs)
    for fp in paths:
        with pytest.raises(B.GhipError) as e:
            fp.dd_step()
        assert "no operation in progress" in str(e.value)
    return errs


class SinkProblem:
    """A Problem with a few Type-5 sinks and Type-2 dust grains (config c5's ingredients): some DM
    particles are re-typed, one sink is the heavy central object.  Parameters of the shipped flag
    bundle's sink passes (blackhole.c) in code units.  box: the same problem in a box of that size
    (scale_cases.rescale_problem): every length here is a multiple of the spacing, every mass one of a
    particle's, so they follow."""

    def __init__(self, ng=8, periodic=1, nsink=6, ndust=200, seed=5, box=1.0):
        pr = Problem(ng=ng, gas=True, periodic=periodic)
        if box != 1.0:
            from scale_cases import rescale_problem
            pr = rescale_problem(pr, box)
        self.pr = pr
        rng = np.random.default_rng(seed)
        n, ngas = pr.n, pr.ngas
        dm = np.arange(ngas, n)
        pick = rng.choice(dm, nsink + ndust, replace=False)
        self.sinks = np.sort(pick[:nsink]).astype(np.int32)
        self.dust = np.sort(pick[nsink:])
        typ = pr.ic["type"].copy()
        typ[self.sinks] = 5
        typ[self.dust] = 2
        pr.ic["type"] = typ
        mass = pr.ic["mass"].copy()
        mass[self.sinks] = 40.0 * mass[ngas]           # heavier than anything around
        mass[self.sinks[0]] = 400.0 * mass[ngas]       # the central object
        pr.ic["mass"] = mass
        pr.ic["vel"] = 0.05 * pr.ic["vel"]             # slow: some neighbours are bound
        pr.velpred = pr.ic["vel"][:ngas] + 0.0
        self.ids = (np.arange(n, dtype=np.uint32) * 7 + 11).astype(np.uint32)   # unique, unordered
        self.hsml = pr.hsml0.copy()
        self.hsml[self.sinks] = 2.6 * pr.ic["spacing"]
        self.bh_mass = np.zeros(n)
        self.bh_mass[self.sinks] = 0.5 * mass[self.sinks]
        self.mdot = 1.0e-3 * (1 + rng.random(nsink))
        self.SMBHmass = mass[self.sinks[0]]
        sp = pr.ic["spacing"]
        self.par = dict(BoxSize=pr.box, periodic=periodic, ascale=1.0, dt_fac=pr.timebase,
                        SMBHmass=self.SMBHmass, InnerBoundary=2.0 * sp, SinkBoundary=1.5 * sp,
                        SofteningBndry=2.4 * sp, CritDensity=0.0, FeedbackCoeff=3.0e-9,
                        UnitMass_in_g=1.989e33, dust=1, accretion_of_dust_only=1,
                        accretion_density=1)

    def params(self, cls, **over):
        p = cls()
        for k, v in {**self.par, **over}.items():
            setattr(p, k, v)
        return p


# ------------------------------------------------------------------------------------------------
# Inputs of the sink tests (tests/test_sink_cpu.py, tests/test_gpu_sink.py) on top of SinkProblem:
# contested victims, chains of claims, mutual claims, the central object's boundaries and the branches
# of the sinks' h iteration.  All of them are checked against tests/sink_ref.py (all pairs, written
# from blackhole.c and density.c), whose density pass rides along as `sp.dens`.
# ------------------------------------------------------------------------------------------------
SINK_SWITCHES = [(1, 1), (0, 1), (0, 0)]       # (accretion_of_dust_only, accretion_density)
SINK_CRIT_DENSITY = 1.0
SINK_TRIES = 20


def sink_over(dust_only, acc_density):
    return dict(accretion_of_dust_only=dust_only, accretion_density=acc_density, CritDensity=SINK_CRIT_DENSITY)


def sink_ref_par(sp, **over):
    """the parameters of the passes for tests/sink_ref.py: any object with the members of ghip_bh_params"""
    import types
    return types.SimpleNamespace(**{**sp.par, **over})


def sink_ref_density(sp):
    import sink_ref
    pr = sp.pr
    return sink_ref.sink_density(pr.ic["pos"], pr.ic["mass"], pr.ic["type"], pr.velpred, pr.entropy, sp.sinks,
                                 sp.hsml, pr.des_ngb, 1.5, pr.max_dev, pr.min_gas_hsml, pr.box, pr.periodic)


def _sink_dist(sp, i):
    pr = sp.pr
    d = pr.ic["pos"][i][None, :] - pr.ic["pos"]
    if pr.periodic:
        d -= pr.box * np.round(d / pr.box)
    return np.sqrt((d * d).sum(axis=1))


def sink_ties(sp, dens, rel=1e-9):
    """How many candidates lie within `rel` (relative) of a threshold at which a sink pass decides: r against
    every h the iteration tried (gas), r against the final h and the three boundaries, e_tot against 0 (all
    candidates of the marking pass), the gas density against CritDensity.  Mass and ID comparisons are exact by
    construction.  An input with such a tie could be decided either way by a correctly rounded variant of the
    same arithmetic, so the generators below reject it."""
    pr = sp.pr
    typ, mass, vel = pr.ic["type"], pr.ic["mass"], pr.ic["vel"]
    ties = int((np.abs(sp.gas_density - SINK_CRIT_DENSITY) <= rel * SINK_CRIT_DENSITY).sum())
    for a, i in enumerate(sp.sinks):
        r = _sink_dist(sp, i)
        for h in dens["h_tried"][a]:
            ties += int((np.abs(r[typ == 0] - h) <= rel * h).sum())
        h = dens["hsml"][i]
        cand = ((typ == 0) | (typ == 2) | (typ == 5)) & (r < 1.001 * h) & (r > 0)
        for b in (h, sp.par["InnerBoundary"], sp.par["SinkBoundary"], sp.par["SofteningBndry"]):
            ties += int((np.abs(r[cand] - b) <= rel * b).sum())
        kin = 0.5 * ((vel[cand] - vel[i]) ** 2).sum(axis=1)
        pot = mass[i] / r[cand]
        ties += int((np.abs(kin - pot) <= rel * (kin + pot)).sum()) if mass[i] > 0 else 0
    return ties


def _dm_mass(pr):
    return float(pr.ic["mass"][pr.ic["type"] == 1][0])


def _unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def _finish(sp):
    pr = sp.pr
    sp.bh_mass = np.zeros(pr.n)
    sp.bh_mass[sp.sinks] = 0.5 * pr.ic["mass"][sp.sinks]
    pr.extent = O.domain_extent(pr.ic["pos"])
    return sp


def _sink_clump(periodic, seed):
    """12 sinks: sink 0 the central object where SinkProblem put it; sinks 1-11 inside a cube of 1.2 spacings
    at the corner of the box (periodic search spheres wrap), so that every one of them lies inside
    SofteningBndry (2.4 spacings > the cube's diagonal) of every other: each claims all that are not heavier.
    Masses 40, 40, 44 ... 72 DM masses and one 0, in a seeded order; IDs a seeded permutation (not monotone in
    list order: "largest ID", "last claim" and "first claim" differ); every third grain 200 times faster
    (unbound: refused); one sink in time bin 0 (no feedback)."""
    sp = SinkProblem(ng=10, periodic=periodic, nsink=12, ndust=300, seed=seed)
    pr = sp.pr
    rng = np.random.default_rng(1000 + seed)
    s, dm = pr.ic["spacing"], _dm_mass(pr)
    cl = sp.sinks[1:]
    pr.ic["pos"][cl] = 0.1 * s + 1.2 * s * rng.random((11, 3))
    pr.ic["mass"][cl] = dm * rng.permutation(np.array([40., 40., 44., 48., 52., 56., 60., 64., 68., 72., 0.]))
    sp.ids = rng.permutation(sp.ids)
    # 40 of the 300 grains around the clump, so that grains are contested under every switch setting and
    # fast ones come inside a boundary whether or not the box wraps
    pr.ic["pos"][sp.dust[:40]] = 0.05 * s + 2.45 * s * rng.random((40, 3))
    pr.ic["vel"][sp.dust[::3]] *= 200.0
    pr.timebin[cl[3]] = 0
    return _finish(sp)


def _sink_pair(periodic, seed, at=None):
    """two isolated sinks of equal mass, neither the central object, 1 spacing apart: inside SofteningBndry of
    each other, `Mass <= mass` holds both ways -- each claims the other, and (blackhole.c:528-532) neither
    swallows anything.  at: where the first of them goes (in box lengths; default: where SinkProblem put it)"""
    sp = SinkProblem(ng=10, periodic=periodic, nsink=2, ndust=300, seed=seed)
    pr = sp.pr
    rng = np.random.default_rng(2000 + seed)
    s, dm = pr.ic["spacing"], _dm_mass(pr)
    if at is not None:
        pr.ic["pos"][sp.sinks[0]] = pr.box * np.asarray(at, np.float64)
    pr.ic["mass"][sp.sinks] = 40.0 * dm
    sp.SMBHmass = sp.par["SMBHmass"] = 400.0 * dm
    pr.ic["pos"][sp.sinks[1]] = np.mod(pr.ic["pos"][sp.sinks[0]] + 1.0 * s * _unit(rng), pr.box)
    return _finish(sp)


def _sink_central(periodic, seed):
    """the central object with two light sinks: one at 1 spacing (inside InnerBoundary = 2: merged) and one at
    2.1 spacings (outside InnerBoundary, inside SofteningBndry = 2.4: the central object must leave it alone,
    any other sink would take it)"""
    sp = SinkProblem(ng=10, periodic=periodic, nsink=3, ndust=300, seed=seed)
    pr = sp.pr
    rng = np.random.default_rng(3000 + seed)
    s, dm = pr.ic["spacing"], _dm_mass(pr)
    c = sp.sinks[0]
    pr.ic["mass"][sp.sinks[1:]] = dm * np.array([40.0, 44.0])
    pr.ic["pos"][sp.sinks[1]] = np.mod(pr.ic["pos"][c] + 1.0 * s * _unit(rng), pr.box)
    pr.ic["pos"][sp.sinks[2]] = np.mod(pr.ic["pos"][c] + 2.1 * s * _unit(rng), pr.box)
    sp.ids = rng.permutation(sp.ids)
    return _finish(sp)


SINK_HITER = ("tight", "minh", "clamp", "small", "large", "void")


def _sink_hiter(variant):
    """the stock problem with the sinks' h iteration (density.c:559-652) sent down its other branches:
    tight   MaxNumNgbDeviation = 1e-9: bisection until (Right - Left) < 1e-3 Left ends it
    minh    MinGasHsml = the median converged h: a sink with too many neighbours at h <= 1.01 MinGasHsml is accepted
    clamp   MinGasHsml = 1.05 x the median converged h: the step h / 1.26 lands below it and is reset to it
    small   first h x 0.2: growth by 1.26, then bisection
    large   first h x 3: shrinking by 1.26, then bisection
    void    one sink where the gas is thinnest, with no gas inside its first h (rho = 0 in that pass)"""
    def build(periodic, seed):
        sp = SinkProblem(ng=10, periodic=periodic, nsink=8, seed=seed)
        pr = sp.pr
        if variant == "tight":
            pr.max_dev = 1e-9
        elif variant in ("minh", "clamp"):
            pr.min_gas_hsml = (1.0 if variant == "minh" else 1.05) * \
                float(np.median(sink_ref_density(sp)["hsml"][sp.sinks]))
        elif variant == "small":
            sp.hsml[sp.sinks] *= 0.2
        elif variant == "large":
            sp.hsml[sp.sinks] *= 3.0
        elif variant == "void":
            rng = np.random.default_rng(4000 + seed)
            pts = rng.random((4000, 3)) * pr.box
            gas = pr.ic["pos"][:pr.ngas]
            d = pts[:, None, :] - gas[None, :, :]
            d -= pr.box * np.round(d / pr.box)
            dmin = np.sqrt((d * d).sum(axis=2)).min(axis=1)
            k = int(np.argmax(dmin))
            pr.ic["pos"][sp.sinks[3]] = pts[k]
            sp.hsml[sp.sinks[3]] = 0.8 * dmin[k]
        else:
            raise ValueError(variant)
        return _finish(sp)
    return build


_SINK_BUILDERS = dict(clump=_sink_clump, pair=_sink_pair, central=_sink_central,
                      **{"hiter-" + v: _sink_hiter(v) for v in SINK_HITER})
_SINK_CACHE = {}


def sink_case(name, periodic=1, seed0=5, **how):
    """The input `name` ("clump", "pair", "central", "hiter-<variant>") from the first of the seeds seed0,
    seed0 + 1, ... that has no candidate within 1e-9 of a decision threshold (sink_ties); fails loudly after
    SINK_TRIES seeds.  `how`: further arguments of the input's builder.  sp.seed is the seed taken, sp.gas_density the gas densities the marking pass reads,
    sp.dens the density pass of tests/sink_ref.py.  A fresh copy per call: the passes change masses."""
    import copy
    key = (name, periodic, seed0, repr(sorted(how.items())))
    if key not in _SINK_CACHE:
        for seed in range(seed0, seed0 + SINK_TRIES):
            sp = _SINK_BUILDERS[name](periodic, seed, **how)
            sp.case, sp.seed = name, seed
            sp.gas_density = 0.5 + np.random.default_rng(3).random(sp.pr.ngas)
            sp.dens = sink_ref_density(sp)
            assert sp.dens["iterations"] >= 0, "%s: the reference's h iteration did not converge" % name
            if sink_ties(sp, sp.dens) == 0:
                _SINK_CACHE[key] = sp
                break
        else:
            raise AssertionError("sink_case(%r): %d seeds from %d on all have a candidate within 1e-9 of a "
                                 "decision threshold" % (name, SINK_TRIES, seed0))
    return copy.deepcopy(_SINK_CACHE[key])


_SINK_REF_CACHE = {}


def sink_reference(name, periodic, dust_only, acc_density, **how):
    """tests/sink_ref.py on the input `name` under one switch setting, computed once and shared (nobody
    changes it): dict(par, over, sw, inj -- the marks under the project's rule; last, first -- the marks under
    the two other rules; claims; swallow -- the swallow pass on `sw`)."""
    import sink_ref
    key = (name, periodic, dust_only, acc_density, repr(sorted(how.items())))
    if key not in _SINK_REF_CACHE:
        sp = sink_case(name, periodic, **how)
        ic, pr, d = sp.pr.ic, sp.pr, sp.dens
        over = sink_over(dust_only, acc_density)
        par = sink_ref_par(sp, **over)
        a = (ic["pos"], ic["vel"], ic["mass"], ic["type"], sp.ids, sp.sinks, d["hsml"])
        ev = {rule: sink_ref.evaluate(*a, pr.timebin, sp.mdot, d["density"], sp.gas_density, par, rule=rule)
              for rule in ("max", "last", "first")}
        _SINK_REF_CACHE[key] = dict(
            par=par, over=over, sw=ev["max"][0], inj=ev["max"][1], last=ev["last"][0], first=ev["first"][0],
            claims=sink_ref.claims(ic["pos"], ic["vel"], ic["mass"], ic["type"], sp.sinks, d["hsml"],
                                   sp.gas_density, par),
            swallow=sink_ref.swallow(*a, ev["max"][0], sp.bh_mass, par))
    return _SINK_REF_CACHE[key]


def check_sink_passes(sp, ref, dens=None, marks=None, swallowed=None, mass=None):
    """One side's results (the oracle's or the device's) of the three passes on the input `sp` against
    tests/sink_ref.py (`ref` = sink_reference(...)), with the tolerances of test_sink_passes_parity:
    marks, counts, iteration counts and masses exact, sums to summation order.  dens: dict(hsml, numngb,
    density, entropy, gasvel [nsink], iterations); marks: (SwallowID [n], injected [ngas]); swallowed:
    dict(counts, acc_mass, acc_bhmass, acc_dustmass, acc_momentum, bh_mass [nsink]); mass [n]: the masses after
    the swallow pass.  Returns the measured errors (the caller prints them).

    Measured worst cases over all inputs (MI355X, one device and 3 / 8 shards; the oracle's are of the same
    size): hsml 0, numngb 1.4e-14 absolute, density 2.7e-16, entropy 3.9e-16, gasvel 3.6e-16, injected energy
    3.9e-16 of the largest, accreted mass 2.7e-17, accreted momentum 1.9e-16, total mass 1.6e-16 -- the order
    of at most 12 atomic adds per particle and of the wave reductions, three to four decades inside the bounds."""
    pr, rd, sk = sp.pr, sp.dens, sp.sinks
    err = {}
    if dens is not None:
        assert dens["iterations"] == rd["iterations"] >= 1
        err["hsml"] = relerr(dens["hsml"], rd["hsml"][sk])
        err["numngb"] = float(np.abs(dens["numngb"] - rd["numngb"]).max())
        err["density"], err["entropy"] = relerr(dens["density"], rd["density"]), relerr(dens["entropy"], rd["entropy"])
        err["gasvel"] = float(np.abs(dens["gasvel"] - rd["gasvel"]).max() / np.abs(rd["gasvel"]).max())
        assert err["hsml"] < 1e-13 and err["numngb"] < 1e-10, err
        assert err["density"] < 1e-12 and err["entropy"] < 1e-12 and err["gasvel"] < 1e-12, err
    if marks is not None:
        sw, inj = marks
        assert np.array_equal(sw, ref["sw"]), "SwallowID differs at %s" % np.where(sw != ref["sw"])[0][:10]
        top = np.abs(ref["inj"]).max()
        assert top > 0
        err["injected"] = float(np.abs(inj - ref["inj"]).max() / top)
        assert err["injected"] <= 1e-12, err
    if swallowed is not None:
        rs = ref["swallow"]
        assert np.array_equal(swallowed["counts"], rs["counts"]), (swallowed["counts"], rs["counts"])
        for k in ("acc_mass", "acc_bhmass", "acc_dustmass", "acc_momentum"):
            top = max(np.abs(rs[k]).max(), 1e-300)
            err[k] = float(np.abs(swallowed[k] - rs[k]).max() / top)
            assert err[k] <= 1e-13, (k, err)
            # a sink that was itself claimed is passed over (blackhole.c:528-532): zero sums, exactly
            assert not np.any(np.asarray(swallowed[k])[rs["skipped"]]), k
        # BH_Mass of a sink is zeroed only if it really was swallowed (:1276), not if it was merely marked
        assert np.array_equal(swallowed["bh_mass"], rs["bh_mass"][sk])
        assert np.array_equal(swallowed["bh_mass"] == 0, rs["swallowed"][sk] | (sp.bh_mass[sk] == 0))
    if mass is not None:
        rs = ref["swallow"]
        assert np.array_equal(mass, rs["mass"]), "masses differ at %s" % np.where(mass != rs["mass"])[0][:10]
        if swallowed is not None:
            before = pr.ic["mass"].sum()
            err["total_mass"] = float(abs(swallowed["acc_mass"].sum() + mass.sum() - before) / before)
            assert err["total_mass"] < 1e-14, err
    return err


# every input under the settings it is run with: (name, periodic, (accretion_of_dust_only, accretion_density))
SINK_CASES = [("clump", p, s) for p in (0, 1) for s in SINK_SWITCHES] + \
             [("pair", 1, s) for s in SINK_SWITCHES] + [("central", 1, s) for s in SINK_SWITCHES] + \
             [("hiter-" + v, 1, (0, 0)) for v in SINK_HITER]
# where the pair goes in the tests on shards: cut into 3 and into 8 key ranges, each of the two sinks has
# victims of its own on other shards than itself (asserted there)
SINK_PAIR_AT = (0.72, 0.53, 0.31)


def oracle_sink_passes(sp, over):
    """the three passes on the oracle's tree -> (dens, marks, swallowed, mass) as check_sink_passes takes them"""
    pr = sp.pr
    ic = pr.ic
    T = O.Tree(ic["pos"], ic["vel"], ic["mass"].copy(), ic["type"], pr.force_soft, hsml=sp.hsml,
               extent=pr.extent)
    od = O.sink_density(T, pr.o_dens(), 1.5, sp.sinks, pr.velpred, pr.entropy, sp.hsml)
    hs = od["hsml"]
    op = sp.params(O.BhParams, **over)
    sw, inj = O.blackhole_evaluate(T, op, sp.sinks, sp.ids, hs, pr.timebin, sp.mdot, od["density"],
                                   sp.gas_density, np.zeros(pr.n, np.uint32), np.zeros(pr.ngas))
    oo = O.blackhole_swallow(T, op, sp.sinks, sp.ids, hs, sw, sp.bh_mass, unclaimed_only=True)
    oo["bh_mass"] = oo["bh_mass"][sp.sinks]
    od["hsml"] = hs[sp.sinks]
    return od, (sw, inj), oo, T.mass
