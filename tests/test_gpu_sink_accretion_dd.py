"""The sinks on the resident state of shards: the sink table on every shard, its rows travelling with
GHIP_DD_MIGRATE, and ghip_sinks_density / ghip_blackhole_accretion as the collectives GHIP_DD_SINK_DENSITY /
GHIP_DD_BH_SWALLOW begun with walk = GHIP_SINKS_RESIDENT_FORM.

Against the per-pass forms (walk = 0) of the same operations, driven with host arrays and with the Mdot step and
the finish of tests/sink_accretion_ref.py on the host: the same kernels on the same inputs, the partial sums added
in the same rank order, the new arithmetic compiled without contraction -- everything is compared bit for bit,
with the one exception tests/test_gpu_sink_accretion.py derives (Injected_BH_Energy of a gas particle with three
or more feeders).  The per-pass GHIP_DD_SINK_DENSITY does not return its iteration count: the count of the
resident form is compared with the single-GPU ghip_sinks_density's (test_against_one_gpu), and here HSML, which
the iteration decides, is compared bit for bit.

Against one GPU: marks, victims, counts and iteration counts exactly; sums to 1e-13 of the field's largest value
(the rank-ordered partial sums associate differently), the bound of test_sink_passes_on_shards."""
import numpy as np
import pytest

import sfr_ref
import sink_accretion_cases as AC
import sink_accretion_ref as AR
from common import (O, SINK_PAIR_AT, SINK_SWITCHES, ShardSet, bindings, failing_collective, sink_case, sink_over)

pytestmark = pytest.mark.gpu
EINVAL = -90002
NGB = AC.NGB_FACTOR


def _gacc(B, acc):
    p = B.BhAccretionParams()
    for k, _ in p._fields_:
        setattr(p, k, getattr(acc, k))
    return p


def _state_of(B, rows):
    return dict(bh_mass=rows[:, B.SK_BH_MASS].copy(), accdisc=rows[:, B.SK_ACCDISC_MASS].copy(),
                mdot=rows[:, B.SK_BH_MDOT].copy(), dust_mass=rows[:, B.SK_DUST_MASS].copy(),
                total_mass=rows[:, B.SK_TOTAL_MASS].copy())


class Run:
    """A ShardSet of a sink problem whose P[].ID is sp.ids (the table's key), the gas densities the marking pass
    reads in place after the trees are built.  rows: the sinks' rows in the order of sp.sinks -> every shard gets
    the table of the sinks it holds; None: no table (the per-pass side keeps a host mirror instead)."""

    def __init__(self, sp, nshards, rows=None, contexts=None):
        self.B = B = bindings()
        self.sp, self.pr = sp, sp.pr
        self.S = S = ShardSet(sp.pr, nshards, fields=dict(hsml=sp.hsml), contexts=contexts)
        order = np.argsort(sp.ids)
        self._sorted_ids, self._order = sp.ids[order], order
        for r, fp in enumerate(S.fp):
            if len(S.gid[r]):
                fp.set_field(B.F_ID, np.ascontiguousarray(sp.ids[S.gid[r]]).view(np.int32))
        if rows is not None:
            assert np.all(np.diff(sp.sinks) > 0)
            for r, fp in enumerate(S.fp):
                g = S.gid[r]
                mine = np.searchsorted(sp.sinks, g[np.isin(g, sp.sinks)])
                fp.sinks_set_table(sp.ids[sp.sinks][mine], rows[mine].reshape(len(mine), B.SK_COUNT))

    def glob_of(self, ids):
        ids = np.asarray(ids).view(np.uint32) if np.asarray(ids).dtype == np.int32 else np.asarray(ids, np.uint32)
        k = np.searchsorted(self._sorted_ids, ids)
        assert np.array_equal(self._sorted_ids[k], ids)
        return self._order[k].astype(np.int64)

    def refresh(self):
        """who holds what, from the ID field (after a migration, a rearrangement or a reordering)"""
        S, B = self.S, self.B
        for r, fp in enumerate(S.fp):
            n, ngl = fp.counts()
            S.gid[r] = self.glob_of(fp.get_field(B.F_ID)) if n else np.zeros(0, np.int64)
            S.ngas[r] = ngl
            S.owner[S.gid[r]] = r

    def trees(self):
        S, B, pr = self.S, self.B, self.pr
        S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
        S.run.density(pr.g_dens())
        S.set_field(B.F_DENSITY, self.sp.gas_density)

    def sinks_on(self, r):
        """(local indices ascending = active-list order, global indices) of the Type-5 particles of shard r"""
        fp = self.S.fp[r]
        if fp.counts()[0] == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int64)
        loc = np.where(fp.get_field(self.B.F_TYPE) == 5)[0]
        return loc.astype(np.int32), self.S.gid[r][loc]

    def close(self):
        self.S.close()


def _op(S, op, make):
    built = [make(r) for r in range(S.P)]
    S.run.run(op, [b[0] for b in built])
    return [b[1] for b in built]


def per_pass_step(run, mirror, gd, gp, par, acc):
    """blackhole_accretion() on shards as a host drives it without the resident forms: the three walk = 0
    operations with host arrays, the Mdot step and the finish on the host, the rows kept in `mirror` [n][SK_COUNT]
    by global particle index (updated in place).  Returns the per-shard reports."""
    B, S, sp = run.B, run.S, run.sp
    on = [run.sinks_on(r) for r in range(S.P)]
    ids = [np.ascontiguousarray(sp.ids[g]) for _, g in on]
    fld = [dict(h=fp.get_field(B.F_HSML), tb=fp.get_field(B.F_TIMEBIN), m=fp.get_field(B.F_MASS))
           if fp.n else dict(h=np.zeros(0), tb=np.zeros(0, np.int32), m=np.zeros(0)) for fp in S.fp]
    dens = _op(S, B.DD_SINK_DENSITY, lambda r: B.dd_sink_args(on[r][0], dens=gd, ngb_factor=NGB,
                                                              hsml=fld[r]["h"][on[r][0]]))
    st = [AR.mdot_step(_state_of(B, mirror[on[r][1]]), fld[r]["m"][on[r][0]], fld[r]["tb"][on[r][0]], par.dt_fac,
                       acc)[0] for r in range(S.P)]
    S.each(lambda fp: fp.sink_reset())
    _op(S, B.DD_BH_EVALUATE, lambda r: B.dd_sink_args(on[r][0], sink_ids=ids[r], bh=gp, mdot=st[r]["mdot"],
                                                      bh_density=dens[r]["density"]))
    go = _op(S, B.DD_BH_SWALLOW, lambda r: B.dd_sink_args(on[r][0], sink_ids=ids[r], bh=gp,
                                                         sink_bh_mass=st[r]["bh_mass"]))
    reps = []
    for r, fp in enumerate(S.fp):
        loc, glob = on[r]
        a, s = go[r], st[r]
        s["bh_mass"] = a["bh_mass"]
        if fp.n == 0:
            reps.append(dict(bin_mass=np.zeros(32), bin_dynmass=np.zeros(32), bin_mdot=np.zeros(32),
                             counts=a["counts"].copy(), nactive=0))
            continue
        vel, mass = fp.get_field(B.F_VEL), fp.get_field(B.F_MASS)
        s, v5, m5, rep, _ = AR.finish(s, vel[loc], mass[loc], fld[r]["tb"][loc], a["acc_mass"], a["acc_bhmass"],
                                      a["acc_dustmass"], a["acc_momentum"], acc, par.dust)
        vel[loc], mass[loc] = v5, m5
        fp.set_field(B.F_VEL, vel)
        fp.set_field(B.F_MASS, mass)
        rows = AC.rows_of(B, s, dens[r])
        rows[:, B.SK_ACC_MASS] = a["acc_mass"]
        rows[:, B.SK_ACC_BHMASS] = a["acc_bhmass"]
        rows[:, B.SK_ACC_DUSTMASS] = a["acc_dustmass"]
        rows[:, B.SK_ACC_MOMENTUM:B.SK_ACC_MOMENTUM + 3] = a["acc_momentum"]
        mirror[glob] = rows
        rep.update(counts=a["counts"].copy(), nactive=len(loc))
        reps.append(rep)
    return reps


def resident_step(run, gd, gp, acc):
    it = run.S.run.sinks_density(gd, NGB)
    return it, run.S.run.blackhole_accretion(gp, _gacc(run.B, acc))


def _feeders(run, sinks_glob):
    """per gas particle (global index), how many of the sinks hold it inside their search sphere, with a margin
    of 1e-9 so that a tie counts (tests/test_gpu_sink_accretion.py::_feeders)"""
    B, pr = run.B, run.pr
    pos, h = run.S.get_field(B.F_POS), run.S.get_field(B.F_HSML)
    k = np.zeros(pr.ngas, np.int64)
    for i in sinks_glob:
        d = pos[:pr.ngas] - pos[i][None, :]
        if pr.periodic:
            d -= pr.box * np.round(d / pr.box)
        k += np.sqrt((d * d).sum(axis=1)) < h[i] * (1 + 1e-9)
    return k


def same_state(ra, rb, feeders=None, mirror=None, fields=None):
    """shard by shard, bit for bit: the fields, SwallowID, Injected_BH_Energy (equal where a gas particle has at
    most two feeders, within (k - 1) 2^-52 of the sum for k feeders), and -- mirror given: rb is the per-pass side
    -- every column of ra's tables against the mirror's rows; else against rb's tables."""
    B = ra.B
    fields = fields or (B.F_MASS, B.F_VEL, B.F_HSML, B.F_POS, B.F_TYPE, B.F_ID)
    for r, (fa, fb) in enumerate(zip(ra.S.fp, rb.S.fp)):
        assert fa.counts() == fb.counts()
        ids_t, rows_t = fa.sinks_table()
        assert np.all(np.diff(ids_t.astype(np.int64)) > 0), "shard %d: the table is not sorted by ID" % r
        if mirror is not None:
            glob = ra.sinks_on(r)[1]
            want_ids = ra.sp.ids[glob]
            o = np.argsort(want_ids)
            assert np.array_equal(ids_t, want_ids[o]), "shard %d: rows %s, sinks %s" % (r, ids_t, want_ids[o])
            want = mirror[glob][o]
        else:
            ids_b, want = fb.sinks_table()
            assert np.array_equal(ids_t, ids_b)
        for c in range(B.SK_COUNT):
            assert np.array_equal(rows_t[:, c], want[:, c]), "shard %d column %d" % (r, c)
        if fa.n == 0:
            continue
        for f in fields:
            a, b = fa.get_field(f), fb.get_field(f)
            assert np.array_equal(a, b), "shard %d field %d differs at %s" % (r, f, np.argwhere(a != b)[:5].tolist())
        (swa, inja), (swb, injb) = fa.sink_marks(), fb.sink_marks()
        assert np.array_equal(swa, swb), "shard %d SwallowID" % r
        k = np.zeros(fa.ngas, np.int64) if feeders is None else feeders[ra.S.gid[r][:fa.ngas]]
        many = k >= 3
        assert np.array_equal(inja[~many], injb[~many]), "shard %d Injected_BH_Energy" % r
        if many.any():
            assert np.all(np.abs(inja - injb)[many] <= (k[many] - 1) * 2.0 ** -52 * np.maximum(inja, injb)[many])


def same_reports(ra, rb):
    for a, b in zip(ra, rb):
        assert np.array_equal(a["counts"], b["counts"]), (a["counts"], b["counts"])
        assert a["nactive"] == b["nactive"]
        for k in ("bin_mass", "bin_dynmass", "bin_mdot"):
            assert np.array_equal(a[k], b[k]), k


def _mirror_of(B, sp, rows):
    m = np.zeros((sp.pr.n, B.SK_COUNT))
    m[sp.sinks] = rows
    return m


# ------------------------------------------------------------------------------------------------
# a. bit for bit against the per-pass shard path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nshards,periodic,switches", [(3, 1, SINK_SWITCHES[0]), (3, 0, SINK_SWITCHES[1]),
                                                       (5, 1, SINK_SWITCHES[2]), (5, 0, SINK_SWITCHES[0]),
                                                       (8, 1, SINK_SWITCHES[1]), (8, 0, SINK_SWITCHES[2])])
def test_resident_form_equals_the_per_pass_forms(nshards, periodic, switches):
    sp = AC.stock(periodic)
    pr = sp.pr
    B = bindings()
    state = AC.state_for(sp)
    acc = AC.acc_for(sp, state)
    par = AC.ref_par(sp, switches)
    rows0 = AC.rows_of(B, state)
    ra, rb = Run(sp, nshards, rows0), Run(sp, nshards)
    try:
        gp = sp.params(B.BhParams, **sink_over(*switches))
        mirror = _mirror_of(B, sp, rows0)
        ra.trees()
        rb.trees()
        it, rep_a = resident_step(ra, pr.g_dens(), gp, acc)
        rep_b = per_pass_step(rb, mirror, pr.g_dens(), gp, par, acc)
        assert it >= 1
        assert sum(len(ra.sinks_on(r)[0]) > 0 for r in range(nshards)) >= 2      # the sinks lie on several shards
        same_reports(rep_a, rep_b)
        same_state(ra, rb, _feeders(ra, sp.sinks), mirror)
        total = sum(r["counts"] for r in rep_a)
        assert total.sum() > 10 and sum(r["nactive"] for r in rep_a) == len(sp.sinks)
        assert (ra.S.get_field(B.F_MASS) == 0).sum() == total.sum()
        # afterwards as after the per-pass GHIP_DD_BH_SWALLOW: the trees are stale (in mass only)
        with pytest.raises(B.GhipError, match="GHIP_DD_GRAVITY of this step first"):
            ra.S.run.blackhole_accretion(gp, _gacc(B, acc))
    finally:
        ra.close()
        rb.close()


# ------------------------------------------------------------------------------------------------
# b. against one GPU
# ------------------------------------------------------------------------------------------------
def _astride(sp):
    """the periodic problem translated (every position by one vector, modulo the box: the same physics) so that
    the central object and the sink it merges with lie on either side of the plane through the middle of the
    box -- a boundary of the cells the curve is cut on at every level, and of the key ranges of 3, 5 and 8
    shards (asserted by the caller: the two end on different shards)"""
    pr = sp.pr
    pos = pr.ic["pos"]
    c, v = sp.sinks[0], sp.sinks[1]
    d = pos[v] - pos[c]
    d -= pr.box * np.round(d / pr.box)
    ax = int(np.argmax(np.abs(d)))
    t = np.zeros(3)
    t[ax] = 0.5 * pr.box - (pos[c] + 0.5 * d)[ax]
    pr.ic["pos"] = np.mod(pos + t, pr.box)
    pr.extent = O.domain_extent(pr.ic["pos"])
    return sp


def _input(name):
    if name == "stock":
        return AC.stock(1)
    return sink_case(name, 1, at=SINK_PAIR_AT) if name == "pair" else _astride(sink_case(name, 1))


@pytest.mark.parametrize("name,nshards", [("stock", 3), ("stock", 8), ("pair", 3), ("pair", 8), ("central", 5)])
def test_against_one_gpu(name, nshards):
    sp = _input(name)
    pr, sk = sp.pr, sp.sinks
    B = bindings()
    state = AC.state_for(sp)
    acc = AC.acc_for(sp, state)
    switches = SINK_SWITCHES[2] if name == "stock" else SINK_SWITCHES[0]
    gp = sp.params(B.BhParams, **sink_over(*switches))
    rows0 = AC.rows_of(B, state)
    one = pr.device()
    run = Run(sp, nshards, rows0)
    try:
        one.set_field(B.F_HSML, sp.hsml)
        one.set_field(B.F_ID, sp.ids.view(np.int32))
        one.set_field(B.F_DENSITY, sp.gas_density)
        pr.device_tree(one)
        one.sinks_set_table(sp.ids[sk], rows0)
        it1 = one.sinks_density(pr.g_dens(), NGB)
        rep1 = one.blackhole_accretion(gp, _gacc(B, acc))
        run.trees()
        it, reps = resident_step(run, pr.g_dens(), gp, acc)
        S = run.S
        # exactly: iteration counts, marks, victims, counts
        assert it == it1 >= 1
        sw1, _ = one.sink_marks()
        sw = np.zeros(pr.n, np.uint32)
        for r, fp in enumerate(S.fp):
            if fp.n:
                sw[S.gid[r]] = fp.sink_marks()[0]
        assert np.array_equal(sw, sw1) and (sw > 0).sum() >= 1
        mass, mass1 = S.get_field(B.F_MASS), one.get_field(B.F_MASS)
        assert np.array_equal(mass == 0, mass1 == 0)
        assert np.array_equal(sum(r["counts"] for r in reps), rep1["counts"])
        assert sum(r["nactive"] for r in reps) == rep1["nactive"] == len(sk)
        # to 1e-13 of the field's largest value: what the rank-ordered partial sums feed
        close = lambda a, b: np.abs(a - b).max() <= 1e-13 * max(np.abs(b).max(), 1e-300)
        rest = np.setdiff1d(np.arange(pr.n), sk)
        assert np.array_equal(mass[rest], mass1[rest])
        assert close(mass[sk], mass1[sk])
        assert close(S.get_field(B.F_HSML)[sk], one.get_field(B.F_HSML)[sk])
        vel, vel1 = S.get_field(B.F_VEL), one.get_field(B.F_VEL)
        assert np.array_equal(vel[rest], vel1[rest]) and close(vel[sk], vel1[sk])
        ids1, rows1 = one.sinks_table()
        got = {}
        for fp in S.fp:
            ids_t, rows_t = fp.sinks_table()
            got.update({int(i): row for i, row in zip(ids_t, rows_t)})
        assert sorted(got) == [int(i) for i in ids1]
        rows = np.array([got[int(i)] for i in ids1])
        for c in range(B.SK_COUNT):
            assert close(rows[:, c], rows1[:, c]), "column %d" % c
        assert np.array_equal(rows[:, B.SK_BH_MASS] == 0, rows1[:, B.SK_BH_MASS] == 0)
        for k in ("bin_mass", "bin_dynmass", "bin_mdot"):
            assert close(sum(r[k] for r in reps), rep1[k]), k
        if name == "pair":
            # each of the two sinks has victims of its own on other shards than itself; neither swallows
            for g in sk:
                marked = np.where(sw == sp.ids[g])[0]
                assert (S.owner[marked] != S.owner[g]).sum() >= 1, "sink %d: all its victims are on its own shard" % g
            assert not rep1["counts"].any() and np.array_equal(mass, pr.ic["mass"])
        if name == "central":
            # the central object swallows the sink inside InnerBoundary, which lies on another shard
            assert rep1["counts"][1] >= 1
            gone = sk[mass1[sk] == 0]
            assert len(gone) >= 1 and any(S.owner[g] != S.owner[sk[0]] for g in gone), \
                "the merger does not cross shards: %s" % S.owner[sk]
    finally:
        one.close()
        run.close()


# ------------------------------------------------------------------------------------------------
# c. the rows migrate
# ------------------------------------------------------------------------------------------------
_COPIED = ("F_POS", "F_VEL", "F_MASS", "F_TYPE", "F_HSML", "F_TIMEBIN", "F_TI_BEGSTEP", "F_OLDACC", "F_ID",
           "F_VELPRED", "F_ENTROPY", "F_DTENTROPY")


def _fresh_copy(run):
    """new contexts loaded with the state of run's shards: the fields, the domain, the key ranges, the tables"""
    B, S = run.B, run.S
    new = Run.__new__(Run)
    new.B, new.sp, new.pr = B, run.sp, run.pr
    new._sorted_ids, new._order = run._sorted_ids, run._order
    import copy
    new.S = T = copy.copy(S)
    T.gid, T.ngas, T.owner = [g.copy() for g in S.gid], list(S.ngas), S.owner.copy()
    T.fp = []
    for r, fp in enumerate(S.fp):
        n, ngl = fp.counts()
        fq = B.ForcePath(0)
        fq.set_counts(n, ngl)
        for name in _COPIED:
            f = getattr(B, name)
            if (ngl if B._FIELD_INFO[f][0] else n) > 0:
                fq.set_field(f, fp.get_field(f))
        fq.dd_init(r, S.P)
        corner, center, ln = fp.dd_get_domain()
        fq.dd_set_domain(corner, center, ln, run.pr.force_soft)
        fq.dd_set_splits(fp.dd_get_splits())
        fq.sinks_set_table(*fp.sinks_table())
        T.fp.append(fq)
    import importlib
    T.run = importlib.import_module("gadget-leicester_amd.sharded").DomainShards(T.fp)
    return new


@pytest.mark.parametrize("nshards", [3, 5])
def test_rows_migrate(nshards):
    sp = AC.stock(1)
    pr = sp.pr
    B = bindings()
    state = AC.state_for(sp)
    acc = AC.acc_for(sp, state)
    gp = sp.params(B.BhParams, **sink_over(*SINK_SWITCHES[0]))
    rng = np.random.default_rng(7)
    rows0 = AC.rows_of(B, state) + rng.random((len(sp.sinks), B.SK_COUNT))      # every column tells its row
    run = Run(sp, nshards, rows0)
    fresh = None
    try:
        S = run.S
        before = {int(i): rows0[k] for k, i in enumerate(sp.ids[sp.sinks])}
        home = S.owner[sp.sinks].copy()
        # the drift: every sink of the shard that holds most of them goes to the middle of the next shard's range
        src = int(np.bincount(home, minlength=nshards).argmax())
        dst = (src + 1) % nshards
        movers = sp.sinks[home == src]
        assert len(movers) >= 2
        there = np.where((S.owner == dst) & (pr.ic["type"] == 1))[0]
        there = there[np.argsort(S.keys[there])]
        mid = there[len(there) // 2 - len(movers) // 2:][:len(movers)]
        fp = S.fp[src]
        pos = fp.get_field(B.F_POS)
        loc, glob = run.sinks_on(src)
        assert np.array_equal(np.sort(glob), np.sort(movers))
        newpos = dict(zip(movers, pr.ic["pos"][mid] + 0.05 * pr.ic["spacing"]))
        for l, g in zip(loc, glob):
            pos[l] = newpos[g]
        fp.set_field(B.F_POS, pos)
        sent0 = [q.dd_bytes_sent(B.DD_MIGRATE) for q in S.fp]
        S.run.redistribute()
        run.refresh()
        now = S.owner[sp.sinks]
        assert (now != home).sum() >= 2 and min(len(run.sinks_on(r)[0]) for r in range(nshards)) == 0, (home, now)
        # the union of the tables is the table before, bit for bit; each row lies with its particle; sorted
        seen = {}
        for r, q in enumerate(S.fp):
            ids_t, rows_t = q.sinks_table()
            assert np.all(np.diff(ids_t.astype(np.int64)) > 0)
            assert np.array_equal(ids_t, np.sort(sp.ids[run.sinks_on(r)[1]])), "shard %d" % r
            for i, row in zip(ids_t, rows_t):
                assert int(i) not in seen
                seen[int(i)] = row
        assert sorted(seen) == sorted(before)
        assert all(np.array_equal(seen[i], before[i]) for i in before)
        # the rows are part of the traffic: 8 + 8 * SK_COUNT bytes for each that left
        rowbytes = 8 + 8 * B.SK_COUNT
        assert S.fp[src].dd_bytes_sent(B.DD_MIGRATE) >= len(movers) * rowbytes
        assert sent0 == [0] * nshards
        # a following resident accretion equals that of shards freshly loaded with the same state
        for q in S.fp:      # (rows with a disc again, so that the sinks accrete)
            ids_t, _ = q.sinks_table()
            k = [list(sp.ids[sp.sinks]).index(i) for i in ids_t]
            q.sinks_set_table(ids_t, AC.rows_of(B, state)[k].reshape(len(k), B.SK_COUNT))
        fresh = _fresh_copy(run)
        run.trees()
        fresh.trees()
        it_a, rep_a = resident_step(run, pr.g_dens(), gp, acc)
        it_b, rep_b = resident_step(fresh, pr.g_dens(), gp, acc)
        assert it_a == it_b >= 1
        same_reports(rep_a, rep_b)
        same_state(run, fresh, _feeders(run, sp.sinks))
        assert sum(r["counts"] for r in rep_a).sum() > 5
        # the table is still accepted: the counts the migration changed did not make it stale
        assert sum(len(q.sinks_table()[0]) for q in S.fp) == len(sp.sinks)
    finally:
        run.close()
        if fresh is not None:
            fresh.close()


# ------------------------------------------------------------------------------------------------
# d. three steps on shards: accretion, formation, redistribution with rearrangement and Peano order
# ------------------------------------------------------------------------------------------------
def _sfr_params(B, pr, crit):
    d = sfr_ref.params(cooling=sfr_ref.NONE, dust=0, Timebase_interval=pr.timebase, CritPhysDensity_code=crit,
                       OriginalGasMass=float(pr.ic["mass"][0]), MinEgySpec=1e-6)
    p = B.SfrParams()
    for k, v in d.items():
        if k == "smbh_pos":
            for c in range(3):
                p.smbh_pos[c] = float(v[c])
        else:
            setattr(p, k, v)
    return p


def test_three_steps_on_shards():
    nshards = 3
    sp = AC.stock(1)
    pr = sp.pr
    B = bindings()
    state = AC.state_for(sp)
    acc = AC.acc_for(sp, state)
    par = AC.ref_par(sp, SINK_SWITCHES[0])
    gp = sp.params(B.BhParams, **sink_over(*SINK_SWITCHES[0]))
    rows0 = AC.rows_of(B, state)
    ra, rb = Run(sp, nshards, rows0), Run(sp, nshards)
    rng = np.random.default_rng(31)
    try:
        mirror = _mirror_of(B, sp, rows0)
        has_row = np.zeros(pr.n, bool)
        has_row[sp.sinks] = True
        formed_total = dropped_total = swallowed_sinks = 0
        for step in range(3):
            # the densest gas converts: a threshold that five more gas particles pass in every step
            sfr = _sfr_params(B, pr, float(np.sort(sp.gas_density)[-5 * (step + 1)]))
            ra.trees()
            rb.trees()
            sinks_now = np.concatenate([ra.sinks_on(r)[1] for r in range(nshards)])
            it, rep_a = resident_step(ra, pr.g_dens(), gp, acc)
            rep_b = per_pass_step(rb, mirror, pr.g_dens(), gp, par, acc)
            same_reports(rep_a, rep_b)
            same_state(ra, rb, _feeders(ra, sinks_now), mirror)
            swallowed_sinks += int(sum(r["counts"][1] for r in rep_a))
            # formation on the shards: the candidates of each shard's own ghip_sfr_cooling, one draw each
            for r in range(nshards):
                fa, fb = ra.S.fp[r], rb.S.fp[r]
                if fa.ngas == 0:
                    continue
                ca, cb = fa.sfr_cooling(sfr), fb.sfr_cooling(sfr)
                assert np.array_equal(ca, cb)
                u = rng.random(len(ca))
                fa.sfr_form_sinks(len(ca), u, True)
                # the per-pass side: the host converts and keeps the new rows
                glob = rb.S.gid[r][cb]
                typ, mass = fb.get_field(B.F_TYPE), fb.get_field(B.F_MASS)
                out = AR.form_sinks(cb, u, mass, typ, fb.get_field(B.F_TIMEBIN), True)
                fb.set_field(B.F_TYPE, out["type"])
                fb.set_field(B.F_MASS, out["mass"])
                mirror[glob] = AC.rows_of(B, out["rows"])
                has_row[glob] = True
                formed_total += len(ca)
                # the new sinks have rows on their shard
                assert np.all(np.isin(sp.ids[glob], fa.sinks_table()[0]))
            same_state(ra, rb, None, mirror, fields=(B.F_MASS, B.F_TYPE, B.F_ID))
            out_a = ra.S.run.redistribute(rearrange=True, peano_order=True)
            out_b = rb.S.run.redistribute(rearrange=True, peano_order=True)
            assert out_a["tot_elim"] == out_b["tot_elim"]
            ra.refresh()
            rb.refresh()
            # the rows of eliminated sinks are gone (the host drops them from its mirror by looking at who is left)
            left = np.zeros(pr.n, bool)
            for r in range(nshards):
                left[ra.S.gid[r]] = True
            dropped_total += int((has_row & ~left).sum())
            has_row &= left
            held = sum(len(q.sinks_table()[0]) for q in ra.S.fp)
            assert held == has_row.sum(), (held, has_row.sum())
            same_state(ra, rb, None, mirror, fields=(B.F_MASS, B.F_VEL, B.F_HSML, B.F_POS, B.F_TYPE, B.F_ID))
        print("three steps on shards: %d sinks formed, %d swallowed, %d rows dropped"
              % (formed_total, swallowed_sinks, dropped_total))
        assert formed_total >= 10 and dropped_total == swallowed_sinks >= 1, (formed_total, swallowed_sinks, dropped_total)
    finally:
        ra.close()
        rb.close()


# ------------------------------------------------------------------------------------------------
# e. failures are collective
# ------------------------------------------------------------------------------------------------
def _snapshot(run):
    B = run.B
    return [(fp.get_field(B.F_MASS), fp.get_field(B.F_VEL), fp.get_field(B.F_HSML), fp.sinks_table())
            for fp in run.S.fp]


def _unchanged(run, snap, tables=True):
    B = run.B
    for fp, (m, v, h, t) in zip(run.S.fp, snap):
        assert np.array_equal(fp.get_field(B.F_MASS), m) and np.array_equal(fp.get_field(B.F_VEL), v)
        assert np.array_equal(fp.get_field(B.F_HSML), h)
        sw, inj = fp.sink_marks()
        assert not sw.any() and not inj.any()          # the marks were reset, nothing else happened
        if tables and t is not None:
            ids_t, rows_t = fp.sinks_table()
            assert np.array_equal(ids_t, t[0]) and np.array_equal(rows_t, t[1])


def _sinks_args(run, acc, gp):
    return [run.B.dd_sinks_args(bh=gp, acc=_gacc(run.B, acc)) for _ in run.S.fp]


def test_failures_are_collective():
    nshards = 3
    sp = AC.stock(1)
    pr = sp.pr
    B = bindings()
    state = AC.state_for(sp)
    acc = AC.acc_for(sp, state)
    gp = sp.params(B.BhParams, **sink_over(*SINK_SWITCHES[0]))
    rows0 = AC.rows_of(B, state)
    ids5 = sp.ids[sp.sinks]
    run = Run(sp, nshards, rows0)
    try:
        S = run.S
        FORM = B.SINKS_RESIDENT_FORM
        held = [len(run.sinks_on(r)[0]) for r in range(nshards)]
        k = int(np.argmax(held))
        assert held[k] >= 2
        full = [fp.sinks_table() for fp in S.fp]
        run.trees()
        snap = _snapshot(run)
        # 1. one shard lacks the row of an active sink
        ids_k, rows_k = snap[k][3]
        lost = int(ids_k[-1])
        S.fp[k].sinks_set_table(ids_k[:-1], rows_k[:-1])
        snap_lost = _snapshot(run)
        built = _sinks_args(run, acc, gp)
        errs = failing_collective(S.fp, B.DD_BH_SWALLOW, [b[0] for b in built], FORM)
        assert all(e.code == EINVAL for e in errs) and all(str(lost) in str(e) for e in errs), [str(e) for e in errs]
        assert "no row" in str(errs[k]) and all("shard %d" % k in str(e) for r, e in enumerate(errs) if r != k)
        _unchanged(run, snap_lost)
        # ... the density form stops in the same way and changes nothing
        built = [B.dd_sinks_args(dens=pr.g_dens(), ngb_factor=NGB) for _ in S.fp]
        errs = failing_collective(S.fp, B.DD_SINK_DENSITY, [b[0] for b in built], FORM)
        assert all(e.code == EINVAL for e in errs) and all(str(lost) in str(e) for e in errs)
        _unchanged(run, snap_lost)
        # 2. one shard without a table while the others hold one
        S.fp[k].sinks_clear()
        errs = failing_collective(S.fp, B.DD_BH_SWALLOW, [b[0] for b in _sinks_args(run, acc, gp)], FORM)
        assert all(e.code == EINVAL for e in errs) and all("no sink table" in str(e) for e in errs)
        _unchanged(run, snap_lost, tables=False)
        errs = failing_collective(S.fp, B.DD_MIGRATE, None)
        assert all(e.code == EINVAL for e in errs) and all("nothing was moved" in str(e) for e in errs)
        assert [fp.counts() for fp in S.fp] == [(len(s[0]), fp.ngas) for s, fp in zip(snap, S.fp)]
        # 3. GHIP_DD_BH_EVALUATE has no resident form
        with pytest.raises(B.GhipError, match="GHIP_DD_BH_EVALUATE") as e:
            S.fp[0].dd_begin(B.DD_BH_EVALUATE, _sinks_args(run, acc, gp)[0][0], FORM)
        assert e.value.code == EINVAL
        # ... and one GPU's entry points name the collective to use on a shard
        with pytest.raises(B.GhipError, match="GHIP_DD_BH_SWALLOW") as e:
            S.fp[0].blackhole_accretion(gp, _gacc(B, acc))
        assert e.value.code == EINVAL
        with pytest.raises(B.GhipError, match="GHIP_DD_SINK_DENSITY") as e:
            S.fp[0].sinks_density(pr.g_dens(), NGB)
        assert e.value.code == EINVAL
        # 4. after the failures the next valid operation runs, and equals a run that never failed
        S.fp[k].sinks_set_table(*full[k])
        it, reps = resident_step(run, pr.g_dens(), gp, acc)
        assert it >= 1 and sum(r["nactive"] for r in reps) == len(sp.sinks)
        assert sum(r["counts"] for r in reps).sum() > 10
        other = Run(sp, nshards, rows0)
        try:
            other.trees()
            it_o, reps_o = resident_step(other, pr.g_dens(), gp, acc)
            assert it_o == it
            same_reports(reps, reps_o)
            same_state(run, other, _feeders(run, sp.sinks))
        finally:
            other.close()
    finally:
        run.close()


def test_one_id_on_two_shards_and_a_replicated_shard():
    nshards = 3
    sp = AC.stock(1)
    pr = sp.pr
    B = bindings()
    state = AC.state_for(sp)
    acc = AC.acc_for(sp, state)
    gp = sp.params(B.BhParams, **sink_over(*SINK_SWITCHES[0]))
    rows0 = AC.rows_of(B, state)
    run = Run(sp, nshards, rows0)
    try:
        S = run.S
        held = [run.sinks_on(r) for r in range(nshards)]
        a, b = [r for r in range(nshards) if len(held[r][0])][:2]
        # a sink of shard b takes the ID of a sink of shard a, in its ID field and in its row: neither shard's
        # table sees a duplicate
        twice = sp.ids[held[a][1][0]]
        fb = S.fp[b]
        idf = fb.get_field(B.F_ID)
        old = idf[held[b][0][0]]
        idf[held[b][0][0]] = np.uint32(twice).view(np.int32)
        fb.set_field(B.F_ID, idf)
        ids_t, rows_t = fb.sinks_table()
        ids_t[ids_t == np.int32(old).view(np.uint32)] = twice
        fb.sinks_set_table(ids_t, rows_t)
        run.trees()
        snap = _snapshot(run)
        errs = failing_collective(S.fp, B.DD_BH_SWALLOW, [x[0] for x in _sinks_args(run, acc, gp)],
                                  B.SINKS_RESIDENT_FORM)
        assert all(e.code == EINVAL for e in errs), [str(e) for e in errs]
        assert all(("the ID %d" % twice) in str(e) for e in errs), [str(e) for e in errs]
        _unchanged(run, snap)
        # the same ID arriving where it already has a row: the migration fails on all shards and names it
        # (moved there by hand: the particle of shard b goes where shard a's lies)
        fa = S.fp[a]
        pos_b = fb.get_field(B.F_POS)
        pos_b[held[b][0][0]] = fa.get_field(B.F_POS)[held[a][0][0]] + 0.01 * pr.ic["spacing"]
        fb.set_field(B.F_POS, pos_b)
        errs = failing_collective(S.fp, B.DD_MIGRATE, None)
        assert all(str(twice) in str(e) for e in errs), [str(e) for e in errs]
    finally:
        run.close()
    # a replicated shard is still refused
    fp = pr.device()
    try:
        fp.set_field(B.F_ID, sp.ids.view(np.int32))
        fp.set_shard(1, 2)
        with pytest.raises(B.GhipError, match="replicated shard") as e:
            fp.sinks_set_table(sp.ids[sp.sinks], rows0)
        assert e.value.code == EINVAL
    finally:
        fp.close()


# ------------------------------------------------------------------------------------------------
# f. two rank processes
# ------------------------------------------------------------------------------------------------
RANK_OPS = ("DD_SINK_DENSITY", "DD_BH_SWALLOW", "DD_MIGRATE")


def rank_case():
    sp = AC.stock(1)
    state = AC.state_for(sp)
    return sp, AC.rows_of(bindings(), state), AC.acc_for(sp, state)


def rank_sequence(run, shards, acc, dom=None):
    """What tests/gpu_host_ranks_sinks.py runs on every rank (dom: its DomainRank, shards = [its rank]) and rank 0
    repeats with both shards in its own process (dom None): the trees, the two resident collectives, a drift that
    sends each shard's first sink to the middle of the other shard's key range, GHIP_DD_MIGRATE.  Returns per shard
    what it holds afterwards."""
    B, S, sp, pr = run.B, run.S, run.sp, run.pr
    gp = sp.params(B.BhParams, **sink_over(*SINK_SWITCHES[0]))
    drv = dom if dom is not None else S.run
    drv.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
    drv.density(pr.g_dens())
    for r in shards:
        g = S.gid[r][:S.ngas[r]]
        if len(g):
            S.fp[r].set_field(B.F_DENSITY, sp.gas_density[g])
    it = drv.sinks_density(pr.g_dens(), NGB)
    reps = drv.blackhole_accretion(gp, _gacc(B, acc))
    reps = {shards[0]: reps} if dom is not None else dict(enumerate(reps))
    marks = {r: S.fp[r].sink_marks() for r in shards}
    for r in shards:
        fp = S.fp[r]
        loc, glob = run.sinks_on(r)
        assert len(loc) >= 1, "shard %d holds no sink" % r
        there = np.where((S.owner == (r + 1) % S.P) & (pr.ic["type"] == 1))[0]
        there = there[np.argsort(S.keys[there])]
        pos = fp.get_field(B.F_POS)
        pos[loc[0]] = pr.ic["pos"][there[len(there) // 2]] + 0.03 * pr.ic["spacing"]
        fp.set_field(B.F_POS, pos)
    drv.migrate()
    out = {}
    for r in shards:
        fp = S.fp[r]
        fp.counts()
        ids_t, rows_t = fp.sinks_table()
        out[r] = dict(it=it, rep=reps[r], sw=marks[r][0], inj=marks[r][1], ids=ids_t, rows=rows_t,
                      fields=[fp.get_field(f) for f in (B.F_POS, B.F_VEL, B.F_MASS, B.F_HSML, B.F_TYPE, B.F_ID)],
                      bytes=[int(fp.dd_bytes_sent(getattr(B, op))) for op in RANK_OPS])
    return out


def rank_results_equal(a, b):
    """bit for bit (two shards: no gas particle has three feeders on one shard's side that the other orders
    differently -- both runs execute the same kernels on the same shard)"""
    same = a["it"] == b["it"] and np.array_equal(a["sw"], b["sw"]) and np.array_equal(a["ids"], b["ids"])
    same = same and np.array_equal(a["rows"], b["rows"]) and a["rep"]["nactive"] == b["rep"]["nactive"]
    same = same and all(np.array_equal(a["rep"][k], b["rep"][k]) for k in ("counts", "bin_mass", "bin_dynmass", "bin_mdot"))
    return bool(same and all(np.array_equal(x, y) for x, y in zip(a["fields"], b["fields"])))


def _run_ranks(transport):
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", SINKS_TRANSPORT=transport)
    if transport == "rccl":
        mock = os.path.join(root, "tests", "mock_rccl", "librccl_mock.so")
        assert os.path.exists(mock), "build tests/mock_rccl first (__graft_entry__.build())"
        env["GHIP_RCCL_LIB"] = mock
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "tests", "gpu_host_ranks_sinks.py")]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_two_rank_processes_equal_the_in_process_run():
    """tests/gpu_host_ranks_sinks.py is the rank program: the resident collectives and a migration that carries rows
    on two rank processes, through the host's all-gather (gloo) and through the RCCL entry points (tests/mock_rccl:
    the real RCCL refuses two ranks on one device); rank 0 compares with both shards in its own process."""
    sent = {}
    for transport in ("host", "rccl"):
        out = _run_ranks(transport)
        assert out["ok"], out
        assert out["transport"] == transport
        if transport == "rccl":
            assert out["rccl_library"].endswith("librccl_mock.so")
        assert out["equal"] == [True, True] and out["iterations"] >= 1, out
        assert out["rows_arrived"] == [1, 1] and sum(out["swallowed"]) > 10, out
        assert out["bytes_equal_in_process"], out
        assert all(b > 0 for rank in out["bytes"] for b in rank), out
        sent[transport] = out["bytes"]
    assert sent["host"] == sent["rccl"], sent
