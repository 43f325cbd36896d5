"""Converted and swallowed gas between two rearrangements, on shards and on a kept gas tree.

A gas record stops being a neighbour in two ways: its Type is no longer 0 (converted: ngb.c:93, 213 skip
it in every neighbour loop, density.c:1049 and hydra.c:184 leave it out of the targets), or its Mass is 0
(swallowed: density.c:831-834 skips it under -DBLACK_HOLES or -DDUST, hydra.c:1235-1238 under
-DBLACK_HOLES only; it stays a target).  ghip_set_massless_gas_rule selects the second behaviour
(1 = -DDUST alone, 3 = -DBLACK_HOLES); the device keeps both as marks in the mass of the gas record.
Here both kinds of record are ghosts of other shards, migrate between shards, and are met again by a
density() that follows a hydro_force() on the same gas tree -- against the oracle's single tree with the
same rule: counts exactly, fields to the suite's tolerance."""
import numpy as np
import pytest

from common import O, Problem, ShardSet, bindings, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-11
SENTINEL = -7.0


def _marked_problem():
    """1000 gas + 1000 DM particles; 25 records of the gas block converted (15 sinks, 10 stars), 40 others
    swallowed (Mass = 0).  Returns the problem, the two sets and the gas that is left (Type 0)."""
    pr = Problem(ng=10, gas=True, periodic=1)
    pick = np.random.default_rng(77).choice(pr.ngas, 65, replace=False)
    conv, gone = np.sort(pick[:25]), np.sort(pick[25:])
    return pr, conv, gone, _mark(pr, conv, gone)


def _mark(pr, conv, gone):
    """the records `conv` of the gas block become sinks (the first 15) and stars, the records `gone` lose their
    mass; returns the gas that is left (Type 0)"""
    assert len(conv) == 25 and len(gone) == 40 and len(np.intersect1d(conv, gone)) == 0
    typ = pr.ic["type"].copy()
    typ[conv[:15]] = 5                      # BH_FORM: gas -> sink
    typ[conv[15:]] = 4                      # SFR: gas -> star
    pr.ic["type"] = typ
    mass = pr.ic["mass"].copy()
    mass[gone] = 0.0
    pr.ic["mass"] = mass
    return np.setdiff1d(np.arange(pr.ngas), conv).astype(np.int32)


class _rule:
    """the massless-gas rule on the oracle (process-global) and on every context, taken back on the way out"""

    def __init__(self, rule, paths=()):
        self.rule, self.paths = rule, paths

    def __enter__(self):
        O.set_massless_gas_rule(self.rule)
        for fp in self.paths:
            fp.set_massless_gas_rule(self.rule)

    def __exit__(self, *exc):
        O.set_massless_gas_rule(0)


def _oracle_step(pr, T, gas, hsml, dtentropy):
    """density(), force_update_hmax() and hydro_force() of the oracle for the targets `gas`"""
    od = T.density(pr.o_dens(), gas, pr.velpred, pr.entropy, dtentropy, pr.timebin, pr.ti_begstep, hsml)
    T.update_hmax(gas, od["hsml"], od["divvel"])
    oh = T.hydro(pr.o_hydro(), gas, pr.velpred, od["hsml"], od["density"], od["pressure"], od["dhsmlfac"],
                 od["divvel"], od["curlvel"], pr.timebin)
    return od, oh


def _frozen(*dicts):
    for d in dicts:
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.flags.writeable = False
    return dicts


@pytest.fixture(scope="module")
def oracle():
    """The oracle's side of the tests on the unshaken problem, computed once for the three rules and
    read-only: oracle[rule] = (od, oh, od2, oh2, visits0), see _oracle_run"""
    return {rule: _oracle_run(rule) for rule in (0, 1, 3)}


def _oracle_run(rule):
    """A step; then density() again from the step's smoothing lengths with the DtEntropy that hydro_force()
    left, and hydro_force() again; and the neighbour visits of that second density() without the rule."""
    pr, conv, gone, gas = _marked_problem()
    T = pr.oracle_tree()
    O.set_massless_gas_rule(rule)
    try:
        od, oh = _oracle_step(pr, T, gas, pr.hsml0, pr.dtentropy)
        dte = pr.dtentropy.copy()
        dte[gas] = oh["dtentropy"][gas]
        od2, oh2 = _oracle_step(pr, T, gas, od["hsml"], dte)
        O.set_massless_gas_rule(0)
        visits0 = T.density(pr.o_dens(), gas, pr.velpred, pr.entropy, dte, pr.timebin, pr.ti_begstep,
                            od["hsml"])["ngb_visits"]
    finally:
        O.set_massless_gas_rule(0)
    return _frozen(od, oh, od2, oh2) + (visits0,)


def _check_density(get, stats, od, gas, conv, full):
    """the device's density() results of the remaining gas (the swallowed records among them: targets)
    against the oracle's; `get` reads a field in global order, `stats` are the contexts' counters"""
    B = bindings()
    fields = [(B.F_NUMNGB, "numngb"), (B.F_HSML, "hsml"), (B.F_DENSITY, "density")]
    if full:
        fields += [(B.F_DHSMLFAC, "dhsmlfac"), (B.F_PRESSURE, "pressure")]
    for fid, key in fields:
        e = relerr(get(fid)[gas], od[key][gas])
        print("%-9s %.3e" % (key, e))
        assert e < TOL, key
    got, want = sum(s["dens_neighbours"] for s in stats), od["ngb_visits"]
    print("neighbour visits %d, oracle %d" % (got, want))
    assert got == want, "neighbour visits"
    got, want = max(s["dens_iterations"] for s in stats), od["iterations"]
    print("h iterations %d, oracle %d" % (got, want))
    assert got == want, "h iterations"
    assert np.array_equal(get(B.F_DENSITY)[conv], np.full(len(conv), SENTINEL)), "a converted record was evaluated"


def _check_hydro(get, stats, oh, gas, full):
    B = bindings()
    got, want = sum(s["hydro_pairs"] for s in stats), oh["npairs"]
    print("hydro pairs %d, oracle %d" % (got, want))
    assert got == want, "hydro pairs"
    want = oh["hydroaccel"][gas]
    e = np.abs(get(B.F_HYDROACCEL)[gas] - want).max() / np.abs(want).max()
    print("hydroaccel %.3e" % e)
    assert e < TOL, "HydroAccel"
    if full:
        want = oh["dtentropy"][gas]
        e = np.abs(get(B.F_DTENTROPY)[gas] - want).max() / np.abs(want).max()
        print("dtentropy %.3e" % e)
        assert e < TOL, "DtEntropy"
    e = relerr(get(B.F_MAXSIGNALVEL)[gas], oh["maxsignalvel"][gas])
    print("maxsignalvel %.3e" % e)
    assert e < TOL, "MaxSignalVel"


def _ghosts_of_other_shards(pr, recs, gas, hsml, owner):
    """which of the records `recs` lie within max(h_i, h_j) of a Type-0 gas target j that another shard owns
    (periodic distances): those are ghosts there, for density() or for hydro_force()"""
    pos, box = pr.ic["pos"], pr.box
    out = np.zeros(len(recs), bool)
    for k, i in enumerate(recs):
        d = pos[gas] - pos[i]
        d -= box * np.round(d / box)
        r = np.sqrt((d * d).sum(axis=1))
        out[k] = np.any((r <= np.maximum(hsml[gas], hsml[i])) & (owner[gas] != owner[i]))
    return out


def _within_h(pr, targets, recs, hsml):
    """which of `targets` have one of the other records `recs` inside their own smoothing length"""
    pos, box = pr.ic["pos"], pr.box
    out = np.zeros(len(targets), bool)
    for k, i in enumerate(targets):
        d = pos[recs] - pos[i]
        d -= box * np.round(d / box)
        out[k] = np.any(((d * d).sum(axis=1) < hsml[i] ** 2) & (recs != i))
    return out


def _shard_step(pr, S):
    B = bindings()
    S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)   # the tree of this step
    S.run.density(pr.g_dens())
    S.each(lambda fp: fp.update_hmax())
    S.run.hydro(pr.g_hydro())


@pytest.mark.parametrize("nshards", [3, 8])
@pytest.mark.parametrize("rule", [0, 1, 3])
def test_converted_and_swallowed_ghosts_on_shards_equal_the_single_tree(oracle, rule, nshards):
    """A converted record travels as a ghost with the converted mark and stays nobody's neighbour in
    density() and in hydro_force() under every rule; a swallowed one travels with mass 0, is skipped by
    density() under rules 1 and 3 and by hydro_force() under rule 3 only."""
    B = bindings()
    pr, conv, gone, gas = _marked_problem()
    od, oh = oracle[rule][:2]
    S = ShardSet(pr, nshards)
    try:
        # the test reaches the ghost path: some record of each kind is in reach of another shard's target
        assert _ghosts_of_other_shards(pr, conv, gas, od["hsml"], S.owner).any()
        assert _ghosts_of_other_shards(pr, gone, gas, od["hsml"], S.owner).any()
        with _rule(rule, S.fp):
            S.set_field(B.F_DENSITY, np.full(pr.ngas, SENTINEL))
            _shard_step(pr, S)
            st = S.each(lambda fp: fp.stats())
            _check_density(S.get_field, st, od, gas, conv, full=True)
            _check_hydro(S.get_field, st, oh, gas, full=True)
    finally:
        S.close()


@pytest.mark.parametrize("nshards", [1, 3], ids=["one context", "3 shards"])
@pytest.mark.parametrize("rule", [1, 3])
def test_density_after_hydro_on_the_kept_gas_tree_still_skips_swallowed_gas(oracle, rule, nshards):
    """A sub-step on the kept tree, or a second density() of a step: under rule 1 hydro_force() has summed
    the swallowed gas, and the density() that follows skips it again (density.c:831).  One context keeps its
    gas tree between the calls; shards build theirs from the ghosts of each call."""
    B = bindings()
    pr, conv, gone, gas = _marked_problem()
    od, oh, od2, oh2, visits0 = oracle[rule]
    # the test can tell the difference: without the rule the second density() visits other neighbours
    assert visits0 != od2["ngb_visits"]
    if nshards == 1:
        paths = [pr.device()]
        fp = paths[0]
        set_field, get, close = fp.set_field, fp.get_field, fp.close
        density = lambda: fp.density(pr.g_dens())                                  # noqa: E731
        hydro = lambda: (fp.update_hmax(), fp.hydro(pr.g_hydro()))                 # noqa: E731
    else:
        S = ShardSet(pr, nshards)
        paths, set_field, get, close = S.fp, S.set_field, S.get_field, S.close
        density = lambda: S.run.density(pr.g_dens())                               # noqa: E731
        hydro = lambda: (S.each(lambda fp: fp.update_hmax()), S.run.hydro(pr.g_hydro()))   # noqa: E731
    stats = lambda: [fp.stats() for fp in paths]                                   # noqa: E731
    try:
        with _rule(rule, paths):
            set_field(B.F_DENSITY, np.full(pr.ngas, SENTINEL))
            if nshards == 1:
                pr.device_tree(fp)
            else:
                S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
            density()
            hydro()
            _check_hydro(get, stats(), oh, gas, full=True)
            density()                       # no tree build since the hydro call
            _check_density(get, stats(), od2, gas, conv, full=False)
            hydro()
            _check_hydro(get, stats(), oh2, gas, full=False)
            if nshards == 1:
                # the single evaluation follows the rule of density() as well, whatever ran before it: three
                # targets with a swallowed record inside their smoothing length
                T = pr.oracle_tree()
                near = _within_h(pr, gas, gone, od2["hsml"])
                assert near.sum() >= 3
                for t in gas[near][:3]:
                    got = fp.density_evaluate(pr.g_dens(), int(t), od2["hsml"][t])
                    want = T.density_evaluate(pr.o_dens(), int(t), od2["hsml"][t], pr.velpred)
                    print("density_evaluate", t, np.abs(got - want).max())
                    assert np.allclose(got, want, rtol=TOL, atol=1e-13 * np.abs(want).max())
    finally:
        close()


@pytest.mark.parametrize("rule", [1, 3])
def test_neighbour_lists_after_hydro_follow_the_rule_of_their_loop(oracle, rule):
    """ghip_ngb_treefind on the kept gas tree after a hydro call.  Without pairs it is the list that density()
    sums: ngb_treefind_variable's (ngb.c:93: no converted record) less the swallowed records, under both
    rules.  With pairs it is the list that hydro_force() sums: ngb_treefind_pairs' with the swallowed records
    under rule 1, without them under rule 3.  Neither depends on which call came before, and a density()
    after the queries visits what it visited without them."""
    B = bindings()
    pr, conv, gone, gas = _marked_problem()
    od, oh, od2, oh2, visits0 = oracle[rule]
    pos = pr.ic["pos"]
    fp = pr.device()
    try:
        with _rule(rule, [fp]):
            T = pr.oracle_tree()
            fp.set_field(B.F_DENSITY, np.full(pr.ngas, SENTINEL))
            pr.device_tree(fp)
            fp.density(pr.g_dens())
            fp.update_hmax()
            fp.hydro(pr.g_hydro())

            def lists(i):
                c, h = pos[i] + 0.05 * od["hsml"][i], od["hsml"][i]
                plain = np.sort(T.ngb_variable(c, h, 1, pr.box))
                pairs = np.sort(T.ngb_pairs(c, h, od["hsml"], 1, pr.box))
                # the test can tell the difference: swallowed records are in reach, converted ones are not listed
                assert len(np.intersect1d(plain, gone)) and len(np.intersect1d(pairs, gone))
                assert not len(np.intersect1d(pairs, conv))
                want = (np.setdiff1d(plain, gone), pairs if rule == 1 else np.setdiff1d(pairs, gone))
                return c, h, want

            for i in gone[:3]:
                c, h, (plain, pairs) = lists(i)
                for with_pairs in (0, 1, 1, 0, 0):      # in every order of the two kinds of call
                    lst, cnt = fp.ngb_treefind(c, h, with_pairs, 1, pr.box)
                    assert cnt == len(lst)
                    assert np.array_equal(np.sort(lst), pairs if with_pairs else plain), \
                        "pairs = %d around record %d" % (with_pairs, i)
            fp.ngb_treefind(pos[gone[0]], od["hsml"][gone[0]], 1, 1, pr.box)    # (the last query: with pairs)
            fp.density(pr.g_dens())
            _check_density(fp.get_field, [fp.stats()], od2, gas, conv, full=False)
    finally:
        fp.close()


def _keys_on_the_curve(pr, pos):
    """Peano-Hilbert keys as the shards compute them (ShardSet checks the device's against the same)"""
    ip = ((pos - pr.extent[0]) * ((1 << 21) / pr.extent[2])).astype(np.int64)
    return np.array([O.peano_hilbert_key(*p) for p in ip], dtype=np.uint64)


def test_migration_carries_converted_and_swallowed_records():
    """After a shake some converted and some swallowed records belong to another shard.  They arrive in the
    gas block of their new shard, which must find that block mixed before it builds the next gas tree.  One
    receiving shard holds pure gas before the migration: nothing but the check that follows an arrival can
    tell it that a converted record is now in its gas block -- without it the arrival would be a density
    target.  After the step the arrival is nobody's neighbour and its density is what it was."""
    B = bindings()
    rule, nshards = 3, 4
    pr = Problem(ng=10, gas=True, periodic=1)
    n, ng = pr.n, pr.ngas
    S = ShardSet(pr, nshards)
    mixed = lambda r: S.fp[r].L.ghip_gas_block_mixed(S.fp[r].h)                    # noqa: E731
    try:
        lo, ln = pr.extent[0], pr.extent[2]
        newpos = pr.ic["pos"] + 0.02 * ln * np.random.default_rng(5).standard_normal((n, 3))
        newpos = np.mod(newpos, pr.box)
        newpos[newpos >= pr.box] = 0.0
        newpos = np.clip(newpos, lo + 1e-9 * ln, lo + ln * (1 - 1e-9))
        # who will move where: the keys of the shaken gas on the shards' splits
        now = S.owner[:ng]
        then = np.searchsorted(S.splits[1:nshards], _keys_on_the_curve(pr, newpos[:ng]), side="right")
        arrivals = [np.where((now != r) & (then == r))[0] for r in range(nshards)]
        R = int(np.argmax([len(a) for a in arrivals]))          # the receiver that stays pure until then
        assert len(arrivals[R]) >= 2
        # 25 converted records, none on R, two of them on their way to R; 40 swallowed ones anywhere, two of
        # them movers as well
        rng = np.random.default_rng(77)
        to_R = rng.choice(arrivals[R], 2, replace=False)
        rest = np.setdiff1d(np.where((now != R) & (then != R))[0], to_R)
        conv = np.concatenate([to_R, rng.choice(rest, 23, replace=False)])
        rng.shuffle(conv)                                        # (sinks and stars among the movers by chance)
        movers = np.setdiff1d(np.where(now != then)[0], conv)
        gone = rng.choice(movers, 2, replace=False)
        gone = np.sort(np.concatenate([gone, rng.choice(np.setdiff1d(np.arange(ng), np.concatenate([conv, gone])),
                                                        38, replace=False)]))
        gas = _mark(pr, conv, gone)
        conv = np.sort(conv)
        with _rule(rule, S.fp):
            S.set_field(B.F_TYPE, pr.ic["type"])
            S.set_field(B.F_MASS, pr.ic["mass"])
            S.set_field(B.F_DENSITY, np.full(ng, SENTINEL))
            assert mixed(R) == 0, "the receiving shard is to hold pure gas before the migration"
            assert not np.any(pr.ic["type"][S.gid[R][:S.ngas[R]]])
            S.set_field(B.F_POS, newpos)
            before = S.owner.copy()
            S.migrate()
            moved = S.owner != before
            print("changed owner: %d converted (%d to the pure shard %d), %d swallowed, %d in all" %
                  (moved[conv].sum(), (S.owner[to_R] == R).sum(), R, moved[gone].sum(), moved.sum()))
            assert np.array_equal(S.owner[:ng], then), "the shards moved the gas where the keys say"
            assert moved[conv].any() and moved[gone].any() and np.all(S.owner[to_R] == R)
            assert np.array_equal(np.sort(np.concatenate(S.gid)), np.arange(n)), "lost or doubled"
            assert np.array_equal(S.get_field(B.F_POS), newpos), "positions after migration"
            for i in conv[moved[conv]]:       # the arrival sits in the gas block of its new shard, with its Type
                r = S.owner[i]
                k = int(np.where(S.gid[r] == i)[0][0])
                assert k < S.ngas[r] and S.fp[r].get_field(B.F_TYPE)[k] == pr.ic["type"][i]
            pr.ic["pos"] = newpos
            od, oh = _oracle_step(pr, pr.oracle_tree(), gas, pr.hsml0, pr.dtentropy)
            _shard_step(pr, S)
            assert mixed(R) == 1, "the receiving shard did not look at the types of its arrivals"
            st = S.each(lambda fp: fp.stats())
            _check_density(S.get_field, st, od, gas, conv, full=True)
            _check_hydro(S.get_field, st, oh, gas, full=True)
    finally:
        S.close()


