"""ghip_rearrange and ghip_peano_order on the device against tests/sequence_ref.py: counts, both maps, every
field and every optional resident array bit for bit (tests/sequence_cases.py fills them from (ID, component)),
what a call invalidates and what it keeps, and the walks over the reordered state against a fresh context."""
import numpy as np
import pytest

import reuse_cases as RC
import sequence_cases as SC
import sequence_ref as R
from common import bindings

pytestmark = pytest.mark.gpu
B = bindings()
N, NGAS = SC.N, SC.NGAS
ALL = SC.OPTIONAL
GHIP_EINVAL = -90002


def _random_marks(seed, n=N, ngas=NGAS):
    rng = np.random.default_rng(seed)
    return (np.nonzero(rng.random(ngas) < 0.04)[0], np.nonzero(rng.random(n) < 0.05)[0])


def _cases():
    conv, zero = _random_marks(5)
    return {
        "converted at the ends": dict(converted=[0, NGAS - 1]),
        "massless at the ends": dict(massless=[0, NGAS - 1, NGAS, N - 1]),
        "massless run": dict(massless=range(900, 1200)),           # crosses the workgroups' and the scan's blocks
        "massless converted": dict(converted=[17, 1024], massless=[17]),
        "all gas eliminated": dict(massless=range(NGAS)),
        "no gas": dict(ngas=0, massless=[0, 5, N - 1]),
        "all gas": dict(ngas=N, converted=[0, 77, N - 1], massless=[1, N - 2]),
        "one survivor": dict(n=1, ngas=1),
        "one eliminated": dict(n=1, ngas=0, massless=[0]),
        "one converted": dict(n=1, ngas=1, converted=[0]),
        "nothing to do": dict(),
        "mixed": dict(converted=conv, massless=zero),
        "mixed, tied keys": dict(converted=conv, massless=zero, tied=True),
    }


CASES = _cases()
_MADE = {}


def _case(name):
    if name not in _MADE:
        _MADE[name] = SC.Case(**CASES[name])
    return _MADE[name]


def _rearranged(fp, case, opts, **switches):
    """rearrange() on the loaded context, checked against the specification -> (spec, ids afterwards)"""
    spec = R.spec_rearrange(case.type_of[case.ids], case.mass_of[case.ids], case.ngas, **switches)
    res = fp.rearrange(**switches).asdict()
    for k in ("numpart", "ngas", "converted", "count_elim", "count_gaselim", "count_dustelim", "changed"):
        assert res[k] == spec[k], (k, res, spec)
    assert (fp.n, fp.ngas) == fp.counts() == (spec["numpart"], spec["ngas"])
    new_of_old, old_of_new = fp.sequence_map()
    assert np.array_equal(new_of_old, spec["new_of_old"]) and np.array_equal(old_of_new, spec["old_of_new"])
    ids = case.ids[spec["old_of_new"]]
    SC.assert_same_bits(SC.read(fp, opts), SC.expected(case, ids, spec["ngas"], opts), "after rearrange:")
    return spec, ids


def _ordered(fp, case, ids, ngas, opts):
    """peano_order() on the context, checked against the specification -> ids afterwards"""
    order = R.spec_peano_order(case.key_of()[ids], ngas)
    changed = fp.peano_order(SC.CORNER, SC.DLEN)
    assert changed == (not np.array_equal(order, np.arange(len(ids))))
    new_of_old, old_of_new = fp.sequence_map()
    assert np.array_equal(old_of_new, order)
    inv = np.empty(len(ids), np.int32)
    inv[order] = np.arange(len(ids), dtype=np.int32)
    assert np.array_equal(new_of_old, inv)
    SC.assert_same_bits(SC.read(fp, opts), SC.expected(case, ids[order], ngas, opts), "after peano_order:")
    assert fp.peano_order(SC.CORNER, SC.DLEN) is False, "a second order moves nothing"
    assert fp.sequence_info()["bytes_moved"] == 0
    return ids[order]


@pytest.mark.parametrize("name", list(CASES))
def test_rearrange_then_order_equals_the_restatements(name):
    case = _case(name)
    fp = SC.load(B.ForcePath(0), case, opts=ALL)
    try:
        spec, ids = _rearranged(fp, case, ALL)
        ng = spec["ngas"]
        assert (fp.get_field(B.F_TYPE)[:ng] == 0).all() and fp.L.ghip_gas_block_mixed(fp.h) == 0
        assert (fp.get_field(B.F_MASS) != 0).all()
        ids = _ordered(fp, case, ids, ng, ALL)
        key = case.key_of()[ids]
        assert (np.diff(key[:ng].astype(np.int64)) >= 0).all() and (np.diff(key[ng:].astype(np.int64)) >= 0).all()
        lit = R.literal_sequence(case.type_of[case.ids], case.mass_of[case.ids], case.ngas, case.key_of()[case.ids])
        assert lit["NumPart"] == len(ids) and lit["N_gas"] == ng
        lit_ids = case.ids[np.array(lit["P"], np.int64)]
        if not CASES[name].get("tied"):
            assert len(np.unique(key)) == len(key), "the case is meant to have distinct keys"
            assert np.array_equal(ids, lit_ids), "the literal restatement, index for index"
            assert np.array_equal(case.ids[np.array(lit["SphP"], np.int64)], ids[:ng])
        else:
            # tied keys keep the compaction's order; the literal sequence holds the same records per key run
            rank = spec["new_of_old"]
            slot_of = np.empty(case.n, np.int64)
            slot_of[case.ids] = np.arange(case.n)
            for blk in (ids[:ng], ids[ng:]):
                same = np.diff(case.key_of()[blk].astype(np.int64)) == 0
                assert same.sum() > 100 and (np.diff(rank[slot_of[blk]])[same] > 0).all()
            assert np.array_equal(case.key_of()[lit_ids], key)
            assert sorted(zip(key.tolist(), lit_ids.tolist())) == sorted(zip(key.tolist(), ids.tolist()))
    finally:
        fp.close()


@pytest.mark.parametrize("opts", [(), ALL[0::2], ALL[1::2]], ids=["none", "even", "odd"])
def test_optional_arrays_present_and_absent(opts):
    """each optional array present in one run and absent in another (all of them present: the test above)"""
    case = _case("mixed")
    fp = SC.load(B.ForcePath(0), case, opts=opts)
    try:
        spec, ids = _rearranged(fp, case, opts)
        _ordered(fp, case, ids, spec["ngas"], opts)
        if "visc" not in opts:
            with pytest.raises(B.GhipError):
                fp.visc_get()
    finally:
        fp.close()


def test_an_array_held_for_other_counts_is_dropped():
    case = _case("mixed")
    fp = B.ForcePath(0)
    try:
        other = SC.Case(n=300, ngas=100)
        SC.load(fp, other, opts=("visc", "inj", "drag", "newdens"))     # arrays for 300 / 100
        SC.load(fp, case, opts=("ra",))                                  # the counts change: those are stale
        spec, ids = _rearranged(fp, case, ("ra",))
        with pytest.raises(B.GhipError):
            fp.visc_get()
        assert fp.kick_fields() == (None, None, None)
    finally:
        fp.close()


@pytest.mark.parametrize("switches", [dict(fix_converted=False), dict(eliminate_massless=False)],
                         ids=["massless only", "converted only"])
def test_each_switch_alone(switches):
    case = _case("mixed")
    fp = SC.load(B.ForcePath(0), case, opts=("heat", "sink"))
    try:
        spec, _ = _rearranged(fp, case, ("heat", "sink"), **switches)
        assert fp.L.ghip_gas_block_mixed(fp.h) == int("fix_converted" in switches)
    finally:
        fp.close()


def test_a_position_outside_the_cube_is_refused_and_nothing_moves():
    case = _case("mixed")
    fp = SC.load(B.ForcePath(0), case, opts=ALL)
    try:
        fp.rearrange()
        maps = fp.sequence_map()
        for bad in (1.0, -1e-9, np.nan, np.inf):
            pos = fp.get_field(B.F_POS)
            pos[fp.n - 3, 1] = bad
            fp.set_field(B.F_POS, pos)
            before = SC.read(fp, ALL)
            with pytest.raises(B.GhipError) as e:
                fp.peano_order(SC.CORNER, SC.DLEN)
            assert e.value.code == GHIP_EINVAL
            after = SC.read(fp, ALL)
            for k in before:
                assert np.ascontiguousarray(before[k]).tobytes() == np.ascontiguousarray(after[k]).tobytes(), k
            assert all(np.array_equal(a, b) for a, b in zip(maps, fp.sequence_map()))
        with pytest.raises(B.GhipError) as e:
            fp.peano_order(None)          # no decomposition: there is no domain to fall back on
        assert e.value.code == GHIP_EINVAL
        fp.set_shard(1, 2)
        for call in (fp.rearrange, lambda: fp.peano_order(SC.CORNER, SC.DLEN)):
            with pytest.raises(B.GhipError) as e:
                call()
            assert e.value.code == GHIP_EINVAL
    finally:
        fp.close()


def _walks(fp, pr, do_build):
    """gravity, density and hydro on the state in place -> results keyed as tests/reuse_cases.py:RULES"""
    if do_build:
        pr.device_tree(fp)
    fp.set_field(B.F_OLDACC, np.zeros(fp.n))
    fp.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
    out = dict(acc=fp.get_field(B.F_GRAVACCEL), cost=fp.get_field(B.F_GRAVCOST))
    if fp.ngas:
        fp.density(pr.g_dens())
        fp.update_hmax()
        fp.hydro(pr.g_hydro())
        st = fp.stats()
        out.update(density=fp.get_field(B.F_DENSITY), hsml=fp.get_field(B.F_HSML)[:fp.ngas],
                   numngb=fp.get_field(B.F_NUMNGB), dhsmlfac=fp.get_field(B.F_DHSMLFAC),
                   divvel=fp.get_field(B.F_DIVVEL), curlvel=fp.get_field(B.F_CURLVEL),
                   pressure=fp.get_field(B.F_PRESSURE), hydroaccel=fp.get_field(B.F_HYDROACCEL),
                   dtentropy=fp.get_field(B.F_DTENTROPY), maxsignalvel=fp.get_field(B.F_MAXSIGNALVEL),
                   pairs=st["hydro_pairs"], dens_iter=st["dens_iterations"])
    out["nodes"] = fp.stats()["tree_nodes"]
    return out


def test_changed_zero_keeps_tree_and_list_and_a_change_drops_them():
    case = _case("nothing to do")
    pr = case.problem(case.ids, case.ngas)
    fp = SC.load(B.ForcePath(0), case)
    try:
        pr.device_tree(fp)
        act = np.arange(0, case.n, 3, dtype=np.int32)
        fp.set_active(act)
        assert fp.rearrange().changed == 0
        assert np.array_equal(fp.get_active(), act)
        fp.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)          # no build: the tree is still there
        cost = fp.get_field(B.F_GRAVCOST)
        assert (cost[act] > 0).all()
        # ordered already: the second of two orders moves nothing and keeps both as well
        assert fp.peano_order(SC.CORNER, SC.DLEN) is True
        with pytest.raises(B.GhipError) as e:
            fp.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)      # a real change: refused until a build
        assert e.value.code == GHIP_EINVAL
        assert np.array_equal(fp.get_active(), np.arange(case.n)), "everybody is active after a change"
        ids = fp.get_field(B.F_ID).astype(np.int64)
        pr2 = case.problem(ids, case.ngas)
        pr2.device_tree(fp)
        fp.set_active(act)
        assert fp.peano_order(SC.CORNER, SC.DLEN) is False
        assert np.array_equal(fp.get_active(), act)
        fp.gravity(pr2.g_grav(pr2.theta), B.WALK_NEWTON)
        # a kept tree is refused after a change until a full build
        fp.set_dynamic_tree(True)
        pr2.device_tree(fp)
        fp.tree_substep(0.0)
        mass = fp.get_field(B.F_MASS)
        mass[5] = 0.0
        fp.set_field(B.F_MASS, mass)
        pr2.device_tree(fp)
        assert fp.rearrange().count_elim == 1
        with pytest.raises(B.GhipError):
            fp.tree_substep(0.0)
    finally:
        fp.close()


def test_walks_on_the_reordered_state_equal_a_fresh_context():
    case = _case("mixed")
    fp = SC.load(B.ForcePath(0), case, opts=ALL)
    fresh = B.ForcePath(0)
    try:
        fp.rearrange()
        fp.peano_order(SC.CORNER, SC.DLEN)
        lit = R.literal_sequence(case.type_of[case.ids], case.mass_of[case.ids], case.ngas, case.key_of()[case.ids])
        ids, ng = case.ids[np.array(lit["P"], np.int64)], lit["N_gas"]
        assert np.array_equal(fp.get_field(B.F_ID), ids)
        pr = case.problem(ids, ng)
        got = _walks(fp, pr, True)
        SC.load(fresh, case, ids=ids, ngas=ng)
        want = _walks(fresh, pr, True)
        assert (want["cost"] > 0).all() and (want["numngb"] > 0).all()
        bad = RC.compare(got, want, 1)
        assert not bad, bad
        assert np.array_equal(got["cost"], want["cost"]) and np.array_equal(got["numngb"], want["numngb"])
    finally:
        fp.close()
        fresh.close()
