"""The two restatements of tests/sequence_ref.py against each other: the literal, serial rearrange_particle_sequence
+ peano_hilbert_order and the specification of ghip_rearrange + ghip_peano_order (stable compaction, stable sort)
give the same sequence wherever keys are distinct, the same multiset inside every run of equal keys, and always
the same counts.  No GPU."""
import numpy as np
import pytest

import sequence_ref as R


def _state(n, ngas, seed, p_conv=0.05, p_massless=0.05, ties=False):
    rng = np.random.default_rng(seed)
    ptype = np.zeros(n, np.int32)
    ptype[ngas:] = rng.integers(1, 6, n - ngas)
    conv = rng.random(ngas) < p_conv
    ptype[:ngas][conv] = rng.choice([4, 5], int(conv.sum()))
    mass = 1.0 + rng.random(n)
    mass[rng.random(n) < p_massless] = 0.0
    key = rng.integers(0, 40, n).astype(np.uint64) if ties else rng.permutation(n).astype(np.uint64) * 7919
    return ptype, mass, key


def _check(ptype, mass, ngas, key):
    lit = R.literal_sequence(ptype, mass, ngas, key)
    spec, order = R.spec_sequence(ptype, mass, ngas, key)
    for k in ("count_elim", "count_gaselim", "count_dustelim"):
        assert lit[k] == spec[k], k
    assert lit["NumPart"] == spec["numpart"] == len(order) and lit["N_gas"] == spec["ngas"]
    assert lit["flag"] == spec["changed"]
    P, S, ng = np.array(lit["P"], np.int64), np.array(lit["SphP"], np.int64), spec["ngas"]
    assert np.array_equal(P[:ng], S), "SphP[i] belongs to P[i] throughout the gas block"
    assert (ptype[P[:ng]] == 0).all() and (mass[P] != 0).all()
    ko = key[order]
    assert np.array_equal(key[P], ko), "the keys of the two sequences, slot for slot"
    assert (np.diff(ko[:ng].astype(np.int64)) >= 0).all() and (np.diff(ko[ng:].astype(np.int64)) >= 0).all()
    for lo, hi in ((0, ng), (ng, len(order))):
        k = ko[lo:hi]
        starts = np.r_[0, np.nonzero(np.diff(k.astype(np.int64)))[0] + 1, hi - lo] + lo
        for a, b in zip(starts[:-1], starts[1:]):
            assert sorted(P[a:b]) == sorted(order[a:b]), "the records of one key run"
    return P, order


@pytest.mark.parametrize("seed", range(6))
def test_distinct_keys_index_for_index(seed):
    n, ngas = 700 + 13 * seed, 300 + 7 * seed
    ptype, mass, key = _state(n, ngas, seed)
    P, order = _check(ptype, mass, ngas, key)
    assert np.array_equal(P, order)


@pytest.mark.parametrize("seed", range(4))
def test_tied_keys_equal_per_key_run_and_the_specification_keeps_the_old_order(seed):
    ptype, mass, key = _state(900, 400, 100 + seed, ties=True)
    _, order = _check(ptype, mass, 400, key)
    ng = R.spec_rearrange(ptype, mass, 400)["ngas"]
    for blk in (order[:ng], order[ng:]):
        same = np.diff(key[blk].astype(np.int64)) == 0
        # inside a key run the compaction's order survives: gas by old index; behind it converted before others
        rank = R.spec_rearrange(ptype, mass, 400)["new_of_old"][blk]
        assert (np.diff(rank)[same] > 0).all()


def _edge(n, ngas):
    ptype = np.zeros(n, np.int32)
    ptype[ngas:] = 1 + np.arange(n - ngas) % 5
    return ptype, 1.0 + np.arange(n) / n, (np.arange(n)[::-1] * 3 + 1).astype(np.uint64)


def test_edge_inputs():
    n, ngas = 257, 120
    cases = {}
    for name, conv, zero in (("converted at 0", [0], []), ("converted at ngas-1", [ngas - 1], []),
                             ("massless at 0", [], [0]), ("massless at ngas-1", [], [ngas - 1]),
                             ("massless at ngas", [], [ngas]), ("massless at n-1", [], [n - 1]),
                             ("massless run", [], list(range(60, 200))), ("massless converted", [17], [17]),
                             ("converted neighbours", [ngas - 2, ngas - 1], [ngas - 1]),
                             ("all gas eliminated", [], list(range(ngas))), ("nothing", [], []),
                             ("everything eliminated", [], list(range(n)))):
        ptype, mass, key = _edge(n, ngas)
        ptype[conv] = 4
        mass[zero] = 0
        cases[name] = (ptype, mass, ngas, key)
    for nn, gg in ((64, 0), (64, 64), (1, 0), (1, 1), (0, 0)):
        cases["n=%d ngas=%d" % (nn, gg)] = _edge(nn, gg)[:2] + (gg, _edge(nn, gg)[2])
    ptype, mass, key = _edge(5, 5)
    mass[:] = 0
    cases["five massless gas"] = (ptype, mass, 5, key)
    for name, (ptype, mass, gg, key) in cases.items():
        P, order = _check(ptype, mass, gg, key)
        assert np.array_equal(P, order), name
    spec = R.spec_rearrange(*cases["nothing"][:3])
    assert spec["changed"] == 0 and np.array_equal(spec["old_of_new"], np.arange(n))
    spec = R.spec_rearrange(*cases["massless converted"][:3])
    assert (spec["converted"], spec["count_elim"], spec["count_gaselim"], spec["ngas"]) == (0, 1, 0, ngas - 1)


def test_the_switches_of_the_specification():
    ptype, mass, _ = _state(500, 200, 9)
    a = R.spec_rearrange(ptype, mass, 200, fix_converted=False)
    assert a["converted"] == 0 and a["ngas"] == int((mass[:200] != 0).sum())
    b = R.spec_rearrange(ptype, mass, 200, eliminate_massless=False)
    assert b["count_elim"] == 0 and b["numpart"] == 500 and b["ngas"] == int((ptype[:200] == 0).sum())
    lit = R.literal_rearrange(ptype, mass, 200, black_holes=False)
    assert lit["N_gas"] == b["ngas"] and sorted(lit["P"][:lit["N_gas"]]) == sorted(b["old_of_new"][:b["ngas"]])
