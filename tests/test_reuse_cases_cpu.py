"""The table of tests/reuse_cases.py, checked without a GPU: every transition a long-lived context must survive
is in it (a removed stage fails here, not silently on the device), the sequences keep their size, and the
oracle alone, run over every stage, finds the preconditions each stage was chosen for -- the h iteration
converges, the node count of the overflow stage exceeds what the build before it left room for, the
problems meant to have no gas, two particles, nobody, cells at the box edge or coincident particles have them."""
import numpy as np
import pytest

import reuse_cases as RC

NAMES = list(RC.SEQUENCES)


def _nodes(seq):
    return [RC.oracle_stage(s)["nodes"] for s in seq]


def test_every_transition_is_in_the_table():
    found = set()
    for name in NAMES:
        seq = RC.SEQUENCES[name]
        t = RC.transitions(seq, _nodes(seq))
        print(name, sorted(t))
        found |= t
    missing = [r for r in RC.REQUIRED if r not in found]
    assert not missing, "no sequence contains: %s" % missing
    assert found <= set(RC.REQUIRED)


def test_a_table_without_a_stage_misses_its_transition():
    """the check above is not vacuous: take a stage away and the transition it stands for is reported missing"""
    for name, drop, gone in (("counts", "nobody", "n -> 0 -> n"), ("gas", "marked, rule 3",
                                                                  "massless rule 0 -> 1 -> 3 -> 0 with marked records"),
                             ("builds", "smooth", "same n, more nodes than the slack"),
                             ("walks", "more walks", "every walk kind after every other"),
                             ("mesh", "open mesh", "periodic mesh -> open mesh -> periodic mesh")):
        seq = RC.SEQUENCES[name]
        assert gone in RC.transitions(seq, _nodes(seq)), (name, gone)
        less = [s for s in seq if s.name != drop]
        assert len(less) == len(seq) - 1
        assert gone not in RC.transitions(less, _nodes(less)), (name, gone)


@pytest.mark.parametrize("name", NAMES)
def test_sequences_keep_their_size(name):
    seq = RC.SEQUENCES[name]
    assert 2 <= len(seq) <= RC.MAX_STAGES
    assert len({s.name for s in seq}) == len(seq)
    for s in seq:
        assert s.pr.n <= RC.MAX_N, s.name
        assert not s.sph() or s.pr.ngas >= 40, s.name       # (gpu_fuzz.one: SPH passes from 40 gas particles on)
        # the first walk of a list of targets is not a bare Ewald correction
        first = {}
        tg = 0
        for p in s.passes:
            if p[0] in ("active", "everybody"):
                tg += 1
            if p[0] == "gravity":
                first.setdefault(tg, p[1])
        assert "ewald" not in first.values(), s.name


def test_the_overflow_stage_outgrows_the_slack_of_the_build_before_it():
    """ghip_tree.hip sizes the element buffers of a first build for nnodes + nnodes / d + c nodes; a later build of
    the same particle number does not wait for its count.  The second problem needs more than that, so the
    asynchronous build fails on the device and is repeated, with the gravity call made in between replayed."""
    d, c = RC.tree_slack()
    assert d >= 1 and c >= 0
    a, b = RC.SEQUENCES["builds"][:2]
    assert (a.pr.n, a.pr.ngas) == (b.pr.n, b.pr.ngas)
    na, nb = RC.oracle_stage(a)["nodes"], RC.oracle_stage(b)["nodes"]
    print("nodes %d -> %d, room for %d" % (na, nb, na + na // d + c))
    assert nb > na + na // d + c
    assert b.passes[0][0] == "gravity"           # (the replay log is not empty when the count is verified)


@pytest.mark.parametrize("name", NAMES)
def test_the_oracle_alone_meets_every_stage_s_preconditions(name):
    for s in RC.SEQUENCES[name]:
        ref = RC.oracle_stage(s)
        pr = s.pr
        if s.sph():
            assert ref["dens_iter"] >= 1, "%s: the h iteration did not converge" % s.name
            assert np.all(np.isfinite(ref["density"])) and (ref["density"] > 0).all(), s.name
        if "pairs" in ref:
            assert ref["pairs"] > 0, s.name
        for k, v in ref.items():
            if k.startswith("acc") or k in ("hydroaccel", "gravpm"):
                assert np.all(np.isfinite(v)), (s.name, k)
                assert pr.n < 2 or np.abs(v).max() > 0, (s.name, k)
        if pr.n:
            assert ref["nodes"] >= 1
        if s.switches["rule"]:
            assert RC._mixed(s) and RC._massless(s), s.name


def test_the_targeted_edges_occur():
    S = {n: {s.name: s for s in RC.SEQUENCES[n]} for n in NAMES}
    assert S["counts"]["nobody"].pr.n == 0
    assert S["counts"]["two particles"].pr.n == 2
    assert S["gas"]["no gas"].pr.ngas == 0 and S["gas"]["no gas"].pr.n > 0
    # a run of keys too long for the 32-bit sort, and none in the problem after it
    assert RC.clumps_run(S["builds"]["clumps"]) > 32
    assert RC.clumps_run(S["builds"]["ordinary after clumps"]) <= 32
    assert S["builds"]["clumps"].pr.n == S["builds"]["ordinary after clumps"].pr.n
    assert RC.coincidences(S["builds"]["coincident, table bound"]) > 20
    assert RC.coincidences(S["builds"]["ordinary, table gone"]) == 0
    # cells at the box edge: coordinates equal to BoxSize, in the last cell and at the origin
    edge = S["mesh"]["cells at the box edge"].pr
    assert (edge.ic["pos"] == edge.box).any() and (edge.ic["pos"] == 0.0).any()
    assert ((edge.ic["pos"] > edge.box * 7 / 8) & (edge.ic["pos"] < edge.box)).any()
    # a partial list that is one: neither nobody nor everybody
    st = S["softening"]["adaptive off, a partial list"]
    k = len(RC._active(st, *[p for p in st.passes if p[0] == "active"][0][1:]))
    assert 0 < k < st.pr.n
    # the box sizes of the Ewald and potential tables
    assert [s.pr.box for s in RC.SEQUENCES["geometry"][:3]] == [1.0, 2.5, 1.0]
    # the marked problems have both kinds of record, the pure one after them neither
    for nm in ("marked, rule 1", "marked, rule 3", "marked, rule 0"):
        assert RC._mixed(S["gas"][nm]) and RC._massless(S["gas"][nm])
    assert not RC._mixed(S["gas"]["pure"]) and not RC._massless(S["gas"]["pure"])
