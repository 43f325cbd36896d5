"""The oracle's sink passes (orc_sink_density, orc_blackhole_evaluate, orc_blackhole_swallow) against
tests/sink_ref.py -- blackhole.c and the BLACK_HOLES branches of density.c restated over all pairs -- on
the inputs of tests/common.py that reach what the stock SinkProblem never does: contested victims whose
IDs are not in list order, chains and mutual claims (a claimed sink swallows nothing, blackhole.c:528-532),
the central object's InnerBoundary for sinks, heavier sinks and unbound grains in range, a massless sink, a
sink in time bin 0, and every branch of the sinks' h iteration.  No GPU: this is the gate for
tests/test_gpu_sink.py, which holds the device to the same reference."""
import numpy as np
import pytest

from common import (SINK_CASES as CASES, SINK_HITER, SINK_PAIR_AT, SINK_SWITCHES, check_sink_passes,
                    oracle_sink_passes, sink_case, sink_reference)

# the seeds sink_case() takes: the first from 5 on without a candidate within 1e-9 of a decision threshold
SEEDS = {("clump", 0): 5, ("clump", 1): 5, ("pair", 1): 5, ("central", 1): 5,
         **{("hiter-" + v, 1): 5 for v in SINK_HITER}}
# what each variant of the h iteration was written to reach (sink_ref.sink_density reports the branches)
HITER_BRANCHES = dict(tight={"bisect", "exit1e-3"}, minh={"minh"}, clamp={"clamp", "minh"},
                      small={"grow", "bisect"}, large={"shrink", "bisect"}, void={"rho0", "grow", "bisect"})


@pytest.mark.parametrize("name,periodic,switches", CASES)
def test_oracle_equals_the_all_pairs_restatement(name, periodic, switches):
    sp = sink_case(name, periodic)
    assert sp.seed == SEEDS[(name, periodic)]
    ref = sink_reference(name, periodic, *switches)
    dens, marks, swallowed, mass = oracle_sink_passes(sp, ref["over"])
    err = check_sink_passes(sp, ref, dens, marks, swallowed, mass)
    print(name, periodic, switches, err)
    # by definition (blackhole.c:528-532): swallowed = marked by a sink of the list that is itself unmarked
    sw, rs = ref["sw"], ref["swallow"]
    free = sp.ids[sp.sinks][sw[sp.sinks] == 0]
    assert np.array_equal(rs["swallowed"], np.isin(sw, free) & (sw > 0))
    assert rs["counts"].sum() == rs["swallowed"].sum()
    assert np.all(rs["mass"][rs["swallowed"]] == 0)
    assert np.array_equal(rs["mass"][~rs["swallowed"]], sp.pr.ic["mass"][~rs["swallowed"]])


@pytest.mark.parametrize("variant", SINK_HITER)
def test_h_iteration_inputs_reach_their_branches(variant):
    sp = sink_case("hiter-" + variant, 1)
    taken = set().union(*sp.dens["branches"])
    assert HITER_BRANCHES[variant] <= taken, (variant, sp.dens["branches"])
    pr, d = sp.pr, sp.dens
    if variant == "tight":      # every sink leaves by the 1e-3 rule, none inside the (1e-9) window
        assert all("exit1e-3" in b for b in d["branches"]) and d["iterations"] >= 10
        assert np.abs(d["numngb"] - 1.5 * pr.des_ngb).min() > 1e-6
    if variant in ("minh", "clamp"):
        at = np.array(["minh" in b for b in d["branches"]])
        assert 2 <= at.sum() < len(sp.sinks)                        # some sinks, not all
        assert np.all(d["hsml"][sp.sinks][at] <= 1.01 * pr.min_gas_hsml)
        assert np.all(d["numngb"][at] > 1.5 * pr.des_ngb + pr.max_dev)      # accepted with too many
    if variant == "clamp":
        assert (d["hsml"][sp.sinks] == pr.min_gas_hsml).sum() >= 2  # exactly AT the clamp
    if variant == "void":
        assert "rho0" in d["branches"][3] and d["density"][3] > 0   # empty first, gas at convergence


@pytest.mark.parametrize("periodic", [0, 1])
@pytest.mark.parametrize("switches", SINK_SWITCHES)
def test_clump_tells_the_claim_rules_apart(periodic, switches):
    """On the reference alone: the input contests victims between sinks whose IDs are not in list order, so
    "largest ID wins" (the project's rule, an atomicMax on the device), "last writer wins" and "first writer
    wins" give different marks.  This is what proves that the comparison of marks in the tests can see a plain
    store in place of the atomicMax; on the device such a store is a race and may or may not lose on a given
    run."""
    sp = sink_case("clump", periodic)
    ref = sink_reference("clump", periodic, *switches)
    sw, sk = ref["sw"], sp.sinks
    wanted = np.zeros(sp.pr.n, int)
    for c in ref["claims"]:
        wanted[c["victims"]] += 1
    contested = wanted > 1
    assert contested.sum() >= 10
    assert (contested & (sw != ref["last"])).sum() >= 5
    assert (contested & (sw != ref["first"])).sum() >= 5
    assert np.array_equal(sw[~contested], ref["last"][~contested])
    own = np.array([(sw == sp.ids[i]).sum() for i in sk])
    assert ((sw[sk] > 0) & (own > 0)).sum() >= 3                    # claimed sinks that hold victims
    assert sum(len(c["refused_unbound"]) for c in ref["claims"]) >= 1
    assert sum(len(c["refused_heavier"]) for c in ref["claims"]) >= 1
    # the ingredients: a massless sink and a sink in time bin 0 in the list, 9 of the 10 massive clump sinks
    # claimed (all but the heaviest), a chain C -> B -> A among them
    mass = sp.pr.ic["mass"]
    assert (mass[sk] == 0).sum() == 1 and (sp.pr.timebin[sk] == 0).sum() == 1
    assert (sw[sk] > 0).sum() == 9
    idx_of = {int(sp.ids[i]): a for a, i in enumerate(sk)}
    chain = [a for a in range(len(sk)) if sw[sk[a]] > 0 and sw[sk[idx_of[int(sw[sk[a]])]]] > 0]
    assert len(chain) >= 1                                          # A claimed by B, B claimed by C
    # what the fix is about: the victims of claimed sinks keep their mass
    rs = ref["swallow"]
    kept = (sw > 0) & ~rs["swallowed"]
    assert kept.sum() >= 3 and np.array_equal(rs["mass"][kept], mass[kept])


@pytest.mark.parametrize("how", [{}, dict(at=SINK_PAIR_AT)], ids=["stock", "placed"])
@pytest.mark.parametrize("switches", SINK_SWITCHES)
def test_pair_is_a_mutual_claim_and_nobody_swallows(switches, how):
    sp = sink_case("pair", 1, **how)
    assert sp.seed == 5
    ref = sink_reference("pair", 1, *switches, **how)
    sw, (a, b) = ref["sw"], sp.sinks
    assert sw[a] == sp.ids[b] and sw[b] == sp.ids[a]                 # each claims the other
    typ = sp.pr.ic["type"]
    for i in (a, b):                                                 # each with victims of its own in reach
        mine = np.where(sw == sp.ids[i])[0]
        assert (typ[mine] == 2).sum() >= 1
        assert switches[0] == 1 or (typ[mine] == 0).sum() >= 1
    rs = ref["swallow"]
    assert rs["skipped"].all() and not rs["counts"].any() and not rs["swallowed"].any()
    assert np.array_equal(rs["mass"], sp.pr.ic["mass"])
    dens, marks, swallowed, mass = oracle_sink_passes(sp, ref["over"])
    assert not swallowed["counts"].any() and np.array_equal(mass, sp.pr.ic["mass"])
    assert np.array_equal(swallowed["bh_mass"], sp.bh_mass[sp.sinks])


@pytest.mark.parametrize("switches", SINK_SWITCHES)
def test_central_object_merges_sinks_inside_inner_boundary_only(switches):
    sp = sink_case("central", 1)
    ref = sink_reference("central", 1, *switches)
    pr = sp.pr
    c, near, far = sp.sinks
    d = pr.ic["pos"][c] - pr.ic["pos"][[near, far]]
    d -= pr.box * np.round(d / pr.box)
    r = np.sqrt((d * d).sum(axis=1))
    h = sp.dens["hsml"][c]
    par = ref["par"]
    assert r[0] < par.InnerBoundary < r[1] < min(h, par.SofteningBndry)     # the far one IS a neighbour
    sw = ref["sw"]
    assert sw[near] == sp.ids[c] and sw[far] != sp.ids[c]
    gas = (sw == sp.ids[c]) & (pr.ic["type"] == 0)
    assert gas.sum() >= 5                                           # gas inside InnerBoundary: no switch needed
