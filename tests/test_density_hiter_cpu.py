"""The gas side of density() -- the smoothing-length rule of density.c:434-652 with its Newton step -- on inputs
that send the targets down every branch of it, judged on the CPU: tests/density_ref.py (all pairs, long-double
sums, branch labels) against the oracle's T.density, and the inputs of density_ref.hiter_case against the
conditions under which a comparison with the device means something (every label carried, no comparison of any
target within 1e-10 of its threshold).  No GPU: this is the gate for tests/test_gpu_density_hiter.py, which holds
k_density and k_dens_finalize to the same reference.

Measured, reference against oracle, worst over all cases and targets (relative; div v and curl v of the largest):
hsml 6.6e-16, numngb 1.3e-15, density 3.0e-15, dhsmlfac 1.2e-14, divvel 1.4e-15, curlvel 1.6e-15, pressure
4.1e-15 -- the oracle's fp64 sums in tree order against long-double sums; iteration and visit counts equal."""
import numpy as np
import pytest

import density_ref as D
from common import O

TOL = 1e-11
# the seeds hiter_case() takes: the first from 12345 on that converge and keep every comparison MARGIN away
SEEDS = {(name, p): 12345 for name in D.CASES for p in (0, 1)}
# what each input was written to reach
REACHES = dict(base={"accept", "few", "many-first", "many-lower", "bisect", "shrink-newton", "shrink-far"},
               tight={"exit1e-3", "bisect"}, minh={"minh"}, clamp={"clamp", "minh"},
               small={"grow-far", "grow-capped", "grow-newton", "dhf-guard"},
               large={"shrink-far", "shrink-newton", "many-lower"},
               mixed={"grow-far", "grow-capped", "grow-newton", "shrink-far", "shrink-newton", "bisect"},
               massless={"rho0", "grow-far", "dhf-guard", "shrink-capped"},
               subset={"grow-far", "shrink-far", "bisect"})
ALL = [(name, p) for p in (0, 1) for name in D.CASES]


def _targets(pr):
    return np.arange(pr.ngas) if pr.active is None else np.asarray(pr.active)


def field_errors(got, ref, tg):
    """per field the worst error of `got` against the reference over the targets tg and where it is: relative per
    target, div v and curl v (which pass through 0) relative to the largest of the targets"""
    err = {}
    for k in D.FIELDS:
        r, g = ref[k][tg], np.asarray(got[k])[tg]
        scale = np.abs(r).max() if k in ("divvel", "curlvel") else np.maximum(np.abs(r), 1e-300)
        e = np.abs(g - r) / scale
        err[k] = (float(e.max()), int(tg[int(np.argmax(e))]))
    return err


def worst_message(pr, err):
    k = max(err, key=lambda f: err[f][0])
    i = err[k][1]
    return "%s periodic %d: %s of target %d off by %.3g; branches %s, h tried %s" % (
        pr.case, pr.periodic, k, i, err[k][0], sorted(pr.ref["branches"][i]), pr.ref["h_tried"][i])


@pytest.mark.parametrize("name,periodic", ALL)
def test_reference_equals_the_oracle(name, periodic):
    pr = D.hiter_case(name, periodic)
    assert pr.seed == SEEDS[(name, periodic)]
    ref, tg = pr.ref, _targets(pr)
    O.set_massless_gas_rule(pr.rule)
    try:
        T = pr.oracle_tree(hsml=pr.hsml0)
        od = T.density(pr.o_dens(), tg.astype(np.int32), pr.velpred, pr.entropy, pr.dtentropy, pr.timebin,
                       pr.ti_begstep, pr.hsml0)
    finally:
        O.set_massless_gas_rule(0)
    assert od["iterations"] == ref["iterations"] >= 1
    assert od["ngb_visits"] == ref["visits"]
    err = field_errors(od, ref, tg)
    print(name, periodic, {k: "%.1e" % v[0] for k, v in err.items()})
    assert max(v[0] for v in err.values()) < TOL, worst_message(pr, err)
    off = np.setdiff1d(np.arange(pr.n), tg)
    assert np.array_equal(od["hsml"][off], pr.hsml0[off])


@pytest.mark.parametrize("name,periodic", ALL)
def test_inputs_keep_their_distance_and_reach_their_branches(name, periodic):
    pr = D.hiter_case(name, periodic)
    ref, tg = pr.ref, _targets(pr)
    assert ref["margin"][tg].min() >= D.MARGIN
    assert np.all(ref["passes"][tg] >= 1) and not ref["passes"][np.setdiff1d(np.arange(pr.n), tg)].any()
    taken = set().union(*[ref["branches"][i] for i in tg])
    assert REACHES[name] <= taken, (name, sorted(REACHES[name] - taken))
    ng = pr.ngas
    if name == "tight":     # whoever bisects leaves by the 1e-3 rule; the others were brought inside by Newton steps
        out = np.array(["exit1e-3" in ref["branches"][i] for i in tg])
        assert out.sum() >= 100 and np.all(np.abs(ref["numngb"][tg][out] - pr.des_ngb) > pr.max_dev)
        assert np.all(np.abs(ref["numngb"][tg][~out] - pr.des_ngb) <= pr.max_dev)
    if name in ("minh", "clamp"):
        at = np.array(["minh" in ref["branches"][i] for i in tg])
        assert 8 <= at.sum() <= ng - 8
        assert np.all(ref["hsml"][tg][at] <= 1.01 * pr.min_gas_hsml)
        assert np.all(ref["numngb"][tg][at] > pr.des_ngb + pr.max_dev)
    if name == "minh" and periodic:
        # accepted strictly between MinGasHsml and 1.01 MinGasHsml: what tells `1.01 *` from its absence (in the open
        # box and under `clamp` every such target was reset to MinGasHsml itself first)
        assert (ref["hsml"][tg][at] > pr.min_gas_hsml).sum() >= 8
    if name == "clamp":
        assert (ref["hsml"][:ng] == pr.min_gas_hsml).sum() >= 8 and ref["hsml"][:ng].min() == pr.min_gas_hsml
    if name == "large":     # the long side of the candidate staging: about 27 x 33 neighbours in the first pass
        first = D._sums(pr.ic["pos"][:ng], pr.velpred, pr.hsml0[:ng], pr.ic["pos"][:ng], pr.velpred,
                        pr.ic["mass"][:ng], pr.box, pr.periodic, 0)[1]
        assert first.max() == ng if periodic else first.mean() > 300
    if name == "massless":
        assert np.all(pr.ic["mass"][pr.massless] == 0)
        for i in pr.massless:   # alone inside the first h: rho = 0, numngb = the target's own weight
            assert "rho0" in ref["branches"][i] and "grow-far" in ref["branches"][i]
            assert ref["density"][i] > 0 and ref["passes"][i] >= 3
        for i in pr.heavy:      # the guard in the accepted pass: DhsmlDensityFactor comes out as 1
            assert "dhf-guard" in ref["branches"][i] and ref["dhsmlfac"][i] == 1.0
    if name == "subset":
        assert len(tg) == 150 and ref["iterations"] >= 8


def test_every_label_is_carried():
    count = D.carriers([D.hiter_case(name, p).ref for name, p in ALL])
    print(count)
    for label in D.LABELS:
        if label in D.UNREACHABLE:
            # no terminating input takes it (density_ref's module text has the argument); were one of the cases to
            # carry it after all, that would be news
            assert count[label] == 0, label
        else:
            assert count[label] >= (3 if label in ("dhf-guard", "rho0") else 8), (label, count[label])
