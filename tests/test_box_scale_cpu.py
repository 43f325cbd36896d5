"""The references follow the scaling law of tests/scale_cases.py (no GPU needed): the oracle and the all-pairs numpy
restatements, run in a box of size L on the rescaled problem, give LAW applied to what they give in the unit box.
Only then can tests/test_gpu_box_scale.py hold the device to them in such boxes.

For L a power of two the oracle's gravity (walks, Ewald add, short-range walk, mesh) is bit-identical; everything
else, and every pass at L = 2.5, holds to RTOL = 1e-13 of the field's largest magnitude -- a dozen times the 7.5e-15
measured for the oracle's SPH passes, while a dropped factor of L is an error of order 1.  Counts are equal."""
import numpy as np
import pytest

import scale_cases as SC
from scale_cases import LAW, ODD, POW2, SCALES, SHIFT, off_law, rescaled

RTOL = 1e-13
GRAVITY = ("acc_bh", "acc_rel", "acc_ew_bh", "acc_ew_rel", "old_bh", "old_rel", "acc_sr", "gravpm")


def test_rescaled_is_the_map_of_the_law():
    from common import ics
    ic = ics.make_ics(4, gas=True, seed=3)
    for L in SCALES:
        s = rescaled(ic, L)
        assert s["boxsize"] == L and s["spacing"] == ic["spacing"] * L
        assert np.array_equal(s["mass"], ic["mass"] * L ** 3) and np.array_equal(s["vel"], ic["vel"] * L)
        assert np.all((s["pos"] >= 0) & (s["pos"] < L))
        assert np.array_equal(s["type"], ic["type"]) and np.array_equal(s["id"], ic["id"])
        o = rescaled(ic, L, SHIFT(L))
        assert np.array_equal(o["pos"], ic["pos"] * L + SHIFT(L)) and (o["pos"] < 0).any()
    assert ic["boxsize"] == 1.0 and ic["pos"].max() < 1.0          # the unit set is left alone
    # a coordinate that rounds to the box size goes to 0
    edge = dict(ic, pos=np.array([[1.0, 0.5, 0.25]]), vel=np.zeros((1, 3)), mass=np.ones(1))
    assert np.array_equal(rescaled(edge, ODD)["pos"], [[0.0, 1.25, 0.625]])
    assert set(LAW.values()) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("periodic", [1, 0])
@pytest.mark.parametrize("L", SCALES)
def test_oracle_follows_the_law(periodic, L):
    """(the open problem is scaled about the origin here: SHIFT is a translation, which changes the rounding of every
    coordinate and belongs to the parity tests on the device)"""
    unit = SC.oracle_cached(periodic, 1.0)
    got = SC.oracle_cached(periodic, L)
    assert set(got) == set(unit)
    assert ("acc_ew_rel" in got and "acc_sr" in got and "gravpm" in got) == bool(periodic)
    worst = {}
    for key, (name, u) in unit.items():
        g = got[key][1]
        if SC.is_count(u):
            assert LAW[name] == 0 and np.array_equal(g, u), key
            continue
        e = off_law(g, u, name, L)
        worst[key] = e
        exact = key in GRAVITY and L in POW2
        assert e == 0.0 if exact else e < RTOL, (key, e)
    print("L = %g periodic %d: worst %s" % (L, periodic, max(worst.items(), key=lambda kv: kv[1])))
    assert unit["cost_sr" if periodic else "cost_bh"][1].max() < SC.unit_problem(periodic).n


# ------------------------------------------------------------------------------------------------
# the case builders: the unit box is what it was
# ------------------------------------------------------------------------------------------------
def test_case_builders_make_the_same_unit_box_with_and_without_the_argument():
    """SinkProblem, DustCase, WindCase and fof_cases.clumps called as every earlier test calls them, and with
    box=1.0 passed: byte for byte the same members.  (Against the builders of the commit before they took the
    argument the digests were compared once by hand: equal.)"""
    import fof_cases as FC
    from common import SinkProblem
    from test_gpu_dust import DustCase
    from test_gpu_wind import WindCase
    for make in (lambda **k: SinkProblem(ng=8, **k), lambda **k: SinkProblem(ng=8, periodic=0, nsink=8, **k),
                 lambda **k: DustCase(1, ndust=200, ng=8, **k), lambda **k: WindCase(0, nwind=100, ng=8, **k),
                 lambda **k: WindCase(1, nwind=100, ng=8, **k), lambda **k: FC.clumps(777, True, **k)):
        assert SC.digest(make()) == SC.digest(make(box=1.0))
    assert SC.digest(SinkProblem(ng=8)) != SC.digest(SinkProblem(ng=8, box=2.0))
    # and what the argument scales
    a, b = WindCase(1, nwind=100, ng=8), WindCase(1, nwind=100, ng=8, box=4.0)
    for k in ("OuterBoundary", "SofteningGas", "SofteningGasMaxPhys", "SofteningBulgeMaxPhys", "PhotonSearchRadius"):
        assert b.par[k] == 4.0 * a.par[k], k
    assert b.par["OriginalGasMass"] == 64.0 * a.par["OriginalGasMass"] and b.par["FeedBackVelocity"] == 0.25
    assert np.array_equal(b.pr.ic["pos"], 4.0 * a.pr.ic["pos"]) and np.array_equal(b.pr.ic["vel"], 4.0 * a.pr.ic["vel"])
    assert np.array_equal(b.hsml, 4.0 * a.hsml) and np.array_equal(b.mass, 64.0 * a.mass)
    s1, s4 = SinkProblem(ng=8), SinkProblem(ng=8, box=4.0)
    for k in ("InnerBoundary", "SinkBoundary", "SofteningBndry", "BoxSize"):
        assert s4.par[k] == 4.0 * s1.par[k], k
    assert s4.par["SMBHmass"] == 64.0 * s1.par["SMBHmass"] and np.array_equal(s4.hsml, 4.0 * s1.hsml)


# ------------------------------------------------------------------------------------------------
# the all-pairs numpy references
# ------------------------------------------------------------------------------------------------
def _held(got, unit, name, L, what):
    e = off_law(got, unit, name, L)
    assert e < RTOL, (what, L, e)
    return e


@pytest.mark.parametrize("L", SCALES)
def test_sink_ref_follows_the_law(L):
    """sink_ref: the density pass of the sinks, the marks and the swallow pass.  The injected energy is left out: it
    carries FeedbackCoeff and UnitMass_in_g, physical constants that no rescaling of the box touches."""
    u, s = SC.sink_setup(1.0), SC.sink_setup(L)
    assert np.array_equal(u.sinks, s.sinks) and np.array_equal(u.ids, s.ids)
    du, ds = u.dens, s.dens
    assert ds["iterations"] == du["iterations"] and np.array_equal(ds["passes"], du["passes"])
    assert [sorted(b) for b in ds["branches"]] == [sorted(b) for b in du["branches"]]
    _held(ds["hsml"][s.sinks], du["hsml"][u.sinks], "hsml", L, "hsml")
    for k, name in (("numngb", "numngb"), ("density", "density"), ("entropy", "entropy"), ("gasvel", "gasvel")):
        _held(ds[k], du[k], name, L, k)
    for sw in SC.SINK_SWITCHES:
        ru, rs = SC.sink_refs(1.0, 1, sw), SC.sink_refs(L, 1, sw)
        assert np.array_equal(rs["sw"], ru["sw"]) and (ru["sw"] > 0).sum() >= 5, sw
        a, b = rs["swallow"], ru["swallow"]
        assert np.array_equal(a["counts"], b["counts"]) and b["counts"].sum() >= 3, (sw, b["counts"])
        assert np.array_equal(a["swallowed"], b["swallowed"]) and np.array_equal(a["skipped"], b["skipped"])
        for k in ("acc_mass", "acc_bhmass", "acc_dustmass", "mass", "bh_mass"):
            _held(a[k], b[k], "mass", L, k)
        _held(a["acc_momentum"], b["acc_momentum"], "momentum", L, "acc_momentum")
    # the sink by the face takes victims from across it
    from common import _sink_dist
    near = u.sinks[1]
    across = np.abs(u.pr.ic["pos"][:, 0] - u.pr.ic["pos"][near, 0]) > 0.5
    inside = (_sink_dist(u, near) < du["hsml"][near]) & (u.pr.ic["type"] == 0)
    assert (across & inside).sum() >= 5 and (~across & inside).sum() >= 5


@pytest.mark.parametrize("periodic", [1, 0])
@pytest.mark.parametrize("L", SCALES)
def test_dust_ref_density_follows_the_law(periodic, L):
    """dust_ref.dust_density only: the drag carries UnitLength_in_cm and the other cgs units of dust_ref.params,
    which break the law, so its grain and gas passes are not held to it."""
    from test_gpu_dust import DustCase
    u, s = DustCase(periodic, ndust=200, ng=8), DustCase(periodic, ndust=200, ng=8, box=L)
    assert np.array_equal(u.dust, s.dust)
    ru, rs = u.ref_density(), s.ref_density()
    assert (ru > 0).all()
    _held(rs, ru, "density", L, "dust density")


@pytest.mark.parametrize("periodic", [1, 0])
@pytest.mark.parametrize("L", SCALES)
def test_wind_ref_geometric_passes_follow_the_law(periodic, L):
    """wind_ref.density and wind_ref.spread: the loop around them (feedback) converts with the cgs units of the
    parameters (UnitVelocity_in_cm_per_s, UnitDensity_in_cgs, the cross-section), which break the law."""
    import wind_ref as R
    from test_gpu_wind import WindCase
    res = []
    for box in (1.0, L):
        c = WindCase(periodic, nwind=200, ng=8, box=box)
        f = c.fields()
        dtj = c.dt_jump()
        M = R.Margins()
        rho, drmin = R.density(c.par, R.gas_of(f), f["pos"][c.wind], f["hsml"][c.wind], dtj, M)
        dmom = c.old * (0.1 + 0.5 * np.random.default_rng(9).random(len(c.wind)))
        inj = np.zeros((c.pr.ngas, 3), R.LD)
        sp = R.spread(c.par, R.gas_of(f), f["pos"][c.wind], f["hsml"][c.wind], f["vel"][c.wind], dtj, rho, dmom, inj, M)
        assert M.smallest() >= 1e-9, M.by_kind
        res.append((rho, drmin, sp, inj.astype(np.float64)))
    (r1, d1, s1, i1), (r2, d2, s2, i2) = res
    assert (r1 > 0).sum() > 30 and np.array_equal(s1, s2) and np.array_equal(d1 == 1.e40, d2 == 1.e40)
    _held(r2, r1, "density", L, "new_density")
    ok = d1 < 1.e40
    assert ok.sum() > 30
    _held(d2[ok], d1[ok], "len", L, "drmin")
    _held(i2, i1, "momentum", L, "injected momentum")


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("L", SCALES)
def test_fof_ref_follows_the_law(periodic, L):
    import fof_cases as FC
    import fof_ref as FR
    c = FC.clumps(2000, periodic)
    s = SC.fof_rescaled(c, L)
    if L in POW2:       # the builder's own box argument makes the same positions
        b = FC.clumps(2000, periodic, box=L)
        assert np.array_equal(b["pos"], s["pos"]) and b["linkl"] == s["linkl"] and np.array_equal(b["hsml"], s["hsml"])
    ru, rs = FR.fof(**FC.ref_args(c)), FR.fof(**FC.ref_args(s))
    assert ru["Ngroups"] > 100 and ru["largest"] > 30
    for k in ("label", "grnr", "ids"):
        assert np.array_equal(rs[k], ru[k]), k
    assert (rs["Ngroups"], rs["Nids"], rs["largest"], rs["nearest_iterations"]) == \
        (ru["Ngroups"], ru["Nids"], ru["largest"], ru["nearest_iterations"])
    gu, gs = ru["groups"], rs["groups"]
    for k in ("Len", "Offset", "MinID", "GrNr", "LenType", "index_maxdens"):
        assert np.array_equal(gs[k], gu[k]), k
    assert np.array_equal(gs["MaxDens"], gu["MaxDens"])
    _held(gs["Mass"], gu["Mass"], "mass", L, "Mass")
    _held(gs["MassType"], gu["MassType"], "mass", L, "MassType")
    _held(gs["Vel"], gu["Vel"], "vel", L, "Vel")
    assert np.abs(gs["CM"] - L * gu["CM"]).max() < RTOL * s["box"]
    if periodic:
        assert np.all((gs["CM"] >= 0) & (gs["CM"] < s["box"]))
        assert (np.abs(gu["CM"][:, 1] - 0.5) > 0.49).any()        # a group by a face (the first clump straddles two)


@pytest.mark.parametrize("L", SCALES)
def test_potential_ref_follows_the_law(L):
    """potential_ref: the walk over the oracle's tree of the open problem, the entries of the Ewald potential table
    (potcorr / BoxSize: exponent -1 for fixed masses, so 2 with the masses' L^3), and the periodic mesh potential"""
    import potential_ref as R
    res = []
    for box in (1.0, L):
        pr = SC.problem(0, box)
        ic = pr.ic
        ps = pr.force_soft[ic["type"]]
        T = R.RefTree.from_oracle(pr.oracle_tree().dump(), ic["pos"], ic["mass"], ps)
        old = SC.oracle_cached(0, box)["old_bh"][1]
        tg = np.arange(0, pr.n, 4)
        w, nint = R.walk_potential(T, ic["pos"][tg], ps[tg], old[tg], 0.0, pr.ErrTolForceAcc, False, pr.box, True)
        pp = SC.problem(1, box)
        mesh = R.pm_potential(pp.ic["pos"], pp.ic["mass"], pp.box, pp.G, SC.PMGRID, SC.asmth_of(pp))
        res.append((w, nint, mesh))
    (w1, n1, m1), (w2, n2, m2) = res
    assert np.array_equal(n1, n2) and n1.max() < SC.unit_problem(0).n
    _held(w2, w1, "potential", L, "walk")
    _held(m2, m1, "potential", L, "mesh")
    idx = [[0, 0, 0], [3, 5, 7], [64, 64, 64], [1, 0, 63]]
    assert np.abs(R.pot_table(L, idx) * L - R.pot_table(1.0, idx)).max() <= 4e-16 * np.abs(R.pot_table(1.0, idx)).max()


@pytest.mark.parametrize("L", SCALES)
def test_pm_nonperiodic_ref_follows_the_law(L):
    import pm_nonperiodic_ref as NP
    res = []
    for box in (1.0, L):
        pr = SC.problem(0, box)
        reg = NP.region(pr.ic["pos"], SC.PMGRID)
        res.append((NP.pm_force(pr.ic["pos"], pr.ic["mass"], reg, pr.G), NP.pm_potential(pr.ic["pos"], pr.ic["mass"], reg, pr.G)))
    _held(res[1][0], res[0][0], "gravpm", L, "mesh force")
    _held(res[1][1], res[0][1], "potential", L, "mesh potential")
