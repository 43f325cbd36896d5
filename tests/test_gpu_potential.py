"""ghip_potential (compute_potential, potential.c:22-325) and ghip_global_quantities
(compute_global_quantities_of_system, global.c:18-238) on the device, against the numpy restatement in
tests/potential_ref.py: the walk over the exported tree of the same device build, the direct sum, the
Ewald potential table, the finish with the PM potential, the kept tree of a sub-step, the per-type sums
and the refusal on a sharded context."""
import numpy as np
import pytest

from common import Problem, bindings, ics
import potential_ref as R

pytestmark = pytest.mark.gpu
B = bindings()
TOL = 1e-12
_TABLES = {}


def _table(box):
    if box not in _TABLES:
        _TABLES[box] = R.pot_table(box)
    return _TABLES[box]


def _pot_params(pr, theta, G=1.0, pmgrid=0, comoving=0, Omega0=0.0, OmegaLambda=0.0, Hubble=0.0):
    p = B.PotParams()
    asmth = 1.25 * pr.box / pmgrid if pmgrid else 0.0
    p.grav = pr.g_grav(theta, 4.5 * asmth, asmth)
    p.pm = B.PmParams(int(pmgrid), pr.box, float(G), asmth)
    p.G = G
    for i in range(6):
        p.SofteningTable[i] = pr.force_soft[i] / 2.8
    p.comoving, p.Omega0, p.OmegaLambda, p.Hubble = int(comoving), Omega0, OmegaLambda, Hubble
    return p


def _err(dev, ref):
    scale = np.maximum(np.abs(ref), np.abs(ref).mean())
    return float(np.max(np.abs(dev - ref) / scale))


def _device(pr, adaptive=False):
    """context with a built tree and OldAcc from a first force walk (the relative criterion reads it)"""
    fp = pr.device()
    if adaptive:
        fp.set_adaptive_gravsoft(True)
    pr.device_tree(fp)
    fp.set_field(B.F_OLDACC, np.zeros(pr.n))
    fp.gravity(pr.g_grav(0.5), B.WALK_NEWTON)
    old = np.linalg.norm(fp.get_field(B.F_GRAVACCEL), axis=1)
    fp.set_field(B.F_OLDACC, old)
    return fp, old


def _psoft(pr, adaptive):
    ps = pr.force_soft[pr.ic["type"]].copy()
    if adaptive:
        ps[:pr.ngas] = pr.hsml0[:pr.ngas]
    return ps


def _ref_walk(fp, pr, theta, old, targets, adaptive=False, pmgrid=0):
    ic = pr.ic
    ps = _psoft(pr, adaptive)
    exp = fp.tree_export(adaptive=adaptive, unequal=int(pr.unequal))
    T = R.RefTree.from_export(exp, pr.n, ic["pos"], ic["mass"], ps, pr.force_soft,
                              unequal=bool(pr.unequal), adaptive=adaptive)
    kw = {}
    if pmgrid:
        asmth = 1.25 * pr.box / pmgrid
        kw = dict(rcut=4.5 * asmth, asmth=asmth)
    periodic = bool(pr.periodic)
    tab = _table(pr.box) if periodic and not pmgrid else None
    return R.walk_potential(T, ic["pos"][targets], ps[targets], old[targets], theta, pr.ErrTolForceAcc,
                            periodic, pr.box, bool(pr.unequal) or adaptive, tab, **kw)


VARIANTS = {
    "newton_bh": dict(periodic=0, theta=0.5),
    "newton_rel": dict(periodic=0, theta=0.0),
    "unequal": dict(periodic=0, theta=0.0, unequal=True),
    "adaptive": dict(periodic=0, theta=0.0, adaptive=True),
    "ewald_bh": dict(periodic=1, theta=0.5),
    "ewald_rel": dict(periodic=1, theta=0.0),
    "shortrange": dict(periodic=1, theta=0.0, pmgrid=16),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_walk_parity_all_targets(name):
    v = VARIANTS[name]
    pr = Problem(ng=8, periodic=v["periodic"], unequal=v.get("unequal", False))
    adaptive = v.get("adaptive", False)
    pmgrid = v.get("pmgrid", 0)
    fp, old = _device(pr, adaptive)
    fp.potential(_pot_params(pr, v["theta"], pmgrid=pmgrid))
    dev = fp.get_potential()
    tg = np.arange(pr.n)
    w, nint = _ref_walk(fp, pr, v["theta"], old, tg, adaptive, pmgrid)
    ic = pr.ic
    pm = dict(pmgrid=pmgrid, box=pr.box, asmth=1.25 * pr.box / pmgrid) if pmgrid else None
    ref = R.finish(w, ic["pos"], ic["mass"], ic["type"], pr.force_soft / 2.8, 1.0, pm=pm)
    # (the mesh part adds the rounding of the FFTs and of the deposit's atomic sums)
    assert _err(dev, ref) < (1e-10 if pmgrid else TOL), name
    assert fp.potential_interactions() == (int(nint.sum()), int(nint.max()))
    fp.close()


def test_walk_parity_c2_sampled_targets():
    """c2 size (2 x 64^3 particles), 2048 sampled targets: periodic with the Ewald potential, and the
    same positions without periodicity"""
    ic = ics.make_ics(64, gas=True)
    rng = np.random.default_rng(9)
    for periodic in (1, 0):
        pr = Problem(ic=ic, periodic=periodic)
        fp, old = _device(pr)
        fp.potential(_pot_params(pr, 0.0))
        dev = fp.get_potential()
        tg = np.sort(rng.choice(pr.n, 2048, replace=False))
        w, _ = _ref_walk(fp, pr, 0.0, old, tg)
        ref = R.finish(w, ic["pos"][tg], ic["mass"][tg], ic["type"][tg], pr.force_soft / 2.8, 1.0)
        assert _err(dev[tg], ref) < TOL, periodic
        fp.close()


def test_tiny_opening_angle_on_the_device_is_the_direct_sum():
    ic = ics.make_plummer(2000, seed=5, gas_fraction=0.0)
    pr = Problem(ic=ic, periodic=0)
    fp, _ = _device(pr)
    fp.potential(_pot_params(pr, 1e-8))
    dev = fp.get_potential()
    ps = _psoft(pr, False)
    d = R.direct_potential(ic["pos"], ic["mass"], ps, ps, np.arange(pr.n))
    ref = d + ic["mass"] / (pr.force_soft / 2.8)[ic["type"]]
    assert _err(dev, ref) < TOL
    assert fp.potential_interactions()[1] == pr.n
    fp.close()


def test_ewald_potential_table():
    pr = Problem(ng=4, periodic=1)
    fp = pr.device()
    for box in (1.0, 2.5):
        t = fp.ewald_pot_table(box)
        ref = _table(box)
        assert t[0, 0, 0] == R.POT_ORIGIN / box
        assert np.max(np.abs(t - ref)) < 1e-13 * np.abs(ref).max()
    fp.close()


@pytest.mark.parametrize("case", ["pm16_comoving", "pm32", "comoving_open", "lambda"])
def test_finish_and_mesh_potential(case):
    periodic = case.startswith("pm")
    pmgrid = {"pm16_comoving": 16, "pm32": 32}.get(case, 0)
    comoving = case in ("pm16_comoving", "comoving_open")
    pr = Problem(ng=8, periodic=int(periodic))
    fp, old = _device(pr)
    cosmo = dict(Omega0=0.3, OmegaLambda=0.7, Hubble=0.8)
    G = 0.7
    fp.potential(_pot_params(pr, 0.0, G=G, pmgrid=pmgrid, comoving=comoving, **cosmo))
    dev = fp.get_potential()
    w, _ = _ref_walk(fp, pr, 0.0, old, np.arange(pr.n), pmgrid=pmgrid)
    ic = pr.ic
    pm = dict(pmgrid=pmgrid, box=pr.box, asmth=1.25 * pr.box / pmgrid) if pmgrid else None
    ref = R.finish(w, ic["pos"], ic["mass"], ic["type"], pr.force_soft / 2.8, G, comoving=comoving,
                   periodic=periodic, pm=pm, **cosmo)
    assert _err(dev, ref) < (1e-10 if pmgrid else TOL), case
    # every term matters: without the mesh / the r^2 terms the result is another one
    bare = R.finish(w, ic["pos"], ic["mass"], ic["type"], pr.force_soft / 2.8, G)
    assert _err(dev, bare) > 1e-6
    fp.close()


def test_mesh_potential_cells_at_the_box_edges():
    """the periodic mesh potential with particles in the last cell of every axis (the +1 corner wraps) and at the
    origin, PMGRID 8: the set of test_pm_periodic_cells_at_the_box_edges without the coordinates equal to BoxSize"""
    from common import box_edge_particles
    pmgrid, G = 8, 0.7
    pr = Problem(ic=box_edge_particles(2.5, pmgrid, on_the_edge=False), periodic=1)
    ic = pr.ic
    j = np.arange(3)
    assert pr.n == 60 and (((pmgrid / pr.box) * ic["pos"]).astype(np.int64)[j, j] == pmgrid - 1).all()
    fp, old = _device(pr)
    fp.potential(_pot_params(pr, 0.0, G=G, pmgrid=pmgrid))
    dev = fp.get_potential()
    w, _ = _ref_walk(fp, pr, 0.0, old, np.arange(pr.n), pmgrid=pmgrid)
    pm = dict(pmgrid=pmgrid, box=pr.box, asmth=1.25 * pr.box / pmgrid)
    ref = R.finish(w, ic["pos"], ic["mass"], ic["type"], pr.force_soft / 2.8, G, periodic=True, pm=pm)
    assert np.isfinite(ref).all()
    print("err = %.3g" % _err(dev, ref))
    assert _err(dev, ref) < 1e-10
    bare = R.finish(w, ic["pos"], ic["mass"], ic["type"], pr.force_soft / 2.8, G)
    assert _err(dev, bare) > 1e-6   # (the mesh part is not lost in the tolerance)
    fp.close()


def test_kept_tree_of_a_substep():
    pr = Problem(ng=8, periodic=0, gas=False)
    ic = pr.ic
    fp = pr.device()
    fp.set_dynamic_tree(True)
    pr.device_tree(fp)
    fp.set_field(B.F_OLDACC, np.zeros(pr.n))
    dt = 0.002 * pr.box / np.abs(ic["vel"]).max()
    pos1 = ic["pos"] + ic["vel"] * dt
    fp.set_field(B.F_POS, pos1)
    fp.tree_substep(dt)
    fp.potential(_pot_params(pr, 0.5))
    dev = fp.get_potential()
    d = fp.tree_dump_dynamic()
    T = R.RefTree.from_elements(d["xm"], d["cl"], d["lk"])
    ps = _psoft(pr, False)
    w, _ = R.walk_potential(T, pos1, ps, np.zeros(pr.n), 0.5)
    ref = R.finish(w, pos1, ic["mass"], ic["type"], pr.force_soft / 2.8, 1.0)
    assert _err(dev, ref) < TOL
    fp.close()


def _gq_state(pr, seed=11):
    rng = np.random.default_rng(seed)
    n, ng = pr.n, pr.ngas
    ptype = pr.ic["type"].copy()
    dm = np.arange(ng, n)
    ptype[dm[rng.random(n - ng) < 0.2]] = 3
    ptype[dm[rng.random(n - ng) < 0.1]] = 4
    return dict(pos=pr.ic["pos"], vel=pr.ic["vel"], mass=pr.ic["mass"] * (0.5 + rng.random(n)),
                ptype=ptype.astype(np.int32), timebin=rng.integers(0, 8, n).astype(np.int32),
                ti_begstep=rng.integers(0, 2000, n).astype(np.int32),
                gravaccel=rng.standard_normal((n, 3)), hydroaccel=rng.standard_normal((ng, 3)),
                entropy=0.05 * (1 + rng.random(ng)), dtentropy=1e-3 * rng.standard_normal(ng),
                density=1 + rng.random(ng), photon=rng.random(n))


def _gq_device(pr, s, perm=None):
    """context holding the state s (particles in the order perm, gas first) with its potential"""
    n, ng = pr.n, pr.ngas
    perm = np.arange(n) if perm is None else perm
    fp = B.ForcePath(0)
    fp.set_counts(n, ng)
    for f, k in ((B.F_POS, "pos"), (B.F_VEL, "vel"), (B.F_MASS, "mass"), (B.F_TYPE, "ptype"),
                 (B.F_TIMEBIN, "timebin"), (B.F_TI_BEGSTEP, "ti_begstep"), (B.F_GRAVACCEL, "gravaccel")):
        fp.set_field(f, s[k][perm])
    gp = perm[:ng]
    for f, k in ((B.F_HYDROACCEL, "hydroaccel"), (B.F_ENTROPY, "entropy"), (B.F_DTENTROPY, "dtentropy"),
                 (B.F_DENSITY, "density")):
        fp.set_field(f, s[k][gp])
    fp.set_field(B.F_HSML, pr.hsml0[perm])
    fp.set_field(B.F_OLDACC, np.zeros(n))
    pr.device_tree(fp)
    fp.potential(_pot_params(pr, 0.5))
    return fp


def _gq_params(comoving):
    p = B.GlobalParams()
    p.Ti_Current, p.Timebase_interval = 3000, (0.0 - np.log(0.1)) / 4096 if comoving else 1e-3
    p.ComovingIntegrationOn, p.Time = int(comoving), 0.6 if comoving else 1.0
    p.logTimeBegin, p.logTimeMax = (np.log(0.1), 0.0) if comoving else (0.0, 0.0)
    p.rad_fac = 3.0
    return p


@pytest.mark.parametrize("comoving", [0, 1])
def test_global_quantities(comoving):
    pr = Problem(ng=8, periodic=1)
    n, ng = pr.n, pr.ngas
    s = _gq_state(pr)
    rng = np.random.default_rng(3)
    gk = np.cumsum(0.01 + rng.random(1000) * 1e-3)
    hk = np.cumsum(0.02 + rng.random(1000) * 1e-3)
    tabs = dict(grav_kick_table=gk, hydro_kick_table=hk) if comoving else {}
    fp = _gq_device(pr, s)
    pot = fp.get_potential()
    p = _gq_params(comoving)
    dev = fp.global_quantities(p, old_photon_momentum=s["photon"], **tabs)
    ref, scale = R.global_quantities(
        s["pos"], s["vel"], s["mass"], s["ptype"], s["timebin"], s["ti_begstep"], s["gravaccel"],
        p.Ti_Current, p.Timebase_interval, pot=pot, ngas=ng, hydroaccel=s["hydroaccel"],
        entropy=s["entropy"], dtentropy=s["dtentropy"], density=s["density"], comoving=comoving,
        time=p.Time, tables=(p.logTimeBegin, p.logTimeMax, gk, hk), photon=s["photon"], rad_fac=3.0)
    assert R.max_rel_diff(dev, ref, scale) < TOL
    assert dev["EnergyRadComp"] > 0 and dev["EnergyPotComp"][0] != 0
    # a second call on the same state: the same bits
    again = fp.global_quantities(_gq_params(comoving), old_photon_momentum=s["photon"], **tabs)
    for k in dev:
        assert np.array_equal(np.asarray(dev[k]), np.asarray(again[k])), k
    fp.close()
    # another particle order (gas block first): the same sums up to rounding
    perm = np.concatenate([rng.permutation(ng), ng + rng.permutation(n - ng)])
    fp2 = _gq_device(pr, s, perm)
    dev2 = fp2.global_quantities(_gq_params(comoving), old_photon_momentum=s["photon"][perm], **tabs)
    assert R.max_rel_diff(dev2, dev, scale) < TOL
    fp2.close()


def test_sharded_context_is_refused_and_nothing_changes():
    pr = Problem(ng=4, periodic=1)
    fp = pr.device()
    pr.device_tree(fp)
    fp.set_field(B.F_OLDACC, np.zeros(pr.n))
    fields = (B.F_POS, B.F_VEL, B.F_MASS, B.F_OLDACC, B.F_HSML)
    before = [fp.get_field(f).copy() for f in fields]
    fp.set_shard(0, 2)
    with pytest.raises(B.GhipError) as e:
        fp.potential(_pot_params(pr, 0.5))
    assert B.GHIP_ERRORS[e.value.code] == "GHIP_EINVAL"
    with pytest.raises(B.GhipError):
        fp.get_potential()
    with pytest.raises(B.GhipError) as e:
        fp.global_quantities(_gq_params(0))
    assert B.GHIP_ERRORS[e.value.code] == "GHIP_EINVAL"
    for f, b in zip(fields, before):
        assert np.array_equal(fp.get_field(f), b)
    fp.close()
