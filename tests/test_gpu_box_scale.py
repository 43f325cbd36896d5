"""The device in boxes that are not the unit cube (tests/scale_cases.py; the references are held to the same law on
the CPU by tests/test_box_scale_cpu.py).  Two kinds of assertion:

  parity (P)  at L in {2.5, 2^17}: the device against the oracle or the numpy restatement on the SAME scaled inputs,
              at the bound of the pass's unit-box test (TOL = 1e-11; dust and wind 1e-12); every count, mark, label
              and integer equal.
  law (S)     at L in POW2 = {4, 2^17}: the device in the scaled box against LAW applied to the device in the unit
              box, two contexts of one process.  A power-of-two scale commutes with every fp64 operation of the
              walks, the cell moments, the keys and the neighbour and pair lists, so those outputs are bit-identical;
              what passes through pow(), a cube root or an atomic add of free order is held to TOL, and the
              operation is named where that is asserted.

ng 8 (512 gas + 512 DM), seed 3, unequal softenings unless a test says otherwise."""
import numpy as np
import pytest

import scale_cases as SC
from common import O, Problem, bindings, box_edge_particles, ics, relerr
from scale_cases import ODD, POW2, SHIFT, law, off_law, rescale_problem, rescaled

pytestmark = pytest.mark.gpu

TOL = 1e-11
PARITY = [ODD, 2.0 ** 17]
BOTH = [ODD] + POW2          # tests that assert parity and, at the powers of two, the law in one go
_DEV = {}


def _maxerr(a, b):
    """max |a - b| in units of the largest |b|"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ------------------------------------------------------------------------------------------------
# one step on the device, under the keys of scale_cases.oracle_step
# ------------------------------------------------------------------------------------------------
def device_step(pr, ref):
    """The passes of scale_cases.oracle_step on a fresh context; the old accelerations of the relative pass are the
    oracle's (`ref`), as in test_gravity_two_pass_parity, so that both sides open the same cells.  Further keys: the
    one-call pair walk (acc_pair_*), the interaction totals of the statistics, gravity_finish, the tree dump."""
    B = bindings()
    n, ng = pr.n, pr.ngas
    fp = pr.device()
    out = {}
    try:
        pr.device_tree(fp)
        out["nodes"] = ("nodes", fp.stats()["tree_nodes"])
        d = fp.tree_dump(0)
        out["tree_lk"], out["tree_perm"] = ("nodes", d["lk"]), ("nodes", d["perm"])
        out["tree_centre"], out["tree_side"] = ("center", d["cl"][:, :3]), ("len", d["cl"][:, 3])
        out["tree_s"], out["tree_mass"] = ("s", d["xm"][:, :3]), ("mass", d["xm"][:, 3])
        old = np.zeros(n)
        for name, theta in (("bh", pr.theta), ("rel", 0.0)):
            fp.set_field(B.F_OLDACC, old)
            fp.gravity(pr.g_grav(theta), B.WALK_NEWTON)
            out["acc_" + name] = ("acc", fp.get_field(B.F_GRAVACCEL))
            out["cost_" + name] = ("cost", fp.get_field(B.F_GRAVCOST))
            tot = fp.stats()["grav_interactions"]
            if pr.periodic:
                fp.gravity(pr.g_grav(theta), B.WALK_EWALD)
                out["acc_ew_" + name] = ("acc", fp.get_field(B.F_GRAVACCEL))
                out["cost_ew_" + name] = ("cost", fp.get_field(B.F_GRAVCOST))
                tot += fp.stats()["ewald_interactions"]
                fp.gravity(pr.g_grav(theta), B.WALK_NEWTON_EWALD)
                out["acc_pair_" + name] = ("acc", fp.get_field(B.F_GRAVACCEL))
                out["cost_pair_" + name] = ("cost", fp.get_field(B.F_GRAVCOST))
            out["interactions_" + name] = ("cost", tot)
            old = ref["old_" + name][1]
        fp.gravity_finish(pr.G * 3.0)
        out["finish_old"], out["finish_acc"] = ("acc", fp.get_field(B.F_OLDACC)), ("acc", fp.get_field(B.F_GRAVACCEL))
        if pr.periodic:
            a = SC.asmth_of(pr)
            fp.set_field(B.F_OLDACC, np.full(n, 3.0 * getattr(pr, "L", 1.0)))
            fp.gravity(pr.g_grav(pr.theta, 4.5 * a, a), B.WALK_SHORTRANGE)
            out["acc_sr"], out["cost_sr"] = ("acc", fp.get_field(B.F_GRAVACCEL)), ("cost", fp.get_field(B.F_GRAVCOST))
            fp.pm_periodic(SC.PMGRID, pr.box, pr.G)
            out["gravpm"] = ("gravpm", fp.get_field(B.F_GRAVPM))
        fp.density(pr.g_dens())
        st = fp.stats()
        out["dens_iterations"], out["ngb_visits"] = ("iterations", st["dens_iterations"]), \
            ("ngb_visits", st["dens_neighbours"])
        for k, f in (("hsml", B.F_HSML), ("numngb", B.F_NUMNGB), ("density", B.F_DENSITY), ("dhsmlfac", B.F_DHSMLFAC),
                     ("divvel", B.F_DIVVEL), ("curlvel", B.F_CURLVEL), ("pressure", B.F_PRESSURE)):
            out[k] = (k, fp.get_field(f)[:ng])
        fp.update_hmax()
        out["hmax"] = ("hsml", fp.tree_dump(1)["aux"])
        fp.hydro(pr.g_hydro())
        out["npairs"] = ("npairs", fp.stats()["hydro_pairs"])
        for k, f in (("hydroaccel", B.F_HYDROACCEL), ("dtentropy", B.F_DTENTROPY), ("maxsignalvel", B.F_MAXSIGNALVEL)):
            out[k] = (k, fp.get_field(f))
    finally:
        fp.close()
    return out


def _device(periodic, L, shifted=False):
    key = (int(periodic), float(L), bool(shifted))
    if key not in _DEV:
        _DEV[key] = device_step(SC.problem(periodic, L, shifted), SC.oracle_cached(periodic, L, shifted))
    return _DEV[key]


WALKS = ("bh", "rel", "ew_bh", "ew_rel", "sr")
# relative to each vector (relerr) in the unit-box tests / relative to the field's largest magnitude
SPH_REL = ("hsml", "numngb", "density", "dhsmlfac", "pressure", "maxsignalvel")
SPH_MAX = ("divvel", "curlvel", "hydroaccel", "dtentropy")
SPH_COUNTS = ("dens_iterations", "ngb_visits", "npairs")


def _check_parity(dev, ref, periodic):
    worst = {}
    for w in WALKS:
        if "acc_" + w not in ref:
            assert not periodic
            continue
        assert np.array_equal(dev["cost_" + w][1], ref["cost_" + w][1]), w
        worst["acc_" + w] = relerr(dev["acc_" + w][1], ref["acc_" + w][1])
    if periodic:
        for name in ("bh", "rel"):       # the pair in one call: the two walks of the reference
            assert np.array_equal(dev["cost_pair_" + name][1], ref["cost_ew_" + name][1])
            worst["acc_pair_" + name] = relerr(dev["acc_pair_" + name][1], ref["acc_ew_" + name][1])
        worst["gravpm"] = _maxerr(dev["gravpm"][1], ref["gravpm"][1])
    for name in ("bh", "rel"):
        assert dev["interactions_" + name][1] == int(ref[("cost_ew_" if periodic else "cost_") + name][1].sum())
    last = ref["acc_ew_rel" if periodic else "acc_rel"][1]
    worst["finish_old"] = relerr(dev["finish_old"][1], np.linalg.norm(last, axis=1))
    worst["finish_acc"] = relerr(dev["finish_acc"][1], 3.0 * last)
    assert dev["nodes"][1] == ref["nodes"][1]
    for k in SPH_COUNTS:
        assert dev[k][1] == ref[k][1], (k, dev[k][1], ref[k][1])
    for k in SPH_REL:
        worst[k] = relerr(dev[k][1], ref[k][1])
    for k in SPH_MAX:
        worst[k] = _maxerr(dev[k][1], ref[k][1])
    print("parity, worst: " + ", ".join("%s %.2e" % kv for kv in sorted(worst.items(), key=lambda kv: -kv[1])[:6]))
    for k, e in worst.items():
        assert e < TOL, (k, e)


# ------------------------------------------------------------------------------------------------
# walks and SPH in the periodic box
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1.0] + PARITY)
def test_step_parity_in_a_scaled_periodic_box(L):
    """P: WALK_NEWTON (theta 0.5, then the relative criterion), WALK_EWALD added to each, the pair in one call,
    WALK_SHORTRANGE and the periodic mesh at grid 16, gravity_finish, density with its h iteration, update_hmax,
    hydro.  (L = 1 is the problem itself in the unit box: seed 3 and unequal softenings are not those of
    test_gpu_parity.py.)"""
    _check_parity(_device(1, L), SC.oracle_cached(1, L), 1)


@pytest.mark.parametrize("L", PARITY)
def test_step_parity_of_a_scaled_open_problem(L):
    """P, scaled about the origin (the shifted one is test_open_and_shifted)"""
    _check_parity(_device(0, L), SC.oracle_cached(0, L), 0)


# What a power-of-two scale leaves bit-identical, and what not.
EXACT = ("tree_centre", "tree_side", "tree_s", "tree_mass",
         "acc_bh", "acc_rel", "acc_ew_bh", "acc_ew_rel", "acc_pair_bh", "acc_pair_rel", "acc_sr",
         "finish_old", "finish_acc")
# held to TOL, with the operation that does not commute with the scale:
ROUNDED = {
    # the deposit adds the particles' cell weights with fp64 atomics in the order the wavefronts arrive
    "gravpm": "atomic adds of free order in the mass assignment",
    # h <- h * cbrt / pow(..., 1/3) steps of the iteration (density.c:601-640): cbrt(8) is exact but cbrt(2^51) is
    # not computed as a scaling of cbrt(1), and every later field is a function of the converged h
    "hsml": "the cube root of the h iteration", "hmax": "the cube root of the h iteration",
    "numngb": "follows hsml", "density": "follows hsml", "dhsmlfac": "follows hsml", "divvel": "follows hsml",
    "curlvel": "follows hsml",
    "pressure": "pow(rho, GAMMA) of the equation of state", "maxsignalvel": "sqrt(GAMMA P / rho) of a rounded P",
    "hydroaccel": "follows pressure and hsml", "dtentropy": "follows pressure and hsml",
}


@pytest.mark.parametrize("periodic", [1, 0])
@pytest.mark.parametrize("L", POW2)
def test_step_follows_the_law(periodic, L):
    """S: the device in the box L against LAW applied to the device in the unit box."""
    unit, got = _device(periodic, 1.0), _device(periodic, L)
    assert set(unit) == set(got)
    worst = {}
    for key, (name, u) in unit.items():
        g = got[key][1]
        if SC.is_count(u):
            assert np.array_equal(g, u), key
        elif key in EXACT:
            e = off_law(g, u, name, L)
            assert e == 0.0, (key, e)
        else:
            assert key in ROUNDED, key
            worst[key] = off_law(g, u, name, L)
    print("law, not exact: " + ", ".join("%s %.2e" % kv for kv in sorted(worst.items(), key=lambda kv: -kv[1])))
    for k, e in worst.items():
        assert e < TOL, (k, ROUNDED[k], e)


# ------------------------------------------------------------------------------------------------
# open and shifted: negative coordinates, a domain corner away from the origin
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", PARITY)
def test_open_and_shifted(L):
    """P: the Plummer set (1 500, 30 % gas) x L + SHIFT(L): Newton walk (both criteria), density, hydro.  A law
    assertion does not apply: the translation changes the rounding of every coordinate."""
    ic = ics.make_plummer(1500, seed=7, gas_fraction=0.3)
    pr = rescale_problem(Problem(ic=ic, periodic=0, unequal=True), L, SHIFT(L))
    assert (pr.ic["pos"][:, 0] < 0).all() and (pr.ic["pos"][:, 1] > 4 * L).all() and np.all(pr.extent[0] != 0)
    ref = SC.oracle_step(pr)
    _check_parity(device_step(pr, ref), ref, 0)


# ------------------------------------------------------------------------------------------------
# tree
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", PARITY)
def test_tree_cells_and_moments_in_a_scaled_box(L):
    """P: the cells and moments of test_tree_cells_and_moments_match_the_insertion_tree, and the exported
    representation's cells and links' consistency; S is part of test_step_follows_the_law (node count, links, the
    cell of each particle equal; centres, sides and moments x L exactly)."""
    pr = SC.problem(1, L)
    fp = pr.device()
    pr.device_tree(fp)
    d = fp.tree_dump(0)
    T = pr.oracle_tree()
    od = T.dump()
    nodes = d["lk"][:, 1] < 0
    assert nodes.sum() == T.numnodes == fp.stats()["tree_nodes"]
    key_g = np.column_stack([d["cl"][nodes][:, 3], d["cl"][nodes][:, :3]])
    key_o = np.column_stack([od["len"], od["center"]])
    og, oo = np.lexsort(key_g.T[::-1]), np.lexsort(key_o.T[::-1])
    assert np.array_equal(key_g[og], key_o[oo])           # identical cells, bit for bit
    assert np.allclose(d["xm"][nodes][og][:, 3], od["mass"][oo], rtol=1e-15, atol=0)
    assert np.allclose(d["xm"][nodes][og][:, :3], od["s"][oo], rtol=1e-14, atol=0)
    assert np.array_equal(d["xm"][~nodes][:, :3], pr.ic["pos"][d["perm"]])
    ex, _, nxt, fat = fp.tree_export(unequal=1)
    key_e = np.column_stack([ex["len"], ex["center"]])
    oe = np.lexsort(key_e.T[::-1])
    assert np.array_equal(key_e[oe], key_o[oo])
    assert np.allclose(ex["s"][oe], od["s"][oo], rtol=1e-14, atol=0)
    o2e = np.empty(T.numnodes, np.int64)
    o2e[oo] = oe

    def conv(idx):
        idx = np.asarray(idx, np.int64)
        out = idx.copy()
        out[idx >= pr.n] = pr.n + o2e[idx[idx >= pr.n] - pr.n]
        return out
    g = ex[o2e]
    for k in ("sibling", "nextnode", "father"):
        assert np.array_equal(g[k], conv(od[k])), k
    assert np.array_equal(nxt[:pr.n], conv(od["p_nextnode"])) and np.array_equal(fat[:pr.n], conv(od["p_father"]))
    fp.close()


# ------------------------------------------------------------------------------------------------
# periodic mesh at the box edge
# ------------------------------------------------------------------------------------------------
def _edge_mesh(box):
    B = bindings()
    ic = box_edge_particles(box, 8)
    fp = B.ForcePath(0)
    fp.set_counts(len(ic["pos"]), 0)
    fp.set_field(B.F_POS, ic["pos"])
    fp.set_field(B.F_MASS, ic["mass"])
    fp.pm_periodic(8, box, 43007.1)
    got = fp.get_field(B.F_GRAVPM)
    fp.close()
    return ic, got


def test_periodic_mesh_cells_at_the_edge_of_a_scaled_box():
    """box_edge_particles(box, 8): coordinates equal to the box size, the last cell, the origin.  P at boxes 2^17 and
    2.5 against the oracle; S: the force at 2^17 against that at box 1 (the set is drawn as box x unit numbers, so
    it is the same set), to TOL: the deposit's atomic adds come in free order.  Masses are not scaled here: the
    mesh force of fixed masses goes as 1 / L^2."""
    unit_ic, unit = _edge_mesh(1.0)
    for box in (2.0 ** 17, 2.5):
        ic, got = _edge_mesh(box)
        cell = ((8 / box) * ic["pos"]).astype(np.int64)
        j = np.arange(3)
        assert (cell[j, j] == 8).all() and (cell[3] == 8).all() and (cell[4 + j, j] == 7).all()
        want = O.pm_periodic(ic["pos"], ic["mass"], box, 43007.1, 8)
        assert np.isfinite(want).all()
        e = _maxerr(got, want)
        print("box %g: %.2e" % (box, e))
        assert e < TOL
        if box == 2.0 ** 17:
            assert np.array_equal(ic["pos"], unit_ic["pos"] * box)
            assert _maxerr(got, unit / box ** 2) < TOL


# ------------------------------------------------------------------------------------------------
# drift with the wrap
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", PARITY)
def test_drift_wraps_at_the_faces_of_a_scaled_box(L):
    """P against O.drift (predict.c:129-259, :282-310) with particles within one step of each face, moving out and
    moving in; every result in [0, box).  The law adds nothing: a rescaling at fixed time keeps the time bins."""
    B = bindings()
    pr = SC.problem(1, L)
    rng = np.random.default_rng(21)
    n, ng = pr.n, pr.ngas
    box = pr.box
    time1, tb = 7, pr.timebase * 50
    step = time1 * tb                                      # every particle starts at time 0
    ic = dict(pr.ic)
    pos, vel = ic["pos"].copy(), ic["vel"].copy()
    k = 0
    for j in range(3):
        for face in (0, 1):
            # the distance to the face in units of what the particle covers in the step: it crosses early, late,
            # stops short of the face, or (negative) starts next to the face and moves inward
            for frac in (0.25, 0.75, 1.5, -0.1):
                i = 10 * k
                k += 1
                v = abs(vel[i, j]) + 0.01 * L
                d = abs(frac) * v * step
                pos[i, j] = box - d if face else d
                vel[i, j] = v * (1 if face else -1) * (1 if frac > 0 else -1)
    assert k == 24 and (pos >= 0).all() and (pos < box).all()
    ic["pos"], ic["vel"] = np.ascontiguousarray(pos), np.ascontiguousarray(vel)
    q = rescale_problem(pr, 1.0)
    q.ic = ic
    ti_cur = np.zeros(n, np.int32)
    grav = L * rng.standard_normal((n, 3))
    hyd = L * rng.standard_normal((ng, 3))
    dens, divv, pres = 1.0 + rng.random(ng), rng.standard_normal(ng), L * L * rng.random(ng)
    hs = q.hsml0[:ng] * (0.5 + rng.random(ng))
    hfull = q.hsml0.copy()
    hfull[:ng] = hs
    fp = q.device()
    for fid, arr in ((B.F_TI_CURRENT, ti_cur), (B.F_GRAVACCEL, grav), (B.F_HYDROACCEL, hyd), (B.F_DENSITY, dens),
                     (B.F_DIVVEL, divv), (B.F_PRESSURE, pres), (B.F_HSML, hfull)):
        fp.set_field(fid, arr)
    minh = float(np.median(hs))
    fp.drift(time1, tb, min_gas_hsml=minh, box_wrap=True, boxsize=box)
    want = O.drift(time1, tb, pos, vel, ic["type"], ti_cur, q.timebin, q.ti_begstep, grav, q.velpred, hyd, dens, hs,
                   divv, q.entropy, q.dtentropy, pres, minhsml=minh, wrap=True, boxsize=box)
    assert want["rc"] == 0
    raw = pos + vel * step
    assert 12 <= ((raw < 0) | (raw >= box)).any(axis=1).sum() and (raw[:, 0] >= box).any() and (raw[:, 2] < 0).any()
    got = fp.get_field(B.F_POS)
    assert np.array_equal(fp.get_field(B.F_TI_CURRENT), want["ti_current"])
    assert np.abs(got - want["pos"]).max() < 1e-15 * box          # (the unit-box test: 1e-15 absolute in box 1)
    assert (got >= 0).all() and (got < box).all()
    assert (want["pos"] >= 0).all() and (want["pos"] < box).all()
    assert relerr(fp.get_field(B.F_VELPRED), want["velpred"]) < 1e-14
    assert relerr(fp.get_field(B.F_DENSITY), want["density"]) < 1e-14
    assert relerr(fp.get_field(B.F_HSML)[:ng], want["hsml"]) < 1e-14
    assert relerr(fp.get_field(B.F_PRESSURE), want["pressure"]) < 1e-13
    fp.close()


# ------------------------------------------------------------------------------------------------
# potential
# ------------------------------------------------------------------------------------------------
_POT = {}


def _potential(L):
    """ghip_potential on problem(1, L): the tree part with the Ewald correction (theta 0, OldAcc the oracle's), and
    with the periodic mesh at grid 16; the exported tree and the device's Ewald potential table for the reference"""
    import test_gpu_potential as TP
    if L not in _POT:
        B = bindings()
        pr = SC.problem(1, L)
        old = SC.oracle_cached(1, L)["old_bh"][1]
        fp = pr.device()
        pr.device_tree(fp)
        fp.set_field(B.F_OLDACC, old)
        out = dict(pr=pr, old=old)
        fp.potential(TP._pot_params(pr, 0.0))
        out["tree"], out["tree_nint"] = fp.get_potential(), fp.get_potential_interactions()
        out["table"] = fp.ewald_pot_table(pr.box)
        out["export"] = fp.tree_export(unequal=1)
        fp.potential(TP._pot_params(pr, 0.0, pmgrid=SC.PMGRID))
        out["mesh"], out["mesh_nint"] = fp.get_potential(), fp.get_potential_interactions()
        fp.close()
        _POT[L] = out
    return _POT[L]


@pytest.mark.parametrize("L", PARITY)
def test_potential_parity_in_a_scaled_box(L):
    """P against potential_ref's walk over the exported tree: tree + Ewald at the walks' 1e-12 (TOL of
    test_gpu_potential.py), with the periodic mesh at its 1e-10.  The walk reads the device's own table of the
    Ewald potential, which is first held to potential_ref.pot_table(box) at 400 entries drawn at random and the
    origin (the whole table takes the reference seconds)."""
    import potential_ref as R
    import test_gpu_potential as TP
    d = _potential(L)
    pr, ic = d["pr"], d["pr"].ic
    idx = np.r_[[[0, 0, 0], [64, 64, 64]], np.random.default_rng(4).integers(0, 65, (400, 3))]
    want = R.pot_table(pr.box, idx)
    got = d["table"][idx[:, 0], idx[:, 1], idx[:, 2]]
    assert got[0] == R.POT_ORIGIN / pr.box
    assert np.abs(got - want).max() < 1e-13 * np.abs(want).max()
    ps = pr.force_soft[ic["type"]]
    T = R.RefTree.from_export(d["export"], pr.n, ic["pos"], ic["mass"], ps, pr.force_soft, unequal=True)
    tg = np.arange(pr.n)
    soft = pr.force_soft / 2.8
    w, nint = R.walk_potential(T, ic["pos"], ps, d["old"], 0.0, pr.ErrTolForceAcc, True, pr.box, True, d["table"])
    ref = R.finish(w, ic["pos"], ic["mass"], ic["type"], soft, 1.0)
    e = TP._err(d["tree"], ref)
    assert np.array_equal(d["tree_nint"], nint)
    a = SC.asmth_of(pr)
    w, nint = R.walk_potential(T, ic["pos"], ps, d["old"], 0.0, pr.ErrTolForceAcc, True, pr.box, True, None,
                               rcut=4.5 * a, asmth=a)
    ref = R.finish(w, ic["pos"], ic["mass"], ic["type"], soft, 1.0, pm=dict(pmgrid=SC.PMGRID, box=pr.box, asmth=a))
    em = TP._err(d["mesh"], ref)
    print("L = %g: tree + Ewald %.2e, with the mesh %.2e" % (L, e, em))
    assert e < 1e-12 and em < 1e-10
    assert np.array_equal(d["mesh_nint"], nint)


@pytest.mark.parametrize("L", POW2)
def test_potential_follows_the_law(L):
    """S: the tree part bit-identical (the walk, the table look-up and the self term scale by powers of two), the
    interactions equal; with the mesh to the 1e-10 of the mesh potential: the deposit's atomic adds come in free
    order."""
    u, s = _potential(1.0), _potential(L)
    assert np.array_equal(s["tree_nint"], u["tree_nint"]) and np.array_equal(s["mesh_nint"], u["mesh_nint"])
    e = off_law(s["tree"], u["tree"], "potential", L)
    et = off_law(s["table"], u["table"] / L ** 3, "potential", L)
    em = off_law(s["mesh"], u["mesh"], "potential", L)
    print("L = %g: tree %.2e table %.2e mesh %.2e" % (L, e, et, em))
    assert et == 0.0 and e == 0.0
    assert em < 1e-10


@pytest.mark.parametrize("L", POW2)
def test_exported_tree_follows_the_law(L):
    """S for ghip_tree_export (the export of the potential's contexts): the same nodes in the same order, every link
    and flag equal, sides, centres and centres of mass x L and masses x L^3 exactly"""
    (nu, xu, nxu, fau), (ns, xs, nxs, fas) = _potential(1.0)["export"], _potential(L)["export"]
    assert len(ns) == len(nu) == SC.oracle_cached(1, 1.0)["nodes"][1]
    for k in ("sibling", "nextnode", "father", "bitflags"):
        assert np.array_equal(ns[k], nu[k]), k
    assert np.array_equal(nxs, nxu) and np.array_equal(fas, fau)
    assert np.array_equal(ns["len"], L * nu["len"]) and np.array_equal(ns["center"], L * nu["center"])
    assert np.array_equal(ns["s"], L * nu["s"]) and np.array_equal(ns["mass"], L ** 3 * nu["mass"])
    assert np.array_equal(xs["vs"], L * xu["vs"]) and np.array_equal(xs["vmax"], L * xu["vmax"])
    assert np.array_equal(xs["hmax"], L * xu["hmax"]) and (xu["hmax"] > 0).any()


# ------------------------------------------------------------------------------------------------
# open mesh on the shifted set
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", PARITY)
def test_open_mesh_on_the_shifted_set(L):
    """P against pm_nonperiodic_ref (region and force) on the Plummer set x L + SHIFT(L), grid 16, at the bound of
    test_gpu_pm_nonperiodic.py.  No law assertion: the translation changes the rounding of every coordinate."""
    import pm_nonperiodic_ref as NP
    B = bindings()
    ic = rescaled(ics.make_plummer(1500, seed=7, gas_fraction=0.3), L, SHIFT(L))
    pr = Problem(ic=ic, periodic=0)
    fp = pr.device()
    from test_gpu_pm_nonperiodic import same_region
    want_reg = NP.region(ic["pos"], SC.PMGRID)
    assert same_region(fp.pm_find_region(SC.PMGRID), want_reg)          # bit for bit
    assert want_reg["Corner"][0] < 0 < want_reg["Corner"][1]
    fp.pm_nonperiodic(SC.PMGRID, pr.G)
    got = fp.get_field(B.F_GRAVPM)
    want = NP.pm_force(ic["pos"], ic["mass"], want_reg, pr.G)
    e = _maxerr(got, want)
    print("L = %g: %.2e" % (L, e))
    assert e < TOL
    fp.close()


# ------------------------------------------------------------------------------------------------
# SPH with the time-dependent viscosity
# ------------------------------------------------------------------------------------------------
_VISC = {}


def _visc(L):
    import test_gpu_visc as TV
    import visc_ref as VR
    if L not in _VISC:
        B = bindings()
        pr = SC.problem(1, L)
        fp, ds = TV.after_density(pr)
        V = VR.params(time_dependent=1, ArtBulkViscConst=0.8)
        alpha = TV.alpha_of(pr.ngas)
        fp.set_viscosity(TV.visc_struct(V))
        fp.visc_set_alpha(alpha)
        fp.hydro(pr.g_hydro())
        out = dict(pr=pr, ds=ds, V=V, alpha=alpha, pairs=fp.stats()["hydro_pairs"], dtalpha=fp.visc_get()[1])
        for k, f in (("hydroaccel", B.F_HYDROACCEL), ("dtentropy", B.F_DTENTROPY), ("maxsignalvel", B.F_MAXSIGNALVEL)):
            out[k] = fp.get_field(f)
        fp.close()
        _VISC[L] = out
    return _VISC[L]


@pytest.mark.parametrize("L", PARITY)
def test_time_dependent_viscosity_parity_in_a_scaled_box(L):
    """P: ghip_set_viscosity (time-dependent) against visc_ref on the device's own density results, as
    test_varying_alpha_against_the_all_pairs_reference"""
    import test_gpu_visc as TV
    import visc_ref as VR
    d = _visc(L)
    pr = d["pr"]
    ref = VR.hydro(pr, d["ds"], d["alpha"], d["V"], pr.g_hydro())
    B = bindings()
    fields = {B.F_HYDROACCEL: d["hydroaccel"], B.F_DTENTROPY: d["dtentropy"], B.F_MAXSIGNALVEL: d["maxsignalvel"]}
    TV.check_hydro(fields.__getitem__, d["pairs"], ref)
    ds = d["ds"]
    want = VR.dtalpha(ds["pressure"], ds["density"], ds["hsml"], ds["divvel"], ds["curlvel"], d["maxsignalvel"],
                      d["alpha"], d["V"], fac_mu=1.0, comoving=0)
    assert np.abs(d["dtalpha"] - want).max() < 1e-13 * np.abs(want).max()
    assert (want > 0).any() and (want < 0).any()


@pytest.mark.parametrize("L", POW2)
def test_time_dependent_viscosity_follows_the_law(L):
    """S to TOL (every input follows the smoothing lengths of the h iteration, with its cube root); the pair count
    equal.  Dtalpha is a rate: exponent 0."""
    u, s = _visc(1.0), _visc(L)
    assert s["pairs"] == u["pairs"]
    for k in ("hydroaccel", "dtentropy", "maxsignalvel"):
        assert off_law(s[k], u[k], k, L) < TOL, k
    assert off_law(s["dtalpha"], u["dtalpha"], "divvel", L) < TOL


# ------------------------------------------------------------------------------------------------
# sinks
# ------------------------------------------------------------------------------------------------
_SINK = {}


def _sink_passes(L, switches):
    """the three passes on the device for scale_cases.sink_setup(L), as test_sink_inputs_against_all_pairs"""
    key = (L, switches)
    if key not in _SINK:
        from test_gpu_sink import _device as sink_device
        sp = SC.sink_setup(L)
        ref = SC.sink_refs(L, 1, switches)
        B, fp = sink_device(sp)
        try:
            fp.set_field(B.F_DENSITY, sp.gas_density)
            gp = sp.params(B.BhParams, **ref["over"])
            ids = sp.ids[sp.sinks]
            dens = fp.sink_density(sp.pr.g_dens(), 1.5, sp.sinks, sp.hsml[sp.sinks])
            fp.sink_reset()
            fp.blackhole_evaluate(gp, sp.sinks, ids, sp.mdot, dens["density"])
            marks = fp.sink_marks()
            go = fp.blackhole_swallow(gp, sp.sinks, ids, sp.bh_mass[sp.sinks])
            mass = fp.get_field(B.F_MASS)
        finally:
            fp.close()
        _SINK[key] = (sp, ref, dens, marks, go, mass)
    return _SINK[key]


@pytest.mark.parametrize("switches", SC.SINK_SWITCHES)
@pytest.mark.parametrize("L", PARITY)
def test_sink_passes_parity_in_a_scaled_box(L, switches):
    """P: sink_density, blackhole_evaluate, blackhole_swallow against tests/sink_ref.py with check_sink_passes; one
    sink lies 0.3 spacings from the face x = 0"""
    from common import check_sink_passes
    sp, ref, dens, marks, go, mass = _sink_passes(L, switches)
    err = check_sink_passes(sp, ref, dens, marks, go, mass)
    print(L, switches, err)
    assert (ref["sw"] > 0).sum() >= 5 and ref["swallow"]["counts"].sum() >= 3


@pytest.mark.parametrize("switches", SC.SINK_SWITCHES)
@pytest.mark.parametrize("L", POW2)
def test_sink_passes_follow_the_law(L, switches):
    """S: marks, counts and the h iterations equal; the sums to the bounds of check_sink_passes.  The injected
    energy carries FeedbackCoeff and UnitMass_in_g and is not held to the law."""
    _, _, du, mu, gu, massu = _sink_passes(1.0, switches)
    _, _, ds, ms, gs, masss = _sink_passes(L, switches)
    assert ds["iterations"] == du["iterations"]
    assert np.array_equal(ms[0], mu[0]) and np.array_equal(gs["counts"], gu["counts"])
    assert np.array_equal(masss == 0, massu == 0)
    # the h iteration of the sinks bisects with a cube root (density.c:597-598): not bit-identical
    assert off_law(ds["hsml"], du["hsml"], "hsml", L) < 1e-13
    for k, name in (("density", "density"), ("entropy", "entropy"), ("gasvel", "gasvel")):
        assert off_law(ds[k], du[k], name, L) < 1e-12, k
    for k in ("acc_mass", "acc_bhmass", "acc_dustmass", "bh_mass"):
        assert off_law(gs[k], gu[k], "mass", L) <= 1e-13, k
    assert off_law(gs["acc_momentum"], gu["acc_momentum"], "momentum", L) <= 1e-13
    assert np.array_equal(masss, law("mass", massu, L))          # the masses that stay are the inputs


# ------------------------------------------------------------------------------------------------
# dust
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic", [1, 0])
@pytest.mark.parametrize("L", BOTH)
def test_dust_density_parity_in_a_scaled_box(L, periodic):
    """P at the 1e-12 of test_gpu_dust.py.  The law is asserted on the same call at L = 4 and 2^17 against the unit box:
    the density m_i sum W carries no power of L."""
    from test_gpu_dust import DustCase, TOL as DTOL
    case = DustCase(periodic, ndust=200, ng=8, box=L)
    B, fp = case.device()
    got = fp.dust_density(case.gparams(), case.dust)
    ref = case.ref_density()
    fp.close()
    assert relerr(got, ref) < DTOL and np.all(ref > 0)
    if L in POW2:
        unit = DustCase(periodic, ndust=200, ng=8)
        B, fp = unit.device()
        got1 = fp.dust_density(unit.gparams(), unit.dust)
        fp.close()
        # 1 / h^3 of the kernel: hinv * hinv * hinv of a power-of-two multiple is exact, so are the sums
        assert np.array_equal(got, got1)


@pytest.mark.parametrize("periodic", [1, 0])
def test_dust_drag_parity_at_box_2_5(periodic):
    """P (L = 2.5 only; the drag converts with the cgs units of its parameters, which no rescaling of the box
    touches, so there is no law to hold it to): the grains' side and the gas side in list order"""
    from test_gpu_dust import DustCase, TOL as DTOL, _scaled_err
    case = DustCase(periodic, ndust=200, ng=8, box=ODD)
    pr = case.pr
    ng, nd = pr.ngas, len(case.dust)
    B, fp = case.device()
    d7 = fp.dust_density(case.gparams(), case.dust)
    fp.set_dust_drag_heating(np.zeros(ng))
    order = np.arange(nd)
    out = case.drag(fp, order, d7)
    ref = case.ref_grains(order, d7)
    assert np.all(np.bincount(ref["regime"], minlength=6) >= 5)
    vel = fp.get_field(B.F_VEL)
    assert _scaled_err(vel[case.dust], ref["vel"]) < DTOL
    assert _scaled_err(out["delta_momentum"], ref["dmom"]) < DTOL
    assert _scaled_err(out["delta_energy"], ref["de"]) < DTOL
    assert relerr(out["vcoll"], ref["vcoll"]) < DTOL
    assert relerr(out["particle_velocity"], ref["d9"]) < DTOL
    gv, ge, gh, c = case.ref_gas(order, out["delta_momentum"], out["delta_energy"])
    assert c["touched"].max() >= 2 and c["floors"] > 0          # MinEgySpec, scaled with the box, still binds
    assert _scaled_err(vel[:ng], gv) < DTOL
    assert relerr(fp.get_field(B.F_ENTROPY), ge) < DTOL
    assert _scaled_err(fp.dust_drag_heating(), gh) < DTOL and np.abs(gh).max() > 0
    fp.close()


# ------------------------------------------------------------------------------------------------
# wind
# ------------------------------------------------------------------------------------------------
def _wind_passes(periodic, L):
    import wind_ref as R
    from test_gpu_wind import WindCase
    c = WindCase(periodic, nwind=200, ng=8, box=L)
    B, fp = c.device()
    f = c.fields()
    dtj = c.dt_jump()
    rho, drmin = fp.wind_density(c.gparams(), c.wind, dtj)
    dmom = c.old * (0.1 + 0.5 * np.random.default_rng(9).random(len(c.wind)))
    fp.wind_spread(c.gparams(), c.wind, dtj, rho, dmom)
    got = fp.wind_injected()
    fp.close()
    M = R.Margins()
    rr, rd = R.density(c.par, R.gas_of(f), f["pos"][c.wind], f["hsml"][c.wind], dtj, M)
    inj = np.zeros((c.pr.ngas, 3), R.LD)
    R.spread(c.par, R.gas_of(f), f["pos"][c.wind], f["hsml"][c.wind], f["vel"][c.wind], dtj, rho, dmom, inj, M)
    assert M.smallest() >= 1e-9, M.by_kind
    return (rho, drmin, got), (rr, rd, inj.astype(np.float64))


@pytest.mark.parametrize("periodic", [1, 0])
@pytest.mark.parametrize("L", BOTH)
def test_wind_density_and_spread_parity_in_a_scaled_box(L, periodic):
    """P: ghip_wind_density and ghip_wind_spread against wind_ref at the 1e-12 of test_gpu_wind.py; at L = 4 and 2^17 also
    the law against the unit box, to that bound (hinv3 and the weights m W / rho are exact under a power of two,
    the gas receives its shares by atomic adds of free order)"""
    from test_gpu_wind import TOL as WTOL, _scaled_err
    (rho, drmin, got), (rr, rd, ref) = _wind_passes(periodic, L)
    assert (rr > 0).sum() > 30 and (rd == 1.e40).sum() > 0
    assert _scaled_err(rho, rr) < WTOL
    assert np.array_equal(drmin == 1.e40, rd == 1.e40) and relerr(drmin, rd) < WTOL
    assert _scaled_err(got, ref) < WTOL and np.abs(ref).max() > 0
    if L in POW2:
        (rho1, drmin1, got1), _ = _wind_passes(periodic, 1.0)
        ok = drmin1 < 1.e40
        assert np.array_equal(rho, rho1) and np.array_equal(drmin[ok], L * drmin1[ok])
        assert off_law(got, got1, "momentum", L) < WTOL


def test_wind_feedback_in_a_periodic_box_of_4():
    """P: the whole loop of ghip_wind_feedback against wind_ref.feedback, periodic, L = 4; some particles leave
    [0, box) on the way (the loop does not wrap them: momentum_feedback.c:367-368; the searches take the nearest
    image).  The loop converts with cgs units: no law."""
    import wind_ref as R
    from test_gpu_wind import MARGIN, UNTOUCHED, WindCase, _check_loop
    c = WindCase(1, nwind=200, ng=8, box=4.0)
    ref = R.feedback(c.par, c.fields(), c.wind, c.state(), active=c.active)
    assert ref["margins"].smallest() >= MARGIN, ref["margins"].by_kind
    assert ref["status"] == "ok" and ref["iterations"] > 8
    end = ref["pos"][c.wind]
    assert ((end < 0) | (end >= c.pr.box)).any(axis=1).sum() >= 3
    B, fp = c.device()
    fp.set_active(c.active)
    start = {f: fp.get_field(f) for f in [B.F_POS, B.F_HSML, B.F_MASS] + [getattr(B, k) for k in UNTOUCHED]}
    out = c.feedback(fp)
    assert out["rc"] == 0
    _check_loop(c, B, fp, out, ref, start)
    fp.close()


# ------------------------------------------------------------------------------------------------
# friends-of-friends
# ------------------------------------------------------------------------------------------------
_FOF = {}


def _fof(case, key):
    import fof_ref as FR
    import fof_cases as FC
    import test_gpu_fof as TF
    if key not in _FOF:
        fp = TF.device(case)
        res = TF.call(fp, case)
        ref = FR.fof(**FC.ref_args(case))
        g = TF.check(fp, res, case, ref)
        _FOF[key] = dict(g=g, labels=fp.fof_labels(), ids=fp.fof_ids(),
                         head=(res.Ngroups, res.Nids, res.largest, res.nearest_iterations))
        fp.close()
    return _FOF[key]


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("L", PARITY)
def test_fof_parity_in_a_scaled_box(L, periodic):
    """P with test_gpu_fof.check: clumps(2000, True, box=L), whose first clump straddles two faces, and the open
    set x L + SHIFT(L)"""
    import fof_cases as FC
    if periodic:
        c = FC.clumps(2000, True, box=L)
    else:
        c = SC.fof_rescaled(FC.clumps(2000, False), L, SHIFT(L))
    d = _fof(c, (L, periodic, "P"))
    assert d["head"][0] > 100 and d["head"][2] > 30
    if periodic:
        assert (np.abs(d["g"]["CM"][:, 1] - 0.5 * L) > 0.49 * L).any()      # a group by a face


@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("L", POW2)
def test_fof_follows_the_law(L, periodic):
    """S: labels, GrNr, the ID list and the integer catalogue equal to the unit box's; Mass and CM to TOL (their sums
    are atomic adds of free order), CM inside the box"""
    import fof_cases as FC
    c1 = FC.clumps(2000, periodic)
    u = _fof(c1, (1.0, periodic, "S"))
    cs = SC.fof_rescaled(c1, L)
    s = _fof(cs, (L, periodic, "S"))
    assert s["head"] == u["head"]
    assert np.array_equal(s["labels"][0], u["labels"][0]) and np.array_equal(s["labels"][1], u["labels"][1])
    assert np.array_equal(s["ids"], u["ids"])
    for k in ("Len", "Offset", "MinID", "GrNr", "LenType", "index_maxdens"):
        assert np.array_equal(s["g"][k], u["g"][k]), k
    assert off_law(s["g"]["Mass"], u["g"]["Mass"], "mass", L) < TOL
    assert np.abs(s["g"]["CM"] - L * u["g"]["CM"]).max() < TOL * cs["box"]
    assert off_law(s["g"]["Vel"], u["g"]["Vel"], "vel", L) < TOL
    if periodic:
        assert np.all((s["g"]["CM"] >= 0) & (s["g"]["CM"] < cs["box"]))


# ------------------------------------------------------------------------------------------------
# shards: decomposition, migration, locally essential trees, ghosts, the sync point, dust, FoF
# ------------------------------------------------------------------------------------------------
NSHARDS = 3
_SHARDS = {}
SHARD_SPH = (("hsml", "F_HSML"), ("numngb", "F_NUMNGB"), ("density", "F_DENSITY"), ("dhsmlfac", "F_DHSMLFAC"),
             ("divvel", "F_DIVVEL"), ("curlvel", "F_CURLVEL"), ("pressure", "F_PRESSURE"),
             ("hydroaccel", "F_HYDROACCEL"), ("dtentropy", "F_DTENTROPY"), ("maxsignalvel", "F_MAXSIGNALVEL"))


def _shard_step(L):
    """problem(1, L) on 3 shards through one full step: GHIP_DD_DECOMPOSE with work weights and the domain cube
    found on the device, migration to the new ranges, the pair walk over the locally essential trees, density and
    hydro with their ghosts, then the sync-point form of the decomposition"""
    import sync_ref as SR
    import test_gpu_decomp as TD
    from common import ShardSet
    if L in _SHARDS:
        return _SHARDS[L]
    B = bindings()
    pr = SC.problem(1, L)
    n = pr.n
    cost, tbin = TD.seeded_work(n, 9)
    out = dict(pr=pr, work=(cost, tbin))
    S = ShardSet(pr, NSHARDS)
    try:
        out["keys"] = S.keys
        S.set_field(B.F_GRAVCOST, cost)
        S.set_field(B.F_TIMEBIN, tbin)
        S.run.decompose(TD.params(0, 1, find_extent=1))
        out["splits"] = TD.all_splits(S)
        out["domain"] = [fp.dd_get_domain() for fp in S.fp]
        before = S.owner.copy()
        S.migrate()
        out["moved"] = int((S.owner != before).sum())
        TD.owners_follow_the_keys(S, out["splits"], S.keys)
        out["owner"] = S.owner.copy()
        S.set_field(B.F_TIMEBIN, pr.timebin)
        S.set_field(B.F_OLDACC, np.zeros(n))
        S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON_EWALD)
        out["acc"], out["cost"] = S.get_field(B.F_GRAVACCEL), S.get_field(B.F_GRAVCOST)
        out["let"] = [i["let_imported"] for i in S.each(lambda fp: fp.dd_info())]
        S.run.density(pr.g_dens())
        S.each(lambda fp: fp.update_hmax())
        S.run.hydro(pr.g_hydro())
        for k, f in SHARD_SPH:
            out[k] = S.get_field(getattr(B, f))[:pr.ngas]
        st = S.each(lambda fp: fp.stats())
        out["ngb_visits"] = sum(s["dens_neighbours"] for s in st)
        out["npairs"] = sum(s["hydro_pairs"] for s in st)
        out["dens_iterations"] = max(s["dens_iterations"] for s in st)
        info = S.each(lambda fp: fp.dd_info())
        out["ghosts"] = ([i["ghosts_imported"] for i in info], [i["ghosts_sent"] for i in info])
        # the sync point: bins by global index, the earliest bin on shard 1 alone
        tb = np.array([5, 6, 9], np.int32)[np.arange(n) % 3]
        tb[S.gid[1][::4]] = 3
        S.set_field(B.F_TIMEBIN, tb)
        sps = S.run.sync_point(8)
        out["sync_bins"] = tb
        out["sync"] = [{k: int(getattr(sp, k)) for k in ("Ti_next", "TimeBinActive", "GlobNumForceUpdate",
                                                         "Flag_FullStep", "NumForceUpdate")} for sp in sps]
        out["sync_ok"] = [SR.same_sync_point(sp, SR.next_sync_point(8, -1, tb[g], pr.ic["type"][g],
                                                                    others=[np.delete(tb, g)]))
                          for sp, g in zip(sps, S.gid)]
        out["active"] = [np.sort(g[fp.get_active()]) for fp, g in zip(S.fp, S.gid)]
        out["gid"] = [g.copy() for g in S.gid]
    finally:
        S.close()
    _SHARDS[L] = out
    return out


@pytest.mark.parametrize("L", PARITY)
def test_shards_full_step_parity_in_a_scaled_box(L):
    """P against the single-tree oracle with exact counts, as tests/test_gpu_dd.py, and against decomp_ref and
    sync_ref for the decomposition and the sync point"""
    import decomp_ref as DR
    import sync_ref as SR
    d = _shard_step(L)
    pr, ref = d["pr"], SC.oracle_cached(1, L)
    cost, tbin = d["work"]
    want, _, keys = DR.decompose(pr.ic["pos"], NSHARDS, 0, cost, tbin, domain=pr.extent)
    assert np.array_equal(keys, d["keys"]) and np.array_equal(d["splits"], want)
    for corner, center, ln in d["domain"]:          # the cube found on the device is the oracle's, bit for bit
        assert np.array_equal(corner, pr.extent[0]) and np.array_equal(center, pr.extent[1]) and ln == pr.extent[2]
    assert d["moved"] > 0 and min(np.bincount(d["owner"], minlength=NSHARDS)) > 0
    assert np.array_equal(d["cost"], ref["cost_ew_bh"][1]), "interaction counts differ from the single tree"
    assert relerr(d["acc"], ref["acc_ew_bh"][1]) < TOL
    assert all(x > 0 for x in d["let"]) and all(x > 0 for x in d["ghosts"][0])
    assert sum(d["ghosts"][0]) == sum(d["ghosts"][1])
    for k in SPH_COUNTS:
        assert d[k] == ref[k][1], k
    for k in SPH_REL:
        assert relerr(d[k], ref[k][1]) < TOL, k
    for k in SPH_MAX:
        assert _maxerr(d[k], ref[k][1]) < TOL, k
    single = SR.next_sync_point(8, -1, d["sync_bins"], pr.ic["type"])
    assert all(bad == [] for bad in d["sync_ok"]), d["sync_ok"]
    for r, sp in enumerate(d["sync"]):
        for key in ("Ti_next", "TimeBinActive", "GlobNumForceUpdate", "Flag_FullStep"):
            assert sp[key] == int(single[key]), (r, key)
        assert (sp["NumForceUpdate"] > 0) == (r == 1)
        g, tb = d["gid"][r], d["sync_bins"]
        assert np.array_equal(d["active"][r], np.sort(g[np.nonzero((single["TimeBinActive"] >> tb[g]) & 1)[0]]))
    assert sum(len(a) for a in d["active"]) == int((d["sync_bins"] == 3).sum()) > 0


@pytest.mark.parametrize("L", POW2)
def test_shards_full_step_follows_the_law(L):
    """S: keys, splits, every particle's owner, the counts and the sync point equal to the unit box's; the domain
    corner, centre and length x L exactly; the accelerations of the pair walk bit-identical (each target sums its
    own tree, then the imported ones in rank order); SPH to TOL as on one device"""
    u, s = _shard_step(1.0), _shard_step(L)
    assert np.array_equal(s["keys"], u["keys"]) and np.array_equal(s["splits"], u["splits"])
    assert np.array_equal(s["owner"], u["owner"]) and s["moved"] == u["moved"]
    for (c1, m1, l1), (c2, m2, l2) in zip(u["domain"], s["domain"]):
        assert np.array_equal(c2, L * c1) and np.array_equal(m2, L * m1) and l2 == L * l1
    assert np.array_equal(s["cost"], u["cost"]) and s["let"] == u["let"] and s["ghosts"] == u["ghosts"]
    assert off_law(s["acc"], u["acc"], "acc", L) == 0.0
    for k in SPH_COUNTS:
        assert s[k] == u[k], k
    for k, _ in SHARD_SPH:
        assert off_law(s[k], u[k], k, L) < TOL, (k, ROUNDED[k])
    assert s["sync"] == u["sync"] and all(np.array_equal(a, b) for a, b in zip(s["active"], u["active"]))


@pytest.mark.parametrize("L", BOTH)
def test_dust_density_on_shards_in_a_scaled_box(L):
    """P: GHIP_DD_DUST_DENSITY on 3 shards against dust_ref at the 1e-12 of test_gpu_dust_dd.py; grains crossed.
    At L = 4 and 2^17 also the law: equal to the unit box's, as on one device."""
    from test_gpu_dust import DustCase
    from test_gpu_dust_dd import DdDust, TOL as DTOL
    res = {}
    for box in [L] + ([1.0] if L in POW2 else []):
        case = DustCase(1, ndust=200, ng=8, box=box)
        T = DdDust(case, NSHARDS)
        try:
            d7, cnt = T.density()
        finally:
            T.S.close()
        sent = sum(int(c[0]) for c in cnt)
        assert sent > 0 and sent == sum(int(c[1]) for c in cnt)
        ref = case.ref_density()
        assert relerr(d7, ref) < DTOL and np.all(ref > 0)
        res[box] = (d7, [c.copy() for c in cnt])
    if L in POW2:
        assert np.array_equal(res[L][0], res[1.0][0])
        assert all(np.array_equal(a, b) for a, b in zip(res[L][1], res[1.0][1]))


@pytest.mark.parametrize("L", BOTH)
def test_fof_on_shards_in_a_scaled_box(L):
    """P: the FoF form on 3 shards for clumps(2000, True, box=L) against fof_ref with test_gpu_fof_dd.check (groups
    span shards and faces).  At L = 4 and 2^17 also the law: holders and the integer catalogue equal to the unit box's."""
    import fof_cases as FC
    import fof_ref as FR
    import test_gpu_fof_dd as TFD
    res = {}
    for box in [L] + ([1.0] if L in POW2 else []):
        c = FC.clumps(2000, True, box=box)
        S = TFD.FofShards(c, NSHARDS)
        try:
            g = TFD.check(S, S.fof(), FR.fof(**FC.ref_args(c)))
            res[box] = (g.copy(), S.holder.copy())
        finally:
            S.close()
    if L in POW2:
        (g, h), (g1, h1) = res[L], res[1.0]
        assert np.array_equal(h, h1)
        for k in ("Len", "Offset", "MinID", "GrNr", "LenType", "index_maxdens"):
            assert np.array_equal(g[k], g1[k]), k
        assert np.abs(g["CM"] - L * g1["CM"]).max() < TOL * L
