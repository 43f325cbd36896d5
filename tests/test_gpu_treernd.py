"""The randomised-subnode tree on the device (ghip_set_rnd_table: the reference without -DNOTREERND,
forcetree.c:208-232, 303-316) against the oracle's insertion tree -- whose `tiny_rng(index + depth)` is the
table tiny_rng(j) read with ID = index -- and, where the oracle cannot express the case (any table, any
IDs), against the trie of tests/treernd_ref.py.  States: the existing parity tests' smallest shapes with
groups of 2, 3, 5, 9 and 17 particles at one position and 20 pairs 1e-12 apart (treernd_ref.crowd).
Tolerances are those of the parity tests these mirror (tests/test_gpu_parity.py).
"""
import ctypes as C
import importlib

import numpy as np
import pytest

import treernd_ref as R
from common import O, Problem, bindings, ics, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-11
NTABLE = 262144
_TABLE = {}


def tiny():
    if "t" not in _TABLE:
        _TABLE["t"] = R.tiny_table(NTABLE)
    return _TABLE["t"]


def _all(n):
    return np.arange(n, dtype=np.int32)


def plummer_problem(gas_fraction=0.0, n=3000, scale=1.0, **kw):
    ic, pick = R.standard_state(n, gas_fraction=gas_fraction)
    pr = Problem(ic=ic, periodic=0, **kw)
    pr.force_soft = pr.force_soft * scale
    return pr, pick


def cosmo_problem(ng=12, periodic=1, gas_only=False, scale=1.0, crowd=None, **kw):
    ic = ics.make_ics(ng, gas=True, seed=12345, clustered=True)
    ic, pick = R.crowd(ic, among=np.arange(int(ic["ngas"])) if gas_only else None, **(crowd or {}))
    pr = Problem(ic=ic, periodic=periodic, **kw)
    pr.force_soft = pr.force_soft * scale      # x 1e-3: the crowd parts ten levels further down, below level 21
    return pr, pick


def device(pr, table=None, ids=None):
    """a context with the problem's particles, ID = index (or `ids`) and the table bound"""
    B = bindings()
    fp = pr.device()
    fp.set_field(B.F_ID, (np.arange(pr.n) if ids is None else ids).astype(np.uint32).view(np.int32))
    fp.set_rnd_table(tiny() if table is None else table)
    return fp


def element_fathers(lk):
    """father element of every element of a pre-order list with skip links"""
    fa = np.full(len(lk), -1, np.int64)
    stack = []
    for e in range(len(lk)):
        while stack and lk[stack[-1], 0] <= e:
            stack.pop()
        fa[e] = stack[-1] if stack else -1
        if lk[e, 1] < 0:
            stack.append(e)
    return fa


def assert_tree_is(d, od, numnodes, pos):
    """cells, moments, links and particle order as test_tree_cells_and_moments_match_the_insertion_tree"""
    nodes = d["lk"][:, 1] < 0
    print("device nodes %d, oracle nodes %d, deepest device level %d" %
          (nodes.sum(), numnodes, (-d["lk"][nodes][:, 1] - 1).max()))
    assert nodes.sum() == numnodes
    key_g = np.round(np.column_stack([d["cl"][nodes][:, 3], d["cl"][nodes][:, :3]]), 15)
    key_o = np.round(np.column_stack([od["len"], od["center"]]), 15)
    og = np.lexsort(key_g.T[::-1])
    oo = np.lexsort(key_o.T[::-1])
    assert np.array_equal(d["cl"][nodes][og][:, 3], od["len"][oo])
    assert np.array_equal(d["cl"][nodes][og][:, :3], od["center"][oo])
    assert np.allclose(d["xm"][nodes][og][:, 3], od["mass"][oo], rtol=1e-15, atol=0)
    assert np.allclose(d["xm"][nodes][og][:, :3], od["s"][oo], rtol=1e-14, atol=0)
    lk = d["lk"]
    for e in np.where(nodes)[0][:200]:
        inside = lk[e + 1:lk[e, 0]]
        assert (inside[:, 1] >= 0).sum() == lk[e, 3]
    part = lk[~nodes]
    assert np.array_equal(part[:, 1], np.arange(len(pos)))
    assert np.array_equal(d["xm"][~nodes][:, :3], pos[d["perm"]])
    # the particles' fathers are the oracle's cells
    fa = element_fathers(lk)
    fcell = np.empty((len(pos), 4))
    pe = np.where(~nodes)[0]
    fcell[d["perm"][lk[pe, 1]]] = d["cl"][fa[pe]][:, [3, 0, 1, 2]]
    n = len(pos)
    assert np.array_equal(fcell, np.column_stack([od["len"], od["center"]])[od["p_father"] - n])


# ------------------------------------------------------------------------------------------------
# the tree
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 1.0e-3])
def test_tree_with_coincident_particles_is_the_insertion_tree(scale):
    pr, _ = plummer_problem(scale=scale)
    fp = device(pr)
    pr.device_tree(fp)
    d = fp.tree_dump(0)
    T = pr.oracle_tree()
    assert T.numnodes == fp.stats()["tree_nodes"]
    assert_tree_is(d, T.dump(), T.numnodes, pr.ic["pos"])
    fp.close()


def test_without_a_table_identical_keys_stay_one_leaf():
    """the feature is off by default: the same state, no table -- not the oracle's tree"""
    pr, _ = plummer_problem()
    fp = pr.device()
    pr.device_tree(fp)
    T = pr.oracle_tree()
    assert fp.stats()["tree_nodes"] != T.numnodes
    # ... and binding, then unbinding, gives that tree again
    n0 = fp.stats()["tree_nodes"]
    fp.set_field(bindings().F_ID, np.arange(pr.n, dtype=np.int32))
    fp.set_rnd_table(tiny())
    pr.device_tree(fp)
    assert fp.stats()["tree_nodes"] == T.numnodes
    fp.set_rnd_table(None)
    pr.device_tree(fp)
    assert fp.stats()["tree_nodes"] == n0
    fp.close()


def test_gas_tree_with_coincident_gas_is_the_insertion_tree_of_the_gas():
    pr, _ = plummer_problem(gas_fraction=0.4, scale=1.0e-3)
    ng = pr.ngas
    rng = np.random.default_rng(1)
    pr.hsml0[:ng] *= 0.5 + rng.random(ng)
    fp = device(pr)
    pr.device_tree(fp)
    d = fp.tree_dump(1)
    ic = pr.ic
    T = O.Tree(ic["pos"][:ng], ic["vel"][:ng], ic["mass"][:ng], ic["type"][:ng], pr.force_soft,
               hsml=pr.hsml0[:ng], extent=pr.extent)
    assert_tree_is(d, T.dump(), T.numnodes, ic["pos"][:ng])
    lk, aux = d["lk"], d["aux"]
    hs = pr.hsml0[d["perm"]]
    for e in np.where(lk[:, 1] < 0)[0]:
        assert aux[e] == hs[lk[e, 2]:lk[e, 2] + lk[e, 3]].max()
    fp.close()


def test_any_table_and_ids_give_the_trie_of_the_definition():
    """a numpy.random table of 262144 entries, shuffled IDs of which some are >= ntable"""
    pr, _ = plummer_problem(scale=1.0e-3)
    rng = np.random.default_rng(11)
    table = rng.random(NTABLE)
    ids = rng.permutation(pr.n).astype(np.uint64) * 173 + 7
    ids[::3] += NTABLE                      # beyond the table ...
    ids[::7] = 2 ** 32 - 1 - ids[::7]       # ... and near the 32-bit wrap of ID + depth
    ids = ids.astype(np.uint32)
    assert len(np.unique(ids)) == pr.n and (ids >= NTABLE).sum() > pr.n // 4
    fp = device(pr, table, ids)
    pr.device_tree(fp)
    d = fp.tree_dump(0)
    tr = R.build(pr.ic["pos"], ids, pr.ic["type"], pr.force_soft, table, pr.extent)
    nodes = d["lk"][:, 1] < 0
    got = d["cl"][nodes][:, [3, 0, 1, 2]]
    want = np.asarray(tr.cells)
    assert len(got) == len(want)
    assert np.array_equal(got[np.lexsort(got.T[::-1])], want[np.lexsort(want.T[::-1])])
    fa = element_fathers(d["lk"])
    pe = np.where(~nodes)[0]
    fcell = np.empty((pr.n, 4))
    fcell[d["perm"][d["lk"][pe, 1]]] = d["cl"][fa[pe]][:, [3, 0, 1, 2]]
    assert np.array_equal(fcell, tr.father_cells())
    fp.close()


def test_threshold_follows_the_type_with_unequal_softenings():
    """two types, softenings 1 : 4, coincident particles of both in one cell: each starts to randomise at
    its own depth"""
    pr, pick = plummer_problem(gas_fraction=0.5, scale=1.0e-3, unequal=True)
    assert pr.force_soft[0] != pr.force_soft[1]
    typ = pr.ic["type"]
    assert len(set(typ[pick[10:19]])) == 2 and len(set(typ[pick[19:36]])) == 2   # the groups of 9 and 17 mix
    fp = device(pr)
    pr.device_tree(fp)
    d = fp.tree_dump(0)
    T = pr.oracle_tree()
    assert_tree_is(d, T.dump(), T.numnodes, pr.ic["pos"])
    fp.close()


# ------------------------------------------------------------------------------------------------
# walks
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic,scale", [(0, 1.0), (1, 1.0), (0, 1.0e-3)])
def test_gravity_two_pass_on_the_randomised_tree(periodic, scale):
    """test_gravity_two_pass_parity on a state with coincident particles: both opening criteria, the
    Ewald walk with periodic = 1; Ninteractions / GravCost exactly the oracle's.  Softening x 1e-3: the
    walks meet nodes of levels 22 .. 29 and chains of ancestors that long."""
    B = bindings()
    pr, _ = cosmo_problem(12, periodic, scale=scale)
    fp = device(pr)
    pr.device_tree(fp)
    T = pr.oracle_tree()
    assert fp.stats()["tree_nodes"] == T.numnodes
    assert (T.dump()["len"].min() < pr.extent[2] * 2.0 ** -22) == (scale < 1)
    tg = _all(pr.n)
    tab = O.ewald_table(pr.box) if periodic else None
    old = np.zeros(pr.n)
    for theta in (pr.theta, 0.0):
        fp.set_field(B.F_OLDACC, old)
        fp.gravity(pr.g_grav(theta), B.WALK_NEWTON)
        oacc, ocost = T.gravity(pr.o_grav(theta), tg, old)
        assert np.array_equal(fp.get_field(B.F_GRAVCOST), ocost)
        assert relerr(fp.get_field(B.F_GRAVACCEL), oacc) < TOL
        if periodic:
            fp.gravity(pr.g_grav(theta), B.WALK_EWALD)
            T.gravity_ewald_add(pr.o_grav(theta), tab, tg, old, oacc, ocost)
            assert np.array_equal(fp.get_field(B.F_GRAVCOST), ocost)
            assert relerr(fp.get_field(B.F_GRAVACCEL), oacc) < TOL
        st = fp.stats()
        assert st["grav_interactions"] + st["ewald_interactions"] == int(ocost.sum())
        fp.gravity_finish(pr.G * 3.0)
        old = np.linalg.norm(oacc, axis=1)
        assert relerr(fp.get_field(B.F_OLDACC), old) < TOL
    fp.close()


def test_shortrange_walk_on_the_randomised_tree():
    B = bindings()
    pr, _ = cosmo_problem(12, 1)
    asmth = 1.25 * pr.box / 16
    rcut = 4.5 * asmth
    fp = device(pr)
    pr.device_tree(fp)
    T = pr.oracle_tree()
    tg = _all(pr.n)
    old = np.full(pr.n, 3.0)
    for theta in (pr.theta, 0.0):
        fp.set_field(B.F_OLDACC, old)
        fp.gravity(pr.g_grav(theta, rcut, asmth), B.WALK_SHORTRANGE)
        oacc, ocost = T.gravity(pr.o_grav(theta, rcut=rcut, asmth=asmth), tg, old, kind="shortrange")
        assert np.array_equal(fp.get_field(B.F_GRAVCOST), ocost)
        assert relerr(fp.get_field(B.F_GRAVACCEL), oacc) < TOL
    fp.close()


@pytest.mark.parametrize("periodic,scale", [(1, 1.0), (0, 1.0), (0, 1.0e-3)])
def test_density_and_hydro_on_coincident_gas(periodic, scale):
    """test_density_and_hydro_parity with a crowd among the gas: the h iteration's count, the neighbour
    visits and the pair count are the oracle's on its insertion tree (softening x 1e-3: a gas tree with
    nodes below level 21).  The crowd is 12 coincident pairs and 20 pairs 1e-12 apart: a gas particle at
    r = 0 adds 32/3 to the weighted neighbour number whatever h is, so with four or more at one position
    no h gives DesNumNgb +- MaxNumNgbDeviation = 33 +- 2 and the reference itself ends in endrun(1155)."""
    B = bindings()
    pr, _ = cosmo_problem(12, periodic, gas_only=True, scale=scale, crowd=dict(groups=(2,) * 12, npairs=20))
    fp = device(pr)
    pr.device_tree(fp)
    T = pr.oracle_tree()
    act = _all(pr.ngas)
    od = T.density(pr.o_dens(), act, pr.velpred, pr.entropy, pr.dtentropy, pr.timebin, pr.ti_begstep, pr.hsml0)
    T.update_hmax(act, od["hsml"], od["divvel"])
    oh = T.hydro(pr.o_hydro(), act, pr.velpred, od["hsml"], od["density"], od["pressure"], od["dhsmlfac"],
                 od["divvel"], od["curlvel"], pr.timebin)
    fp.density(pr.g_dens())
    st = fp.stats()
    assert st["gastree_nodes"] > 0
    assert 1 < od["iterations"] < 150
    assert st["dens_iterations"] == od["iterations"]
    assert st["dens_neighbours"] == od["ngb_visits"]
    ng = pr.ngas
    assert relerr(fp.get_field(B.F_HSML)[:ng], od["hsml"][:ng]) < TOL
    for fid, name in ((B.F_NUMNGB, "numngb"), (B.F_DENSITY, "density"), (B.F_DHSMLFAC, "dhsmlfac"),
                      (B.F_PRESSURE, "pressure")):
        assert relerr(fp.get_field(fid), od[name][:ng]) < TOL, name
    for fid, name in ((B.F_DIVVEL, "divvel"), (B.F_CURLVEL, "curlvel")):
        got, want = fp.get_field(fid), od[name][:ng]
        assert np.abs(got - want).max() < TOL * np.abs(want).max(), name
    fp.update_hmax()
    fp.hydro(pr.g_hydro())
    assert fp.stats()["hydro_pairs"] == oh["npairs"]
    ha = fp.get_field(B.F_HYDROACCEL)
    assert np.abs(ha - oh["hydroaccel"][:ng]).max() < TOL * np.abs(oh["hydroaccel"]).max()
    de = fp.get_field(B.F_DTENTROPY)
    assert np.abs(de - oh["dtentropy"][:ng]).max() < TOL * np.abs(oh["dtentropy"]).max()
    assert relerr(fp.get_field(B.F_MAXSIGNALVEL), oh["maxsignalvel"][:ng]) < TOL
    fp.close()


def test_ngb_treefind_around_crowded_spots():
    """ghip_ngb_treefind on the deep gas tree, centred on coincident gas: the oracle's lists"""
    pr, pick = cosmo_problem(12, 1, gas_only=True)
    fp = device(pr)
    pr.device_tree(fp)
    T = pr.oracle_tree()
    for t in (pick[0], pick[5], pick[19], pick[40]):
        c = pr.ic["pos"][t]
        for h in (pr.hsml0[t], 1.0e-9):
            lst, cnt = fp.ngb_treefind(c, h, 0, 1, pr.box)
            assert cnt == len(lst)
            assert np.array_equal(np.sort(lst), np.sort(T.ngb_variable(c, h, 1, pr.box)))
        lst, cnt = fp.ngb_treefind(c, pr.hsml0[t], 1, 1, pr.box)
        assert np.array_equal(np.sort(lst), np.sort(T.ngb_pairs(c, pr.hsml0[t], pr.hsml0, 1, pr.box)))
    fp.close()


# ------------------------------------------------------------------------------------------------
# export, sub-steps, the host mirror
# ------------------------------------------------------------------------------------------------
def test_exported_randomised_tree_is_the_reference_representation():
    """test_exported_tree_is_the_reference_representation on the crowded state, softening x 1e-3"""
    B = bindings()
    ic, _ = R.crowd(ics.make_plummer(4000, gas_fraction=0.4))
    pr = Problem(ic=ic, periodic=0, unequal=True)
    pr.force_soft = pr.force_soft * 1.0e-3
    n, ng = pr.n, pr.ngas
    rng = np.random.default_rng(2)
    hs = pr.hsml0.copy()
    hs[:ng] *= 0.5 + rng.random(ng)
    divv = rng.standard_normal(ng)
    fp = device(pr)
    fp.set_field(B.F_HSML, hs)
    fp.set_field(B.F_DIVVEL, divv)
    pr.device_tree(fp)
    maxpart = n + 100
    nodes, ext, nxt, fat = fp.tree_export(maxpart=maxpart, ti_current=7, unequal=1)
    dvfull = np.zeros(n)
    dvfull[:ng] = divv
    T = O.Tree(ic["pos"], ic["vel"], ic["mass"], ic["type"], pr.force_soft, hsml=hs, divvel=dvfull,
               extent=pr.extent)
    od = T.dump()
    assert len(nodes) == T.numnodes
    assert nodes["len"].min() < pr.extent[2] * 2.0 ** -22          # nodes below level 21 are among them
    key_g = np.column_stack([nodes["len"], nodes["center"]])
    key_o = np.column_stack([od["len"], od["center"]])
    og, oo = np.lexsort(key_g.T[::-1]), np.lexsort(key_o.T[::-1])
    assert np.array_equal(key_g[og], key_o[oo])
    o2g = np.empty(T.numnodes, np.int64)
    o2g[oo] = og

    def conv(idx):
        idx = np.asarray(idx, np.int64)
        out = idx.copy()
        isnode = idx >= n
        out[isnode] = maxpart + o2g[idx[isnode] - n]
        return out

    g = nodes[o2g]
    x = ext[o2g]
    assert np.allclose(g["mass"], od["mass"], rtol=1e-15, atol=0)
    assert np.allclose(g["s"], od["s"], rtol=1e-14, atol=0)
    assert np.allclose(x["vs"], od["vs"], rtol=1e-13, atol=1e-16)
    assert np.array_equal(x["vmax"], od["vmax"])
    assert np.array_equal(x["hmax"], od["hmax"]) and np.array_equal(x["divVmax"], od["divvmax"])
    assert np.array_equal((g["bitflags"] >> 7) & 1, od["multi"])
    soft_of_type = pr.force_soft[(g["bitflags"] >> 2) & 7]
    assert np.array_equal(soft_of_type, od["maxsoft"])
    assert np.array_equal((g["bitflags"] >> 5) & 1, od["mixedsoft"])
    assert np.array_equal(g["sibling"], conv(od["sibling"]))
    assert np.array_equal(g["nextnode"], conv(od["nextnode"]))
    assert np.array_equal(g["father"], conv(od["father"]))
    assert np.array_equal(nxt[:n], conv(od["p_nextnode"]))
    assert np.array_equal(fat[:n], conv(od["p_father"]))
    fp.close()


def test_one_substep_on_the_kept_randomised_tree():
    """the kept tree of a full build with a table bound, kicked and drifted once (forcetree.c:1356-1520):
    interaction counts of the sub-step are the oracle's on its drifted insertion tree"""
    B = bindings()
    pr, _ = cosmo_problem(10, 0)
    n = pr.n
    rng = np.random.default_rng(17)
    c, ce, ln = pr.extent
    pr.extent = (c - 0.05 * ln, ce.copy(), 1.1 * ln)
    ext = (pr.extent[0], pr.extent[1], pr.extent[2], pr.force_soft)
    pos, vel = pr.ic["pos"].copy(), pr.ic["vel"].copy()
    fp = device(pr)
    fp.set_dynamic_tree(True)
    fp.tree_build(*ext)
    T = O.Tree(pos, vel, pr.ic["mass"], pr.ic["type"], pr.force_soft, hsml=pr.hsml0, extent=pr.extent)
    assert fp.stats()["tree_nodes"] == T.numnodes
    everybody = _all(n)
    fp.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
    a0, c0 = T.gravity(pr.o_grav(pr.theta), everybody, np.zeros(n))
    assert np.array_equal(fp.get_field(B.F_GRAVCOST), c0)
    old = np.linalg.norm(a0, axis=1)
    fp.set_field(B.F_OLDACC, old)
    vscale = np.abs(vel).max()
    act = np.sort(rng.choice(n, n // 3, replace=False)).astype(np.int32)
    dv = 0.1 * vscale * rng.standard_normal((len(act), 3))
    T.vel[act] += dv
    T.kick_nodes(act, dv)
    fp.set_field(B.F_VEL, T.vel)
    fp.tree_kick_nodes(act, dv)
    dt = 0.004 * pr.box / vscale
    T.pos += T.vel * dt
    T.drift_nodes(dt)
    fp.set_field(B.F_POS, T.pos)
    fp.tree_substep(dt)
    d = fp.tree_dump_dynamic()
    assert (d["lk"][:, 1] < 0).sum() == T.numnodes
    fp.gravity(pr.g_grav(0.0), B.WALK_NEWTON)
    oa, oc = T.gravity(pr.o_grav(0.0), everybody, old)
    assert np.array_equal(fp.get_field(B.F_GRAVCOST), oc)
    assert relerr(fp.get_field(B.F_GRAVACCEL), oa) < TOL
    fp.close()


def test_force_treebuild_with_a_bound_rndtable_fills_the_hosts_arrays_with_the_oracles_tree():
    H = importlib.import_module("gadget-leicester_amd.hostapi")
    B = bindings()
    pr, _ = cosmo_problem(8, 0)
    n = pr.n
    host = H.Host(periodic=0)
    P = np.zeros(n, H.P_DTYPE)
    S = np.zeros(pr.ngas, H.SPH_DTYPE)
    P["Pos"], P["Vel"], P["Mass"], P["Type"] = pr.ic["pos"], pr.ic["vel"], pr.ic["mass"], pr.ic["type"]
    P["ID"] = np.arange(n)
    P["TimeBin"], P["Ti_begstep"] = pr.timebin, pr.ti_begstep
    S["VelPred"], S["Entropy"], S["DtEntropy"] = pr.velpred, pr.entropy, pr.dtentropy
    S["Hsml"] = pr.hsml0[:pr.ngas]
    host.set_particles(P, S)
    A = host.All
    A.G, A.ErrTolTheta, A.ErrTolForceAcc, A.TypeOfOpeningCriterion = pr.G, pr.theta, pr.ErrTolForceAcc, 1
    A.BoxSize, A.DesNumNgb, A.MaxNumNgbDeviation = pr.box, pr.des_ngb, pr.max_dev
    A.ArtBulkViscConst, A.Ti_Current, A.Timebase_interval = pr.visc, pr.ti_current, pr.timebase
    A.ComovingIntegrationOn, A.MinGasHsmlFractional = 0, 0.0
    eps = pr.force_soft[0] / 2.8
    for name in ("Gas", "Halo", "Disk", "Bulge", "Stars", "Bndry"):
        setattr(A, "Softening" + name, eps)
    host.L.set_softenings()
    host.set_active(None)
    corner, center, dlen = host.domain()             # the domain the mirror found is the oracle's
    L = host.L
    A.MaxPart = n
    maxnodes = 2 * n
    nodes = np.zeros(maxnodes, B.NODE_DTYPE)
    ext = np.zeros(maxnodes, B.EXTNODE_DTYPE)
    nxt = np.full(n, -1, np.int32)
    fat = np.full(n, -1, np.int32)
    for name, arr in (("Nodes_base", nodes), ("Extnodes_base", ext), ("Nextnode", nxt), ("Father", fat)):
        C.c_void_p.in_dll(L, name).value = arr.ctypes.data
    C.c_int.in_dll(L, "MaxNodes").value = maxnodes
    soft = np.array(A.ForceSoftening[:])
    T = O.Tree(pr.ic["pos"], pr.ic["vel"], pr.ic["mass"], pr.ic["type"], soft, hsml=pr.hsml0,
               extent=(corner, center, dlen))
    od = T.dump()
    plain = L.force_treebuild(n, None)
    assert host.endrun_codes == [] and plain != T.numnodes                # no table: the level-21 leaves
    table = tiny().copy()
    host.bind_rndtable(table)
    numnodes = L.force_treebuild(n, None)
    assert host.endrun_codes == [] and numnodes == T.numnodes
    key_g = np.column_stack([nodes["len"][:numnodes], nodes["center"][:numnodes]])
    key_o = np.column_stack([od["len"], od["center"]])
    og, oo = np.lexsort(key_g.T[::-1]), np.lexsort(key_o.T[::-1])
    assert np.array_equal(key_g[og], key_o[oo])
    o2g = np.empty(T.numnodes, np.int64)
    o2g[oo] = og
    conv = lambda idx: np.where(np.asarray(idx) >= n, n + o2g[np.maximum(np.asarray(idx, np.int64) - n, 0)], idx)
    assert np.array_equal(fat, conv(od["p_father"]))
    assert np.array_equal(nxt, conv(od["p_nextnode"]))
    assert np.array_equal(nodes["sibling"][:numnodes][o2g], conv(od["sibling"]))
    # the host refills its table every step: the next build reads the new values
    table[:] = np.random.default_rng(5).random(NTABLE)
    n2 = L.force_treebuild(n, None)
    tr = R.build(pr.ic["pos"], np.arange(n), pr.ic["type"], soft, table, (corner, center, dlen))
    assert host.endrun_codes == [] and n2 == tr.numnodes
    host.bind_rndtable(None)
    assert L.force_treebuild(n, None) == plain
    host.close()


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def test_domain_decomposed_operations_refuse_a_bound_table():
    B = bindings()
    pr, _ = plummer_problem()
    fp = pr.device()
    fp.dd_init(0, 1)
    fp.dd_set_domain(pr.extent[0], pr.extent[1], pr.extent[2], pr.force_soft)
    fp.set_rnd_table(tiny())
    with pytest.raises(B.GhipError) as e:
        fp.dd_begin(B.DD_GRAVITY, pr.g_grav(pr.theta), B.WALK_NEWTON)
    assert B.GHIP_ERRORS[e.value.code] == "GHIP_EINVAL" and "ghip_set_rnd_table" in str(e.value)
    fp.set_rnd_table(None)
    fp.dd_begin(B.DD_GRAVITY, pr.g_grav(pr.theta), B.WALK_NEWTON)       # without a table: as ever
    fp.close()


def test_paths_deeper_than_the_key_words_fail_the_build_and_leave_the_context_usable():
    """softening x 1e-9: identical positions part only below 2^-50 of the domain; two key words hold 42
    levels.  An error return (the tree error), not a fault; the next build on the same context works."""
    B = bindings()
    pr, _ = plummer_problem()
    fp = device(pr)
    assert 42 <= fp.tree_max_level() < 50      # (a library whose paths reach level 50 builds this state)
    good = pr.force_soft
    with pytest.raises(B.GhipError) as e:
        fp.tree_build(pr.extent[0], pr.extent[1], pr.extent[2], good * 1.0e-9)
        fp.stats()
    assert B.GHIP_ERRORS[e.value.code] == "GHIP_EDEVICE" and "tree error" in str(e.value)
    fp.tree_build(pr.extent[0], pr.extent[1], pr.extent[2], good)
    T = pr.oracle_tree()
    assert fp.stats()["tree_nodes"] == T.numnodes
    fp.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
    _, ocost = T.gravity(pr.o_grav(pr.theta), _all(pr.n), np.zeros(pr.n))
    assert np.array_equal(fp.get_field(B.F_GRAVCOST), ocost)
    # ... also when the build that fails is an asynchronous one (same particle number as the last)
    with pytest.raises(B.GhipError) as e:
        fp.tree_build(pr.extent[0], pr.extent[1], pr.extent[2], good * 1.0e-9)
        fp.stats()
    assert "tree error" in str(e.value)
    fp.tree_build(pr.extent[0], pr.extent[1], pr.extent[2], good)
    assert fp.stats()["tree_nodes"] == T.numnodes
    fp.close()
