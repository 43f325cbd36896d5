"""ghip_fof on the device against tests/fof_ref.py (fof.c restated, pinned in tests/test_fof_cpu.py): labels, GrNr,
Len, LenType, MinID, Offset, index_maxdens, the ID list and Ngroups / Nids / largest exactly; Mass, MassType, CM,
Vel and MaxDens -- sums taken in another order -- within 1e-11 of the largest magnitude of the compared array (for
CM: of the box or the extent), the bound of tests/test_gpu_dd.py for such sums."""
import numpy as np
import pytest

import fof_cases as FC
import fof_ref as FR
import treernd_ref
from common import bindings

pytestmark = pytest.mark.gpu

TOL = 1e-11
_REF = {}


def extent(pos):
    """domain_findExtent (domain.c:1972-2014) of a particle set; a single point gets a cube of side 1"""
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    ln = 1.001 * float((hi - lo).max())
    if not ln > 0:
        ln = 1.0
    center = 0.5 * (lo + hi)
    return center - 0.5 * ln, center, ln


def device(c, ids=True, tree=True, table=None):
    B = bindings()
    fp = B.ForcePath(0)
    n = len(c["pos"])
    fp.set_counts(n, c["ngas"])
    fp.set_field(B.F_POS, c["pos"])
    fp.set_field(B.F_VEL, c["vel"])
    fp.set_field(B.F_MASS, c["mass"])
    fp.set_field(B.F_TYPE, c["type"])
    fp.set_field(B.F_HSML, c["hsml"])
    if c["ngas"]:
        fp.set_field(B.F_DENSITY, c["density"])
    if ids:
        fp.set_field(B.F_ID, c["ids"])
    if table is not None:
        fp.set_rnd_table(table)
    if tree:
        fp.tree_build(*extent(c["pos"]), np.full(6, 1e-3 * c["linkl"]))
    return fp


def call(fp, c, **over):
    a = dict(link_length=c["linkl"], primary_types=c["primary_types"], secondary_types=c["secondary_types"],
             group_min_len=c["group_min_len"], boxsize=c["box"], periodic=c["periodic"], max_iter=c["max_iter"])
    a.update(over)
    return fp.fof(**a)


def reference(key, c, **over):
    """tests/fof_ref.py on a case, computed once per key and shared (nobody changes it).  The labels do not depend
    on group_min_len: a key (name, ..., min_len) shares them with (name, ..., 1) and only compiles its catalogue."""
    if key not in _REF:
        base = key[:-1] + (1,) if isinstance(key, tuple) and key[0] == "clumps" else None
        if base is not None and base != key:
            r1 = reference(base, dict(c, group_min_len=1))
            r = FR.catalogue(c["pos"], c["vel"], c["mass"], c["type"].astype(np.int64), c["ids"].astype(np.int64),
                             c["density"], c["ngas"], r1["label"], c["group_min_len"], c["box"], c["periodic"])
            r.update(LinkL=r1["LinkL"], nearest_iterations=r1["nearest_iterations"])
            _REF[key] = r
        else:
            _REF[key] = FR.fof(**FC.ref_args(c, **over))
    return _REF[key]


def check(fp, res, c, ref):
    """everything the call left behind against the reference's; returns the measured errors"""
    G = ref["groups"]
    assert (res.Ngroups, res.Nids, res.largest) == (ref["Ngroups"], ref["Nids"], ref["largest"])
    assert res.nearest_iterations == ref["nearest_iterations"]
    minid, grnr = fp.fof_labels()
    assert np.array_equal(minid, ref["label"]), "labels differ at %s" % np.where(minid != ref["label"])[0][:10]
    assert np.array_equal(grnr, ref["grnr"])
    assert np.array_equal(fp.fof_ids(), ref["ids"])
    g = fp.fof_groups()
    assert len(g) == ref["Ngroups"]
    for k in ("Len", "Offset", "MinID", "GrNr", "LenType", "index_maxdens"):
        assert np.array_equal(g[k], G[k]), k
    err = {}
    span = c["box"] if c["periodic"] else max(extent(c["pos"])[2], np.abs(c["pos"]).max())
    for k in ("Mass", "MassType", "CM", "Vel", "MaxDens"):
        if len(g) == 0:
            continue
        top = span if k == "CM" else max(np.abs(G[k]).max(), 1e-300)
        err[k] = float(np.abs(g[k] - G[k]).max() / top)
        assert err[k] <= TOL, (k, err)
    if c["periodic"] and len(g):
        assert np.all((g["CM"] >= 0) & (g["CM"] < c["box"]))
    print(err)
    return g


@pytest.mark.parametrize("min_len", [1, 32])
@pytest.mark.parametrize("periodic", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 777, 66000])
def test_sizes(n, periodic, min_len):
    c = FC.clumps(n, periodic)
    c["group_min_len"] = min_len
    fp = device(c)
    res = call(fp, c)
    check(fp, res, c, reference(("clumps", n, periodic, min_len), c))
    if n == 66000:
        assert res.Ngroups > 100 if min_len == 32 else res.Ngroups > 20000
    fp.close()


def test_equality_links():
    c = FC.lattice(0.25)
    fp = device(c)
    res = call(fp, c)
    assert (res.Ngroups, res.largest) == (1, 64)
    check(fp, res, c, reference("lattice", c))
    c1 = FC.lattice(np.nextafter(0.25, 0))
    res = call(fp, c1)
    assert (res.Ngroups, res.largest) == (64, 1)
    check(fp, res, c1, reference("lattice-", c1))
    fp.close()


@pytest.mark.parametrize("across_face", [False, True])
def test_long_chain(across_face):
    c = FC.chain(across_face)
    fp = device(c)
    res = call(fp, c)
    assert (res.Ngroups, res.largest, res.Nids) == (1, 4097, 4097)
    check(fp, res, c, reference(("chain", across_face), c))
    fp.close()


def test_bridge():
    for with_bridge, want in ((True, [81]), (False, [40, 40])):
        c = FC.bridge(with_bridge)
        fp = device(c)
        res = call(fp, c)
        g = check(fp, res, c, reference(("bridge", with_bridge), c))
        assert g["Len"].tolist() == want
        fp.close()


@pytest.mark.parametrize("table", [False, True])
def test_coincident_primaries(table):
    c = FC.coincident()
    fp = device(c, table=treernd_ref.tiny_table(4096) if table else None)
    res = call(fp, c)
    check(fp, res, c, reference("coincident", c))
    minid, _ = fp.fof_labels()
    assert minid[5] == minid[11] == minid[23] == c["ids"][[5, 11, 23]].min()
    fp.close()


def test_secondaries():
    c = FC.secondary_rounds([0, 1, 3, 12])
    fp = device(c)
    res = call(fp, c)
    assert res.nearest_iterations == 12
    check(fp, res, c, reference("rounds", c))
    minid, _ = fp.fof_labels()
    assert minid[0] == c["ids"][3] and np.all(minid[4:] == c["ids"][1:3].min())   # gas -> the far group; stars
    for k in (0, 1, 3):
        ck = FC.secondary_rounds([k])
        fk = device(ck)
        assert call(fk, ck).nearest_iterations == k
        fk.close()
    B = bindings()
    with pytest.raises(B.GhipError) as e:
        call(fp, c, max_iter=2)
    assert B.GHIP_ERRORS.get(e.value.code) == "GHIP_ENOCONV"
    res = call(fp, c)                                    # the context still works
    check(fp, res, c, reference("rounds", c))
    fp.close()


def test_equidistant_primaries_the_smaller_id_wins():
    c = FC.equidistant()
    fp = device(c)
    res = call(fp, c)
    check(fp, res, c, reference("equidistant", c))
    assert fp.fof_labels()[0].tolist() == [20, 30, 20, 30]
    fp.close()


def test_catalogue_order_and_the_periodic_corner():
    c = FC.equal_len()
    fp = device(c)
    res = call(fp, c)
    g = check(fp, res, c, reference("equal_len", c))
    assert g["Len"].tolist() == [5] * 6 + [3] * 3
    assert np.all(np.diff(g["MinID"][:6]) > 0) and np.all(np.diff(g["MinID"][6:]) > 0)
    _, grnr = fp.fof_labels()
    corner = [k for k in range(9) if np.ptp(c["pos"][grnr == k], axis=0).max() > 0.5]
    assert len(corner) == 1
    cm = g["CM"][corner[0]]
    assert np.all((cm >= 0) & (cm < 1.0)) and np.all(np.minimum(cm, 1.0 - cm) < 0.01)
    fp.close()


def test_two_calls_give_the_same_bytes():
    c = FC.clumps(66000, True)
    fp = device(c)
    call(fp, c)
    a, ia, la = fp.fof_groups().tobytes(), fp.fof_ids().tobytes(), fp.fof_labels()
    call(fp, c)
    assert fp.fof_groups().tobytes() == a and fp.fof_ids().tobytes() == ia
    assert np.array_equal(fp.fof_labels()[0], la[0]) and np.array_equal(fp.fof_labels()[1], la[1])
    fp.close()


def test_linklength_rule():
    c = FC.clumps(777, True)
    rhodm = 0.7 * c["mass"][c["type"] == 1].sum() / c["box"] ** 3
    want = FR.linklength_rule(c["mass"], c["type"], c["primary_types"], 0.2, rhodm)
    fp = device(c)
    res = call(fp, c, link_length=0.0, linklength=0.2, rhodm=rhodm)
    assert abs(res.LinkL / want - 1) <= 1e-14, (res.LinkL, want)
    c2 = dict(c, linkl=want)
    check(fp, res, c2, reference("rule", c2))
    fp.close()


def test_refusals_leave_the_context_usable():
    B = bindings()
    c = FC.clumps(777, True)

    def refused(fp, what, **over):
        with pytest.raises(B.GhipError) as e:
            call(fp, c, **over)
        assert B.GHIP_ERRORS.get(e.value.code) == "GHIP_EINVAL" and what in str(e.value), str(e.value)

    fp = device(c, tree=False)
    refused(fp, "ghip_tree_build")                       # no tree built
    fp.tree_build(*extent(c["pos"]), np.full(6, 1e-3 * c["linkl"]))
    refused(fp, "primary", primary_types=8)              # no particle of a primary type
    refused(fp, "primary", primary_types=0)
    check(fp, call(fp, c), c, reference(("clumps", 777, True, 1), c))
    fp.close()
    fp = device(c, ids=False)
    refused(fp, "ID")                                    # no ID field set
    fp.set_field(B.F_ID, c["ids"])
    fp.tree_build(*extent(c["pos"]), np.full(6, 1e-3 * c["linkl"]))
    check(fp, call(fp, c), c, reference(("clumps", 777, True, 1), c))
    fp.close()
    fp = device(c, tree=False)
    fp.dd_init(0, 1)                                     # a domain decomposition on
    refused(fp, "shard")
    assert np.array_equal(fp.get_field(B.F_ID), c["ids"])    # (a shard stays a shard: its other calls still work)
    fp.close()
