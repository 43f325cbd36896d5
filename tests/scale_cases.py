"""Problems in boxes that are not the unit cube, and the law their results follow.

A problem is rescaled by L at fixed time, density and G: lengths and velocities x L, masses x L^3, specific energies
and the entropic function x L^2.  Every pass of the code is covariant under that map; LAW gives the exponent of L
that each output picks up.  For L a power of two the map commutes with every fp64 operation that is not a pow(), a
cube root or a sum of free order, so the outputs of such passes are bit-identical after the law is applied; for any
other L they agree to rounding.

tests/test_box_scale_cpu.py holds the references to the law, tests/test_gpu_box_scale.py the device."""
import copy

import numpy as np

POW2 = [4.0, 2.0 ** 17]
ODD = 2.5
SCALES = POW2 + [ODD]


def SHIFT(L):
    """where an open problem goes: negative coordinates, a domain corner that is not the origin"""
    return L * np.array([-3.0, 5.0, -0.5])


# output name -> exponent of L
LAW = {}
LAW.update(dict.fromkeys(("acc", "hydroaccel", "hsml", "maxsignalvel", "cm", "linkl", "corner", "center", "len",
                          "pos", "vel", "gasvel", "gravpm", "s"), 1))
LAW.update(dict.fromkeys(("potential", "entropy", "dtentropy", "u"), 2))
LAW.update(dict.fromkeys(("mass",), 3))
LAW.update(dict.fromkeys(("momentum",), 4))
LAW.update(dict.fromkeys(("density", "divvel", "curlvel", "dhsmlfac", "numngb", "cost",
                          "iterations", "ngb_visits", "npairs", "nodes", "label", "len_group", "minid", "grnr", "ids",
                          "keys", "splits", "owner", "timebin", "marks", "counts"), 0))
# P = A rho^gamma with the entropic function A x L^2 and the density fixed: the pressure carries L^2 (and the hydro
# acceleration grad P / rho one power of L)
LAW["pressure"] = 2


def law(name, unit, L):
    """the unit-box result `unit` of the output `name`, as the box of size L must give it"""
    e = LAW[name]
    return unit if e == 0 else np.asarray(unit) * float(L) ** e


def rescaled(ic, L, shift=None):
    """the ics dict `ic` in a box L times as large: positions, velocities and the spacing x L, masses x L^3, u x L^2;
    shift (open problems only) is added to the scaled positions.  A periodic coordinate that rounds to >= box goes
    to 0, as ics.make_ics does in the unit box."""
    L = float(L)
    box = float(ic["boxsize"]) * L
    out = dict(ic)
    pos = np.ascontiguousarray(ic["pos"] * L)
    if shift is not None:
        pos = np.ascontiguousarray(pos + np.asarray(shift, np.float64)[None, :])
    else:
        pos[pos >= box] = 0.0
    out["pos"] = pos
    out["vel"] = np.ascontiguousarray(ic["vel"] * L)
    out["mass"] = ic["mass"] * L ** 3
    out["boxsize"] = box
    out["spacing"] = ic["spacing"] * L
    if "u" in ic:
        out["u"] = ic["u"] * L ** 2
    return out


def rescale_problem(pr, L, shift=None):
    """common.Problem `pr` (built in the unit box, left unchanged) in the box of size L: the particle set through
    rescaled(), and what the constructor draws unscaled brought along -- velpred x L, entropy and dtentropy x L^2,
    hsml0, the softenings and MinGasHsml x L.  Time bins, tolerances and the neighbour number stay.  The domain
    cube is that of the scaled positions."""
    from common import O
    assert shift is None or not pr.periodic, "only an open problem can be shifted"
    L = float(L)
    q = copy.copy(pr)
    q.ic = rescaled(pr.ic, L, shift)
    q.box = float(q.ic["boxsize"])
    q.force_soft = pr.force_soft * L
    q.min_gas_hsml = pr.min_gas_hsml * L
    q.hsml0 = pr.hsml0 * L
    q.velpred = pr.velpred * L
    q.entropy = pr.entropy * L ** 2
    q.dtentropy = pr.dtentropy * L ** 2
    q.timebin = pr.timebin.copy()
    q.ti_begstep = pr.ti_begstep.copy()
    q.extent = O.domain_extent(q.ic["pos"])
    q.L = L * getattr(pr, "L", 1.0)
    return q


# ------------------------------------------------------------------------------------------------
# one step of the oracle on a problem, every output under the name of its law
# ------------------------------------------------------------------------------------------------
PMGRID = 16
_UNIT = {}
_ORACLE = {}


def unit_problem(periodic, unequal=True):
    """the ng = 8, seed 3 problem (512 gas + 512 DM) of these tests in the unit box, built once"""
    from common import Problem, ics
    key = (int(periodic), bool(unequal))
    if key not in _UNIT:
        _UNIT[key] = Problem(ic=ics.make_ics(8, gas=True, seed=3), periodic=periodic, unequal=unequal, seed=3)
        _UNIT[key].L = 1.0
    return _UNIT[key]


def problem(periodic, L, shifted=False):
    """unit_problem in the box of size L; shifted (open only): moved by SHIFT(L) as well"""
    pr = unit_problem(periodic)
    if L == 1.0 and not shifted:
        return pr
    return rescale_problem(pr, L, SHIFT(L) if shifted else None)


def asmth_of(pr):
    return 1.25 * pr.box / PMGRID          # ASMTH * BoxSize / PMGRID (pm_periodic.c:83-84)


def oracle_step(pr):
    """{key: (law name, value)} of one step of the oracle on `pr`: the Barnes-Hut pass, the relative pass on its
    |acc|, for a periodic problem the Ewald add to both, the short-range walk and the mesh force, then density and
    hydro.  The old accelerations of the short-range walk are 3 L."""
    from common import O
    n, ng = pr.n, pr.ngas
    T = pr.oracle_tree()
    tg = np.arange(n, dtype=np.int32)
    out = {"nodes": ("nodes", T.numnodes)}
    old = np.zeros(n)
    tab = O.ewald_table(pr.box) if pr.periodic else None
    for name, theta in (("bh", pr.theta), ("rel", 0.0)):
        acc, cost = T.gravity(pr.o_grav(theta), tg, old)
        out["acc_" + name], out["cost_" + name] = ("acc", acc.copy()), ("cost", cost.copy())
        if pr.periodic:
            T.gravity_ewald_add(pr.o_grav(theta), tab, tg, old, acc, cost)
            out["acc_ew_" + name], out["cost_ew_" + name] = ("acc", acc), ("cost", cost)
        old = np.linalg.norm(acc, axis=1)
        out["old_" + name] = ("acc", old)
    if pr.periodic:
        a = asmth_of(pr)
        acc, cost = T.gravity(pr.o_grav(pr.theta, rcut=4.5 * a, asmth=a), tg, np.full(n, 3.0 * getattr(pr, "L", 1.0)), kind="shortrange")
        out["acc_sr"], out["cost_sr"] = ("acc", acc), ("cost", cost)
        out["gravpm"] = ("gravpm", O.pm_periodic(pr.ic["pos"], pr.ic["mass"], pr.box, pr.G, PMGRID))
    act = np.arange(ng, dtype=np.int32)
    od = T.density(pr.o_dens(), act, pr.velpred, pr.entropy, pr.dtentropy, pr.timebin, pr.ti_begstep, pr.hsml0)
    for k in ("hsml", "numngb", "density", "dhsmlfac", "divvel", "curlvel", "pressure"):
        out[k] = (k, od[k][:ng])
    out["dens_iterations"], out["ngb_visits"] = ("iterations", od["iterations"]), ("ngb_visits", od["ngb_visits"])
    T.update_hmax(act, od["hsml"], od["divvel"])
    oh = T.hydro(pr.o_hydro(), act, pr.velpred, od["hsml"], od["density"], od["pressure"], od["dhsmlfac"],
                 od["divvel"], od["curlvel"], pr.timebin)
    for k in ("hydroaccel", "dtentropy", "maxsignalvel"):
        out[k] = (k, oh[k][:ng])
    out["npairs"] = ("npairs", oh["npairs"])
    return out


def oracle_cached(periodic, L, shifted=False):
    """oracle_step(problem(periodic, L, shifted)), computed once and shared: nobody changes it"""
    key = (int(periodic), float(L), bool(shifted))
    if key not in _ORACLE:
        _ORACLE[key] = oracle_step(problem(periodic, L, shifted))
    return _ORACLE[key]


def digest(obj):
    """sha256 over everything a case builder made: the arrays (dtype, shape, bytes), numbers and strings of a dict or
    of an object's members, in the order of the sorted names, nested cases included"""
    import hashlib
    h = hashlib.sha256()

    def feed(x, seen):
        if isinstance(x, np.ndarray):
            h.update(("%s%s" % (x.dtype.str, x.shape)).encode())
            h.update(np.ascontiguousarray(x).tobytes())
        elif isinstance(x, (bool, int, float, str, np.generic)) or x is None:
            h.update(repr(x.item() if isinstance(x, np.generic) else x).encode())
        elif isinstance(x, (list, tuple)):
            h.update(b"[")
            for y in x:
                feed(y, seen)
        elif isinstance(x, dict) or hasattr(x, "__dict__"):
            if id(x) in seen:
                return
            seen = seen | {id(x)}
            d = x if isinstance(x, dict) else vars(x)
            for k in sorted(d, key=str):
                h.update(str(k).encode())
                feed(d[k], seen)
        else:
            raise TypeError("digest: %r" % type(x))
    feed(obj, frozenset())
    return h.hexdigest()


def is_count(v):
    return isinstance(v, (int, np.integer)) or np.asarray(v).dtype.kind in "iu"


def off_law(got, unit, lawname, L):
    """max |got - law(unit)| over the field, in units of the field's largest magnitude (0.0: bit-identical)"""
    want = law(lawname, unit, L)
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if np.array_equal(got, want):
        return 0.0
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


# ------------------------------------------------------------------------------------------------
# sinks, dust, wind and friends-of-friends in a box of size L
# ------------------------------------------------------------------------------------------------
SINK_SWITCHES = [(0, 0), (1, 1)]       # (accretion_of_dust_only, accretion_density): gas by energy / dust only
_SINKS = {}


def sink_setup(L, periodic=1):
    """SinkProblem(ng=8, box=L) with its second sink moved to 0.3 spacings from the face x = 0 (its search sphere of
    about 2.6 spacings wraps), and, as common.sink_case leaves them, sp.gas_density and sp.dens (the density pass of
    tests/sink_ref.py).  No candidate lies within 1e-9 of a decision threshold (common.sink_ties), so marks and
    counts are decided, not luck.  A fresh copy per call: the passes change masses."""
    from common import O, SinkProblem, sink_ref_density, sink_ties
    key = (float(L), int(periodic))
    if key not in _SINKS:
        sp = SinkProblem(ng=8, periodic=periodic, box=L)
        pr = sp.pr
        near = sp.sinks[1]
        pr.ic["pos"][near] = float(L) * np.array([0.3 / 8, 0.37, 0.61])
        pr.extent = O.domain_extent(pr.ic["pos"])
        sp.gas_density = 0.5 + np.random.default_rng(3).random(pr.ngas)
        sp.dens = sink_ref_density(sp)
        assert sp.dens["iterations"] >= 1
        assert sp.dens["hsml"][near] > 4 * pr.ic["pos"][near, 0], "the sink's sphere does not reach the face"
        assert sink_ties(sp, sp.dens) == 0
        _SINKS[key] = sp
    return copy.deepcopy(_SINKS[key])


_SINK_REFS = {}


def sink_refs(L, periodic, switches):
    """what common.sink_reference makes for a named case, for sink_setup(L, periodic): tests/sink_ref.py's marks
    under the project's rule and its swallow pass on them (computed once, changed by nobody)"""
    import sink_ref
    from common import sink_over, sink_ref_par
    key = (float(L), int(periodic), tuple(switches))
    if key not in _SINK_REFS:
        sp = sink_setup(L, periodic)
        ic, pr, d = sp.pr.ic, sp.pr, sp.dens
        over = sink_over(*switches)
        par = sink_ref_par(sp, **over)
        a = (ic["pos"], ic["vel"], ic["mass"], ic["type"], sp.ids, sp.sinks, d["hsml"])
        sw, inj = sink_ref.evaluate(*a, pr.timebin, sp.mdot, d["density"], sp.gas_density, par, rule="max")
        _SINK_REFS[key] = dict(par=par, over=over, sw=sw, inj=inj,
                               swallow=sink_ref.swallow(*a, sw, sp.bh_mass, par))
    return _SINK_REFS[key]


def fof_rescaled(c, L, shift=None):
    """a case of tests/fof_cases.py under the map of the law: positions, velocities, Hsml, LinkL and the box x L,
    masses x L^3 (the gas densities stay); shift: added to the positions of an open case"""
    L = float(L)
    out = dict(c)
    pos = c["pos"] * L
    if shift is not None:
        assert not c["periodic"]
        pos = pos + np.asarray(shift, np.float64)[None, :]
    elif c["periodic"]:
        pos[pos >= c["box"] * L] = 0.0
    out.update(pos=np.ascontiguousarray(pos), vel=c["vel"] * L, mass=c["mass"] * L ** 3, hsml=c["hsml"] * L,
               linkl=c["linkl"] * L, box=c["box"] * L)
    return out
