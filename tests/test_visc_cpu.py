"""The all-pairs numpy reference of the viscosity switches (tests/visc_ref.py) anchored to the oracle, its
own properties, and the ABI of the viscosity mode (ghip_set_viscosity, gadget_force_bind_viscosity).
No GPU needed."""
import ctypes as C
import importlib

import numpy as np
import pytest

import visc_ref as VR
from common import Problem, bindings

COMOVING = (1, 0.37, 0.81, 1.9)      # the tuple of test_density_and_hydro_parity
ANCHOR_TOL = 1e-12                   # of the field's largest magnitude (measured: <= 3.7e-15)


def _all(n):
    return np.arange(n, dtype=np.int32)


_CACHE = {}


def oracle_state(periodic=1, timebase=None, comoving=None):
    """Problem(ng=8) after the oracle's density(): (pr, density results, oracle hydro results), made once"""
    key = (periodic, timebase, comoving)
    if key not in _CACHE:
        pr = Problem(ng=8, gas=True, periodic=periodic)
        if timebase is not None:
            pr.timebase = timebase            # (before the density: it enters the pressure prediction)
        T = pr.oracle_tree()
        act = _all(pr.ngas)
        od = T.density(pr.o_dens(), act, pr.velpred, pr.entropy, pr.dtentropy, pr.timebin, pr.ti_begstep,
                       pr.hsml0)
        T.update_hmax(act, od["hsml"], od["divvel"])
        hp = pr.o_hydro(*comoving) if comoving else pr.o_hydro()
        oh = T.hydro(hp, act, pr.velpred, od["hsml"], od["density"], od["pressure"], od["dhsmlfac"],
                     od["divvel"], od["curlvel"], pr.timebin)
        _CACHE[key] = (pr, od, oh, hp)
    return _CACHE[key]


def _moved(a, b):
    """largest difference in units of b's largest magnitude"""
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


# ---- 1. anchor ------------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic,timebase,comoving", [(1, None, None), (0, None, None), (1, None, COMOVING),
                                                       (1, 1.0, None)])
def test_reference_reproduces_the_oracle(periodic, timebase, comoving):
    pr, od, oh, hp = oracle_state(periodic, timebase, comoving)
    ng = pr.ngas
    ref = VR.hydro(pr, od, np.full(ng, pr.visc), VR.params(ArtBulkViscConst=pr.visc), hp)
    assert ref["npairs"] == oh["npairs"]
    for k in ("hydroaccel", "dtentropy", "maxsignalvel"):
        d = _moved(ref[k], oh[k][:ng])
        print(k, d)
        assert d < ANCHOR_TOL, k
    if timebase == 1.0:
        # the limiter of hydra.c:1583-1595 binds (it never does at Problem's timebase = 1e-3)
        print("limited", ref["nlimited"], "of", ref["napproach"])
        assert 4 * ref["nlimited"] >= ref["napproach"] > 0
    else:
        assert ref["napproach"] > 0


def test_time_dependent_with_constant_alpha_is_the_constant_case():
    pr, od, oh, hp = oracle_state()
    ref = VR.hydro(pr, od, np.full(pr.ngas, pr.visc), VR.params(time_dependent=1, ArtBulkViscConst=pr.visc), hp)
    for k in ("hydroaccel", "dtentropy", "maxsignalvel"):
        assert _moved(ref[k], oh[k][:pr.ngas]) < ANCHOR_TOL, k


# ---- 2. the switches do something ---------------------------------------------------------------
def test_varying_alpha_moves_the_force():
    pr, od, oh, hp = oracle_state()
    ng = pr.ngas
    alpha = 0.1 + 0.7 * np.random.default_rng(7).random(ng)
    ref = VR.hydro(pr, od, alpha, VR.params(time_dependent=1, ArtBulkViscConst=0.8), hp)
    assert ref["npairs"] == oh["npairs"]
    assert _moved(ref["hydroaccel"], oh["hydroaccel"][:ng]) > 0.01      # measured: 12 %
    assert _moved(ref["dtentropy"], oh["dtentropy"][:ng]) > 0.01        # measured: 47 %


def test_no_limiter_moves_the_force_where_the_limiter_binds():
    pr, od, oh, hp = oracle_state(1, 1.0)
    ng = pr.ngas
    ref = VR.hydro(pr, od, np.full(ng, pr.visc), VR.params(ArtBulkViscConst=pr.visc, no_limiter=1), hp)
    assert ref["npairs"] == oh["npairs"] and ref["nlimited"] == 0
    assert _moved(ref["hydroaccel"], oh["hydroaccel"][:ng]) > 0.01      # measured: 24 %
    assert _moved(ref["maxsignalvel"], oh["maxsignalvel"][:ng]) < ANCHOR_TOL


@pytest.mark.parametrize("switch", ["conventional", "no_shear_limiter"])
def test_other_uniform_switches_are_not_rounding_noise(switch):
    """at Problem's own timebase (the limiter never binds and cannot mask them): a change a million times the
    anchor tolerance is no rounding effect"""
    pr, od, oh, hp = oracle_state()
    ng = pr.ngas
    ref = VR.hydro(pr, od, np.full(ng, pr.visc), VR.params(ArtBulkViscConst=pr.visc, **{switch: 1}), hp)
    assert ref["npairs"] == oh["npairs"]
    print(switch, _moved(ref["hydroaccel"], oh["hydroaccel"][:ng]), _moved(ref["dtentropy"], oh["dtentropy"][:ng]))
    assert _moved(ref["hydroaccel"], oh["hydroaccel"][:ng]) > 1e6 * ANCHOR_TOL
    assert _moved(ref["dtentropy"], oh["dtentropy"][:ng]) > 1e6 * ANCHOR_TOL
    if switch == "conventional":       # hydra.c:1520 takes the conventional mu_ij too
        assert _moved(ref["maxsignalvel"], oh["maxsignalvel"][:ng]) > 1e6 * ANCHOR_TOL
    else:
        assert _moved(ref["maxsignalvel"], oh["maxsignalvel"][:ng]) < ANCHOR_TOL


# ---- 3. kick_alpha --------------------------------------------------------------------------------
def test_kick_alpha_clamps_and_leaves_alpha_alone_without_a_rate():
    V = VR.params(ArtBulkViscConst=0.8, AlphaMin=0.1)
    alpha = np.array([0.3, 0.75, 0.15, 0.8, 0.1])
    rate = np.array([1.0, 5.0, -5.0, 3.0, -2.0])
    got = VR.kick_alpha(alpha, rate, 0.02, V)
    assert got[0] == 0.3 + 1.0 * 0.02
    assert got[1] == 0.8 and got[3] == 0.8          # upper clamp, timestep.c:531
    assert got[2] == 0.1 and got[4] == 0.1          # lower clamp, timestep.c:532-533
    a = 0.1 + 0.7 * np.random.default_rng(3).random(100)
    assert np.array_equal(VR.kick_alpha(a, np.zeros(100), 0.37, V).view(np.uint64), a.view(np.uint64))


# ---- 4. dtalpha -----------------------------------------------------------------------------------
def test_dtalpha_source_decay_and_comoving_division():
    rng = np.random.default_rng(5)
    n = 64
    pres, rho, h = 1 + rng.random(n), 1 + rng.random(n), 0.1 + rng.random(n)
    curl, vsig = rng.random(n), 1 + rng.random(n)
    alpha = 0.1 + 0.7 * rng.random(n)
    V = VR.params(AlphaMin=0.1, ViscSource=0.9, DecayTime=0.7, dtalpha_comoving_div=2.5)
    # expansion or rest: no source, pure decay towards AlphaMin (hydra.c:739-741)
    div_pos = np.concatenate([rng.random(n // 2), np.zeros(n // 2)])
    d = VR.dtalpha(pres, rho, h, div_pos, curl, vsig, alpha, V, fac_mu=1.3)
    want = -(alpha - 0.1) * 0.7 * 0.5 * vsig / (h * 1.3)
    assert np.array_equal(d, want)
    assert (d[alpha > 0.1] < 0).all()
    at_min = VR.dtalpha(pres, rho, h, div_pos, curl, vsig, np.full(n, 0.1), V)
    assert (at_min == 0).all()
    # compression: the source is f ViscSource |div v| > 0 on top of the same decay
    div_neg = -(0.1 + rng.random(n))
    dc = VR.dtalpha(pres, rho, h, div_neg, curl, vsig, alpha, V, fac_mu=1.3)
    src = dc - want
    f = src / (0.9 * -div_neg)
    assert (src > 0).all() and (f > 0).all() and (f < 1).all()
    no_shear = VR.dtalpha(pres, rho, h, div_neg, np.zeros(n), vsig, alpha, V, fac_mu=1.3) - want
    assert (no_shear >= src).all()             # curl suppresses the source (Balsara factor)
    # hydra.c:742-743
    assert np.array_equal(VR.dtalpha(pres, rho, h, div_neg, curl, vsig, alpha, V, fac_mu=1.3, comoving=1),
                          dc / 2.5)


def test_derive_is_begrun_as_written():
    vs, dt = VR.derive(2.0, 4.0)
    g = 7.0 / 5.0
    assert vs == 2.0 / np.log((g + 1) / (g - 1))
    assert dt == 1 / 4.0 * np.sqrt((g - 1) / 2 * g)
    assert bindings().visc_derive(2.0, 4.0) == pytest.approx((vs, dt), rel=1e-15)


# ---- 5. ABI ---------------------------------------------------------------------------------------
def test_libraries_export_the_viscosity_entry_points():
    B = bindings()
    L = B.lib()
    for name in ("ghip_set_viscosity", "ghip_visc_set_alpha", "ghip_visc_get", "ghip_visc_derive"):
        assert hasattr(L, name), name
    assert C.sizeof(B.ViscParams) == L.ghip_visc_params_size()
    H = importlib.import_module("gadget-leicester_amd.hostapi")
    assert hasattr(H.lib(), "gadget_force_bind_viscosity")
    assert C.sizeof(H.ViscLayout) == 9 * C.sizeof(C.c_int)
