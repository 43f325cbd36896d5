"""CPU checks of the dust model (ghip_set_dust_model: DUST_GROWTH, DUST_REAL_PEBBLE_COLLISIONS, DUST_VAPORIZE,
DUST_FE_AND_ICE_GRAINS, DUST_EPSTEIN, DUST_NO_FRICTION_HEATING): the new names are exported and the Python mirrors
have the libraries' struct sizes; with every switch off the reference of tests/dust_model_ref.py is dust_ref.py bit
for bit; its rules give values computed here from the formulas; and the case the GPU tests run reaches every branch."""
import ctypes as C
import importlib
import os
import re

import numpy as np

import dust_model_case as DC
import dust_model_ref as MR
import dust_ref as R
from common import REPO, bindings, pkg


# ---- 1. exports and layouts ----------------------------------------------------------------------
def test_libraries_export_the_dust_model_and_mirrors_have_their_sizes():
    L = C.CDLL(pkg.lib_path())
    B = bindings()
    for name in ("ghip_set_dust_model", "ghip_dust_model_size", "ghip_dust_grains_size",
                 "ghip_dust_density_grains", "ghip_dust_drag_grains"):
        assert hasattr(L, name), name
        assert name in B.EXPORTS
    lib = B.lib()
    assert C.sizeof(B.DustModel) == lib.ghip_dust_model_size() == 6 * 4 + 5 * 8
    assert C.sizeof(B.DustGrains) == lib.ghip_dust_grains_size()
    assert C.sizeof(B.DdDustGrainsArgs) == C.sizeof(C.c_void_p) + C.sizeof(B.DustGrains)
    assert B.DUST_GRAINS_FORM == 1 and re.search(r"#define\s+GHIP_DUST_GRAINS_FORM\s+1\b", open(os.path.join(REPO, "include", "ghip.h")).read())
    H = importlib.import_module("gadget-leicester_amd.hostapi")
    assert hasattr(H.lib(), "gadget_force_bind_dust_model")
    assert "gadget_force_bind_dust_model" in H.EXPORTS
    assert C.sizeof(H.DustModelLayout) == 11 * C.sizeof(C.c_int)


# ---- 2. flags off --------------------------------------------------------------------------------
def test_every_switch_off_is_dust_ref_bit_for_bit():
    c = DC.case(1)
    m = MR.model()
    assert not any(m[k] for k in MR.SWITCHES)
    d7, d9 = c.ref_density9(m)
    assert d9 is None and np.array_equal(d7, c.ref_density())
    sel = np.arange(len(c.dust))
    got, ref = c.ref_model(m, d7=d7), c.ref_grains(sel, d7)
    for k in ("vel", "d9", "dmom", "de", "vcoll", "regime"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["radius"], c.radius) and np.array_equal(got["logr"], c.logr0)


# ---- 3. independent pins -------------------------------------------------------------------------
PAR = R.params(1.0, 1, 1e-3)


def test_growth_rate_is_d7_vcoll_over_twelve_grain_densities():
    m = MR.model("growth")
    a, d7, vc = 7.0, 2.5, 3.0                      # cm, code density, m/s
    vc_code = vc * 1.e2 / PAR["UnitVelocity_in_cm_per_s"]
    rho_grain_code = 3.0 / PAR["UnitDensity_in_cgs"]
    t_coll, adot = MR.growth_rate(PAR, m, a, d7, vc)
    assert abs(adot / (d7 * vc_code / (12 * rho_grain_code)) - 1) < 1e-14
    assert abs(t_coll / (a / PAR["UnitLength_in_cm"] / (3 * adot)) - 1) < 1e-14


def test_fragmentation_factor():
    a, d7 = 7.0, 2.5
    grow = MR.growth_rate(PAR, MR.model("growth"), a, d7, 10.0)[1]
    peb = lambda vc, vf: MR.growth_rate(PAR, MR.model("growth", "real_pebble_collisions",
                                                      FragmentationVelocity=vf), a, d7, vc)[1]
    assert peb(10.0, 10.0) == 0.0                  # x = 1
    assert peb(10.0, 5.0) == grow * ((1 - 4.0) / (1 + 4.0)) < 0         # x = 2: fragmentation
    assert peb(10.0, 20.0) == grow * ((1 - 0.25) / (1 + 0.25)) > 0      # x = 1/2
    assert peb(10.0, 0.0999) == 0.0 and peb(1e-3, 0.05) == 0.0         # FragmentationVelocity < 0.1
    assert peb(10.0, 0.1) < 0


def test_rock_vapour_at_1717_kelvin():
    rho, ent = 1.5e-3, 0.0936
    cs2 = 8. / np.pi * ent * rho ** 0.4
    T = np.pi / 8. * cs2 * PAR["UnitVelocity_in_cm_per_s"] ** 2 * 2.3 * 1.6726e-24 / 1.3806e-16
    pvap = 10. ** (13.176 - 24605. / T)
    assert abs(T - 1717) < 1 and abs(pvap - 0.0705) < 5e-4
    Tr, pr, term = MR.vapour(PAR, rho, ent, False)
    assert abs(Tr / T - 1) < 1e-13 and abs(pr / pvap - 1) < 1e-13
    uv = PAR["UnitVelocity_in_cm_per_s"]
    assert abs(term / (pvap / (3.0 * np.sqrt(6.283) * np.sqrt(cs2) * uv * uv)) - 1) < 1e-13


def test_ice_vapour_below_and_above_600_kelvin():
    rho = 1.5e-3
    for ent, cold in ((0.0156, True), (0.0936, False)):
        T = np.pi / 8. * (8. / np.pi * ent * rho ** 0.4) * PAR["UnitVelocity_in_cm_per_s"] ** 2 * \
            2.3 * 1.6726e-24 / 1.3806e-16
        assert (T <= 600.) == cold
        want = 10. ** (11.6 - 2104. / T) if cold else 5. + 5.2e-3 * T
        Ti, pi_, _ = MR.vapour(PAR, rho, ent, True)
        assert abs(Ti / T - 1) < 1e-13 and abs(pi_ / want - 1) < 1e-13
        assert pi_ != MR.vapour(PAR, rho, ent, False)[1]


def test_latent_heat_has_the_sign_of_the_radius_change():
    m = MR.model("growth", "vaporize", InitialDustRadius=1.0)
    L = lambda a, ice=False: MR.latent_heat(m, a, ice)
    assert L(2.0) - L(1.0) > 0 > L(0.5) - L(1.0) and L(1.0) - L(1.0) == 0.0
    assert L(1.0) == 1.e11 and L(1.0, True) == 4.e10 and L(0.1) == 0.0
    # ... and so has what a grain hands to the gas: one grain, no dt (no friction), clamped up from below
    one = lambda radius: MR.grain_update(PAR, m, np.zeros((1, 3)), np.ones(1), np.zeros((1, 3)), np.zeros(1),
                                         np.array([1.5e-3]), np.array([0.0156]), np.zeros((1, 3)),
                                         np.array([radius]), np.ones(1), np.zeros((1, 3)), np.ones(1))
    up, same = one(0.05), one(3.0)
    assert up["radius"][0] == 0.1 and up["de"][0] > 0 and up["lo"][0]
    assert same["radius"][0] == 3.0 and same["de"][0] == 0.0


# ---- 4. the case reaches every branch ------------------------------------------------------------
def test_the_case_reaches_every_branch():
    for periodic in (0, 1):
        c = DC.case(periodic)
        assert len(c.dust) == 600
        m = c.model(*DC.ALL_SIX)
        r = c.ref_model(m)
        dt, d7 = c.dt(), c.base()[0]
        shrink = r["vap"] * dt * c.par["UnitLength_in_cm"]      # cm the vapour term takes off in this step
        rock = ~r["ice"]
        census = {
            "gate passes with d7 > 0": r["gate"] & (d7 > 0),
            "dt == 0": dt == 0,
            "x < 1": r["x"] < 1,
            "x > 1": r["x"] > 1,
            "rock, negligible vapour": rock & (dt > 0) & (shrink < 1e-12 * c.radius),
            "rock, vapour shrinks by more than 1 %": rock & (shrink > 0.01 * c.radius),
            "ice": r["ice"],
            "ice above 600 K": r["ice"] & (r["T"] > 600),
            "ice at or below 600 K": r["ice"] & (r["T"] <= 600),
            "lower clamp binds": r["lo"],
            "upper clamp binds": r["hi"],
            "a radius moves without reaching a clamp": ~r["lo"] & ~r["hi"] & (r["radius"] != c.radius),
        }
        for what, mask in census.items():
            assert mask.sum() >= 5, (what, int(mask.sum()))
        still = (dt == 0) & (c.radius < 0.1)
        assert still.sum() >= 1 and np.all(r["radius"][still] == 0.1) and np.all(r["lo"][still])
        assert np.all(r["regime"][dt > 0] == R.EPSTEIN)                 # (epstein is one of the six)
        grown = c.ref_model(c.model("growth", "vaporize"))
        assert np.all(np.bincount(grown["regime"], minlength=6) >= 5)   # without it, every stopping-time regime
        # the quirk of dust.c:437-444: t_coll is formed with the DustVcoll the dynamics block leaves
        moved = (dt > 0) & r["gate"]
        t_first = MR.growth_rate(c.par, m, c.radius[moved][0], d7[moved][0], r["vcoll"][moved][0])[0]
        assert r["logr"][moved][0] == t_first
        # closed gates: nothing grows, log_radius_by_dt keeps the caller's values, the clamps still act
        for over in (dict(Time=0.5, VirtualTime=0.5), dict(Time=0.0, VirtualTime=-1.0)):
            g = c.ref_model(c.model("growth", **over))
            assert not g["gate"].any() and np.array_equal(g["logr"], c.logr0)
            assert np.array_equal(g["radius"], np.clip(c.radius, 0.1, 1e5)) and g["lo"].sum() >= 1
