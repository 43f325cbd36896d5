"""CPU checks of cooling_and_starformation with DoCooling and the drag heating (ghip_sfr_cooling): the
new C-ABI symbols are exported, ghip_sfr_params has the layout its Python mirror assumes, and the numpy
restatement the GPU tests compare against (tests/sfr_ref.py) is pinned -- to the oracle where the
cooling function is the identity, and by hand for the closed forms, the order of the terms and the
Mass == 0 quirks."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import sfr_ref as R
from common import O, REPO, bindings, pkg


def test_libghip_exports_the_sfr_cooling_pass():
    L = C.CDLL(pkg.lib_path())
    B = bindings()
    for name in ("ghip_sfr_cooling", "ghip_find_smbh"):
        assert hasattr(L, name), name
        assert name in B.EXPORTS
    B.lib()   # argtypes of every export resolve
    assert (B.COOL_NONE, B.COOL_ISOTHERM, B.COOL_EVAPORATION, B.COOL_EVAPORATION_RADIAL, B.COOL_BETA) == \
        (R.NONE, R.ISOTHERM, R.EVAPORATION, R.EVAPORATION_RADIAL, R.BETA)


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ghip.h"
int main(void)
{
  printf("%zu %zu %zu %zu %zu %zu %d %d %d %d %d\n", sizeof(ghip_sfr_params),
         offsetof(ghip_sfr_params, comoving), offsetof(ghip_sfr_params, Timebase_interval),
         offsetof(ghip_sfr_params, OriginalGasMass), offsetof(ghip_sfr_params, Evap_dens),
         offsetof(ghip_sfr_params, smbh_pos), GHIP_COOL_NONE, GHIP_COOL_ISOTHERM, GHIP_COOL_EVAPORATION,
         GHIP_COOL_EVAPORATION_RADIAL, GHIP_COOL_BETA);
  return 0;
}
"""


def test_sfr_params_match_the_python_mirror(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler to build the layout probe")
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    B = bindings()
    S = B.SfrParams
    assert got == [C.sizeof(S), S.comoving.offset, S.Timebase_interval.offset, S.OriginalGasMass.offset,
                   S.Evap_dens.offset, S.smbh_pos.offset, B.COOL_NONE, B.COOL_ISOTHERM,
                   B.COOL_EVAPORATION, B.COOL_EVAPORATION_RADIAL, B.COOL_BETA]
    assert got[0] == 4 * 4 + 15 * 8 + 3 * 8


def _particles(seed=4, ngas=400, nother=120):
    rng = np.random.default_rng(seed)
    n = ngas + nother
    ptype = np.zeros(n, np.int32)
    ptype[ngas:] = rng.choice([1, 2, 5], nother)
    pos = rng.random((n, 3)) - 0.5
    mass = np.full(n, 1e-6)
    mass[rng.choice(ngas, 6, replace=False)] = 0.0
    timebin = rng.integers(0, 5, n).astype(np.int32)
    dens = 0.2 + 3.0 * rng.random(ngas)
    ent = 0.05 * (1 + 0.2 * rng.random(ngas))
    dte = 1e-3 * rng.standard_normal(ngas)
    inj = np.where(rng.random(ngas) < 0.3, 1e-9 * rng.random(ngas), 0.0)
    return dict(ptype=ptype, pos=pos, mass=mass, timebin=timebin, density=dens, entropy=ent, dtentropy=dte,
                injected=inj, rng=rng, n=n, ngas=ngas)


def test_identity_cooling_reproduces_the_oracle_bit_for_bit():
    """cooling NONE, dust 0, the origin as centre: O.cooling_and_starformation, bit for bit"""
    d = _particles()
    p = R.params(cooling=R.NONE, dust=0, CritPhysDensity_code=2.5, MinEgySpec=0.05, Timebase_interval=1e-3)
    inj = d["injected"].copy()
    inj[3] = 1e3                                               # runs into the 5e9 K ceiling
    act = d["rng"].permutation(d["n"]).astype(np.int32)[: d["n"] // 2 + 50]
    od, oi, of = O.cooling_and_starformation(act, d["ngas"], d["ptype"], d["mass"], d["timebin"],
                                             p["Timebase_interval"], p["CritPhysDensity_code"],
                                             p["MinEgySpec"], R.u_to_temp(p), d["density"], d["entropy"],
                                             d["dtentropy"], inj)
    r = R.sfr_cooling(p, act, d["ngas"], d["ptype"], d["pos"], d["mass"], d["timebin"], d["density"],
                      d["entropy"], d["dtentropy"], inj)
    assert np.array_equal(r["dtentropy"], od) and not np.array_equal(od, d["dtentropy"])
    assert np.array_equal(r["injected"], oi)
    want = np.array([i for i in act if i < d["ngas"] and of[i]], np.int32)
    assert 0 < len(want) and np.array_equal(r["cand"], want)


@pytest.mark.parametrize("variant", [R.EVAPORATION, R.EVAPORATION_RADIAL, R.BETA])
def test_no_step_is_the_identity(variant):
    p = R.params(cooling=variant, beta_tapper_off=1)
    for u, rho, r2 in ((3.7e-3, 1.0, 0.3), (1.0, 1e-9, 4.0), (2e5, 50.0, 1e-4)):
        assert R.do_cooling(p, u, rho, 0.0, r2) == u


@pytest.mark.parametrize("variant", [R.EVAPORATION, R.EVAPORATION_RADIAL, R.BETA])
def test_a_long_step_relaxes_to_the_equilibrium(variant):
    p = R.params(cooling=variant)
    u2t = R.u_to_temp(p)
    for rho, r2 in ((1e-3, 0.3), (2.0, 4.0)):
        r = math.sqrt(r2)
        u_eq = {R.EVAPORATION: p["EqTemp"] / u2t,
                R.EVAPORATION_RADIAL: p["EqTemp"] / u2t / (r ** p["Cool_ind"] + 1e-10),
                R.BETA: p["EqTemp"] / u2t / (r ** 0.5 + 1e-10)}[variant]
        got = R.do_cooling(p, 123.0 * u_eq, rho, 1e30, r2)
        assert abs(got - u_eq) <= 1e-12 * u_eq


def test_isotherm_is_exactly_the_equilibrium_energy():
    p = R.params(cooling=R.ISOTHERM)
    u_eq = p["EqTemp"] / R.u_to_temp(p)
    for u in (0.0, 1e-7, 5.0, 1e9):
        assert R.do_cooling(p, u, 0.7, 3.0, 2.0) == u_eq


def test_one_particle_by_hand_with_the_shipped_parameters():
    """MeanWeight 2.45, BetaCool 5, EquilibriumTemp 20, Cool_ind 0.5, Evap_dens 2e-11: a gas particle at
    r = 2 from the SMBH, at the density where rho / Evap_dens = 1 (tcool = 5 (1 + 1) = 10), a step of
    dt = 10 (dt / tcool = 1: unew = (u_old + u_eq) / 2)"""
    p = R.params(dust=0, Timebase_interval=5.0, smbh_pos=(1.0, -1.0, 0.5))
    uv = 297837.66
    u2t = 2.45 * 1.6726e-24 / 1.3806e-16 * 0.4 * uv * uv         # UnitEnergy / UnitMass = UnitVelocity^2
    assert abs(R.u_to_temp(p) - u2t) <= 1e-15 * u2t
    u_eq = 20.0 / u2t / (math.sqrt(2.0) + 1e-10)
    rho = 2e-11 / p["UnitDensity_in_cgs"]
    u_old = 7.0 * u_eq
    A = 0.4 * u_old / rho ** 0.4
    pos = np.array([[1.0 + 2.0 * 0.6, -1.0 + 2.0 * 0.8, 0.5]])    # |pos - smbh| = 2
    r = R.sfr_cooling(p, [0], 1, np.zeros(1, np.int32), pos, np.ones(1), np.array([1], np.int32),
                      np.array([rho]), np.array([A]), np.zeros(1), np.zeros(1))
    unew = (u_old + u_eq) / 2
    want = (unew * 0.4 / rho ** 0.4 - A) / 10.0                   # = -A / 2 / 10 * (6 / 7): above the floor
    assert abs(r["dtentropy"][0] - want) <= 1e-13 * A / 10.0
    assert abs(want - (-(3.0 / 7.0) * A / 10.0)) <= 1e-13 * A / 10.0
    assert len(r["cand"]) == 0


def test_terms_in_order_drag_then_injection_and_ceiling_then_cooling():
    p = R.params(Timebase_interval=0.5, cooling=R.EVAPORATION_RADIAL, MinEgySpec=0.0)
    u2t = R.u_to_temp(p)
    cap = 5.0e9 / u2t
    rho, A, m = 1e-3, 1e-6, 2.0
    pos = np.array([[0.0, 3.0, 4.0]])                             # r = 5
    dt = 2 * 0.5
    u0 = A / 0.4 * rho ** 0.4
    # drag alone stays below the ceiling, drag + injection goes through it: the ceiling applies to both
    dh = np.array([0.5 * cap * m / dt])
    inj = np.array([0.7 * cap * m])
    r = R.sfr_cooling(p, [0], 1, np.zeros(1, np.int32), pos, np.array([m]), np.array([1], np.int32),
                      np.array([rho]), np.array([A]), np.zeros(1), inj, dh)
    assert r["dragheat"][0] == 0 and r["injected"][0] == 0
    ucool = R.do_cooling(p, cap, rho, dt, 25.0)
    g1 = R.GAMMA_MINUS1                                           # 7/5 - 1, not quite 0.4
    want = (ucool * g1 / rho ** g1 - A) / dt
    assert r["dtentropy"][0] == want
    # the ceiling before the drag, or the cooling before the heating, would give other values
    other = (R.do_cooling(p, min(u0 + inj[0] / m, cap) + dh[0] / m * dt, rho, dt, 25.0) * 0.4 / rho ** 0.4 - A) / dt
    assert other != want
    other = (min(R.do_cooling(p, u0, rho, dt, 25.0) + dh[0] / m * dt + inj[0] / m, cap) * 0.4 / rho ** 0.4 - A) / dt
    assert other != want


def test_massless_gas_quirks():
    """Mass == 0: never a candidate; DragHeating neither spent nor cleared; the injection cleared unspent"""
    p = R.params(Timebase_interval=0.25, CritPhysDensity_code=1.0, cooling=R.ISOTHERM)
    ptype = np.zeros(3, np.int32)
    mass = np.array([0.0, 0.0, 1.0])
    dens = np.array([5.0, 0.5, 5.0])                              # above, below, above the threshold
    ent = np.array([1.0, 1.0, 1.0])
    r = R.sfr_cooling(p, [0, 1, 2], 3, ptype, np.zeros((3, 3)), mass, np.ones(3, np.int32), dens, ent,
                      np.zeros(3), np.array([1.0, 2.0, 3.0]), np.array([4.0, 5.0, 6.0]))
    assert np.array_equal(r["cand"], [2])
    assert np.array_equal(r["dragheat"], [4.0, 5.0, 6.0])       # the candidate keeps its heating too
    assert np.array_equal(r["injected"], [0.0, 0.0, 3.0])
    u_eq = p["EqTemp"] / R.u_to_temp(p)
    for i in (0, 1):
        want = max((u_eq * 0.4 / dens[i] ** 0.4 - 1.0) / 0.5, -0.5 / 0.5)
        assert abs(r["dtentropy"][i] - want) <= 1e-15 * max(abs(want), 1.0)
    assert r["dtentropy"][2] == 0


def test_grain_floor_applies_to_active_grains_only():
    p = R.params(OriginalGasMass=1.0)
    ptype = np.array([0, 2, 2, 2, 5], np.int32)
    mass = np.array([1.0, 1e-5, 2e-5, 1e-6, 1e-7])
    r = R.sfr_cooling(p, [4, 3, 1, 0], 1, ptype, np.ones((5, 3)), mass, np.ones(5, np.int32), np.array([0.1]),
                      np.array([1.0]), np.zeros(1), np.zeros(1))
    assert np.array_equal(r["mass"], [1.0, 0.0, 2e-5, 0.0, 1e-7])


def test_find_smbh_takes_the_last_in_active_order():
    ptype = np.array([5, 0, 5, 5, 5], np.int32)
    mass = np.array([1.0, 9.0, 0.95, 0.2, 2.0])
    pos = np.arange(15, dtype=np.float64).reshape(5, 3)
    got, cnt = R.find_smbh([1, 3], ptype, mass, pos, 1.0)
    assert cnt == 0 and np.array_equal(got, np.zeros(3))
    got, cnt = R.find_smbh([4, 2, 0, 1], ptype, mass, pos, 1.0)
    assert cnt == 3 and np.array_equal(got, pos[0])
