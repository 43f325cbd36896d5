"""CPU checks of the wind pass: the C-ABI of the new structs and symbols, and hand-computed pins of the numpy
restatement tests/wind_ref.py (momentum_feedback.c, virtual_density.c, virtual_spread_momentum.c) that the GPU
tests compare the device against."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import wind_ref as W
from common import REPO, bindings, pkg

K1, K2, K5 = 2.546479089470, 15.278874536822, 5.092958178941

WIND_SYMBOLS = ("ghip_wind_params_size", "ghip_wind_density", "ghip_wind_spread", "ghip_wind_feedback",
                "ghip_wind_get_injected", "ghip_wind_set_injected", "ghip_wind_get_rad_accel",
                "ghip_wind_set_rad_accel", "ghip_set_rad_accel", "ghip_wind_get_timing")
STATE_MEMBERS = ("stellar_age", "birth_energy", "old_momentum", "new_density", "drmin", "dt1", "dt2", "dt_jump",
                 "delta_momentum", "deleted")
RESULT_MEMBERS = ("iterations", "bits", "ndeleted", "deleted_momentum")


def test_symbols_are_declared_exported_and_bound():
    B = bindings()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ghip.h")).read(), flags=re.S)
    L = C.CDLL(pkg.lib_path())
    for name in WIND_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), "%s is not declared in ghip.h" % name
        assert hasattr(L, name), "libghip.so does not export %s" % name
        assert name in B.EXPORTS
        assert getattr(B.lib(), name).argtypes is not None, "%s has no argument types in bindings.py" % name
    for m in ("wind_density", "wind_spread", "wind_feedback", "wind_injected", "set_wind_injected", "wind_rad_accel",
              "set_wind_rad_accel", "set_rad_accel"):
        assert callable(getattr(B.ForcePath, m))
    assert "ghip_wind.hip" in pkg.HIP_SOURCES
    assert B.lib().ghip_wind_params_size() == C.sizeof(B.WindParams)


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ghip.h"
int main(void)
{
  printf("%zu %zu %zu", sizeof(ghip_wind_params), sizeof(ghip_wind_state), sizeof(ghip_wind_result));
""" + "".join('  printf(" %%zu", offsetof(ghip_wind_params, %s));\n' % m for m in W.PARAMS) + \
    "".join('  printf(" %%zu", offsetof(ghip_wind_state, %s));\n' % m for m in STATE_MEMBERS) + \
    "".join('  printf(" %%zu", offsetof(ghip_wind_result, %s));\n' % m for m in RESULT_MEMBERS) + r"""
  printf(" %zu\n", sizeof(ghip_integration_flags));
  return 0;
}
"""


def test_structs_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler to build the layout probe")
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    B = bindings()
    want = [C.sizeof(B.WindParams), C.sizeof(B.WindState), C.sizeof(B.WindResult)]
    for cls, members in ((B.WindParams, W.PARAMS), (B.WindState, STATE_MEMBERS), (B.WindResult, RESULT_MEMBERS)):
        want += [getattr(cls, m).offset for m in members]
        assert [k for k, _ in cls._fields_] == list(members)
    want.append(C.sizeof(B.IntegrationFlags))          # (left as it was)
    assert got == want
    assert set(W.params()) == set(W.PARAMS)


# ---- hand-computed pins of the restatement ----------------------------------------------------------------
def _gas(pos, h, m):
    pos = np.atleast_2d(np.asarray(pos, np.float64))
    n = len(pos)
    return dict(pos=pos, hsml=np.full(n, h, np.float64) if np.isscalar(h) else np.asarray(h, np.float64),
                mass=np.full(n, m, np.float64) if np.isscalar(m) else np.asarray(m, np.float64),
                type=np.zeros(n, np.int32))


def test_density_of_one_pair_at_u_025_and_075():
    par = W.params()
    g = _gas([0., 0., 0.], 1.0, 3.0)
    wpos = np.array([[0.25, 0., 0.], [0., -0.75, 0.]])
    rho, drmin = W.density(par, g, wpos, np.array([2.0, 2.0]), np.array([1.0, 1.0]))
    # u = 0.25: W = K1 + K2 (u - 1) u^2 = 2.546479089470 - 15.278874536822 * 0.75 * 0.0625 = 1.83028184555647
    assert rho[0] == pytest.approx(3.0 * 1.83028184555647, rel=1e-13)
    assert rho[0] == pytest.approx(3.0 * (K1 + K2 * (0.25 - 1) * 0.25 * 0.25), rel=1e-15)
    # u = 0.75: W = K5 (1 - u)^3 = 5.092958178941 / 64 = 0.0795774715459531
    assert rho[1] == pytest.approx(3.0 * 0.0795774715459531, rel=1e-13)
    assert drmin.tolist() == [1.0, 0.5]                  # |r - h_j| + h_j / 4
    # dt_jump <= 0: reset, not evaluated
    rho, drmin = W.density(par, g, wpos, np.array([2.0, 2.0]), np.array([0.0, 1.0]))
    assert rho[0] == 0.0 and drmin[0] == 1.e40 and rho[1] > 0


def test_density_gas_in_reach_but_outside_its_own_h_sets_drmin_only():
    par = W.params()
    g = _gas([[0., 0., 0.], [0.3, 0., 0.], [5., 5., 5.]], [0.1, 0.1, 0.1], [1.0, 0.0, 1.0])
    rho, drmin = W.density(par, g, np.array([[0.5, 0., 0.]]), np.array([1.0]), np.array([1.0]))
    # gas 0: r = 0.5 > h_j: drmin = 0.4 + 0.025; gas 1 (massless, r = 0.2) is nobody's neighbour; gas 2 out of reach
    assert rho[0] == 0.0 and drmin[0] == pytest.approx(0.425, rel=1e-15)
    rho, drmin = W.density(par, g, np.array([[0.5, 0., 0.]]), np.array([0.4]), np.array([1.0]))
    assert rho[0] == 0.0 and drmin[0] == 1.e40           # nothing within the particle's own h
    # periodic: the nearest image by the two comparisons
    rho, drmin = W.density(W.params(periodic=1, BoxSize=1.0), _gas([0.95, 0., 0.], 0.5, 1.0),
                           np.array([[0.05, 0., 0.]]), np.array([0.2]), np.array([1.0]))
    assert rho[0] == pytest.approx(8 * (K1 + K2 * (0.2 - 1) * 0.2 * 0.2), rel=1e-13)   # r = 0.1, u = 0.2, h_j^-3 = 8


def test_spread_weights_sum_to_one():
    par = W.params()
    rng = np.random.default_rng(3)
    g = _gas(rng.random((40, 3)), 0.3 + 0.2 * rng.random(40), 0.5 + rng.random(40))
    wpos, wh = np.array([[0.5, 0.5, 0.5], [0.2, 0.3, 0.4]]), np.array([0.6, 0.5])
    wvel = np.array([[3., 0., 4.], [0., -2., 0.]])
    dtj = np.array([1.0, 1.0])
    rho, _ = W.density(par, g, wpos, wh, dtj)
    assert np.all(rho > 0)
    inj = np.zeros((40, 3), W.LD)
    W.spread(par, g, wpos, wh, wvel, dtj, rho, np.array([2.0, 5.0]), inj)
    tot = inj.sum(axis=0).astype(np.float64)
    assert tot == pytest.approx([2.0 * 0.6, -5.0, 2.0 * 0.8], rel=1e-13)
    # a particle whose dt_jump reached 0 does not spread
    inj2 = np.zeros((40, 3), W.LD)
    W.spread(par, g, wpos, wh, wvel, np.array([0.0, 1.0]), rho, np.array([2.0, 5.0]), inj2)
    assert inj2.sum(axis=0).astype(np.float64) == pytest.approx([0., -5.0, 0.], abs=1e-13)


def _one(par, gas_m=1.0, gas_h=1.0, wpos=(0.25, 0., 0.), wh=1.0, wvel=(1., 0., 0.), tb=4, old=1.0, birth=0.0,
         age=0.0, **kw):
    """one gas particle at the origin, one wind particle; U = C and FBV = 1, so that a length is a time"""
    fields = dict(pos=np.array([[0., 0., 0.], list(wpos)]), vel=np.array([[0., 0., 0.], list(wvel)]),
                  hsml=np.array([gas_h, wh]), mass=np.array([gas_m, 1e-6]), type=np.array([0, 3], np.int32),
                  timebin=np.array([1, tb], np.int32), ngas=1)
    state = dict(stellar_age=[age], birth_energy=[birth], old_momentum=[old], new_density=[0.], drmin=[0.])
    return W.feedback(par, fields, [1], state, **kw)


PIN = dict(UnitVelocity_in_cm_per_s=W.C_LIGHT, FeedBackVelocity=1.0, dt_fac=1.0 / 16, fly_through_empty_space=0,
           variable_search_radius=0, max_iter=1)


def test_first_iteration_dtau_and_its_cap_and_the_dense_hsml():
    # dt_jump = 16 / 16 = 1; desired = 0.2 h = 0.2 < cap = 1; dt1 = 0.2; rho = m W(0.25)
    par = W.params(**PIN)
    w025 = K1 + K2 * (0.25 - 1) * 0.25 * 0.25
    r = _one(par, gas_m=0.5)
    assert r["status"] == "noconv" and r["under_way"] == 1 and r["iterations"] == 1 and r["bits"] == 1
    dtau = 0.5 * w025 * 0.2
    assert dtau < 2.0
    assert r["delta_momentum"][0] == pytest.approx(1 - math.exp(-dtau), rel=1e-13)
    assert r["old_momentum"][0] == pytest.approx(math.exp(-dtau), rel=1e-13)
    assert r["mass"][1] == pytest.approx(1e-6 * math.exp(-dtau), rel=1e-13)
    assert r["pos"][1].tolist() == [0.25 + 0.2, 0., 0.]
    assert r["dt1"][0] == pytest.approx(0.2, rel=1e-15) and r["dt2"][0] == r["dt1"][0]
    assert r["dt_jump"][0] == pytest.approx(0.8, rel=1e-15)
    # rho > 0: h = 3 (DesNumNgb OriginalGasMass / rho)^0.33333 + SofteningGasMaxPhys
    assert r["hsml"][1] == pytest.approx(3 * (33.0 * 1e-3 / (0.5 * w025)) ** 0.33333 + 0.01, rel=1e-13)
    # the cap: dtau_max = 10 desired / h = 2
    r = _one(par, gas_m=100.0)
    assert 1 in r["ends"]["dtau_cap"] or 0 in r["ends"]["dtau_cap"]
    assert r["delta_momentum"][0] == pytest.approx(1 - math.exp(-2.0), rel=1e-13)


def test_empty_space_grows_hsml_and_the_search_radius_cap():
    par = W.params(**PIN)
    r = _one(par, wpos=(3., 0., 0.))                      # no gas in reach
    assert r["delta_momentum"][0] == 0.0 and r["hsml"][1] == pytest.approx(1.2, rel=1e-15)
    # VARIABLE_PHOTON_SEARCH_RADIUS: h <= PhotonSearchRadius r + SofteningBulgeMaxPhys, r after the move
    r = _one(W.params(**dict(PIN, variable_search_radius=1, PhotonSearchRadius=0.25)), wpos=(3., 0., 0.))
    assert r["hsml"][1] == pytest.approx(0.25 * 3.2 + 0.02, rel=1e-15)
    # VIRTUAL_FLY_THORUGH_EMPTY_SPACE: desired <= 0.5 drmin + 2 SofteningGas; gas h_j = 0.1 at r = 0.2: drmin = 0.1 + 0.025
    r = _one(W.params(**dict(PIN, fly_through_empty_space=1)), gas_h=0.1, wpos=(0.2, 0., 0.))
    assert r["dt1"][0] == pytest.approx(0.5 * 0.125 + 0.02, rel=1e-14) and 0 in r["ends"]["fly"]


def test_time_cap_ends_the_particle_exactly():
    # dt_jump = 2 / 16 = 0.125 < 0.2 h: the jump is the time that is left, and nothing is left after it
    par = W.params(**dict(PIN, max_iter=50))
    r = _one(par, tb=1, wpos=(3., 0., 0.))
    assert r["status"] == "ok" and r["iterations"] == 1 and r["bits"] == 1
    assert r["dt1"][0] == 0.125 and r["dt2"][0] == 0.125 and r["dt_jump"][0] == 0.0
    assert r["pos"][1, 0] == 3.125 and 0 in r["ends"]["cap"]
    # several iterations: 1 = 0.2 + 0.24 + 0.288 + (rest, capped); h grows by 1.2 each time
    r = _one(par, tb=4, wpos=(3., 0., 0.))
    assert r["iterations"] == 4 and r["bits"] == 4 and r["dt2"][0] == pytest.approx(1.0, rel=1e-15)
    assert r["pos"][1, 0] == pytest.approx(4.0, rel=1e-15) and r["hsml"][1] == pytest.approx(1.2 ** 4, rel=1e-14)


def test_hide_rule_below_one_percent():
    # birth = 50: threshold 0.01 * 50 = 0.5; old = 1 -> exp(-2) = 0.135 < 0.5 after one capped dtau
    par = W.params(**dict(PIN, max_iter=50))
    r = _one(par, gas_m=100.0, birth=50.0)
    assert r["status"] == "ok" and r["iterations"] == 1 and 0 in r["ends"]["hidden"]
    assert r["dt_jump"][0] == 0.0 and r["dt1"][0] == 0.0 and r["dt2"][0] == pytest.approx(1.0, rel=1e-15)
    assert r["deleted"][0] == 2 and r["mass"][1] == 0.0 and r["ndeleted"] == 1 and r["deleted_momentum"] == 0.0
    # hidden in that iteration: its DeltaPhotonMomentum is not spread
    assert np.all(r["injected"] == 0.0) and r["delta_momentum"][0] > 0


def test_elimination_codes():
    par = W.params(**dict(PIN, max_iter=50, OuterBoundary=3.5, VirtualTime=2.0, Time=3.0))
    r = _one(par, tb=1, wpos=(3., 0., 0.), age=1.5)
    assert r["deleted"][0] == 0 and r["mass"][1] == pytest.approx(1e-6)
    r = _one(par, tb=4, wpos=(3., 0., 0.), age=1.5)           # ends at x = 4 > OuterBoundary
    assert r["deleted"][0] == 1 and r["mass"][1] == 0.0 and r["deleted_momentum"] == 1.0 and r["ndeleted"] == 1
    r = _one(par, tb=1, wpos=(3., 0., 0.), age=0.5)           # Time - age = 2.5 > VirtualTime
    assert r["deleted"][0] == 1 and r["deleted_momentum"] == 1.0
    r = _one(par, tb=1, wpos=(3., 0., 0.), age=1.5, old=0.1, birth=50.0)   # depleted (and hidden at once)
    assert r["deleted"][0] == 2 and r["deleted_momentum"] == 0.0 and r["ndeleted"] == 1


def test_dt_total_floor_changes_nothing():
    par = W.params(**dict(PIN, dt_total_floor=10.0))
    r = _one(par)
    assert r["status"] == "floor" and r["iterations"] == 0 and r["pos"][1].tolist() == [0.25, 0., 0.]
    assert r["hsml"][1] == 1.0 and r["old_momentum"][0] == 1.0 and r["dt_jump"][0] == 1.0


def test_rad_accel_and_its_cap():
    par = W.params(dt_fac_gas=0.5)
    fields = dict(type=np.array([0, 0, 0, 0, 1]), timebin=np.array([1, 1, 0, 1, 1]),
                  mass=np.array([2.0, 2.0, 2.0, 0.0, 1.0]), ngas=4)
    inj = np.array([[3., 0., 4.], [3e6, 0., 4e6], [1., 1., 1.], [1., 1., 1.]])
    ra, left, touched = W.rad_accel(par, fields, [0, 1, 2, 4], inj)
    # dt = 2 * 0.5 = 1: RadAccel = Injected / dt / Mass; |a| <= 1e4 / dt
    assert ra[0].tolist() == [1.5, 0., 2.0]
    assert ra[1] == pytest.approx([0.6e4, 0., 0.8e4], rel=1e-15)
    assert ra[2].tolist() == [0., 0., 0.]                 # dt == 0
    assert touched.tolist() == [True, True, True, False]  # gas 3 is not active
    assert left[:3].tolist() == [[0., 0., 0.]] * 3 and left[3].tolist() == [1., 1., 1.]


def test_reference_round_trip_residue_takes_both_signs():
    par = W.params()
    U, FBV = par["UnitVelocity_in_cm_per_s"], 0.37
    dt = (1 << np.arange(1, 11))[None, :] * (1e-3 * (1 + np.arange(40) / 64.0))[:, None]
    res = W.round_trip_residue(dt.ravel(), U, FBV)
    assert len(res) == 400
    assert (res > 0).sum() > 10 and (res < 0).sum() > 10 and (res == 0).sum() > 10
    assert np.abs(res / dt.ravel()).max() < 4e-16
    # ... and on its sign hangs one more iteration: the two rules differ where it is positive
    a = np.flatnonzero(res > 0)[0]
    tb, fac = 1 + a % 10, 1e-3 * (1 + (a // 10) / 64.0)
    p = W.params(**dict(PIN, max_iter=50, FeedBackVelocity=FBV, UnitVelocity_in_cm_per_s=U, dt_fac=fac))
    mine = _one(p, tb=int(tb), wpos=(3., 0., 0.), wh=100.0)
    theirs = _one(p, tb=int(tb), wpos=(3., 0., 0.), wh=100.0, round_trip=True)
    assert mine["iterations"] == 1 and theirs["iterations"] == 2
    assert mine["hsml"][1] == pytest.approx(120.0) and theirs["hsml"][1] == pytest.approx(144.0)
