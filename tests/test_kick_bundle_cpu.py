"""CPU checks of the shipped bundle's integrator (ghip_set_integration_flags, gadget_force_bind_integration):
the new C-ABI symbols are exported, the new structs have the layouts their Python mirrors assume, and
the numpy restatement the GPU tests compare against (tests/kick_ref.py) is pinned -- to the oracle
for the minimal flag set, and by hand for every rule the bundle adds."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import kick_ref as R
from common import O, REPO, bindings, pkg


def test_libraries_export_the_integration_flags():
    L = C.CDLL(pkg.lib_path())
    B = bindings()
    for name in ("ghip_set_integration_flags", "ghip_kick_set_fields", "ghip_kick_get_drag_accel"):
        assert hasattr(L, name), name
        assert name in B.EXPORTS
    B.lib()
    import importlib
    H = importlib.import_module("gadget-leicester_amd.hostapi")
    assert hasattr(C.CDLL(H.lib_path()), "gadget_force_bind_integration")
    assert "gadget_force_bind_integration" in H.EXPORTS
    H.lib()


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "gadget_force.h"
int main(void)
{
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ghip_integration_flags),
         offsetof(ghip_integration_flags, virtual_particles), offsetof(ghip_integration_flags, OuterBoundary),
         offsetof(ghip_integration_flags, UnitVelocity_in_cm_per_s),
         sizeof(struct gadget_force_integration_layout),
         offsetof(struct gadget_force_integration_layout, p_new_density),
         offsetof(struct gadget_force_integration_layout, s_drag_accel),
         offsetof(struct gadget_force_integration_layout, a_unit_velocity));
  return 0;
}
"""


def test_structs_match_the_python_mirrors(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler to build the layout probe")
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    import importlib
    H = importlib.import_module("gadget-leicester_amd.hostapi")
    F, Lay = bindings().IntegrationFlags, H.IntegrationLayout
    assert got == [C.sizeof(F), F.virtual_particles.offset, F.OuterBoundary.offset,
                   F.UnitVelocity_in_cm_per_s.offset, C.sizeof(Lay), Lay.p_new_density.offset,
                   Lay.s_drag_accel.offset, Lay.a_unit_velocity.offset]
    assert got[0] == 5 * 4 + 4 + 7 * 8 and got[4] == 13 * 4
    assert sorted(k for k, _ in F._fields_) == sorted(R.flags())


# ---- a mixed problem: gas, halo, grains, virtual particles, sinks ----------------------------------
def problem(seed=3, ngas=160, nother=90, types=(1, 2, 3, 5), comoving=False):
    rng = np.random.default_rng(seed)
    n = ngas + nother
    ptype = np.zeros(n, np.int32)
    ptype[ngas:] = rng.choice(types, nother)
    mass = np.full(n, 1e-3)
    mass[ptype == 5] = np.where(rng.random((ptype == 5).sum()) < 0.5, 0.8, 0.05)   # both sink branches
    mass[rng.choice(ngas, 3, replace=False)] = 0.0                                  # massless gas
    s = R.state(
        type=ptype, mass=mass, vel=rng.standard_normal((n, 3)),
        grav=rng.standard_normal((n, 3)) * 10 ** rng.uniform(-1, 1.5, (n, 1)),
        hyd=rng.standard_normal((ngas, 3)) * 3.0, velpred=rng.standard_normal((ngas, 3)),
        entropy=0.05 * (1 + rng.random(ngas)),
        dtentropy=np.where(rng.random(ngas) < 0.1, -50.0, 0.3) * rng.random(ngas),
        density=1.0 + rng.random(ngas), hsml=0.02 * (0.5 + rng.random(n)), vsig=0.5 + 2 * rng.random(ngas),
        timebin=rng.integers(19, 25, n).astype(np.int32),
        ti_begstep=(rng.integers(0, 4, n) << 25).astype(np.int32),
        drag=rng.standard_normal((ngas, 3)) * 2.0, ddm=rng.standard_normal((ngas, 3)) * 1e-4)
    p = dict(Ti_Current=1 << 27, Timebase_interval=1.0 / (1 << 29), ComovingIntegrationOn=0, Time=1.0,
             hubble_a=1.0, ErrTolIntAccuracy=0.025, CourantFac=0.15, MaxSizeTimestep=0.02,
             MinSizeTimestep=1e-9, dt_displacement=0.015, SofteningTable=[0.01, 0.02, 0.005, 0.01, 0.03, 0.01],
             MinEgySpec=0.0, TimeBinActive=0b1010110101 << 16, logTimeBegin=0.0, logTimeMax=0.0,
             AdaptiveGravsoftForGasHsml=0, pmgrid=0, dt_gravkickB=0.0)
    tabs = None
    if comoving:
        t = np.linspace(0.01, 1.0, 1000)
        tabs = [np.cumsum(t ** 1.5) * 1e-3, np.cumsum(t ** 0.5) * 1e-3, np.cumsum(t ** 0.2) * 1e-3]
        p.update(ComovingIntegrationOn=1, Time=0.37, hubble_a=1.9, MinEgySpec=0.02,
                 logTimeBegin=math.log(0.02), logTimeMax=math.log(1.0))
        p["Timebase_interval"] = (p["logTimeMax"] - p["logTimeBegin"]) / (1 << 29)
    return p, s, tabs


def oracle_params(p):
    P = O.KickParams()
    for k, v in p.items():
        if k == "SofteningTable":
            for t in range(6):
                P.SofteningTable[t] = v[t]
        else:
            setattr(P, k, v)
    return P


@pytest.mark.parametrize("comoving", [False, True])
@pytest.mark.parametrize("subset", [False, True])
@pytest.mark.parametrize("adaptive", [0, 1])
def test_all_switches_off_equal_the_oracle_bit_for_bit(comoving, subset, adaptive):
    p, s, tabs = problem(types=(1,), comoving=comoving)
    p["AdaptiveGravsoftForGasHsml"] = adaptive
    n, ng = len(s["type"]), len(s["entropy"])
    act = None
    if subset:
        act = np.random.default_rng(9).permutation(n)[: n // 3].astype(np.int32)
    want = O.advance_timesteps(oracle_params(p), s["type"], s["vel"], s["grav"], s["hyd"], s["velpred"],
                               s["entropy"], s["dtentropy"], s["density"], np.zeros(ng), s["hsml"][:ng],
                               s["vsig"], s["timebin"], s["ti_begstep"], active=act, tables=tabs)
    got = R.advance_timesteps(p, R.flags(), s, active=act, tables=None if tabs is None else tabs[1:])
    assert want["rc"] == got["rc"] == 0
    for k in ("vel", "velpred", "entropy", "dtentropy", "timebin", "ti_begstep"):
        assert np.array_equal(s[k], want[k]), k
    assert len(np.unique(s["timebin"])) > 2


def _one(ptype, grav=(3.0, 0, 0), mass=1e-3, hsml=0.02, timebin=20, ngas=None, **kw):
    """a state of one particle (plus one gas particle when ptype != 0, so that SphP exists)"""
    t = [ptype] if ptype == 0 else [0, ptype]
    n = len(t)
    ng = 1
    s = R.state(type=t, mass=[1e-3] * (n - 1) + [mass], vel=np.ones((n, 3)), grav=[list(grav)] * n,
                hyd=[[0.5, -0.25, 0.0]], velpred=np.ones((1, 3)), entropy=[1.0], dtentropy=[0.1], density=[1.0],
                hsml=[0.02] * (n - 1) + [hsml], vsig=[1e-3], timebin=[timebin] * n, ti_begstep=[0] * n, **kw)
    return s, n - 1


P0 = dict(Ti_Current=1 << 20, Timebase_interval=1.0 / (1 << 29), ComovingIntegrationOn=0, Time=1.0, hubble_a=1.0,
          ErrTolIntAccuracy=0.025, CourantFac=0.15, MaxSizeTimestep=0.05, MinSizeTimestep=1e-12,
          dt_displacement=0.05, SofteningTable=[0.01] * 6, MinEgySpec=0.0, TimeBinActive=(1 << 29) - 1,
          logTimeBegin=0.0, logTimeMax=0.0, AdaptiveGravsoftForGasHsml=0, pmgrid=0, dt_gravkickB=0.0)


def _step(s, i, f, p=P0):
    return R.get_timestep(i, p, f, s, R._factors(p))


def test_grains_take_half_the_step_and_no_gravity_kick():
    s, i = _one(2)
    dt0 = math.sqrt(2 * 0.025 * 0.01 / 3.0)
    assert _step(s, i, R.flags()) == int(dt0 / P0["Timebase_interval"])
    assert _step(s, i, R.bundle()) == int(dt0 / 2 / P0["Timebase_interval"])
    v0 = s["vel"][i].copy()
    out = R.advance_timesteps(P0, R.bundle(), s)
    assert out["rc"] == 0 and np.array_equal(s["vel"][i], v0)            # dv = 0 (timestep.c:410-418)
    assert out["kick_flag"][i] == 1 and not out["kick_dv"][i].any()      # the node still gets its kick
    s2, _ = _one(2)
    R.advance_timesteps(P0, R.flags(), s2)
    assert not np.array_equal(s2["vel"][i], v0)                          # minimal set: kicked


def test_sink_steps_of_both_branches_and_without_boundaries():
    f = R.bundle()
    big, small = 0.8, 0.05                                              # >= / < 0.45 SMBHmass
    for m, bound in ((big, f["InnerBoundary"]), (small, f["SinkBoundary"])):
        s, i = _one(5, grav=(1e-6, 0, 0), mass=m, hsml=0.04)
        want = min(0.03 * (3.0 / 100.), 0.05 * math.pow(bound + 0.5 * 0.04, 1.5) / math.pow(m, 0.5))
        assert _step(s, i, f) == int(want / P0["Timebase_interval"])
    s, i = _one(5, grav=(1e-6, 0, 0), mass=big, hsml=0.04)
    for g in (dict(InnerBoundary=0.0), dict(accretion_radius=0)):
        assert _step(s, i, R.bundle(**g)) == int(0.03 * (3.0 / 100.) / P0["Timebase_interval"])
    s, i = _one(5, grav=(1e-6, 0, 0), mass=small, hsml=0.04)
    assert _step(s, i, R.bundle(SinkBoundary=0.0)) == int(0.03 * (3.0 / 100.) / P0["Timebase_interval"])
    assert _step(s, i, R.bundle(black_holes=0)) == int(0.05 / P0["Timebase_interval"])   # MaxSizeTimestep


def test_virtual_particles_are_neither_kicked_nor_drifted():
    f = R.bundle(OuterBoundary=300.0, FeedBackVelocity=10.0)
    s, i = _one(3, grav=(1e-6, 0, 0))
    dt_abs = 0.03 * 300.0 / R.C_LIGHT * 2.97837e5 * 10.0
    assert dt_abs < 0.05
    assert _step(s, i, f) == int(dt_abs / P0["Timebase_interval"])
    assert _step(s, i, R.bundle(OuterBoundary=3e9, FeedBackVelocity=1e6)) == \
        int(min(1.0, 0.05) / P0["Timebase_interval"])                  # dt_ff = 1 caps dt_abs
    v0, tb0 = s["vel"][i].copy(), int(s["ti_begstep"][i])
    out = R.advance_timesteps(P0, f, s)
    assert out["rc"] == 0 and np.array_equal(s["vel"][i], v0) and out["kick_flag"][i] == 0
    assert s["ti_begstep"][i] == tb0 + (1 << 20)                        # the timeline still advances
    s.update(pos=np.zeros((2, 3)), ti_current=np.zeros(2, np.int32), divvel=np.zeros(1), pressure=np.zeros(1))
    dp = dict(Timebase_interval=P0["Timebase_interval"], ComovingIntegrationOn=0, MinGasHsml=0.0)
    assert R.drift(dp, f, s, 1 << 21) == 0
    assert not s["pos"][i].any() and s["ti_current"][i] == 0 and s["ti_current"][0] == 1 << 21
    assert s["pos"][0].all()


def test_drag_accel_enters_the_criterion_and_the_drift_and_is_reset():
    drag = np.array([[40.0, 0.0, 0.0]])
    s, i = _one(0, grav=(1.0, 0, 0), drag=drag)
    s["vsig"][:] = 1e-9                                                 # no Courant limit
    ac = math.sqrt((1.0 + 0.5 + 40.0) ** 2 + 0.25 ** 2)
    assert _step(s, i, R.bundle()) == int(math.sqrt(2 * 0.025 * 0.01 / ac) / P0["Timebase_interval"])
    dt_no = _step(s, i, R.flags())
    assert _step(s, i, R.bundle()) < dt_no
    R.advance_timesteps(P0, R.bundle(), s)
    assert not s["drag"].any()                                          # timestep.c:508
    s2, _ = _one(0, grav=(1.0, 0, 0), drag=drag)
    R.advance_timesteps(P0, R.flags(), s2)
    assert np.array_equal(s2["drag"], drag)
    # drift: VelPred += DragAccel dt_hydrokick after the gravity / hydro term (predict.c:195-198)
    for f in (R.bundle(), R.flags()):
        s, _ = _one(0, grav=(1.0, 0, 0), drag=drag)
        s.update(pos=np.zeros((1, 3)), ti_current=np.zeros(1, np.int32), divvel=np.zeros(1), pressure=np.zeros(1))
        vp0 = s["velpred"][0].copy()
        dp = dict(Timebase_interval=P0["Timebase_interval"], ComovingIntegrationOn=0, MinGasHsml=0.0)
        R.drift(dp, f, s, 1 << 20)
        dt = (1 << 20) * P0["Timebase_interval"]
        want = vp0 + (s["grav"][0] * dt + s["hyd"][0] * dt)
        if f["dust"]:
            want = want + drag[0] * dt
        assert np.array_equal(s["velpred"][0], want)


def test_dust_timestep_and_its_overwrite_by_the_adaptive_softening():
    ddm = np.array([[0.0, 5e-4, 0.0]])
    s, i = _one(0, grav=(1.0, 0, 0), mass=1e-3, ddm=ddm)
    s["hyd"][:] = 0.0
    s["vsig"][:] = 1e-9
    dt0 = math.sqrt(2 * 0.025 * 0.01 / 1.0)
    a2 = math.sqrt(1.0 + (5e-4 / 1e-3 / dt0) ** 2)
    want = min(dt0, math.sqrt(2 * 0.025 * 0.01 / a2))
    assert want < dt0
    assert _step(s, i, R.bundle()) == int(want / P0["Timebase_interval"])
    assert _step(s, i, R.bundle(dust_timestep=0)) == int(dt0 / P0["Timebase_interval"])
    # ADAPTIVE_GRAVSOFT_FORGAS_HSML overwrites dt -- with the ac that DUST_TIMESTEP left behind
    pa = dict(P0, AdaptiveGravsoftForGasHsml=1)
    assert _step(s, i, R.bundle(), pa) == int(math.sqrt(2 * 0.025 * 0.02 / 2.8 / a2) / P0["Timebase_interval"])
    assert _step(s, i, R.bundle(dust_timestep=0), pa) == \
        int(math.sqrt(2 * 0.025 * 0.02 / 2.8 / 1.0) / P0["Timebase_interval"])
    # massless gas and a zero new acceleration take no part
    s0, i0 = _one(0, grav=(1.0, 0, 0), mass=0.0, ddm=ddm)
    s0["hyd"][:] = 0.0
    s0["vsig"][:] = 1e-9
    assert _step(s0, i0, R.bundle()) == int(dt0 / P0["Timebase_interval"])
    sz, iz = _one(0, grav=(0.0, 0, 0), mass=1e-3)
    sz["hyd"][:] = 0.0
    sz["vsig"][:] = 1e-9
    assert _step(sz, iz, R.bundle()) == _step(sz, iz, R.bundle(dust_timestep=0))


def test_per_bin_sums_move_incrementally_in_list_order():
    ptype = np.array([0, 0, 5, 1, 5, 0], np.int32)
    binold = np.array([3, 4, 5, 3, 6, 2])
    binnew = np.array([4, 4, 3, 2, 6, 5])
    sfr = np.array([0.1, 0.2, 0, 0, 0, 1e-17])
    dm, tm, m = np.array([0, 0, 1.0, 0, 2.0, 0]), np.array([0, 0, 3.0, 0, 4.0, 0]), np.array([0, 0, 5.0, 0, 6.0, 0])
    S = np.zeros(8)
    S[2] = 1.0
    BH = [np.zeros(8) for _ in range(3)]
    order = [5, 0, 1, 2, 3, 4]
    R.bin_sums(order, ptype, binold, binnew, sfr, dm, tm, m, S, *BH)
    want = np.zeros(8)
    want[2] = 1.0
    want[2] -= 1e-17                                                    # particle 5 first: 1 - 1e-17 rounds to 1
    want[5] += 1e-17
    want[3] -= 0.1
    want[4] += 0.1
    assert np.array_equal(S, want)
    assert S[2] == 1.0 and S[5] == 1e-17
    assert BH[0][5] == -1.0 and BH[0][3] == 1.0 and not BH[0][6]        # unchanged bin: untouched
    assert BH[1][5] == -3.0 and BH[2][3] == 5.0


def test_displacement_merge_of_gas_stars_and_sinks():
    v, c, m = [1.0, 2.0, 0, 0, 4.0, 8.0], [10, 20, 0, 0, 40, 80], [0.1, 0.2, 0, 0, 0.4, 0.8]
    assert R.merge_displacement_sums(v, c, m, 0, 1) == (v, c, m)
    v1, c1, m1 = R.merge_displacement_sums(v, c, m, 1, 0)
    assert v1[0] == v1[4] == 5.0 and c1[0] == c1[4] == 50 and v1[5] == 8.0 and m1[5] == 0.8
    v2, c2, m2 = R.merge_displacement_sums(v, c, m, 1, 1)
    assert v2[0] == v2[5] == 13.0 and v2[4] == 5.0 and c2[0] == c2[5] == 130 and c2[4] == 50
    assert m2[5] == 0.1 and m2[4] == 0.4
