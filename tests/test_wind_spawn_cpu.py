"""The invariants of tests/wind_spawn_ref.py, the numpy restatement of momentum_feedback.c:70-246 that
tests/test_gpu_wind_resident.py holds ghip_wind_spawn to.  No GPU."""
import math

import numpy as np
import pytest

import wind_spawn_ref as R


def _par_for_exact(exact, **over):
    """parameters under which a sink of Mass 1 in time bin 3 has new_wind_exact == exact, bit for bit where exact
    is a small integer: VirtualFeedBack = 1, and dt_fac chosen so that L_Edd * dt = exact * energy_wind_min"""
    par = R.params(**over)
    ledd, ewm = R.l_edd_dimensionless(par), R.energy_wind_min(par)
    par["dt_fac"] = exact * ewm / ledd / 8.0
    return par


def _neighbours(base, steps):
    yield base
    up = dn = base
    for _ in range(steps):
        up, dn = float(np.nextafter(up, np.inf)), float(np.nextafter(dn, -np.inf))
        yield up
        yield dn


def integer_exact_par(exact, **over):
    """parameters under which the sink of _par_for_exact has new_wind_exact == exact bit for bit: dt_fac and
    VirtualMomentum moved ulp by ulp until the rounded chain of :85 hits it (one of them alone can step over it)"""
    par = _par_for_exact(exact, **over)
    for vm in _neighbours(par["VirtualMomentum"], 16):
        for f in _neighbours(par["dt_fac"], 16):
            q = dict(par, VirtualMomentum=vm, dt_fac=f)
            if R.count(q, 1.0, 3, 1.0, 0.0)[1] == exact:
                return q
    raise AssertionError("no neighbouring parameters give new_wind_exact == %r exactly" % exact)


def _one_sink(par, n=1000, mass=1.0, tb=3, sid=77, bh_mass=1.0, mdot=0.0, nrnd=4096, seed=1):
    rnd = np.random.default_rng(seed).random(nrnd)
    m, t, h, ids = np.zeros(n), np.zeros(n, np.int32), np.full(n, 0.1), np.arange(n, dtype=np.uint32)
    m[5], t[5], ids[5] = mass, tb, sid
    return R.spawn(par, n, [5], m, t, h, ids, [bh_mass], [mdot], [0.3], rnd), rnd


def test_new_wind_is_floor_plus_one_also_for_an_integer():
    dt, exact, new_wind, corr = R.count(integer_exact_par(3.0), 1.0, 3, 1.0, 0.0)
    assert exact == 3.0 and new_wind == 4 and corr == 0.75
    for exact_target in (0.25, 0.999, 1.5, 64.3, 299.01):
        dt, exact, new_wind, corr = R.count(_par_for_exact(exact_target), 1.0, 3, 1.0, 0.0)
        assert new_wind == int(np.floor(exact)) + 1 and corr == exact / new_wind
        assert abs(exact - exact_target) < 1e-12 * exact_target


def test_thresholds_and_who_counts():
    par = _par_for_exact(5e-5)
    assert R.count(par, 1.0, 3, 1.0, 0.0)[2] == 1                                   # above 0
    assert R.count(dict(par, startup_luminosity=1), 1.0, 3, 1.0, 0.0)[2:] == (0, 1.)   # not above 1e-4
    assert R.count(par, 1.0, 0, 1.0, 0.0)[1:] == (0.0, 0, 1.)                       # time bin 0: dt = 0
    assert R.count(par, 0.5 * par["SMBHmass"], 3, 1.0, 0.0) is None                 # Mass > 0.5 SMBHmass
    assert R.count(dict(par, VirtualStart=par["Time"]), 1.0, 3, 1.0, 0.0) is None   # Time > VirtualStart
    # the accretion luminosity, and its cap at the Eddington luminosity
    q = R.params(fraction_of_ledd_feedback=0, dt_fac=1.0)
    cu = R.C_LIGHT / q["UnitVelocity_in_cm_per_s"]
    lo = R.count(q, 1.0, 1, 1.0, 1e-12)
    assert lo[1] == 1.0 * (1.0 * 0.1 * 1e-12 * (cu * cu)) * 2.0 / R.energy_wind_min(q)
    hi = R.count(q, 1.0, 1, 1.0, 1e30)
    assert hi[1] == 1.0 * (R.l_edd_dimensionless(q) * 1.0) * 2.0 / R.energy_wind_min(q)
    # at the Eddington rate BH_Mass stands for Mass
    e = dict(_par_for_exact(10.0), accretion_at_eddington_rate=1)
    assert R.count(e, 1.0, 3, 0.5, 0.0)[1] == pytest.approx(5.0, rel=1e-14)


@pytest.mark.parametrize("exact", [0.4, 1.0, 65.5, 300.25])
def test_momentum_budget_per_sink(exact):
    par = _par_for_exact(exact)
    out, _ = _one_sink(par)
    dt, ex, new_wind, corr = R.count(par, 1.0, 3, 1.0, 0.0)
    assert out["report"]["spawned"] == new_wind == len(out["rows"])
    want = ex * R.energy_wind_min(par) / R.C_LIGHT * par["UnitVelocity_in_cm_per_s"]
    got = out["rows"][:, R.WK_OLD_MOMENTUM].sum()
    assert abs(got - want) <= 4 * np.finfo(float).eps * new_wind * want
    assert np.all(out["rows"][:, R.WK_BIRTH_ENERGY] == R.energy_wind_min(par) * corr)
    assert np.all(out["mass"] == par["VirtualMass"] * out["rows"][:, R.WK_OLD_MOMENTUM])
    assert np.all(out["rows"][:, R.WK_STELLAR_AGE] == par["Time"]) and np.all(out["rows"][:, R.WK_DT1] == dt)
    assert out["report"]["gsl_draws"] == 3 * new_wind and out["report"]["new_wind_exact_sum"] == ex


@pytest.mark.parametrize("isotropic", [0, 1])
def test_directions(isotropic):
    par = _par_for_exact(2000.0, isotropic=isotropic)
    out, rnd = _one_sink(par)
    d = out["dir"]
    assert len(d) == 2001
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() < 8 * np.finfo(float).eps
    if isotropic:
        assert np.all(d[:, 2] > -1.0) and np.all(d[:, 2] <= 1.0) and d[:, 2].min() < -0.9 and d[:, 2].max() > 0.9
    else:
        assert np.all(d[:, 2] >= 0.5) and np.all(d[:, 2] < 1.0)
    speed = R.C_LIGHT / par["UnitVelocity_in_cm_per_s"] / par["FeedBackVelocity"]
    assert np.abs(np.linalg.norm(out["vel"], axis=1) / speed - 1.0).max() < 8 * np.finfo(float).eps
    # the table entries: ID + 2 + bits + step and ID + 3 + bits + step
    b = 17
    r1 = rnd[(77 + 2 + b + par["NumCurrentTiStep"]) % len(rnd)]
    assert d[b, 2] == math.cos(math.acos(2. * r1 - 1.) if isotropic else math.acos(0.5 * r1 + 0.5))


def test_id_and_table_index_wrap_at_2_to_32():
    par = _par_for_exact(3.5)
    sid = 2 ** 32 - 1001                       # the sink's ID: ID + j passes 2^32 inside the batch (n = 1000)
    out, rnd = _one_sink(par, sid=sid)
    assert out["report"]["first_index"] == 1000 and len(out["id"]) == 4
    assert out["id"].dtype == np.uint32
    assert [int(v) for v in out["id"]] == [(sid + 1000 + k) % 2 ** 32 for k in range(4)]
    assert int(out["id"][0]) == 2 ** 32 - 1 and int(out["id"][1]) == 0
    # the RndTable index wraps before the modulus
    par2 = dict(par, NumCurrentTiStep=2000)
    d, theta, phi = R.direction(par2, sid, 0, rnd)
    r1 = rnd[((sid + 2 + 2000) % 2 ** 32) % len(rnd)]
    assert d[2] == math.cos(math.acos(0.5 * r1 + 0.5))


def test_hsml_drmin_and_the_edd_mass():
    par = _par_for_exact(1.5, accretion_radius=0, fly_through_empty_space=0)
    out, _ = _one_sink(par)
    assert np.all(out["hsml"] == 0.1 + par["SofteningBndryMaxPhys"])
    assert np.all(out["rows"][:, R.WK_DRMIN] == 0.3)                 # :158 copies the sink's b1.BH_Density
    par = _par_for_exact(1.5)
    out, _ = _one_sink(par)
    assert np.all(out["hsml"] == (0.1 + par["SofteningBndryMaxPhys"]) + par["InnerBoundary"])
    assert np.all(out["rows"][:, R.WK_DRMIN] == 0.0) and out["sink_mass"] == {}
    out, _ = _one_sink(dict(par, accretion_at_eddington_rate=1), bh_mass=0.875)
    assert out["sink_mass"] == {5: 0.875}
    with pytest.raises(OverflowError):
        _one_sink(dict(par, MaxPart=1001))
