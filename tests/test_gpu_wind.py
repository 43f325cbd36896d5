"""The wind particles (momentum_feedback.c: the propagation loop with virtual_density and
virtual_spread_momentum) on the device, through the C-ABI, against the independent numpy restatement of
tests/wind_ref.py with brute-force neighbour search.  fp64 within 1e-12 of the field's largest magnitude; every
loop test first asserts that the restatement's smallest decision margin is >= 1e-9 (below that, agreement on a
discrete decision would be luck); fields the passes must not touch bit-unchanged; two identical calls
bit-identical; RAD_ACCEL in the kick and the drift against tests/kick_ref.py."""
import functools

import numpy as np
import pytest

import kick_ref as KR
import wind_ref as R
from common import O, Problem, bindings, relerr
from test_gpu_kick_bundle import check as kick_check, device as kick_device, flags_struct, kick_params
from test_kick_bundle_cpu import problem as kick_problem

pytestmark = pytest.mark.gpu
TOL = 1e-12
MARGIN = 1e-9


def _scaled_err(a, b):
    """max |a - b| over the array, relative to the largest |b| (sums with cancellation)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


class WindCase:
    """A Problem gas lattice (ng = 10: 1 000 gas) in which 480 of the other particles are Type-3 wind particles,
    strewn through the lattice and, without periodic boundaries, just outside it.  The gas of the slab x < 0.4 and
    a few more are massless (nobody's neighbour: empty space for the wind); the gas of the slab next to it has a
    small h_j and mostly only sets drmin.  `wind` is the list in list order.  Units: a wind particle covers
    C / U / FBV = 50 lengths per time, its speed; per step (time bins 0..3 of 1e-3) up to 0.4 box lengths in jumps
    of at most 0.2 Hsml.  box: all of it in a box of that size (scale_cases.rescale_problem): the placement range,
    the slab limits, the boundaries, softenings and search radius x box, the masses x box^3, the momenta x box^4,
    and the wind's speed x box through FeedBackVelocity / box."""

    def __init__(self, periodic, nwind=480, ng=10, seed=2, box=1.0):
        pr = Problem(ng=ng, gas=True, periodic=periodic)
        if box != 1.0:
            from scale_cases import rescale_problem
            pr = rescale_problem(pr, box)
        self.pr = pr
        rng = np.random.default_rng(seed)
        n, ngas = pr.n, pr.ngas
        self.wind = np.sort(rng.choice(np.arange(ngas, n), nwind, replace=False)).astype(np.int32)
        typ = pr.ic["type"].copy()
        typ[self.wind] = 3
        pr.ic["type"] = typ
        pos = pr.ic["pos"].copy()
        lo, hi = (0.02, 0.98) if periodic else (-0.15, 1.15)
        pos[self.wind] = rng.uniform(lo, hi, (nwind, 3)) * box
        pr.ic["pos"] = pos
        pr.extent = O.domain_extent(pos)
        self.par = R.params(periodic=periodic, BoxSize=pr.box, Time=1.0, dt_fac=pr.timebase, dt_fac_gas=pr.timebase,
                            UnitDensity_in_cgs=60.0, VirtualTime=0.5, OuterBoundary=1.45 * box,
                            OriginalGasMass=1.6e-4 * box ** 3, SofteningGas=0.004 * box,
                            SofteningGasMaxPhys=0.004 * box, SofteningBulgeMaxPhys=0.02 * box,
                            PhotonSearchRadius=0.3 * box, dt_total_floor=1e-15 * 0.5 * n, rad_accel=1, max_iter=400,
                            FeedBackVelocity=1.0 / box)
        speed = R.C_LIGHT / self.par["UnitVelocity_in_cm_per_s"] / self.par["FeedBackVelocity"]
        d = rng.standard_normal((nwind, 3))
        vel = pr.ic["vel"].copy()
        vel[self.wind] = speed * d / np.linalg.norm(d, axis=1)[:, None]
        pr.ic["vel"] = vel
        self.hsml = pr.hsml0.copy()
        self.hsml[self.wind] = pr.ic["spacing"] * (1.2 + 1.0 * rng.random(nwind))
        gx = pos[:ngas, 0]
        self.hsml[:ngas][(gx >= 0.4 * box) & (gx < 0.5 * box)] = 0.3 * pr.ic["spacing"]    # gas that only sets drmin
        self.mass = pr.ic["mass"].copy()
        self.mass[:ngas][gx < 0.4 * box] = 0.0                                       # empty space
        self.mass[rng.choice(ngas, 25, replace=False)] = 0.0
        self.mass[self.wind] = 1e-6 * box ** 3
        self.timebin = pr.timebin.copy()
        self.timebin[self.wind[rng.random(nwind) < 0.1]] = 0                        # listed, dt_jump = 0
        self.timebin[rng.choice(ngas, 30, replace=False)] = 0                        # gas with dt = 0 (RadAccel)
        self.active = np.sort(np.concatenate([rng.choice(ngas, ngas // 2, replace=False), self.wind])).astype(np.int32)
        # the state: ages on both sides of VirtualTime; every third particle is born bright (hidden at 50 %)
        self.age = rng.uniform(0.2, 0.95, nwind)
        self.old = 1e-3 * (1 + rng.random(nwind)) * box ** 4
        self.birth = self.old * 50.0 * box * np.where(np.arange(nwind) % 3 == 0, 50.0, 1.0)
        self.rho0 = rng.random(nwind)
        self.drmin0 = rng.random(nwind)

    def fields(self):
        pr = self.pr
        return dict(pos=pr.ic["pos"], vel=pr.ic["vel"], hsml=self.hsml, mass=self.mass, type=pr.ic["type"],
                    timebin=self.timebin, ngas=pr.ngas)

    def state(self, sel=slice(None)):
        return dict(stellar_age=self.age[sel], birth_energy=self.birth[sel], old_momentum=self.old[sel],
                    new_density=self.rho0[sel], drmin=self.drmin0[sel])

    def gparams(self, **over):
        p = bindings().WindParams()
        for k, v in {**self.par, **over}.items():
            setattr(p, k, v)
        return p

    def device(self, tree=True):
        B = bindings()
        pr = self.pr
        fp = pr.device()
        fp.set_field(B.F_MASS, self.mass)
        fp.set_field(B.F_TIMEBIN, self.timebin)
        fp.set_field(B.F_HSML, self.hsml)
        if tree:
            pr.device_tree(fp)
        return B, fp

    def dt_jump(self):
        tb = self.timebin[self.wind].astype(np.int64)
        return np.where(tb > 0, (1 << tb).astype(np.float64), 0.0) * self.par["dt_fac"]

    def feedback(self, fp, **over):
        return fp.wind_feedback(self.gparams(**over), self.wind, self.age, self.birth, self.old, self.rho0,
                                self.drmin0, check=False)


@functools.lru_cache(maxsize=None)
def _case(periodic):
    return WindCase(periodic)


@functools.lru_cache(maxsize=None)
def _loop_ref(periodic):
    """the restatement of the whole loop, once per boundary kind (read-only afterwards)"""
    c = _case(periodic)
    return R.feedback(c.par, c.fields(), c.wind, c.state(), active=c.active)


UNTOUCHED = ("F_VEL", "F_TYPE", "F_TIMEBIN", "F_ENTROPY", "F_DTENTROPY", "F_VELPRED", "F_TI_BEGSTEP")


@pytest.mark.parametrize("periodic", [0, 1])
def test_density_pass_matches_brute_force(periodic):
    c = _case(periodic)
    B, fp = c.device()
    dtj = c.dt_jump()
    dtj[::7] = -1.0                                     # reset, not evaluated
    before = {f: fp.get_field(getattr(B, f)) for f in UNTOUCHED + ("F_POS", "F_HSML", "F_MASS")}
    rho, drmin = fp.wind_density(c.gparams(), c.wind, dtj)
    M = R.Margins()
    f = c.fields()
    rr, rd = R.density(c.par, R.gas_of(f), f["pos"][c.wind], f["hsml"][c.wind], dtj, M)
    assert M.smallest() >= MARGIN, M.by_kind
    off = ~(dtj > 0)
    assert off.sum() > 60 and np.all(rho[off] == 0) and np.all(drmin[off] == 1.e40)
    assert _scaled_err(rho, rr) < TOL
    assert np.array_equal(drmin == 1.e40, rd == 1.e40) and relerr(drmin, rd) < TOL
    on = dtj > 0
    assert (on & (rr > 0)).sum() > 100                   # in the gas
    assert (on & (rr == 0) & (rd < 1.e40)).sum() > 5     # gas in reach that only sets drmin
    assert (on & (rd == 1.e40)).sum() > 5                # no gas in reach: 0 and 1e40
    for k, v in before.items():                          # a read-only pass
        assert np.array_equal(fp.get_field(getattr(B, k)), v), k
    fp.close()


@pytest.mark.parametrize("periodic", [0, 1])
def test_spread_pass_order_conservation_and_determinism(periodic):
    c = _case(periodic)
    B, fp = c.device()
    pr, f = c.pr, c.fields()
    ng, nw = pr.ngas, len(c.wind)
    dtj = c.dt_jump()
    rho, _ = fp.wind_density(c.gparams(), c.wind, dtj)
    dmom = c.old * (0.1 + 0.5 * np.random.default_rng(9).random(nw))
    before = {k: fp.get_field(getattr(B, k)) for k in UNTOUCHED + ("F_POS", "F_HSML", "F_MASS")}
    assert np.all(fp.wind_injected() == 0)               # zero when first used
    fp.wind_spread(c.gparams(), c.wind, dtj, rho, dmom)
    got = fp.wind_injected()
    M = R.Margins()
    inj = np.zeros((ng, 3), R.LD)
    sp = R.spread(c.par, R.gas_of(f), f["pos"][c.wind], f["hsml"][c.wind], f["vel"][c.wind], dtj, rho, dmom, inj, M)
    assert M.smallest() >= MARGIN, M.by_kind
    assert 100 < len(sp) < nw
    ref = inj.astype(np.float64)
    assert _scaled_err(got, ref) < TOL and np.abs(ref).max() > 0
    # the weights m_j W / new_density sum to 1: what the gas receives is what the spreading particles gave
    v = f["vel"][c.wind][sp]
    given = (dmom[sp][:, None] * v / np.linalg.norm(v, axis=1)[:, None]).sum(axis=0)
    assert np.abs(got.sum(axis=0) - given).max() < 1e-11 * np.abs(dmom[sp]).sum()
    assert np.all(got[c.mass[:ng] == 0] == 0)            # massless gas receives nothing
    for k, val in before.items():
        assert np.array_equal(fp.get_field(getattr(B, k)), val), k
    # the same call from the same state, bit for bit
    fp.set_wind_injected(np.zeros((ng, 3)))
    fp.wind_spread(c.gparams(), c.wind, dtj, rho, dmom)
    assert np.array_equal(fp.wind_injected(), got)
    # the list in reverse order: another order of the sums, the same values to TOL; it adds to what is there
    rev = np.arange(nw)[::-1]
    fp.wind_spread(c.gparams(), c.wind[rev], dtj[rev], rho[rev], dmom[rev])
    assert _scaled_err(fp.wind_injected(), 2 * ref) < TOL
    fp.close()


def _check_loop(c, B, fp, out, ref, start):
    pr = c.pr
    n, ng = pr.n, pr.ngas
    assert out["iterations"] == ref["iterations"] and out["bits"] == ref["bits"]
    assert np.array_equal(out["deleted"], ref["deleted"]) and out["ndeleted"] == ref["ndeleted"]
    assert abs(out["deleted_momentum"] - ref["deleted_momentum"]) <= TOL * max(abs(ref["deleted_momentum"]), 1e-300)
    pos, hsml, mass = fp.get_field(B.F_POS), fp.get_field(B.F_HSML), fp.get_field(B.F_MASS)
    assert _scaled_err(pos[c.wind], ref["pos"][c.wind]) < TOL
    assert relerr(hsml[c.wind], ref["hsml"][c.wind]) < TOL
    assert np.array_equal(mass[c.wind] == 0, ref["mass"][c.wind] == 0)
    assert _scaled_err(mass[c.wind], ref["mass"][c.wind]) < TOL
    for k in ("old_momentum", "dt2", "dt1", "dt_jump", "delta_momentum", "new_density"):
        assert _scaled_err(out[k], ref[k]) < TOL, k
    assert np.array_equal(out["drmin"] == 1.e40, ref["drmin"] == 1.e40) and relerr(out["drmin"], ref["drmin"]) < TOL
    assert _scaled_err(fp.wind_injected(), ref["injected"]) < TOL
    # nothing else changes
    other = np.setdiff1d(np.arange(n), c.wind)
    for f, v in ((B.F_POS, pos), (B.F_HSML, hsml), (B.F_MASS, mass)):
        assert np.array_equal(v[other], start[f][other])
    for k in UNTOUCHED:
        assert np.array_equal(fp.get_field(getattr(B, k)), start[getattr(B, k)]), k


@pytest.mark.parametrize("periodic", [0, 1])
def test_loop_matches_the_restatement(periodic):
    c, ref = _case(periodic), _loop_ref(periodic)
    M = ref["margins"]
    assert M.smallest() >= MARGIN, M.by_kind
    assert set(M.by_kind) == {"search_radius", "u_vs_1", "time_cap", "depletion", "outer_boundary", "virtual_time",
                              "dt_total_floor"}
    assert ref["status"] == "ok" and ref["iterations"] > 8
    # the inputs make particles end each way
    ends = ref["ends"]
    past = ref["deleted"] == 1
    r_end = np.linalg.norm(ref["pos"][c.wind], axis=1)
    old_age = c.par["Time"] - c.age > c.par["VirtualTime"]
    assert len(ends["cap"]) > 50 and len(ends["hidden"]) > 20
    assert (past & (r_end > c.par["OuterBoundary"])).sum() > 3 and (past & old_age).sum() > 50
    assert (ref["deleted"] == 2).sum() > 10 and (ref["deleted"] == 0).sum() > 50
    assert len(ends["grow"]) > 20 and len(ends["hcap"]) > 10 and len(ends["fly"]) > 50
    assert (c.dt_jump() == 0).sum() > 20
    B, fp = c.device()
    fp.set_active(c.active)
    ng = c.pr.ngas
    ra0 = np.random.default_rng(6).standard_normal((ng, 3))      # what the inactive gas keeps
    start = {f: fp.get_field(f) for f in [B.F_POS, B.F_HSML, B.F_MASS] + [getattr(B, k) for k in UNTOUCHED]}
    fp.set_wind_rad_accel(ra0)
    out = c.feedback(fp)
    assert out["rc"] == 0
    _check_loop(c, B, fp, out, ref, start)
    # RAD_ACCEL at the end: RadAccel and the zeroed injection on the active gas only
    touched = ref["rad_touched"]
    assert 300 < touched.sum() < ng
    ra = fp.wind_rad_accel()
    assert _scaled_err(ra[touched], ref["rad_accel"][touched]) < TOL and np.abs(ref["rad_accel"]).max() > 0
    assert np.array_equal(ra[~touched], ra0[~touched])
    assert np.all(fp.wind_injected()[touched] == 0) and np.abs(ref["injected"][~touched]).max() > 0
    assert np.all(ra[touched & (c.timebin[:ng] == 0)] == 0) and (touched & (c.timebin[:ng] == 0)).sum() > 3
    first = (out, fp.get_field(B.F_POS), fp.get_field(B.F_HSML), fp.get_field(B.F_MASS), fp.wind_injected(), ra)
    fp.close()
    # the same call from the same state, bit for bit
    B, fp = c.device()
    fp.set_active(c.active)
    fp.set_wind_rad_accel(ra0)
    again = c.feedback(fp)
    for k in again:
        assert np.array_equal(again[k], first[0][k]), k
    for a, b in zip((fp.get_field(B.F_POS), fp.get_field(B.F_HSML), fp.get_field(B.F_MASS), fp.wind_injected(),
                     fp.wind_rad_accel()), first[1:]):
        assert np.array_equal(a, b)
    fp.close()


def test_the_two_round_trip_rules_differ_on_these_inputs():
    """(CPU only, but about the inputs of the test above: the deviation is exercised by them)"""
    c, ref = _case(0), _loop_ref(0)
    theirs = R.feedback(c.par, c.fields(), c.wind, c.state(), active=c.active, round_trip=True)
    assert theirs["bits"] > ref["bits"] and theirs["iterations"] >= ref["iterations"]


@pytest.mark.parametrize("periodic", [0, 1])
def test_under_the_floor_nothing_changes_and_max_iter_stops(periodic):
    c = _case(periodic)
    B, fp = c.device()
    fp.set_active(c.active)
    watch = [B.F_POS, B.F_HSML, B.F_MASS] + [getattr(B, k) for k in UNTOUCHED]
    start = {f: fp.get_field(f) for f in watch}
    floor = float(c.dt_jump().sum()) * 1.001
    ref = R.feedback(dict(c.par, dt_total_floor=floor), c.fields(), c.wind, c.state(), active=c.active)
    assert ref["status"] == "floor" and ref["margins"].smallest() >= MARGIN
    out = c.feedback(fp, dt_total_floor=floor)
    assert out["rc"] == 0 and out["iterations"] == 0 and out["bits"] == 0 and out["ndeleted"] == 0
    for f in watch:
        assert np.array_equal(fp.get_field(f), start[f])
    assert np.all(fp.wind_injected() == 0) and np.all(fp.wind_rad_accel() == 0)
    for k, v in (("old_momentum", c.old), ("new_density", c.rho0), ("drmin", c.drmin0), ("dt_jump", c.dt_jump())):
        assert np.array_equal(out[k], v), k
    assert not out["deleted"].any() and not out["dt2"].any()
    # max_iter = 2: GHIP_ENOCONV, the state as it stands after two iterations
    ref = R.feedback(dict(c.par, max_iter=2), c.fields(), c.wind, c.state(), active=c.active)
    assert ref["status"] == "noconv" and ref["under_way"] > 100 and ref["margins"].smallest() >= MARGIN
    out = c.feedback(fp, max_iter=2)
    assert out["rc"] == B.GHIP_ENOCONV
    assert ("%d wind particles still under way" % ref["under_way"]) in fp.L.ghip_last_error(fp.h).decode()
    _check_loop(c, B, fp, out, ref, start)
    assert np.all(fp.wind_rad_accel() == 0)              # no RAD_ACCEL, no elimination
    fp.close()


def test_rad_accel_in_the_kick_and_the_drift():
    B = bindings()
    f = KR.bundle(OuterBoundary=300.0, FeedBackVelocity=10.0, dust=0, dust_timestep=0)
    results = {}
    for mode in ("on", "off", "never"):
        p, s, _ = kick_problem(seed=13, ngas=3000, nother=2000, types=(1, 3, 5))
        s["drag"][:] = 0
        s["ddm"][:] = 0
        n, ng = len(s["type"]), len(s["entropy"])
        ra = np.random.default_rng(21).standard_normal((ng, 3)) * 4.0
        fp = kick_device(s, fields=False)
        fp.set_integration_flags(flags_struct(f))
        act = np.random.default_rng(4).permutation(n)[: n // 2].astype(np.int32)
        fp.set_active(act)
        if mode != "never":
            fp.set_wind_rad_accel(ra)
            fp.set_rad_accel(mode == "on")
        fp.advance_timesteps(kick_params(p))
        if mode == "on":
            plain = {k: np.array(v) for k, v in s.items()}
            assert KR.advance_timesteps(p, f, plain, active=act)["rc"] == 0
            assert R.advance_timesteps_rad(p, f, s, ra, active=act)["rc"] == 0
            assert not np.array_equal(s["timebin"], plain["timebin"])      # the criterion sees RadAccel
            assert relerr(s["velpred"], plain["velpred"]) > 0.1             # VelPred is set, not added to
        else:
            assert KR.advance_timesteps(p, f, s, active=act)["rc"] == 0
        kick_check(fp, s)
        s.update(pos=np.zeros((n, 3)), ti_current=np.full(n, p["Ti_Current"], np.int32),
                 divvel=0.1 * np.random.default_rng(2).standard_normal(ng), pressure=np.zeros(ng))
        for key, fld in (("pos", "F_POS"), ("ti_current", "F_TI_CURRENT"), ("divvel", "F_DIVVEL")):
            fp.set_field(getattr(B, fld), s[key])
        for key, fld in (("vel", "F_VEL"), ("density", "F_DENSITY"), ("hsml", "F_HSML"), ("velpred", "F_VELPRED")):
            s[key] = fp.get_field(getattr(B, fld))
        time1 = p["Ti_Current"] + (1 << 22)
        dp = dict(Timebase_interval=p["Timebase_interval"], ComovingIntegrationOn=0, logTimeBegin=0.0,
                  logTimeMax=0.0, MinGasHsml=0.0)
        fp.drift(time1, p["Timebase_interval"])
        vp0 = s["velpred"].copy()
        if mode == "on":
            assert R.drift_rad(dp, f, s, ra, time1) == 0
            dt_hk = (1 << 22) * p["Timebase_interval"]
            plain = vp0 + s["grav"][:ng] * dt_hk + s["hyd"] * dt_hk
            assert relerr(s["velpred"], plain) > 1e-3                       # RadAccel shows in the drift
        else:
            assert KR.drift(dp, f, s, time1) == 0
        assert relerr(fp.get_field(B.F_VELPRED), s["velpred"]) <= 1e-13
        assert relerr(fp.get_field(B.F_POS), s["pos"]) <= 1e-14
        results[mode] = [fp.get_field(getattr(B, k)) for k in ("F_VEL", "F_VELPRED", "F_ENTROPY", "F_DTENTROPY",
                                                               "F_TIMEBIN", "F_TI_BEGSTEP", "F_POS")]
        if mode == "off":
            assert np.array_equal(fp.wind_rad_accel(), ra)                  # resident, and not read
        fp.close()
    # the switch off, with a non-zero RadAccel resident: the bits of a context that never heard of it
    for a, b in zip(results["off"], results["never"]):
        assert np.array_equal(a, b)
    assert not np.array_equal(results["on"][0], results["never"][0])


def test_rad_accel_in_the_pm_kick():
    B = bindings()
    got = {}
    for mode in ("on", "off", "never"):
        p, s, _ = kick_problem(seed=14, ngas=2000, nother=1000, types=(1, 3, 5))
        n, ng = len(s["type"]), len(s["entropy"])
        rng = np.random.default_rng(22)
        ra, pm = rng.standard_normal((ng, 3)) * 4.0, rng.standard_normal((n, 3))
        fp = kick_device(s, fields=False)
        fp.set_field(B.F_GRAVPM, pm)
        if mode != "never":
            fp.set_wind_rad_accel(ra)
            fp.set_rad_accel(mode == "on")
        ti = p["Ti_Current"] + (1 << 20)
        fp.pm_kick(ti, p["Timebase_interval"], 0.0123, -0.0045)
        R.pm_kick_rad(s, pm, ra, ti, p["Timebase_interval"], 0.0123, -0.0045, rad=mode == "on")
        got[mode] = (fp.get_field(B.F_VEL), fp.get_field(B.F_VELPRED))
        assert relerr(got[mode][0], s["vel"]) <= 1e-14 and relerr(got[mode][1], s["velpred"]) <= 1e-13
        fp.close()
    assert np.array_equal(got["off"][0], got["never"][0]) and np.array_equal(got["off"][1], got["never"][1])
    assert np.array_equal(got["on"][0], got["never"][0]) and relerr(got["on"][1], got["never"][1]) > 1e-3


def test_refusals():
    c = _case(0)
    B, fp = c.device(tree=False)
    dtj = c.dt_jump()
    # no tree: the error of the dust passes
    with pytest.raises(B.GhipError, match="call ghip_tree_build first") as e:
        fp.wind_density(c.gparams(), c.wind, dtj)
    assert e.value.code == -90002
    with pytest.raises(B.GhipError, match="call ghip_tree_build first"):
        fp.wind_feedback(c.gparams(), c.wind, c.age, c.birth, c.old, c.rho0, c.drmin0)
    with pytest.raises(B.GhipError, match="call ghip_tree_build first"):
        fp.dust_density(B.DustParams(), c.wind)
    c.pr.device_tree(fp)
    # an index that is not Type 3
    bad = c.wind.copy()
    bad[17] = 3                                           # a gas particle
    start = fp.get_field(B.F_POS)
    for call in (lambda: fp.wind_density(c.gparams(), bad, dtj),
                 lambda: fp.wind_spread(c.gparams(), bad, dtj, dtj, dtj),
                 lambda: fp.wind_feedback(c.gparams(), bad, c.age, c.birth, c.old, c.rho0, c.drmin0)):
        with pytest.raises(B.GhipError, match="not Type 3") as e:
            call()
        assert e.value.code == -90002
    assert np.array_equal(fp.get_field(B.F_POS), start) and np.all(fp.wind_injected() == 0)
    # values held for one ngas are refused after the counts change
    fp.set_wind_injected(np.ones((c.pr.ngas, 3)))
    fp.set_counts(c.pr.n, c.pr.ngas - 1)
    with pytest.raises(B.GhipError, match="ghip_wind_set_injected again"):
        fp.wind_injected()
    fp.close()
    # a sharded context
    B, fp = c.device(tree=False)
    fp.set_shard(0, 2)
    for call in (lambda: fp.wind_density(c.gparams(), c.wind, dtj),
                 lambda: fp.wind_spread(c.gparams(), c.wind, dtj, dtj, dtj),
                 lambda: fp.wind_feedback(c.gparams(), c.wind, c.age, c.birth, c.old, c.rho0, c.drmin0),
                 lambda: fp.wind_injected(), lambda: fp.set_wind_injected(np.zeros((c.pr.ngas, 3))),
                 lambda: fp.wind_rad_accel(), lambda: fp.set_wind_rad_accel(np.zeros((c.pr.ngas, 3))),
                 lambda: fp.set_rad_accel(1)):
        with pytest.raises(B.GhipError, match="single-rank only") as e:
            call()
        assert e.value.code == -90002
    fp.close()
