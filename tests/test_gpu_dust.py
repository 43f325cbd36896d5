"""The dust-gas drag passes (dust.c: dust_density, dust_drag) on the device, through the C-ABI and the
drop-in symbols of libgadget_force.so, against the independent numpy restatement of tests/dust_ref.py
with brute-force neighbour search.  fp64 within 1e-12; fields the passes must not touch bit-unchanged;
two identical calls bit-identical."""
import ctypes as C
import importlib
import time

import numpy as np
import pytest

import dust_ref as R
from common import Problem, SinkProblem, bindings, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-12


def _scaled_err(a, b):
    """max |a - b| over the array, relative to the largest |b| (sums with cancellation)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


class DustCase:
    """A SinkProblem whose Type-2 grains get drag inputs (d1-d3, radius, d7, d9, DustVcoll) chosen so
    that every stopping-time regime of dust.c:385-417 occurs, plus gas that the scatter must skip
    (massless, dt == 0).  `dust` is the grain list in list order.  box: the SinkProblem in a box of that
    size; the accelerations, the grains' summed velocities (d9) and MinEgySpec go with it, the drag inputs
    stay as drawn: they are chosen against the sound speed of (rho, ent), in the physical units of
    dust_ref.params."""

    def __init__(self, periodic, ndust=600, ng=10, seed=7, sp=None, box=1.0):
        sp = sp or SinkProblem(ng=ng, periodic=periodic, nsink=2, ndust=ndust, seed=seed, box=box)
        pr = sp.pr
        self.sp, self.pr = sp, pr
        rng = np.random.default_rng(seed)
        n, ngas = pr.n, pr.ngas
        self.dust = sp.dust.astype(np.int32)
        nd = len(self.dust)
        sp.hsml[self.dust] = 1.1 * pr.ic["spacing"] * (1 + 0.3 * rng.random(nd))
        self.hsml = sp.hsml
        self.mass = pr.ic["mass"].copy()
        self.timebin = pr.timebin.copy()
        gas_zero_mass = rng.choice(ngas, max(ngas // 40, 3), replace=False)
        self.mass[gas_zero_mass] = 0.0
        rest = np.setdiff1d(np.arange(ngas), gas_zero_mass)
        self.timebin[rng.choice(rest, max(ngas // 40, 3), replace=False)] = 0
        self.grav = 0.1 * rng.standard_normal((n, 3)) * box
        self.par = R.params(pr.box, periodic, pr.timebase, MinEgySpec=0.008 * box ** 2)
        par = self.par
        # per-grain drag inputs, by group a % 6: Epstein, Stokes rey < 1, 1 <= rey < 800, rey >= 800,
        # delta_vel == 0, dt == 0
        vel = pr.ic["vel"][self.dust]
        self.rho = 1e-3 * (1 + rng.random(nd))
        self.ent = 0.0156 * (1 + 0.2 * rng.random(nd))
        cs = np.sqrt(8. / np.pi * self.ent * self.rho ** R.GAMMA_MINUS1)
        lam = R.mean_free_path(par, self.rho)
        rstar = 1.5 * lam * par["UnitLength_in_cm"]
        grp = np.arange(nd) % 6
        self.radius = np.where(grp == 0, 0.3 * rstar, 3.0 * rstar)
        rey = np.choose(grp, [1.0, 0.3, 30.0, 3000.0, 0.0, 1.0])
        dv = rey * par["UnitLength_in_cm"] * lam * cs / (6 * self.radius)
        dv = np.where(grp == 0, 0.01, dv)
        d = rng.standard_normal((nd, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        self.gasvel = vel - dv[:, None] * d
        self.gasvel[grp == 4] = vel[grp == 4]
        self.timebin[self.dust[grp == 5]] = 0
        self.d9 = 1e-4 * (1 + rng.random((nd, 3))) * box
        self.vcoll = rng.random(nd)
        self.gas_entropy = pr.entropy * (0.5 + rng.random(ngas))

    def device(self):
        B = bindings()
        pr = self.pr
        fp = pr.device()
        fp.set_field(B.F_MASS, self.mass)
        fp.set_field(B.F_TIMEBIN, self.timebin)
        fp.set_field(B.F_HSML, self.hsml)
        fp.set_field(B.F_ENTROPY, self.gas_entropy)
        fp.set_field(B.F_GRAVACCEL, self.grav)
        pr.device_tree(fp)
        return B, fp

    def gparams(self):
        B = bindings()
        p = B.DustParams()
        for k, v in self.par.items():
            setattr(p, k, v)
        return p

    def ref_density(self, dust=None):
        pr = self.pr
        dust = self.dust if dust is None else dust
        return R.dust_density(pr.ic["pos"], self.mass, pr.ic["type"], self.hsml, dust, pr.box, pr.periodic)

    def ref_grains(self, sel, d7):
        """grain update of the list positions `sel`"""
        i = self.dust[sel]
        dt = np.where(self.timebin[i] > 0, (1 << self.timebin[i]).astype(np.float64), 0.0) * self.par["dt_fac"]
        return R.grain_update(self.par, self.pr.ic["vel"][i], self.mass[i], self.grav[i], dt, self.rho[sel],
                              self.ent[sel], self.gasvel[sel], self.radius[sel], d7, self.d9[sel],
                              self.vcoll[sel])

    def ref_gas(self, order, dmom, de, gas_idx=None, heat0=None):
        """the serial scatter of the grains in list positions `order` (dmom, de: their results, in that
        order), on (copies of) the start state"""
        pr = self.pr
        ng = pr.ngas
        gidx = np.arange(ng) if gas_idx is None else np.asarray(gas_idx)
        vel = pr.ic["vel"][gidx].copy()
        ent = self.gas_entropy[gidx].copy()
        heat = np.zeros(len(gidx)) if heat0 is None else np.array(heat0, np.float64)
        dtg = np.where(self.timebin > 0, (1 << self.timebin).astype(np.float64), 0.0) * self.par["dt_fac_gas"]
        i = self.dust[order]
        c = R.gas_scatter(self.par, pr.ic["pos"][i], self.hsml[i], self.rho[order], dmom, de,
                          pr.ic["pos"], self.mass, pr.ic["type"], ng, dtg, vel, ent, heat, gas_idx=gidx)
        return vel, ent, heat, c

    def drag(self, fp, order, d7):
        return fp.dust_drag(self.gparams(), self.dust[order], self.rho[order], self.ent[order],
                            self.gasvel[order], self.radius[order], d7[order], self.d9[order],
                            self.vcoll[order])


@pytest.mark.parametrize("periodic", [0, 1])
def test_dust_density_matches_brute_force(periodic):
    case = DustCase(periodic)
    B, fp = case.device()
    act = case.dust[::2]                       # the active half of the grains
    before = {f: fp.get_field(f) for f in (B.F_VEL, B.F_MASS, B.F_HSML, B.F_ENTROPY, B.F_POS)}
    got = fp.dust_density(case.gparams(), act)
    ref = case.ref_density(act)
    assert relerr(got, ref) < TOL and np.all(ref > 0)
    for f, v in before.items():                # a read-only pass
        assert np.array_equal(fp.get_field(f), v), f
    fp.close()


@pytest.mark.parametrize("periodic", [0, 1])
def test_dust_drag_grains_gas_order_and_determinism(periodic):
    case = DustCase(periodic)
    pr = case.pr
    n, ng, nd = pr.n, pr.ngas, len(case.dust)
    B, fp = case.device()
    d7 = fp.dust_density(case.gparams(), case.dust)
    assert relerr(d7, case.ref_density()) < TOL
    start = {B.F_VEL: fp.get_field(B.F_VEL), B.F_ENTROPY: fp.get_field(B.F_ENTROPY)}

    def reset():
        for f, v in start.items():
            fp.set_field(f, v)
        fp.set_dust_drag_heating(np.zeros(ng))

    # ---- grain side ----
    order = np.arange(nd)
    reset()
    out = case.drag(fp, order, d7)
    ref = case.ref_grains(order, d7)
    counts = np.bincount(ref["regime"], minlength=6)
    assert np.all(counts >= 5), counts
    vel = fp.get_field(B.F_VEL)
    assert _scaled_err(vel[case.dust], ref["vel"]) < TOL
    assert _scaled_err(out["delta_momentum"], ref["dmom"]) < TOL
    assert _scaled_err(out["delta_energy"], ref["de"]) < TOL
    assert relerr(out["vcoll"], ref["vcoll"]) < TOL
    assert relerr(out["particle_velocity"], ref["d9"]) < TOL
    assert not np.allclose(ref["d9"], case.d9)            # the in-place division shows
    # ---- gas side, list order ----
    gv, ge, gh, c = case.ref_gas(order, out["delta_momentum"], out["delta_energy"])
    assert c["caps"] > 0 and c["floors"] > 0 and c["touched"].max() >= 2
    assert _scaled_err(vel[:ng], gv) < TOL
    assert relerr(fp.get_field(B.F_ENTROPY), ge) < TOL
    heat = fp.dust_drag_heating()
    assert _scaled_err(heat, gh) < TOL and np.abs(gh).max() > 0
    # untouched: gas with dt == 0, massless gas, gas outside every grain's h -- and DM, sinks
    keep = c["touched"] == 0
    assert keep.sum() > 0 and np.all(keep[(case.timebin[:ng] == 0) | (case.mass[:ng] == 0)])
    assert np.array_equal(vel[:ng][keep], start[B.F_VEL][:ng][keep])
    assert np.array_equal(fp.get_field(B.F_ENTROPY)[keep], start[B.F_ENTROPY][keep])
    assert np.all(heat[keep] == 0)
    other = np.setdiff1d(np.arange(ng, n), case.dust)
    assert np.array_equal(vel[other], start[B.F_VEL][other])
    # ---- determinism: the same call from the same state, bit for bit ----
    first = (vel, fp.get_field(B.F_ENTROPY), heat, out)
    reset()
    again = case.drag(fp, order, d7)
    assert np.array_equal(fp.get_field(B.F_VEL), first[0])
    assert np.array_equal(fp.get_field(B.F_ENTROPY), first[1])
    assert np.array_equal(fp.dust_drag_heating(), first[2])
    for k in again:
        assert np.array_equal(again[k], first[3][k]), k
    # ---- a permuted list: the gas receives the grains in the permuted order ----
    perm = np.random.default_rng(11).permutation(nd)
    reset()
    outp = case.drag(fp, perm, d7)
    gvp, gep, ghp, cp = case.ref_gas(perm, outp["delta_momentum"], outp["delta_energy"])
    assert cp["caps"] > 0 and cp["floors"] > 0
    assert relerr(fp.get_field(B.F_ENTROPY), gep) < TOL
    assert _scaled_err(fp.get_field(B.F_VEL)[:ng], gvp) < TOL
    assert _scaled_err(fp.dust_drag_heating(), ghp) < TOL
    assert not np.array_equal(gep, ge)                    # the order matters under the cap and floor
    fp.close()


def test_dust_passes_refuse_sharded_contexts():
    B = bindings()
    case = DustCase(1, ndust=60, ng=6)
    for how in ("shard", "dd"):
        _, fp = case.device()
        if how == "shard":
            fp.set_shard(0, 2)
        else:
            fp.dd_init(0, 2)
        with pytest.raises(B.GhipError) as e:
            fp.dust_density(case.gparams(), case.dust)
        assert e.value.code == -90002 and "single-rank" in str(e.value)
        with pytest.raises(B.GhipError) as e:
            case.drag(fp, np.arange(len(case.dust)), np.ones(len(case.dust)))
        assert e.value.code == -90002
        fp.close()


# ---- the drop-in: the shipped bundle's 536 / 264-byte records, dust members in their spare bytes ----
P536D = np.dtype({
    "names": ["Pos", "Vel", "Mass", "ID", "GravAccel", "OldAcc", "GravCost", "Ti_begstep", "Ti_current",
              "Type", "TimeBin", "Hsml", "NumNgb", "SwallowID", "BH_Mass", "BH_Mdot", "BH_Density",
              "BH_Entropy", "BH_SurroundingGasVel", "DUST_Density", "DUST_Entropy",
              "DUST_SurroundingGasVel", "DUST_particle_density", "DUST_particle_velocity",
              "DeltaDustMomentum", "NewDragAcc", "DeltaDragEnergy", "DustRadius", "DustVcoll", "rest"],
    "formats": [("f8", 3), ("f8", 3), "f8", "u4", ("f8", 3), "f8", "f4", "i4", "i4", "i2", "i2", "f8",
                "f8", "u4", "f8", "f8", "f8", "f8", ("f8", 3), "f8", "f8", ("f8", 3), "f8", ("f8", 3),
                ("f8", 3), ("f8", 3), "f8", "f8", "f8", ("u1", 144)],
    "offsets": [0, 24, 48, 56, 64, 88, 96, 100, 104, 108, 110, 112, 120, 128, 136, 144, 152, 160, 168,
                240, 248, 256, 288, 296, 320, 344, 368, 376, 384, 392],
    "itemsize": 536})
S264D = np.dtype({
    "names": ["Entropy", "Pressure", "VelPred", "MaxSignalVel", "Density", "DtEntropy", "HydroAccel",
              "DhsmlDensityFactor", "DivVel", "Rot", "Injected_BH_Energy", "DragHeating", "rest"],
    "formats": ["f8", "f8", ("f8", 3), "f8", "f8", "f8", ("f8", 3), "f8", "f8", ("f8", 3), "f8", "f8",
                ("u1", 120)],
    "offsets": [0, 8, 16, 40, 48, 56, 64, 88, 96, 104, 128, 136, 144],
    "itemsize": 264})
ALLD = np.dtype({"names": ["MeanWeight", "UnitDensity_in_cgs", "UnitVelocity_in_cm_per_s", "pad"],
                 "formats": ["f8", "f8", "f8", ("u1", 40)], "offsets": [8, 24, 48, 56], "itemsize": 96})


def _layouts(B, H):
    lay = B.Layout()
    C.memset(C.byref(lay), 0xff, C.sizeof(lay))
    lay.p_stride, lay.s_stride = P536D.itemsize, S264D.itemsize
    for name, key in (("Pos", "p_pos"), ("Vel", "p_vel"), ("Mass", "p_mass"), ("GravAccel", "p_gravaccel"),
                      ("OldAcc", "p_oldacc"), ("GravCost", "p_gravcost"), ("Ti_begstep", "p_ti_begstep"),
                      ("Ti_current", "p_ti_current"), ("Type", "p_type"), ("TimeBin", "p_timebin"),
                      ("Hsml", "p_hsml"), ("NumNgb", "p_numngb")):
        setattr(lay, key, P536D.fields[name][1])
    for name, key in (("Entropy", "s_entropy"), ("Pressure", "s_pressure"), ("VelPred", "s_velpred"),
                      ("MaxSignalVel", "s_maxsignalvel"), ("Density", "s_density"),
                      ("DtEntropy", "s_dtentropy"), ("HydroAccel", "s_hydroaccel"),
                      ("DhsmlDensityFactor", "s_dhsmlfac"), ("DivVel", "s_divvel"), ("Rot", "s_curlvel")):
        setattr(lay, key, S264D.fields[name][1])
    bh = H.BhLayout()
    C.memset(C.byref(bh), 0xff, C.sizeof(bh))
    for name, key in (("ID", "p_id"), ("SwallowID", "p_swallowid"), ("BH_Mass", "p_bh_mass"),
                      ("BH_Mdot", "p_bh_mdot"), ("BH_Density", "p_bh_density"),
                      ("BH_Entropy", "p_bh_entropy"), ("BH_SurroundingGasVel", "p_bh_gasvel"),
                      ("DUST_Density", "p_dust_density"), ("DUST_Entropy", "p_dust_entropy"),
                      ("DUST_SurroundingGasVel", "p_dust_gasvel")):
        setattr(bh, key, P536D.fields[name][1])
    bh.s_injected_bh_energy = S264D.fields["Injected_BH_Energy"][1]
    du = H.DustLayout()
    for name, key in (("DUST_particle_density", "p_particle_density"),
                      ("DUST_particle_velocity", "p_particle_velocity"),
                      ("DeltaDustMomentum", "p_delta_momentum"), ("NewDragAcc", "p_new_drag_acc"),
                      ("DeltaDragEnergy", "p_delta_energy"), ("DustRadius", "p_radius"),
                      ("DustVcoll", "p_vcoll")):
        setattr(du, key, P536D.fields[name][1])
    du.s_drag_heating = S264D.fields["DragHeating"][1]
    du.a_mean_weight = ALLD.fields["MeanWeight"][1]
    du.a_unit_density = ALLD.fields["UnitDensity_in_cgs"][1]
    du.a_unit_velocity = ALLD.fields["UnitVelocity_in_cm_per_s"][1]
    return lay, bh, du


def _host(case, H, B, nranks=1):
    pr, sp = case.pr, case.sp
    lay, bh, du = _layouts(B, H)
    P = np.zeros(pr.n, P536D)
    S = np.zeros(pr.ngas, S264D)
    rng = np.random.default_rng(2)
    P["rest"] = rng.integers(0, 255, (pr.n, 144), dtype=np.uint8)
    S["rest"] = rng.integers(0, 255, (pr.ngas, 120), dtype=np.uint8)
    P["Pos"], P["Vel"], P["Mass"], P["Type"] = pr.ic["pos"], pr.ic["vel"], case.mass, pr.ic["type"]
    P["ID"], P["TimeBin"], P["Hsml"], P["GravAccel"] = sp.ids, case.timebin, case.hsml, case.grav
    S["VelPred"], S["Entropy"], S["DtEntropy"] = pr.velpred, case.gas_entropy, pr.dtentropy
    S["DragHeating"] = 1e-28 * rng.random(pr.ngas)           # in/out: the step's heating adds to it
    d = case.dust
    P["DustRadius"][d], P["DUST_particle_velocity"][d], P["DustVcoll"][d] = case.radius, case.d9, case.vcoll
    P["NewDragAcc"][d] = 5.0
    A = np.zeros(1, ALLD)
    A["MeanWeight"], A["UnitDensity_in_cgs"] = case.par["MeanWeight"], case.par["UnitDensity_in_cgs"]
    A["UnitVelocity_in_cm_per_s"] = case.par["UnitVelocity_in_cm_per_s"]
    host = H.Host(periodic=pr.periodic, black_holes=1, dust=1, accretion_of_dust_only=1, accretion_density=1,
                  rank=0, nranks=nranks)
    host.bind_records(P, S, lay, bh)
    host.bind_dust(A, du)
    a = host.All
    a.G, a.ErrTolTheta, a.ErrTolForceAcc, a.TypeOfOpeningCriterion = pr.G, pr.theta, pr.ErrTolForceAcc, 0
    a.BoxSize, a.DesNumNgb, a.MaxNumNgbDeviation = pr.box, pr.des_ngb, pr.max_dev
    a.ArtBulkViscConst, a.Ti_Current, a.Timebase_interval = pr.visc, pr.ti_current, pr.timebase
    a.ComovingIntegrationOn, a.MinGasHsmlFractional = 0, 0.0
    eps = pr.force_soft[0] / 2.8
    for name in ("Gas", "Halo", "Disk", "Bulge", "Stars", "Bndry"):
        setattr(a, "Softening" + name, eps)
    a.MinEgySpec = case.par["MinEgySpec"]
    a.UnitLength_in_cm, a.UnitMass_in_g = case.par["UnitLength_in_cm"], case.par["UnitMass_in_g"]
    host.L.set_softenings()
    host.set_active(None)
    host.domain()
    return host, P, S, A


@pytest.mark.parametrize("periodic", [0, 1])
def test_dropin_density_then_dust_passes_on_bundle_records(periodic):
    B = bindings()
    H = importlib.import_module("gadget-leicester_amd.hostapi")
    case = DustCase(periodic, ndust=300)
    pr = case.pr
    ng, d = pr.ngas, case.dust
    host, P, S, A = _host(case, H, B)
    try:
        L = host.L
        L.density()                               # fills Hsml and d1-d3 of the grains (Type-2 targets)
        assert host.endrun_codes == [], L.gadget_force_last_error()
        # the grains' drag inputs as density() left them
        case.hsml = P["Hsml"].copy()
        case.rho, case.ent = P["DUST_Density"][d].copy(), P["DUST_Entropy"][d].copy()
        case.gasvel = P["DUST_SurroundingGasVel"][d].copy()
        assert np.all(case.rho > 0)
        keep = P.copy()
        keep_s = S.copy()
        L.dust_density()
        assert host.endrun_codes == [], L.gadget_force_last_error()
        d7 = case.ref_density()
        assert relerr(P["DUST_particle_density"][d], d7) < TOL
        L.dust_drag()
        assert host.endrun_codes == [], L.gadget_force_last_error()
        ref = case.ref_grains(np.arange(len(d)), P["DUST_particle_density"][d])
        assert _scaled_err(P["Vel"][d], ref["vel"]) < TOL
        assert _scaled_err(P["DeltaDustMomentum"][d], ref["dmom"]) < TOL
        assert _scaled_err(P["DeltaDragEnergy"][d], ref["de"]) < TOL
        assert relerr(P["DustVcoll"][d], ref["vcoll"]) < TOL
        assert relerr(P["DUST_particle_velocity"][d], ref["d9"]) < TOL
        assert np.all(P["NewDragAcc"][d] == 0)
        gv, ge, gh, c = case.ref_gas(np.arange(len(d)), P["DeltaDustMomentum"][d], P["DeltaDragEnergy"][d],
                                     heat0=keep_s["DragHeating"])
        assert c["touched"].max() >= 2
        assert _scaled_err(P["Vel"][:ng], gv) < TOL
        assert relerr(S["Entropy"], ge) < TOL
        assert _scaled_err(S["DragHeating"], gh) < TOL and not np.array_equal(gh, keep_s["DragHeating"])
        # nothing else in either record
        written = {"Vel", "DUST_particle_density", "DUST_particle_velocity", "DeltaDustMomentum", "NewDragAcc",
                   "DeltaDragEnergy", "DustVcoll"}
        for name in P536D.names:
            if name not in written:
                assert np.array_equal(P[name], keep[name]), name
        other = np.setdiff1d(np.arange(ng, pr.n), d)
        assert np.array_equal(P["Vel"][other], keep["Vel"][other])
        for name in ("DUST_particle_density", "DUST_particle_velocity", "DeltaDustMomentum", "NewDragAcc",
                     "DeltaDragEnergy", "DustVcoll"):
            assert np.array_equal(P[name][other], keep[name][other]), name
        for name in S264D.names:
            if name not in ("Entropy", "DragHeating"):
                assert np.array_equal(S[name], keep_s[name]), name
    finally:
        host.close()


def test_dropin_refuses_more_than_one_rank():
    B = bindings()
    H = importlib.import_module("gadget-leicester_amd.hostapi")
    case = DustCase(1, ndust=60, ng=6)
    host, P, S, A = _host(case, H, B, nranks=2)
    try:
        keep = P.copy()
        host.L.dust_density()
        host.L.dust_drag()
        assert host.endrun_codes == [90010, 90010]
        assert b"single rank" in host.L.gadget_force_last_error()
        assert np.array_equal(P, keep)
    finally:
        host.close()


def test_dust_passes_at_c2_size_with_timings():
    """64^3 gas, a quarter of the other particles re-typed as grains: an exact sample of 2048 grains
    and 512 gas particles, and the device time of both passes next to ghip_density's"""
    ng = 64
    pr = Problem(ng=ng, gas=True, periodic=1)
    n, ngas = pr.n, pr.ngas
    ndust = (n - ngas) // 4
    sp = SinkProblem.__new__(SinkProblem)
    rng = np.random.default_rng(9)
    sp.pr = pr
    sp.dust = np.sort(rng.choice(np.arange(ngas, n), ndust, replace=False))
    typ = pr.ic["type"].copy()
    typ[sp.dust] = 2
    pr.ic["type"] = typ
    sp.hsml = pr.hsml0.copy()
    sp.ids = np.arange(n, dtype=np.uint32)
    case = DustCase(1, sp=sp, seed=9)
    B, fp = case.device()
    dp = pr.g_dens()
    fp.set_active(np.arange(ngas, dtype=np.int32))
    t0 = time.perf_counter()
    fp.density(dp)
    t_dens = time.perf_counter() - t0
    p = case.gparams()
    fp.dust_density(p, case.dust)          # warm-up (allocations)
    t0 = time.perf_counter()
    d7 = fp.dust_density(p, case.dust)
    t_dd = time.perf_counter() - t0
    order = np.arange(ndust)
    start = (fp.get_field(B.F_VEL), fp.get_field(B.F_ENTROPY))
    case.drag(fp, order, d7)               # warm-up
    fp.set_field(B.F_VEL, start[0])
    fp.set_field(B.F_ENTROPY, start[1])
    fp.set_dust_drag_heating(np.zeros(ngas))
    t0 = time.perf_counter()
    out = case.drag(fp, order, d7)
    t_drag = time.perf_counter() - t0
    print("\n  c2-size dust passes: %d gas, %d grains: ghip_density %.2f ms (%.2f ms device), "
          "ghip_dust_density %.2f ms, ghip_dust_drag %.2f ms"
          % (ngas, ndust, 1e3 * t_dens, fp.stats()["ms_dens"], 1e3 * t_dd, 1e3 * t_drag))
    # grain side on a sample
    sel = np.sort(rng.choice(ndust, 2048, replace=False))
    assert relerr(d7[sel], case.ref_density(case.dust[sel])) < TOL
    ref = case.ref_grains(sel, d7[sel])
    vel = fp.get_field(B.F_VEL)
    assert _scaled_err(vel[case.dust[sel]], ref["vel"]) < TOL
    assert _scaled_err(out["delta_momentum"][sel], ref["dmom"]) < TOL
    assert _scaled_err(out["delta_energy"][sel], ref["de"]) < TOL
    assert relerr(out["vcoll"][sel], ref["vcoll"]) < TOL
    # gas side on a sample: every grain scanned for each sampled particle, applied in list order
    gs = np.sort(rng.choice(ngas, 512, replace=False))
    gv, ge, gh, c = case.ref_gas(order, out["delta_momentum"], out["delta_energy"], gas_idx=gs)
    assert c["touched"].max() >= 2
    assert _scaled_err(vel[gs], gv) < TOL
    assert relerr(fp.get_field(B.F_ENTROPY)[gs], ge) < TOL
    assert _scaled_err(fp.dust_drag_heating()[gs], gh) < TOL
    fp.close()
