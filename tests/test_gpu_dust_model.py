"""The dust model on the device (ghip_set_dust_model: DUST_GROWTH, DUST_REAL_PEBBLE_COLLISIONS, DUST_VAPORIZE,
DUST_FE_AND_ICE_GRAINS, DUST_EPSTEIN, DUST_NO_FRICTION_HEATING) through ghip_dust_density_grains /
ghip_dust_drag_grains, GHIP_DD_DUST_DENSITY / GHIP_DD_DUST_DRAG in the GHIP_DUST_GRAINS_FORM on logical shards and the drop-in
symbols, against the numpy restatement of tests/dust_model_ref.py on the case of tests/dust_model_case.py.  fp64
within 1e-12 (TOL of test_gpu_dust.py); off means off, bit for bit; two identical calls bit-identical."""
import ctypes as C
import importlib

import numpy as np
import pytest

import dust_model_case as DC
import dust_model_ref as MR
from common import bindings, relerr
from test_gpu_dust import P536D, TOL, _host, _scaled_err
from test_gpu_dust_dd import DdDust

pytestmark = pytest.mark.gpu

SETS = [("epstein",), ("no_friction_heating",), ("growth",), ("growth", "real_pebble_collisions"),
        ("growth", "vaporize"), ("growth", "vaporize", "fe_and_ice_grains"), DC.ALL_SIX]


def _device(case, ids=None):
    B, fp = case.device()
    fp.set_field(B.F_ID, (case.sp.ids if ids is None else ids).astype(np.int32))
    return B, fp


def _drag(fp, case, m, d7, sel=None, logr=True):
    sel = np.arange(len(case.dust)) if sel is None else sel
    return fp.dust_drag_grains(case.gparams(), case.dust[sel], case.rho[sel], case.ent[sel], case.gasvel[sel],
                               case.radius[sel], d7[sel], case.d9_in(m)[sel], case.vcoll[sel],
                               log_radius_by_dt=case.logr0[sel], logr=logr)


def _check_grains(out, ref, vel_dust):
    """the grain side of a drag pass against the reference"""
    err = dict(vel=_scaled_err(vel_dust, ref["vel"]), dmom=_scaled_err(out["delta_momentum"], ref["dmom"]),
               de=_scaled_err(out["delta_energy"], ref["de"]), vcoll=relerr(out["vcoll"], ref["vcoll"]),
               d9=_scaled_err(out["particle_velocity"], ref["d9"]), radius=relerr(out["dust_radius"], ref["radius"]),
               logr=relerr(out["log_radius_by_dt"], ref["logr"]))
    print("  grain errors: " + ", ".join("%s %.2e" % kv for kv in err.items()))
    for k, v in err.items():
        assert v < TOL, (k, v)


# ---- 1. density -----------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic", [0, 1])
def test_density_sums_the_neighbours_velocities(periodic):
    case = DC.case(periodic)
    B, fp = _device(case)
    try:
        act = case.dust[::2]                       # the active half of the grains
        p = case.gparams()
        d7_old = fp.dust_density(p, act)
        before = {f: fp.get_field(f) for f in (B.F_VEL, B.F_MASS, B.F_HSML, B.F_ENTROPY, B.F_POS)}
        m = case.model("real_pebble_collisions")
        fp.set_dust_model(case.gmodel(m))
        out = fp.dust_density_grains(p, act)
        d7, d9 = case.base()
        print("  d9 %.2e d7 %.2e" % (_scaled_err(out["particle_velocity"], d9[::2]),
                                     relerr(out["particle_density"], d7[::2])))
        assert _scaled_err(out["particle_velocity"], d9[::2]) < TOL and np.abs(d9).max() > 0
        assert relerr(out["particle_density"], d7[::2]) < TOL
        assert np.array_equal(out["particle_density"], d7_old)
        # without real_pebble_collisions the d9 array handed in comes back untouched
        fp.set_dust_model(case.gmodel(case.model("growth", "epstein")))
        mark = np.random.default_rng(3).random((len(act), 3))
        g, a = B.dust_grains(act, particle_velocity=mark)
        fp._chk(fp.L.ghip_dust_density_grains(fp.h, C.byref(p), C.byref(g)))
        assert np.array_equal(a["particle_velocity"], mark) and np.array_equal(a["particle_density"], d7_old)
        for f, v in before.items():                # a read-only pass
            assert np.array_equal(fp.get_field(f), v), f
    finally:
        fp.close()


# ---- 2. drag under every switch set ---------------------------------------------------------------
@pytest.mark.parametrize("switches,periodic", [(s, 1) for s in SETS] + [(DC.ALL_SIX, 0)],
                         ids=["+".join(s) + ("" if per else "-open") for s, per in
                              [(s, 1) for s in SETS] + [(DC.ALL_SIX, 0)]])
def test_drag_under_the_switches(switches, periodic):
    case = DC.case(periodic)
    ng, nd = case.pr.ngas, len(case.dust)
    B, fp = _device(case)
    try:
        m = case.model(*switches)
        fp.set_dust_model(case.gmodel(m))
        d7 = case.base()[0]
        out = _drag(fp, case, m, d7)
        ref = case.ref_model(m)
        vel = fp.get_field(B.F_VEL)
        _check_grains(out, ref, vel[case.dust])
        # log_radius_by_dt keeps the caller's value exactly where dust.c:465 does not write; so does the radius
        # without growth
        kept = ~ref["gate"]
        assert np.array_equal(out["log_radius_by_dt"][kept], case.logr0[kept])
        if m["growth"]:
            assert ref["gate"].sum() >= 5 and not np.array_equal(out["dust_radius"], case.radius)
            assert np.all(out["log_radius_by_dt"][~kept] != case.logr0[~kept])
        else:
            assert kept.all() and np.array_equal(out["dust_radius"], case.radius)
        if m["vaporize"]:
            assert (out["delta_energy"] < 0).sum() >= 5          # vaporising grains cool the gas
        # the gas side, fed with the device's own grain results
        gv, ge, gh, c = case.ref_gas(np.arange(nd), out["delta_momentum"], out["delta_energy"])
        assert c["touched"].max() >= 2
        assert _scaled_err(vel[:ng], gv) < TOL
        assert relerr(fp.get_field(B.F_ENTROPY), ge) < TOL
        assert _scaled_err(fp.dust_drag_heating(), gh) < TOL
        assert (np.abs(gh).max() > 0) == bool(out["delta_energy"].any())   # (no_friction_heating alone: none)
        assert np.all(ge > 0)
    finally:
        fp.close()


# ---- 3. the gates, each in a call of its own ------------------------------------------------------
@pytest.mark.parametrize("over", [dict(Time=0.5, VirtualTime=0.5), dict(Time=0.0, VirtualTime=-1.0),
                                  dict(FragmentationVelocity=0.0999)],
                         ids=["Time<=VirtualTime", "Time<=0", "FragmentationVelocity<0.1"])
def test_gates(over):
    case = DC.case(1)
    B, fp = _device(case)
    try:
        m = case.model(*DC.ALL_SIX, **over)
        fp.set_dust_model(case.gmodel(m))
        out = _drag(fp, case, m, case.base()[0])
        ref = case.ref_model(m)
        _check_grains(out, ref, fp.get_field(B.F_VEL)[case.dust])
        if "Time" in over:                         # a closed gate: no t_coll anywhere, vapour and clamps still act
            assert not ref["gate"].any() and np.array_equal(out["log_radius_by_dt"], case.logr0)
            assert ref["lo"].sum() >= 5 and (ref["vap"] > 0).sum() >= 5
        else:                                      # no growth at all: t_coll written, nothing grows
            assert ref["gate"].all() and not ref["hi"].any()
            assert np.all(out["log_radius_by_dt"] != case.logr0)
            assert np.all(out["dust_radius"] <= np.clip(case.radius, 0.1, 1e5))
    finally:
        fp.close()


# ---- 4. off means off -----------------------------------------------------------------------------
def test_off_means_off_and_the_refusals():
    case = DC.case(1)
    nd = len(case.dust)
    B, fp = _device(case)
    try:
        p = case.gparams()
        start = {f: fp.get_field(f) for f in (B.F_VEL, B.F_ENTROPY)}

        def reset():
            for f, v in start.items():
                fp.set_field(f, v)
            fp.set_dust_drag_heating(np.zeros(case.pr.ngas))

        off = case.model()
        d7_old = fp.dust_density(p, case.dust)
        old = case.drag(fp, np.arange(nd), d7_old)
        old_state = (fp.get_field(B.F_VEL), fp.get_field(B.F_ENTROPY), fp.dust_drag_heating())
        for setting in (None, case.gmodel(off)):
            fp.set_dust_model(setting)
            reset()
            dn = fp.dust_density_grains(p, case.dust)
            assert np.array_equal(dn["particle_density"], d7_old) and not dn["particle_velocity"].any()
            new = _drag(fp, case, off, d7_old)
            for k in old:
                assert np.array_equal(new[k], old[k]), k
            assert np.array_equal(new["dust_radius"], case.radius)
            assert np.array_equal(new["log_radius_by_dt"], case.logr0)
            for got, want in zip((fp.get_field(B.F_VEL), fp.get_field(B.F_ENTROPY), fp.dust_drag_heating()),
                                 old_state):
                assert np.array_equal(got, want)
        # the old entry points refuse exactly the switch sets they cannot serve, naming the new ones; the setter
        # refuses each invalid input; nothing of it launches a kernel
        reset()
        fp.sync()
        fp.run_begin(1)
        for sw in SETS:
            m = case.model(*sw)
            fp.set_dust_model(case.gmodel(m))
            if m["real_pebble_collisions"]:
                with pytest.raises(B.GhipError) as e:
                    fp.dust_density(p, case.dust)
                assert e.value.code == -90002 and "ghip_dust_density_grains" in str(e.value)
            if m["growth"] or m["vaporize"]:
                with pytest.raises(B.GhipError) as e:
                    case.drag(fp, np.arange(nd), d7_old)
                assert e.value.code == -90002 and "ghip_dust_drag_grains" in str(e.value)
        fp.set_dust_model(None)
        bad = [dict(Time=np.nan), dict(VirtualTime=np.inf), dict(FragmentationVelocity=-np.inf),
               dict(InitialDustRadius=np.nan), dict(UnitEnergy_in_cgs=np.inf)]
        for over in bad:
            with pytest.raises(B.GhipError) as e:
                fp.set_dust_model(case.gmodel(case.model("growth", **over)))
            assert e.value.code == -90002 and "not finite" in str(e.value)
        for sw, over, word in ((("vaporize",), {}, "growth"), (("growth", "fe_and_ice_grains"), {}, "vaporize"),
                               (("growth", "vaporize"), dict(InitialDustRadius=0.1), "InitialDustRadius")):
            with pytest.raises(B.GhipError) as e:
                fp.set_dust_model(case.gmodel(case.model(*sw, **over)))
            assert e.value.code == -90002 and word in str(e.value)
        assert fp.run_end()["launches"] == 0
        # ... and the model is still off: a refused setting changes nothing
        assert np.array_equal(fp.dust_density(p, case.dust), d7_old)
        # the old entry points honour epstein / no_friction_heating
        for sw in (("epstein",), ("no_friction_heating",)):
            m = case.model(*sw)
            fp.set_dust_model(case.gmodel(m))
            reset()
            o = case.drag(fp, np.arange(nd), d7_old)
            ref = case.ref_model(m, d7=d7_old)
            assert _scaled_err(o["delta_energy"], ref["de"]) < TOL
            assert _scaled_err(fp.get_field(B.F_VEL)[case.dust], ref["vel"]) < TOL
            assert not np.array_equal(o["delta_energy"], old["delta_energy"])
        # fe_and_ice_grains reads GHIP_F_ID: a context that never got the IDs refuses
        _, fp2 = case.device()
        try:
            fp2.set_dust_model(case.gmodel(case.model("growth", "vaporize", "fe_and_ice_grains")))
            with pytest.raises(B.GhipError) as e:
                _drag(fp2, case, case.model("growth"), d7_old)
            assert e.value.code == -90002 and "GHIP_F_ID" in str(e.value)
            fp2.set_shard(0, 2)                    # a context of ghip_set_shard refuses the setting
            with pytest.raises(B.GhipError) as e:
                fp2.set_dust_model(case.gmodel(case.model("growth")))
            assert e.value.code == -90002 and "ghip_set_shard" in str(e.value)
        finally:
            fp2.close()
    finally:
        fp.close()


# ---- 5. determinism -------------------------------------------------------------------------------
def test_two_identical_calls_are_bit_identical():
    case = DC.case(1)
    B, fp = _device(case)
    try:
        m = case.model(*DC.ALL_SIX)
        fp.set_dust_model(case.gmodel(m))
        start = {f: fp.get_field(f) for f in (B.F_VEL, B.F_ENTROPY)}
        res = []
        for _ in range(2):
            for f, v in start.items():
                fp.set_field(f, v)
            fp.set_dust_drag_heating(np.zeros(case.pr.ngas))
            dn = fp.dust_density_grains(case.gparams(), case.dust)
            out = _drag(fp, case, m, dn["particle_density"])
            res.append(dict(out, **dn, gas_vel=fp.get_field(B.F_VEL), ent=fp.get_field(B.F_ENTROPY),
                            heat=fp.dust_drag_heating()))
        for k in res[0]:
            assert np.array_equal(res[0][k], res[1][k]), k
    finally:
        fp.close()


# ---- 6. shards ------------------------------------------------------------------------------------
class DdModel(DdDust):
    """the case on logical shards with the trees of the step (DdDust of test_gpu_dust_dd.py), driven through
    either pair of operations"""

    def set_model(self, m):
        for fp in self.S.fp:
            fp.set_dust_model(None if m is None else self.case.gmodel(m))

    def run(self, op, grains, d7=None, d9=None):
        """operation `op` (density or drag) in the old form or the grains form on all shards -> (outputs in
        list order, counts)"""
        B, c = self.B, self.case
        drag = op == B.DD_DUST_DRAG
        built = []
        for r in range(self.P):
            o = self.lists[r]
            kw = {}
            if drag:
                kw = dict(particle_density=d7[o], dust_density=c.rho[o], dust_entropy=c.ent[o],
                          dust_gasvel=c.gasvel[o], dust_radius=c.radius[o], particle_velocity=d9[o],
                          vcoll=c.vcoll[o])
                if grains:
                    kw["log_radius_by_dt"] = c.logr0[o]
            built.append((B.dd_dust_grains_args if grains else B.dd_dust_args)(c.gparams(), self.local[r], **kw))
        self.S.run.run(op, [b[0] for b in built], B.DUST_GRAINS_FORM if grains else 0)
        nd = len(c.dust)
        keys = [k for k in ("particle_density", "particle_velocity", "delta_momentum", "delta_energy", "vcoll",
                            "dust_radius", "log_radius_by_dt") if k in built[0][1]]
        out = {k: np.zeros((nd,) + built[0][1][k].shape[1:]) for k in keys}
        for r, b in enumerate(built):
            for k in keys:
                out[k][self.lists[r]] = b[1][k]
        return out, [b[1]["counts"].copy() for b in built]


@pytest.mark.parametrize("nshards,periodic", [(2, 1), (3, 0)])
def test_shards_against_the_single_gpu_call(nshards, periodic):
    case = DC.case(periodic)
    pr = case.pr
    n, ng = pr.n, pr.ngas
    B = bindings()
    m = case.model(*DC.ALL_SIX)
    # one GPU, with the shards' IDs (the global index)
    _, fp = _device(case, ids=np.arange(n))
    try:
        fp.set_dust_model(case.gmodel(m))
        one_d = fp.dust_density_grains(case.gparams(), case.dust)
        one = fp.dust_drag_grains(case.gparams(), case.dust, case.rho, case.ent, case.gasvel, case.radius,
                                  one_d["particle_density"], one_d["particle_velocity"], case.vcoll,
                                  log_radius_by_dt=case.logr0)
        one_state = (fp.get_field(B.F_VEL), fp.get_field(B.F_ENTROPY), fp.dust_drag_heating())
    finally:
        fp.close()
    T = DdModel(case, nshards)
    try:
        vel0, ent0 = T.S.get_field(B.F_VEL), T.S.get_field(B.F_ENTROPY)
        # without real_pebble_collisions not a byte more travels than in the old form of the operations
        T.set_model(None)
        d_old, c_old = T.run(B.DD_DUST_DENSITY, False)
        T.set_model(case.model("growth", "vaporize", "fe_and_ice_grains", "epstein", "no_friction_heating"))
        d_new, c_new = T.run(B.DD_DUST_DENSITY, True)
        assert np.array_equal(d_new["particle_density"], d_old["particle_density"])
        assert not d_new["particle_velocity"].any()
        assert [int(c[3]) for c in c_new] == [int(c[3]) for c in c_old] and sum(int(c[0]) for c in c_old) > 0
        # with it, 24 bytes more per returned record
        T.set_model(m)
        d_peb, c_peb = T.run(B.DD_DUST_DENSITY, True)
        for r in range(nshards):
            assert int(c_peb[r][0]) == int(c_old[r][0]) and int(c_peb[r][1]) == int(c_old[r][1])
            assert int(c_peb[r][3]) == int(c_old[r][3]) + 24 * int(c_old[r][1])   # (records it received, returned)
        assert relerr(d_peb["particle_density"], one_d["particle_density"]) < TOL
        assert _scaled_err(d_peb["particle_velocity"], one_d["particle_velocity"]) < TOL
        # the old form refuses as the old entry points do, on every shard, before anything is posted
        for op, word in ((B.DD_DUST_DENSITY, "GHIP_DUST_GRAINS_FORM"), (B.DD_DUST_DRAG, "GHIP_DUST_GRAINS_FORM")):
            for r, f in enumerate(T.S.fp):
                with pytest.raises(B.GhipError) as e:
                    f.dd_begin(op, B.dd_dust_args(case.gparams(), T.local[r],
                                                  particle_density=np.ones(len(T.local[r])))[0])
                assert e.value.code == -90002 and word in str(e.value)
        # the drag pass: same inputs as the single-GPU call
        out, c_drag = T.run(B.DD_DUST_DRAG, True, d7=one_d["particle_density"], d9=one_d["particle_velocity"])
        for k in ("particle_velocity", "delta_momentum", "delta_energy"):
            assert _scaled_err(out[k], one[k]) < TOL, k
        for k in ("vcoll", "dust_radius", "log_radius_by_dt"):
            assert relerr(out[k], one[k]) < TOL, k
        vel, ent, heat = T.S.get_field(B.F_VEL), T.S.get_field(B.F_ENTROPY), T.heat()
        assert _scaled_err(vel[case.dust], one_state[0][case.dust]) < TOL
        # the gas receives the grains in the per-rank order, the single GPU in list order, and the cap and the
        # floor of the entropy update bind in this case: the gas side is compared with the per-rank restatement
        gv, ge, gh, counts = T.ref_gas(out)
        for r in range(nshards):
            assert int(c_drag[r][2]) == int(counts[r]["touched"].sum()), r
        assert _scaled_err(vel[:ng], gv) < TOL and relerr(ent, ge) < TOL and _scaled_err(heat, gh) < TOL
        assert _scaled_err(one_state[0][:ng], gv) < 1e-3 and np.abs(gh).max() > 0   # (and near the one-GPU result)
        other = np.setdiff1d(np.arange(ng, n), case.dust)
        assert np.array_equal(vel[other], vel0[other])
        # the drag records are those of the old form, with and without the model: same bytes, and with only
        # epstein / no_friction_heating set both forms give the same bits
        for f, v in ((B.F_VEL, vel0), (B.F_ENTROPY, ent0)):
            T.S.set_field(f, v)
        eh = case.model("epstein", "no_friction_heating")
        T.set_model(eh)
        o10, c10 = T.run(B.DD_DUST_DRAG, False, d7=one_d["particle_density"], d9=case.d9)
        for f, v in ((B.F_VEL, vel0), (B.F_ENTROPY, ent0)):
            T.S.set_field(f, v)
        o17, c17 = T.run(B.DD_DUST_DRAG, True, d7=one_d["particle_density"], d9=case.d9)
        assert [int(c[3]) for c in c17] == [int(c[3]) for c in c10] == [int(c[3]) for c in c_drag]
        for k in o10:
            assert np.array_equal(o17[k], o10[k]), k
    finally:
        T.S.close()


# ---- 7. the mirror on bundle records ----------------------------------------------------------------
ALLM = np.dtype({"names": ["VirtualTime", "FragmentationVelocity", "InitialDustRadius", "UnitEnergy_in_cgs"],
                 "formats": ["f8"] * 4, "offsets": [16, 40, 8, 56], "itemsize": 64})
LOGR_OFFSET = P536D.fields["rest"][1] + 16     # P[].LogDustRadius_by_dt in the records' spare bytes


def _bind_model(host, H, case, m):
    A = np.zeros(1, ALLM)
    for k in ALLM.names:
        A[k] = m[k]
    lay = H.DustModelLayout()
    for k in MR.SWITCHES:
        setattr(lay, k, m[k])
    lay.a_virtual_time, lay.a_fragmentation_velocity = ALLM.fields["VirtualTime"][1], ALLM.fields["FragmentationVelocity"][1]
    lay.a_initial_dust_radius, lay.a_unit_energy = ALLM.fields["InitialDustRadius"][1], ALLM.fields["UnitEnergy_in_cgs"][1]
    lay.p_log_radius_by_dt = LOGR_OFFSET
    host.bind_dust_model(A, lay)
    host.All.Time = m["Time"]


def _logr(P):
    o = LOGR_OFFSET - P536D.fields["rest"][1]
    return np.ascontiguousarray(P["rest"][:, o:o + 8]).view(np.float64)[:, 0]


def _set_logr(P, idx, v):
    o = LOGR_OFFSET - P536D.fields["rest"][1]
    P["rest"][idx, o:o + 8] = np.ascontiguousarray(v, np.float64).view(np.uint8).reshape(-1, 8)


def test_dropin_writes_d9_radius_and_log_radius_on_bundle_records():
    B = bindings()
    H = importlib.import_module("gadget-leicester_amd.hostapi")
    case = DC.DustModelCase(1, ndust=300)          # (its own: density() below changes its Hsml and d1-d3)
    d = case.dust
    m = case.model(*DC.ALL_SIX, FragmentationVelocity=120.0)
    host, P, S, A = _host(case, H, B)
    try:
        L = host.L
        _bind_model(host, H, case, m)
        _set_logr(P, d, case.logr0)
        L.density()
        assert host.endrun_codes == [], L.gadget_force_last_error()
        case.hsml = P["Hsml"].copy()
        case.rho, case.ent = P["DUST_Density"][d].copy(), P["DUST_Entropy"][d].copy()
        case.gasvel = P["DUST_SurroundingGasVel"][d].copy()
        # the C-ABI on the same state
        _, fp = _device(case)
        try:
            fp.set_dust_model(case.gmodel(m))
            dn = fp.dust_density_grains(case.gparams(), d)
            out = fp.dust_drag_grains(case.gparams(), d, case.rho, case.ent, case.gasvel, case.radius,
                                      dn["particle_density"], dn["particle_velocity"], case.vcoll,
                                      log_radius_by_dt=case.logr0)
        finally:
            fp.close()
        keep = P.copy()
        L.dust_density()
        assert host.endrun_codes == [], L.gadget_force_last_error()
        assert relerr(P["DUST_particle_density"][d], dn["particle_density"]) < TOL
        assert _scaled_err(P["DUST_particle_velocity"][d], dn["particle_velocity"]) < TOL
        assert not np.array_equal(P["DUST_particle_velocity"][d], keep["DUST_particle_velocity"][d])
        L.dust_drag()
        assert host.endrun_codes == [], L.gadget_force_last_error()
        assert _scaled_err(P["DUST_particle_velocity"][d], out["particle_velocity"]) < TOL
        assert relerr(P["DustRadius"][d], out["dust_radius"]) < TOL
        assert relerr(_logr(P)[d], out["log_radius_by_dt"]) < TOL
        assert _scaled_err(P["DeltaDragEnergy"][d], out["delta_energy"]) < TOL
        assert not np.array_equal(P["DustRadius"][d], keep["DustRadius"][d])
        assert not np.array_equal(_logr(P)[d], case.logr0)
        other = np.setdiff1d(np.arange(case.pr.n), d)
        assert np.array_equal(P["DustRadius"][other], keep["DustRadius"][other])
        assert np.array_equal(P["rest"][other], keep["rest"][other])
    finally:
        host.close()


def test_dropin_refuses_the_model_on_more_than_one_rank():
    B = bindings()
    H = importlib.import_module("gadget-leicester_amd.hostapi")
    case = DC.DustModelCase(1, ndust=60, ng=6)
    host, P, S, A = _host(case, H, B, nranks=2)
    try:
        _bind_model(host, H, case, case.model(*DC.ALL_SIX, FragmentationVelocity=120.0, InitialDustRadius=1.e5))
        keep = P.copy()
        host.L.dust_density()
        host.L.dust_drag()
        assert host.endrun_codes == [90015, 90015]
        assert b"single rank" in host.L.gadget_force_last_error()
        assert np.array_equal(P, keep)
    finally:
        host.close()


# ---- 8. the argument rules, one set for the four entry forms ----------------------------------------
DRAG_ARRAYS = ("dust_density", "dust_entropy", "dust_gasvel", "dust_radius", "particle_density", "particle_velocity",
               "delta_momentum", "delta_energy", "vcoll")


def _call_form(B, f, form, drag, p, g):
    """one dust pass on context f with the arrays of the DustGrains g, through entry form `form` -> return code"""
    L, h = f.L, f.h
    if form == "positional" and drag:
        return L.ghip_dust_drag(h, C.byref(p), g.ndust, g.dust_idx, g.dust_density, g.dust_entropy, g.dust_gasvel,
                                g.dust_radius, g.particle_density, g.particle_velocity, g.delta_momentum,
                                g.delta_energy, g.vcoll)
    if form == "positional":
        return L.ghip_dust_density(h, C.byref(p), g.ndust, g.dust_idx, g.particle_density)
    if form == "grains":
        return (L.ghip_dust_drag_grains if drag else L.ghip_dust_density_grains)(h, C.byref(p), C.byref(g))
    if form == "dd":
        A = B.DdDustArgs()
        for k, _ in B.DdDustArgs._fields_[1:]:
            setattr(A, k, getattr(g, k))
    else:
        A = B.DdDustGrainsArgs()
        A.g = g
    A.p = C.pointer(p)
    return L.ghip_dd_begin(h, B.DD_DUST_DRAG if drag else B.DD_DUST_DENSITY, C.cast(C.byref(A), C.c_void_p),
                           B.DUST_GRAINS_FORM if form == "dd_grains" else 0)


def test_every_form_refuses_a_missing_array_alike():
    """Each member a pass requires set to NULL in turn, ndust > 0, in all four forms: GHIP_EINVAL "bad arguments",
    nothing launched.  Required: the list and d7; in the drag pass its nine arrays; in the density pass of the
    grains forms d9 under real_pebble_collisions.  A NULL log_radius_by_dt is accepted."""
    case = DC.case(1)
    B, fp = _device(case)
    T = DdModel(case, 2)
    try:
        p = case.gparams()
        d7, d9 = case.base()
        f0, o, local = T.S.fp[0], T.lists[0], T.local[0]
        assert len(local) > 0
        kw = lambda s: dict(particle_density=d7[s], dust_density=case.rho[s], dust_entropy=case.ent[s],
                            dust_gasvel=case.gasvel[s], dust_radius=case.radius[s], particle_velocity=d9[s],
                            vcoll=case.vcoll[s], log_radius_by_dt=case.logr0[s])
        one = B.dust_grains(case.dust, **kw(slice(None)))
        shard = B.dust_grains(local, **kw(o))
        full = case.model(*DC.ALL_SIX)
        fp.sync()
        fp.run_begin(1)
        for form in ("positional", "grains", "dd", "dd_grains"):
            f, (g, _) = (fp, one) if form in ("positional", "grains") else (f0, shard)
            grains = form in ("grains", "dd_grains")
            # (the forms without arrays for what the model writes refuse growth and real_pebble_collisions)
            f.set_dust_model(case.gmodel(full if grains else case.model("epstein")))
            for drag in (False, True):
                needs = ("dust_idx",) + DRAG_ARRAYS if drag else \
                    ("dust_idx", "particle_density") + (("particle_velocity",) if grains else ())
                for member in needs:
                    h = type(g).from_buffer_copy(g)
                    setattr(h, member, None)
                    rc = _call_form(B, f, form, drag, p, h)
                    msg = f.L.ghip_last_error(f.h).decode()
                    assert rc == -90002 and "bad arguments" in msg, (form, drag, member, rc, msg)
        assert fp.run_end()["launches"] == 0
        # log_radius_by_dt == NULL: both grains forms run, under growth too
        out = _drag(fp, case, full, d7, logr=False)
        assert "log_radius_by_dt" not in out and not np.array_equal(out["dust_radius"], case.radius)
        built = [B.dd_dust_grains_args(p, T.local[r], logr=False, **dict(kw(T.lists[r]), log_radius_by_dt=None))
                 for r in range(2)]
        T.set_model(full)
        T.S.run.run(B.DD_DUST_DRAG, [b[0] for b in built], B.DUST_GRAINS_FORM)
        assert not np.array_equal(built[0][1]["dust_radius"], case.radius[T.lists[0]])
    finally:
        T.S.close()
        fp.close()
