"""The viscosity mode of the SPH path on the device (ghip_set_viscosity): -DTIME_DEP_ART_VISC with the
uniform switches of hydra.c:1512-1595, against the all-pairs numpy reference tests/visc_ref.py (itself
pinned to the oracle by tests/test_visc_cpu.py) fed with the device's own density results: the pair
kernel, the Dtalpha post-pass, the alpha update of the kick, the refusals, shards (ghosts, migration) and
the reference-named mirror on bound records."""
import ctypes as C
import importlib

import numpy as np
import pytest

import kick_ref as KR
import visc_ref as VR
from common import Problem, ShardSet, bindings

pytestmark = pytest.mark.gpu

TOL = 1e-11                          # of the field's largest magnitude: the bound of tests/test_gpu_parity.py
COMOVING = (1, 0.37, 0.81, 1.9)      # the tuple of test_density_and_hydro_parity


def _all(n):
    return np.arange(n, dtype=np.int32)


def visc_struct(V):
    B = bindings()
    P = B.ViscParams()
    for k, v in V.items():
        setattr(P, k, v)
    return P


def alpha_of(ng, seed=7):
    return 0.1 + 0.7 * np.random.default_rng(seed).random(ng)


def dens_state(get_field, B, ng):
    return {k: np.asarray(get_field(f), np.float64)[:ng].copy() for k, f in (
        ("hsml", B.F_HSML), ("density", B.F_DENSITY), ("pressure", B.F_PRESSURE), ("dhsmlfac", B.F_DHSMLFAC),
        ("divvel", B.F_DIVVEL), ("curlvel", B.F_CURLVEL))}


def after_density(pr, dynamic_tree=False):
    B = bindings()
    fp = pr.device()
    if dynamic_tree:
        fp.set_dynamic_tree(True)
    pr.device_tree(fp)
    fp.density(pr.g_dens())
    fp.update_hmax()
    return fp, dens_state(fp.get_field, B, pr.ngas)


def check_hydro(get_field, pairs, ref, act=None, tol=TOL):
    B = bindings()
    sel = slice(None) if act is None else act
    assert pairs == ref["npairs"]
    for fid, k in ((B.F_HYDROACCEL, "hydroaccel"), (B.F_DTENTROPY, "dtentropy"), (B.F_MAXSIGNALVEL, "maxsignalvel")):
        err = np.abs(get_field(fid)[sel] - ref[k][sel]).max() / np.abs(ref[k][sel]).max()
        print(k, err)
        assert err < tol, k


# ---- 1. varying alpha ----------------------------------------------------------------------------
@pytest.mark.parametrize("ng,periodic,comoving", [(12, 1, None), (8, 0, None), (8, 1, COMOVING)])
def test_varying_alpha_against_the_all_pairs_reference(ng, periodic, comoving):
    B = bindings()
    pr = Problem(ng=ng, gas=True, periodic=periodic)
    fp, ds = after_density(pr)
    V = VR.params(time_dependent=1, ArtBulkViscConst=0.8, dtalpha_comoving_div=1.9 * 0.37 * 0.37)
    alpha = alpha_of(pr.ngas)
    hp = pr.g_hydro(*comoving) if comoving else pr.g_hydro()
    fp.set_viscosity(visc_struct(V))
    fp.visc_set_alpha(alpha)
    fp.hydro(hp)
    ref = VR.hydro(pr, ds, alpha, V, hp)
    check_hydro(fp.get_field, fp.stats()["hydro_pairs"], ref)
    # Dtalpha of the post-pass from the device's own fields: a closed form of about ten operations
    got_a, got_d = fp.visc_get()
    assert np.array_equal(got_a, alpha)
    want = VR.dtalpha(ds["pressure"], ds["density"], ds["hsml"], ds["divvel"], ds["curlvel"],
                      fp.get_field(B.F_MAXSIGNALVEL), alpha, V, fac_mu=hp.fac_mu, comoving=hp.ComovingIntegrationOn)
    assert np.abs(got_d - want).max() < 1e-13 * np.abs(want).max()
    assert (want > 0).any() and (want < 0).any()           # sources and decay both occur
    # the mode off again: the default kernels' result (what the parity tests pin to the oracle)
    fp.set_viscosity(None)
    fp.hydro(hp)
    off = VR.hydro(pr, ds, alpha, VR.params(), hp)
    check_hydro(fp.get_field, fp.stats()["hydro_pairs"], off)
    fp.close()


# ---- 2. the uniform switches ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def limited():
    """Problem(ng=8) at timebase = 1 (the limiter binds) after the device's density"""
    pr = Problem(ng=8, gas=True, periodic=1)
    pr.timebase = 1.0
    fp, ds = after_density(pr)
    yield pr, fp, ds
    fp.close()


ONE_BY_ONE = [("conventional",), ("no_limiter",), ("no_shear_limiter",),
              ("conventional", "no_limiter", "no_shear_limiter")]


@pytest.mark.parametrize("time_dependent,switches", [(0, sw) for sw in ONE_BY_ONE] +
                         [(1, sw) for sw in ONE_BY_ONE + [()]])
def test_uniform_switches(limited, time_dependent, switches):
    pr, fp, ds = limited
    V = VR.params(time_dependent=time_dependent, ArtBulkViscConst=pr.visc, **{k: 1 for k in switches})
    alpha = alpha_of(pr.ngas)
    base = VR.hydro(pr, ds, alpha, VR.params(ArtBulkViscConst=pr.visc), pr.g_hydro())
    assert 4 * base["nlimited"] >= base["napproach"] > 0      # the limiter binds in this problem
    fp.set_viscosity(visc_struct(V))
    fp.visc_set_alpha(alpha)
    fp.hydro(pr.g_hydro())
    ref = VR.hydro(pr, ds, alpha, V, pr.g_hydro())
    check_hydro(fp.get_field, fp.stats()["hydro_pairs"], ref)
    # (and the case is not the constant one in disguise)
    assert np.abs(ref["hydroaccel"] - base["hydroaccel"]).max() > 1e-6 * np.abs(base["hydroaccel"]).max()
    fp.set_viscosity(None)


# ---- 3. alpha = ArtBulkViscConst is the constant case ------------------------------------------------
def test_constant_alpha_equals_the_mode_off(limited):
    B = bindings()
    pr, fp, ds = limited
    fp.set_viscosity(None)
    fp.hydro(pr.g_hydro())
    off = [fp.get_field(f).copy() for f in (B.F_HYDROACCEL, B.F_DTENTROPY, B.F_MAXSIGNALVEL)]
    pairs = fp.stats()["hydro_pairs"]
    fp.set_viscosity(visc_struct(VR.params(time_dependent=1, ArtBulkViscConst=pr.visc)))
    fp.visc_set_alpha(np.full(pr.ngas, pr.visc))
    fp.hydro(pr.g_hydro())
    assert fp.stats()["hydro_pairs"] == pairs
    for a, f in zip(off, (B.F_HYDROACCEL, B.F_DTENTROPY, B.F_MAXSIGNALVEL)):
        got = fp.get_field(f)
        print(f, "bitwise" if np.array_equal(got, a) else np.abs(got - a).max() / np.abs(a).max())
        assert np.abs(got - a).max() < TOL * np.abs(a).max()
    fp.set_viscosity(None)


# ---- 4. Dtalpha on an active subset -------------------------------------------------------------
@pytest.mark.parametrize("comoving", [None, COMOVING])
def test_dtalpha_of_an_active_subset_with_inactive_neighbours_alpha(comoving):
    B = bindings()
    pr = Problem(ng=10, gas=True, periodic=1)
    ng = pr.ngas
    fp, _ = after_density(pr)
    rng = np.random.default_rng(2)
    act = np.sort(rng.choice(ng, 150, replace=False)).astype(np.int32)
    alpha, old = alpha_of(ng), rng.standard_normal(ng)
    V = VR.params(time_dependent=1, ArtBulkViscConst=0.8, AlphaMin=0.05, ViscSource=0.7, DecayTime=1.3,
                  dtalpha_comoving_div=1.9 * 0.37 * 0.37)
    hp = pr.g_hydro(*comoving) if comoving else pr.g_hydro()
    fp.set_viscosity(visc_struct(V))
    fp.visc_set_alpha(alpha, old)
    fp.set_active(act)
    fp.density(pr.g_dens())
    fp.update_hmax()
    fp.hydro(hp)
    ds = dens_state(fp.get_field, B, ng)
    ref = VR.hydro(pr, ds, alpha, V, hp, act=act)            # (every neighbour with its own stored alpha)
    check_hydro(fp.get_field, fp.stats()["hydro_pairs"], ref, act=act)
    _, got = fp.visc_get()
    want = VR.dtalpha(ds["pressure"], ds["density"], ds["hsml"], ds["divvel"], ds["curlvel"],
                      fp.get_field(B.F_MAXSIGNALVEL), alpha, V, fac_mu=hp.fac_mu, comoving=hp.ComovingIntegrationOn)
    assert np.abs(got[act] - want[act]).max() < 1e-13 * np.abs(want[act]).max()
    rest = np.setdiff1d(_all(ng), act)
    assert np.array_equal(got[rest].view(np.uint64), old[rest].view(np.uint64))
    if comoving:
        plain = VR.dtalpha(ds["pressure"], ds["density"], ds["hsml"], ds["divvel"], ds["curlvel"],
                           fp.get_field(B.F_MAXSIGNALVEL), alpha, V, fac_mu=hp.fac_mu)
        assert np.abs(got[act] - plain[act]).max() > 0.1 * np.abs(plain[act]).max()    # the division is seen
    fp.close()


# ---- 5. freshness ---------------------------------------------------------------------------------
def test_a_kept_tree_uses_the_alpha_of_the_call():
    pr = Problem(ng=8, gas=True, periodic=1)
    fp, ds = after_density(pr, dynamic_tree=True)
    V = VR.params(time_dependent=1, ArtBulkViscConst=0.8)
    fp.set_viscosity(visc_struct(V))
    fp.visc_set_alpha(alpha_of(pr.ngas, 7))
    fp.hydro(pr.g_hydro())
    new = alpha_of(pr.ngas, 8)
    fp.visc_set_alpha(new)                                   # no tree build in between
    fp.hydro(pr.g_hydro())
    check_hydro(fp.get_field, fp.stats()["hydro_pairs"], VR.hydro(pr, ds, new, V, pr.g_hydro()))
    fp.close()


# ---- 6. the kick ----------------------------------------------------------------------------------
KICK = dict(Timebase_interval=1e-3, ComovingIntegrationOn=0, Time=1.0, hubble_a=1.0, ErrTolIntAccuracy=0.5,
            CourantFac=0.15, MaxSizeTimestep=0.2, MinSizeTimestep=1e-9, dt_displacement=0.2, MinEgySpec=0.0,
            TimeBinActive=(1 << 29) - 1, logTimeBegin=0.0, logTimeMax=0.0, AdaptiveGravsoftForGasHsml=0, pmgrid=0,
            dt_gravkickB=0.0)


def kick_struct(p):
    B = bindings()
    K = B.KickParams()
    for k, v in p.items():
        if k == "SofteningTable":
            for t in range(6):
                K.SofteningTable[t] = v[t]
        else:
            setattr(K, k, v)
    return K


def dt_entr_of(binold, binnew, timebase):
    """timestep.c:378-395, not comoving: (tend - tstart) Timebase_interval of each particle's kick"""
    old = np.where(binold > 0, np.left_shift(1, binold), 0)
    new = np.where(binnew > 0, np.left_shift(1, binnew), 0)
    return ((old + new // 2) - old // 2) * timebase


def test_kick_updates_alpha_of_the_active_gas_only():
    B = bindings()
    pr = Problem(ng=8, gas=True, periodic=1)
    n, ng = pr.n, pr.ngas
    fp, ds = after_density(pr)
    V = VR.params(time_dependent=1, ArtBulkViscConst=0.8, AlphaMin=0.3, ViscSource=2.0, DecayTime=3.0)
    alpha = alpha_of(ng)
    fp.set_viscosity(visc_struct(V))
    fp.visc_set_alpha(alpha)
    fp.hydro(pr.g_hydro())
    _, rate = fp.visc_get()
    rate = rate * 40.0                                       # (steep enough for both clamps)
    rng = np.random.default_rng(11)
    grav = 0.3 * rng.standard_normal((n, 3))
    fp.set_field(B.F_GRAVACCEL, grav)
    typ = pr.ic["type"].copy()
    conv = rng.choice(ng, 5, replace=False)
    typ[conv] = 4                                            # converted records of the gas block
    fp.set_field(B.F_TYPE, typ)
    act = rng.permutation(n)[: n // 2].astype(np.int32)      # gas and others, not in index order
    p = dict(KICK, Ti_Current=pr.ti_current, SofteningTable=list(pr.force_soft / 2.8))
    keep = {f: fp.get_field(f).copy() for f in (B.F_VEL, B.F_VELPRED, B.F_ENTROPY, B.F_DTENTROPY, B.F_TIMEBIN,
                                                B.F_TI_BEGSTEP)}
    s = KR.state(type=typ, mass=pr.ic["mass"], vel=keep[B.F_VEL], grav=grav, hyd=fp.get_field(B.F_HYDROACCEL),
                 velpred=keep[B.F_VELPRED], entropy=keep[B.F_ENTROPY], dtentropy=keep[B.F_DTENTROPY],
                 density=ds["density"], hsml=fp.get_field(B.F_HSML), vsig=fp.get_field(B.F_MAXSIGNALVEL),
                 timebin=keep[B.F_TIMEBIN], ti_begstep=keep[B.F_TI_BEGSTEP])
    out = KR.advance_timesteps(p, KR.flags(), s, active=act)
    assert out["rc"] == 0
    results = {}
    for mode in ("on", "off"):
        for f, a in keep.items():
            fp.set_field(f, a)
        fp.set_viscosity(visc_struct(V) if mode == "on" else None)
        fp.visc_set_alpha(alpha, rate)
        fp.set_active(act)
        fp.advance_timesteps(kick_struct(p))
        results[mode] = {f: fp.get_field(f).copy() for f in keep}
        results[mode]["alpha"], results[mode]["rate"] = fp.visc_get()
    assert np.array_equal(results["on"][B.F_TIMEBIN], s["timebin"])
    for f in keep:
        assert np.array_equal(results["on"][f], results["off"][f]), f
    assert np.array_equal(results["off"]["alpha"], alpha)                   # mode off: alpha stays
    kicked = np.zeros(ng, bool)
    gas_act = act[act < ng]
    kicked[gas_act[typ[gas_act] == 0]] = True
    assert kicked.sum() > 100 and (~kicked).sum() > 100 and not kicked[conv].any()
    dt_entr = dt_entr_of(out["binold"][:ng], s["timebin"][:ng], p["Timebase_interval"])
    want = np.where(kicked, VR.kick_alpha(alpha, rate, dt_entr, V), alpha)
    got = results["on"]["alpha"]
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert (got[kicked] == 0.8).any() and (got[kicked] == 0.3).any()        # both clamps
    assert ((got[kicked] > 0.3) & (got[kicked] < 0.8)).any()
    assert np.array_equal(results["on"]["rate"], rate)                      # the kick leaves Dtalpha
    fp.close()


# ---- 7. refusals ----------------------------------------------------------------------------------
def test_refusals_carry_a_message_and_leave_the_context_usable():
    B = bindings()
    pr = Problem(ng=8, gas=True, periodic=1)
    fp, ds = after_density(pr)
    ng = pr.ngas

    def refused(fn, *words):
        with pytest.raises(B.GhipError) as e:
            fn()
        assert e.value.code == -90002, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    for k in ("ArtBulkViscConst", "AlphaMin", "ViscSource", "DecayTime", "dtalpha_comoving_div"):
        for bad in (float("nan"), float("inf")):
            refused(lambda: fp.set_viscosity(visc_struct(VR.params(time_dependent=1, **{k: bad}))), k, "finite")
    refused(lambda: fp.set_viscosity(visc_struct(VR.params(time_dependent=1, AlphaMin=-0.1))), "AlphaMin", "< 0")
    refused(lambda: fp.set_viscosity(visc_struct(VR.params(time_dependent=1, AlphaMin=0.9, ArtBulkViscConst=0.8))),
            "AlphaMin", "ArtBulkViscConst")
    refused(lambda: fp.visc_get(), "no alpha")
    V = VR.params(time_dependent=1, ArtBulkViscConst=0.8)
    fp.set_viscosity(visc_struct(V))
    before = [fp.get_field(f).copy() for f in (B.F_HYDROACCEL, B.F_VEL)]
    refused(lambda: fp.hydro(pr.g_hydro()), "ghip_hydro", "no alpha")
    p = dict(KICK, Ti_Current=pr.ti_current, SofteningTable=list(pr.force_soft / 2.8))
    refused(lambda: fp.advance_timesteps(kick_struct(p)), "ghip_advance_timesteps", "no alpha")
    for a, f in zip(before, (B.F_HYDROACCEL, B.F_VEL)):
        assert np.array_equal(fp.get_field(f), a)            # nothing ran
    bad = alpha_of(ng)
    bad[17] = float("nan")
    refused(lambda: fp.visc_set_alpha(bad), "17", "finite")
    # shards: the domain-decomposed context asks the same, the replicated one refuses the mode
    dd = pr.device()
    dd.dd_init(0, 1)
    dd.dd_set_domain(pr.extent[0], pr.extent[1], pr.extent[2], pr.force_soft)
    dd.set_viscosity(visc_struct(V))
    refused(lambda: dd.dd_begin(B.DD_HYDRO, pr.g_hydro()), "GHIP_DD_HYDRO", "no alpha")
    dd.close()
    rep = pr.device()
    rep.set_shard(0, 2)
    refused(lambda: rep.set_viscosity(visc_struct(V)), "ghip_set_shard")
    rep.close()
    # ... and the first context still computes
    alpha = alpha_of(ng, 9)
    fp.visc_set_alpha(alpha)
    fp.hydro(pr.g_hydro())
    check_hydro(fp.get_field, fp.stats()["hydro_pairs"], VR.hydro(pr, ds, alpha, V, pr.g_hydro()))
    fp.close()


# ---- 8. shards ------------------------------------------------------------------------------------
def test_shards_carry_alpha_in_the_ghost_records_and_through_a_migration():
    B = bindings()
    sh = importlib.import_module("gadget-leicester_amd.sharded")
    pr = Problem(ng=12, gas=True, periodic=1)
    ng = pr.ngas
    V = VR.params(time_dependent=1, ArtBulkViscConst=0.8, AlphaMin=0.05, ViscSource=0.7, DecayTime=1.3)
    alpha = alpha_of(ng)
    one, _ = after_density(pr)
    one.set_viscosity(visc_struct(V))
    one.visc_set_alpha(alpha)
    one.hydro(pr.g_hydro())
    want = {f: one.get_field(f).copy() for f in (B.F_HYDROACCEL, B.F_DTENTROPY, B.F_MAXSIGNALVEL)}
    want_pairs = one.stats()["hydro_pairs"]
    _, want_rate = one.visc_get()
    one.close()
    S = ShardSet(pr, 3)
    try:
        gas = lambda r: S.gid[r][:S.ngas[r]]
        bytes_sent = {}
        for mode in ("off", "on"):
            S.set_field(B.F_HSML, pr.hsml0)
            S.set_field(B.F_OLDACC, np.zeros(pr.n))
            S.set_field(B.F_DTENTROPY, pr.dtentropy)         # (hydro wrote it; the density reads it)
            if mode == "on":
                S.run.set_viscosity(visc_struct(V))
                S.run.visc_set_alpha([alpha[gas(r)] for r in range(3)])
            S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
            S.run.density(pr.g_dens())
            S.each(lambda fp: fp.update_hmax())
            S.run.hydro(pr.g_hydro())
            bytes_sent[mode] = [(fp.dd_bytes_sent(B.DD_DENSITY), fp.dd_bytes_sent(B.DD_HYDRO)) for fp in S.fp]
        assert bytes_sent["on"] == bytes_sent["off"] and sum(b[0] for b in bytes_sent["on"]) > 0
        assert sum(s["hydro_pairs"] for s in S.each(lambda fp: fp.stats())) == want_pairs
        for f, w in want.items():
            assert np.abs(S.get_field(f) - w).max() < TOL * np.abs(w).max(), f
        rate = np.zeros(ng)
        for r, (a, d) in enumerate(S.run.visc_get()):
            assert np.array_equal(a, alpha[gas(r)])
            rate[gas(r)] = d
        assert np.abs(rate - want_rate).max() < TOL * np.abs(want_rate).max()
        # alpha given again after the density: the ghosts carry the old epoch, the hydro call is refused
        S.run.visc_set_alpha([alpha[gas(r)] for r in range(3)], [rate[gas(r)] for r in range(3)])
        with pytest.raises(B.GhipError) as e:
            S.run.hydro(pr.g_hydro())
        assert e.value.code == -90002 and "GHIP_DD_DENSITY" in str(e.value)
        # new splits, GHIP_DD_MIGRATE: alpha and Dtalpha are found with their particles
        work = np.ones(pr.n)
        work[np.argsort(S.keys)[: pr.n // 2]] = 4.0          # the first half of the curve is four times as dear
        splits, owner = sh.decompose(S.keys, 3, work)
        assert (owner != S.owner).sum() > pr.n // 20
        S.splits = splits
        S.each(lambda fp: fp.dd_set_splits(splits))
        S.migrate()
        assert np.array_equal(S.owner, owner)
        moved_gas = 0
        for r, fp in enumerate(S.fp):
            a, d = fp.visc_get()
            assert len(a) == S.ngas[r]
            assert np.array_equal(a.view(np.uint64), alpha[gas(r)].view(np.uint64))
            assert np.array_equal(d.view(np.uint64), rate[gas(r)].view(np.uint64))
            moved_gas += sum(i["migrated_in"] for i in [fp.dd_info()])
        assert moved_gas > 0
    finally:
        S.close()


# ---- 9. the mirror --------------------------------------------------------------------------------
def _mirror(pr, H, overlap, nranks=1):
    B = bindings()
    host = H.Host(periodic=1, overlap_sph=overlap, nranks=nranks)
    sd = H.SPH_DTYPE
    SD = np.dtype({"names": list(sd.names) + ["alpha", "Dtalpha"],
                   "formats": [sd.fields[k][0] for k in sd.names] + ["f8", "f8"],
                   "offsets": [sd.fields[k][1] for k in sd.names] + [sd.itemsize, sd.itemsize + 8],
                   "itemsize": sd.itemsize + 16})
    AD = np.dtype({"names": ["AlphaMin", "ViscSource", "DecayTime"], "formats": ["f8"] * 3,
                   "offsets": [8, 24, 32], "itemsize": 48})
    P = np.zeros(pr.n, H.P_DTYPE)
    S = np.zeros(pr.ngas, SD)
    P["Pos"], P["Vel"], P["Mass"], P["Type"] = pr.ic["pos"], pr.ic["vel"], pr.ic["mass"], pr.ic["type"]
    P["ID"] = pr.ic["id"]
    P["TimeBin"], P["Ti_begstep"] = pr.timebin, pr.ti_begstep
    S["VelPred"], S["Entropy"], S["DtEntropy"] = pr.velpred, pr.entropy, pr.dtentropy
    S["Hsml"] = pr.hsml0[:pr.ngas]
    lay = B.Layout()
    host.L.gadget_force_layout(C.byref(lay))
    lay.s_stride = SD.itemsize
    host.bind_records(P, S, lay)
    A = host.All
    A.G, A.ErrTolTheta, A.ErrTolForceAcc, A.TypeOfOpeningCriterion = pr.G, pr.theta, pr.ErrTolForceAcc, 1
    A.BoxSize, A.DesNumNgb, A.MaxNumNgbDeviation = pr.box, pr.des_ngb, pr.max_dev
    A.ArtBulkViscConst, A.Ti_Current, A.Timebase_interval = 0.8, pr.ti_current, pr.timebase
    A.ComovingIntegrationOn, A.MinGasHsmlFractional, A.Time = 0, 0.0, 1.0
    A.ErrTolIntAccuracy, A.CourantFac = KICK["ErrTolIntAccuracy"], KICK["CourantFac"]
    A.MaxSizeTimestep, A.MinSizeTimestep = KICK["MaxSizeTimestep"], KICK["MinSizeTimestep"]
    A.MinEgySpec, A.TypeOfTimestepCriterion = 0.0, 0
    eps = pr.force_soft[0] / 2.8
    for name in ("Gas", "Halo", "Disk", "Bulge", "Stars", "Bndry"):
        setattr(A, "Softening" + name, eps)
        setattr(A, "Softening" + name + "MaxPhys", 1e30)
    host.L.set_softenings()
    tba = (C.c_int * 29).in_dll(host.L, "TimeBinActive")
    for b in range(29):
        tba[b] = 1
    C.c_int.in_dll(host.L, "Flag_FullStep").value = 1
    host.set_active(None)
    host.domain()
    HA = np.zeros(1, AD)
    HA["AlphaMin"], HA["ViscSource"], HA["DecayTime"] = 0.3, 2.0, 3.0
    vl = H.ViscLayout(a_alpha_min=AD.fields["AlphaMin"][1], a_visc_source=AD.fields["ViscSource"][1],
                      a_decay_time=AD.fields["DecayTime"][1], s_alpha=SD.fields["alpha"][1],
                      s_dtalpha=SD.fields["Dtalpha"][1], time_dependent=1, conventional=0, no_limiter=0,
                      no_shear_limiter=0)
    host.bind_viscosity(HA, vl)
    return host, P, S


def test_mirror_gathers_alpha_and_scatters_dtalpha_and_alpha():
    B = bindings()
    H = importlib.import_module("gadget-leicester_amd.hostapi")
    pr = Problem(ng=8, gas=True, periodic=1)
    ng = pr.ngas
    alpha = alpha_of(ng)
    V = VR.params(time_dependent=1, ArtBulkViscConst=0.8, AlphaMin=0.3, ViscSource=2.0, DecayTime=3.0)
    # the C-ABI path
    fp, ds = after_density(pr)
    fp.set_viscosity(visc_struct(V))
    fp.visc_set_alpha(alpha)
    fp.hydro(pr.g_hydro())
    want_acc = fp.get_field(B.F_HYDROACCEL).copy()
    _, want_rate = fp.visc_get()
    fp.close()
    res = []
    for overlap in (0, 1):
        host, P, S = _mirror(pr, H, overlap)
        try:
            S["alpha"] = alpha
            S["Dtalpha"] = 123.0
            L = host.L
            L.gravity_tree()
            L.density()
            L.force_update_hmax()
            L.hydro_force()
            assert host.endrun_codes == [], L.gadget_force_last_error()
            assert np.array_equal(S["alpha"], alpha)
            assert np.abs(S["HydroAccel"] - want_acc).max() < TOL * np.abs(want_acc).max()
            assert np.abs(S["Dtalpha"] - want_rate).max() < TOL * np.abs(want_rate).max()
            S["Dtalpha"] *= 40.0                            # (steep enough for the clamps)
            rate = S["Dtalpha"].copy()
            binold, tb0 = P["TimeBin"].astype(np.int32), P["Ti_begstep"].copy()
            L.advance_and_find_timesteps()
            assert host.endrun_codes == [], L.gadget_force_last_error()
            assert np.array_equal(P["Ti_begstep"][:ng], tb0[:ng] + np.left_shift(1, binold[:ng]))
            dt_entr = dt_entr_of(binold[:ng], P["TimeBin"][:ng].astype(np.int32), pr.timebase)
            got = S["alpha"].copy()
            assert np.array_equal(got.view(np.uint64), VR.kick_alpha(alpha, rate, dt_entr, V).view(np.uint64))
            assert (got == 0.8).any() and (got == 0.3).any() and ((got > 0.3) & (got < 0.8)).any()
            assert np.array_equal(S["Dtalpha"], rate)
            res.append((got, rate))
        finally:
            host.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def test_mirror_refuses_more_than_one_rank():
    H = importlib.import_module("gadget-leicester_amd.hostapi")
    pr = Problem(ng=8, gas=True, periodic=1)
    host, P, S = _mirror(pr, H, 0, nranks=2)
    try:
        S["alpha"] = 0.5
        keep = S.copy()
        host.L.hydro_force()
        assert host.endrun_codes == [90014]
        assert b"GHIP_DD_HYDRO" in host.L.gadget_force_last_error()
        host.L.advance_and_find_timesteps()
        assert host.endrun_codes == [90014, 90014]
        assert np.array_equal(S, keep)
    finally:
        host.close()
