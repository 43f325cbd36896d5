"""cooling_and_starformation with DoCooling and the dust drag heating on the device (ghip_sfr_cooling,
ghip_find_smbh), against the numpy restatement of tests/sfr_ref.py: every cooling variant, comoving or
not, an active subset in permuted order; the resident chain dust_drag -> sfr_cooling; logical shards;
the size of config c5's gas with the time of the pass."""
import ctypes as C
import time

import numpy as np
import pytest

import sfr_ref as R
from common import ShardSet, SinkProblem, bindings
from test_gpu_dust import DustCase

pytestmark = pytest.mark.gpu
VARIANTS = [R.NONE, R.ISOTHERM, R.EVAPORATION, R.EVAPORATION_RADIAL, R.BETA]


def _gparams(d):
    B = bindings()
    p = B.SfrParams()
    for k, v in d.items():
        if k == "smbh_pos":
            for c in range(3):
                p.smbh_pos[c] = float(v[c])
        else:
            setattr(p, k, v)
    return p


def _check_dtentropy(got, ref, entropy, timebin, timebase):
    """the existing cooling/SF test's bound, 1e-13 A / dt, per particle with A the larger of the old and
    the new entropy: dA/dt is a difference of nearly equal numbers, and pow() differs in the last bit"""
    tb = np.asarray(timebin)[:len(ref)]
    dt = np.where(tb > 0, (1 << tb).astype(np.float64), 1.0) * timebase
    scale = (np.abs(entropy) + np.abs(ref) * dt) / dt
    err = np.abs(got - ref)
    assert np.all(err <= 1e-13 * scale), float((err / scale).max())


class SfrCase:
    """A SinkProblem (gas, Type-2 grains, Type-5 sinks) with densities around the sink threshold, black-hole
    injections (one through the 5e9 K ceiling), DragHeating, massless gas, light grains under the floor,
    a DtEntropy that hits the -A/(2 dt) floor and a few particles with dt == 0"""

    def __init__(self, seed=9, ng=10):
        sp = SinkProblem(ng=ng, periodic=1, nsink=6, ndust=200, seed=seed)
        pr = sp.pr
        self.sp, self.pr = sp, pr
        rng = np.random.default_rng(seed)
        n, ngas = pr.n, pr.ngas
        self.mass = pr.ic["mass"].copy()
        ogm = self.mass[0]
        light = sp.dust[::3]
        self.mass[light] = 1e-6 * ogm                       # under the grain floor 1e-5 OriginalGasMass
        self.mass[rng.choice(ngas, 8, replace=False)] = 0.0
        self.timebin = pr.timebin.copy()
        self.timebin[rng.choice(ngas, 6, replace=False)] = 0
        self.density = 0.2 + 3.0 * rng.random(ngas)
        self.dtentropy = pr.dtentropy.copy()
        self.dtentropy[11] = -1.0e6                         # the prediction goes negative: MinEgySpec, floor
        self.density[11], self.mass[11], self.timebin[11] = 1.0, self.mass[12] or self.mass[13], 2
        u = pr.entropy / R.GAMMA_MINUS1 * self.density ** R.GAMMA_MINUS1
        dt = (1 << pr.timebin[:ngas]).astype(np.float64) * pr.timebase
        self.injected = np.where(rng.random(ngas) < 0.3, self.mass[:ngas] * u * rng.random(ngas), 0.0)
        self.dragheat = np.where(rng.random(ngas) < 0.4, self.mass[:ngas] * u / dt * rng.random(ngas), 0.0)
        self.dragheat[np.where(self.mass[:ngas] == 0)[0][:4]] = 1.0   # kept: massless gas does not spend it
        box = pr.box
        self.par = R.params(dust=1, Timebase_interval=pr.timebase, CritPhysDensity_code=2.5,
                            OriginalGasMass=ogm, MinEgySpec=0.1 * float(np.median(u)),
                            smbh_pos=(0.45 * box, 0.52 * box, 0.49 * box))
        # units with the equilibrium a few times the mean energy and tcool of the order of a step
        p = self.par
        u2t = R.u_to_temp(p)
        p["EqTemp"] = 3.0 * float(np.median(u)) * u2t
        p["BetaCool"] = float(np.median(dt))
        p["UnitDensity_in_cgs"] = p["Evap_dens"] / 1.5
        ceil_i = np.where((self.mass[:ngas] > 0) & (self.density < 2.5))[0][0]
        self.injected[ceil_i] = 10.0 * self.mass[ceil_i] * 5.0e9 / u2t
        self.ceil_i = ceil_i

    def params(self, **over):
        return {**self.par, **over}

    def device(self):
        B = bindings()
        fp = self.pr.device()
        fp.set_field(B.F_MASS, self.mass)
        fp.set_field(B.F_TIMEBIN, self.timebin)
        fp.set_field(B.F_DENSITY, self.density)
        fp.set_field(B.F_DTENTROPY, self.dtentropy)
        fp.set_sink_marks(injected=self.injected)
        return B, fp

    def ref(self, p, act, dragheat=None):
        pr = self.pr
        return R.sfr_cooling(p, act, pr.ngas, pr.ic["type"], pr.ic["pos"], self.mass, self.timebin,
                             self.density, pr.entropy, self.dtentropy, self.injected,
                             self.dragheat if dragheat is None else dragheat)


@pytest.mark.parametrize("comoving", [0, 1])
@pytest.mark.parametrize("variant", VARIANTS)
def test_sfr_cooling_parity(variant, comoving):
    case = SfrCase()
    pr = case.pr
    n, ngas = pr.n, pr.ngas
    B, fp = case.device()
    fp.set_dust_drag_heating(case.dragheat)
    rng = np.random.default_rng(17)
    act = rng.permutation(n)[: (3 * n) // 4].astype(np.int32)          # an active subset, permuted
    fp.set_active(act)
    p = case.params(cooling=variant, beta_tapper_off=1 if variant == R.BETA else 0, comoving=comoving,
                    Time=0.62, hubble_a=1.7)
    before = {f: fp.get_field(f) for f in (B.F_POS, B.F_ENTROPY, B.F_DENSITY, B.F_TYPE, B.F_VEL)}
    cand = fp.sfr_cooling(_gparams(p))
    r = case.ref(p, act)
    assert 5 < len(r["cand"]) and np.array_equal(cand, r["cand"])
    _check_dtentropy(fp.get_field(B.F_DTENTROPY), r["dtentropy"], pr.entropy, case.timebin, pr.timebase)
    assert np.array_equal(fp.get_field(B.F_MASS), r["mass"]) and not np.array_equal(r["mass"], case.mass)
    assert np.array_equal(fp.dust_drag_heating(), r["dragheat"])
    _, inj = fp.sink_marks()
    assert np.array_equal(inj, r["injected"])
    # the inactive particles and the fields the pass only reads are untouched
    rest = np.setdiff1d(np.arange(ngas), act)
    assert len(rest) > 0 and np.array_equal(fp.get_field(B.F_DTENTROPY)[rest], case.dtentropy[rest])
    assert np.array_equal(r["dtentropy"][rest], case.dtentropy[rest])
    for f, v in before.items():
        assert np.array_equal(fp.get_field(f), v), f
    # the ceiling, the floor and the quirks did occur in the active subset
    acts = set(act.tolist())
    assert case.ceil_i in acts and 11 in acts
    kept = (case.dragheat != 0) & (r["dragheat"] != 0) & (case.mass[:ngas] == 0) & np.isin(np.arange(ngas), act)
    assert kept.any()
    assert fp.sfr_cooling(_gparams(p), count_only=True) == len(r["cand"])   # count only
    fp.close()


def test_identity_variant_equals_the_old_entry_point_bit_for_bit():
    case = SfrCase()
    pr = case.pr
    act = np.sort(np.random.default_rng(4).choice(pr.n, pr.n // 2, replace=False)).astype(np.int32)
    p = case.params(cooling=R.NONE, dust=0, smbh_pos=(0.0, 0.0, 0.0))
    u2t = R.u_to_temp(p)
    out = []
    for new in (0, 1):
        B, fp = case.device()
        fp.set_active(act)
        if new:
            cand = fp.sfr_cooling(_gparams(p))
        else:
            flag = fp.cooling_and_starformation(pr.timebase, p["CritPhysDensity_code"], p["MinEgySpec"], u2t)
            cand = np.array([i for i in act if i < pr.ngas and flag[i]], np.int32)
        out.append((cand, fp.get_field(B.F_DTENTROPY), fp.sink_marks()[1]))
        fp.close()
    assert len(out[0][0]) > 0
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


def test_resident_chain_dust_drag_then_sfr_cooling():
    """dust_density + dust_drag leave DragHeating and the gas entropy on the device; sfr_cooling spends
    them: the same state as the reference fed what dust_drag produced"""
    case = DustCase(1)
    pr = case.pr
    n, ngas = pr.n, pr.ngas
    B, fp = case.device()
    d7 = fp.dust_density(case.gparams(), case.dust)
    case.drag(fp, np.arange(len(case.dust)), d7)
    heat = fp.dust_drag_heating()
    entropy = fp.get_field(B.F_ENTROPY)
    assert np.count_nonzero(heat) > 10
    dens = 0.2 + 3.0 * np.random.default_rng(5).random(ngas)
    fp.set_field(B.F_DENSITY, dens)
    u = entropy / R.GAMMA_MINUS1 * dens ** R.GAMMA_MINUS1
    p = R.params(dust=1, Timebase_interval=pr.timebase, CritPhysDensity_code=2.8, OriginalGasMass=pr.ic["mass"][0],
                 MinEgySpec=0.1 * float(np.median(u)), smbh_pos=(0.5 * pr.box,) * 3, BetaCool=8 * pr.timebase)
    p["EqTemp"] = 2.0 * float(np.median(u)) * R.u_to_temp(p)
    p["UnitDensity_in_cgs"] = p["Evap_dens"]
    fp.set_active(None)
    cand = fp.sfr_cooling(_gparams(p))
    r = R.sfr_cooling(p, np.arange(n), ngas, pr.ic["type"], pr.ic["pos"], case.mass, case.timebin, dens,
                      entropy, pr.dtentropy, np.zeros(ngas), heat)
    assert len(r["cand"]) > 0 and np.array_equal(cand, r["cand"])
    _check_dtentropy(fp.get_field(B.F_DTENTROPY), r["dtentropy"], entropy, case.timebin, pr.timebase)
    assert np.array_equal(fp.dust_drag_heating(), r["dragheat"])
    assert np.array_equal(fp.get_field(B.F_MASS), r["mass"])
    spent = (heat != 0) & (r["dragheat"] == 0)
    assert spent.sum() > 10 and not np.array_equal(r["dtentropy"][spent], pr.dtentropy[spent])
    fp.close()


def test_dragheating_never_set_counts_as_zero():
    case = SfrCase()
    B, fp = case.device()
    fp.set_active(None)
    p = case.params(dust=1)
    cand = fp.sfr_cooling(_gparams(p))
    r = case.ref(p, np.arange(case.pr.n), dragheat=np.zeros(case.pr.ngas))
    assert np.array_equal(cand, r["cand"])
    _check_dtentropy(fp.get_field(B.F_DTENTROPY), r["dtentropy"], case.pr.entropy, case.timebin,
                     case.pr.timebase)
    fp.close()


def test_find_smbh_last_in_active_order():
    case = SfrCase()
    pr, sp = case.pr, case.sp
    B, fp = case.device()
    mass = fp.get_field(B.F_MASS)
    pos = pr.ic["pos"]
    big = sp.SMBHmass
    s = sp.sinks
    mass[s] = 0.5 * big                              # none qualifies
    for k, heavy in ((0, []), (1, [s[3]]), (2, [s[1], s[4]])):
        m = mass.copy()
        m[heavy] = 1.2 * big
        fp.set_field(B.F_MASS, m)
        for act in (None, np.random.default_rng(k).permutation(pr.n).astype(np.int32)):
            fp.set_active(act)
            got, cnt = fp.find_smbh(big)
            want, wcnt = R.find_smbh(np.arange(pr.n) if act is None else act, pr.ic["type"], m, pos, big)
            assert cnt == wcnt == k and np.array_equal(got, want)
        if k == 2:   # the last in ACTIVE order, not in index order
            fp.set_active(np.array([heavy[1], heavy[0]], np.int32))
            got, cnt = fp.find_smbh(big)
            assert cnt == 2 and np.array_equal(got, pos[heavy[0]])
    fp.close()


def test_sfr_cooling_on_logical_shards():
    case = SfrCase()
    pr = case.pr
    ngas = pr.ngas
    p = case.params(dust=0)
    B, fp = case.device()
    fp.set_active(None)
    cand1 = fp.sfr_cooling(_gparams(p))
    want = {f: fp.get_field(f) for f in (B.F_DTENTROPY, B.F_MASS)}
    _, inj1 = fp.sink_marks()
    fp.close()
    S = ShardSet(pr, 3)
    try:
        S.set_field(B.F_MASS, case.mass)
        S.set_field(B.F_TIMEBIN, case.timebin)
        S.set_field(B.F_DENSITY, case.density)
        S.set_field(B.F_DTENTROPY, case.dtentropy)
        for r, sfp in enumerate(S.fp):
            sfp.set_sink_marks(injected=case.injected[S.gid[r][:S.ngas[r]]])
        for r, sfp in enumerate(S.fp):
            cand = S.gid[r][sfp.sfr_cooling(_gparams(p))]
            mine = np.isin(cand1, S.gid[r])
            assert np.array_equal(cand, cand1[mine])
            with pytest.raises(B.GhipError) as e:
                sfp.sfr_cooling(_gparams(case.params(dust=1)))
            assert e.value.code == -90002 and "single-rank" in str(e.value)
        for f, v in want.items():
            assert np.array_equal(S.get_field(f), v), f
        inj = np.zeros(ngas)
        for r, sfp in enumerate(S.fp):
            inj[S.gid[r][:S.ngas[r]]] = sfp.sink_marks()[1]
        assert np.array_equal(inj, inj1)
    finally:
        S.close()
    # the replicated multi-GPU mode refuses dust = 1 too
    B, fp = case.device()
    fp.set_shard(0, 2)
    with pytest.raises(B.GhipError) as e:
        fp.sfr_cooling(_gparams(case.params(dust=1)))
    assert e.value.code == -90002
    fp.close()


def test_refusals():
    case = SfrCase(ng=6)
    B, fp = case.device()
    nc = C.c_int(0)
    assert fp.L.ghip_sfr_cooling(fp.h, None, C.byref(nc), None) == -90002
    for bad in (-1, 5):
        with pytest.raises(B.GhipError) as e:
            fp.sfr_cooling(_gparams(case.params(cooling=bad)))
        assert e.value.code == -90002 and "unknown cooling" in str(e.value)
    fp.close()


def test_sfr_cooling_at_c5_gas_count_with_timing():
    """256^3 gas (config c5's 16.8 M) plus 2^16 grains and a few sinks, all active: the candidate list and
    a seeded sample of 4096 gas particles and all grains against the reference; the time of the call"""
    B = bindings()
    ngas, nother = 256 ** 3, 1 << 16
    n = ngas + nother
    rng = np.random.default_rng(23)
    ptype = np.zeros(n, np.int32)
    ptype[ngas:] = 2
    ptype[ngas + rng.choice(nother, 8, replace=False)] = 5
    pos = rng.random((n, 3))
    mass = np.full(n, 1.0 / ngas)
    mass[ngas + rng.choice(nother, nother // 4, replace=False)] = 1e-7 / ngas
    mass[rng.choice(ngas, 1000, replace=False)] = 0.0
    timebin = rng.integers(1, 6, n).astype(np.int32)
    dens = 0.2 + 3.0 * rng.random(ngas)
    ent = 0.05 * (1 + 0.2 * rng.random(ngas))
    dte = 1e-3 * rng.standard_normal(ngas)
    timebase = 1e-4
    u = ent / R.GAMMA_MINUS1 * dens ** R.GAMMA_MINUS1
    inj = np.where(rng.random(ngas) < 0.05, mass[:ngas] * u * rng.random(ngas), 0.0)
    heat = np.where(rng.random(ngas) < 0.3, mass[:ngas] * u / timebase * 1e-2 * rng.random(ngas), 0.0)
    p = R.params(Timebase_interval=timebase, CritPhysDensity_code=3.19, OriginalGasMass=1.0 / ngas,
                 MinEgySpec=0.01, BetaCool=4 * timebase, smbh_pos=(0.5, 0.5, 0.5))
    p["EqTemp"] = 2.0 * float(np.median(u)) * R.u_to_temp(p)
    p["UnitDensity_in_cgs"] = p["Evap_dens"]
    gp = _gparams(p)
    fp = B.ForcePath(0)
    fp.set_counts(n, ngas)
    for f, v in ((B.F_POS, pos), (B.F_MASS, mass), (B.F_TYPE, ptype), (B.F_TIMEBIN, timebin),
                 (B.F_DENSITY, dens), (B.F_ENTROPY, ent)):
        fp.set_field(f, v)

    def reset():
        fp.set_field(B.F_MASS, mass)
        fp.set_field(B.F_DTENTROPY, dte)
        fp.set_sink_marks(injected=inj)
        fp.set_dust_drag_heating(heat)

    reset()
    cand = fp.sfr_cooling(gp)
    gas_s = np.sort(rng.choice(ngas, 4096, replace=False))
    sample = np.concatenate([gas_s, np.arange(ngas, n)])
    r = R.sfr_cooling(p, sample, ngas, ptype, pos, mass, timebin, dens, ent, dte, inj, heat)
    assert np.array_equal(cand[np.isin(cand, sample)], r["cand"]) and len(r["cand"]) > 10
    assert np.all(dens[cand] >= 3.19) and np.all(mass[cand] != 0)
    assert len(cand) == int(((dens >= 3.19) & (mass[:ngas] != 0)).sum())
    _check_dtentropy(fp.get_field(B.F_DTENTROPY)[gas_s], r["dtentropy"][gas_s], ent[gas_s], timebin[gas_s],
                     timebase)
    assert np.array_equal(fp.get_field(B.F_MASS)[sample], r["mass"][sample])
    assert np.array_equal(fp.dust_drag_heating()[gas_s], r["dragheat"][gas_s])
    assert np.array_equal(fp.sink_marks()[1][gas_s], r["injected"][gas_s])
    times = []
    for _ in range(5):
        reset()
        t0 = time.perf_counter()
        fp.sfr_cooling(gp)
        times.append(time.perf_counter() - t0)
    print("\n  c5-size sfr_cooling: %d gas + %d others, %d candidates: call %.3f ms (min of 5; median %.3f ms)"
          % (ngas, nother, len(cand), 1e3 * min(times), 1e3 * float(np.median(times))))
    fp.close()
