"""The drop-in boundary beyond the minimal flag set (VERDICT r2 "close the boundary"):
accel.c's four-call sequence through the reference-named symbols of libgadget_force.so
  * on the shipped bundle's records -- 536-byte struct particle_data with Hsml / NumNgb in P (the PPP
    macro) and the BLACK_HOLES / DUST unions, 264-byte struct sph_particle_data -- bound by byte
    offsets (gadget_force_bind_records), with Type-5 and Type-2 density targets and the black-hole
    neighbour passes (blackhole_evaluate / blackhole_evaluate_swallow, proto.h:110-111);
  * on more than one rank: two processes, each holding the particles of its Peano-Hilbert key range,
    the key ranges taken from TopNodes[] / DomainStartList[] as domain_Decomposition leaves them,
    every exchange through the host's all-gather.
Checked against the oracle's single global tree: counts exact, sums to summation order."""
import ctypes as C
import importlib
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from common import O, SinkProblem, bindings, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-11

# struct particle_data of the shipped bundle (Makefile:8-255; SURVEY 8a a1: 536 bytes): the members
# the path and the sink passes touch, at offsets of this test's choosing inside the record -- the
# library only ever sees the offsets tables
P536 = np.dtype({
    "names": ["Pos", "Vel", "Mass", "ID", "GravAccel", "OldAcc", "GravCost", "Ti_begstep", "Ti_current",
              "Type", "TimeBin", "Hsml", "NumNgb", "SwallowID", "BH_Mass", "BH_Mdot", "BH_Density",
              "BH_Entropy", "BH_SurroundingGasVel", "BH_accreted_Mass", "BH_accreted_BHMass",
              "BH_accreted_DustMass", "BH_accreted_momentum", "DUST_Density", "DUST_Entropy",
              "DUST_SurroundingGasVel", "Dust_Mass", "rest"],
    "formats": [("f8", 3), ("f8", 3), "f8", "u4", ("f8", 3), "f8", "f4", "i4", "i4", "i2", "i2", "f8",
                "f8", "u4", "f8", "f8", "f8", "f8", ("f8", 3), "f8", "f8", "f8", ("f8", 3), "f8", "f8",
                ("f8", 3), "f8", ("u1", 248)],
    "offsets": [0, 24, 48, 56, 64, 88, 96, 100, 104, 108, 110, 112, 120, 128, 136, 144, 152, 160, 168,
                192, 200, 208, 216, 240, 248, 256, 280, 288],
    "itemsize": 536})
S264 = np.dtype({
    "names": ["Entropy", "Pressure", "VelPred", "MaxSignalVel", "Density", "DtEntropy", "HydroAccel",
              "DhsmlDensityFactor", "DivVel", "Rot", "Injected_BH_Energy", "rest"],
    "formats": ["f8", "f8", ("f8", 3), "f8", "f8", "f8", ("f8", 3), "f8", "f8", ("f8", 3), "f8",
                ("u1", 128)],
    "offsets": [0, 8, 16, 40, 48, 56, 64, 88, 96, 104, 128, 136],
    "itemsize": 264})


def bundle_layouts(B, H):
    lay = B.Layout()
    C.memset(C.byref(lay), 0xff, C.sizeof(lay))
    lay.p_stride, lay.s_stride = P536.itemsize, S264.itemsize
    for name, key in (("Pos", "p_pos"), ("Vel", "p_vel"), ("Mass", "p_mass"), ("GravAccel", "p_gravaccel"),
                      ("OldAcc", "p_oldacc"), ("GravCost", "p_gravcost"), ("Ti_begstep", "p_ti_begstep"),
                      ("Ti_current", "p_ti_current"), ("Type", "p_type"), ("TimeBin", "p_timebin"),
                      ("Hsml", "p_hsml"), ("NumNgb", "p_numngb")):
        setattr(lay, key, P536.fields[name][1])
    for name, key in (("Entropy", "s_entropy"), ("Pressure", "s_pressure"), ("VelPred", "s_velpred"),
                      ("MaxSignalVel", "s_maxsignalvel"), ("Density", "s_density"),
                      ("DtEntropy", "s_dtentropy"), ("HydroAccel", "s_hydroaccel"),
                      ("DhsmlDensityFactor", "s_dhsmlfac"), ("DivVel", "s_divvel"), ("Rot", "s_curlvel")):
        setattr(lay, key, S264.fields[name][1])
    bh = H.BhLayout()
    C.memset(C.byref(bh), 0xff, C.sizeof(bh))
    for name, key in (("ID", "p_id"), ("SwallowID", "p_swallowid"), ("BH_Mass", "p_bh_mass"),
                      ("BH_Mdot", "p_bh_mdot"), ("BH_Density", "p_bh_density"),
                      ("BH_Entropy", "p_bh_entropy"), ("BH_SurroundingGasVel", "p_bh_gasvel"),
                      ("BH_accreted_Mass", "p_bh_accreted_mass"),
                      ("BH_accreted_BHMass", "p_bh_accreted_bhmass"),
                      ("BH_accreted_DustMass", "p_bh_accreted_dustmass"),
                      ("BH_accreted_momentum", "p_bh_accreted_momentum"),
                      ("DUST_Density", "p_dust_density"), ("DUST_Entropy", "p_dust_entropy"),
                      ("DUST_SurroundingGasVel", "p_dust_gasvel"), ("Dust_Mass", "p_dust_mass")):
        setattr(bh, key, P536.fields[name][1])
    bh.s_injected_bh_energy = S264.fields["Injected_BH_Energy"][1]
    return lay, bh


def bundle_records(sp, idx=None):
    """the problem's particles (all, or those of `idx`: gas first) as 536 / 264-byte records"""
    pr = sp.pr
    idx = np.arange(pr.n) if idx is None else np.asarray(idx)
    gas = idx[idx < pr.ngas]
    P = np.zeros(len(idx), P536)
    S = np.zeros(len(gas), S264)
    rng = np.random.default_rng(2)
    P["rest"] = rng.integers(0, 255, (len(idx), 248), dtype=np.uint8)   # what the path must not touch
    S["rest"] = rng.integers(0, 255, (len(gas), 128), dtype=np.uint8)
    ic = pr.ic
    P["Pos"], P["Vel"], P["Mass"], P["Type"] = ic["pos"][idx], ic["vel"][idx], ic["mass"][idx], ic["type"][idx]
    P["ID"] = sp.ids[idx]
    P["TimeBin"], P["Ti_begstep"], P["Hsml"] = pr.timebin[idx], pr.ti_begstep[idx], sp.hsml[idx]
    P["BH_Mass"] = sp.bh_mass[idx]
    mdot = np.zeros(pr.n)
    mdot[sp.sinks] = sp.mdot
    P["BH_Mdot"] = mdot[idx]
    S["VelPred"], S["Entropy"], S["DtEntropy"] = pr.velpred[gas], pr.entropy[gas], pr.dtentropy[gas]
    return P, S


def set_all(host, sp, eps):
    pr, A = sp.pr, host.All
    A.G, A.ErrTolTheta, A.ErrTolForceAcc, A.TypeOfOpeningCriterion = pr.G, pr.theta, pr.ErrTolForceAcc, 1
    A.BoxSize, A.DesNumNgb, A.MaxNumNgbDeviation = pr.box, pr.des_ngb, pr.max_dev
    A.ArtBulkViscConst, A.Ti_Current, A.Timebase_interval = pr.visc, pr.ti_current, pr.timebase
    A.ComovingIntegrationOn, A.MinGasHsmlFractional = 0, 0.0
    for name in ("Gas", "Halo", "Disk", "Bulge", "Stars", "Bndry"):
        setattr(A, "Softening" + name, eps)
    A.BlackHoleNgbFactor = 1.5
    # ghip_bh_params out of All the way blackhole.c forms them (:1099, 1138-1139)
    A.UnitLength_in_cm, A.UnitMass_in_g, A.UnitEnergy_in_cgs = 1.0, sp.par["UnitMass_in_g"], 1.0
    A.CritOverDensity = 1.0 * sp.par["UnitMass_in_g"]           # -> CritDensity = 1
    A.BlackHoleFeedbackFactor = sp.par["FeedbackCoeff"] / (6.67e-8 * (4. * 3.1415 / 3. * 5.) ** 0.3333)
    A.SMBHmass, A.InnerBoundary, A.SinkBoundary = sp.SMBHmass, sp.par["InnerBoundary"], sp.par["SinkBoundary"]
    host.L.set_softenings()


def test_shipped_bundle_records_through_the_reference_named_drivers():
    B = bindings()
    H = importlib.import_module("gadget-leicester_amd.hostapi")
    sp = SinkProblem(ng=10, periodic=1, nsink=6, ndust=150)
    pr = sp.pr
    n, ng = pr.n, pr.ngas
    sp.hsml[sp.dust] = 2.0 * pr.ic["spacing"]      # a first guess for the grains' smoothing lengths
    eps = pr.force_soft[0] / 2.8
    lay, bh = bundle_layouts(B, H)
    P, S = bundle_records(sp)
    keep = P.copy()
    host = H.Host(periodic=1, black_holes=1, dust=1, accretion_of_dust_only=1, accretion_density=1)
    try:
        host.bind_records(P, S, lay, bh)
        set_all(host, sp, eps)
        host.set_active(None)
        host.domain()
        L = host.L
        # ---- accel.c:61-106 ----
        L.gravity_tree()
        L.gravity_tree()
        L.density()
        L.force_update_hmax()
        L.hydro_force()
        assert host.endrun_codes == [], L.gadget_force_last_error()
        # ---- the oracle's single tree on the same particles ----
        T = O.Tree(pr.ic["pos"], pr.ic["vel"], pr.ic["mass"], pr.ic["type"], pr.force_soft, hsml=sp.hsml,
                   extent=pr.extent)
        tg = np.arange(n, dtype=np.int32)
        tab = O.ewald_table(pr.box)
        a0, c0 = T.gravity(pr.o_grav(pr.theta), tg, np.zeros(n))
        T.gravity_ewald_add(pr.o_grav(pr.theta), tab, tg, np.zeros(n), a0, c0)
        old = np.linalg.norm(a0, axis=1)
        a1, c1 = T.gravity(pr.o_grav(0.0), tg, old)
        T.gravity_ewald_add(pr.o_grav(0.0), tab, tg, old, a1, c1)
        assert np.array_equal(P["GravCost"].astype(np.int64), c1)
        assert relerr(P["GravAccel"], pr.G * a1) < TOL
        act = np.arange(ng, dtype=np.int32)
        od = T.density(pr.o_dens(), act, pr.velpred, pr.entropy, pr.dtentropy, pr.timebin, pr.ti_begstep,
                       sp.hsml)
        assert relerr(P["Hsml"][:ng], od["hsml"][:ng]) < 1e-13
        assert relerr(S["Density"], od["density"][:ng]) < TOL
        assert np.abs(P["NumNgb"][:ng] - od["numngb"][:ng]).max() < 1e-10
        # the Type-5 and Type-2 density targets (density.c:549-556): h iterated in P[], the smoothed
        # surroundings in the b1-b3 / d1-d3 unions
        osk = O.sink_density(T, pr.o_dens(), 1.5, sp.sinks, pr.velpred, pr.entropy, sp.hsml)
        assert relerr(P["Hsml"][sp.sinks], osk["hsml"][sp.sinks]) < 1e-13
        assert relerr(P["BH_Density"][sp.sinks], osk["density"]) < 1e-12
        assert relerr(P["BH_Entropy"][sp.sinks], osk["entropy"]) < 1e-12
        assert np.abs(P["BH_SurroundingGasVel"][sp.sinks] - osk["gasvel"]).max() < 1e-12 * np.abs(osk["gasvel"]).max()
        dust = sp.dust.astype(np.int32)
        odu = O.sink_density(T, pr.o_dens(), 1.0, dust, pr.velpred, pr.entropy, sp.hsml)
        assert relerr(P["Hsml"][dust], odu["hsml"][dust]) < 1e-13
        assert relerr(P["DUST_Density"][dust], odu["density"]) < 1e-12
        other = np.setdiff1d(np.arange(ng, n), np.concatenate([sp.sinks, dust]))
        assert np.array_equal(P["Hsml"][other], keep["Hsml"][other])       # nobody else's
        hs = od["hsml"].copy()
        hs[sp.sinks], hs[dust] = osk["hsml"][sp.sinks], odu["hsml"][dust]
        T.update_hmax(act, od["hsml"], od["divvel"])
        oh = T.hydro(pr.o_hydro(), act, pr.velpred, od["hsml"], od["density"], od["pressure"],
                     od["dhsmlfac"], od["divvel"], od["curlvel"], pr.timebin)
        assert np.abs(S["HydroAccel"] - oh["hydroaccel"][:ng]).max() < TOL * np.abs(oh["hydroaccel"]).max()
        assert np.abs(S["DtEntropy"] - oh["dtentropy"][:ng]).max() < TOL * np.abs(oh["dtentropy"]).max()
        # ---- the neighbour passes of blackhole_accretion() (blackhole.c:294-660) ----
        over = dict(accretion_of_dust_only=1, accretion_density=1, CritDensity=1.0, SofteningBndry=eps)
        op = sp.params(O.BhParams, **over)
        T2 = O.Tree(pr.ic["pos"], pr.ic["vel"], pr.ic["mass"].copy(), pr.ic["type"], pr.force_soft, hsml=hs,
                    extent=pr.extent)
        osw, oinj = O.blackhole_evaluate(T2, op, sp.sinks, sp.ids, hs, pr.timebin, sp.mdot, osk["density"],
                                         od["density"][:ng], np.zeros(n, np.uint32), np.zeros(ng))
        oo = O.blackhole_swallow(T2, op, sp.sinks, sp.ids, hs, osw, sp.bh_mass, unclaimed_only=True)
        L.blackhole_accretion_neighbour_passes()
        assert host.endrun_codes == [], L.gadget_force_last_error()
        assert np.array_equal(P["SwallowID"], osw) and (osw > 0).sum() > 3
        assert np.abs(S["Injected_BH_Energy"] - oinj).max() <= 1e-12 * max(np.abs(oinj).max(), 1e-300)
        assert np.abs(P["BH_accreted_Mass"][sp.sinks] - oo["acc_mass"]).max() <= 1e-13 * np.abs(oo["acc_mass"]).max()
        assert np.abs(P["BH_accreted_momentum"][sp.sinks] - oo["acc_momentum"]).max() <= \
            1e-13 * max(np.abs(oo["acc_momentum"]).max(), 1e-300)
        assert np.array_equal(P["Mass"], T2.mass)            # the victims at zero, nobody else touched
        counts = [C.c_int.in_dll(L, k).value for k in ("N_gas_swallowed", "N_BH_swallowed", "N_dust_swallowed")]
        assert counts == [int(v) for v in oo["counts"]]
        # the per-sink entry points (proto.h:110-111) do the same one sink at a time
        P2, S2 = bundle_records(sp)
        P2["Hsml"], P2["BH_Density"] = hs, P["BH_Density"]
        S2["Density"] = S["Density"]
        host.bind_records(P2, S2, lay, bh)
        host.set_active(None)
        for t in sp.sinks:
            assert L.blackhole_evaluate(int(t), 0, None, None) == 0
        assert np.array_equal(P2["SwallowID"], osw)
        for t in sp.sinks:
            assert L.blackhole_evaluate_swallow(int(t), 0, None, None) == 0
        assert np.array_equal(P2["Mass"], T2.mass)
        assert np.abs(P2["BH_accreted_Mass"][sp.sinks] - oo["acc_mass"]).max() <= 1e-13 * np.abs(oo["acc_mass"]).max()
        assert host.endrun_codes == [], L.gadget_force_last_error()
        for name in ("Pos", "Vel", "ID", "Type", "rest"):
            assert np.array_equal(P[name], keep[name]), name
    finally:
        host.close()


@pytest.mark.parametrize("name", ["pair", "clump"])
def test_claimed_sinks_swallow_nothing_through_the_reference_named_driver(name):
    """blackhole_accretion_neighbour_passes() on 536-byte records of the two inputs in which sinks claim each
    other (tests/common.py: `pair`, the mutual claim; `clump`, the chain C -> B -> A), accretion of gas on:
    P[].SwallowID and P[].Mass afterwards are those of blackhole.c restated over all pairs
    (tests/sink_ref.py), where the swallow pass runs only for sinks with SwallowID == 0 (blackhole.c:528-532).
    The sinks' Hsml and BH_Density and the gas Density are put into the records as density() leaves them."""
    from common import check_sink_passes, sink_case, sink_reference
    B = bindings()
    H = importlib.import_module("gadget-leicester_amd.hostapi")
    sp = sink_case(name, 1)
    ref = sink_reference(name, 1, 0, 0)
    pr, sk, rs = sp.pr, sp.sinks, ref["swallow"]
    lay, bh = bundle_layouts(B, H)
    P, S = bundle_records(sp)
    P["Hsml"] = sp.dens["hsml"]
    P["BH_Density"][sk] = sp.dens["density"]
    S["Density"] = sp.gas_density
    keep = P.copy()
    host = H.Host(periodic=1, black_holes=1, dust=1, accretion_of_dust_only=0, accretion_density=0)
    try:
        host.bind_records(P, S, lay, bh)
        set_all(host, sp, pr.force_soft[0] / 2.8)
        host.All.SofteningBndry = sp.par["SofteningBndry"]      # (after set_softenings(): the table keeps eps)
        host.set_active(None)
        host.domain()
        L = host.L
        L.blackhole_accretion_neighbour_passes()
        assert host.endrun_codes == [], L.gadget_force_last_error()
        got = dict(counts=np.array([C.c_int.in_dll(L, k).value for k in
                                    ("N_gas_swallowed", "N_BH_swallowed", "N_dust_swallowed")]),
                   acc_mass=P["BH_accreted_Mass"][sk], acc_bhmass=P["BH_accreted_BHMass"][sk],
                   acc_dustmass=P["BH_accreted_DustMass"][sk], acc_momentum=P["BH_accreted_momentum"][sk],
                   bh_mass=P["BH_Mass"][sk])
        err = check_sink_passes(sp, ref, None, (P["SwallowID"], S["Injected_BH_Energy"]), got, P["Mass"])
        print(name, err)
        claimed = ref["sw"][sk] > 0
        assert claimed.sum() >= 2 and rs["skipped"][claimed].all()
        kept = (ref["sw"] > 0) & ~rs["swallowed"]               # the victims of claimed sinks
        assert kept.sum() >= 6 and np.array_equal(P["Mass"][kept], keep["Mass"][kept])
        if name == "pair":
            assert not got["counts"].any() and np.array_equal(P["Mass"], keep["Mass"])
        for field in ("Pos", "Vel", "ID", "Type", "rest"):
            assert np.array_equal(P[field], keep[field]), field
    finally:
        host.close()


def test_four_call_sequence_on_two_ranks_through_the_reference_named_symbols():
    """accel.c's sequence with NTask = 2: one process per rank (as the reference's MPI ranks), both on
    this box's one GPU, each with its 536-byte records, the ranks' key ranges out of TopNodes /
    DomainStartList, exchanges through the host's all-gather (gloo here, MPI_Allgather in a host).
    tests/gpu_host_ranks.py is the rank program (BLACK_HOLES + DUST configuration: density() also serves
    the Type-5 / Type-2 targets, and blackhole_accretion's neighbour passes follow); rank 0 checks the
    gathered records against the oracle's single global tree."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "tests", "gpu_host_ranks.py")]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["ok"], out
    assert out["counts_equal"] and out["rel_acc"] < TOL and out["rel_density"] < TOL
    assert out["rel_hydro"] < TOL and out["particles"] == out["particles_expected"]
    # density() of the sinks and dust grains, and the neighbour passes of blackhole_accretion(), as
    # collectives: every rank's sinks meet every rank's particles
    assert out["rel_sink_density"] < 1e-12
    assert out["marks_equal"] and out["victims"] > 3 and out["masses_equal"]
    assert out["rel_injected"] < 1e-12 and out["rel_accreted"] < 1e-13
    assert out["swallow_counts"] == out["swallow_counts_oracle"]


# ------------------------------------------------------------------------------------------------
# one mirror through a changing NumPart
# ------------------------------------------------------------------------------------------------
def _mirror_problems():
    from common import Problem
    rng = np.random.default_rng(41)

    def uniform(n, ngas):
        typ = np.where(np.arange(n) < ngas, 0, 1).astype(np.int32)
        return dict(pos=rng.random((n, 3)), vel=rng.standard_normal((n, 3)), mass=rng.uniform(0.5, 2.0, n) / n,
                    type=typ, ngas=ngas, boxsize=1.0, spacing=1.0 / max(2.0, n ** (1 / 3)),
                    id=np.arange(1, n + 1, dtype=np.uint32), u=np.full(ngas, 0.01))
    return [Problem(ng=8, gas=True, periodic=1),                       # 1024 particles, 512 of them gas
            Problem(ic=uniform(1500, 300), periodic=1),                # fewer gas records, more particles
            Problem(ic=uniform(50, 0), periodic=1)]                    # a small set with no gas


def _mirror_step(host, H, pr):
    """accel.c's sequence on the particles of `pr`, given to the mirror `host` with set_particles"""
    P = np.zeros(pr.n, H.P_DTYPE)
    S = np.zeros(pr.ngas, H.SPH_DTYPE) if pr.ngas else None
    P["Pos"], P["Vel"], P["Mass"], P["Type"] = pr.ic["pos"], pr.ic["vel"], pr.ic["mass"], pr.ic["type"]
    P["ID"] = pr.ic["id"]
    P["TimeBin"], P["Ti_begstep"] = pr.timebin, pr.ti_begstep
    if pr.ngas:
        S["VelPred"], S["Entropy"], S["DtEntropy"] = pr.velpred, pr.entropy, pr.dtentropy
        S["Hsml"] = pr.hsml0[:pr.ngas]
    host.set_particles(P, S)
    A = host.All
    A.G, A.ErrTolTheta, A.ErrTolForceAcc, A.TypeOfOpeningCriterion = pr.G, pr.theta, pr.ErrTolForceAcc, 1
    A.BoxSize, A.DesNumNgb, A.MaxNumNgbDeviation = pr.box, pr.des_ngb, pr.max_dev
    A.ArtBulkViscConst, A.Ti_Current, A.Timebase_interval = pr.visc, pr.ti_current, pr.timebase
    A.ComovingIntegrationOn, A.MinGasHsmlFractional = 0, 0.0
    eps = pr.force_soft[0] / 2.8
    for name in ("Gas", "Halo", "Disk", "Bulge", "Stars", "Bndry"):
        setattr(A, "Softening" + name, eps)
    host.L.set_softenings()
    host.set_active(None)
    host.domain()
    L = host.L
    L.gravity_tree()
    L.gravity_tree()                     # (the second pass opens cells by the first one's accelerations)
    if pr.ngas:
        L.density()
        L.force_update_hmax()
        L.hydro_force()
    assert host.endrun_codes == [], L.gadget_force_last_error()
    out = {k: P[k].copy() for k in ("GravAccel", "OldAcc", "GravCost")}
    if pr.ngas:
        out.update({k: S[k].copy() for k in ("Density", "Hsml", "HydroAccel", "DtEntropy", "DivVel", "Pressure",
                                             "MaxSignalVel")})
    return out


def test_one_mirror_through_three_particle_sets_equals_a_mirror_per_set():
    """set_particles three times on ONE Host -- some n and ngas; fewer gas records but more particles; a small
    set with no gas -- with accel.c's gravity (and, where there is gas, density and hydro) after each: what the
    mirror keeps between the calls (gadget_force_mark_dirty, TreeReconstructFlag, its context) does not reach
    the results.  Each step equals a Host created for it alone: every integer and every SPH result to the
    bit, the gravity accelerations (and OldAcc, their norm) to 1e-10 of the largest -- the order of a target's
    partial sums follows the plan history of the context, the bound is that of tests/gpu_fuzz.py."""
    H = importlib.import_module("gadget-leicester_amd.hostapi")
    problems = _mirror_problems()
    assert problems[1].n > problems[0].n and 0 < problems[1].ngas < problems[0].ngas
    assert problems[2].ngas == 0 and problems[2].n < problems[0].n // 2
    host = H.Host(periodic=1)
    try:
        kept = [_mirror_step(host, H, pr) for pr in problems]
    finally:
        host.close()
    for step, pr in enumerate(problems):
        host = H.Host(periodic=1)
        try:
            alone = _mirror_step(host, H, pr)
        finally:
            host.close()
        assert kept[step].keys() == alone.keys()
        differ = {k: float(np.abs(kept[step][k] - alone[k]).max() / np.abs(alone[k]).max())
                  for k in alone if not np.array_equal(kept[step][k], alone[k])}
        print("step %d (n %d, gas %d): not bit-equal to a mirror of its own: %r" % (step, pr.n, pr.ngas, differ))
        assert np.abs(alone["GravAccel"]).max() > 0
        for k, v in differ.items():
            assert k in ("GravAccel", "OldAcc"), "step %d: %s differs by %.3e" % (step, k, v)
            assert v < 1e-10, (step, k, v)
