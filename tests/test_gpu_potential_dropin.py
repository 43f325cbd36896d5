"""The drop-in compute_potential() / compute_global_quantities_of_system() (include/gadget_force.h) on the
shipped bundle's 536 / 264-byte records, and the argument rules of ghip_potential /
ghip_global_quantities: checks before any launch, OldAcc only for the relative criterion, a potential
that no longer belongs to the state, the short-range walk alone."""
import importlib

import numpy as np
import pytest

from common import Problem, bindings
import potential_ref as R
from test_gpu_potential import TOL, _device, _err, _pot_params, _ref_walk

pytestmark = pytest.mark.gpu
B = bindings()

# the bundle's particle_data with p.Potential and OldPhotonMomentum in its spare bytes; every byte belongs
# to a field (the members the potential does not use are opaque bytes), so that a copy is exact
P536 = np.dtype({
    "names": ["Pos", "Vel", "Mass", "ID", "pad0", "GravAccel", "OldAcc", "GravCost", "Ti_begstep",
              "Ti_current", "Type", "TimeBin", "Hsml", "NumNgb", "bundle", "Potential", "OldPhotonMomentum",
              "rest"],
    "formats": [("f8", 3), ("f8", 3), "f8", "u4", ("u1", 4), ("f8", 3), "f8", "f4", "i4", "i4", "i2", "i2",
                "f8", "f8", ("u1", 264), "f8", "f8", ("u1", 128)],
    "offsets": [0, 24, 48, 56, 60, 64, 88, 96, 100, 104, 108, 110, 112, 120, 128, 392, 400, 408],
    "itemsize": 536})
S264 = np.dtype({
    "names": ["Entropy", "Pressure", "VelPred", "MaxSignalVel", "Density", "DtEntropy", "HydroAccel",
              "DhsmlDensityFactor", "DivVel", "Rot", "pad0", "rest"],
    "formats": ["f8", "f8", ("f8", 3), "f8", "f8", "f8", ("f8", 3), "f8", "f8", ("f8", 3), ("u1", 8),
                ("u1", 128)],
    "offsets": [0, 8, 16, 40, 48, 56, 64, 88, 96, 104, 128, 136],
    "itemsize": 264})
# struct state_of_system of the fork (allvars.h:1646-1667, without CHECK_ENERGY_CONSERVATION)
_SYS = [("Mass", 1), ("EnergyRadComp", 1), ("EnergyRadAdded", 1), ("EnergyRadDeleted", 1), ("EnergyKin", 1),
        ("EnergyPot", 1), ("EnergyInt", 1), ("EnergyTot", 1), ("Momentum", 4), ("AngMomentum", 4),
        ("CenterOfMass", 4), ("MassComp", 6), ("EnergyKinComp", 6), ("EnergyPotComp", 6),
        ("EnergyIntComp", 6), ("EnergyTotComp", 6), ("MomentumComp", 24), ("AngMomentumComp", 24),
        ("CenterOfMassComp", 24)]
SYSD = np.dtype({"names": [k for k, _ in _SYS],
                 "formats": ["f8" if c == 1 else ("f8", c) for _, c in _SYS],
                 "offsets": list(np.cumsum([0] + [8 * c for _, c in _SYS])[:-1]),
                 "itemsize": 8 * sum(c for _, c in _SYS)})


def _layout():
    lay = B.Layout()
    import ctypes as C
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
    return lay


def test_dropin_potential_and_global_quantities_on_bundle_records():
    H = importlib.import_module("gadget-leicester_amd.hostapi")
    pr = Problem(ng=8, periodic=1)
    n, ng = pr.n, pr.ngas
    rng = np.random.default_rng(21)
    P = np.zeros(n, P536)
    S = np.zeros(ng, S264)
    P["rest"] = rng.integers(0, 255, (n, 128), dtype=np.uint8)
    P["bundle"] = rng.integers(0, 255, (n, 264), dtype=np.uint8)
    P["pad0"] = rng.integers(0, 255, (n, 4), dtype=np.uint8)
    S["rest"] = rng.integers(0, 255, (ng, 128), dtype=np.uint8)
    S["pad0"] = rng.integers(0, 255, (ng, 8), dtype=np.uint8)
    ptype = pr.ic["type"].astype(np.int16).copy()
    ptype[ng:][rng.random(n - ng) < 0.2] = 3
    P["Pos"], P["Vel"], P["Mass"], P["Type"] = pr.ic["pos"], pr.ic["vel"], pr.ic["mass"], ptype
    P["ID"] = np.arange(1, n + 1)
    P["TimeBin"] = rng.integers(0, 6, n)
    P["Ti_begstep"] = rng.integers(0, 200, n)
    P["Ti_current"] = 400
    P["GravAccel"] = rng.standard_normal((n, 3))
    P["Hsml"][:ng] = pr.hsml0[:ng]
    P["Potential"] = 7.0
    P["OldPhotonMomentum"] = rng.random(n)
    S["Entropy"], S["DtEntropy"] = pr.entropy, pr.dtentropy
    S["Density"], S["HydroAccel"] = 1 + rng.random(ng), rng.standard_normal((ng, 3))
    host = H.Host(periodic=1)
    try:
        host.bind_records(P, S, _layout())
        a = host.All
        a.G, a.ErrTolTheta, a.ErrTolForceAcc, a.TypeOfOpeningCriterion = 0.9, 0.5, pr.ErrTolForceAcc, 0
        a.BoxSize, a.Ti_Current, a.Timebase_interval, a.ComovingIntegrationOn = pr.box, 400, 1e-3, 0
        a.Time, a.OmegaLambda, a.Hubble = 1.0, 0.0, 0.1
        eps = pr.force_soft[0] / 2.8
        for name in ("Gas", "Halo", "Disk", "Bulge", "Stars", "Bndry"):
            setattr(a, "Softening" + name, eps)
        host.L.set_softenings()
        host.set_active(None)
        host.domain()
        sysst = np.zeros(1, SYSD)
        sysst["EnergyRadAdded"], sysst["EnergyRadDeleted"] = 11.0, 13.0
        pl = H.PotentialLayout()
        for k in ("p_potential", "p_old_photon_momentum"):
            setattr(pl, k, P536.fields["Potential" if k == "p_potential" else "OldPhotonMomentum"][1])
        for k, _ in _SYS:
            setattr(pl, "sys_" + k, SYSD.fields[k][1])
        pl.a_pm_ti_begstep = pl.a_pm_ti_endstep = -1
        pl.rad_fac = 2.0
        host.bind_potential(sysst, pl)
        P0, S0 = P.copy(), S.copy()
        host.compute_potential()
        assert host.endrun_codes == []
        # only the bytes of p.Potential changed
        pb, p0b = P.view(np.uint8).reshape(n, -1), P0.view(np.uint8).reshape(n, -1)
        other = np.ones(P536.itemsize, bool)
        other[392:400] = False
        assert np.array_equal(pb[:, other], p0b[:, other])
        assert np.array_equal(S.view(np.uint8), S0.view(np.uint8))
        assert not np.any(P["Potential"] == 7.0)
        # = the device potential of the same state through the C-ABI, with All's G and softenings
        fp = pr.device()
        fp.set_field(B.F_TYPE, ptype.astype(np.int32))
        fp.set_field(B.F_OLDACC, np.zeros(n))
        fp.tree_build(*host.domain(), np.full(6, 2.8 * eps))
        p = _pot_params(pr, 0.5, G=0.9, Hubble=0.1)
        for i in range(6):
            p.SofteningTable[i] = eps
            p.grav.ForceSoftening[i] = 2.8 * eps
        fp.potential(p)
        dev = fp.get_potential()
        fp.close()
        assert _err(P["Potential"], dev) < TOL
        # compute_global_quantities_of_system: SysState from the records, nothing else written
        P1 = P.copy()
        host.compute_global_quantities_of_system()
        assert host.endrun_codes == []
        assert np.array_equal(P.view(np.uint8), P1.view(np.uint8))
        ref, scale = R.global_quantities(
            P["Pos"], P["Vel"], P["Mass"], P["Type"], P["TimeBin"], P["Ti_begstep"], P["GravAccel"], 400,
            1e-3, pot=P["Potential"], ngas=ng, hydroaccel=S["HydroAccel"], entropy=S["Entropy"],
            dtentropy=S["DtEntropy"], density=S["Density"], photon=P["OldPhotonMomentum"], rad_fac=2.0)
        st = sysst[0]
        dev = {k: st[k] for k in ("MassComp", "EnergyKinComp", "EnergyPotComp", "EnergyIntComp")}
        for k in ("MomentumComp", "AngMomentumComp"):
            v = st[k].reshape(6, 4).copy()
            # global.c:214-227: element [3] of each row is the norm of the first three
            assert np.allclose(v[:, 3], np.linalg.norm(v[:, :3], axis=1), rtol=1e-14, atol=0)
            v[:, 3] = 0.0
            dev[k] = v
        dev["EnergyRadComp"] = st["EnergyRadComp"]
        sub = {k: ref[k] for k in dev}
        assert R.max_rel_diff(dev, sub, scale) < TOL
        assert st["EnergyTot"] == pytest.approx(ref["EnergyKinComp"].sum() + ref["EnergyPotComp"].sum() +
                                                ref["EnergyIntComp"].sum(), rel=1e-12)
        com = st["CenterOfMassComp"].reshape(6, 4)
        m = ref["MassComp"]
        for t in np.nonzero(m > 0)[0]:
            assert np.allclose(com[t, :3], ref["CenterOfMassComp"][t, :3] / m[t], rtol=1e-12, atol=1e-14)
            assert com[t, 3] == pytest.approx(np.linalg.norm(com[t, :3]), rel=1e-14)
        assert st["EnergyRadAdded"] == 11.0 and st["EnergyRadDeleted"] == 13.0
        # more than one rank: endrun(90012), nothing written
        host._seti("NTask", 2)
        P2 = P.copy()
        host.compute_potential()
        host.compute_global_quantities_of_system()
        assert host.endrun_codes == [90012, 90012]
        assert np.array_equal(P.view(np.uint8), P2.view(np.uint8))
        host._seti("NTask", 1)
    finally:
        host.close()


def test_shortrange_walk_alone_at_full_precision():
    """pm.G = 0 adds a mesh potential of exactly zero: what remains is the short-range walk"""
    pr = Problem(ng=8, periodic=1)
    fp, old = _device(pr)
    p = _pot_params(pr, 0.0, pmgrid=16)
    p.pm.G = 0.0
    fp.potential(p)
    dev = fp.get_potential()
    w, nint = _ref_walk(fp, pr, 0.0, old, np.arange(pr.n), pmgrid=16)
    ic = pr.ic
    ref = R.finish(w, ic["pos"], ic["mass"], ic["type"], pr.force_soft / 2.8, 1.0)
    assert _err(dev, ref) < TOL
    assert fp.potential_interactions()[0] == int(nint.sum())
    fp.close()


def test_arguments_are_checked_before_anything_runs():
    pr = Problem(ng=4, periodic=1)
    fp = pr.device()
    pr.device_tree(fp)
    # Barnes-Hut does not read OldAcc: the field is never set here
    fp.potential(_pot_params(pr, 0.5))
    first = fp.get_potential()
    bad = []
    p = _pot_params(pr, 0.5, pmgrid=16)
    p.grav.periodic = 0
    bad.append(p)
    p = _pot_params(pr, 0.5, pmgrid=15)
    bad.append(p)
    p = _pot_params(pr, 0.5, pmgrid=16)
    p.pm.BoxSize = 2 * pr.box
    bad.append(p)
    p = _pot_params(pr, 0.5, pmgrid=16)
    p.pm.Asmth = 0.0
    bad.append(p)
    for p in bad:
        with pytest.raises(B.GhipError) as e:
            fp.potential(p)
        assert B.GHIP_ERRORS[e.value.code] == "GHIP_EINVAL"
        # refused before the walk: the last result is still the one handed out
        assert np.array_equal(fp.get_potential(), first)
    # a potential stops belonging to the state when the positions change
    fp.set_field(B.F_POS, pr.ic["pos"])
    with pytest.raises(B.GhipError):
        fp.get_potential()
    # the binding leaves no pointers in the caller's parameters
    g = B.GlobalParams()
    g.Ti_Current, g.Timebase_interval, g.Time = 2, 1e-3, 1.0
    fp.set_field(B.F_GRAVACCEL, np.zeros((pr.n, 3)))
    fp.set_field(B.F_HYDROACCEL, np.zeros((pr.ngas, 3)))
    fp.set_field(B.F_DENSITY, np.ones(pr.ngas))
    out = fp.global_quantities(g, old_photon_momentum=np.ones(pr.n), potential=np.full(pr.n, -1.0))
    assert g.OldPhotonMomentum is None and g.Potential is None
    assert out["EnergyPotComp"].sum() == pytest.approx(-0.5 * pr.ic["mass"].sum(), rel=1e-12)
    fp.close()
