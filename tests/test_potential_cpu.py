"""CPU checks of the potential restatement (tests/potential_ref.py) and of the C-ABI of ghip_potential /
ghip_global_quantities: the walk over the oracle's tree with every node opened is the direct sum, the
Ewald potential correction is consistent with the oracle's correction force, the global.c sums of
hand-made particle sets, the exported symbols and the struct layouts.  No GPU is used."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from common import O, REPO, bindings, ics, pkg
import potential_ref as R


def _plummer(n=600, seed=3):
    ic = ics.make_plummer(n, seed=seed, gas_fraction=0.3)
    rng = np.random.default_rng(seed)
    ptype = ic["type"].copy()
    dm = np.nonzero(ptype != 0)[0]
    ptype[dm[rng.random(len(dm)) < 0.3]] = 2
    ptype[dm[rng.random(len(dm)) < 0.1]] = 4
    mass = ic["mass"] * (0.5 + rng.random(n))
    return ic["pos"], ic["vel"], mass, ptype, int(ic["ngas"])


@pytest.mark.parametrize("mode", ["equal", "unequal", "adaptive"])
def test_walk_with_every_node_opened_is_the_direct_sum(mode):
    pos, vel, mass, ptype, ngas = _plummer()
    n = len(pos)
    table = np.full(6, 0.01) if mode == "equal" else np.array([0.010, 0.020, 0.005, 0.015, 0.030, 0.008])
    fs = 2.8 * table
    hs = np.zeros(n)
    hs[:ngas] = 0.02 + 0.05 * np.random.default_rng(1).random(ngas)
    T = O.Tree(pos, vel, mass, ptype, fs, hsml=hs, extent=O.domain_extent(pos))
    if mode == "adaptive":
        T.adaptive_gravsoft()
    psoft = fs[ptype].copy()
    if mode == "adaptive":
        psoft[:ngas] = hs[:ngas]
    unequal = mode != "equal"
    rt = R.RefTree.from_oracle(T.dump(), pos, mass, psoft, adaptive=(mode == "adaptive"))
    pot, nint = R.walk_potential(rt, pos, psoft, np.zeros(n), theta=1e-8, unequal=unequal)
    assert np.all(nint == n)                       # every particle, one by one, itself included
    ref = R.direct_potential(pos, mass, psoft, psoft, np.arange(n), unequal=unequal)
    assert np.max(np.abs(pot - ref) / np.abs(ref)) < 1e-12
    # an ordinary opening angle accepts nodes: fewer interactions, close to the sum
    p5, n5 = R.walk_potential(rt, pos, psoft, np.zeros(n), theta=0.5, unequal=unequal)
    assert n5.mean() < 0.5 * n
    assert np.max(np.abs(p5 - ref) / np.abs(ref)) < 1e-2


def test_ewald_psi_is_symmetric_and_its_gradient_is_the_oracle_correction_force():
    rng = np.random.default_rng(4)
    x = rng.uniform(0.05, 0.45, (6, 3))
    psi = R.ewald_psi(x)
    assert np.all(np.isfinite(psi))
    for perm in ([1, 0, 2], [2, 1, 0], [0, 2, 1]):
        assert np.allclose(R.ewald_psi(x[:, perm]), psi, rtol=1e-13, atol=0)
    assert np.allclose(R.ewald_psi(-x), psi, rtol=1e-13, atol=0)
    assert np.allclose(R.ewald_psi(x * [-1, 1, -1]), psi, rtol=1e-13, atol=0)
    eps = 1e-5
    G, F = [], []
    for xi in x:
        G.append([(R.ewald_psi(xi + d)[0] - R.ewald_psi(xi - d)[0]) / (2 * eps) for d in np.eye(3) * eps])
        F.append(O.ewald_force(1, 1, 1, xi))   # (0, 0, 0 is the origin entry: no force)
    G, F = np.array(G), np.array(F)
    sign = np.sign(np.sum(G * F))
    assert np.max(np.abs(G - sign * F)) < 1e-6 * np.abs(F).max()
    # the table: the origin entry and psi / BoxSize elsewhere
    t = R.pot_table(2.0, idx=[[0, 0, 0], [3, 5, 7]])
    assert t[0] == R.POT_ORIGIN / 2.0
    assert t[1] == R.ewald_psi(0.5 * np.array([[3.0, 5.0, 7.0]]) / R.EN)[0] / 2.0


def _hand_set():
    pos = np.array([[1., 0, 0], [0, 2., 0], [0, 0, 3.], [1., 1., 1.]])
    vel = np.array([[0., 1, 0], [1., 0, 0], [0, 0, -1.], [2., 0, 0]])
    mass = np.array([2.0, 1.0, 3.0, 0.5])
    ptype = np.array([0, 1, 1, 3])
    timebin = np.array([2, 0, 3, 1])               # steps 4, 0, 8, 2
    ti_begstep = np.array([10, 12, 8, 11])         # mid-points all 12
    gacc = np.array([[1., 0, 0], [0, 0, 0], [0, 0, 1.], [0, 0, 0]])
    return dict(pos=pos, vel=vel, mass=mass, ptype=ptype, timebin=timebin, ti_begstep=ti_begstep,
                gravaccel=gacc, Ti_Current=14, pot=np.array([-1.0, -2.0, -0.5, -4.0]), ngas=1,
                hydroaccel=np.array([[0., 0, 2.]]), entropy=np.array([3.0]), dtentropy=np.array([1.0]),
                density=np.array([8.0]), photon=np.array([0, 0, 0, 5.0]), rad_fac=2.0)


def test_global_quantities_of_a_hand_made_set():
    s = _hand_set()
    out, _ = R.global_quantities(timebase=0.5, **s)       # dt = (14 - 12) * 0.5 = 1 for all
    # predicted velocities (1,1,2), (1,0,0), (0,0,0), (2,0,0)
    assert out["MassComp"].tolist() == [2, 4, 0, 0.5, 0, 0]
    assert out["EnergyKinComp"].tolist() == [6.0, 0.5, 0, 1.0, 0, 0]
    assert out["EnergyPotComp"].tolist() == [-1.0, -1.75, 0, -1.0, 0, 0]
    assert np.isclose(out["EnergyIntComp"][0], 2 * 4 / 0.4 * 8 ** 0.4, rtol=1e-14)
    assert out["EnergyIntComp"][1:].tolist() == [0] * 5
    assert out["MomentumComp"][0].tolist() == [2, 2, 4, 0]
    assert out["MomentumComp"][1].tolist() == [1, 0, 0, 0]
    assert out["MomentumComp"][3].tolist() == [1, 0, 0, 0]
    assert out["CenterOfMassComp"][1].tolist() == [0, 2, 9, 0]
    assert out["AngMomentumComp"][0].tolist() == [0, -4, 2, 0]
    assert out["AngMomentumComp"][1].tolist() == [0, 0, -2, 0]
    assert out["AngMomentumComp"][3].tolist() == [0, 1, -1, 0]
    assert out["EnergyRadComp"] == 10.0


def test_global_quantities_of_a_hand_made_set_comoving():
    s = _hand_set()
    # linear kick tables: factor(t0, t1) = alpha * 1000 * (t1 - t0) * timebase / (logTimeMax - logTimeBegin)
    gk = 0.01 * np.arange(1, 1001)
    hk = 0.02 * np.arange(1, 1001)
    out, _ = R.global_quantities(timebase=0.5, comoving=1, time=0.5, tables=(0.0, 10.0, gk, hk), **s)
    # dt_gravkick 1, dt_hydrokick 2, dt_entr 1; a = 0.5
    assert np.allclose(out["EnergyKinComp"], [72.0, 2.0, 0, 4.0, 0, 0], rtol=1e-12, atol=0)
    assert np.allclose(out["EnergyPotComp"], [-2.0, -3.5, 0, -2.0, 0, 0], rtol=1e-14, atol=0)
    assert np.isclose(out["EnergyIntComp"][0], 2 * 4 / 0.4 * 64.0 ** 0.4, rtol=1e-12)
    assert np.allclose(out["MomentumComp"][0], [2, 2, 8, 0], rtol=1e-12, atol=0)


NEW_SYMBOLS = ("ghip_potential", "ghip_get_potential", "ghip_potential_interactions",
               "ghip_ewald_get_pot_table", "ghip_global_quantities")


def test_new_entry_points_are_exported_and_structs_match_the_ctypes_mirrors(tmp_path):
    L = C.CDLL(pkg.lib_path())
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    B = bindings()
    src = tmp_path / "probe.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "ghip.h"\n'
        'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ghip_pot_params),'
        ' offsetof(ghip_pot_params, pm), offsetof(ghip_pot_params, G), offsetof(ghip_pot_params, Hubble),'
        ' sizeof(ghip_global_params), offsetof(ghip_global_params, rad_fac), sizeof(ghip_global_sums),'
        ' offsetof(ghip_global_sums, EnergyRadComp)); return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(B.PotParams), B.PotParams.pm.offset, B.PotParams.G.offset, B.PotParams.Hubble.offset,
            C.sizeof(B.GlobalParams), B.GlobalParams.rad_fac.offset, C.sizeof(B.GlobalSums),
            B.GlobalSums.EnergyRadComp.offset]
    assert got == want
