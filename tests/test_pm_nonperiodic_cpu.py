"""CPU checks of tests/pm_nonperiodic_ref.py, the numpy restatement of pm_nonperiodic.c that the device
code is compared with (tests/test_gpu_pm_nonperiodic.py): it has to be right itself before parity with it
means anything.  300 particles uniform in [-1, 1]^3, masses in [0.5, 1.5], PMGRID 16 and 32."""
import ctypes as C

import numpy as np
import pytest

import pm_nonperiodic_ref as R
from common import pkg

G = 43007.1

NEW_SYMBOLS = ("ghip_pm_find_region", "ghip_pm_set_region", "ghip_pm_get_region", "ghip_pm_nonperiodic")


def particles():
    rng = np.random.default_rng(3)
    pos = rng.uniform(-1.0, 1.0, (300, 3))
    mass = rng.uniform(0.5, 1.5, 300)
    return pos, mass


_CACHE = {}


def case(pmgrid):
    if pmgrid not in _CACHE:
        pos, mass = particles()
        reg = R.region(pos, pmgrid)
        _CACHE[pmgrid] = (pos, mass, reg, R.pm_force(pos, mass, reg, G), R.pm_potential(pos, mass, reg, G))
    return _CACHE[pmgrid]


@pytest.mark.parametrize("pmgrid", [16, 32])
def test_long_range_force_against_the_exact_split(pmgrid):
    pos, mass, reg, acc, _ = case(pmgrid)
    want, newton = R.exact_longrange(pos, mass, reg["Asmth"], G)
    err = np.linalg.norm(acc - want, axis=1) / np.linalg.norm(newton, axis=1)
    print("PMGRID %d: median %.3g, 95th percentile %.3g, max %.3g" %
          (pmgrid, np.median(err), np.percentile(err, 95), err.max()))
    assert np.median(err) < 0.01
    assert np.percentile(err, 95) < 0.03


@pytest.mark.parametrize("pmgrid", [16, 32])
def test_potential_against_the_exact_split(pmgrid):
    pos, mass, reg, _, pot = case(pmgrid)
    want = R.exact_longrange_potential(pos, mass, reg["Asmth"], G)
    err = np.abs(pot - want) / np.abs(want)
    print("PMGRID %d: median %.3g, max %.3g" % (pmgrid, np.median(err), err.max()))
    assert np.median(err) < 0.005
    assert err.max() < 0.02


@pytest.mark.parametrize("pmgrid", [16, 32])
def test_momentum_is_conserved(pmgrid):
    pos, mass, reg, acc, _ = case(pmgrid)
    mom = mass[:, None] * acc
    print("PMGRID %d: |sum| / sum|.| = %.3g" % (pmgrid, np.linalg.norm(mom.sum(axis=0)) / np.abs(mom).sum()))
    assert np.linalg.norm(mom.sum(axis=0)) < 1e-9 * np.abs(mom).sum()


@pytest.mark.parametrize("pmgrid", [16, 32])
def test_region_arithmetic_and_cell_range(pmgrid):
    pos, mass, reg, _, _ = case(pmgrid)
    GRID = 2 * pmgrid
    c = R.cells(pos, reg)
    assert c.min() >= 2 and c.max() < GRID // 2 - 2
    assert np.all(R.in_region(pos, reg))
    # :123-159 written out once more, from the extremes
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    ext = max(hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2])
    tms = ext * (2.001 * GRID / float(GRID - 10))
    assert reg["TotalMeshSize"] == tms
    for j in range(3):
        xmin = (lo[j] + hi[j]) / 2 - ext / 2
        assert reg["Xmintot"][j] == xmin and reg["Xmaxtot"][j] == xmin + ext
        corner = xmin - 2.0005 * tms / GRID
        assert reg["Corner"][j] == corner
        assert reg["UpperCorner"][j] == corner + (GRID // 2 - 1) * (tms / GRID)
    assert reg["Asmth"] == 1.25 * tms / GRID and reg["Rcut"] == 4.5 * reg["Asmth"]
    # the mass lies in the lower octant and all of it is on the mesh
    rho = R.deposit(pos, mass, reg)
    assert np.isclose(rho[:pmgrid, :pmgrid, :pmgrid].sum(), mass.sum(), rtol=1e-13)
    assert rho.sum() == rho[:pmgrid, :pmgrid, :pmgrid].sum()


def test_out_of_range_particle_is_refused():
    pos, mass, reg, _, _ = case(16)
    p2 = pos.copy()
    p2[7, 1] = reg["Xmaxtot"][1] + 1e-9 * (reg["Xmaxtot"][1] - reg["Xmintot"][1])
    with pytest.raises(ValueError):
        R.pm_force(p2, mass, reg, G)


def test_libghip_exports_the_non_periodic_mesh():
    L = C.CDLL(pkg.lib_path())
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), "libghip.so does not export %s" % name
