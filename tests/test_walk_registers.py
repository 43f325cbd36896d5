"""Register budget of the gravity walks (ghip_walk.h).  How many wavefronts of
the Newtonian walk share a SIMD with the Ewald walk and the SPH kernels is decided by the vector
registers per wavefront in granules of 8: 5 * 56 + 112 + 112 fits the 512 of a SIMD lane,
5 * 64 + 112 + 112 does not.  The numbers are read from the compiler's own summary of each kernel in
the gfx950 listing; nothing else of the assembly is looked at.
"""
import os
import re
import shutil
import subprocess

import pytest

from common import pkg

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def walk_kernels(tmp_path_factory):
    """{(mode, periodic, unequal): {"NumVgprs": .., "ScratchSize": .., "TotalNumSgprs": ..}}"""
    if HIPCC is None:
        pytest.skip("hipcc not found")
    src = os.path.join(pkg.PKG_DIR, "csrc", "ghip_gravity.hip")
    out = str(tmp_path_factory.mktemp("listing") / "g.s")
    subprocess.run([HIPCC] + pkg.HIPCC_FLAGS + ["-S", "--cuda-device-only", "-o", out, src],
                   check=True, stderr=subprocess.DEVNULL)
    res, cur = {}, None
    for line in open(out):
        m = re.match(r"^_Z11k_grav_walkILi(\d)ELb(\d)ELb(\d)E\S*:", line)
        if m:
            cur = res.setdefault(tuple(int(g) for g in m.groups()), {})
            continue
        m = re.match(r"^; (NumVgprs|ScratchSize|TotalNumSgprs): (\d+)\s*$", line)
        if m and cur is not None and m.group(1) not in cur:
            cur[m.group(1)] = int(m.group(2))
            if len(cur) == 3:
                cur = None
    return res


def test_every_walk_instantiation_is_in_the_listing(walk_kernels):
    assert sorted(walk_kernels) == [(m, p, u) for m in (0, 1, 2) for p in (0, 1) for u in (0, 1)]
    for k in walk_kernels.values():
        assert sorted(k) == ["NumVgprs", "ScratchSize", "TotalNumSgprs"]


@pytest.mark.parametrize("mode", [0, 1])        # GHIP_WALK_NEWTON, GHIP_WALK_SHORTRANGE
@pytest.mark.parametrize("periodic", [0, 1])
@pytest.mark.parametrize("unequal", [0, 1])
def test_newtonian_and_short_range_walks_fit_56_registers(walk_kernels, mode, periodic, unequal):
    k = walk_kernels[(mode, periodic, unequal)]
    print(mode, periodic, unequal, k)
    assert k["NumVgprs"] <= 56
    assert k["ScratchSize"] == 0
    # no more scalar registers than before the softened branch became a call (78: an allocation of 80)
    assert k["TotalNumSgprs"] <= 78


@pytest.mark.parametrize("periodic", [0, 1])
@pytest.mark.parametrize("brick", [0, 1])
def test_ewald_walk_fits_112_registers(walk_kernels, periodic, brick):
    k = walk_kernels[(2, periodic, brick)]
    print(periodic, brick, k)
    assert k["NumVgprs"] <= 112
    assert k["ScratchSize"] == 0
