"""Register budget of the SPH bucket kernels (ghip_sph.hip).  k_density<TG> and
k_hydro<TG[, HydV]> run on one bucket sweep (d_sph_sweep) that takes what differs between them as
callables; those must dissolve into the kernels: no scratch, and no more vector registers than the
granule of 8 the kernels had with their own loops -- 128 for k_hydro (four wavefronts per SIMD, the
slot the walks leave it) and 112 for k_density.  The numbers are read from the compiler's own summary
of each kernel in the gfx950 listing; nothing else of the assembly is looked at.
"""
import os
import re
import shutil
import subprocess

import pytest

from common import pkg

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
TGS = (8, 16, 32, 64)


@pytest.fixture(scope="module")
def sph_kernels(tmp_path_factory):
    """{(kernel, TG, visc): {"NumVgprs": .., "ScratchSize": ..}}"""
    if HIPCC is None:
        pytest.skip("hipcc not found")
    src = os.path.join(pkg.PKG_DIR, "csrc", "ghip_sph.hip")
    out = str(tmp_path_factory.mktemp("listing") / "sph.s")
    subprocess.run([HIPCC] + pkg.HIPCC_FLAGS + ["-S", "--cuda-device-only", "-o", out, src],
                   check=True, stderr=subprocess.DEVNULL)
    res, cur = {}, None
    for line in open(out):
        # _Z9k_densityILi16EEv...  _Z7k_hydroILi16EJEEv...  _Z7k_hydroILi16EJ4HydVEEv...
        m = re.match(r"^_Z\d+k_(density|hydro)ILi(\d+)E(?:J(4HydV)?E)?Ev\S*:", line)
        if m:
            cur = res.setdefault((m.group(1), int(m.group(2)), m.group(3) is not None), {})
            continue
        m = re.match(r"^; (NumVgprs|ScratchSize): (\d+)\s*$", line)
        if m and cur is not None and m.group(1) not in cur:
            cur[m.group(1)] = int(m.group(2))
            if len(cur) == 2:
                cur = None
    return res


def test_every_sph_instantiation_is_in_the_listing(sph_kernels):
    want = [("density", tg, False) for tg in TGS] + [("hydro", tg, v) for tg in TGS for v in (False, True)]
    assert sorted(sph_kernels) == sorted(want)
    for k in sph_kernels.values():
        assert sorted(k) == ["NumVgprs", "ScratchSize"]


@pytest.mark.parametrize("tg", TGS)
def test_density_fits_112_registers_without_scratch(sph_kernels, tg):
    k = sph_kernels[("density", tg, False)]
    print(tg, k)
    assert k["ScratchSize"] == 0
    assert k["NumVgprs"] <= 112


@pytest.mark.parametrize("tg", TGS)
@pytest.mark.parametrize("visc", [False, True])
def test_hydro_fits_128_registers_without_scratch(sph_kernels, tg, visc):
    k = sph_kernels[("hydro", tg, visc)]
    print(tg, visc, k)
    assert k["ScratchSize"] == 0
    assert k["NumVgprs"] <= 128
