"""The bucket widths of the SPH kernels other than the default: GHIP_SPH_TG = 8, 32, 64 select the
k_density<TG> / k_hydro<TG[, HydV]> instantiations that no other test runs (the variable is read once
per process, the default is 16).  All of them are the one bucket sweep d_sph_sweep, so each is held to
what the default is held to: the oracle, as in test_density_and_hydro_parity (tests/test_gpu_parity.py),
and the all-pairs reference tests/visc_ref.py for the time-dependent viscosity, as in
tests/test_gpu_visc.py.  Each width runs in a fresh process (tests/gpu_sph_tg_child.py), one after the
other.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_sph_tg_child as child
import visc_ref as VR
from common import relerr

pytestmark = pytest.mark.gpu

TOL = 1e-11                          # the bound of tests/test_gpu_parity.py and tests/test_gpu_visc.py


@pytest.fixture(scope="module")
def oracle_sph():
    """the oracle's density and hydro of the child's problem, once for all widths"""
    pr = child.problem()
    T = pr.oracle_tree()
    act = np.arange(pr.ngas, dtype=np.int32)
    od = T.density(pr.o_dens(), act, pr.velpred, pr.entropy, pr.dtentropy, pr.timebin, pr.ti_begstep, pr.hsml0)
    T.update_hmax(act, od["hsml"], od["divvel"])
    oh = T.hydro(pr.o_hydro(), act, pr.velpred, od["hsml"], od["density"], od["pressure"], od["dhsmlfac"],
                 od["divvel"], od["curlvel"], pr.timebin)
    return pr, od, oh


@pytest.mark.parametrize("tg", [8, 32, 64])
def test_bucket_width_against_the_oracle_and_the_all_pairs_reference(oracle_sph, tmp_path, tg):
    pr, od, oh = oracle_sph
    ng = pr.ngas
    assert ng == 1000              # 16 to 125 buckets: several wavefronts per bucket; 32 and 64 leave a ragged one
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / ("tg%d.npz" % tg))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "gpu_sph_tg_child.py"), out], cwd=root,
                       env=dict(os.environ, GHIP_SPH_TG=str(tg)), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "GHIP_SPH_TG=%d: exit %d\n%s" % (tg, r.returncode, r.stderr[-3000:])
    d = np.load(out)
    assert int(d["tg"]) == tg
    # density: as test_density_and_hydro_parity
    assert int(d["dens_iterations"]) == od["iterations"]
    assert int(d["dens_neighbours"]) == od["ngb_visits"]
    for name in ("hsml", "numngb", "density", "dhsmlfac", "pressure"):
        e = relerr(d[name], od[name][:ng])
        print(tg, name, e)
        assert e < TOL, name
    for name in ("divvel", "curlvel"):
        e = np.abs(d[name] - od[name][:ng]).max() / np.abs(od[name][:ng]).max()
        print(tg, name, e)
        assert e < TOL, name
    # hydro, the default kernels
    assert int(d["hydro_pairs"]) == oh["npairs"]
    for name in ("hydroaccel", "dtentropy"):
        e = np.abs(d[name] - oh[name][:ng]).max() / np.abs(oh[name]).max()
        print(tg, name, e)
        assert e < TOL, name
    e = relerr(d["maxsignalvel"], oh["maxsignalvel"][:ng])
    print(tg, "maxsignalvel", e)
    assert e < TOL
    # hydro with varying alpha: as test_varying_alpha_against_the_all_pairs_reference, on the device's own density
    V = VR.params(**child.VISC)
    alpha = child.alpha(pr)
    ref = VR.hydro(pr, d, alpha, V, pr.g_hydro())
    assert int(d["visc_hydro_pairs"]) == ref["npairs"]
    for name in ("hydroaccel", "dtentropy", "maxsignalvel"):
        e = np.abs(d["visc_" + name] - ref[name]).max() / np.abs(ref[name]).max()
        print(tg, "visc", name, e)
        assert e < TOL, name
    assert np.abs(ref["hydroaccel"] - oh["hydroaccel"][:ng]).max() > 1e-6 * np.abs(oh["hydroaccel"]).max()
    want = VR.dtalpha(d["pressure"], d["density"], d["hsml"], d["divvel"], d["curlvel"], d["visc_maxsignalvel"],
                      alpha, V, fac_mu=1.0, comoving=0)
    assert np.abs(d["visc_dtalpha"] - want).max() < 1e-13 * np.abs(want).max()
