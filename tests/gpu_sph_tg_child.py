"""Child of tests/test_gpu_sph_tg.py: density, update_hmax and hydro, then hydro once more in the
time-dependent viscosity mode, at whatever bucket width GHIP_SPH_TG the parent has put into the
environment (the library reads it once per process).  1000 gas particles: the last bucket is ragged
(at every width but 8), the launch has fewer workgroups than the SPH kernels want, so several
wavefronts share a bucket and deal its batches among them, and the gas tree has leaves of more than
one staging round as well as lone-particle elements.  Writes the fields and the counts to the .npz named on the
command line."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import visc_ref as VR  # noqa: E402
from common import Problem, bindings  # noqa: E402

VISC = dict(time_dependent=1, ArtBulkViscConst=0.8, dtalpha_comoving_div=1.9 * 0.37 * 0.37)   # tests/test_gpu_visc.py
DENS = (("hsml", "F_HSML"), ("numngb", "F_NUMNGB"), ("density", "F_DENSITY"), ("dhsmlfac", "F_DHSMLFAC"),
        ("pressure", "F_PRESSURE"), ("divvel", "F_DIVVEL"), ("curlvel", "F_CURLVEL"))
HYDRO = (("hydroaccel", "F_HYDROACCEL"), ("dtentropy", "F_DTENTROPY"), ("maxsignalvel", "F_MAXSIGNALVEL"))


def problem():
    """the parent builds the same one for the references"""
    pr = Problem(ng=10, gas=True, periodic=1)
    rng = np.random.default_rng(31)
    pr.hsml0[:pr.ngas] *= 0.6 + 0.8 * rng.random(pr.ngas)      # targets of one bucket differ in radius
    return pr


def alpha(pr):
    return 0.1 + 0.7 * np.random.default_rng(7).random(pr.ngas)


def main(out):
    B = bindings()
    pr = problem()
    ng = pr.ngas
    fp = pr.device()
    pr.device_tree(fp)
    res = {"tg": np.int64(os.environ.get("GHIP_SPH_TG", "16"))}
    fp.density(pr.g_dens())
    st = fp.stats()
    res["dens_neighbours"], res["dens_iterations"] = np.int64(st["dens_neighbours"]), np.int64(st["dens_iterations"])
    for k, f in DENS:
        res[k] = np.asarray(fp.get_field(getattr(B, f)), np.float64)[:ng].copy()
    fp.update_hmax()
    fp.hydro(pr.g_hydro())
    res["hydro_pairs"] = np.int64(fp.stats()["hydro_pairs"])
    for k, f in HYDRO:
        res[k] = fp.get_field(getattr(B, f)).copy()
    P = B.ViscParams()
    for k, v in VR.params(**VISC).items():
        setattr(P, k, v)
    fp.set_viscosity(P)
    fp.visc_set_alpha(alpha(pr))
    fp.hydro(pr.g_hydro())
    res["visc_hydro_pairs"] = np.int64(fp.stats()["hydro_pairs"])
    for k, f in HYDRO:
        res["visc_" + k] = fp.get_field(getattr(B, f)).copy()
    res["visc_dtalpha"] = fp.visc_get()[1].copy()
    fp.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
