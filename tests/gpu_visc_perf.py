"""Development aid: what the viscosity mode (ghip_set_viscosity, time_dependent, varying alpha) costs the
hydro phase -- ms_hydro of ghip_get_stats with the mode on against the mode off, alternating in one
process at converged smoothing lengths.  python tests/gpu_visc_perf.py [ng] [reps]   (c2: ng = 64)"""
import sys

import numpy as np

from common import Problem, bindings


def main():
    ng = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    B = bindings()
    pr = Problem(ng=ng, gas=True, periodic=1)
    fp = pr.device()
    pr.device_tree(fp)
    fp.density(pr.g_dens())
    fp.update_hmax()
    V = B.ViscParams(time_dependent=1, ArtBulkViscConst=0.8, AlphaMin=0.1, ViscSource=1.0, DecayTime=1.0,
                     dtalpha_comoving_div=1.0)
    alpha = 0.1 + 0.7 * np.random.default_rng(7).random(pr.ngas)
    fp.hydro(pr.g_hydro())               # warm-up of both instantiations
    fp.set_viscosity(V)
    fp.visc_set_alpha(alpha)
    fp.hydro(pr.g_hydro())
    ms = {"off": [], "on": []}
    for _ in range(reps):
        for mode in ("off", "on"):
            fp.set_viscosity(V if mode == "on" else None)
            fp.hydro(pr.g_hydro())
            s = fp.stats()
            ms[mode].append(s["ms_hydro"])
    off, on = float(np.median(ms["off"])), float(np.median(ms["on"]))
    print("ng=%d gas=%d pairs=%d  ms_hydro off %.3f (%.3f .. %.3f)  on %.3f (%.3f .. %.3f)  on/off %.4f" %
          (ng, pr.ngas, s["hydro_pairs"], off, min(ms["off"]), max(ms["off"]), on, min(ms["on"]), max(ms["on"]),
           on / off))


if __name__ == "__main__":
    main()
