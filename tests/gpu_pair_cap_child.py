"""Child of tests/test_gpu_pair_caps.py: the overlapped step of
test_overlapped_step_equals_the_phase_by_phase_step (tests/test_gpu_parity.py) at ng = 48, under
whatever GHIP_PAIR_NEWTON_LDS the parent has put into the environment.  Writes GravAccel and
GravCost to the .npz named on the command line."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from common import Problem, bindings  # noqa: E402


def main(out):
    B = bindings()
    pr = Problem(ng=48, gas=True, periodic=1)
    rng = np.random.default_rng(12)
    old = 0.5 + rng.random(pr.n)
    fp = pr.device()
    fp.set_field(B.F_OLDACC, old)
    for rep in range(2):                     # second repetition: adaptive plans are warm
        pr.device_tree(fp)
        fp.gravity(pr.g_grav(0.0), B.WALK_NEWTON_EWALD)
        fp.density(pr.g_dens())
        fp.update_hmax()
        fp.hydro(pr.g_hydro())
        if rep == 0:
            fp.set_field(B.F_OLDACC, old)    # same inputs for the second repetition
            fp.set_field(B.F_HSML, pr.hsml0)
    fp.gravity_finish(pr.G)
    np.savez(out, acc=fp.get_field(B.F_GRAVACCEL), cost=fp.get_field(B.F_GRAVCOST),
             lds=np.int64(os.environ.get("GHIP_PAIR_NEWTON_LDS", "0")))


if __name__ == "__main__":
    main(sys.argv[1])
