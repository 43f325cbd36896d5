"""How many Newtonian wavefronts a Newton + Ewald pair admits per SIMD (the dynamic-LDS cap of
launch_walk, chosen by pair_balance among 6 KB / 8 KB / 10 KB = 6 / 5 / 4 per SIMD) is scheduling
only: a launch's sums must not depend on it.  Each setting is pinned with GHIP_PAIR_NEWTON_LDS in a
fresh process (the variable is read once per process) that runs the overlapped step at ng = 48, the
smallest of the parity sets with enough buckets (>= 1 536) for the cap to apply.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAPS = (6144, 8192, 10240)


def test_pair_sums_do_not_depend_on_the_newtonian_cap(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = os.path.join(root, "tests", "gpu_pair_cap_child.py")
    res = []
    for cap in CAPS:                       # one after the other; the first failure ends the test
        out = str(tmp_path / ("cap%d.npz" % cap))
        env = dict(os.environ, GHIP_PAIR_NEWTON_LDS=str(cap))
        r = subprocess.run([sys.executable, child, out], cwd=root, env=env, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, "cap %d: exit %d\n%s" % (cap, r.returncode, r.stderr[-3000:])
        d = np.load(out)
        assert int(d["lds"]) == cap
        res.append((d["acc"], d["cost"]))
    acc0, cost0 = res[0]
    assert cost0.sum() > 0 and np.abs(acc0).max() > 0
    for cap, (acc, cost) in zip(CAPS[1:], res[1:]):
        assert np.array_equal(cost, cost0), cap
        # (the bound of test_overlapped_step_equals_the_phase_by_phase_step: the per-bucket wavefront
        # split, hence the grouping of the partial sums, may differ between runs)
        d = np.abs(acc - acc0).max()
        print("cap %d against %d: max |d acc| = %.3e of %.3e" % (cap, CAPS[0], d, np.abs(acc0).max()))
        assert d <= 1e-13 * np.abs(acc0).max(), cap
