"""compute_potential() and compute_global_quantities_of_system() with NTask = 2: one process per rank, both
on this box's one GPU, 536 / 264-byte records, exchanges through the host's all-gather (gloo).
tests/gpu_host_ranks_potential.py is the rank program; rank 0 gathers the records and checks them against
tests/potential_ref.py on the exported tree of a single-context build of all particles."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
TOL_POT = 1e-11   # the shard tolerance (tests/test_gpu_dd.py)
TOL_SYS = 1e-12   # the sums' tolerance (tests/test_gpu_potential.py)


def test_dropin_potential_and_energy_statistics_on_two_ranks():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "tests", "gpu_host_ranks_potential.py")]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    print(lines[0])
    assert out["ok"], out
    # P[].p.Potential of both ranks' records against the reference walk; every other byte unchanged
    assert out["rel_potential"] < TOL_POT, out
    assert out["potential_written"] and out["untouched_equal"], out
    # SysState: the same bytes on both ranks, the reference's sums
    assert out["sysstate_identical"] and out["rad_members_kept"] and out["energy_pot_nonzero"], out
    assert out["rel_sysstate"] < TOL_SYS, out
    assert out["exported"] > 0 and out["exported_drifted"] > 0
    # the second call: particles behind Ti_Current were drifted on the device
    assert out["drifted"] > 10 and out["drift_matters"] > 1e-9, out
    assert out["rel_potential_drifted"] < TOL_POT, out
