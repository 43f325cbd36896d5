"""Rank program of tests/test_gpu_pm_nonperiodic.py::test_two_rank_processes_region_force_and_refusal: run under
torch.distributed.run, one process per rank, all ranks on GPU 0.

Every rank keeps the particles it was dealt (global index modulo the number of ranks) of the seeded
300-particle set.  DomainRank.pm_region (GHIP_DD_PM_REGION) and DomainRank.pm_nonperiodic
(GHIP_DD_PM_NONPERIODIC) run with every exchange staged through the host's all-gather (gloo).  Then one
particle of rank 1 steps outside the region: every rank must get GHIP_EREGION and keep its GRAVPM; after a new
region the call succeeds.  Rank 0 gathers and compares with tests/pm_nonperiodic_ref.py; prints one JSON line."""
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

PMGRID, G, SENTINEL = 16, 43007.1, -7.25


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    json_fd = os.dup(1)
    os.dup2(2, 1)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from common import O, bindings
    import pm_nonperiodic_ref as R
    B = bindings()
    S = importlib.import_module("gadget-leicester_amd.sharded")

    rng = np.random.default_rng(3)
    pos, mass = rng.uniform(-1.0, 1.0, (300, 3)), rng.uniform(0.5, 1.5, 300)
    n = len(pos)
    reg0 = R.region(pos, PMGRID)
    moved = pos.copy()
    stray = 1 + world * 20                      # a particle of rank 1
    moved[stray, 2] = reg0["Xmaxtot"][2] + 1e-9 * (reg0["Xmaxtot"][2] - reg0["Xmintot"][2])
    mine = np.arange(rank, n, world)

    def allgather(data):
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        out = torch.empty(world * len(data), dtype=torch.uint8)
        dist.all_gather_into_tensor(out, t)
        return out.numpy().tobytes()

    ok, err, res = True, "", {}
    fp = B.ForcePath(0)
    try:
        fp.set_counts(len(mine), 0)
        fp.set_field(B.F_POS, pos[mine])
        fp.set_field(B.F_MASS, mass[mine])
        dom = S.DomainRank(fp, rank, world, transport="host", allgather=allgather)
        corner, center, length = O.domain_extent(pos)
        fp.dd_set_domain(corner, center, length, np.full(6, 0.01))
        prm = B.PmnpParams(PMGRID, G, 0, 0.0, 0.0, 0.0)
        res["region"] = {k: np.asarray(v).tolist() for k, v in dom.pm_region(PMGRID).asdict().items()}
        dom.pm_nonperiodic(prm)
        res["force"] = fp.get_field(B.F_GRAVPM)
        res["bytes"] = fp.dd_bytes_sent(B.DD_PM_NONPERIODIC)
        # the stray particle: every rank is refused, nothing is written
        fp.set_field(B.F_POS, moved[mine])
        sentinel = np.full((len(mine), 3), SENTINEL)
        fp.set_field(B.F_GRAVPM, sentinel)
        try:
            dom.pm_nonperiodic(prm)
            res["stray_code"] = 0
        except B.GhipError as e:
            res["stray_code"] = e.code
        res["sentinel_intact"] = bool(np.array_equal(fp.get_field(B.F_GRAVPM), sentinel))
        dom.pm_region(PMGRID)
        dom.pm_nonperiodic(prm)
        res["force2"] = fp.get_field(B.F_GRAVPM)
    except Exception as e:   # noqa: BLE001
        ok, err = False, repr(e)
    blob = [None] * world
    dist.all_gather_object(blob, (ok, err, res))
    if rank == 0:
        ok = all(b[0] for b in blob)
        out = {"ok": ok, "error": "; ".join(b[1] for b in blob if b[1])}
        if ok:
            def same(d):
                return all(np.asarray(d[k], np.float64).tobytes() == np.asarray(reg0[k], np.float64).tobytes()
                           for k in ("Xmintot", "Xmaxtot", "Corner", "UpperCorner", "TotalMeshSize", "Asmth", "Rcut"))

            def glob(key):
                a = np.zeros((n, 3))
                for r, b in enumerate(blob):
                    a[np.arange(r, n, world)] = b[2][key]
                return a
            out["region_equal_on_ranks"] = all(b[2]["region"] == blob[0][2]["region"] for b in blob)
            out["region_equal_restatement"] = bool(same(blob[0][2]["region"]))
            want = R.pm_force(pos, mass, reg0, G)
            out["rel_force"] = float(np.abs(glob("force") - want).max() / np.abs(want).max())
            out["bytes"] = int(blob[0][2]["bytes"])
            out["stray_codes"] = [int(b[2]["stray_code"]) for b in blob]
            out["sentinels_intact"] = all(b[2]["sentinel_intact"] for b in blob)
            want2 = R.pm_force(moved, mass, R.region(moved, PMGRID), G)
            out["rel_force_after_region"] = float(np.abs(glob("force2") - want2).max() / np.abs(want2).max())
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    fp.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
