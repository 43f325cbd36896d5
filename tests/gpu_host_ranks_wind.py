"""Rank program of tests/test_gpu_wind_dd.py::test_two_rank_processes_equal_the_in_process_run: run under
torch.distributed.run, one process per rank, all ranks on GPU 0.

Every rank holds its shard of the periodic WindCase of tests/test_gpu_wind.py (the key ranges of ShardSet), runs
GHIP_DD_GRAVITY, GHIP_DD_DENSITY and GHIP_DD_WIND (the whole loop) through DomainRank, and reads its outputs and
resident fields.  WIND_TRANSPORT=host: the exchanges go through the host's all-gather (gloo); =rccl: through the RCCL
entry points (GHIP_RCCL_LIB selects tests/mock_rccl).  Rank 0 gathers the results, repeats the run with both shards
in its own process and compares bit for bit; prints one JSON line."""
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    transport = os.environ.get("WIND_TRANSPORT", "host")
    json_fd = os.dup(1)
    os.dup2(2, 1)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from common import bindings
    import test_gpu_wind_dd as TW
    B = bindings()
    S = importlib.import_module("gadget-leicester_amd.sharded")
    c = TW._case(1)
    ra0 = np.random.default_rng(6).standard_normal((c.pr.ngas, 3))

    def bcast(obj):
        box = [obj]
        dist.broadcast_object_list(box, src=0)
        return box[0]

    def allgather(data):
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        out = torch.empty(world * len(data), dtype=torch.uint8)
        dist.all_gather_into_tensor(out, t)
        return out.numpy().tobytes()

    def run(T, shards):
        T.set_active()
        T.set_gas("set_wind_rad_accel", ra0)
        out, per = T.loop()
        res = {}
        for r in shards:
            fp = T.S.fp[r]
            res[r] = dict(out={k: np.asarray(v) for k, v in per[r].items()},
                          resident=[fp.get_field(f) for f in (B.F_POS, B.F_HSML, B.F_MASS, B.F_VEL, B.F_TIMEBIN)] +
                          [fp.wind_injected(), fp.wind_rad_accel()], bytes=fp.dd_bytes_sent(B.WIND_OP))
        return res

    ok, err, res, lib = True, "", None, ""
    paths = [B.ForcePath(0) for _ in range(world)]
    try:
        for r, p in enumerate(paths):
            if r != rank:
                p.dd_init(r, world)           # (a stand-in: ShardSet loads it, nothing runs on it)
        if transport == "rccl":
            dom = S.DomainRank(paths[rank], rank, world, bcast, transport="rccl")
            lib = B.dd_rccl_library()
        else:
            dom = S.DomainRank(paths[rank], rank, world, transport="host", allgather=allgather)
        T = TW.DdWind(c, world, contexts=paths, dom=dom, rank=rank)
        res = run(T, [rank])[rank]
    except Exception as e:   # noqa: BLE001
        ok, err = False, repr(e)
    blob = [None] * world
    dist.all_gather_object(blob, (ok, err, res))
    if rank == 0:
        ok = all(b[0] for b in blob)
        out = {"ok": ok, "error": "; ".join(b[1] for b in blob if b[1]), "transport": transport, "rccl_library": lib}
        if ok:
            T = TW.DdWind(c, world)
            here = run(T, range(world))
            T.close()
            theirs = [b[2] for b in blob]
            out["iterations"] = int(theirs[0]["out"]["iterations"])
            out["outputs_equal"] = all(np.array_equal(theirs[r]["out"][k], here[r]["out"][k])
                                       for r in range(world) for k in here[r]["out"])
            out["resident_equal"] = all(np.array_equal(a, b) for r in range(world)
                                        for a, b in zip(theirs[r]["resident"], here[r]["resident"]))
            out["bytes_wind"] = [int(t["bytes"]) for t in theirs]
            out["bytes_equal_in_process"] = all(int(theirs[r]["bytes"]) == int(here[r]["bytes"]) for r in range(world))
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    for p in paths:
        p.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
