"""Rank program of tests/test_gpu_sink_accretion_dd.py::test_two_rank_processes_equal_the_in_process_run: run under
torch.distributed.run, one process per rank, all ranks on GPU 0.

Every rank holds its shard of the stock sink problem (the key ranges of ShardSet) with the rows of its own sinks in
its sink table, and runs GHIP_DD_GRAVITY, GHIP_DD_DENSITY, GHIP_DD_SINK_DENSITY and GHIP_DD_BH_SWALLOW in their
resident form and, after a drift that sends one sink of each rank to the other, GHIP_DD_MIGRATE -- all through
DomainRank (rank_sequence of the test module).  SINKS_TRANSPORT=host: the exchanges go through the host's
all-gather (gloo); =rccl: through the RCCL entry points (GHIP_RCCL_LIB selects tests/mock_rccl).  Rank 0 gathers
the results, repeats the run with both shards in its own process and compares bit for bit; prints one JSON line."""
import importlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    transport = os.environ.get("SINKS_TRANSPORT", "host")
    json_fd = os.dup(1)
    os.dup2(2, 1)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from common import bindings
    import test_gpu_sink_accretion_dd as TS
    B = bindings()
    S = importlib.import_module("gadget-leicester_amd.sharded")
    sp, rows0, acc = TS.rank_case()

    def bcast(obj):
        box = [obj]
        dist.broadcast_object_list(box, src=0)
        return box[0]

    def allgather(data):
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        out = torch.empty(world * len(data), dtype=torch.uint8)
        dist.all_gather_into_tensor(out, t)
        return out.numpy().tobytes()

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
        run = TS.Run(sp, world, rows0, contexts=paths)
        before = len(paths[rank].sinks_table()[0])
        res = TS.rank_sequence(run, [rank], acc, dom=dom)[rank]
        res["before"] = before
    except Exception as e:   # noqa: BLE001
        ok, err = False, repr(e)
    blob = [None] * world
    dist.all_gather_object(blob, (ok, err, res))
    if rank == 0:
        ok = all(b[0] for b in blob)
        out = {"ok": ok, "error": "; ".join(b[1] for b in blob if b[1]), "transport": transport, "rccl_library": lib}
        if ok:
            run = TS.Run(sp, world, rows0)
            here = TS.rank_sequence(run, list(range(world)), acc)
            run.close()
            theirs = [b[2] for b in blob]
            out["iterations"] = int(theirs[0]["it"])
            out["equal"] = [TS.rank_results_equal(theirs[r], here[r]) for r in range(world)]
            out["swallowed"] = [int(t["rep"]["counts"].sum()) for t in theirs]
            # one sink left and one arrived on every rank: the arrival's ID was not in the table before
            out["rows_arrived"] = [int(len(t["ids"]) - t["before"] + 1) for t in theirs]
            out["bytes"] = [t["bytes"] for t in theirs]
            out["bytes_equal_in_process"] = all(theirs[r]["bytes"] == here[r]["bytes"] for r in range(world))
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    for p in paths:
        p.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
