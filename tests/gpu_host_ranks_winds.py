"""Rank program of tests/test_gpu_winds_dd.py::test_two_rank_processes_equal_the_in_process_run: run under
torch.distributed.run, one process per rank, all ranks on GPU 0.

Every rank first holds its shard of the SpawnCase of tests/test_gpu_wind_resident.py with its own sink and wind
tables and runs GHIP_DD_WIND in its WINDS_SPAWN_FORM.  Then every rank holds its shard of the periodic case of tests/test_gpu_wind_resident.py with the wind table of its own
wind particles (ghip_dd_winds_set_table), runs GHIP_DD_GRAVITY, GHIP_DD_DENSITY, GHIP_DD_WIND in its
WINDS_RESIDENT_FORM and then a decomposition in a fresh cube with GHIP_DD_MIGRATE, which carries the rows, through
DomainRank.  WINDS_TRANSPORT=host: the exchanges go through the host's all-gather (gloo); =rccl: through the RCCL
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
    transport = os.environ.get("WINDS_TRANSPORT", "host")
    json_fd = os.dup(1)
    os.dup2(2, 1)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from common import bindings
    import test_gpu_winds_dd as TW
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

    def spawn(shards, ranks, dom):
        sc, T, _, _ = TW._spawn_shards(world, ranks=ranks)
        if dom is not None:
            reps = {rank: dom.wind_spawn(sc.gparams(B), sc.rnd)}
        else:
            reps = dict(enumerate(T.S.run.wind_spawn(sc.gparams(B), sc.rnd)))
        res = {}
        for r in shards:
            fp = T.S.fp[r]
            fp.counts()
            res[r] = dict(rep=reps[r], state=[fp.get_field(f) for f in (B.F_POS, B.F_VEL, B.F_MASS, B.F_HSML, B.F_ID,
                                                                         B.F_TYPE)] + list(fp.dd_winds_table()))
            fp.sinks_clear()
        if dom is None:
            T.close()
        return res

    def run(T, shards, dom):
        T.set_active()
        T.set_gas("set_wind_rad_accel", ra0)
        T.set_tables()
        if dom is not None:
            per = {T.rank: dom.winds_feedback(c.gparams())}
            dom.redistribute(B.DecompParams(0, 0, 1, 0))
        else:
            per = dict(enumerate(T.S.run.winds_feedback(c.gparams())))
            T.S.run.redistribute(B.DecompParams(0, 0, 1, 0))
        res = {}
        for r in shards:
            fp = T.S.fp[r]
            fp.counts()
            idx, rows = fp.dd_winds_table()
            res[r] = dict(out={k: np.asarray(v) for k, v in per[r].items()}, table=[idx, rows],
                          resident=[fp.get_field(f) for f in (B.F_POS, B.F_HSML, B.F_MASS, B.F_VEL, B.F_ID, B.F_TYPE)] +
                          [fp.wind_injected(), fp.wind_rad_accel()], bytes=fp.dd_bytes_sent(B.WIND_OP),
                          migrated=[fp.dd_info()["migrated_out"], fp.dd_info()["migrated_in"]])
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
        born = spawn([rank], dict(contexts=paths, dom=dom, rank=rank), dom)[rank]
        T = TW.Shards(c, world, active=TW._active(c), contexts=paths, dom=dom, rank=rank)
        res = run(T, [rank], dom)[rank]
        res["born"] = born
    except Exception as e:   # noqa: BLE001
        ok, err = False, repr(e)
    blob = [None] * world
    dist.all_gather_object(blob, (ok, err, res))
    if rank == 0:
        ok = all(b[0] for b in blob)
        out = {"ok": ok, "error": "; ".join(b[1] for b in blob if b[1]), "transport": transport, "rccl_library": lib}
        if ok:
            born = spawn(range(world), None, None)
            T = TW.Shards(c, world, active=TW._active(c))
            here = run(T, range(world), None)
            T.close()
            theirs = [b[2] for b in blob]
            out["iterations"] = int(theirs[0]["out"]["iterations"])
            out["outputs_equal"] = all(np.array_equal(theirs[r]["out"][k], here[r]["out"][k])
                                       for r in range(world) for k in here[r]["out"])
            out["tables_equal"] = all(np.array_equal(a, b) for r in range(world)
                                      for a, b in zip(theirs[r]["table"], here[r]["table"]))
            out["resident_equal"] = all(a.shape == b.shape and np.array_equal(a, b) for r in range(world)
                                        for a, b in zip(theirs[r]["resident"], here[r]["resident"]))
            out["spawn_equal"] = all(theirs[r]["born"]["rep"] == born[r]["rep"] and
                                     all(a.shape == b.shape and np.array_equal(a, b)
                                         for a, b in zip(theirs[r]["born"]["state"], born[r]["state"]))
                                     for r in range(world))
            out["spawned"] = [int(t["born"]["rep"]["spawned"]) for t in theirs]
            out["tot_spawned"] = [int(t["born"]["rep"]["tot_spawned"]) for t in theirs]
            out["rows"] = [int(len(t["table"][0])) for t in theirs]
            out["migrated"] = [[int(v) for v in t["migrated"]] for t in theirs]
            out["bytes_wind"] = [int(t["bytes"]) for t in theirs]
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    for p in paths:
        p.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
