"""Rank program of tests/test_gpu_decomp.py::test_two_rank_processes_redistribute_...: run under
torch.distributed.run, one process per rank, all ranks on GPU 0.

Every rank keeps the particles it was DEALT (global index modulo the number of ranks: where a reader of a
snapshot would leave them), with seeded GravCost / TimeBin, under the default key ranges of ghip_dd_init.  It
never forms a key and never sees another rank's particles: DomainRank.redistribute (GHIP_DD_DECOMPOSE with
use_work and find_extent, then GHIP_DD_MIGRATE) finds the cube and the ranges and moves the particles, then
GHIP_DD_GRAVITY runs on them.  DECOMP_TRANSPORT=host: the exchanges go through the host's all-gather (gloo);
=rccl: through the RCCL entry points (GHIP_RCCL_LIB selects tests/mock_rccl).  Rank 0 gathers the results,
repeats the run with both shards in its own process and against tests/decomp_ref.py; prints one JSON line."""
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
    transport = os.environ.get("DECOMP_TRANSPORT", "host")
    json_fd = os.dup(1)
    os.dup2(2, 1)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from common import Problem, bindings, relerr
    import decomp_ref as DR
    import test_gpu_decomp as TD
    B = bindings()
    S = importlib.import_module("gadget-leicester_amd.sharded")

    pr = Problem(ng=12, gas=True, periodic=0)
    n, ng = pr.n, pr.ngas
    cost, tbin = TD.seeded_work(n, 13)
    prm = B.DecompParams(0, 1, 1, 0)
    # a cube that holds the particles and is NOT their extent (a stale one): find_extent replaces it
    stale = (pr.extent[0] - 0.5 * pr.extent[2], pr.extent[1], 2.0 * pr.extent[2])

    def shard_of(fp, gid, r, nranks):
        ngl = int((gid < ng).sum())
        fp.set_counts(len(gid), ngl)
        fp.set_field(B.F_POS, pr.ic["pos"][gid])
        fp.set_field(B.F_VEL, pr.ic["vel"][gid])
        fp.set_field(B.F_MASS, pr.ic["mass"][gid])
        fp.set_field(B.F_TYPE, pr.ic["type"][gid])
        fp.set_field(B.F_HSML, pr.hsml0[gid])
        fp.set_field(B.F_TIMEBIN, tbin[gid])
        fp.set_field(B.F_TI_BEGSTEP, pr.ti_begstep[gid])
        fp.set_field(B.F_OLDACC, np.zeros(len(gid)))
        fp.set_field(B.F_GRAVCOST, cost[gid])
        fp.set_field(B.F_ID, gid.astype(np.int32))
        fp.set_field(B.F_VELPRED, pr.velpred[gid[:ngl]])
        fp.set_field(B.F_ENTROPY, pr.entropy[gid[:ngl]])
        fp.set_field(B.F_DTENTROPY, pr.dtentropy[gid[:ngl]])

    def dealt(r, nranks):
        mine = np.arange(r, n, nranks)
        return np.concatenate([mine[mine < ng], mine[mine >= ng]])

    def results(fp):
        fp.counts()
        return (fp.get_field(B.F_ID).astype(np.int64), fp.get_field(B.F_GRAVCOST), fp.get_field(B.F_GRAVACCEL),
                fp.dd_get_splits(), fp.dd_get_domain(), fp.dd_bytes_sent(B.DD_DECOMPOSE))

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
    fp = B.ForcePath(0)
    try:
        shard_of(fp, dealt(rank, world), rank, world)
        if transport == "rccl":
            dom = S.DomainRank(fp, rank, world, bcast, transport="rccl")
            lib = B.dd_rccl_library()
        else:
            dom = S.DomainRank(fp, rank, world, transport="host", allgather=allgather)
        fp.dd_set_domain(stale[0], stale[1], stale[2], pr.force_soft)
        dom.redistribute(prm)
        dom.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
        res = results(fp)
    except Exception as e:   # noqa: BLE001
        ok, err = False, repr(e)
    blob = [None] * world
    dist.all_gather_object(blob, (ok, err, res))
    if rank == 0:
        ok = all(b[0] for b in blob)
        out = {"ok": ok, "error": "; ".join(b[1] for b in blob if b[1]), "transport": transport,
               "rccl_library": lib}
        if ok:
            # the same run with both shards in this process
            paths = [B.ForcePath(0) for _ in range(world)]
            for r, p in enumerate(paths):
                shard_of(p, dealt(r, world), r, world)
                p.dd_init(r, world)
                p.dd_set_domain(stale[0], stale[1], stale[2], pr.force_soft)
            run = S.DomainShards(paths)
            run.redistribute(prm)
            run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
            here = [results(p) for p in paths]
            for p in paths:
                p.close()
            ref_splits, ref_dom, keys = DR.decompose(pr.ic["pos"], world, 0, cost, tbin)

            def glob(rs):
                gc, ga = np.zeros(n, np.int64), np.zeros((n, 3))
                for gid, c, a, *_ in rs:
                    gc[gid], ga[gid] = c, a
                return gc, ga
            theirs = [b[2] for b in blob]
            gc_r, ga_r = glob(theirs)
            gc_h, ga_h = glob(here)
            ids = np.concatenate([t[0] for t in theirs])
            sp = theirs[0][3]
            out["level"] = DR.histogram_level(n, world)
            out["splits_equal_on_ranks"] = all(t[3].tobytes() == sp.tobytes() for t in theirs)
            out["splits_equal_in_process"] = all(h[3].tobytes() == sp.tobytes() for h in here)
            out["splits_equal_restatement"] = bool(np.array_equal(sp, ref_splits))
            out["domain_equal_restatement"] = all(
                t[4][0].tobytes() == ref_dom[0].tobytes() and t[4][1].tobytes() == ref_dom[1].tobytes()
                and t[4][2] == ref_dom[2] for t in theirs + here)
            out["nobody_lost"] = bool(np.array_equal(np.sort(ids), np.arange(n)))
            out["owners_follow_keys"] = all(
                bool(np.all(np.searchsorted(sp[1:world], keys[t[0]], side="right") == r))
                for r, t in enumerate(theirs))
            out["moved"] = int(sum((t[0] % world != r).sum() for r, t in enumerate(theirs)))
            out["gravcost_equal"] = bool(np.array_equal(gc_r, gc_h)) and int(gc_r.min()) > 0
            out["rel_accel"] = float(relerr(ga_r, ga_h))
            out["bytes_decompose"] = int(theirs[0][5])
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    fp.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
