"""Rank program of tests/test_gpu_dd_guests.py::test_two_rank_processes_*: run under torch.distributed.run,
one process per rank, all ranks on GPU 0.  argv[1]: "accept" (gadget_force_config.accept_guests = 1) or
"refuse" (0, the default).

Every rank builds the same seeded problem, keeps the particles of its Peano-Hilbert key ranges as 536 /
264-byte records (the shipped bundle's layout, bound by byte offsets) and describes the decomposition the
way domain_Decomposition leaves it (TopNodes[] leaves in key order, DomainStartList / DomainEndList,
DomainTask[] per leaf: every rank owns FOUR pieces of the curve).  A first gravity_tree() runs on the
initial positions.  Then the particles move (test_gpu_dd_guests.displaced) and every rank writes the new
positions into the records it holds: the decomposition stays the first call's, as on a host that skips
domain_Decomposition between two force computations (domain.c:115-135).
  accept  gravity_tree(), density(), force_update_hmax(), hydro_force(); rank 0 gathers the records and checks
          them against the oracle's single tree of the moved positions
  refuse  the second gravity_tree() leaves through endrun on every rank and writes nothing
Exchanges go through the host's all-gather (gloo).  Rank 0 prints one JSON line."""
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    accept = {"accept": 1, "refuse": 0}[sys.argv[1]]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    json_fd = os.dup(1)
    os.dup2(2, 1)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from common import O, SinkProblem, bindings, relerr
    import test_gpu_boundary as TB
    import test_gpu_dd_guests as TG
    B = bindings()
    H = importlib.import_module("gadget-leicester_amd.hostapi")
    S = importlib.import_module("gadget-leicester_amd.sharded")

    sp = SinkProblem(ng=12, periodic=1, nsink=5, ndust=100)   # (sinks and grains are gravity sources here)
    pr = sp.pr
    n, ng = pr.n, pr.ngas
    eps = pr.force_soft[0] / 2.8

    def device_keys(pos):
        probe = B.ForcePath(0)
        probe.set_counts(n, 0)
        probe.set_field(B.F_POS, pos)
        probe.dd_init(0, 1)
        probe.dd_set_domain(pr.extent[0], pr.extent[1], pr.extent[2], pr.force_soft)
        k = probe.dd_keys()
        probe.close()
        return k

    # the decomposition of the INITIAL positions, as tests/gpu_host_ranks.py cuts it (-DMULTIPLEDOMAINS=4)
    keys = device_keys(pr.ic["pos"])
    level = S.histogram_level(n)
    while 8 ** level < world:
        level += 1
    shift = np.uint64(63 - 3 * level)
    cell = (keys >> shift).astype(np.int64)
    hist = np.bincount(cell, minlength=8 ** level).astype(np.float64)
    md = 4
    start, end = B.dd_find_split(world * md, hist)
    leaf_keys = (np.arange(8 ** level, dtype=np.uint64) << shift)
    leaf_size = np.full(8 ** level, np.uint64(1) << shift, np.uint64)
    piece = np.searchsorted(np.asarray(start[1:], np.int64), np.arange(8 ** level), side="right")
    piece_task = (np.arange(world * md) % world).astype(np.int32)
    domain_task = piece_task[piece].astype(np.int32)           # per top-leaf
    owner = domain_task[cell]
    bounds = np.concatenate([leaf_keys[np.asarray(start, np.int64)], [np.uint64(1) << np.uint64(63)]]).astype(np.uint64)
    bounds[0] = 0
    order = np.argsort(piece_task, kind="stable")
    start, end = np.asarray(start, np.int32)[order], np.asarray(end, np.int32)[order]
    mine = np.where(owner == rank)[0]
    gid = np.concatenate([mine[mine < ng], mine[mine >= ng]])

    # the displacement, and the guests it makes under that decomposition
    holder = owner.astype(np.int64)
    moved, _, _, _ = TG.displaced(pr, keys, holder, bounds, piece_task.astype(np.int64), TG.SEED)
    g, host_of, held, hosted = TG.expected_guests(pr, device_keys(moved), holder, world,
                                                  segments=(bounds, piece_task))

    lay, bh = TB.bundle_layouts(B, H)
    P, Sp = TB.bundle_records(sp, gid)
    host = H.Host(periodic=1, rank=rank, nranks=world, accept_guests=accept)

    def allgather(data):
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        out = torch.empty(world * len(data), dtype=torch.uint8)
        dist.all_gather_into_tensor(out, t)
        return out.numpy().tobytes()

    ok, err, codes, untouched = True, "", [], True
    try:
        host.set_allgather(allgather)
        host.bind_records(P, Sp, lay, bh)
        TB.set_all(host, sp, eps)
        host.set_topnodes(leaf_keys, leaf_size, start, end, domain_task=domain_task)
        host.set_active(None)
        host.set_domain(*pr.extent)      # the cube of the decomposition, kept for both calls
        L = host.L
        L.gravity_tree()                 # the first call: Barnes-Hut, leaves OldAcc
        if host.endrun_codes:
            raise RuntimeError("the first call: endrun %r: %s" % (host.endrun_codes,
                                                                 L.gadget_force_last_error().decode()))
        P["Pos"] = moved[gid]            # the particles drift; nobody decomposes
        L.gadget_force_mark_dirty()
        before_P, before_S = P.copy(), Sp.copy()
        L.gravity_tree()
        codes = [int(c) for c in host.endrun_codes]
        if accept:
            L.density()
            L.force_update_hmax()
            L.hydro_force()
            if host.endrun_codes:
                ok, err = False, "endrun %r: %s" % (host.endrun_codes, L.gadget_force_last_error().decode())
        else:
            # (member by member: a copy of a record array need not carry the bytes between the members)
            untouched = all(np.array_equal(P[k], before_P[k]) for k in P.dtype.names) and \
                all(np.array_equal(Sp[k], before_S[k]) for k in Sp.dtype.names)
            err = L.gadget_force_last_error().decode()
    except Exception as e:   # noqa: BLE001
        ok, err = False, repr(e)

    blob = [None] * world
    dist.all_gather_object(blob, (ok, err, gid, P.tobytes(), Sp.tobytes(), codes, untouched))
    if rank == 0:
        out = {"ok": all(b[0] for b in blob), "error": "; ".join(b[1] for b in blob if b[1]),
               "particles_expected": n, "guests": int(len(g)), "guests_held": [int(v) for v in held],
               "guests_hosted": [int(v) for v in hosted], "endrun_codes": [b[5] for b in blob],
               "untouched": [b[6] for b in blob]}
        if out["ok"] and accept:
            Pg = np.zeros(n, TB.P536)
            Sg = np.zeros(ng, TB.S264)
            seen = 0
            for _ok, _e, gd, pb, sb, _c, _u in blob:
                Pg[gd] = np.frombuffer(pb, TB.P536)
                Sg[gd[gd < ng]] = np.frombuffer(sb, TB.S264)
                seen += len(gd)
            out["particles"] = seen
            out["positions_moved"] = bool(np.array_equal(Pg["Pos"], moved))
            tg = np.arange(n, dtype=np.int32)
            tab = O.ewald_table(pr.box)
            T0 = O.Tree(pr.ic["pos"], pr.ic["vel"], pr.ic["mass"], pr.ic["type"], pr.force_soft,
                        hsml=sp.hsml, extent=pr.extent)
            a0, c0 = T0.gravity(pr.o_grav(pr.theta), tg, np.zeros(n))
            T0.gravity_ewald_add(pr.o_grav(pr.theta), tab, tg, np.zeros(n), a0, c0)
            old = np.linalg.norm(a0, axis=1)
            T = O.Tree(moved, pr.ic["vel"], pr.ic["mass"], pr.ic["type"], pr.force_soft, hsml=sp.hsml,
                       extent=pr.extent)
            a1, c1 = T.gravity(pr.o_grav(0.0), tg, old)
            T.gravity_ewald_add(pr.o_grav(0.0), tab, tg, old, a1, c1)
            out["counts_equal"] = bool(np.array_equal(Pg["GravCost"].astype(np.int64), c1))
            out["rel_acc"] = float(relerr(Pg["GravAccel"], pr.G * a1))
            act = np.arange(ng, dtype=np.int32)
            od = T.density(pr.o_dens(), act, pr.velpred, pr.entropy, pr.dtentropy, pr.timebin,
                           pr.ti_begstep, sp.hsml)
            out["rel_density"] = float(max(relerr(Sg["Density"], od["density"][:ng]),
                                           relerr(Pg["Hsml"][:ng], od["hsml"][:ng])))
            out["numngb_err"] = float(np.abs(Pg["NumNgb"][:ng] - od["numngb"][:ng]).max())
            T.update_hmax(act, od["hsml"], od["divvel"])
            oh = T.hydro(pr.o_hydro(), act, pr.velpred, od["hsml"], od["density"], od["pressure"],
                         od["dhsmlfac"], od["divvel"], od["curlvel"], pr.timebin)
            out["rel_hydro"] = float(np.abs(Sg["HydroAccel"] - oh["hydroaccel"][:ng]).max() /
                                     np.abs(oh["hydroaccel"]).max())
            out["rel_dtentropy"] = float(np.abs(Sg["DtEntropy"] - oh["dtentropy"][:ng]).max() /
                                         np.abs(oh["dtentropy"][:ng]).max())
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    host.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
