"""What the friends-of-friends groups cost on shards (a measurement script, not a test; DESIGN.md 4.17 "On shards"):
the c2 state of tests/gpu_fof_perf.py (64^3 halo particles + 64^3 gas in a periodic box) with the three LinkL of
that script, as 1 context (ghip_fof) and as 2, 4 and 8 logical shards on one GPU (GHIP_DD_GLOBAL_QUANTITIES begun with
walk = GHIP_FOF_FORM after GHIP_DD_GRAVITY).  Medians of REPS calls after one warm-up call per shape: the four stage
times per shard (ghip_fof_get_timing, exchanges excluded), label rounds, secondary rounds, records and bytes sent,
wall time of the call.  The labels of the shards are checked against the single-context run.

Logical shards on one GPU run one after the other: the SUM of a stage over the shards is the figure to compare with
the single context, not the maximum.  Prints one JSON line; --out FILE keeps it.

    python tests/gpu_fof_dd_perf.py [--ng 64] [--reps 7] [--shards 2,4,8] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ng", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shards", default="2,4,8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import fof_ref as FR
    from common import Problem, ShardSet, bindings
    B = bindings()
    pr = Problem(ng=a.ng, gas=True, periodic=1)
    n, ptype, mass = pr.n, pr.ic["type"], pr.ic["mass"]
    prim = np.where(ptype == 1)[0]
    rhodm = float(mass[prim].sum()) / pr.box ** 3
    rule = FR.linklength_rule(mass, ptype, 2, 0.2, rhodm)
    cases = (("LINKLENGTH rule", 0.0), ("2 x LINKLENGTH rule", 2.0 * rule), ("5.2 x LINKLENGTH rule", 5.2 * rule))
    par = dict(linklength=0.2, rhodm=rhodm, primary_types=2, secondary_types=1, group_min_len=32, boxsize=pr.box,
               periodic=True)

    # one context: the labels every shape is compared with, and its stage times
    fp = pr.device()
    fp.set_field(B.F_ID, np.arange(n, dtype=np.int32))
    pr.device_tree(fp)
    fp.density(pr.g_dens())
    density = fp.get_field(B.F_DENSITY)
    hsml = np.zeros(n)
    hsml[:pr.ngas] = fp.get_field(B.F_HSML)[:pr.ngas]
    out = {"n": n, "ngas": pr.ngas, "nprim": int(len(prim)), "reps": a.reps, "shapes": []}
    want = {}
    one = {"shards": 1, "cases": []}
    for label, linkl in cases:
        ms = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            res = fp.fof(link_length=linkl, **par)
            wall = (time.perf_counter() - t0) * 1e3
            ms.append(np.r_[fp.fof_timing(), wall])
        med = np.median(np.array(ms[1:]), axis=0)
        want[label] = (fp.fof_labels()[0], res)
        one["cases"].append({"case": label, "LinkL": res.LinkL, "Ngroups": res.Ngroups, "largest": res.largest,
                             "nearest_iterations": res.nearest_iterations, "ms_stages": med[:4].tolist(),
                             "ms_wall_call": med[4]})
    out["shapes"].append(one)
    fp.close()

    for P in [int(s) for s in a.shards.split(",")]:
        S = ShardSet(pr, P, fields={"oldacc": np.ones(n), "hsml": np.where(hsml > 0, hsml, pr.hsml0)})
        S.set_field(B.F_DENSITY, density)
        S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
        shape = {"shards": P, "cases": []}
        for label, linkl in cases:
            ms, cnt = [], None
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                res = S.run.fof(link_length=linkl, **par)
                wall = (time.perf_counter() - t0) * 1e3
                ms.append((np.array([f.fof_timing() for f in S.fp]), wall))
                cnt = np.array([r.counts for r in res])
            stages = np.median(np.array([m[0] for m in ms[1:]]), axis=0)       # [shard][stage]
            lab = np.zeros(n, np.int32)
            for r, f in enumerate(S.fp):
                if len(S.gid[r]):
                    lab[S.gid[r]] = f.fof_labels()[0]
            ref_lab, ref_res = want[label]
            shape["cases"].append({
                "case": label, "LinkL": res[0].LinkL, "Ngroups": res[0].Ngroups, "largest": res[0].largest,
                "nearest_iterations": res[0].nearest_iterations,
                "labels_equal_single_context": bool(np.array_equal(lab, ref_lab)),
                "result_equal_single_context": (res[0].Ngroups, res[0].Nids, res[0].largest, res[0].nearest_iterations)
                == (ref_res.Ngroups, ref_res.Nids, ref_res.largest, ref_res.nearest_iterations),
                "ms_stages_per_shard": stages.tolist(), "ms_stages_sum": stages.sum(axis=0).tolist(),
                "ms_stages_max": stages.max(axis=0).tolist(), "ms_wall_call": float(np.median([m[1] for m in ms[1:]])),
                "label_rounds": int(cnt[0][3]), "primaries_sent": int(cnt[:, 1].sum()),
                "queries_sent": int(cnt[:, 4].sum()), "partials_sent": int(cnt[:, 5].sum()),
                "bytes_sent": int(cnt[:, 6].sum()), "groups_owned": cnt[:, 7].tolist()})
        out["shapes"].append(shape)
        S.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
