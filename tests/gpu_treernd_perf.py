"""Development aid: what a bound RndTable (ghip_set_rnd_table) costs the tree phase -- ms_tree of
ghip_get_stats (the gravity tree's build on the main stream) and the wall time of build + gas tree + sync,
with the table against without it, alternating in one process, on
  * the c2 state (nothing crowded: the detection pass finds nothing to do), and
  * the c2 state with 1 % of the particles put into coincident pairs.
python tests/gpu_treernd_perf.py [ng] [reps]   (c2: ng = 64)"""
import sys
import time

import numpy as np

import treernd_ref as R
from common import Problem, bindings, ics


def measure(pr, table, reps, label):
    B = bindings()
    fp = pr.device()
    fp.set_field(B.F_ID, np.arange(pr.n, dtype=np.int32))
    out = {}
    for mode in ("off", "on"):                       # warm-up of both paths, buffers sized
        fp.set_rnd_table(table if mode == "on" else None)
        pr.device_tree(fp)
        fp.tree_dump(1)
        out["nodes_" + mode] = fp.stats()["tree_nodes"]
    ms = {"off": [], "on": []}
    wall = {"off": [], "on": []}
    for _ in range(reps):
        for mode in ("off", "on"):
            fp.set_rnd_table(table if mode == "on" else None)
            fp.stats()
            t0 = time.perf_counter()
            pr.device_tree(fp)
            s = fp.stats()                           # joins: the deferred gas tree is built, everything waited for
            wall[mode].append(1e3 * (time.perf_counter() - t0))
            ms[mode].append(s["ms_tree"])
    med = lambda v: float(np.median(v))
    print("%-28s n=%d  nodes off %d on %d  ms_tree off %.3f (%.3f .. %.3f)  on %.3f (%.3f .. %.3f)  "
          "build+gas tree+sync wall ms off %.3f on %.3f" %
          (label, pr.n, out["nodes_off"], out["nodes_on"], med(ms["off"]), min(ms["off"]), max(ms["off"]),
           med(ms["on"]), min(ms["on"]), max(ms["on"]), med(wall["off"]), med(wall["on"])), flush=True)
    fp.close()


def main():
    ng = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    table = np.random.default_rng(1).random(262144)
    ic = ics.make_ics(ng, gas=True, seed=12345, clustered=True)
    measure(Problem(ic=ic, periodic=1), table, reps, "c2")
    n = len(ic["pos"])
    crowded, _ = R.crowd(ic, groups=(2,) * (n // 200), npairs=0)      # 1 % of the particles
    measure(Problem(ic=crowded, periodic=1), table, reps, "c2, 1 % in coincident pairs")


if __name__ == "__main__":
    main()
