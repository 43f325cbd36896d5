"""What the friends-of-friends group finder costs on the c2 state (a measurement script, not a test):
64^3 halo particles + 64^3 gas in a periodic box, after a tree build and a converged density pass.  Device
milliseconds of ghip_fof's four stages (ghip_fof_get_timing: the linking kernel, the flattening and labels, the
secondary rounds, the catalogue) for LinkL from the LINKLENGTH rule, twice and 5.2 times that value (the last gives one
percolating group: the worst case of the union-find), medians of REPS calls; the tree build's and the density pass's device
time of the same run for scale; and the same partition on the CPU by scipy (cKDTree.query_pairs +
connected_components), which the device labels are compared with.  Prints one JSON line; --out FILE keeps it.

    python tests/gpu_fof_perf.py [--ng 64] [--reps 7] [--out FILE]
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree

    import fof_ref as FR
    from common import Problem, bindings
    B = bindings()
    pr = Problem(ng=a.ng, gas=True, periodic=1)
    n, ptype, pos, mass = pr.n, pr.ic["type"], pr.ic["pos"], pr.ic["mass"]
    fp = pr.device()
    fp.set_field(B.F_ID, np.arange(1, n + 1, dtype=np.int32))
    for _ in range(2):                                     # (the first build and pass allocate)
        pr.device_tree(fp)
        fp.density(pr.g_dens())
    fp.sync()
    st = fp.stats()
    prim = np.where(ptype == 1)[0]
    rhodm = float(mass[prim].sum()) / pr.box ** 3
    out = {"n": n, "ngas": pr.ngas, "nprim": int(len(prim)), "ms_tree": st["ms_tree"], "ms_dens": st["ms_dens"],
           "cases": []}
    # (the c2 state is a perturbed lattice of spacing 5 LinkL: the rule and twice the rule link nothing; 5.2 x the
    # rule, just over one spacing, gives the one percolating group)
    for label, fac in (("LINKLENGTH rule", 1.0), ("2 x LINKLENGTH rule", 2.0), ("5.2 x LINKLENGTH rule", 5.2)):
        linkl = fac * FR.linklength_rule(mass, ptype, 2, 0.2, rhodm) if fac != 1.0 else 0.0
        ms = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            res = fp.fof(link_length=linkl, linklength=0.2, rhodm=rhodm, primary_types=2, secondary_types=1,
                         group_min_len=32, boxsize=pr.box, periodic=True)
            wall = (time.perf_counter() - t0) * 1e3
            ms.append(np.r_[fp.fof_timing(), wall])
        med = np.median(np.array(ms[1:]), axis=0)          # (the first call allocates)
        minid, _ = fp.fof_labels()
        # the CPU: the link graph of the primaries and its components
        t0 = time.perf_counter()
        pp = np.mod(pos[prim], pr.box)
        pairs = cKDTree(pp, boxsize=pr.box).query_pairs(res.LinkL, output_type="ndarray")
        g = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(len(prim), len(prim)))
        ncomp, comp = connected_components(g, directed=False)
        cpu_s = time.perf_counter() - t0
        # same partition: components <-> labels one to one (up to pairs within rounding of LinkL)
        pairs_lab = np.unique(np.stack([comp, minid[prim]], axis=1), axis=0)
        same = len(pairs_lab) == ncomp == len(np.unique(minid[prim]))
        out["cases"].append({"case": label, "LinkL": res.LinkL, "Ngroups": res.Ngroups, "Nids": res.Nids,
                             "largest": res.largest, "nearest_iterations": res.nearest_iterations,
                             "ms_link": med[0], "ms_flatten": med[1], "ms_secondaries": med[2], "ms_catalogue": med[3],
                             "ms_wall_call": med[4], "link_pairs": int(len(pairs)), "components_of_primaries": int(ncomp),
                             "cpu_scipy_s": cpu_s, "same_partition_as_scipy": bool(same)})
    fp.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
