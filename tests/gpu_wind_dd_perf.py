"""What the wind loop costs on shards (a measurement script, not a test; the sibling of gpu_wind_perf.py and
gpu_fof_dd_perf.py): c2 (64^3 halo particles + 64^3 gas, periodic) as 8 logical shards on one GPU, with 1e4 and 1e5
of the halo particles turned into Type-3 wind particles as gpu_wind_perf.py makes them.  Per iteration, medians of
REPS calls from the same start state after one that allocates: the slowest shard's move, own density, imported
density, spread and list times (ghip_wind_get_timing after GHIP_DD_WIND: device events), the exchanges and the
bytes all shards sent, and the records exported per listed particle; the bytes again with the selection cut switched
off (GHIP_WIND_DD_CUT=0: the whole sphere Hsml), one call.  Prints one JSON line; --out FILE keeps it.

    python tests/gpu_wind_dd_perf.py [--ng 64] [--shards 8] [--reps 5] [--out FILE]
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
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--counts", default="10000,100000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import wind_ref as R
    from common import Problem, ShardSet, bindings
    B = bindings()
    pr = Problem(ng=a.ng, gas=True, periodic=1)
    n, ngas = pr.n, pr.ngas
    sp = pr.ic["spacing"]
    par = R.params(periodic=1, BoxSize=pr.box, dt_fac=6.25e-4, dt_fac_gas=6.25e-4, UnitDensity_in_cgs=100.0,
                   OriginalGasMass=float(pr.ic["mass"][0]), SofteningGas=0.03 * sp, SofteningGasMaxPhys=0.03 * sp,
                   SofteningBulgeMaxPhys=0.02, PhotonSearchRadius=0.3, rad_accel=1, max_iter=2000)
    speed = R.C_LIGHT / par["UnitVelocity_in_cm_per_s"] / par["FeedBackVelocity"]
    wp = B.WindParams()
    for k, v in par.items():
        setattr(wp, k, v)
    out = {"n": n, "ngas": ngas, "shards": a.shards, "cases": []}
    rng = np.random.default_rng(17)
    for nw in [int(c) for c in a.counts.split(",")]:
        wind = np.sort(rng.choice(np.arange(ngas, n), nw, replace=False)).astype(np.int32)
        typ = pr.ic["type"].copy()
        typ[wind] = 3
        vel = pr.ic["vel"].copy()
        d = rng.standard_normal((nw, 3))
        vel[wind] = speed * d / np.linalg.norm(d, axis=1)[:, None]
        mass = pr.ic["mass"].copy()
        mass[wind] = 1e-6
        old = 1e-3 * (1 + rng.random(nw))
        state = dict(stellar_age=rng.uniform(0.2, 0.95, nw), birth_energy=50.0 * old, old_momentum=old,
                     new_density=np.zeros(nw), drmin=np.zeros(nw))
        S = ShardSet(pr, a.shards)
        S.set_field(B.F_TYPE, typ)
        S.set_field(B.F_VEL, vel)
        S.set_field(B.F_MASS, mass)
        S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
        S.run.density(pr.g_dens())                          # (the gas's converged h)
        hsml = S.get_field(B.F_HSML)
        hsml[wind] = 2.0 * sp
        where = S.locate(wind)
        rows = []
        for rep in range(a.reps + 2):
            nocut = rep == a.reps + 1                        # the last call: the same run without the selection cut
            os.environ["GHIP_WIND_DD_CUT"] = "0" if nocut else "1"
            # the same start state: the wind particles back where they were, the trees of the step
            S.set_field(B.F_POS, pr.ic["pos"])
            S.set_field(B.F_MASS, mass)
            S.set_field(B.F_HSML, hsml)
            S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
            S.run.density(pr.g_dens())
            S.set_field(B.F_HSML, hsml)
            for fp in S.fp:
                fp.set_wind_injected(np.zeros((fp.ngas, 3)))
                fp.sync()
            t0 = time.perf_counter()
            res = S.run.wind_feedback(wp, [w[0] for w in where], [{k: v[w[1]] for k, v in state.items()} for w in where])
            for fp in S.fp:
                fp.sync()
            wall = (time.perf_counter() - t0) * 1e3
            ms = np.array([fp.wind_timing() for fp in S.fp]).max(axis=0)       # the slowest shard, phase by phase
            cnt = np.array([r["counts"] for r in res]).sum(axis=0)
            rows.append(np.r_[ms, wall, res[0]["iterations"], sum(int(r["bits"]) for r in res), cnt[0], cnt[2], cnt[4],
                              res[0]["counts"][3]])
        S.close()
        os.environ.pop("GHIP_WIND_DD_CUT")
        whole = rows.pop()
        med = np.median(np.array(rows[1:]), axis=0)          # (the first call allocates)
        it = med[6]
        out["cases"].append({"nwind": nw, "iterations": int(it), "basic_steps": int(med[7]),
                             "ms_move_per_iter": med[0] / it, "ms_own_density_per_iter": med[1] / it,
                             "ms_imported_density_per_iter": med[4] / it, "ms_spread_per_iter": med[2] / it,
                             "ms_list_per_iter": med[3] / it, "ms_call_wall": med[5],
                             "exchanges_per_iter": (med[11] - 3) / it, "bytes_per_iter": med[10] / it,
                             "records_exported_per_listed_particle": med[8] / max(med[7], 1),
                             "imported_pairs": int(med[9]),
                             "without_cut": {"iterations": int(whole[6]), "bytes_per_iter": whole[10] / whole[6],
                                             "records_exported_per_listed_particle": whole[8] / max(whole[7], 1),
                                             "imported_pairs": int(whole[9])}})
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
