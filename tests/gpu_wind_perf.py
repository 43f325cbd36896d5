"""What the wind pass costs on the c2 gas (a measurement script, not a test): 64^3 halo particles + 64^3 gas in a
periodic box after a tree build and a converged density pass, with 1e4 and 1e5 of the halo particles turned into
Type-3 wind particles (Hsml two mean spacings, speed C / U / FBV, time bins 1..3: up to 0.25 box lengths per step
in jumps of at most 0.2 Hsml).  Device milliseconds of ghip_wind_feedback's phases per iteration
(ghip_wind_get_timing: move, density with the pair count and its scan, spread = fill + sort + apply, list = flags +
selection) and the whole call on the host's clock, medians of REPS calls from the same start state; one
ghip_wind_density call and, as a yardstick of the same shape, one ghip_dust_density call for the same particles
(then typed 2) on the host's clock.  Prints one JSON line; --out FILE keeps it.

    python tests/gpu_wind_perf.py [--ng 64] [--reps 5] [--out FILE]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--counts", default="10000,100000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import wind_ref as R
    from common import Problem, bindings
    B = bindings()
    pr = Problem(ng=a.ng, gas=True, periodic=1)
    n, ngas = pr.n, pr.ngas
    sp = pr.ic["spacing"]
    fp = pr.device()
    for _ in range(2):                                     # (the first build and pass allocate)
        pr.device_tree(fp)
        fp.density(pr.g_dens())
    fp.sync()
    st = fp.stats()
    hsml = fp.get_field(B.F_HSML)
    out = {"n": n, "ngas": ngas, "ms_tree": st["ms_tree"], "ms_dens": st["ms_dens"], "cases": []}
    par = R.params(periodic=1, BoxSize=pr.box, dt_fac=6.25e-4, dt_fac_gas=6.25e-4, UnitDensity_in_cgs=100.0,
                   OriginalGasMass=float(pr.ic["mass"][0]), SofteningGas=0.03 * sp, SofteningGasMaxPhys=0.03 * sp,
                   SofteningBulgeMaxPhys=0.02, PhotonSearchRadius=0.3, rad_accel=1, max_iter=2000)
    speed = R.C_LIGHT / par["UnitVelocity_in_cm_per_s"] / par["FeedBackVelocity"]
    wp = B.WindParams()
    for k, v in par.items():
        setattr(wp, k, v)
    dp = B.DustParams()
    dp.periodic, dp.BoxSize = 1, pr.box
    rng = np.random.default_rng(17)
    for nw in [int(c) for c in a.counts.split(",")]:
        wind = np.sort(rng.choice(np.arange(ngas, n), nw, replace=False)).astype(np.int32)
        typ = pr.ic["type"].copy()
        vel = pr.ic["vel"].copy()
        d = rng.standard_normal((nw, 3))
        vel[wind] = speed * d / np.linalg.norm(d, axis=1)[:, None]
        h = hsml.copy()
        h[wind] = 2.0 * sp
        mass = pr.ic["mass"].copy()
        mass[wind] = 1e-6
        tb = pr.timebin.copy()
        old = 1e-3 * (1 + rng.random(nw))
        state = (rng.uniform(0.2, 0.95, nw), 50.0 * old, old, np.zeros(nw), np.zeros(nw))
        dtj = (1 << tb[wind].astype(np.int64)) * par["dt_fac"]

        def start(t):
            typ[wind] = t
            fp.set_field(B.F_TYPE, typ)
            fp.set_field(B.F_POS, pr.ic["pos"])
            fp.set_field(B.F_VEL, vel)
            fp.set_field(B.F_HSML, h)
            fp.set_field(B.F_MASS, mass)
            fp.set_field(B.F_TIMEBIN, tb)
            pr.device_tree(fp)
            fp.sync()

        def clock(fn):
            fp.sync()
            t0 = time.perf_counter()
            r = fn()
            fp.sync()
            return (time.perf_counter() - t0) * 1e3, r

        # the yardstick: the dust density pass for the same particles, typed 2
        start(2)
        ms_dust = [clock(lambda: fp.dust_density(dp, wind))[0] for _ in range(a.reps + 1)]
        start(3)
        ms_wdens = [clock(lambda: fp.wind_density(wp, wind, dtj))[0] for _ in range(a.reps + 1)]
        rows = []
        for _ in range(a.reps + 1):
            start(3)
            fp.set_wind_injected(np.zeros((ngas, 3)))
            fp.wind_density(wp, wind[:1], dtj[:1])         # (completes the deferred gas tree outside the clock)
            wall, res = clock(lambda: fp.wind_feedback(wp, wind, *state))
            rows.append(np.r_[fp.wind_timing(), wall, res["iterations"], res["bits"]])
        med = np.median(np.array(rows[1:]), axis=0)        # (the first call allocates)
        it = med[6]
        out["cases"].append({"nwind": nw, "iterations": int(it), "basic_steps": int(med[7]),
                             "ms_move_per_iter": med[0] / it, "ms_density_per_iter": med[1] / it,
                             "ms_spread_per_iter": med[2] / it, "ms_list_per_iter": med[3] / it,
                             "ms_phases_sum": float(med[:4].sum()), "ms_call_in_library": med[4],
                             "ms_call_wall": med[5], "ndeleted": int(res["ndeleted"]),
                             "ms_wind_density_call": float(np.median(ms_wdens[1:])),
                             "ms_dust_density_call": float(np.median(ms_dust[1:]))})
    fp.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
