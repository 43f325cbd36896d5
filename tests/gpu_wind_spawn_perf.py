"""Measurement tool (not a test): ghip_wind_spawn next to the host round trip it replaces (every field down, the new
particles appended on the host, set_counts, every field up), and ghip_winds_feedback next to ghip_wind_feedback with
host arrays on the same list, at 2 x ng^3 particles with 300 sinks that emit about 10^4 wind particles.

    python tests/gpu_wind_spawn_perf.py [--ng 64] [--reps 3] [--out FILE]

Every timed region ends with a synchronisation inside the clock (the calls synchronise themselves), every shape is
run once untimed first, and the versions compared are alternated inside one run.  Prints one JSON line per
measurement; DESIGN.md 4.18 records the numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wind_ref as WR  # noqa: E402
import wind_spawn_ref as SR  # noqa: E402
from common import Problem, bindings  # noqa: E402

B = bindings()
NSINK = 300


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


class Case:
    def __init__(self, ng, seed=3):
        self.pr = pr = Problem(ng=ng, gas=True, periodic=1)
        rng = np.random.default_rng(seed)
        n, ngas = pr.n, pr.ngas
        sp = pr.ic["spacing"]
        self.sinks = np.sort(rng.choice(np.arange(ngas, n), NSINK, replace=False)).astype(np.int32)
        typ = pr.ic["type"].copy()
        typ[self.sinks] = 5
        mass = pr.ic["mass"].copy()
        mass[self.sinks] = rng.uniform(20.0, 46.0, NSINK)        # new_wind_exact = Mass: about 33 each
        timebin = pr.timebin.copy()
        timebin[self.sinks] = 1
        hsml = pr.hsml0.copy()
        hsml[self.sinks] = 2.0 * sp
        self.ids = np.arange(n, dtype=np.uint32)
        self.st = {B.F_POS: pr.ic["pos"], B.F_VEL: pr.ic["vel"], B.F_MASS: mass, B.F_TYPE: typ, B.F_HSML: hsml,
                   B.F_TIMEBIN: timebin, B.F_TI_BEGSTEP: pr.ti_begstep, B.F_ID: self.ids.view(np.int32),
                   B.F_VELPRED: pr.velpred, B.F_ENTROPY: pr.entropy, B.F_DTENTROPY: pr.dtentropy}
        par = SR.params(Time=1.0, SMBHmass=1.0, dt_fac=pr.timebase, MaxPart=n + 40 * NSINK,
                        SofteningBndryMaxPhys=0.1 * sp, InnerBoundary=0.1 * sp)
        par["VirtualMomentum"] *= SR.l_edd_dimensionless(par) * (2 * par["dt_fac"]) / SR.energy_wind_min(par)
        self.par = par
        self.rnd = rng.random(8192)
        self.sink_rows = np.zeros((NSINK, B.SK_COUNT))
        self.sink_rows[:, B.SK_BH_MASS] = mass[self.sinks]
        cnt = np.array([SR.count(par, mass[i], 1, mass[i], 0.0)[2] for i in self.sinks])
        self.parent = np.repeat(self.sinks, cnt)
        self.wind = WR.params(periodic=1, BoxSize=pr.box, Time=1.0 + 2 * pr.timebase, dt_fac=pr.timebase,
                              dt_fac_gas=pr.timebase, UnitDensity_in_cgs=60.0, VirtualTime=0.5, OuterBoundary=10.0,
                              OriginalGasMass=float(pr.ic["mass"][0]), SofteningGas=0.04 * sp,
                              SofteningGasMaxPhys=0.04 * sp, SofteningBulgeMaxPhys=0.2 * sp, PhotonSearchRadius=0.3,
                              dt_total_floor=1e-15 * 0.5 * n, rad_accel=1, max_iter=2000)

    def struct(self, cls, d):
        p = cls()
        for k, v in d.items():
            setattr(p, k, v)
        return p

    def load(self, fp):
        fp.set_counts(self.pr.n, self.pr.ngas)
        for f, a in self.st.items():
            fp.set_field(f, a)
        fp.sinks_set_table(self.ids[self.sinks], self.sink_rows)
        fp.winds_set_table([], np.zeros((0, B.WK_COUNT)))
        fp.sync()


def host_spawn(fp, c):
    """the round trip of a host without ghip_wind_spawn: every field down, P[NumPart + k] = P[parent] appended for
    every field (the host's own loop over :159-228 would follow on these arrays; it is not counted), set_counts,
    every field up.  The tables that set_counts refuses afterwards are not counted either."""
    f = {k: fp.get_field(k) for k in range(B.F_COUNT)}
    n = fp.n
    fp.set_counts(n + len(c.parent), fp.ngas)
    for k, a in f.items():
        fp.set_field(k, a if B._FIELD_INFO[k][0] else np.concatenate([a, a[c.parent]]))
    fp.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ng", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sink = open(a.out, "w") if a.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    c = Case(a.ng)
    pr = c.pr
    fp, fh = B.ForcePath(0), B.ForcePath(0)
    sp = c.struct(B.WindSpawnParams, c.par)
    # ---- the spawn against the round trip ----
    t_dev, t_host, rep = [], [], None
    for r in range(a.reps + 1):                # rep 0 warms every shape
        c.load(fp)
        ms, rep = clock(lambda: fp.wind_spawn(sp, c.rnd))
        c.load(fh)
        mh, _ = clock(lambda: host_spawn(fh, c))
        assert rep["spawned"] == len(c.parent) and fh.n == fp.n
        if r:
            t_dev.append(ms)
            t_host.append(mh)
    emit(dict(what="ghip_wind_spawn", n=pr.n, sinks=NSINK, spawned=rep["spawned"], ms=float(np.median(t_dev)),
              all_ms=t_dev))
    emit(dict(what="host round trip (get_field all, append, set_counts, set_field all)", n=pr.n,
              spawned=rep["spawned"], ms=float(np.median(t_host)), all_ms=t_host,
              ratio_to_the_call=float(np.median(t_host) / np.median(t_dev))))
    # ---- the loop: resident against host arrays, on the particles just born (fp holds them and their rows) ----
    idx, rows0 = fp.winds_table()
    start = {f: fp.get_field(f) for f in range(B.F_COUNT)}
    fh.set_counts(fp.n, fp.ngas)
    wp = c.struct(B.WindParams, c.wind)
    t_res, t_arr, its = [], [], None
    for r in range(a.reps + 1):
        for which, ctx in (("resident", fp), ("arrays", fh)):     # alternated
            for f in (B.F_POS, B.F_VEL, B.F_MASS, B.F_TYPE, B.F_HSML, B.F_TIMEBIN, B.F_ID) if r else range(B.F_COUNT):
                ctx.set_field(f, start[f])
            ctx.set_wind_injected(np.zeros((ctx.ngas, 3)))
            ctx.tree_build(pr.extent[0], pr.extent[1], pr.extent[2], pr.force_soft)
            if which == "resident":
                ctx.winds_set_table(idx, rows0)
                ctx.sync()
                ms, out = clock(lambda: ctx.winds_feedback(wp))
            else:
                ctx.sync()
                ms, out = clock(lambda: ctx.wind_feedback(wp, idx, rows0[:, B.WK_STELLAR_AGE],
                                                          rows0[:, B.WK_BIRTH_ENERGY], rows0[:, B.WK_OLD_MOMENTUM],
                                                          rows0[:, B.WK_NEW_DENSITY], rows0[:, B.WK_DRMIN]))
            its = its or out["iterations"]
            assert out["iterations"] == its
            if r:
                (t_res if which == "resident" else t_arr).append(ms)
    assert np.array_equal(fp.get_field(B.F_POS), fh.get_field(B.F_POS))
    emit(dict(what="ghip_winds_feedback", n=fp.n, nwind=len(idx), iterations=its, ms=float(np.median(t_res)),
              all_ms=t_res))
    emit(dict(what="ghip_wind_feedback with host arrays", n=fp.n, nwind=len(idx), iterations=its,
              ms=float(np.median(t_arr)), all_ms=t_arr, ratio_to_the_resident_call=float(np.median(t_arr) / np.median(t_res))))
    fp.close()
    fh.close()


if __name__ == "__main__":
    main()
