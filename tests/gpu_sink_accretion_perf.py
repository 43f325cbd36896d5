"""Time of blackhole_accretion() on a resident run, per-pass path against the resident sink table:

  per-pass   ghip_sink_density, ghip_blackhole_evaluate, ghip_blackhole_swallow with host arrays, the Mdot step
             and the finish on the host in vectorised numpy.  NOT included, in the per-pass path's favour: the
             read and write of the sinks' Vel and Mass around the finish (a host would move 32 bytes per sink;
             the bindings only move whole fields)
  resident   ghip_sinks_density + ghip_blackhole_accretion

on one context and one problem, alternating, after one warm-up call of each.  Both change masses, so before
every call MASS, VEL and HSML are restored and the trees rebuilt (not timed).

    python tests/gpu_sink_accretion_perf.py [ng] [nsink] [reps]      (default 256 300 6: c5's size class)
"""
import sys
import time

import numpy as np

import sink_accretion_cases as AC
import sink_accretion_ref as AR
from common import SinkProblem, bindings, sink_over


def main():
    ng = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    nsink = int(sys.argv[2]) if len(sys.argv) > 2 else 300
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    B = bindings()
    t0 = time.perf_counter()
    sp = SinkProblem(ng=ng, periodic=1, nsink=nsink, ndust=10 * nsink)
    pr = sp.pr
    print("problem: %d particles, %d gas, %d sinks (%.0f s)" % (pr.n, pr.ngas, nsink, time.perf_counter() - t0),
          flush=True)
    sk = sp.sinks
    ids5 = sp.ids[sk]
    state = AC.state_for(sp)
    acc = AC.acc_for(sp, state)
    rows0 = AC.rows_of(B, state)
    gp = sp.params(B.BhParams, **sink_over(0, 0))
    gacc = B.BhAccretionParams()
    for k, _ in gacc._fields_:
        setattr(gacc, k, getattr(acc, k))
    fp = pr.device()
    fp.set_field(B.F_ID, sp.ids.view(np.int32))
    fp.set_field(B.F_DENSITY, 0.5 + np.random.default_rng(3).random(pr.ngas))
    dens = pr.g_dens()
    mass0, vel0 = pr.ic["mass"], pr.ic["vel"]
    tb = pr.timebin[sk]
    dt = AR.timestep(tb, sp.par["dt_fac"])

    def restore():
        fp.set_field(B.F_MASS, mass0)
        fp.set_field(B.F_VEL, vel0)
        fp.set_field(B.F_HSML, sp.hsml)
        pr.device_tree(fp)
        fp.sync()

    def per_pass():
        t = time.perf_counter()
        d = fp.sink_density(dens, AC.NGB_FACTOR, sk, sp.hsml[sk])
        m = mass0[sk]
        lim = acc.EddingtonFactor * (acc.medd_fac * m)
        mdot = np.minimum(state["accdisc"] / (dt + acc.tvisc), lim)
        disc, hole = state["accdisc"] - mdot * dt, state["bh_mass"] + mdot * dt
        fp.sink_reset()
        fp.blackhole_evaluate(gp, sk, ids5, mdot, d["density"])
        go = fp.blackhole_swallow(gp, sk, ids5, hole)
        am = go["acc_mass"]
        took = am > 0
        v = np.where(took[:, None], (vel0[sk] * m[:, None] + go["acc_momentum"]) / (m + am)[:, None], vel0[sk])
        m = m + am
        hole = go["bh_mass"] + np.where(took, go["acc_bhmass"], 0.0)
        disc = disc + am
        ms = (time.perf_counter() - t) * 1e3
        return ms, int(go["counts"].sum()), float(m.sum() + v.sum() + hole.sum() + disc.sum())

    def resident():
        fp.sinks_set_table(ids5, rows0)          # (not timed: once per run in a real host)
        fp.sync()
        t = time.perf_counter()
        fp.sinks_density(dens, AC.NGB_FACTOR)
        rep = fp.blackhole_accretion(gp, gacc)
        ms = (time.perf_counter() - t) * 1e3
        return ms, int(rep["counts"].sum()), 0.0

    out = {"per_pass": [], "resident": []}
    for r in range(reps + 1):
        for name, fn in (("per_pass", per_pass), ("resident", resident)):
            restore()
            ms, swallowed, _ = fn()
            if r > 0:
                out[name].append(ms)
            print("%s %-9s %8.3f ms   %d swallowed" % ("warm-up" if r == 0 else "rep %d  " % r, name, ms, swallowed),
                  flush=True)
    for name, v in out.items():
        v = np.array(v)
        print("%-9s median %.3f ms, min %.3f, max %.3f over %d calls" % (name, np.median(v), v.min(), v.max(), len(v)))
    fp.close()


if __name__ == "__main__":
    main()
