"""Time and blocking reads of blackhole_accretion() on 8 logical shards of one GPU, per-pass forms against the
resident forms:

  per-pass   GHIP_DD_SINK_DENSITY, GHIP_DD_BH_EVALUATE, GHIP_DD_BH_SWALLOW (walk = 0) with host arrays, the Mdot step
             and the finish on the host in vectorised numpy, per shard.  NOT included, in the per-pass path's
             favour: the read and write of the sinks' Vel and Mass around the finish, and the re-indexing of the
             host's per-sink arrays after a migration
  resident   GHIP_DD_SINK_DENSITY + GHIP_DD_BH_SWALLOW with walk = GHIP_SINKS_RESIDENT_FORM

alternating, after one warm-up call of each.  Both change masses, so before every call MASS, VEL and HSML are
restored, the tables given again and the trees rebuilt (not timed).  Blocking reads: the host waits of shard 0
inside the library during the call (ghip_run_stats.blocking_syncs); the device-to-device exchanges of logical shards
wait too, once per exchange and shard, for both paths alike.

    python tests/gpu_sink_accretion_dd_perf.py [ng] [nsink] [reps] [nshards]   (default 256 300 6 8: c5's size class)
"""
import sys
import time

import numpy as np

import sink_accretion_cases as AC
import sink_accretion_ref as AR
import test_gpu_sink_accretion_dd as TS
from common import SinkProblem, bindings, sink_over


def main():
    arg = lambda k, d: int(sys.argv[k]) if len(sys.argv) > k else d
    ng, nsink, reps, nshards = arg(1, 256), arg(2, 300), arg(3, 6), arg(4, 8)
    B = bindings()
    t0 = time.perf_counter()
    sp = SinkProblem(ng=ng, periodic=1, nsink=nsink, ndust=10 * nsink)
    sp.gas_density = 0.5 + np.random.default_rng(3).random(sp.pr.ngas)
    pr = sp.pr
    state = AC.state_for(sp)
    acc = AC.acc_for(sp, state)
    rows0 = AC.rows_of(B, state)
    gp = sp.params(B.BhParams, **sink_over(0, 0))
    gacc = TS._gacc(B, acc)
    run = TS.Run(sp, nshards, rows0)
    S = run.S
    print("problem: %d particles, %d gas, %d sinks on %d shards (%.0f s)"
          % (pr.n, pr.ngas, nsink, nshards, time.perf_counter() - t0), flush=True)
    dens = pr.g_dens()
    on = [run.sinks_on(r) for r in range(nshards)]
    slot = {int(g): k for k, g in enumerate(sp.sinks)}
    where = [np.array([slot[int(g)] for g in glob], np.int64) for _, glob in on]
    ids = [np.ascontiguousarray(sp.ids[glob]) for _, glob in on]
    tables = [fp.sinks_table() for fp in S.fp]
    saved = [[fp.get_field(f) for f in (B.F_MASS, B.F_VEL, B.F_HSML)] for fp in S.fp]
    dt = AR.timestep(pr.timebin[sp.sinks], sp.par["dt_fac"])
    m0, v0 = pr.ic["mass"][sp.sinks], pr.ic["vel"][sp.sinks]

    def restore():
        for fp, (m, v, h), t in zip(S.fp, saved, tables):
            fp.set_field(B.F_MASS, m)
            fp.set_field(B.F_VEL, v)
            fp.set_field(B.F_HSML, h)
            fp.sinks_set_table(*t)
        run.trees()
        for fp in S.fp:
            fp.sync()

    def per_pass():
        d = TS._op(S, B.DD_SINK_DENSITY, lambda r: B.dd_sink_args(on[r][0], dens=dens, ngb_factor=AC.NGB_FACTOR,
                                                                   hsml=sp.hsml[on[r][1]]))
        out = 0.0
        st = []
        for r in range(nshards):
            w = where[r]
            lim = acc.EddingtonFactor * (acc.medd_fac * m0[w])
            mdot = np.minimum(state["accdisc"][w] / (dt[w] + acc.tvisc), lim)
            st.append((mdot, state["accdisc"][w] - mdot * dt[w], state["bh_mass"][w] + mdot * dt[w]))
        S.each(lambda fp: fp.sink_reset())
        TS._op(S, B.DD_BH_EVALUATE, lambda r: B.dd_sink_args(on[r][0], sink_ids=ids[r], bh=gp, mdot=st[r][0],
                                                              bh_density=d[r]["density"]))
        go = TS._op(S, B.DD_BH_SWALLOW, lambda r: B.dd_sink_args(on[r][0], sink_ids=ids[r], bh=gp,
                                                                 sink_bh_mass=st[r][2]))
        swallowed = 0
        for r in range(nshards):
            w, g = where[r], go[r]
            am = g["acc_mass"]
            took = am > 0
            v = np.where(took[:, None], (v0[w] * m0[w][:, None] + g["acc_momentum"]) / (m0[w] + am)[:, None], v0[w])
            hole = g["bh_mass"] + np.where(took, g["acc_bhmass"], 0.0)
            out += float((m0[w] + am).sum() + v.sum() + hole.sum() + (st[r][1] + am).sum())
            swallowed += int(g["counts"].sum())
        return swallowed

    def resident():
        S.run.sinks_density(dens, AC.NGB_FACTOR)
        return int(sum(r["counts"].sum() for r in S.run.blackhole_accretion(gp, gacc)))

    res = {"per_pass": [], "resident": []}
    reads = {}
    for rep in range(reps + 1):
        for name, fn in (("per_pass", per_pass), ("resident", resident)):
            restore()
            S.fp[0].run_begin(1)
            t = time.perf_counter()
            swallowed = fn()
            ms = (time.perf_counter() - t) * 1e3
            reads[name] = S.fp[0].run_end()["blocking_syncs"]
            if rep > 0:
                res[name].append(ms)
            print("%s %-9s %8.3f ms   %d swallowed   %d blocking reads on shard 0"
                  % ("warm-up" if rep == 0 else "rep %d  " % rep, name, ms, swallowed, reads[name]), flush=True)
    for name, v in res.items():
        v = np.array(v)
        print("%-9s median %.3f ms, min %.3f, max %.3f over %d calls; %d blocking reads per call on shard 0"
              % (name, np.median(v), v.min(), v.max(), len(v), reads[name]))
    run.close()


if __name__ == "__main__":
    main()
