"""What the resident wind particles cost on shards (a measurement script, not a test; the sibling of
gpu_wind_dd_perf.py and gpu_sink_accretion_dd_perf.py): c2 (64^3 halo particles + 64^3 gas, periodic) as 8 logical
shards on one GPU, with 1e4 of the halo particles turned into Type-3 wind particles as gpu_wind_dd_perf.py makes them.
Medians of REPS calls after one that allocates, the two sides alternated from the same start state:

  loop       GHIP_DD_WIND with walk = GHIP_WINDS_RESIDENT_FORM (the list and the planes from the shards' wind tables)
             against walk = GHIP_WIND_FORM with host arrays on the same lists; wall time of the call, the exchanges,
             and the blocking waits inside the library per shard (ghip_run_stats.blocking_syncs)
  migration  GHIP_DD_MIGRATE of the same moves with wind tables on all shards against without: wall time, the
             exchanges taken, the kernel launches of all shards (ghip_run_stats.launches); and the run without tables
             against itself, which shows the spread of the figure

  spawn      GHIP_DD_WIND with walk = GHIP_WINDS_SPAWN_FORM on the case of gpu_wind_spawn_perf.py (300 sinks emitting
             about 1e4 wind particles) against the per-shard host round trip it replaces (every field down, append,
             ghip_set_counts, every field up, on every shard)

Prints one JSON line; --out FILE keeps it.  --only migration: the migration without tables alone, which also runs on
a tree from before the wind tables existed on shards (for the launch and exchange counts of that tree).

    python tests/gpu_winds_dd_perf.py [--ng 64] [--shards 8] [--reps 5] [--nwind 10000] [--only migration] [--out FILE]
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


def spawn_part(B, P, ng, reps):
    """form 33 on P shards against the host round trip on every shard, alternated from the same start state"""
    import gpu_wind_spawn_perf as GS
    from common import ShardSet
    GS.B = B
    c = GS.Case(ng)
    S = ShardSet(c.pr, P)
    counts = [fp.counts() for fp in S.fp]
    sinks = S.locate(c.sinks)
    parents = [w[0] for w in S.locate(c.parent)]             # the local sink of every new particle, per shard
    prm = c.struct(B.WindSpawnParams, c.par)

    def reset():
        for r, fp in enumerate(S.fp):
            fp.set_counts(*counts[r])
        for f, v in c.st.items():
            S.set_field(f, v)
        for r, fp in enumerate(S.fp):
            loc, at = sinks[r]
            fp.sinks_set_table(c.ids[c.sinks[at]], c.sink_rows[at].reshape(len(at), B.SK_COUNT))
            fp.dd_winds_set_table([], np.zeros((0, B.WK_COUNT)))
            fp.set_active(None)
            fp.sync()

    def round_trip():
        for r, fp in enumerate(S.fp):
            f = {k: fp.get_field(k) for k in range(B.F_COUNT)}
            fp.set_counts(fp.n + len(parents[r]), fp.ngas)
            for k, v in f.items():
                fp.set_field(k, v if B._FIELD_INFO[k][0] else np.concatenate([v, v[parents[r]]]))
            fp.sync()

    t = {"form33": [], "round_trip": []}
    spawned = 0
    for rep in range(reps + 1):
        reset()
        t0 = time.perf_counter()
        res = S.run.wind_spawn(prm, c.rnd)
        for fp in S.fp:
            fp.sync()
        t["form33"].append((time.perf_counter() - t0) * 1e3)
        spawned = res[0]["tot_spawned"]
        assert [r["spawned"] for r in res] == [len(q) for q in parents]
        reset()
        t0 = time.perf_counter()
        round_trip()
        t["round_trip"].append((time.perf_counter() - t0) * 1e3)
    S.close()
    a, b = float(np.median(t["form33"][1:])), float(np.median(t["round_trip"][1:]))
    return {"sinks": len(c.sinks), "tot_spawned": int(spawned), "ms_form33": a, "ms_host_round_trip_all_shards": b,
            "round_trip_over_form33": b / a, "exchanges_form33": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ng", type=int, default=64)
    ap.add_argument("--shards", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nwind", type=int, default=10000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    only_mig = a.only == "migration"
    import wind_ref as R
    from common import Problem, ShardSet, bindings
    B = bindings()
    pr = Problem(ng=a.ng, gas=True, periodic=1)
    n, ngas, P = pr.n, pr.ngas, a.shards
    sp = pr.ic["spacing"]
    par = R.params(periodic=1, BoxSize=pr.box, dt_fac=6.25e-4, dt_fac_gas=6.25e-4, UnitDensity_in_cgs=100.0,
                   OriginalGasMass=float(pr.ic["mass"][0]), SofteningGas=0.03 * sp, SofteningGasMaxPhys=0.03 * sp,
                   SofteningBulgeMaxPhys=0.02, PhotonSearchRadius=0.3, rad_accel=1, max_iter=2000)
    speed = R.C_LIGHT / par["UnitVelocity_in_cm_per_s"] / par["FeedBackVelocity"]
    wp = B.WindParams()
    for k, v in par.items():
        setattr(wp, k, v)
    rng = np.random.default_rng(17)
    nw = a.nwind
    wind = np.sort(rng.choice(np.arange(ngas, n), nw, replace=False)).astype(np.int32)
    typ = pr.ic["type"].copy()
    typ[wind] = 3
    vel = pr.ic["vel"].copy()
    d = rng.standard_normal((nw, 3))
    vel[wind] = speed * d / np.linalg.norm(d, axis=1)[:, None]
    mass = pr.ic["mass"].copy()
    mass[wind] = 1e-6
    old = 1e-3 * (1 + rng.random(nw))
    rows = np.zeros((nw, B.WK_COUNT))
    rows[:, B.WK_STELLAR_AGE] = rng.uniform(0.2, 0.95, nw)
    rows[:, B.WK_BIRTH_ENERGY] = 50.0 * old
    rows[:, B.WK_OLD_MOMENTUM] = old
    state = dict(stellar_age=rows[:, B.WK_STELLAR_AGE], birth_energy=rows[:, B.WK_BIRTH_ENERGY],
                 old_momentum=rows[:, B.WK_OLD_MOMENTUM], new_density=np.zeros(nw), drmin=np.zeros(nw))
    S = ShardSet(pr, P)
    S.set_field(B.F_TYPE, typ)
    S.set_field(B.F_VEL, vel)
    S.set_field(B.F_MASS, mass)
    S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
    S.run.density(pr.g_dens())                              # (the gas's converged h)
    hsml = S.get_field(B.F_HSML)
    hsml[wind] = 2.0 * sp
    where = S.locate(wind)

    def begin():
        for fp in S.fp:
            fp.run_begin(1)

    def end():
        """-> (the most blocking waits of a shard, the launches of all shards) since begin()"""
        st = [fp.run_end() for fp in S.fp]
        return max(int(q["blocking_syncs"]) for q in st), sum(int(q["launches"]) for q in st)

    # ---- the loop ----
    loop = {"resident": [], "host": []}
    for rep in range(0 if only_mig else a.reps + 1):
        for side in ("resident", "host"):
            S.set_field(B.F_POS, pr.ic["pos"])
            S.set_field(B.F_MASS, mass)
            S.set_field(B.F_HSML, hsml)
            S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
            S.run.density(pr.g_dens())
            S.set_field(B.F_HSML, hsml)
            for r, fp in enumerate(S.fp):
                fp.set_wind_injected(np.zeros((fp.ngas, 3)))
                if side == "resident":
                    fp.dd_winds_set_table(where[r][0], rows[where[r][1]])
                fp.sync()
            begin()
            t0 = time.perf_counter()
            if side == "resident":
                res = S.run.winds_feedback(wp)
            else:
                res = S.run.wind_feedback(wp, [w[0] for w in where], [{k: v[w[1]] for k, v in state.items()} for w in where])
            for fp in S.fp:
                fp.sync()
            wall = (time.perf_counter() - t0) * 1e3
            loop[side].append((wall, res[0]["iterations"], int(res[0]["counts"][3]), end()[0],
                               sum(int(r["bits"]) for r in res)))
    out = {"n": n, "ngas": ngas, "shards": P, "nwind": nw, "loop": {}}
    for side, v in ([] if only_mig else loop.items()):
        med = np.median(np.array(v[1:]), axis=0)             # (the first call allocates)
        out["loop"][side] = {"ms_call_wall": med[0], "iterations": int(med[1]), "exchanges": int(med[2]),
                             "blocking_syncs_per_shard": int(med[3]), "basic_steps": int(med[4])}
    if not only_mig:
        out["loop"]["resident_over_host"] = out["loop"]["resident"]["ms_call_wall"] / out["loop"]["host"]["ms_call_wall"]

    # ---- the migration ----
    has_tables = hasattr(S.fp[0], "dd_winds_clear")
    for fp in S.fp:
        if has_tables:
            fp.dd_winds_clear()
    pos0 = pr.ic["pos"].copy()
    movers = rng.choice(n, n // 20, replace=False)
    pos1 = pos0.copy()
    pos1[movers] = pos0[rng.permutation(movers)] + 1e-5

    def migrate():
        nx = 0
        for fp in S.fp:
            fp.dd_begin(B.DD_MIGRATE, None, 0)
        while True:
            rcs = [fp.dd_step() for fp in S.fp]
            if rcs[0] == 0:
                break
            B.dd_exchange_local(S.fp)
            nx += 1
        for r, fp in enumerate(S.fp):
            cn, ngl = fp.counts()
            S.gid[r] = fp.get_field(B.F_ID).astype(np.int64)
            S.ngas[r] = ngl
            S.owner[S.gid[r]] = r
        return nx

    mig = {"with_tables": [], "without": [], "without_again": []}
    for rep in range(a.reps + 1):
        for side in (("without",) if only_mig else ("with_tables", "without", "without_again")):
            S.set_field(B.F_POS, pos0)
            migrate()                                         # everybody home
            for r, fp in enumerate(S.fp):
                if side == "with_tables":
                    loc, at = S.locate(wind)[r]
                    fp.dd_winds_set_table(loc, rows[at])
                elif has_tables:
                    fp.dd_winds_clear()
            S.set_field(B.F_POS, pos1)
            for fp in S.fp:
                fp.sync()
            begin()
            t0 = time.perf_counter()
            nx = migrate()
            for fp in S.fp:
                fp.sync()
            wall = (time.perf_counter() - t0) * 1e3
            moved = sum(fp.dd_info()["migrated_out"] for fp in S.fp)
            held = sum(len(fp.dd_winds_table()[0]) for fp in S.fp) if side == "with_tables" else 0
            mig[side].append((wall, nx, end()[1], moved, held))
    out["migration"] = {}
    for side, v in mig.items():
        if not v:
            continue
        med = np.median(np.array(v[1:]), axis=0)
        out["migration"][side] = {"ms_wall": med[0], "exchanges": int(med[1]), "launches_all_shards": int(med[2]),
                                  "particles_moved": int(med[3]), "rows_held_after": int(med[4])}
    S.close()
    if not only_mig:
        out["spawn"] = spawn_part(B, P, a.ng, a.reps)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
