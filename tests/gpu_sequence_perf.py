"""Measurement tool (not a test): ghip_rearrange / ghip_peano_order on a memory-shuffled state with 1 % massless
records, next to the host round trip they replace, and the resident step from shuffled and from ordered memory.

    python tests/gpu_sequence_perf.py [--sizes 64,128] [--reps 3] [--step-ng 64] [--out FILE]

Every timed region ends with a synchronisation inside the clock (the calls synchronise themselves; the step ends
with sync()), every shape is run once untimed first, and the versions compared are alternated inside one run.
Prints one JSON line per measurement; DESIGN.md 4.19 records the numbers."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reuse_cases as RC  # noqa: E402
from common import Problem, bindings  # noqa: E402

B = bindings()
PEAK = 6.3e12   # achievable HBM rate, bytes / s


def shuffled_state(ng, seed=1, massless=0.01):
    """{field: array} of a periodic gas + dark matter problem whose two blocks are shuffled in memory"""
    pr = Problem(ng=ng, gas=True, periodic=1)
    rng = np.random.default_rng(seed)
    n, ngas = pr.n, pr.ngas
    perm = np.concatenate([rng.permutation(ngas), ngas + rng.permutation(n - ngas)])
    mass = pr.ic["mass"].copy()
    mass[rng.random(n) < massless] = 0.0
    per_particle = {B.F_POS: pr.ic["pos"], B.F_VEL: pr.ic["vel"], B.F_MASS: mass, B.F_TYPE: pr.ic["type"],
                    B.F_HSML: pr.hsml0, B.F_TIMEBIN: pr.timebin, B.F_TI_BEGSTEP: pr.ti_begstep,
                    B.F_ID: np.arange(n, dtype=np.int32)}
    per_gas = {B.F_VELPRED: pr.velpred, B.F_ENTROPY: pr.entropy, B.F_DTENTROPY: pr.dtentropy}
    st = {f: np.ascontiguousarray(a[perm]) for f, a in per_particle.items()}
    st.update({f: np.ascontiguousarray(a[perm[:ngas]]) for f, a in per_gas.items()})
    return pr, st


def load(fp, pr, st, n=None, ngas=None):
    fp.set_counts(pr.n if n is None else n, pr.ngas if ngas is None else ngas)
    for f, a in st.items():
        fp.set_field(f, a)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def host_round_trip(fp):
    """the only way through a decomposition without the two calls: every field and the keys to the host, the
    compaction and the two stable sorts there, set_counts and every field back"""
    n, ngas = fp.n, fp.ngas
    f = {k: fp.get_field(k) for k in range(B.F_COUNT)}
    key = fp.dd_keys()
    keep = f[B.F_MASS] != 0
    idx = np.arange(n)
    gas = idx[keep & (idx < ngas)]
    oth = idx[keep & (idx >= ngas)]
    gas, oth = gas[np.argsort(key[gas], kind="stable")], oth[np.argsort(key[oth], kind="stable")]
    order = np.concatenate([gas, oth])
    fp.set_counts(len(order), len(gas))
    for k, a in f.items():
        fp.set_field(k, a[gas] if B._FIELD_INFO[k][0] else a[order])


def part_calls(ng, reps, emit):
    pr, st = shuffled_state(ng)
    corner, dlen = pr.extent[0], pr.extent[2]
    fp = B.ForcePath(0)
    fp.dd_set_domain(pr.extent[0], pr.extent[1], pr.extent[2], pr.force_soft)   # (for dd_keys of the round trip)
    res = {"rearrange": [], "order": [], "order_sorted": [], "host": []}
    info = {}
    for rep in range(reps + 1):               # rep 0 warms every shape
        load(fp, pr, st)
        fp.sync()
        t_re, r = clock(lambda: fp.rearrange())
        info["rearrange"] = fp.sequence_info()
        t_or, ch = clock(lambda: fp.peano_order(corner, dlen))
        info["order"] = fp.sequence_info()
        t_os, ch2 = clock(lambda: fp.peano_order(corner, dlen))      # keys + sort + compare, nothing moves
        assert r.changed and ch and not ch2
        load(fp, pr, st)
        fp.sync()
        t_h, _ = clock(lambda: host_round_trip(fp))
        if rep:
            for k, v in (("rearrange", t_re), ("order", t_or), ("order_sorted", t_os), ("host", t_h)):
                res[k].append(v)
    med = {k: float(np.median(v)) for k, v in res.items()}
    for k in ("rearrange", "order"):
        b = info[k]["bytes_moved"]
        emit(dict(what=k, n=pr.n, ngas=pr.ngas, ms=med[k], all_ms=res[k], bytes_moved=b, planes=info[k]["planes"],
                  share_of_peak=b / (med[k] * 1e-3) / PEAK))
    emit(dict(what="order, already ordered (keys, sort, compare; no move)", n=pr.n, ms=med["order_sorted"],
              all_ms=res["order_sorted"], share_of_the_order_call=med["order_sorted"] / med["order"]))
    emit(dict(what="host round trip (get_field all + keys, compaction and sorts on the host, set_counts, set_field all)",
              n=pr.n, ms=med["host"], all_ms=res["host"],
              ratio_to_both_calls=med["host"] / (med["rearrange"] + med["order"])))
    fp.close()


def step(fp, pr):
    pr.device_tree(fp)
    fp.set_field(B.F_OLDACC, np.zeros(fp.n))
    fp.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON_EWALD)
    fp.density(pr.g_dens())
    fp.update_hmax()
    fp.hydro(pr.g_hydro())
    fp.sync()


def results(fp):
    ids = fp.get_field(B.F_ID)
    inv = np.argsort(ids)
    gas = np.argsort(ids[:fp.ngas])
    return dict(acc=fp.get_field(B.F_GRAVACCEL)[inv], cost=fp.get_field(B.F_GRAVCOST)[inv],
                density=fp.get_field(B.F_DENSITY)[gas], hsml=fp.get_field(B.F_HSML)[inv],
                numngb=fp.get_field(B.F_NUMNGB)[gas], hydroaccel=fp.get_field(B.F_HYDROACCEL)[gas],
                pairs=fp.stats()["hydro_pairs"])


def part_step(ng, reps, emit):
    pr, st = shuffled_state(ng, massless=0.0)
    corner, dlen = pr.extent[0], pr.extent[2]
    ctx = {"shuffled": B.ForcePath(0), "ordered": B.ForcePath(0)}
    for fp in ctx.values():
        load(fp, pr, st)
        fp.ewald_init(pr.box)
    assert ctx["ordered"].peano_order(corner, dlen)
    keys = ("ms_tree", "ms_grav", "ms_ewald", "ms_dens", "ms_hydro")
    t = {k: [] for k in ctx}
    parts = {k: [] for k in ctx}
    out = {}
    for rep in range(reps + 1):
        for name, fp in ctx.items():          # alternated
            fp.set_field(B.F_HSML, _by_id(st, fp, B.F_HSML))     # every step starts from the same guess
            fp.sync()
            ms, _ = clock(lambda: step(fp, pr))
            if rep:
                t[name].append(ms)
                s = fp.stats()
                parts[name].append([s[k] for k in keys])
            out[name] = results(fp)
    bad = RC.compare(out["ordered"], out["shuffled"], 1)
    for name in ctx:
        emit(dict(what="step from %s memory" % name, n=pr.n, ms=float(np.median(t[name])), all_ms=t[name],
                  kernels=dict(zip(keys, np.median(np.array(parts[name]), axis=0).tolist()))))
    emit(dict(what="ordered / shuffled", ratio=float(np.median(t["ordered"]) / np.median(t["shuffled"])),
              outputs_that_differ_per_id=bad, rules="tests/reuse_cases.py:RULES, column 1"))
    for fp in ctx.values():
        fp.close()


def _by_id(st, fp, field):
    """the initial values of `field` in the context's present order"""
    first = np.empty(len(st[B.F_ID]), np.int64)
    first[st[B.F_ID]] = np.arange(len(first))
    return st[field][first[fp.get_field(B.F_ID)]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-ng", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sink = open(a.out, "w") if a.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    for ng in [int(s) for s in a.sizes.split(",") if s]:
        part_calls(ng, a.reps, emit)
    if a.step_ng:
        part_step(a.step_ng, a.reps, emit)


if __name__ == "__main__":
    main()
