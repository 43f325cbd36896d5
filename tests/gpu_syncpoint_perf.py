"""What a sync point costs between two steps of a resident run (a measurement script, not a test):

  host form    get_field(TIMEBIN), get_field(TI_BEGSTEP), the rule in NumPy, set_active  -- what a caller had to do
  device form  find_next_sync_point                                                      -- ghip_sync.hip

at the c2 size (524 288 particles, time bins spread over four values) for active fractions of about 1, 1/4 and
1/64.  Per fraction: warm-up, then the two forms in turn, REPS times each; wall-clock around calls that end in a
device synchronise; medians with the 10th / 90th percentile.  Both forms must leave the same list.  Also the
launches and blocking host waits of one device-form call between the marks of a step (the library's own
counters, ghip_run_stats: its kernels, and every wait of the host for the device including ghip_run_end's).
Prints one JSON line; --out FILE keeps it.

    python tests/gpu_syncpoint_perf.py [--n 524288] [--reps 40] [--warmup 5] [--out FILE]
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

# (label, the four bins, their shares, Ti_Current): the bins that 2^b | Ti_next are active
CASES = (("1", (3, 4, 5, 6), (0.25, 0.25, 0.25, 0.25), 63),          # -> 64: everybody
         ("1/4", (3, 5, 6, 9), (0.25, 0.25, 0.25, 0.25), 8),        # -> 16: bin 3
         ("1/64", (3, 5, 6, 9), (1 / 64, 21 / 64, 21 / 64, 21 / 64), 8))


def host_form(fp, B, n):
    tb = fp.get_field(B.F_TIMEBIN)
    beg = fp.get_field(B.F_TI_BEGSTEP)
    ends = beg + np.where(tb > 0, np.left_shift(1, tb), 0)
    ti_next = int(ends.min())
    act = np.nonzero(ends == ti_next)[0].astype(np.int32)
    fp.set_active(None if len(act) == n else act)
    return ti_next


def stats(ms):
    a = np.sort(np.array(ms))
    return {"median_ms": float(np.median(a)), "p10_ms": float(a[int(0.1 * (len(a) - 1))]),
            "p90_ms": float(a[int(round(0.9 * (len(a) - 1)))])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=524288)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from common import bindings
    B = bindings()
    n, rng = a.n, np.random.default_rng(3)
    fp = B.ForcePath(0)
    fp.set_counts(n, n // 2)
    fp.set_field(B.F_TYPE, (np.arange(n) >= n // 2).astype(np.int32))
    out = {"n": n, "reps": a.reps, "warmup": a.warmup, "cases": []}
    for label, bins, shares, ti in CASES:
        tb = rng.choice(np.array(bins, np.int32), n, p=np.array(shares)).astype(np.int32)
        fp.set_field(B.F_TIMEBIN, tb)
        fp.set_field(B.F_TI_BEGSTEP, ((ti >> tb) << tb).astype(np.int32))
        t_host, t_dev = [], []
        for rep in range(a.warmup + a.reps):
            fp.set_active(np.zeros(1, np.int32))        # (neither form finds the list it is about to make)
            fp.sync()
            t0 = time.perf_counter()
            ti_host = host_form(fp, B, n)
            t1 = time.perf_counter()
            list_host = fp.get_active()
            fp.set_active(np.zeros(1, np.int32))
            fp.sync()
            t2 = time.perf_counter()
            sp = fp.find_next_sync_point(ti)
            t3 = time.perf_counter()
            if rep == 0:
                assert sp.Ti_next == ti_host and np.array_equal(fp.get_active(), list_host), label
            if rep >= a.warmup:
                t_host.append(1e3 * (t1 - t0))
                t_dev.append(1e3 * (t3 - t2))
        out["cases"].append({"active_fraction": label, "active": int(sp.NumForceUpdate), "Ti_next": int(sp.Ti_next),
                             "host_form": stats(t_host), "device_form": stats(t_dev)})
    # one device-form call between the marks of a step: the library's own counters (last, so that nothing runs
    # behind a step that recorded no phase event)
    fp.run_begin(2)
    fp.step_begin()
    fp.find_next_sync_point(ti)
    fp.step_end()
    rs = fp.run_end()
    out["device_form_launches"], out["device_form_blocking_syncs"] = int(rs["launches"]), int(rs["blocking_syncs"])
    fp.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
