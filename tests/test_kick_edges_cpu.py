"""The inputs of tests/kick_edges.py judged on the CPU: every label of kick_ref's trace is carried by at least 8
particles over the runs, the comoving kick intervals reach the first two table cells, the interior and the end clamp,
kick_ref equals the oracle's advance_timesteps on the flag-free runs (integers exactly, floats at the levels of
test_timestep_and_kick_parity) and its drift on the drift cases, each endrun case fails with its code because of one
particle, and the drift cases hold what they were built for (no-ops, both sides of MinGasHsml, the wrap edges).
No GPU: this is the gate for tests/test_gpu_kick_edges.py."""
from collections import Counter

import numpy as np
import pytest

import kick_edges as E
import kick_ref as R
from common import O, relerr
from test_kick_bundle_cpu import oracle_params

_RUNS = {}


def runs(comoving):
    """the runs with kick_ref's result, computed once: [(run, state after, out, trace)]"""
    if comoving not in _RUNS:
        _RUNS[comoving] = [(r,) + E.run_reference(r) for r in E.kick_edge_case(comoving)]
    return _RUNS[comoving]


def test_every_label_is_carried_by_eight_particles():
    count = Counter()
    for comoving in (False, True):
        for run, s, out, trace in runs(comoving):
            assert out["rc"] == 0, run["name"]
            n = len(s["type"])
            assert len(trace) == (n if run["active"] is None else len(run["active"]))
            count.update(l for labels in trace.values() for l in labels)
            if run["name"] == "end":
                assert all("end" in v for v in trace.values()) and len(trace) == n
                assert not s["timebin"].any() and np.all(s["ti_begstep"] == R.TIMEBASE)
            if run["name"] == "t0":
                assert all("binold0" in v and "up" in v for v in trace.values())
    print({k: count[k] for k in R.KICK_LABELS})
    for label in R.KICK_LABELS:
        assert count[label] >= 8, (label, count[label])


def test_the_consistent_timeline_and_the_table_cells():
    for comoving in (False, True):
        cells = set()
        for run, s, out, trace in runs(comoving):
            b = run["s"]
            act = np.arange(len(b["type"])) if run["active"] is None else run["active"]
            step = np.where(b["timebin"] > 0, 1 << b["timebin"].astype(np.int64), 0)
            assert np.all(b["ti_begstep"][act] + step[act] == run["p"]["Ti_Current"]), run["name"]
            if run["active"] is not None:
                assert np.all((run["p"]["TimeBinActive"] >> b["timebin"][act]) & 1)
                rest = np.setdiff1d(np.arange(len(b["type"])), act)
                assert len(rest) >= 8 and not np.any((run["p"]["TimeBinActive"] >> b["timebin"][rest]) & 1)
            if comoving:
                cells |= E.table_cells(run, b, s)
        if comoving:
            assert cells == {"first", "interior", "clamp"}
    # MaxSizeTimestep can win in one parameter set only
    p = {r["name"]: r["p"] for r in E.kick_edge_case(False)}
    assert p["mid-max"]["MaxSizeTimestep"] < p["mid-max"]["dt_displacement"]
    assert p["mid-disp"]["MaxSizeTimestep"] > p["mid-disp"]["dt_displacement"]


@pytest.mark.parametrize("comoving", [False, True])
def test_kick_ref_equals_the_oracle_on_the_flag_free_runs(comoving):
    for run, s, out, trace in runs(comoving):
        if not run["flagfree"]:
            continue
        b = run["s"]
        ng = len(b["entropy"])
        want = O.advance_timesteps(oracle_params(run["p"]), b["type"], b["vel"], b["grav"], b["hyd"], b["velpred"],
                                   b["entropy"], b["dtentropy"], b["density"], np.zeros(ng), b["hsml"][:ng],
                                   b["vsig"], b["timebin"], b["ti_begstep"], active=run["active"],
                                   tables=run["tables"])
        assert want["rc"] == 0, run["name"]
        for k in ("timebin", "ti_begstep", "vel", "velpred"):
            assert np.array_equal(s[k], want[k]), (run["name"], k)
        assert np.array_equal(want["bincount"][:30], np.bincount(s["timebin"], minlength=30))
        assert np.array_equal(want["bincount_sph"][:30], np.bincount(s["timebin"][:ng], minlength=30))
        if comoving:
            assert relerr(s["entropy"], want["entropy"]) < 1e-14, run["name"]
            assert np.abs(s["dtentropy"] - want["dtentropy"]).max() <= 1e-14 * np.abs(want["dtentropy"]).max()
        else:
            assert np.array_equal(s["entropy"], want["entropy"]), run["name"]
            assert np.array_equal(s["dtentropy"], want["dtentropy"]), run["name"]


def test_endrun_cases_fail_by_one_particle_with_the_code():
    names = []
    for name, code, p, s, i in E.endrun_cases():
        names.append(name)
        bad = E.copy_state(s)
        assert R.advance_timesteps(p, R.flags(), bad)["rc"] == code, name
        trace = {}
        act = np.setdiff1d(np.arange(len(s["type"])), [i])
        assert R.advance_timesteps(p, R.flags(), E.copy_state(s), active=act, trace=trace)["rc"] == 0, name
        assert len(trace) == len(act)
        ng = len(s["entropy"])
        want = O.advance_timesteps(oracle_params(p), s["type"], s["vel"], s["grav"], s["hyd"], s["velpred"],
                                   s["entropy"], s["dtentropy"], s["density"], np.zeros(ng), s["hsml"][:ng], s["vsig"],
                                   s["timebin"], s["ti_begstep"])
        assert want["rc"] == code, name
    assert names == ["888-min", "818", "112313", "888-end"]


@pytest.mark.parametrize("comoving", [False, True])
@pytest.mark.parametrize("box", [1.0, 2.5])
@pytest.mark.parametrize("when", E.DRIFT_WHEN)
def test_drift_case_holds_what_it_was_built_for_and_equals_the_oracle(comoving, box, when):
    c = E.drift_edge_case(comoving, box, when)
    b = c["s"]
    s, p, (clamped, free) = E.drift_reference(c)
    n, ng = len(b["type"]), len(b["entropy"])
    assert clamped >= 8 and free >= 8
    assert n // 4 <= len(c["noop"]) <= n // 2
    plain = np.setdiff1d(c["noop"], c["wrapset"])
    for k in ("pos", "vel", "ti_current"):
        assert np.array_equal(s[k][plain], b[k][plain]), k
    gas = plain[plain < ng]
    for k in ("velpred", "density", "pressure"):
        assert np.array_equal(s[k][gas], b[k][gas]), k
    assert np.array_equal(s["hsml"][plain], b["hsml"][plain])
    assert np.all(s["ti_current"] == c["time1"])
    assert (s["pos"] >= 0).all() and (s["pos"] < box).all()
    # the wrap edges, row by row: -1e-17 and BoxSize give 0.0; the far coordinates take several turns of the loops
    w = s["pos"][c["wrapset"][:E.WRAP_ROWS], 0]
    assert np.array_equal(w, [0.0, 0.0, 0.75 * box, 0.5 * box, 0.25 * box, 0.0, 0.0, np.nextafter(box, 0.0)])
    if not comoving:
        assert len(c["wrapset"]) == E.WRAP_ROWS + 7
        assert np.array_equal(s["pos"][c["wrapset"][E.WRAP_ROWS:], 0], w[:7])
    if comoving:    # where the intervals lie on the tables
        u = lambda t: int(t * p["Timebase_interval"] / (p["logTimeMax"] - p["logTimeBegin"]) * R.TABLE)
        u0, u1 = [u(int(t)) for t in np.unique(b["ti_current"])], u(c["time1"])
        if when == "first":     # i == 1 at both ends of an interval, i == 0 at a start
            assert u1 == 1 and sorted(u0) == [0, 1, 1]
        elif when == "interior":
            assert 1 < min(u0) and u1 < R.TABLE
        else:
            assert u1 >= R.TABLE and min(u0) <= 1 < max(u for u in u0 if u < R.TABLE)
    want = O.drift(c["time1"], p["Timebase_interval"], b["pos"], b["vel"], b["type"], b["ti_current"], b["timebin"],
                   b["ti_begstep"], b["grav"], b["velpred"], b["hyd"], b["density"], b["hsml"][:ng], b["divvel"],
                   b["entropy"], b["dtentropy"], b["pressure"], minhsml=p["MinGasHsml"], wrap=True, boxsize=box,
                   tables=c["tables"], log_time_begin=p["logTimeBegin"], log_time_max=p["logTimeMax"])
    assert want["rc"] == 0
    assert np.array_equal(want["ti_current"], s["ti_current"])
    assert np.array_equal(want["pos"], s["pos"])
    for k in ("velpred", "density", "pressure"):
        assert np.array_equal(want[k], s[k]), k
    assert np.array_equal(want["hsml"], s["hsml"][:ng])
