"""GHIP_DD_DECOMPOSE (domain_Decomposition on shards, include/ghip.h): the key ranges -- and on request the
domain cube -- are computed from the resident particles of all shards, no shard ever sees another shard's
keys.  Several logical shards on one GPU (ghip_dd_exchange_local), two rank processes through the host's
all-gather and through the RCCL entry points (tests/mock_rccl).  Checked against the NumPy restatement
tests/decomp_ref.py and against the host cut sharded.decompose of the keys of all particles."""
import importlib
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import decomp_ref as DR
from common import Problem, ShardSet, bindings, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-11


def sharded():
    return importlib.import_module("gadget-leicester_amd.sharded")


def seeded_work(n, seed=77):
    """GravCost < 5000, TimeBin in 8..24 with 1 % zeros (bin 0 costs (1 + GravCost) / 2^29): times 2^29 the
    reference's float weights are integers below 2^34, their sums over a few thousand particles exact"""
    rng = np.random.default_rng(seed)
    cost = rng.integers(0, 5000, n).astype(np.int32)
    tbin = rng.integers(8, 25, n).astype(np.int32)
    tbin[rng.random(n) < 0.01] = 0
    return cost, tbin


def float_work(cost, tbin):
    return (1.0 + cost) / 2.0 ** DR.effective_bins(tbin)


def params(level=0, use_work=0, find_extent=0):
    return bindings().DecompParams(level, use_work, find_extent, 0)


def all_splits(S):
    sp = S.each(lambda fp: fp.dd_get_splits())
    for s in sp[1:]:
        assert s.tobytes() == sp[0].tobytes(), "the shards hold different splits"
    return sp[0]


def owners_follow_the_keys(S, splits, keys):
    """every particle sits on the shard its key names (who holds what: read through F_ID by ShardSet.migrate)"""
    assert np.array_equal(np.sort(np.concatenate(S.gid)), np.arange(S.pr.n))
    for r, g in enumerate(S.gid):
        want = np.searchsorted(splits[1:S.P], keys[g], side="right")
        assert np.all(want == r), r


@pytest.mark.parametrize("nshards,ng", [(2, 12), (3, 16), (8, 12)])
def test_splits_equal_the_restatement_and_the_host_cut(nshards, ng):
    B, sh = bindings(), sharded()
    pr = Problem(ng=ng, gas=True, periodic=1)
    cost, tbin = seeded_work(pr.n)
    S = ShardSet(pr, nshards)            # the unweighted host cut
    try:
        S.set_field(B.F_GRAVCOST, cost)
        S.set_field(B.F_TIMEBIN, tbin)
        pos = pr.ic["pos"]
        for level in (0, 2, 3):
            for use_work in (1, 0):
                S.run.decompose(params(level, use_work))
                got = all_splits(S)
                ref, _, keys = DR.decompose(pos, nshards, level, cost if use_work else None, tbin, domain=pr.extent)
                assert np.array_equal(keys, S.keys)
                host, _ = sh.decompose(S.keys, nshards, float_work(cost, tbin) if use_work else None,
                                       level=level or None)
                print("P=%d level=%d use_work=%d splits %s" % (nshards, level, use_work, [hex(int(v)) for v in got]))
                assert np.array_equal(got, ref), (level, use_work)
                assert np.array_equal(got, host), (level, use_work)
                assert got[0] == 0 and got[-1] == 1 << 63
                # ... the all-gathers of the 128-byte block and of the histogram, and nothing else
                L = level or DR.histogram_level(pr.n, nshards)
                assert S.fp[0].dd_bytes_sent(B.DD_DECOMPOSE) == (nshards - 1) * (128 + 8 ** L * 8)
        # the weighted cut differs from the unweighted one the shards started from, or the test shows nothing
        S.run.decompose(params(0, 1))
        assert not np.array_equal(all_splits(S), S.splits)
    finally:
        S.close()


def test_splits_do_not_depend_on_who_holds_what():
    B = bindings()
    pr = Problem(ng=12, gas=True, periodic=1)
    cost, tbin = seeded_work(pr.n, 5)
    res = []
    for layout in ("equal-width", "host-cut"):
        S = ShardSet(pr, 3)
        try:
            S.set_field(B.F_GRAVCOST, cost)
            S.set_field(B.F_TIMEBIN, tbin)
            if layout == "equal-width":
                # the ranges of ghip_dd_init's default: a third of the key space each
                for r, fp in enumerate(S.fp):
                    fp.dd_init(r, 3)
                S.migrate()
                assert sum(len(g) for g in S.gid) == pr.n
            S.run.decompose(params(0, 1))
            first = [fp.dd_get_splits().tobytes() for fp in S.fp]
            S.run.decompose(params(0, 1))
            again = [fp.dd_get_splits().tobytes() for fp in S.fp]
            assert first == again and len(set(first)) == 1
            res.append(first[0])
        finally:
            S.close()
    assert res[0] == res[1]


def test_decompose_migrate_gravity_is_the_single_trees_step():
    B = bindings()
    pr = Problem(ng=12, gas=True, periodic=1)
    n = pr.n
    cost, tbin = seeded_work(n, 9)
    S = ShardSet(pr, 3)
    S2 = None
    try:
        S.set_field(B.F_GRAVCOST, cost)
        S.set_field(B.F_TIMEBIN, tbin)
        S.run.decompose(params(0, 1))
        splits = all_splits(S)
        before = S.owner.copy()
        S.migrate()
        assert int((S.owner != before).sum()) > 0, "the weighted cut moved nobody: the test shows nothing"
        owners_follow_the_keys(S, splits, S.keys)
        for r, fp in enumerate(S.fp):
            k = fp.dd_keys()
            assert np.all((k >= splits[r]) & (k < splits[r + 1]))
        S.set_field(B.F_OLDACC, np.zeros(n))
        S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
        # a set of shards built directly on those splits
        S2 = ShardSet(pr, 3, work=float_work(cost, tbin))
        assert np.array_equal(S2.splits, splits)
        S2.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
        assert np.array_equal(S.get_field(B.F_GRAVCOST), S2.get_field(B.F_GRAVCOST))
        assert S.get_field(B.F_GRAVCOST).min() > 0
        err = relerr(S.get_field(B.F_GRAVACCEL), S2.get_field(B.F_GRAVACCEL))
        print("accelerations after decompose + migrate against shards built on the splits: %.3e" % err)
        assert err < TOL
    finally:
        S.close()
        if S2 is not None:
            S2.close()


def test_extent_of_particles_that_left_the_cube():
    B = bindings()
    pr = Problem(ng=12, gas=True, periodic=0)
    n = pr.n
    S = ShardSet(pr, 2)
    try:
        rng = np.random.default_rng(31)
        pos = pr.ic["pos"].copy()
        out = rng.choice(n, n // 100, replace=False)
        axis = rng.integers(0, 3, len(out))
        sign = rng.choice([-1.0, 1.0], len(out))
        pos[out, axis] = pr.extent[1][axis] + sign * (0.55 + 0.3 * rng.random(len(out))) * pr.extent[2]
        S.set_field(B.F_POS, pos)
        S.set_field(B.F_OLDACC, np.zeros(n))
        # without a fresh extent: the decomposition says so on all shards, and -- as before -- the migration
        # keeps the leavers in the boundary cells and the next force computation is refused
        with pytest.raises(B.GhipError) as e:
            S.run.decompose(params(0, 0, find_extent=0))
        assert "domain cube" in str(e.value)
        S.migrate()
        with pytest.raises(B.GhipError) as e:
            S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
        assert "domain cube" in str(e.value) or "reported an error" in str(e.value)
        # with it
        S.run.decompose(params(0, 0, find_extent=1))
        want = DR.extent(pos)
        for fp in S.fp:
            corner, center, ln = fp.dd_get_domain()
            assert corner.tobytes() == want[0].tobytes() and center.tobytes() == want[1].tobytes()
            assert ln == want[2]
        ref, _, keys = DR.decompose(pos, 2, 0)
        splits = all_splits(S)
        assert np.array_equal(splits, ref)
        S.migrate()
        owners_follow_the_keys(S, splits, keys)
        S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
        # a fresh single-GPU path built on that extent
        pr2 = Problem(ng=12, gas=True, periodic=0)
        pr2.ic["pos"] = pos
        pr2.extent = want
        fp = pr2.device()
        try:
            pr2.device_tree(fp)
            fp.set_field(B.F_OLDACC, np.zeros(n))
            fp.gravity(pr2.g_grav(pr.theta), B.WALK_NEWTON)
            assert np.array_equal(S.get_field(B.F_GRAVCOST), fp.get_field(B.F_GRAVCOST))
            err = relerr(S.get_field(B.F_GRAVACCEL), fp.get_field(B.F_GRAVACCEL))
            print("accelerations on the found extent against the single GPU: %.3e" % err)
            assert err < TOL
        finally:
            fp.close()
    finally:
        S.close()


def test_all_particles_in_one_cell_and_empty_shards():
    B = bindings()
    pr = Problem(ng=12, gas=True, periodic=1)
    n = pr.n
    S = ShardSet(pr, 3)
    try:
        rng = np.random.default_rng(4)
        pos = pr.extent[0] + pr.extent[2] * (0.3 + 1e-4 * rng.random((n, 3)))   # one cell of level 3
        S.set_field(B.F_POS, pos)
        S.run.decompose(params(3, 0))
        splits = all_splits(S)
        ref, _, keys = DR.decompose(pos, 3, 3, domain=pr.extent)
        assert len(np.unique(keys >> np.uint64(63 - 9))) == 1
        assert np.array_equal(splits, ref)
        assert np.all(np.diff(splits.astype(np.float64)) >= 0) and splits[0] == 0 and splits[-1] == 1 << 63
        S.migrate()
        owners_follow_the_keys(S, splits, keys)
        sizes = sorted(len(g) for g in S.gid)
        assert sizes == [0, 0, n]
        # shards that hold nothing take part: same splits again, with and without work, and a finer level
        S.set_field(B.F_GRAVCOST, np.full(n, 7, np.int32))
        S.run.decompose(params(3, 1))
        assert np.array_equal(all_splits(S), splits)
        S.run.decompose(params(5, 0))
        assert np.array_equal(all_splits(S), DR.decompose(pos, 3, 5, domain=pr.extent)[0])
        S.migrate()
        assert sorted(len(g) for g in S.gid) == [0, 0, n]
    finally:
        S.close()


def test_refusals_leave_the_shards_usable():
    B = bindings()
    pr = Problem(ng=12, gas=True, periodic=1)
    n = pr.n
    S = ShardSet(pr, 8)
    S9 = None
    try:
        # 8^L < nranks needs more than 8 ranks: nine contexts, nothing resident
        S9 = [B.ForcePath(0) for _ in range(9)]
        for r, fp in enumerate(S9):
            fp.set_counts(0, 0)
            fp.dd_init(r, 9)
            fp.dd_set_domain(pr.extent[0], pr.extent[1], pr.extent[2], pr.force_soft)
        with pytest.raises(B.GhipError) as e:
            S9[0].dd_begin(B.DD_DECOMPOSE, params(1))
        assert "fewer than the 9 ranks" in str(e.value)
        S9[0].dd_begin(B.DD_DECOMPOSE, params(2))       # 64 cells: accepted (and abandoned)
        for bad in (8, -1):
            with pytest.raises(B.GhipError) as e:
                S.fp[0].dd_begin(B.DD_DECOMPOSE, params(bad))
            assert "level" in str(e.value)
        # a pending exchange of another operation
        for fp in S.fp:
            fp.dd_begin(B.DD_MIGRATE, None)
        assert [fp.dd_step() for fp in S.fp] == [1] * 8
        with pytest.raises(B.GhipError) as e:
            S.fp[0].dd_begin(B.DD_DECOMPOSE, params())
        assert "pending" in str(e.value)
        B.dd_exchange_local(S.fp)
        assert [fp.dd_step() for fp in S.fp] == [0] * 8
        # a position that is not a number, on one shard: all shards fail together, with one message
        good = all_splits(S)
        r_bad = 5
        local = S.fp[r_bad].get_field(B.F_POS)
        broken = local.copy()
        broken[len(broken) // 2, 1] = np.nan
        S.fp[r_bad].set_field(B.F_POS, broken)
        for fp in S.fp:
            fp.dd_begin(B.DD_DECOMPOSE, params(0, 0, find_extent=1))
        assert [fp.dd_step() for fp in S.fp] == [1] * 8
        B.dd_exchange_local(S.fp)
        msgs = []
        for fp in S.fp:
            with pytest.raises(B.GhipError) as e:
                fp.dd_step()
            msgs.append(str(e.value))
        assert len(set(msgs)) == 1 and "not finite" in msgs[0] and "shard 5" in msgs[0]
        assert np.array_equal(all_splits(S), good)       # nothing was changed
        for fp in S.fp:                                  # no exchange is pending, no operation in progress
            with pytest.raises(B.GhipError) as e:
                fp.dd_step()
            assert "no operation in progress" in str(e.value)
        # ... and the next valid call succeeds
        S.fp[r_bad].set_field(B.F_POS, local)
        S.run.decompose(params(0, 0, find_extent=1))
        ref, dom, _ = DR.decompose(pr.ic["pos"], 8, 0)
        assert np.array_equal(all_splits(S), ref)
        assert S.fp[0].dd_get_domain()[2] == dom[2]
    finally:
        S.close()
        for fp in S9 or []:
            fp.close()


def _run_ranks(transport):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", DECOMP_TRANSPORT=transport)
    if transport == "rccl":
        mock = os.path.join(root, "tests", "mock_rccl", "librccl_mock.so")
        assert os.path.exists(mock), "build tests/mock_rccl first (__graft_entry__.build())"
        env["GHIP_RCCL_LIB"] = mock
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "tests", "gpu_host_ranks_decomp.py")]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("transport", ["host", "rccl"])
def test_two_rank_processes_redistribute_without_seeing_each_others_keys(transport):
    """tests/gpu_host_ranks_decomp.py is the rank program: every rank holds the particles it was dealt (every
    second one), runs redistribute and GHIP_DD_GRAVITY; rank 0 gathers and compares with the in-process run.
    "host": the exchanges go through the host's all-gather (gloo); "rccl": through the RCCL entry points,
    supplied by tests/mock_rccl as in test_gpu_dd.py (the real RCCL refuses two ranks on one device)."""
    out = _run_ranks(transport)
    assert out["ok"], out
    assert out["transport"] == transport
    if transport == "rccl":
        assert out["rccl_library"].endswith("librccl_mock.so")
    assert out["splits_equal_in_process"] and out["splits_equal_on_ranks"] and out["splits_equal_restatement"]
    assert out["domain_equal_restatement"]
    assert out["moved"] > 0 and out["nobody_lost"] and out["owners_follow_keys"]
    assert out["gravcost_equal"]
    assert out["rel_accel"] < TOL
    assert out["bytes_decompose"] == 128 + 8 ** out["level"] * 8
