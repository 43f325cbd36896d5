"""ghip_find_next_sync_point / ghip_get_active / ghip_find_extent on the device, and the sync point of shards
(GHIP_DD_DECOMPOSE begun with walk = SYNC_POINT_FORM), against tests/sync_ref.py (run.c:199-320) and the
oracle's loop.  Everything is integer or a copy of the oracle's arithmetic: the comparisons are exact unless a
bound of an existing test is named."""
import ctypes as C

import numpy as np
import pytest

import sync_ref as SR
from common import O, Problem, ShardSet, bindings, failing_collective, relerr
from test_gpu_parity import _fill

pytestmark = pytest.mark.gpu
TOL = 1e-11          # the shard-comparison bound of test_gpu_dd.py

BIN_SETS = ([0, 3, 5, 6, 9], [3, 5], [5, 6, 9], [0], [3, 5, 6, 9])
TI_CURRENT = (0, 8, 24, 32, 96)


def _bare(n, seed):
    """a context that holds only what the sync point reads: mixed types (gas in front) and time bins"""
    B = bindings()
    rng = np.random.default_rng(seed)
    ngas = n // 3
    typ = np.concatenate([np.zeros(ngas, np.int32), rng.integers(1, 6, n - ngas).astype(np.int32)])
    fp = B.ForcePath(0)
    fp.set_counts(n, ngas)
    fp.set_field(B.F_TYPE, typ)
    return B, fp, typ, rng


@pytest.mark.parametrize("n", [1, 63, 777, 66000])
def test_rule_and_list_against_the_restatement(n):
    """one lane, less than a wavefront, a ragged tail, 65 blocks of 1024 (the block offsets); bins drawn from
    {0, 3, 5, 6, 9} with some left empty; every member of ghip_sync_point and the list, exactly"""
    B, fp, typ, rng = _bare(n, 100 + n)
    try:
        seen_full = seen_partial = False
        for bins in BIN_SETS:
            tb = rng.choice(np.array(bins, np.int32), n).astype(np.int32)
            fp.set_field(B.F_TIMEBIN, tb)
            for ti in TI_CURRENT:
                want = SR.next_sync_point(ti, -1, tb, typ)
                got = fp.find_next_sync_point(ti)
                assert SR.same_sync_point(got, want) == [], (bins, ti)
                act = fp.get_active()
                assert act.dtype == np.int32 and np.array_equal(act, want["active"]), (bins, ti)
                assert np.array_equal(act, np.nonzero((want["TimeBinActive"] >> tb) & 1)[0])
                assert got.Flag_FullStep == int(len(act) == n)
                seen_full |= len(act) == n
                seen_partial |= len(act) < n
        assert seen_full and (seen_partial or n == 1)
        # only bin 0 populated: the next sync point is the current one, everybody is active
        fp.set_field(B.F_TIMEBIN, np.zeros(n, np.int32))
        got = fp.find_next_sync_point(40)
        assert got.Ti_next == 40 and got.Flag_FullStep == 1 and got.NumForceUpdate == n
        assert np.array_equal(fp.get_active(), np.arange(n))
    finally:
        fp.close()


def test_get_active_returns_what_set_active_gave():
    B, fp, typ, rng = _bare(777, 5)
    try:
        assert np.array_equal(fp.get_active(), np.arange(777))
        mine = np.array([700, 3, 64, 65], np.int32)            # (a caller's list keeps the caller's order)
        fp.set_active(mine)
        assert np.array_equal(fp.get_active(), mine)
        fp.set_active(np.zeros(0, np.int32))
        assert len(fp.get_active()) == 0
        fp.set_active(None)
        assert np.array_equal(fp.get_active(), np.arange(777))
    finally:
        fp.close()


def test_everybody_active_is_the_all_state_and_gravity_takes_all_targets():
    B = bindings()
    pr = Problem(ng=6, gas=True, periodic=0)
    n = pr.n
    fp = pr.device()
    try:
        pr.device_tree(fp)
        fp.set_field(B.F_OLDACC, np.zeros(n))
        tb = np.where(np.arange(n) % 2 == 0, 3, 5).astype(np.int32)
        fp.set_field(B.F_TIMEBIN, tb)
        sp = fp.find_next_sync_point(8)                         # -> 16: bin 3 only
        assert sp.Ti_next == 16 and sp.Flag_FullStep == 0 and sp.NumForceUpdate == (n + 1) // 2
        fp.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
        assert fp.stats()["grav_targets"] == (n + 1) // 2
        cost_half = fp.get_field(B.F_GRAVCOST)
        sp = fp.find_next_sync_point(24)                        # -> 32: both bins
        assert sp.Ti_next == 32 and sp.Flag_FullStep == 1 and sp.GlobNumForceUpdate == n
        assert np.array_equal(fp.get_active(), np.arange(n))
        fp.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
        assert fp.stats()["grav_targets"] == n
        # ... and they are the targets of ghip_set_active(NULL): the same walk, the same counts
        cost_sync = fp.get_field(B.F_GRAVCOST)
        acc_sync = fp.get_field(B.F_GRAVACCEL)
        fp.set_active(None)
        fp.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
        assert np.array_equal(fp.get_field(B.F_GRAVCOST), cost_sync)
        assert np.array_equal(fp.get_field(B.F_GRAVACCEL), acc_sync)
        assert np.array_equal(cost_half[::2], cost_sync[::2]) and np.all(cost_sync > 0)
    finally:
        fp.close()


def test_an_output_that_is_due_leaves_the_list_alone():
    B, fp, typ, rng = _bare(777, 7)
    try:
        tb = rng.choice(np.array([3, 5, 6], np.int32), 777).astype(np.int32)
        fp.set_field(B.F_TIMEBIN, tb)
        first = fp.find_next_sync_point(8)
        assert first.Ti_next == 16 and first.output_due == 0
        before = fp.get_active()
        assert 0 < len(before) < 777
        for ti_out in (20, 32):                                 # before the next kick of Ti = 24 (32), and on it
            want = SR.next_sync_point(24, ti_out, tb, typ)
            got = fp.find_next_sync_point(24, ti_out)
            assert SR.same_sync_point(got, want) == []
            assert got.output_due == 1 and got.Ti_next == ti_out
            assert np.array_equal(fp.get_active(), before)
        got = fp.find_next_sync_point(24, 33)                   # the output lies behind the kick: no longer due
        assert got.output_due == 0 and got.Ti_next == 32
        assert np.array_equal(fp.get_active(), np.nonzero(tb <= 5)[0])
    finally:
        fp.close()


def test_refusals_leave_the_list_alone():
    B, fp, typ, rng = _bare(66000, 9)
    try:
        tb = rng.choice(np.array([3, 5], np.int32), 66000).astype(np.int32)
        fp.set_field(B.F_TIMEBIN, tb)
        fp.find_next_sync_point(8)
        before = fp.get_active()
        assert np.array_equal(before, np.nonzero(tb == 3)[0])
        for bad, where in ((29, [5, 4000, 65999]), (-1, [1024]), (61, [0, 63])):   # (61 & 31 == 29, -1 & 31 == 31)
            t2 = tb.copy()
            t2[where] = bad
            fp.set_field(B.F_TIMEBIN, t2)
            with pytest.raises(B.GhipError) as e:
                fp.find_next_sync_point(24)
            assert B.GHIP_ERRORS[e.value.code] == "GHIP_EINVAL"
            assert "%d resident TIMEBIN" % len(where) in str(e.value)
            assert np.array_equal(fp.get_active(), before)
        fp.set_field(B.F_TIMEBIN, tb)
        for ti in (-1, (1 << 29) + 1):
            with pytest.raises(B.GhipError) as e:
                fp.find_next_sync_point(ti)
            assert B.GHIP_ERRORS[e.value.code] == "GHIP_EINVAL" and "Ti_Current" in str(e.value)
            assert np.array_equal(fp.get_active(), before)
        L, p, out, cnt = B.lib(), B.SyncParams(8, -1), B.SyncPoint(), C.c_int(0)
        einval = [k for k, v in B.GHIP_ERRORS.items() if v == "GHIP_EINVAL"][0]
        assert L.ghip_find_next_sync_point(fp.h, None, C.byref(out)) == einval
        assert L.ghip_find_next_sync_point(fp.h, C.byref(p), None) == einval
        assert L.ghip_find_next_sync_point(None, C.byref(p), C.byref(out)) == einval
        assert L.ghip_get_active(fp.h, None, None) == einval
        assert L.ghip_get_active(None, None, C.byref(cnt)) == einval
        assert np.array_equal(fp.get_active(), before)
        assert fp.find_next_sync_point(1 << 29).Ti_next == 1 << 29      # TIMEBASE itself is allowed
    finally:
        fp.close()


@pytest.mark.parametrize("n", [1, 2, 777])
def test_extent_is_the_oracles(n):
    B = bindings()
    rng = np.random.default_rng(40 + n)
    pos = rng.standard_normal((n, 3)) * np.array([3.0, 1.0, 0.1]) + np.array([0.5, -20.0, 1e3])
    fp = B.ForcePath(0)
    try:
        fp.set_counts(n, 0)
        fp.set_field(B.F_POS, pos)
        if n == 1:
            with pytest.raises(B.GhipError) as e:
                fp.find_extent()
            assert B.GHIP_ERRORS[e.value.code] == "GHIP_EINVAL" and "length 0" in str(e.value)
        else:
            corner, center, ln = fp.find_extent()
            want = O.domain_extent(pos)
            assert np.array_equal(corner, want[0]) and np.array_equal(center, want[1]) and ln == want[2]
            bad = pos.copy()
            bad[n // 2, 1] = np.nan
            fp.set_field(B.F_POS, bad)
            with pytest.raises(B.GhipError) as e:
                fp.find_extent()
            assert B.GHIP_ERRORS[e.value.code] == "GHIP_EINVAL" and "not finite" in str(e.value)
            fp.dd_init(0, 1)
            with pytest.raises(B.GhipError) as e:
                fp.find_extent()
            assert "GHIP_DD_DECOMPOSE" in str(e.value)
        fp.set_counts(0, 0)
    finally:
        fp.close()


def test_resident_run_with_individual_timesteps_finds_its_own_sync_points():
    """The loop of test_gpu_parity's "individual steps" flavour with the oracle in lockstep; on the device side
    the next sync point, the bins the kick may open and the active set come from find_next_sync_point alone:
    no set_active, and no TIMEBIN, TI_BEGSTEP or POS crosses the link between the steps.  The cube stays the
    oracle's, as there: device and oracle positions differ in the last bits and both sides need the same cube."""
    B = bindings()
    pr = Problem(ng=10, gas=True, periodic=1)
    n, ng, box = pr.n, pr.ngas, pr.box
    typ, mass = pr.ic["type"], pr.ic["mass"]
    tb = 1.0e-3 / (1 << 20)
    pr.timebase = tb
    soft = pr.force_soft / 2.8
    par = dict(Timebase_interval=tb, ComovingIntegrationOn=0, Time=1.0, hubble_a=1.0,
               ErrTolIntAccuracy=1.0e3, CourantFac=1.0e3, MaxSizeTimestep=1.0e-3,
               MinSizeTimestep=0.0, dt_displacement=1.0, MinEgySpec=0.0,
               TimeBinActive=0xffffffff, logTimeBegin=0.0, logTimeMax=0.0)
    tab = O.ewald_table(box)
    zero_i = np.zeros(n, np.int32)
    fp = pr.device()
    for fid in (B.F_TIMEBIN, B.F_TI_BEGSTEP, B.F_TI_CURRENT):
        fp.set_field(fid, zero_i)
    fp.set_field(B.F_OLDACC, np.zeros(n))
    in_loop = [False]
    plain_get = fp.get_field

    def guarded_get(field):
        assert not (in_loop[0] and field in (B.F_TIMEBIN, B.F_TI_BEGSTEP, B.F_POS)), "field %d was downloaded" % field
        return plain_get(field)
    fp.get_field = guarded_get
    o = dict(pos=pr.ic["pos"].copy(), vel=pr.ic["vel"].copy(), velpred=pr.velpred.copy(),
             entropy=pr.entropy.copy(), dtentropy=pr.dtentropy.copy(), hsml=pr.hsml0.copy(),
             timebin=zero_i.copy(), ti_begstep=zero_i.copy(), ti_current=zero_i.copy(),
             oldacc=np.zeros(n), grav=np.zeros((n, 3)), hyd=np.zeros((ng, 3)),
             density=np.ones(ng), divvel=np.zeros(ng), pressure=np.zeros(ng),
             dhsmlfac=np.ones(ng), curlvel=np.zeros(ng), vsig=np.zeros(ng))
    ti, ti_done, nact_seen = 0, 0, []
    in_loop[0] = True
    for step in range(6):
        # -- the oracle's sync point: the particles whose step ends at ti (run.c:300-320) --
        ends = o["ti_begstep"] + np.where(o["timebin"] > 0, 1 << o["timebin"], 0)
        act = np.where(ends == ti)[0].astype(np.int32)
        gas = act[act < ng]
        allact = len(act) == n
        nact_seen.append(len(act))
        # -- the device's: from the sync point just completed, on the resident bins --
        sp = fp.find_next_sync_point(ti_done)
        assert sp.output_due == 0 and sp.Ti_next == ti, (step, sp.Ti_next, ti)
        assert np.array_equal(fp.get_active(), act), step
        assert sp.Flag_FullStep == int(allact) and sp.NumForceUpdate == len(act)
        assert np.array_equal(np.array(sp.TimeBinCount[:]), np.bincount(o["timebin"], minlength=32))
        par["TimeBinActive"] = sum(1 << b for b in range(30) if ti % (1 << b) == 0)  # timestep.c:163
        pr.ti_current = ti
        theta = pr.theta if step == 0 else 0.0           # accel.c:61-68: first pass Barnes-Hut
        d = O.drift(ti, tb, o["pos"], o["vel"], typ, o["ti_current"], o["timebin"],
                    o["ti_begstep"], o["grav"], o["velpred"], o["hyd"], o["density"],
                    o["hsml"][:ng], o["divvel"], o["entropy"], o["dtentropy"], o["pressure"],
                    wrap=True, boxsize=box, gravpm=None)
        assert d["rc"] == 0
        o["pos"], o["ti_current"], o["velpred"] = d["pos"], d["ti_current"], d["velpred"]
        o["hsml"][:ng], o["density"], o["pressure"] = d["hsml"], d["density"], d["pressure"]
        extent = O.domain_extent(o["pos"])
        T = O.Tree(o["pos"], o["vel"], mass, typ, pr.force_soft, hsml=o["hsml"], extent=extent)
        acc, cost = T.gravity(pr.o_grav(theta), act, o["oldacc"])
        T.gravity_ewald_add(pr.o_grav(theta), tab, act, o["oldacc"], acc, cost)
        o["oldacc"][act], o["grav"][act] = O.gravity_finish(acc, pr.G, gravpm=None)
        if len(gas):
            od = T.density(pr.o_dens(), gas, o["velpred"], o["entropy"], o["dtentropy"],
                           o["timebin"], o["ti_begstep"], o["hsml"])
            for key in ("density", "divvel", "pressure", "dhsmlfac", "curlvel"):
                o[key][gas] = od[key][gas]
            o["hsml"][gas] = od["hsml"][gas]
            T.update_hmax(gas, o["hsml"], np.concatenate([o["divvel"], np.zeros(n - ng)]))
            full = lambda a: np.concatenate([a, np.zeros(n - ng)])      # noqa: E731
            oh = T.hydro(pr.o_hydro(), gas, o["velpred"], o["hsml"], full(o["density"]),
                         full(o["pressure"]), full(o["dhsmlfac"]), full(o["divvel"]),
                         full(o["curlvel"]), o["timebin"])
            o["hyd"][gas], o["dtentropy"][gas] = oh["hydroaccel"][gas], oh["dtentropy"][gas]
            o["vsig"][gas] = oh["maxsignalvel"][gas]
        if step == 0:
            # spread the particles over a few bins: median acceleration-criterion step = 0.7e-3
            amed = np.median(np.linalg.norm(o["grav"], axis=1))
            par["ErrTolIntAccuracy"] = (0.7e-3) ** 2 * amed / (2 * soft[1])
        par["Ti_Current"] = ti
        k = O.advance_timesteps(_fill(O.KickParams(), par, soft), typ, o["vel"], o["grav"],
                                o["hyd"], o["velpred"], o["entropy"], o["dtentropy"],
                                o["density"], o["pressure"], o["hsml"][:ng], o["vsig"],
                                o["timebin"], o["ti_begstep"], active=None if allact else act,
                                gravpm=None, tables=None)
        assert k["rc"] == 0
        for key in ("vel", "velpred", "entropy", "dtentropy", "timebin", "ti_begstep"):
            o[key] = k[key]
        # -- device: the same phases on the resident fields; the list is already in place --
        fp.drift(sp.Ti_next, tb, box_wrap=True, boxsize=box)
        fp.tree_build(extent[0], extent[1], extent[2], pr.force_soft)
        fp.gravity(pr.g_grav(theta), B.WALK_NEWTON_EWALD)
        fp.density(pr.g_dens())
        fp.update_hmax()
        fp.hydro(pr.g_hydro())
        fp.gravity_finish_ex(pr.G)
        dpar = dict(par, Ti_Current=sp.Ti_next, TimeBinActive=sp.TimeBinActive)
        fp.advance_timesteps(_fill(B.KickParams(), dpar, soft))
        assert np.array_equal(fp.get_field(B.F_GRAVCOST)[act], cost), (step, ti)
        ti_done = ti
        ti = int((o["ti_begstep"] + (1 << o["timebin"])).min())      # the oracle's next sync point
    in_loop[0] = False
    # what keeps the case honest
    assert len(np.unique(o["timebin"])) >= 3
    assert sum(1 for a in nact_seen if a < n // 2) >= 2
    # the end state, at the bounds of the existing flavour
    assert np.array_equal(fp.get_field(B.F_TIMEBIN), o["timebin"])
    assert np.abs(fp.get_field(B.F_POS) - o["pos"]).max() < 1e-13
    assert np.array_equal(fp.get_field(B.F_TI_BEGSTEP), o["ti_begstep"])
    assert np.array_equal(fp.get_field(B.F_TI_CURRENT), o["ti_current"])
    for fid, want in ((B.F_VEL, o["vel"]), (B.F_VELPRED, o["velpred"]), (B.F_GRAVACCEL, o["grav"]),
                      (B.F_HYDROACCEL, o["hyd"])):
        assert np.abs(fp.get_field(fid) - want).max() <= 1e-9 * np.abs(want).max(), fid
    assert relerr(fp.get_field(B.F_ENTROPY), o["entropy"]) < 1e-10
    assert relerr(fp.get_field(B.F_HSML)[:ng], o["hsml"][:ng]) < 1e-9
    assert relerr(fp.get_field(B.F_DENSITY), o["density"]) < 1e-9
    assert np.abs(o["pos"] - pr.ic["pos"]).max() > 1e-8       # the particles did move
    fp.close()


def _shard_bins(S, pr, k):
    """bins by global id from {5, 6, 9}; bin 3, the earliest, for every fourth particle of shard k alone"""
    tb = np.array([5, 6, 9], np.int32)[np.arange(pr.n) % 3]
    tb[S.gid[k][::4]] = 3
    return tb


@pytest.mark.parametrize("nshards", [3, 8])
def test_shards_agree_on_the_sync_point_and_select_their_own(nshards):
    B = bindings()
    pr = Problem(ng=12, gas=True, periodic=1)
    S = ShardSet(pr, nshards)
    try:
        k = nshards - 2
        tb = _shard_bins(S, pr, k)
        typ = pr.ic["type"]
        S.set_field(B.F_TIMEBIN, tb)
        for ti in (8, 24):      # -> 16: bin 3 only, which lives on shard k; -> 32: bins 3 and 5, on every shard
            single = SR.next_sync_point(ti, -1, tb, typ)
            sps = S.run.sync_point(ti)
            for r, (fp, sp) in enumerate(zip(S.fp, sps)):
                g = S.gid[r]
                want = SR.next_sync_point(ti, -1, tb[g], typ[g], others=[np.delete(tb, g)])
                assert SR.same_sync_point(sp, want) == [], (ti, r)
                for key in ("Ti_next", "TimeBinActive", "GlobNumForceUpdate", "Flag_FullStep"):
                    assert int(getattr(sp, key)) == int(single[key]), (ti, r, key)
                assert np.array_equal(fp.get_active(), np.nonzero((single["TimeBinActive"] >> tb[g]) & 1)[0])
                if ti == 8:
                    assert (sp.NumForceUpdate > 0) == (r == k)
            assert sum(int(sp.NumForceUpdate) for sp in sps) == single["NumForceUpdate"]
        # an output that is due: the same on every shard, the lists stay
        lists = S.each(lambda fp: fp.get_active())
        for sp in S.run.sync_point(24, 30):
            assert sp.output_due == 1 and sp.Ti_next == 30 and sp.TimeBinActive == 0
        assert all(np.array_equal(a, fp.get_active()) for a, fp in zip(lists, S.fp))
        # gravity on the lists the collective left, against the same lists given by the host
        S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
        acc, cost = S.get_field(B.F_GRAVACCEL), S.get_field(B.F_GRAVCOST)
        for fp, a in zip(S.fp, lists):
            fp.set_active(a)
        S.set_field(B.F_GRAVACCEL, np.zeros((pr.n, 3)))
        S.set_field(B.F_GRAVCOST, np.zeros(pr.n, np.int32))
        S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
        active = np.nonzero(tb <= 5)[0]
        assert len(active) > pr.n // 3
        assert np.array_equal(S.get_field(B.F_GRAVCOST)[active], cost[active]) and np.all(cost[active] > 0)
        assert relerr(S.get_field(B.F_GRAVACCEL)[active], acc[active]) < TOL
        # everybody in one bin: every shard goes to the "all" state
        S.set_field(B.F_TIMEBIN, np.full(pr.n, 5, np.int32))
        for fp, sp in zip(S.fp, S.run.sync_point(24)):
            assert sp.Flag_FullStep == 1 and sp.Ti_next == 32
            assert np.array_equal(fp.get_active(), np.arange(fp.n))
    finally:
        S.close()


@pytest.mark.parametrize("nshards", [3, 8])
def test_a_bad_bin_on_one_shard_stops_every_shard(nshards):
    B = bindings()
    pr = Problem(ng=12, gas=True, periodic=1)
    S = ShardSet(pr, nshards)
    try:
        k = 1
        tb = _shard_bins(S, pr, k)
        S.set_field(B.F_TIMEBIN, tb)
        S.run.sync_point(24)
        lists = S.each(lambda fp: fp.get_active())
        results = [fp.dd_get_sync_point().Ti_next for fp in S.fp]
        bad = tb.copy()
        bad[S.gid[nshards - 1][[0, 7]]] = 29
        S.set_field(B.F_TIMEBIN, bad)
        errs = failing_collective(S.fp, B.DD_DECOMPOSE, B.SyncParams(8, -1), B.SYNC_POINT_FORM)
        msgs = {str(e) for e in errs}
        assert len(msgs) == 1 and all(B.GHIP_ERRORS[e.code] == "GHIP_EINVAL" for e in errs)
        msg = msgs.pop()
        assert "2 resident TIMEBIN" in msg and "first on shard %d" % (nshards - 1) in msg
        assert all(np.array_equal(a, fp.get_active()) for a, fp in zip(lists, S.fp))
        assert [fp.dd_get_sync_point().Ti_next for fp in S.fp] == results
        # Ti_Current is refused by ghip_dd_begin, and the single-context call points to the collective
        with pytest.raises(B.GhipError) as e:
            S.fp[0].dd_begin(B.DD_DECOMPOSE, B.SyncParams(-3, -1), B.SYNC_POINT_FORM)
        assert "Ti_Current" in str(e.value)
        with pytest.raises(B.GhipError) as e:
            S.fp[0].find_next_sync_point(8)
        assert "GHIP_SYNC_POINT_FORM" in str(e.value)
        # with the bins mended the same contexts go on
        S.set_field(B.F_TIMEBIN, tb)
        assert {int(sp.Ti_next) for sp in S.run.sync_point(8)} == {16}
    finally:
        S.close()


def _run_ranks(transport):
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", SYNC_TRANSPORT=transport)
    if transport == "rccl":
        mock = os.path.join(root, "tests", "mock_rccl", "librccl_mock.so")
        assert os.path.exists(mock), "build tests/mock_rccl first (__graft_entry__.build())"
        env["GHIP_RCCL_LIB"] = mock
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "tests", "gpu_host_ranks_syncpoint.py")]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("transport", ["host", "rccl"])
def test_two_rank_processes_agree_on_the_sync_point(transport):
    """tests/gpu_host_ranks_syncpoint.py is the rank program: two processes, each with the particles it was dealt,
    the earliest bin on rank 1 alone.  "host": the exchanges go through the host's all-gather (gloo); "rccl":
    through the RCCL entry points, supplied by tests/mock_rccl (the real RCCL refuses two ranks on one device)."""
    out = _run_ranks(transport)
    assert out["ok"], out
    assert out["transport"] == transport
    if transport == "rccl":
        assert out["rccl_library"].endswith("librccl_mock.so")
    assert out["points_equal_restatement"] and out["lists_equal_restatement"]
    assert out["ti_next"] == [16, 32] and out["earliest_bin_on_last_rank_only"] == [0, 1]
    assert out["output_due"]
    assert len(out["refusals"]) == 1, out["refusals"]       # the same code and message on both ranks
    assert out["refusals"][0].startswith("GHIP_EINVAL|") and "3 resident TIMEBIN" in out["refusals"][0]
    assert "first on shard 0" in out["refusals"][0]
    assert out["lists_kept_after_refusal"]
    assert out["bytes_sync_point"] == 256 + 16              # the bin populations and the status record, to one peer
