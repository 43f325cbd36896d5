"""The resident wind particles on domain-decomposed shards: the wind table of a shard (ghip_dd_winds_set_table /
_get_table / _clear, local indices) and ghip_winds_feedback as a collective (GHIP_DD_WIND begun with walk =
GHIP_WINDS_RESIDENT_FORM), the rows through GHIP_DD_MIGRATE (re-keyed where the particle stays, sent where it leaves),
and two rank processes.  Logical shards in one process (ShardSet) on the small case of the wind tests (1 000 gas,
480 wind particles).  The resident form runs the kernels, the exchanges and the sums of GHIP_WIND_FORM and differs
only in where the list and the planes come from, so every comparison with GHIP_WIND_FORM -- given the list the
selection yields and the rows' state as host arrays -- is bit for bit."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from common import bindings, failing_collective
from test_gpu_wind_dd import CASES, DdWind
from test_gpu_wind_resident import _case, _rows, _same

pytestmark = pytest.mark.gpu
EINVAL = -90002
OUT_COLS = (("WK_OLD_MOMENTUM", "old_momentum"), ("WK_NEW_DENSITY", "new_density"), ("WK_DRMIN", "drmin"),
            ("WK_DT1", "dt1"), ("WK_DT2", "dt2"), ("WK_DT_JUMP", "dt_jump"), ("WK_DELTA_MOMENTUM", "delta_momentum"),
            ("WK_DELETED", "deleted"))


def _active(c, drop=0.15, seed=12):
    """the case's active list without some of the wind particles"""
    rng = np.random.default_rng(seed)
    return np.setdiff1d(c.active, c.wind[rng.random(len(c.wind)) < drop]).astype(np.int32)


class Shards(DdWind):
    """DdWind with an active list of the test's choosing and, per shard, the wind table of its part of the case"""

    def __init__(self, case, nshards, domains=1, active=None, trees=True, **ranks):
        super().__init__(case, nshards, domains, trees=trees, **ranks)
        if active is not None:
            self.active = [w[0] for w in self.S.locate(active)]
        self.rows = _rows(self.B, case)

    def set_tables(self, skip=()):
        for r in self.shards():
            if r not in skip:
                self.S.fp[r].dd_winds_set_table(self.local[r], self.rows[self.lists[r]])

    def listed(self, r):
        """positions in the case's list of the particles shard r's selection lists, in its active-list order"""
        c, B = self.case, self.B
        pos_of = {int(i): int(o) for i, o in zip(self.local[r], self.lists[r])}
        out = [pos_of[int(i)] for i in self.active[r] if int(i) in pos_of]
        return np.array([o for o in out if self.rows[o, B.WK_STELLAR_AGE] < c.par["Time"]], np.int64)

    def host_args(self, r, params):
        """GHIP_WIND_FORM for shard r on the list the selection yields, the state from the rows"""
        B, o = self.B, self.listed(r)
        loc = {int(p): int(i) for i, p in zip(self.local[r], self.lists[r])}
        st = dict(stellar_age=self.rows[o, B.WK_STELLAR_AGE], birth_energy=self.rows[o, B.WK_BIRTH_ENERGY],
                  old_momentum=self.rows[o, B.WK_OLD_MOMENTUM], new_density=self.rows[o, B.WK_NEW_DENSITY],
                  drmin=self.rows[o, B.WK_DRMIN])
        return B.dd_wind_args(params, np.array([loc[int(p)] for p in o], np.int32), state=st)

    def per_shard(self):
        B = self.B
        out = []
        for fp in self.S.fp:
            d = {f: fp.get_field(getattr(B, f)) for f in ("F_POS", "F_HSML", "F_MASS")}
            d.update(injected=fp.wind_injected(), rad_accel=fp.wind_rad_accel())
            out.append(d)
        return out


# ------------------------------------------------------------------------------------------------
# 1. the table of a shard
# ------------------------------------------------------------------------------------------------
def test_table_per_shard_and_its_refusals():
    c = _case(1)
    T = Shards(c, 2, trees=False)
    try:
        B = T.B
        assert all(len(x) > 100 for x in T.local)
        for r, fp in enumerate(T.S.fp):
            loc, rows = T.local[r], T.rows[T.lists[r]]
            perm = np.random.default_rng(3 + r).permutation(len(loc))
            fp.dd_winds_set_table(loc[perm], rows[perm])
            idx, got = fp.dd_winds_table()
            _same(idx, np.sort(loc), "local indices")
            _same(got, rows[np.argsort(loc, kind="stable")], "rows")
            typ = fp.get_field(B.F_TYPE)
            assert np.all(typ[idx] == 3)
            not3 = int(np.where(typ != 3)[0][-1])
            for bad, msg in ((np.r_[loc[:9], loc[3]], "index %d" % loc[3]), (np.r_[loc[:9], not3], "not Type 3"),
                             (np.r_[loc[:9], fp.n], "out of range"), (np.r_[loc[:9], -1], "out of range")):
                fp.dd_winds_set_table(loc, rows)
                with pytest.raises(B.GhipError, match=msg) as e:
                    fp.dd_winds_set_table(bad, rows[:10])
                assert e.value.code == EINVAL
                with pytest.raises(B.GhipError, match="no wind table") as e:
                    fp.dd_winds_table()
                assert e.value.code == EINVAL
            fp.dd_winds_set_table([], np.zeros((0, B.WK_COUNT)))
            assert len(fp.dd_winds_table()[0]) == 0
            # other counts: refused until given again
            fp.dd_winds_set_table(loc, rows)
            n, ng = fp.counts()
            fp.set_counts(n, ng - 1)
            with pytest.raises(B.GhipError, match="given for other counts") as e:
                fp.dd_winds_table()
            assert e.value.code == EINVAL
            fp.set_counts(n, ng)
            fp.dd_winds_clear()
            with pytest.raises(B.GhipError, match="no wind table"):
                fp.dd_winds_table()
            # the single-rank names keep refusing this context, and say where to go
            with pytest.raises(B.GhipError, match="the shard form is not built.*ghip_dd_winds_set_table") as e:
                fp.winds_set_table(loc, rows)
            assert e.value.code == EINVAL
    finally:
        T.close()
    # a plain context and a ghip_set_shard context refuse the new names
    B, fp = c.device(tree=False)
    rows = _rows(B, c)
    for call in (lambda: fp.dd_winds_set_table(c.wind, rows), fp.dd_winds_table, fp.dd_winds_clear):
        with pytest.raises(B.GhipError, match="ghip_winds_set_table") as e:
            call()
        assert e.value.code == EINVAL
    fp.winds_set_table(c.wind, rows)                         # (and the single-rank name serves it)
    fp.close()
    B, fp = c.device(tree=False)
    fp.set_shard(0, 2)
    for call in (lambda: fp.dd_winds_set_table(c.wind, rows), fp.dd_winds_table, fp.dd_winds_clear):
        with pytest.raises(B.GhipError, match="ghip_set_shard") as e:
            call()
        assert e.value.code == EINVAL
    fp.close()


def test_table_follows_rearrange_and_peano_order_on_a_shard():
    """ghip_rearrange and ghip_peano_order are local on a ghip_dd_init context and carry the shard's table"""
    c = _case(0)
    T = Shards(c, 3, trees=False)
    try:
        B = T.B
        T.set_tables()
        for r, fp in enumerate(T.S.fp):
            loc = T.local[r]
            mass = fp.get_field(B.F_MASS)
            gone = loc[::5]
            mass[gone] = 0.0                                  # what the elimination of the loop leaves
            fp.set_field(B.F_MASS, mass)
            idx, want = fp.dd_winds_table()
            for step in ("rearrange", "peano"):
                if step == "rearrange":
                    assert fp.rearrange().count_elim >= len(gone)
                else:
                    fp.peano_order()                     # (the domain in force)
                new_of_old, _ = fp.sequence_map()
                j = new_of_old[idx]
                want, j = want[j >= 0], j[j >= 0]
                order = np.argsort(j, kind="stable")
                want, idx = want[order], j[order].astype(np.int32)
                gi, got = fp.dd_winds_table()
                _same(gi, idx, "indices after %s" % step)
                _same(got, want, "rows after %s" % step)
                assert np.all(fp.get_field(B.F_TYPE)[gi] == 3)
            assert len(idx) == len(loc) - len(gone)
    finally:
        T.close()


# ------------------------------------------------------------------------------------------------
# 2. the loop from the rows = the loop with host arrays, bit for bit
# ------------------------------------------------------------------------------------------------
def _both_loops(nshards, periodic, domains, **over):
    c = _case(periodic)
    active = _active(c)
    ra0 = np.random.default_rng(6).standard_normal((c.pr.ngas, 3))
    TA, TB = Shards(c, nshards, domains, active), Shards(c, nshards, domains, active)
    try:
        B = TA.B
        for T in (TA, TB):
            T.set_active()
            T.set_gas("set_wind_rad_accel", ra0)
        TA.set_tables()
        params = c.gparams(**over)
        res = TA.S.run.winds_feedback(params)
        built = [TB.host_args(r, params) for r in range(nshards)]
        TB.run(B.WIND_OP, [b[0] for b in built], B.WIND_FORM)
        host = [B.dd_wind_result(b[1]) for b in built]
        tables = [fp.dd_winds_table() for fp in TA.S.fp]
        return c, TA.listed, [TA.listed(r) for r in range(nshards)], TA.rows, TA.local, TA.lists, res, host, tables, \
            TA.per_shard(), TB.per_shard(), TA.resident(), TB.resident()
    finally:
        TA.close()
        TB.close()


def _check_against_host(B, run, floor=False):
    c, _, listed, rows, local, lists, res, host, tables, sa, sb, ga, gb = run
    for r in range(len(res)):
        for k in ("iterations", "bits", "ndeleted", "deleted_momentum"):
            assert res[r][k] == host[r][k], (r, k, res[r][k], host[r][k])
        _same(res[r]["counts"], host[r]["counts"], "counts of shard %d" % r)
        # every column of every row: the listed ones against the host form's out arrays, the others untouched
        want = rows.copy()
        o = listed[r]
        for col, k in OUT_COLS:
            if not floor or k in ("dt1", "dt2", "dt_jump", "delta_momentum", "deleted"):
                want[o, getattr(B, col)] = host[r][k]
        order = np.argsort(local[r], kind="stable")
        idx, got = tables[r]
        _same(idx, local[r][order], "indices of shard %d" % r)
        for col in range(B.WK_COUNT):
            _same(got[:, col], want[lists[r][order], col], "column %d of shard %d" % (col, r))
        unlisted = np.setdiff1d(lists[r], o)
        assert len(unlisted) > 0
        for k in sa[r]:
            _same(sa[r][k], sb[r][k], "%s of shard %d" % (k, r))
    for f in ga:
        _same(ga[f], gb[f], "global field %d" % f)
    return sum(len(o) for o in listed)


@pytest.mark.parametrize("nshards,periodic,domains", [(2, 0, 1), (3, 1, 1), (8, 0, 1), (8, 1, 1), (3, 1, 4)])
def test_loop_from_the_rows_equals_the_host_array_form(nshards, periodic, domains):
    assert (nshards, periodic, domains) in CASES
    B = bindings()
    run = _both_loops(nshards, periodic, domains)
    c, rows, res = run[0], run[3], run[6]
    nlisted = _check_against_host(B, run)
    assert 300 < nlisted < len(c.wind) - 40
    inactive = ~np.isin(c.wind, _active(c))
    born_now = np.isin(c.wind, _active(c)) & (c.age == c.par["Time"])
    assert inactive.sum() > 30 and born_now.sum() > 5       # both kinds of unlisted rows were there
    assert res[0]["iterations"] > 8 and sum(r["ndeleted"] for r in res) > 50
    assert sum(int(r["counts"][0]) for r in res) > 0          # particles went to other shards
    assert all(int(r["counts"][3]) == 3 + 4 * res[0]["iterations"] for r in res)


def test_loop_under_the_floor_writes_the_out_columns_only():
    B = bindings()
    run = _both_loops(3, 1, 1, dt_total_floor=1e30)
    _check_against_host(B, run, floor=True)
    assert all(r["iterations"] == 0 for r in run[6])


def test_two_runs_of_the_resident_loop_are_bit_identical():
    a, b = _both_loops(3, 0, 1), _both_loops(3, 0, 1)
    for r in range(3):
        _same(a[8][r][1], b[8][r][1], "rows of shard %d" % r)
        for k in a[9][r]:
            _same(a[9][r][k], b[9][r][k], k)
        assert a[6][r]["bits"] == b[6][r]["bits"] and a[6][r]["deleted_momentum"] == b[6][r]["deleted_momentum"]


# ------------------------------------------------------------------------------------------------
# 6. what one shard cannot do ends the operation on all, in the same step
# ------------------------------------------------------------------------------------------------
def _everything(T):
    B = T.B
    out = T.resident()
    out["injected"], out["rad_accel"] = T.injected(), T.rad_accel()
    return out


def test_an_active_wind_particle_without_a_row_fails_on_all_shards():
    c = _case(0)
    T = Shards(c, 3, active=c.active)
    try:
        B = T.B
        T.set_active()
        T.set_tables(skip=(1,))
        missing = int(T.local[1][len(T.local[1]) // 2])
        assert T.rows[T.lists[1][len(T.local[1]) // 2], B.WK_STELLAR_AGE] < c.par["Time"]
        keep = T.local[1] != missing
        T.S.fp[1].dd_winds_set_table(T.local[1][keep], T.rows[T.lists[1]][keep])
        tables = [fp.dd_winds_table() for fp in T.S.fp]
        start = _everything(T)
        built = [B.dd_winds_args(c.gparams()) for _ in range(3)]
        errs = failing_collective(T.S.fp, B.WIND_OP, [b[0] for b in built], B.WINDS_RESIDENT_FORM)
        assert "Type-3 particle %d of rank 1 has no row" % missing in str(errs[1]) and errs[1].code == EINVAL
        assert all("shard 1" in str(errs[r]) and errs[r].code == EINVAL for r in (0, 2))
        now = _everything(T)
        for f in start:
            _same(now[f], start[f], "field %s" % f)
        for fp, (idx, rows) in zip(T.S.fp, tables):
            gi, got = fp.dd_winds_table()
            _same(gi, idx, "indices")
            _same(got, rows, "rows")
        # a shard without a table beside shards with one
        T.S.fp[2].dd_winds_clear()
        T.S.fp[1].dd_winds_set_table(T.local[1], T.rows[T.lists[1]])
        errs = failing_collective(T.S.fp, B.WIND_OP, [b[0] for b in built], B.WINDS_RESIDENT_FORM)
        assert "no wind table" in str(errs[2]) and "rank 2" in str(errs[2]) and errs[2].code == EINVAL
        assert all("shard 2" in str(errs[r]) and errs[r].code == EINVAL for r in (0, 1))
        now = _everything(T)
        for f in start:
            _same(now[f], start[f], "field %s" % f)
        # with all tables in place the same contexts run the loop
        T.S.fp[2].dd_winds_set_table(T.local[2], T.rows[T.lists[2]])
        res = T.S.run.winds_feedback(c.gparams())
        assert res[0]["iterations"] > 8
    finally:
        T.close()


# ------------------------------------------------------------------------------------------------
# 3. GHIP_DD_MIGRATE carries the rows and re-keys them
# ------------------------------------------------------------------------------------------------
def _tagged(B, r, idx):
    """rows for the local indices idx of shard r: every double names (origin shard, origin index, column)"""
    idx = np.asarray(idx, np.int64)
    return (r * 1e7 + idx[:, None] * 16.0 + np.arange(B.WK_COUNT)[None, :]).astype(np.float64)


def _give_tagged(T, holders):
    """holders[r]: the local indices that get a row on shard r (None: no table) -> {particle ID: its row}"""
    B, want = T.B, {}
    for r, fp in enumerate(T.S.fp):
        if holders[r] is None:
            fp.dd_winds_clear()
            continue
        idx = np.asarray(holders[r], np.int32)
        rows = _tagged(B, r, idx)
        fp.dd_winds_set_table(idx, rows)
        ids = fp.get_field(B.F_ID)
        for i, row in zip(idx, rows):
            assert int(ids[i]) not in want               # (the IDs of a ShardSet are the global indices)
            want[int(ids[i])] = row
    return want


def _check_tagged(T, want):
    """every shard's keys are ascending local indices of Type-3 particles, every row is the one its particle (by
    ID, which migrates) had, and no row was lost or made"""
    B, seen = T.B, 0
    for r, fp in enumerate(T.S.fp):
        idx, rows = fp.dd_winds_table()
        assert np.all(np.diff(idx) > 0), "keys of shard %d" % r
        if len(idx) == 0:
            continue
        assert idx[0] >= fp.ngas and idx[-1] < fp.n
        assert np.all(fp.get_field(B.F_TYPE)[idx] == 3)
        ids = fp.get_field(B.F_ID)[idx]
        for k, i in enumerate(ids):
            assert int(i) in want, "shard %d: a row for particle %d, which had none" % (r, i)
            _same(rows[k], want[int(i)], "row of particle %d on shard %d" % (i, r))
        seen += len(idx)
    assert seen == len(want), (seen, len(want))
    return [len(fp.dd_winds_table()[0]) for fp in T.S.fp]


def _refresh(S):
    """who holds what after a migration, from the ID field (as ShardSet.migrate)"""
    for r, fp in enumerate(S.fp):
        n, ngl = fp.counts()
        S.gid[r] = fp.get_field(S.B.F_ID).astype(np.int64) if n else np.zeros(0, np.int64)
        S.ngas[r] = ngl
        S.owner[S.gid[r]] = r


def _migrate_counting(S):
    """GHIP_DD_MIGRATE on all shards -> the exchanges it took"""
    B, nx = S.B, 0
    for fp in S.fp:
        fp.dd_begin(B.DD_MIGRATE, None, 0)
    while True:
        rcs = [fp.dd_step() for fp in S.fp]
        assert len(set(rcs)) == 1, rcs
        if rcs[0] == 0:
            break
        B.dd_exchange_local(S.fp)
        nx += 1
    _refresh(S)
    return nx


def _send(S, pos, who, to, rng):
    """the particles `who` (global indices) to places next to gas particles of shard `to`"""
    gas = S.gid[to][:S.ngas[to]]
    pos[who] = S.pr.ic["pos"][rng.choice(gas, len(who))] + 1e-4


def _local_of(S, r, glob):
    loc = {int(g): k for k, g in enumerate(S.gid[r])}
    return np.array([loc[int(g)] for g in glob], np.int32)


def test_migration_of_constructed_moves():
    """Three shards, no decomposition in between (the key ranges stand, the test moves particles across them).
    First migration: ALL rows of shard 0 leave; shard 1 ONLY receives; shard 2 holds a table of 0 rows and sends
    Type-3 particles that have no row; every fourth wind particle of shard 1 has no row either; gas and other
    particles move too, so every block of the new layout is renumbered.  Second migration: 257 rows in one run
    (shard 1 to shard 2), across the 256-thread boundary of the pack, unpack and re-key kernels."""
    c = _case(1)
    T = Shards(c, 3, trees=False)
    try:
        B, S, pr = T.B, T.S, c.pr
        rng = np.random.default_rng(5)
        wind_of = [c.wind[S.owner[c.wind] == r] for r in range(3)]
        assert all(len(w) > 60 for w in wind_of)
        with_row1 = np.delete(wind_of[1], np.s_[::4])
        want = _give_tagged(T, [_local_of(S, 0, wind_of[0]), _local_of(S, 1, with_row1), np.zeros(0, np.int32)])
        pos = pr.ic["pos"].copy()
        _send(S, pos, wind_of[0], 1, rng)
        _send(S, pos, wind_of[2][::2], 1, rng)               # Type 3 without rows
        others = np.setdiff1d(np.arange(pr.ngas, pr.n), c.wind)
        _send(S, pos, rng.choice(S.gid[1][:S.ngas[1]], 50, replace=False), 0, rng)         # gas 1 -> 0
        _send(S, pos, rng.choice(S.gid[0][:S.ngas[0]], 40, replace=False), 1, rng)         # gas 0 -> 1
        _send(S, pos, rng.choice(others[S.owner[others] == 0], 30, replace=False), 1, rng)
        _send(S, pos, rng.choice(others[S.owner[others] == 1], 30, replace=False), 2, rng)
        S.set_field(B.F_POS, pos)
        assert _migrate_counting(S) == 2                    # the particles, the wind rows
        held = _check_tagged(T, want)
        assert held == [0, len(wind_of[0]) + len(with_row1), 0]
        assert np.all(S.owner[wind_of[0]] == 1) and np.all(S.owner[wind_of[2][::2]] == 1)
        holds = lambda: [int((S.owner[np.array(sorted(want))] == r).sum()) for r in range(3)]
        assert held == holds()
        # the second migration: 257 rows in one run, some more the other way
        rows1 = np.concatenate([wind_of[0], with_row1])
        assert len(rows1) > 280
        go2, go0 = rows1[:264], rows1[264:280]               # (a place next to a range's edge may lie beyond it)
        _send(S, pos, go2, 2, rng)
        _send(S, pos, go0, 0, rng)
        S.set_field(B.F_POS, pos)
        assert _migrate_counting(S) == 2
        held = _check_tagged(T, want)
        assert held == holds() and held[2] >= 257 and held[0] > 0 and held[1] > 0
        assert (S.owner[go2] == 2).sum() >= 257
        # nobody moves: the exchanges are taken, every table stands
        before = [fp.dd_winds_table() for fp in S.fp]
        assert _migrate_counting(S) == 2
        for fp, (idx, rows) in zip(S.fp, before):
            _same(fp.dd_winds_table()[0], idx, "keys")
            _same(fp.dd_winds_table()[1], rows, "rows")
        # one shard without a wind table: every shard refuses, nothing moved
        _send(S, pos, go2[:40], 1, rng)
        S.set_field(B.F_POS, pos)
        S.fp[1].dd_winds_clear()
        fields = [{f: fp.get_field(getattr(B, f)) for f in ("F_POS", "F_ID", "F_TYPE", "F_MASS")} for fp in S.fp]
        errs = failing_collective(S.fp, B.DD_MIGRATE, None)
        assert all(e.code == EINVAL and "wind table" in str(e) and "nothing was moved" in str(e) for e in errs)
        assert "1 of the 2 other shards hold a wind table and this one holds one" in str(errs[0])
        assert "2 of the 2 other shards hold a wind table and this one holds none" in str(errs[1])
        for fp, old in zip(S.fp, fields):
            for f, v in old.items():
                _same(fp.get_field(getattr(B, f)), v, f)
        for r in (0, 2):
            _same(S.fp[r].dd_winds_table()[1], before[r][1], "rows of shard %d" % r)
        # no shard holds one: the migration of before this table existed, one exchange
        for r in (0, 2):
            S.fp[r].dd_winds_clear()
        assert _migrate_counting(S) == 1
        assert (S.owner[go2[:40]] == 1).sum() > 30
    finally:
        T.close()


def test_migration_with_sink_tables_and_wind_tables_together_and_each_alone():
    c = _case(0)
    T = Shards(c, 3, trees=False)
    try:
        B, S, pr = T.B, T.S, c.pr
        rng = np.random.default_rng(11)
        others = np.setdiff1d(np.arange(pr.ngas, pr.n), c.wind)
        sinks = rng.choice(others, 24, replace=False)
        typ = pr.ic["type"].copy()
        typ[sinks] = 5
        S.set_field(B.F_TYPE, typ)
        sink_rows = {int(g): rng.random(B.SK_COUNT) for g in sinks}

        def give_sinks():
            for r, fp in enumerate(S.fp):
                mine = sinks[S.owner[sinks] == r]
                fp.sinks_set_table(mine.astype(np.uint32), np.array([sink_rows[int(g)] for g in mine]).reshape(len(mine), B.SK_COUNT))

        def check_sinks():
            for r, fp in enumerate(S.fp):
                ids, rows = fp.sinks_table()
                _same(np.sort(ids.astype(np.int64)), np.sort(sinks[S.owner[sinks] == r]), "sink IDs of shard %d" % r)
                for i, row in zip(ids, rows):
                    _same(row, sink_rows[int(i)], "sink row %d" % i)

        pos = pr.ic["pos"].copy()
        for both, sinks_on, winds_on, exchanges in ((1, 1, 1, 4), (0, 1, 0, 3), (0, 0, 1, 2)):
            for fp in S.fp:
                fp.sinks_clear()
            if sinks_on:
                give_sinks()
            wind_of = [c.wind[S.owner[c.wind] == r] for r in range(3)]
            want = _give_tagged(T, [_local_of(S, r, wind_of[r]) if winds_on else None for r in range(3)])
            for r in range(3):
                _send(S, pos, wind_of[r][::3], (r + 1) % 3, rng)
                mine = sinks[S.owner[sinks] == r]
                _send(S, pos, mine[::2], (r + 2) % 3, rng)
            S.set_field(B.F_POS, pos)
            assert _migrate_counting(S) == exchanges, (sinks_on, winds_on)
            if winds_on:
                assert sum(_check_tagged(T, want)) == len(c.wind)
            if sinks_on:
                check_sinks()
    finally:
        T.close()


@pytest.mark.parametrize("nshards,eliminate", [(3, False), (8, False), (3, True), (8, True)])
def test_rows_follow_the_particles_the_loop_has_flown_out(nshards, eliminate):
    """The loop, then redistribute(): decompose in a fresh cube and migrate; with `eliminate` every shard first runs
    ghip_rearrange (the rows of the eliminated wind particles go) and ends with ghip_peano_order."""
    c = _case(1)
    T = Shards(c, nshards, active=c.active)
    try:
        B, S = T.B, T.S
        T.set_active()
        T.set_tables()
        res = S.run.winds_feedback(c.gparams())
        assert sum(r["ndeleted"] for r in res) > 50
        holders = [fp.dd_winds_table()[0] for fp in S.fp]
        want = _give_tagged(T, holders)
        if eliminate:
            for fp in S.fp:
                ids, mass = fp.get_field(B.F_ID), fp.get_field(B.F_MASS)
                for i in fp.dd_winds_table()[0]:
                    if mass[i] == 0:
                        del want[int(ids[i])]
            assert len(want) == len(c.wind) - sum(r["ndeleted"] for r in res)
        owner0 = S.owner.copy()
        out = S.run.redistribute(B.DecompParams(0, 0, 1, 0), rearrange=True if eliminate else None,
                                 peano_order=eliminate)
        if eliminate:
            assert out["tot_elim"] >= sum(r["ndeleted"] for r in res)
        for r, fp in enumerate(S.fp):
            fp.counts()
        alive = np.concatenate([fp.get_field(B.F_ID) for fp in S.fp]).astype(np.int64)
        now = np.full(c.pr.n, -1)
        for r, fp in enumerate(S.fp):
            now[fp.get_field(B.F_ID)] = r
        moved = np.array([g for g in want if now[g] != owner0[g]])
        assert len(moved) > 10, "too few wind particles changed shards: %d" % len(moved)
        assert len(alive) == len(set(alive.tolist()))
        _check_tagged(T, want)
    finally:
        T.close()


# ------------------------------------------------------------------------------------------------
# 7. two rank processes
# ------------------------------------------------------------------------------------------------
def _run_ranks(transport):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", WINDS_TRANSPORT=transport)
    if transport == "rccl":
        mock = os.path.join(root, "tests", "mock_rccl", "librccl_mock.so")
        assert os.path.exists(mock), "build tests/mock_rccl first (__graft_entry__.build())"
        env["GHIP_RCCL_LIB"] = mock
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "tests", "gpu_host_ranks_winds.py")]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_two_rank_processes_equal_the_in_process_run():
    """tests/gpu_host_ranks_winds.py is the rank program: form 33, the resident loop and a migration that carries the
    rows on two rank processes, through the host's all-gather (gloo) and through the RCCL entry points (tests/mock_rccl);
    rank 0 compares with the run of both shards in its own process.  The second transport starts only after the
    first has ended well."""
    bytes_sent = {}
    for transport in ("host", "rccl"):
        out = _run_ranks(transport)
        assert out["ok"], out
        assert out["transport"] == transport
        if transport == "rccl":
            assert out["rccl_library"].endswith("librccl_mock.so")
        assert out["iterations"] > 8
        assert out["spawn_equal"] and sum(out["spawned"]) > 300 and out["tot_spawned"] == [sum(out["spawned"])] * 2, out
        assert out["outputs_equal"] and out["tables_equal"] and out["resident_equal"], out
        assert sum(out["rows"]) == 480 and all(m[0] > 0 or m[1] > 0 for m in out["migrated"]), out
        assert all(b > 0 for b in out["bytes_wind"])
        bytes_sent[transport] = out["bytes_wind"]
    assert bytes_sent["host"] == bytes_sent["rccl"]


# ------------------------------------------------------------------------------------------------
# 4. ghip_wind_spawn as a collective
# ------------------------------------------------------------------------------------------------
def _spawn_shards(nshards, ranks=None, **over):
    """SpawnCase(1) of tests/test_gpu_wind_resident.py on shards.  The shard that holds the sink emitting 300 is
    `emit`; on three shards the next one keeps its sinks but none of them is active (its sinks emit nothing) and
    the third has its sinks turned into ordinary particles (a shard without sinks, with an empty sink table).
    -> (sc, T, per shard the positions in sc.sinks of its listed sinks in active-list order, emit)"""
    from test_gpu_wind_resident import SINK_TARGETS, SpawnCase
    sc = SpawnCase(1, **over)
    T = Shards(sc.c, nshards, trees=False, **(ranks or {}))
    B, S = T.B, T.S
    names = [nm for nm, _ in SINK_TARGETS]
    owner = S.owner[sc.sinks]
    emit = int(owner[names.index("threehundred")])
    typ, active = sc.type.copy(), sc.active
    sinks_on = np.ones(len(sc.sinks), bool)
    if nshards == 3:
        quiet, none = (emit + 1) % 3, (emit + 2) % 3
        active = np.setdiff1d(active, sc.sinks[owner == quiet]).astype(np.int32)
        typ[sc.sinks[owner == none]] = 1
        sinks_on = owner != none
    for f, v in ((B.F_TYPE, typ), (B.F_MASS, sc.mass), (B.F_HSML, sc.hsml), (B.F_TIMEBIN, sc.timebin),
                 (B.F_ID, sc.ids.view(np.int32)), (B.F_TI_BEGSTEP, (np.arange(sc.c.pr.n) % 5).astype(np.int32))):
        S.set_field(f, v)
    rows = sc.sink_rows(B)
    listed = []
    for r, fp in enumerate(S.fp):
        mine = np.where((owner == r) & sinks_on)[0]
        fp.sinks_set_table(sc.ids[sc.sinks[mine]], rows[mine].reshape(len(mine), B.SK_COUNT))
        loc_act = S.locate(active)[r][0]
        fp.set_active(loc_act)
        glob_act = S.gid[r][loc_act]
        listed.append(np.array([a for g in glob_act for a in np.where((sc.sinks == g) & sinks_on)[0]], np.int64))
    T.set_tables()
    return sc, T, listed, emit


SPAWN_FIELDS = ("F_POS", "F_VEL", "F_MASS", "F_TYPE", "F_HSML", "F_TIMEBIN", "F_TI_BEGSTEP", "F_ID")


def _shard_bytes(B, fp):
    out = {f: fp.get_field(getattr(B, f)) for f in SPAWN_FIELDS}
    out["wind"] = np.c_[fp.dd_winds_table()]
    out["sink"] = np.c_[fp.sinks_table()]
    out["active"] = fp.get_active()
    return out


@pytest.mark.parametrize("nshards", [2, 3])
def test_spawn_on_shards_equals_the_restatement_on_each_shards_own_state(nshards):
    import wind_spawn_ref as SR
    sc, T, listed, emit = _spawn_shards(nshards)
    try:
        B, S = T.B, T.S
        EPS = np.finfo(float).eps
        before = [_shard_bytes(B, fp) for fp in S.fp]
        refs = []
        for r in range(nshards):
            g = S.gid[r]
            loc = {int(x): k for k, x in enumerate(g)}
            a = listed[r]
            local_sinks = np.array([loc[int(sc.sinks[k])] for k in a], np.int64)
            refs.append(SR.spawn(sc.par, len(g), local_sinks, before[r]["F_MASS"], before[r]["F_TIMEBIN"],
                                 before[r]["F_HSML"], before[r]["F_ID"].view(np.uint32), sc.bh_mass[a], sc.mdot[a],
                                 sc.bh_density[a], sc.rnd))
        spawned = [ref["report"]["spawned"] for ref in refs]
        assert spawned[emit] >= 300 and (nshards == 2 or sorted(spawned)[:2] == [0, 0]), spawned
        reps = S.run.wind_spawn(sc.gparams(B), sc.rnd)
        speed = SR.C_LIGHT / sc.par["UnitVelocity_in_cm_per_s"] / sc.par["FeedBackVelocity"]
        for r, fp in enumerate(S.fp):
            ref, rep, n, t = refs[r], reps[r], len(S.gid[r]), spawned[r]
            for k in ("spawned", "nsinks_emitting", "first_index", "new_wind_exact_sum", "gsl_draws"):
                assert rep[k] == ref["report"][k], (r, k, rep[k], ref["report"][k])
            assert rep["tot_spawned"] == sum(spawned)            # the sum, on every shard
            assert (fp.n, fp.ngas) == (n + t, S.ngas[r])
            now = _shard_bytes(B, fp)
            if t == 0:                                           # nothing spawned: nothing changed
                for k in now:
                    _same(now[k], before[r][k], "%s of shard %d" % (k, r))
                continue
            for f in SPAWN_FIELDS:
                if B._FIELD_INFO[getattr(B, f)][0]:
                    continue
                first = before[r][f].copy()
                if f == "F_MASS":
                    for i, m in ref["sink_mass"].items():
                        first[i] = m
                _same(now[f][:n], first, "%s of the first n of shard %d" % (f, r))
                if f in ("F_POS", "F_TIMEBIN", "F_TI_BEGSTEP"):
                    _same(now[f][n:], first[ref["parent"]], f + " copied")
            assert np.all(now["F_TYPE"][n:] == 3)
            _same(now["F_HSML"][n:], ref["hsml"], "Hsml")
            _same(now["F_ID"][n:].view(np.uint32), ref["id"], "ID (the sink's + the LOCAL index)")
            _same(now["F_MASS"][n:], ref["mass"], "Mass")
            bound = 16 * EPS * (1 + np.abs(ref["phi"]))          # (the bound of test_gpu_wind_resident.py)
            ratio = (np.abs(now["F_VEL"][n:] / speed - ref["dir"]) / bound[:, None]).max()
            print("shard %d: %d new particles, direction / bound = %.3g" % (r, t, ratio))
            assert ratio <= 1.0
            gi, got = fp.dd_winds_table()
            nold = len(before[r]["wind"])
            _same(gi, np.r_[before[r]["wind"][:, 0], np.arange(n, n + t)].astype(np.int32), "indices")
            _same(got[:nold], before[r]["wind"][:, 1:], "old rows")
            _same(got[nold:], ref["rows"], "new rows")
            _same(now["active"], np.r_[before[r]["active"], np.arange(n, n + t)].astype(np.int32), "active list")
            _same(now["sink"], before[r]["sink"], "sink table")
    finally:
        T.close()


def test_spawn_overflow_on_one_shard_changes_nothing_anywhere():
    sc, T, listed, emit = _spawn_shards(3)
    try:
        B, S = T.B, T.S
        before = [_shard_bytes(B, fp) for fp in S.fp]
        # MaxPart per shard: room for everything but on `emit`, which lacks one
        built = [B.dd_winds_args(spawn=sc.gparams(B, MaxPart=len(S.gid[r]) + (299 if r == emit else 1000)),
                                 rnd_table=sc.rnd) for r in range(3)]
        errs = failing_collective(S.fp, B.WIND_OP, [b[0] for b in built], B.WINDS_SPAWN_FORM)
        assert all(e.code == EINVAL for e in errs)
        assert "do not fit MaxPart" in str(errs[emit]) and "rank %d" % emit in str(errs[emit])
        assert all("shard %d" % emit in str(errs[r]) for r in range(3) if r != emit)
        for r, fp in enumerate(S.fp):
            fp.counts()
            now = _shard_bytes(B, fp)
            for k in now:
                _same(now[k], before[r][k], "%s of shard %d" % (k, r))
        # a shard without a wind table, and no RndTable in the params
        S.fp[(emit + 1) % 3].dd_winds_clear()
        built = [B.dd_winds_args(spawn=sc.gparams(B), rnd_table=sc.rnd) for _ in range(3)]
        errs = failing_collective(S.fp, B.WIND_OP, [b[0] for b in built], B.WINDS_SPAWN_FORM)
        assert all(e.code == EINVAL for e in errs) and "no wind table" in str(errs[(emit + 1) % 3])
        T.set_tables()
        built = [B.dd_winds_args(spawn=sc.gparams(B), rnd_table=None) for _ in range(3)]
        errs = failing_collective(S.fp, B.WIND_OP, [b[0] for b in built], B.WINDS_SPAWN_FORM)
        assert all(e.code == EINVAL and "RndTable" in str(e) for e in errs)
        assert all(fp.counts()[0] == len(S.gid[r]) for r, fp in enumerate(S.fp))
    finally:
        T.close()


# ------------------------------------------------------------------------------------------------
# 5. three steps of the cycle on 3 shards against a host-driven ShardSet
# ------------------------------------------------------------------------------------------------
CYCLE_FIELDS = ("F_POS", "F_VEL", "F_MASS", "F_TYPE", "F_HSML", "F_TIMEBIN", "F_TI_BEGSTEP", "F_ID", "F_GRAVACCEL",
                "F_TI_CURRENT", "F_VELPRED", "F_ENTROPY", "F_DTENTROPY")


def _cycle_shards(cc):
    """CycleCase of tests/test_gpu_wind_resident.py on 3 shards: the fields, the sink tables, the integrator's flags"""
    from test_gpu_kick_bundle import flags_struct
    sc = cc.sc
    T = Shards(sc.c, 3, trees=False)
    B, S = T.B, T.S
    glob = dict(F_TYPE=sc.type, F_MASS=sc.mass, F_HSML=cc.hsml, F_TIMEBIN=cc.timebin, F_ID=sc.ids.view(np.int32))
    glob.update(cc.fields)
    for k, v in glob.items():
        S.set_field(getattr(B, k), v)
    rows = cc.sink_rows(B)
    owner = S.owner[sc.sinks]
    for r, fp in enumerate(S.fp):
        mine = np.where(owner == r)[0]
        fp.sinks_set_table(sc.ids[sc.sinks[mine]], rows[mine].reshape(len(mine), B.SK_COUNT))
        fp.set_integration_flags(flags_struct(cc.flags))
        fp.set_wind_rad_accel(np.zeros((fp.ngas, 3)))
        fp.set_active(np.arange(fp.n, dtype=np.int32))
    return T


PASS_OUTPUTS = ("F_GRAVACCEL", "F_OLDACC", "F_HSML", "F_DENSITY", "F_DIVVEL", "F_PRESSURE", "F_MAXSIGNALVEL",
                "F_HYDROACCEL")


def _cycle_trees(T, pr):
    """the trees of the step (GHIP_DD_GRAVITY, GHIP_DD_DENSITY).  The cycle needs the trees, not the passes' numbers:
    what they wrote is put back, so that the kick sees the accelerations and signal velocities of CycleCase, which
    keep everybody in its time bin (setting these fields leaves the trees in place)"""
    B = T.B
    keep = [{f: fp.get_field(getattr(B, f)) for f in PASS_OUTPUTS} for fp in T.S.fp]
    T.S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
    T.S.run.density(B.DensParams(pr.des_ngb, 1e9, pr.min_gas_hsml, pr.box, pr.periodic, pr.ti_current, pr.timebase, 150))
    for fp, old in zip(T.S.fp, keep):
        for f, v in old.items():
            if len(v):
                fp.set_field(getattr(B, f), v)


def _keys(B, fp):
    """what a host follows a particle by through a migration: ID, Pos and Vel together (two live wind particles can
    carry one ID, and the particles a sink emits in one step share its position)"""
    ids, pos, vel = fp.get_field(B.F_ID), fp.get_field(B.F_POS), fp.get_field(B.F_VEL)
    return [ids[i].tobytes() + pos[i].tobytes() + vel[i].tobytes() for i in range(fp.n)]


def test_three_steps_of_the_cycle_on_shards_equal_a_host_driven_set():
    """Accretion (resident form), form 32, form 33, the kick, the sync-point form and redistribute(rearrange,
    peano_order) on 3 shards, three times.  The second ShardSet is driven by a host that keeps the wind state itself:
    GHIP_WIND_FORM with host arrays on the lists it selects, the new particles through download, append,
    ghip_set_counts and upload (with the values the first set gave them, so that the comparison stays bit for bit),
    its rows carried through ghip_rearrange by the map and through the migration and the order by (ID, Pos, Vel)."""
    from test_gpu_wind_resident import CYCLE_BIN, CycleCase
    cc = CycleCase()
    sc, c, pr = cc.sc, cc.sc.c, cc.sc.c.pr
    TA, TB = _cycle_shards(cc), _cycle_shards(cc)
    try:
        B, SA, SB = TA.B, TA.S, TB.S
        wrows = cc.wind_rows(B)
        for r, fp in enumerate(SA.fp):
            fp.dd_winds_set_table(TA.local[r], wrows[TA.lists[r]])
        hidx = [np.sort(TB.local[r]).astype(np.int32) for r in range(3)]           # the host's own wind state
        hrows = [wrows[TB.lists[r]][np.argsort(TB.local[r], kind="stable")] for r in range(3)]
        decomp = B.DecompParams(0, 0, 1, 0)
        spawned, eliminated, moved = [], [], []
        for k in (1, 2, 3):
            Time, wp, sp, kp, bh, acc = cc.step_params(B, k)
            # ---- the resident set
            _cycle_trees(TA, pr)
            SA.run.blackhole_accretion(bh, acc)
            ra = SA.run.winds_feedback(wp)
            n_old = [fp.n for fp in SA.fp]
            reps = SA.run.wind_spawn(sp, sc.rnd)
            assert all(rep["tot_spawned"] == sum(q["spawned"] for q in reps) for rep in reps)
            # ---- the host-driven set
            _cycle_trees(TB, pr)
            SB.run.blackhole_accretion(bh, acc)
            sels, built = [], []
            for r, fp in enumerate(SB.fp):
                act = fp.get_active()
                pos_of = {int(i): j for j, i in enumerate(hidx[r])}
                sel = np.array([pos_of[int(i)] for i in act if int(i) in pos_of], np.int64)
                sel = sel[hrows[r][sel, B.WK_STELLAR_AGE] < Time] if len(sel) else sel
                sels.append(sel)
                st = dict(stellar_age=hrows[r][sel, B.WK_STELLAR_AGE], birth_energy=hrows[r][sel, B.WK_BIRTH_ENERGY],
                          old_momentum=hrows[r][sel, B.WK_OLD_MOMENTUM], new_density=hrows[r][sel, B.WK_NEW_DENSITY],
                          drmin=hrows[r][sel, B.WK_DRMIN])
                built.append(B.dd_wind_args(wp, hidx[r][sel], state=st))
            SB.run.run(B.WIND_OP, [b[0] for b in built], B.WIND_FORM)
            for r, fp in enumerate(SB.fp):
                out = B.dd_wind_result(built[r][1])
                for key in ("iterations", "bits", "ndeleted", "deleted_momentum"):
                    assert ra[r][key] == out[key], (k, r, key, ra[r][key], out[key])
                if len(sels[r]):
                    for col, name in OUT_COLS:
                        hrows[r][sels[r], getattr(B, col)] = out[name]
                # the host's spawn: everything down, the new particles appended, the new counts, everything up
                t = reps[r]["spawned"]
                if t:
                    fa = SA.fp[r]
                    down = [fp.get_field(f) for f in range(B.F_COUNT)]
                    new = [fa.get_field(f) for f in range(B.F_COUNT)]
                    ids, srows = fp.sinks_table()
                    inj, rad = fp.wind_injected(), fp.wind_rad_accel()
                    active = fp.get_active()
                    fp.set_counts(n_old[r] + t, fp.ngas)
                    for f in range(B.F_COUNT):
                        gas = B._FIELD_INFO[f][0]
                        fp.set_field(f, down[f] if gas else np.concatenate([down[f], new[f][n_old[r]:]]))
                    fp.sinks_set_table(ids, srows)
                    fp.set_wind_injected(inj)
                    fp.set_wind_rad_accel(rad)
                    fp.set_active(np.r_[active, np.arange(n_old[r], n_old[r] + t)].astype(np.int32))
                    gi, grows = fa.dd_winds_table()
                    _same(gi[-t:], np.arange(n_old[r], n_old[r] + t).astype(np.int32), "keys of the new rows")
                    hidx[r] = np.r_[hidx[r], gi[-t:]].astype(np.int32)
                    hrows[r] = np.vstack([hrows[r], grows[-t:]])
            spawned.append(sum(q["spawned"] for q in reps))
            eliminated.append(sum(q["ndeleted"] for q in ra))
            # ---- both: the kick, the next sync point, the decomposition
            nexts = []
            for S in (SA, SB):
                for fp in S.fp:
                    fp.advance_timesteps(kp)
                nexts.append([s.Ti_next for s in S.run.sync_point(k << CYCLE_BIN)])
            print("step %d: Ti_next" % k, nexts, "expected", (k + 1) << CYCLE_BIN)
            assert nexts[0] == nexts[1] == [(k + 1) << CYCLE_BIN] * 3, nexts
            SA.run.redistribute(decomp, rearrange=True, peano_order=True)
            want = {}
            for r, fp in enumerate(SB.fp):
                fp.rearrange()
                new_of_old, _ = fp.sequence_map()
                j = new_of_old[hidx[r]]
                hrows[r], hidx[r] = hrows[r][j >= 0], j[j >= 0].astype(np.int32)
                key = _keys(B, fp)
                for i, row in zip(hidx[r], hrows[r]):
                    assert key[i] not in want
                    want[key[i]] = (r, row)
            SB.run.decompose(decomp)
            SB.run.migrate()
            nmoved = 0
            for r, fp in enumerate(SB.fp):
                fp.peano_order()
                found = [(i, want[q]) for i, q in enumerate(_keys(B, fp)) if q in want]
                hidx[r] = np.array([i for i, _ in found], np.int32)
                hrows[r] = np.array([w[1] for _, w in found]).reshape(len(found), B.WK_COUNT)
                nmoved += sum(1 for _, w in found if w[0] != r)
            assert sum(len(x) for x in hidx) == len(want)
            moved.append(nmoved)
            # ---- after the step: the fields, the wind state and the tables, bit for bit, shard by shard
            for r, (fa, fb) in enumerate(zip(SA.fp, SB.fp)):
                assert (fa.n, fa.ngas) == (fb.n, fb.ngas)
                for f in CYCLE_FIELDS:
                    _same(fa.get_field(getattr(B, f)), fb.get_field(getattr(B, f)), "%s of shard %d, step %d" % (f, r, k))
                gi, grows = fa.dd_winds_table()
                _same(gi, hidx[r], "wind indices of shard %d after step %d" % (r, k))
                _same(grows, hrows[r], "wind rows of shard %d after step %d" % (r, k))
                _same(np.c_[fa.sinks_table()], np.c_[fb.sinks_table()], "sink table")
                _same(fa.wind_injected(), fb.wind_injected(), "Injected_BH_Momentum")
                _same(fa.wind_rad_accel(), fb.wind_rad_accel(), "RadAccel")
                _same(fa.get_active(), fb.get_active(), "active list")
        print("cycle on shards: spawned", spawned, "eliminated", eliminated, "rows that changed shards", moved)
        assert spawned[0] > 100, spawned
        assert max(eliminated) >= 1, eliminated
        assert sum(len(x) for x in hidx) == len(c.wind) + sum(spawned) - sum(eliminated)
    finally:
        TA.close()
        TB.close()
