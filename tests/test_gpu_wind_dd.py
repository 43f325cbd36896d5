"""The wind particles on domain-decomposed shards (GHIP_DD_WIND begun with one of the wind forms as `walk`: the loop of
momentum_feedback() and its two single passes): logical shards in one process (ShardSet) against the numpy
restatement of tests/wind_ref.py, the inputs of tests/test_gpu_wind.py; the resident Injected_BH_Momentum / RadAccel
through GHIP_DD_MIGRATE and in the integrator; two rank processes through the host all-gather and the RCCL entry
points.  fp64 within 1e-12 of the field's largest magnitude; every loop test first asserts that the restatement's
smallest decision margin is >= 1e-9; two identical runs bit-identical."""
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import kick_ref as KR
import wind_ref as R
from common import ShardSet, bindings, failing_collective, relerr
from test_gpu_kick_bundle import FIELDS as KICK_FIELDS, flags_struct, kick_params
from test_gpu_wind import MARGIN, TOL, UNTOUCHED, WindCase, _case, _check_loop, _loop_ref, _scaled_err
from test_kick_bundle_cpu import problem as kick_problem

pytestmark = pytest.mark.gpu
CASES = [(2, 0, 1), (3, 1, 1), (8, 0, 1), (8, 1, 1), (3, 1, 4)]      # shards, periodic, domains


class DdWind:
    """A WindCase on `nshards` logical shards with the trees of this step (GHIP_DD_GRAVITY, _DENSITY); every shard's
    list is its part of the case's list (S.locate), in the case's order.  dom / rank: this process is one rank of
    several (tests/gpu_host_ranks_wind.py): the collectives go through `dom` and only shard `rank` is real."""

    def __init__(self, case, nshards, domains=1, trees=True, contexts=None, dom=None, rank=None):
        B = bindings()
        pr = case.pr
        self.case, self.B, self.P, self.dom, self.rank = case, B, nshards, dom, rank
        S = ShardSet(pr, nshards, fields=dict(hsml=case.hsml), domains=domains, contexts=contexts)
        self.S = S
        S.set_field(B.F_MASS, case.mass)
        S.set_field(B.F_TIMEBIN, case.timebin)
        if trees:
            self.trees()
        where = S.locate(case.wind)
        self.local = [w[0] for w in where]
        self.lists = [w[1] for w in where]
        assert sum(len(x) for x in self.lists) == len(case.wind)
        self.active = [w[0] for w in S.locate(case.active)]

    def run(self, op, args, walk=0):
        if self.dom is not None:
            self.dom._run(op, args[self.rank], walk)
        else:
            self.S.run.run(op, args, walk)

    def trees(self):
        B, pr = self.B, self.case.pr
        self.run(B.DD_GRAVITY, [pr.g_grav(pr.theta)] * self.P, B.WALK_NEWTON)
        # (the operation needs the gas tree of GHIP_DD_DENSITY, not its numbers: every h counts as converged, so the
        # massless slab and the slab of small h_j do not send the iteration anywhere)
        dens = B.DensParams(pr.des_ngb, 1e9, pr.min_gas_hsml, pr.box, pr.periodic, pr.ti_current, pr.timebase, 150)
        self.run(B.DD_DENSITY, [dens] * self.P)
        self.S.set_field(B.F_HSML, self.case.hsml)        # (the density pass wrote the gas's)

    def shards(self):
        return range(self.P) if self.rank is None else [self.rank]

    def density(self, dtj, **over):
        B, c = self.B, self.case
        built = [B.dd_wind_args(c.gparams(**over), self.local[r], dt_jump=dtj[self.lists[r]]) for r in range(self.P)]
        self.run(B.WIND_OP, [b[0] for b in built], B.WIND_DENSITY_FORM)
        rho, drmin = np.zeros(len(c.wind)), np.zeros(len(c.wind))
        for r in self.shards():
            rho[self.lists[r]], drmin[self.lists[r]] = built[r][1]["new_density"], built[r][1]["drmin"]
        return rho, drmin, [b[1]["counts"].copy() for b in built]

    def spread(self, dtj, rho, dmom):
        B, c = self.B, self.case
        built = [B.dd_wind_args(c.gparams(), self.local[r], dt_jump=dtj[o], new_density=rho[o], delta_momentum=dmom[o])
                 for r, o in enumerate(self.lists)]
        self.run(B.WIND_OP, [b[0] for b in built], B.WIND_SPREAD_FORM)
        return [b[1]["counts"].copy() for b in built]

    def loop_args(self, lists=None, bad=None, **over):
        B, c = self.B, self.case
        built = []
        for r in range(self.P):
            o = self.lists[r] if lists is None else lists[r]
            loc = self.local[r] if lists is None else self.local[r][:len(o)]
            if bad == r:
                loc = loc.copy()
                loc[len(loc) // 2] = 0                     # a gas particle of this shard
            built.append(B.dd_wind_args(c.gparams(**over), loc, state=c.state(o)))
        return built

    def loop(self, lists=None, **over):
        """-> (out of the whole list as ForcePath.wind_feedback returns it, per-shard results)"""
        B, c = self.B, self.case
        built = self.loop_args(lists, **over)
        self.run(B.WIND_OP, [b[0] for b in built], B.WIND_FORM)
        per = [B.dd_wind_result(b[1]) for b in built]
        nw = len(c.wind)
        out = {k: np.zeros(nw, np.int32 if k == "deleted" else np.float64)
               for k in ("old_momentum", "new_density", "drmin", "dt1", "dt2", "dt_jump", "delta_momentum", "deleted")}
        for r in self.shards():
            o = self.lists[r] if lists is None else lists[r]
            for k in out:
                out[k][o] = per[r][k]
        its = [per[r]["iterations"] for r in self.shards()]
        assert len(set(its)) == 1, its                     # the global count, on every shard
        out.update(rc=0, iterations=its[0], bits=sum(int(per[r]["bits"]) for r in self.shards()),
                   ndeleted=sum(per[r]["ndeleted"] for r in self.shards()), deleted_momentum=0.0)
        for r in self.shards():                            # (the host adds them in rank order)
            out["deleted_momentum"] += per[r]["deleted_momentum"]
        return out, per

    def gas(self, getter):
        S = self.S
        out = np.zeros((self.case.pr.ngas, 3))
        for r in self.shards():
            out[S.gid[r][:S.ngas[r]]] = getattr(S.fp[r], getter)()
        return out

    def set_gas(self, setter, glob):
        S = self.S
        for r in self.shards():
            getattr(S.fp[r], setter)(glob[S.gid[r][:S.ngas[r]]])

    def injected(self):
        return self.gas("wind_injected")

    def rad_accel(self):
        return self.gas("wind_rad_accel")

    def set_active(self):
        for r in self.shards():
            self.S.fp[r].set_active(self.active[r])

    # what _check_loop of test_gpu_wind.py asks of a context
    def get_field(self, f):
        return self.S.get_field(f)

    def wind_injected(self):
        return self.injected()

    def resident(self):
        B = self.B
        return {f: self.S.get_field(f) for f in [B.F_POS, B.F_HSML, B.F_MASS] + [getattr(B, k) for k in UNTOUCHED]}

    def close(self):
        self.S.close()


def _dtj(c):
    dtj = c.dt_jump()
    dtj[::7] = -1.0                                        # reset, not evaluated
    return dtj


@functools.lru_cache(maxsize=None)
def _density_ref(periodic):
    c = _case(periodic)
    f, M = c.fields(), R.Margins()
    rr, rd = R.density(c.par, R.gas_of(f), f["pos"][c.wind], f["hsml"][c.wind], _dtj(c), M)
    return rr, rd, M


@pytest.mark.parametrize("nshards,periodic,domains", CASES)
def test_density_form(nshards, periodic, domains):
    c = _case(periodic)
    rr, rd, M = _density_ref(periodic)
    assert M.smallest() >= MARGIN, M.by_kind
    T = DdWind(c, nshards, domains)
    try:
        before = T.resident()
        rho, drmin, cnt = T.density(_dtj(c))
        off = ~(_dtj(c) > 0)
        assert np.all(rho[off] == 0) and np.all(drmin[off] == 1.e40)
        print("density: err", _scaled_err(rho, rr), relerr(drmin, rd), "sent", [int(k[0]) for k in cnt])
        assert _scaled_err(rho, rr) < TOL
        assert np.array_equal(drmin == 1.e40, rd == 1.e40) and relerr(drmin, rd) < TOL
        sent = sum(int(k[0]) for k in cnt)
        assert sent > 0 and sent == sum(int(k[1]) for k in cnt)
        assert all(k[4] > 0 for k in cnt if k[0] > 0) and all(k[3] == 3 for k in cnt)
        for f, v in before.items():
            assert np.array_equal(T.S.get_field(f), v), f
    finally:
        T.close()


@pytest.mark.parametrize("nshards,periodic,domains", CASES)
def test_spread_form(nshards, periodic, domains):
    c = _case(periodic)
    f = c.fields()
    ng, nw = c.pr.ngas, len(c.wind)
    dtj = c.dt_jump()
    M = R.Margins()
    rho, _ = R.density(c.par, R.gas_of(f), f["pos"][c.wind], f["hsml"][c.wind], dtj, M)
    dmom = c.old * (0.1 + 0.5 * np.random.default_rng(9).random(nw))
    inj = np.zeros((ng, 3), R.LD)
    sp = R.spread(c.par, R.gas_of(f), f["pos"][c.wind], f["hsml"][c.wind], f["vel"][c.wind], dtj, rho, dmom, inj, M)
    assert M.smallest() >= MARGIN, M.by_kind
    ref = inj.astype(np.float64)
    T = DdWind(c, nshards, domains)
    try:
        before = T.resident()
        assert np.all(T.injected() == 0)                  # zero when first used
        cnt = T.spread(dtj, rho, dmom)
        got = T.injected()
        print("spread: err", _scaled_err(got, ref), "imported pairs", [int(k[2]) for k in cnt])
        assert _scaled_err(got, ref) < TOL and np.abs(ref).max() > 0
        assert sum(int(k[2]) for k in cnt) > 0             # pairs across shards
        v = f["vel"][c.wind][sp]
        given = (dmom[sp][:, None] * v / np.linalg.norm(v, axis=1)[:, None]).sum(axis=0)
        assert np.abs(got.sum(axis=0) - given).max() < 1e-11 * np.abs(dmom[sp]).sum()
        reached = np.any(ref != 0, axis=1)
        assert (~reached).sum() > 100 and np.all(got[~reached] == 0)    # gas nobody reaches stays bit-zero
        for k, val in before.items():
            assert np.array_equal(T.S.get_field(k), val), k
    finally:
        T.close()


def test_spread_of_imported_particles_alone_of_mixed_runs_and_without_pairs():
    """The three shapes of a shard's scatter, on two shards.  A shard that lists no wind particle and imports some: its
    gas receives pairs, all of imported particles.  Both shards with lists: gas particles receive own and imported
    particles in one run.  new_density = 0 everywhere: no pair anywhere, Injected_BH_Momentum stays bit-zero."""
    c = _case(0)
    f = c.fields()
    ng, nw = c.pr.ngas, len(c.wind)
    dtj = c.dt_jump()
    M = R.Margins()
    rho, _ = R.density(c.par, R.gas_of(f), f["pos"][c.wind], f["hsml"][c.wind], dtj, M)
    dmom = c.old * (0.1 + 0.5 * np.random.default_rng(9).random(nw))

    def ref_of(sub):                                       # what the gas receives from the particles `sub` of the list
        inj = np.zeros((ng, 3), R.LD)
        w = c.wind[sub]
        R.spread(c.par, R.gas_of(f), f["pos"][w], f["hsml"][w], f["vel"][w], dtj[sub], rho[sub], dmom[sub], inj, M)
        return inj.astype(np.float64)

    for own1 in (False, True):
        T = DdWind(c, 2)
        try:
            if not own1:
                T.lists[1], T.local[1] = T.lists[1][:0], T.local[1][:0]
            parts = [ref_of(o) for o in T.lists]
            assert M.smallest() >= MARGIN, M.by_kind
            cnt = T.spread(dtj, rho, dmom)
            got, ref = T.injected(), parts[0] + parts[1]
            assert _scaled_err(got, ref) < TOL and np.abs(ref).max() > 0
            gas1 = T.S.gid[1][:T.S.ngas[1]]
            if not own1:
                assert int(cnt[1][0]) == 0 and int(cnt[1][1]) > 0 and int(cnt[1][2]) > 0
                assert np.abs(got[gas1]).max() > 0
            else:
                for r in range(2):
                    gas = T.S.gid[r][:T.S.ngas[r]]
                    assert np.count_nonzero(np.any(parts[0][gas] != 0, axis=1) & np.any(parts[1][gas] != 0, axis=1)) > 0
        finally:
            T.close()
    T = DdWind(c, 2)
    try:
        cnt = T.spread(dtj, np.zeros(nw), dmom)
        assert all(int(k[2]) == 0 for k in cnt) and sum(int(k[1]) for k in cnt) > 0
        assert np.all(T.injected() == 0)
    finally:
        T.close()


def _check_rad_accel(c, T, ref, ra0):
    ng = c.pr.ngas
    touched = ref["rad_touched"]
    ra = T.rad_accel()
    assert _scaled_err(ra[touched], ref["rad_accel"][touched]) < TOL and np.abs(ref["rad_accel"]).max() > 0
    assert np.array_equal(ra[~touched], ra0[~touched])
    assert np.all(T.injected()[touched] == 0) and np.abs(ref["injected"][~touched]).max() > 0
    assert np.all(ra[touched & (c.timebin[:ng] == 0)] == 0)


def _run_loop(c, nshards, domains, ref):
    T = DdWind(c, nshards, domains)
    try:
        T.set_active()
        ra0 = np.random.default_rng(6).standard_normal((c.pr.ngas, 3))
        T.set_gas("set_wind_rad_accel", ra0)
        start = T.resident()
        out, per = T.loop()
        print("loop: iterations", out["iterations"], ref["iterations"], "bits", out["bits"], ref["bits"],
              "counts", [p["counts"].tolist() for p in per])
        _check_loop(c, T.B, T, out, ref, start)
        _check_rad_accel(c, T, ref, ra0)
        sent = sum(int(p["counts"][0]) for p in per)
        assert sent > 0 and sent == sum(int(p["counts"][1]) for p in per)
        assert all(int(p["counts"][5]) == ref["iterations"] for p in per)
        assert all(int(p["counts"][3]) == 3 + 4 * ref["iterations"] for p in per)   # exchanges: begin, start, 4 each
        return out, T.resident(), T.injected(), T.rad_accel()
    finally:
        T.close()


@pytest.mark.parametrize("nshards,periodic,domains", CASES)
def test_loop_matches_the_restatement(nshards, periodic, domains):
    c, ref = _case(periodic), _loop_ref(periodic)
    assert ref["margins"].smallest() >= MARGIN, ref["margins"].by_kind
    assert ref["status"] == "ok" and ref["iterations"] > 8
    _run_loop(c, nshards, domains, ref)


def test_loop_in_a_box_of_four():
    """WindCase(box=4.0) on 3 shards against the restatement on the same scaled inputs: iterations, bits and every
    quantity of _check_loop.  The loop converts with cgs units (the optical depth, the time cap), so the box of 4 does
    NOT repeat the unit box's counts, on the CPU already: the restatement gives 18 iterations and 1 947 basic steps
    there against 23 and 2 781 in the unit box (periodic: 23 / 1 835 against 43 / 3 466), as
    test_gpu_box_scale.py::test_wind_feedback_in_a_periodic_box_of_4 says of one GPU ("no law").  What the device
    must equal is the restatement in the same box."""
    unit = _loop_ref(0)
    c = WindCase(0, box=4.0)
    ref = R.feedback(c.par, c.fields(), c.wind, c.state(), active=c.active)
    assert ref["margins"].smallest() >= MARGIN, ref["margins"].by_kind
    assert ref["status"] == "ok" and (ref["iterations"], ref["bits"]) == (18, 1947)
    assert (unit["iterations"], unit["bits"]) == (23, 2781)
    out, *_ = _run_loop(c, 3, 1, ref)
    assert out["iterations"] == ref["iterations"] and out["bits"] == ref["bits"]


def test_two_runs_are_bit_identical():
    c, ref = _case(1), _loop_ref(1)
    assert ref["margins"].smallest() >= MARGIN
    a, b = _run_loop(c, 3, 1, ref), _run_loop(c, 3, 1, ref)
    for k in a[0]:
        assert np.array_equal(a[0][k], b[0][k]), k
    for f in a[1]:
        assert np.array_equal(a[1][f], b[1][f]), f
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_lock_step():
    c = _case(0)
    T = DdWind(c, 3)
    try:
        P, B = T.P, T.B
        empty = [np.zeros(0, np.int64)] * P
        start = T.resident()
        # all lists empty: every shard returns 0 after the same number of steps (dd_run_local holds them to that)
        out, per = T.loop(lists=empty)
        assert out["iterations"] == 0 and out["bits"] == 0 and all(int(p["counts"][3]) == 1 for p in per)
        # the global sum under the floor: nothing changes anywhere
        out, per = T.loop(dt_total_floor=float(c.dt_jump().sum()) * 1.001)
        assert out["iterations"] == 0 and out["bits"] == 0 and out["ndeleted"] == 0
        assert np.array_equal(out["dt_jump"], c.dt_jump()) and np.array_equal(out["old_momentum"], c.old)
        now = T.resident()
        for f in start:
            assert np.array_equal(now[f], start[f]), f
        assert np.all(T.injected() == 0)
        # one shard's own sum under the floor, the global sum above it: the loop runs
        sums = [float(c.dt_jump()[o].sum()) for o in T.lists]
        floor = 1.01 * min(sums)
        assert min(sums) > 0 and floor < 0.5 * sum(sums)
        ref = R.feedback(dict(c.par, dt_total_floor=floor), c.fields(), c.wind, c.state(), active=c.active)
        assert ref["status"] == "ok" and ref["margins"].smallest() >= MARGIN
        T.set_active()
        out, _ = T.loop(dt_total_floor=floor)
        _check_loop(c, B, T, out, ref, start)
    finally:
        T.close()
    # only shard 0 passes its list
    T = DdWind(c, 3)
    try:
        sub = T.lists[0]
        assert 50 < len(sub) < len(c.wind)
        ref = R.feedback(c.par, c.fields(), c.wind[sub], c.state(sub), active=c.active)
        assert ref["status"] == "ok" and ref["margins"].smallest() >= MARGIN
        T.set_active()
        out, per = T.loop(lists=[sub] + [np.zeros(0, np.int64)] * (T.P - 1))
        assert out["iterations"] == ref["iterations"] and out["bits"] == ref["bits"]
        assert sum(int(p["counts"][1]) for p in per[1:]) > 0           # the others took part
        assert np.array_equal(out["deleted"][sub], ref["deleted"]) and out["ndeleted"] == ref["ndeleted"]
        for k in ("old_momentum", "dt2", "dt1", "dt_jump", "delta_momentum", "new_density"):
            assert _scaled_err(out[k][sub], ref[k]) < TOL, k
        assert _scaled_err(T.S.get_field(T.B.F_POS)[c.wind[sub]], ref["pos"][c.wind[sub]]) < TOL
        assert _scaled_err(T.rad_accel()[ref["rad_touched"]], ref["rad_accel"][ref["rad_touched"]]) < TOL
    finally:
        T.close()


def test_a_failure_on_one_shard_ends_the_operation_on_all():
    c = _case(0)
    T = DdWind(c, 3)
    try:
        B = T.B
        start = T.resident()
        built = T.loop_args(bad=1)
        errs = failing_collective(T.S.fp, B.WIND_OP, [b[0] for b in built], B.WIND_FORM)
        assert "not Type 3" in str(errs[1]) and errs[1].code == -90002
        assert all("shard 1" in str(errs[r]) for r in (0, 2))
        now = T.resident()
        for f in start:
            assert np.array_equal(now[f], start[f]), f
        assert np.all(T.injected() == 0)
        ref = R.feedback(dict(c.par, max_iter=3), c.fields(), c.wind, c.state(), active=c.active)
        assert ref["status"] == "noconv" and ref["margins"].smallest() >= MARGIN
        built = T.loop_args(max_iter=3)
        errs = failing_collective(T.S.fp, B.WIND_OP, [b[0] for b in built], B.WIND_FORM)
        assert all(e.code == B.GHIP_ENOCONV for e in errs)
        assert all(("%d wind particles still under way" % ref["under_way"]) in str(e) for e in errs)
        assert all(B.dd_wind_result(b[1])["iterations"] == 3 for b in built)
    finally:
        T.close()


def test_refusals():
    c = _case(0)
    T = DdWind(c, 2, trees=False)
    try:
        B, pr = T.B, c.pr
        args = T.loop_args()
        for fp, a in zip(T.S.fp, args):
            with pytest.raises(B.GhipError, match="run GHIP_DD_GRAVITY of this step first") as e:
                fp.dd_begin(B.WIND_OP, a[0], B.WIND_FORM)
            assert e.value.code == -90002
        T.run(B.DD_GRAVITY, [pr.g_grav(pr.theta)] * T.P, B.WALK_NEWTON)
        for fp, a in zip(T.S.fp, args):
            with pytest.raises(B.GhipError, match="run GHIP_DD_DENSITY of this step first"):
                fp.dd_begin(B.WIND_OP, a[0], B.WIND_FORM)
        T.trees()
        fp = T.S.fp[0]
        for walk in (3, B.WIND_SPREAD_FORM + 1):
            with pytest.raises(B.GhipError, match="GHIP_WIND_DENSITY_FORM") as e:
                fp.dd_begin(B.WIND_OP, args[0][0], walk)
            assert e.value.code == -90002
        with pytest.raises(B.GhipError, match="neither 0 nor") as e:      # the dust density hosts no wind form
            fp.dd_begin(B.DD_DUST_DENSITY, args[0][0], B.WIND_FORM)
        assert e.value.code == -90002
        loc, dtj = T.local[0], c.dt_jump()[T.lists[0]]
        st = c.state(T.lists[0])
        for call in (lambda: fp.wind_density(c.gparams(), loc, dtj), lambda: fp.wind_spread(c.gparams(), loc, dtj, dtj, dtj),
                     lambda: fp.wind_feedback(c.gparams(), loc, st["stellar_age"], st["birth_energy"], st["old_momentum"],
                                              st["new_density"], st["drmin"])):
            with pytest.raises(B.GhipError, match="GHIP_DD_WIND") as e:
                call()
            assert e.value.code == -90002
    finally:
        T.close()


def test_the_gas_fields_migrate_with_their_particles():
    c = _case(1)
    T = DdWind(c, 3, trees=False)
    try:
        B, S, pr = T.B, T.S, c.pr
        ng = pr.ngas
        code = np.arange(3 * ng, dtype=np.float64).reshape(ng, 3)
        T.set_gas("set_wind_injected", code + 0.25)
        T.set_gas("set_wind_rad_accel", -code - 0.5)
        rng = np.random.default_rng(3)
        pos = pr.ic["pos"].copy()
        movers = rng.choice(ng, 300, replace=False)
        pos[movers] = pos[rng.permutation(movers)] + 1e-4
        owner0 = S.owner.copy()
        S.set_field(B.F_POS, pos)
        S.migrate()
        assert 100 < (S.owner[:ng] != owner0[:ng]).sum() <= 300
        assert np.array_equal(T.injected(), code + 0.25) and np.array_equal(T.rad_accel(), -code - 0.5)
        # a field held for another gas count is not carried
        fp = S.fp[0]
        n0, g0 = fp.counts()
        fp.set_counts(n0, g0 - 1)
        fp.set_wind_injected(np.ones((g0 - 1, 3)))
        fp.set_counts(n0, g0)
        pos[movers] = pr.ic["pos"][movers]
        S.set_field(B.F_POS, pos)
        S.migrate()
        assert (S.owner[:ng] != owner0[:ng]).sum() == 0
        assert np.all(fp.wind_injected() == 0)
        assert np.array_equal(T.rad_accel(), -code - 0.5)
    finally:
        T.close()


def _kick_shards(s, mode, ra, f, p, act, nshards=3):
    """advance_timesteps and drift on `nshards` ghip_dd_init contexts that hold every nshards-th particle (or, nshards
    = 0, on one plain context); -> the fields in global order"""
    B = bindings()
    n, ng = len(s["type"]), len(s["entropy"])
    parts = [(np.arange(ng), np.arange(ng, n))] if nshards == 0 else \
        [(np.arange(r, ng, nshards), np.arange(ng + r, n, nshards)) for r in range(nshards)]
    names = ("F_VEL", "F_VELPRED", "F_ENTROPY", "F_DTENTROPY", "F_TIMEBIN", "F_TI_BEGSTEP", "F_POS")
    out = {k: None for k in names}
    isact = np.zeros(n, bool)
    isact[act] = True
    for r, (g, o) in enumerate(parts):
        idx = np.concatenate([g, o])
        nl, ngl = len(idx), len(g)
        fp = B.ForcePath(0)
        fp.set_counts(nl, ngl)
        fp.set_field(B.F_POS, np.zeros((nl, 3)))
        fp.set_field(B.F_TI_CURRENT, np.zeros(nl, np.int32))
        fp.set_field(B.F_DIVVEL, np.zeros(ngl))
        fp.set_field(B.F_PRESSURE, np.zeros(ngl))
        for fld, k in KICK_FIELDS:
            v = np.asarray(s[k])
            fp.set_field(getattr(B, fld), v[g] if len(v) == ng else v[idx])
        if nshards:
            fp.dd_init(r, nshards)
        fp.set_integration_flags(flags_struct(f))
        fp.set_active(np.flatnonzero(isact[idx]).astype(np.int32))
        if mode != "never":
            fp.set_wind_rad_accel(ra[g])
            fp.set_rad_accel(mode == "on")
        fp.advance_timesteps(kick_params(p))
        fp.set_field(B.F_TI_CURRENT, np.full(nl, p["Ti_Current"], np.int32))
        fp.set_field(B.F_DIVVEL, (0.1 * np.random.default_rng(2).standard_normal(ng))[g])
        fp.drift(p["Ti_Current"] + (1 << 22), p["Timebase_interval"])
        for k in names:
            v = fp.get_field(getattr(B, k))
            gas = B._FIELD_INFO[getattr(B, k)][0]
            if out[k] is None:
                out[k] = np.zeros((ng if gas else n,) + v.shape[1:], v.dtype)
            out[k][g if gas else idx] = v
        if mode == "off":
            assert np.array_equal(fp.wind_rad_accel(), ra[g])          # resident, and not read
        fp.close()
    return out


def test_rad_accel_in_the_kick_and_the_drift_on_shards():
    f = KR.bundle(OuterBoundary=300.0, FeedBackVelocity=10.0, dust=0, dust_timestep=0)
    p, s, _ = kick_problem(seed=13, ngas=3000, nother=2000, types=(1, 3, 5))
    s["drag"][:] = 0
    s["ddm"][:] = 0
    n, ng = len(s["type"]), len(s["entropy"])
    ra = np.random.default_rng(21).standard_normal((ng, 3)) * 4.0
    act = np.random.default_rng(4).permutation(n)[: n // 2].astype(np.int32)
    res = {m: _kick_shards(s, m, ra, f, p, act) for m in ("on", "off", "never")}
    plain = _kick_shards(s, "on", ra, f, p, act, nshards=0)
    for k in plain:                                        # per-particle arithmetic, no sums: the bits of one context
        assert np.array_equal(res["on"][k], plain[k]), k
        assert np.array_equal(res["off"][k], res["never"][k]), k
    assert not np.array_equal(res["on"]["F_VEL"], res["never"]["F_VEL"])
    assert not np.array_equal(res["on"]["F_VELPRED"], res["never"]["F_VELPRED"])


def _run_ranks(transport):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", WIND_TRANSPORT=transport)
    if transport == "rccl":
        mock = os.path.join(root, "tests", "mock_rccl", "librccl_mock.so")
        assert os.path.exists(mock), "build tests/mock_rccl first (__graft_entry__.build())"
        env["GHIP_RCCL_LIB"] = mock
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "tests", "gpu_host_ranks_wind.py")]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_two_rank_processes_equal_the_in_process_run():
    """tests/gpu_host_ranks_wind.py is the rank program: the loop on two rank processes, through the host's all-gather
    (gloo) and through the RCCL entry points (tests/mock_rccl: the real RCCL refuses two ranks on one device); rank 0
    compares with the run of both shards in its own process."""
    bytes_sent = {}
    for transport in ("host", "rccl"):
        out = _run_ranks(transport)
        assert out["ok"], out
        assert out["transport"] == transport
        if transport == "rccl":
            assert out["rccl_library"].endswith("librccl_mock.so")
        assert out["iterations"] == _loop_ref(1)["iterations"]
        assert out["outputs_equal"] and out["resident_equal"], out
        assert all(b > 0 for b in out["bytes_wind"])
        bytes_sent[transport] = out["bytes_wind"]
    assert bytes_sent["host"] == bytes_sent["rccl"]
