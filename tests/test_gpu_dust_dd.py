"""The dust-gas drag passes on domain-decomposed shards (GHIP_DD_DUST_DENSITY / GHIP_DD_DUST_DRAG): logical
shards in one process (ShardSet) against the numpy restatement of tests/dust_ref.py, with the reference's
multi-rank scatter order of tests/dust_dd_ref.py; the resident DragHeating through GHIP_DD_MIGRATE into
ghip_sfr_cooling; two rank processes through the drop-in symbols.  fp64 within 1e-12, pair counts exact,
two identical runs bit-identical."""
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

import dust_dd_ref as DR
import dust_ref as R
import sfr_ref as SR
from common import Problem, ShardSet, SinkProblem, bindings, relerr
from test_gpu_dust import DustCase, _scaled_err
from test_gpu_sfr_cooling import _gparams

pytestmark = pytest.mark.gpu
TOL = 1e-12


class DdDust:
    """A DustCase on `nshards` logical shards with the trees of this step (GHIP_DD_GRAVITY, _DENSITY);
    every shard's grain list is its part of the case's list, in the case's order unless `perm` reorders it."""

    def __init__(self, case, nshards, domains=1, perm=False):
        B = bindings()
        pr = case.pr
        self.case, self.B, self.P = case, B, nshards
        S = ShardSet(pr, nshards, fields=dict(hsml=case.hsml), domains=domains)
        self.S = S
        S.set_field(B.F_MASS, case.mass)
        S.set_field(B.F_TIMEBIN, case.timebin)
        S.set_field(B.F_ENTROPY, case.gas_entropy)
        S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
        S.run.density(pr.g_dens())
        S.set_field(B.F_GRAVACCEL, case.grav)          # (gravity wrote its own)
        S.set_field(B.F_HSML, case.hsml)               # the grains' h as the case has them
        where = S.locate(case.dust)
        rng = np.random.default_rng(5)
        self.lists, self.local = [], []
        for loc, pos in where:
            o = rng.permutation(len(pos)) if perm else np.arange(len(pos))
            self.lists.append(pos[o])
            self.local.append(loc[o])
        assert sum(len(x) for x in self.lists) == len(case.dust)

    def density(self):
        B, case = self.B, self.case
        built = [B.dd_dust_args(case.gparams(), self.local[r]) for r in range(self.P)]
        self.S.run.run(B.DD_DUST_DENSITY, [b[0] for b in built])
        d7 = np.zeros(len(case.dust))
        for r, b in enumerate(built):
            d7[self.lists[r]] = b[1]["particle_density"]
        return d7, [b[1]["counts"].copy() for b in built]

    def drag(self, d7):
        B, c = self.B, self.case
        built = []
        for r in range(self.P):
            o = self.lists[r]
            built.append(B.dd_dust_args(c.gparams(), self.local[r], particle_density=d7[o], dust_density=c.rho[o],
                                        dust_entropy=c.ent[o], dust_gasvel=c.gasvel[o], dust_radius=c.radius[o],
                                        particle_velocity=c.d9[o], vcoll=c.vcoll[o]))
        self.S.run.run(B.DD_DUST_DRAG, [b[0] for b in built])
        nd = len(c.dust)
        out = dict(particle_velocity=np.zeros((nd, 3)), delta_momentum=np.zeros((nd, 3)), delta_energy=np.zeros(nd),
                   vcoll=np.zeros(nd))
        for r, b in enumerate(built):
            for k in out:
                out[k][self.lists[r]] = b[1][k]
        return out, [b[1]["counts"].copy() for b in built]

    def heat(self):
        S = self.S
        h = np.zeros(self.case.pr.ngas)
        for r, fp in enumerate(S.fp):
            h[S.gid[r][:S.ngas[r]]] = fp.dust_drag_heating()
        return h

    def ref_gas(self, out, orders=None):
        """the scatter of every shard in the reference's per-rank order (or in the given orders)"""
        c, pr, S = self.case, self.case.pr, self.S
        ng = pr.ngas
        dtg = np.where(c.timebin > 0, (1 << c.timebin).astype(np.float64), 0.0) * c.par["dt_fac_gas"]
        vel, ent, heat = pr.ic["vel"][:ng].copy(), c.gas_entropy.copy(), np.zeros(ng)
        orders = orders or DR.rank_orders(self.lists, self.local)
        i = c.dust
        cnt = DR.shard_scatter(c.par, pr.ic["pos"][i], c.hsml[i], c.rho, out["delta_momentum"], out["delta_energy"],
                               pr.ic["pos"], c.mass, pr.ic["type"], ng, dtg, vel, ent, heat, orders,
                               [S.gid[r][:S.ngas[r]] for r in range(self.P)])
        return vel, ent, heat, cnt


def _check_both_passes(nshards, periodic, domains=1, ndust=600, ng=10):
    case = DustCase(periodic, ndust=ndust, ng=ng)
    pr = case.pr
    n, ngas = pr.n, pr.ngas
    B = bindings()
    T = DdDust(case, nshards, domains=domains)
    S = T.S
    try:
        before = {f: S.get_field(f) for f in (B.F_POS, B.F_MASS, B.F_TYPE, B.F_HSML, B.F_TIMEBIN, B.F_GRAVACCEL,
                                              B.F_DENSITY, B.F_VELPRED)}
        vel0, ent0 = S.get_field(B.F_VEL), S.get_field(B.F_ENTROPY)
        # ---- density ----
        d7, cnt = T.density()
        sent = sum(int(c[0]) for c in cnt)
        assert sent > 0 and sent == sum(int(c[1]) for c in cnt)
        assert all(c[3] > 0 for c in cnt if c[0] > 0)
        ref = case.ref_density()
        assert relerr(d7, ref) < TOL and np.all(ref > 0)
        for f, v in before.items():
            assert np.array_equal(S.get_field(f), v), f
        assert np.array_equal(S.get_field(B.F_VEL), vel0)
        # ---- drag: grains ----
        out, cnt = T.drag(d7)
        assert sum(int(c[0]) for c in cnt) > 0
        rg = case.ref_grains(np.arange(len(case.dust)), d7)
        vel = S.get_field(B.F_VEL)
        assert _scaled_err(vel[case.dust], rg["vel"]) < TOL
        assert _scaled_err(out["delta_momentum"], rg["dmom"]) < TOL
        assert _scaled_err(out["delta_energy"], rg["de"]) < TOL
        assert relerr(out["vcoll"], rg["vcoll"]) < TOL
        assert relerr(out["particle_velocity"], rg["d9"]) < TOL
        # ---- drag: every shard's gas in its own order ----
        gv, ge, gh, counts = T.ref_gas(out)
        for r in range(nshards):
            assert int(cnt[r][2]) == int(counts[r]["touched"].sum()), r      # (gas, grain) pairs exactly
        assert sum(c["caps"] for c in counts) > 0 and sum(c["floors"] for c in counts) > 0
        assert _scaled_err(vel[:ngas], gv) < TOL
        assert relerr(S.get_field(B.F_ENTROPY), ge) < TOL
        heat = T.heat()
        assert _scaled_err(heat, gh) < TOL and np.abs(gh).max() > 0
        touched = np.zeros(ngas, bool)
        for r in range(nshards):
            touched[S.gid[r][:S.ngas[r]]] = counts[r]["touched"] > 0
        assert np.array_equal(vel[:ngas][~touched], vel0[:ngas][~touched])
        assert np.array_equal(S.get_field(B.F_ENTROPY)[~touched], ent0[~touched])
        assert np.all(heat[~touched] == 0)
        other = np.setdiff1d(np.arange(ngas, n), case.dust)
        assert np.array_equal(vel[other], vel0[other])
        for f, v in before.items():
            assert np.array_equal(S.get_field(f), v), f
    finally:
        S.close()


@pytest.mark.parametrize("nshards,periodic,domains", [(2, 1, 1), (3, 0, 1), (8, 1, 1), (8, 0, 1), (3, 1, 4)])
def test_dust_passes_on_shards(nshards, periodic, domains):
    _check_both_passes(nshards, periodic, domains)


def test_dust_passes_on_shards_are_deterministic():
    case = DustCase(1, ndust=400)
    B = bindings()
    res = []
    for _ in range(2):
        T = DdDust(case, 3)
        try:
            d7, _ = T.density()
            out, _ = T.drag(d7)
            res.append((d7, out, T.S.get_field(B.F_VEL), T.S.get_field(B.F_ENTROPY), T.heat()))
        finally:
            T.S.close()
    a, b = res
    assert np.array_equal(a[0], b[0])
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k]), k
    for x, y in zip(a[2:], b[2:]):
        assert np.array_equal(x, y)


def test_gas_receives_grains_in_the_per_rank_order():
    """Shard lists in a permuted order: a gas particle takes this shard's grains in list order, then the
    other shards' by rank and local index.  Under the 1.5 cap and the floor that differs from the global
    list order and from the shards' list order of the imported grains; the device follows the first."""
    case = DustCase(1, ndust=600)
    B = bindings()
    T = DdDust(case, 4, perm=True)
    S = T.S
    try:
        d7, _ = T.density()
        out, _ = T.drag(d7)
        ent = S.get_field(B.F_ENTROPY)
        gv, ge, gh, counts = T.ref_gas(out)
        assert relerr(ent, ge) < TOL and _scaled_err(T.heat(), gh) < TOL
        # the same scatter in the global list order, and with the imported grains in their senders' list order
        glob = [np.arange(len(case.dust))] * T.P
        _, ge_glob, _, _ = T.ref_gas(out, orders=glob)
        lst = [np.concatenate([T.lists[s]] + [T.lists[r] for r in range(T.P) if r != s]) for s in range(T.P)]
        _, ge_lst, _, _ = T.ref_gas(out, orders=lst)
        for other in (ge_glob, ge_lst):
            d = np.abs(other - ge) / np.abs(ge)
            assert d.max() > 1e-6                      # the order shows ...
            assert np.abs(ent - other).max() / np.abs(ge).max() > 1e3 * TOL   # ... and the device follows ge
    finally:
        S.close()


def _drag_on_two_shards(case, own1=True, gas_timebin=None):
    """both passes on two shards (own1 = False: shard 1 lists no grain of its own) -> what the scatter left and, per
    shard, the restatement's pair counts per gas particle of the own and of the imported grains"""
    B = bindings()
    ngas = case.pr.ngas
    T = DdDust(case, 2)
    S = T.S
    try:
        if not own1:
            T.lists[1], T.local[1] = T.lists[1][:0], T.local[1][:0]
        if gas_timebin is not None:
            S.set_field(B.F_TIMEBIN, np.concatenate([np.full(ngas, gas_timebin, case.timebin.dtype), case.timebin[ngas:]]))
        vel0, ent0 = S.get_field(B.F_VEL), S.get_field(B.F_ENTROPY)
        d7, _ = T.density()
        out, cnt = T.drag(d7)
        vel, ent, heat = S.get_field(B.F_VEL), S.get_field(B.F_ENTROPY), T.heat()
        if gas_timebin == 0:
            return cnt, (vel[:ngas], vel0[:ngas]), (ent, ent0), heat
        gv, ge, gh, counts = T.ref_gas(out)
        assert [int(c[2]) for c in cnt] == [int(c["touched"].sum()) for c in counts]      # (gas, grain) pairs exactly
        assert _scaled_err(vel[:ngas], gv) < TOL and relerr(ent, ge) < TOL and _scaled_err(heat, gh) < TOL
        orders, nown = DR.rank_orders(T.lists, T.local), [len(x) for x in T.lists]
        own = T.ref_gas(out, orders=[o[:k] for o, k in zip(orders, nown)])[3]
        imp = T.ref_gas(out, orders=[o[k:] for o, k in zip(orders, nown)])[3]
        return cnt, [c["touched"] for c in own], [c["touched"] for c in imp]
    finally:
        S.close()


def test_scatter_of_imported_grains_alone_of_mixed_runs_and_without_pairs():
    """The three shapes of a shard's scatter, on two shards.  A shard that lists no grain and imports some: its gas
    receives pairs, all of imported grains.  Both shards with lists: gas particles receive own and imported grains in
    one run.  No gas particle on a timestep: no pair anywhere, and the gas stays as it was bit for bit."""
    case = DustCase(1, ndust=600)
    cnt, own, imp = _drag_on_two_shards(case, own1=False)
    assert int(cnt[1][0]) == 0 and int(cnt[1][1]) > 0 and int(cnt[1][2]) > 0
    assert own[1].sum() == 0 and imp[1].sum() == int(cnt[1][2])
    cnt, own, imp = _drag_on_two_shards(case)
    assert all(np.count_nonzero((o > 0) & (i > 0)) > 0 for o, i in zip(own, imp))
    cnt, vel, ent, heat = _drag_on_two_shards(case, gas_timebin=0)
    assert all(int(c[2]) == 0 for c in cnt) and sum(int(c[1]) for c in cnt) > 0
    assert np.array_equal(*vel) and np.array_equal(*ent) and np.all(heat == 0)


def test_dust_operations_refuse_without_the_trees_of_the_step():
    case = DustCase(1, ndust=100, ng=8)
    pr = case.pr
    B = bindings()
    S = ShardSet(pr, 2, fields=dict(hsml=case.hsml))
    try:
        where = S.locate(case.dust)
        with pytest.raises(B.GhipError) as e:
            S.run.run(B.DD_DUST_DENSITY, [B.dd_dust_args(case.gparams(), where[r][0])[0] for r in range(2)])
        assert e.value.code == -90002 and "GHIP_DD_GRAVITY" in str(e.value)
        S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
        keep = [B.dd_dust_args(case.gparams(), where[r][0], particle_density=np.ones(len(where[r][0])),
                               dust_density=np.ones(len(where[r][0])), dust_entropy=np.ones(len(where[r][0])),
                               dust_radius=np.ones(len(where[r][0])))
                for r in range(2)]
        with pytest.raises(B.GhipError) as e:
            S.run.run(B.DD_DUST_DRAG, [k[0] for k in keep])
        assert e.value.code == -90002 and "GHIP_DD_DENSITY" in str(e.value)
    finally:
        S.close()


def test_drag_heating_follows_migration_into_sfr_cooling():
    """After the drag pass the gas drifts across the splits and migrates: DragHeating follows each gas
    particle (by global id), and ghip_sfr_cooling(dust = 1) on every shard equals one single-GPU call on
    the same state bit for bit (DtEntropy, DragHeating spent, candidates)."""
    case = DustCase(1, ndust=600)
    pr = case.pr
    n, ngas = pr.n, pr.ngas
    B = bindings()
    T = DdDust(case, 3)
    S = T.S
    try:
        d7, _ = T.density()
        T.drag(d7)
        heat = T.heat()
        assert np.count_nonzero(heat) > 10
        rng = np.random.default_rng(4)
        density = 0.2 + 3.0 * rng.random(ngas)
        S.set_field(B.F_DENSITY, density)
        S.set_field(B.F_DTENTROPY, pr.dtentropy)
        # drift across the splits (periodic wrap), then domain_exchange
        pos = (S.get_field(B.F_POS) + np.array([0.13, -0.07, 0.05]) * pr.box) % pr.box
        S.set_field(B.F_POS, pos)
        S.migrate()
        moved = sum(fp.dd_info()["migrated_out"] for fp in S.fp)
        assert moved > 50
        assert np.array_equal(T.heat(), heat)
        state = {f: S.get_field(f) for f in (B.F_POS, B.F_MASS, B.F_TYPE, B.F_TIMEBIN, B.F_DENSITY, B.F_ENTROPY,
                                             B.F_DTENTROPY)}
        p = SR.params(dust=1, Timebase_interval=pr.timebase, CritPhysDensity_code=2.8,
                      OriginalGasMass=float(pr.ic["mass"][0]), smbh_pos=(0.45 * pr.box, 0.5 * pr.box, 0.5 * pr.box))
        cand = []
        for r, fp in enumerate(S.fp):
            fp.set_active(None)
            cand.append(S.gid[r][fp.sfr_cooling(_gparams(p))])
        got_dA, got_heat = S.get_field(B.F_DTENTROPY), T.heat()
        # one GPU, the same state
        fp = B.ForcePath(0)
        fp.set_counts(n, ngas)
        for f, v in state.items():
            fp.set_field(f, v)
        fp.set_dust_drag_heating(heat)
        fp.set_active(None)
        c1 = fp.sfr_cooling(_gparams(p))
        try:
            assert np.array_equal(got_dA, fp.get_field(B.F_DTENTROPY))
            assert np.array_equal(got_heat, fp.dust_drag_heating())
            assert np.array_equal(np.sort(np.concatenate(cand)), np.sort(c1))
            assert not np.array_equal(got_dA, state[B.F_DTENTROPY])
        finally:
            fp.close()
    finally:
        S.close()


def test_dust_passes_on_8_shards_at_c2_size_with_timings():
    """64^3 gas plus 65 536 grains as 8 logical shards: parity on a sample of grains and gas, the wall time of
    both passes per shard (ghip_dd_step phases of one shard run back to back on one GPU), grains exported
    and bytes sent per shard"""
    ng = 64
    pr = Problem(ng=ng, gas=True, periodic=1)
    n, ngas = pr.n, pr.ngas
    ndust = (n - ngas) // 4
    sp = SinkProblem.__new__(SinkProblem)
    rng = np.random.default_rng(9)
    sp.pr = pr
    sp.dust = np.sort(rng.choice(np.arange(ngas, n), ndust, replace=False))
    typ = pr.ic["type"].copy()
    typ[sp.dust] = 2
    pr.ic["type"] = typ
    sp.hsml = pr.hsml0.copy()
    sp.ids = np.arange(n, dtype=np.uint32)
    case = DustCase(1, sp=sp, seed=9)
    B = bindings()
    T = DdDust(case, 8)
    S = T.S
    try:
        # warm-up (allocations), then the timed passes phase by phase
        d7, _ = T.density()
        t_dens = np.zeros(8)
        t_drag = np.zeros(8)

        def timed(op, args):
            for fp, a in zip(S.fp, args):
                fp.dd_begin(op, a)
            while True:
                rcs = []
                for r, fp in enumerate(S.fp):
                    t0 = time.perf_counter()
                    rcs.append(fp.dd_step())
                    dt = time.perf_counter() - t0
                    (t_dens if op == B.DD_DUST_DENSITY else t_drag)[r] += dt
                if rcs[0] == 0:
                    return
                B.dd_exchange_local(S.fp)

        built = [B.dd_dust_args(case.gparams(), T.local[r]) for r in range(8)]
        timed(B.DD_DUST_DENSITY, [b[0] for b in built])
        d7b = np.zeros(ndust)
        for r, b in enumerate(built):
            d7b[T.lists[r]] = b[1]["particle_density"]
        assert np.array_equal(d7, d7b)
        cnt_d = [b[1]["counts"].copy() for b in built]
        c = case
        built = []
        for r in range(8):
            o = T.lists[r]
            built.append(B.dd_dust_args(c.gparams(), T.local[r], particle_density=d7[o], dust_density=c.rho[o],
                                        dust_entropy=c.ent[o], dust_gasvel=c.gasvel[o], dust_radius=c.radius[o],
                                        particle_velocity=c.d9[o], vcoll=c.vcoll[o]))
        timed(B.DD_DUST_DRAG, [b[0] for b in built])
        cnt_g = [b[1]["counts"].copy() for b in built]
        out = dict(delta_momentum=np.zeros((ndust, 3)), delta_energy=np.zeros(ndust))
        for r, b in enumerate(built):
            for k in out:
                out[k][T.lists[r]] = b[1][k]
        # parity on a sample
        samp = np.sort(rng.choice(ndust, 2048, replace=False))
        assert relerr(d7[samp], case.ref_density(case.dust[samp])) < TOL
        rg = case.ref_grains(samp, d7[samp])
        assert _scaled_err(out["delta_energy"][samp], rg["de"]) < TOL
        assert _scaled_err(out["delta_momentum"][samp], rg["dmom"]) < TOL
        gsamp = np.sort(rng.choice(ngas, 512, replace=False))
        owner = np.full(ngas, -1)
        for r in range(8):
            owner[S.gid[r][:S.ngas[r]]] = r
        orders = DR.rank_orders(T.lists, T.local)
        dtg = np.where(c.timebin > 0, (1 << c.timebin).astype(np.float64), 0.0) * c.par["dt_fac_gas"]
        vel, ent, heat = pr.ic["vel"][:ngas].copy(), c.gas_entropy.copy(), np.zeros(ngas)
        i = c.dust
        DR.shard_scatter(c.par, pr.ic["pos"][i], c.hsml[i], c.rho, out["delta_momentum"], out["delta_energy"],
                         pr.ic["pos"], c.mass, pr.ic["type"], ngas, dtg, vel, ent, heat, orders,
                         [gsamp[owner[gsamp] == r] for r in range(8)])
        assert relerr(S.get_field(B.F_ENTROPY)[gsamp], ent[gsamp]) < TOL
        assert _scaled_err(S.get_field(B.F_VEL)[gsamp], vel[gsamp]) < TOL
        assert _scaled_err(T.heat()[gsamp], heat[gsamp]) < TOL
        rec = dict(ms_density=[round(1e3 * v, 3) for v in t_dens], ms_drag=[round(1e3 * v, 3) for v in t_drag],
                   exported_density=[int(x[0]) for x in cnt_d], imported_density=[int(x[1]) for x in cnt_d],
                   bytes_density=[int(x[3]) for x in cnt_d], exported_drag=[int(x[0]) for x in cnt_g],
                   bytes_drag=[int(x[3]) for x in cnt_g], pairs=[int(x[2]) for x in cnt_g],
                   grains=[len(x) for x in T.lists], gas=list(map(int, S.ngas)))
        print("\nDUST_DD_C2 " + json.dumps(rec))
        assert sum(rec["exported_density"]) > 0
    finally:
        S.close()


def test_dropin_dust_passes_on_two_ranks():
    """density(), dust_density() and dust_drag() with NTask = 2: one process per rank, both on this box's
    one GPU, 536 / 264-byte records, exchanges through the host's all-gather (gloo).
    tests/gpu_host_ranks_dust.py is the rank program; rank 0 gathers the records and checks them against
    the per-rank-order restatement."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "tests", "gpu_host_ranks_dust.py")]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["ok"], out
    assert out["exported"] > 0
    for k in ("rel_d7", "rel_grain_vel", "rel_dmom", "rel_de", "rel_vcoll", "rel_d9", "rel_gas_vel", "rel_entropy",
              "rel_heat"):
        assert out[k] < TOL, (k, out[k])
    assert out["untouched_equal"]
