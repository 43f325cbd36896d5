"""GHIP_DD_POTENTIAL and GHIP_DD_GLOBAL_QUANTITIES: compute_potential() (potential.c:22-325) and the sums of
compute_global_quantities_of_system() (global.c:18-238) on domain-decomposed shards, several logical shards
on one GPU (ShardSet).  The yardstick is the numpy restatement in tests/potential_ref.py on the exported
tree of a SINGLE-context build of the same particles -- the reference's potential does not depend on the
number of ranks -- so the interaction count of every particle must be exact and the sums agree to the
order in which the moments of cells that span shards are added (TOL of tests/test_gpu_dd.py).  The
single-context ghip_potential is a second comparison."""
import json
import threading
import time

import numpy as np
import pytest

from common import Problem, ShardSet, bindings, ics
import potential_ref as R
import test_gpu_potential as TP

pytestmark = pytest.mark.gpu
B = bindings()
TOL = 1e-11        # the shard tolerance (tests/test_gpu_dd.py)
TOL_MESH = 1e-10   # the mesh tolerance (tests/test_gpu_potential.py)
_REF = {}


def _reference(name):
    """the variant's problem, OldAcc of a first force walk, the reference walk of every particle with its
    interaction counts, and the single-context device potential"""
    if name not in _REF:
        v = TP.VARIANTS[name]
        # (the Barnes-Hut cases are larger: their imports must stay below the other shards' particle total)
        pr = Problem(ng=16 if v["theta"] else 12, periodic=v["periodic"], unequal=v.get("unequal", False))
        adaptive, pmgrid = v.get("adaptive", False), v.get("pmgrid", 0)
        fp, old = TP._device(pr, adaptive)
        fp.potential(TP._pot_params(pr, v["theta"], pmgrid=pmgrid))
        single = fp.get_potential()
        w, nint = TP._ref_walk(fp, pr, v["theta"], old, np.arange(pr.n), adaptive, pmgrid)
        fp.close()
        ic = pr.ic
        pm = dict(pmgrid=pmgrid, box=pr.box, asmth=1.25 * pr.box / pmgrid) if pmgrid else None
        ref = R.finish(w, ic["pos"], ic["mass"], ic["type"], pr.force_soft / 2.8, 1.0, pm=pm)
        _REF[name] = (pr, old, ref, nint, single)
    return _REF[name]


def _shards(pr, nshards, old, adaptive=False, domains=1):
    S = ShardSet(pr, nshards, fields={"oldacc": old}, domains=domains)
    if adaptive:
        S.each(lambda fp: fp.set_adaptive_gravsoft(True))
    return S


def _gather(S, fn, dtype=np.float64):
    out = np.zeros(S.pr.n, dtype)
    for r, fp in enumerate(S.fp):
        if len(S.gid[r]):
            out[S.gid[r]] = fn(fp)
    return out


def _check_walk(name, S, params):
    pr, old, ref, nint, single = _reference(name)
    v = TP.VARIANTS[name]
    S.run.potential(params)
    dev = _gather(S, lambda fp: fp.get_potential())
    cnt = _gather(S, lambda fp: fp.get_potential_interactions(), np.int64)
    info = S.each(lambda fp: fp.dd_info())
    tol = TOL_MESH if v.get("pmgrid", 0) else TOL
    e_ref, e_single = TP._err(dev, ref), TP._err(dev, single)
    print("%s on %d shards: err vs reference %.3e, vs one context %.3e, imports %r" %
          (name, S.P, e_ref, e_single, [i["let_imported"] for i in info]))
    assert np.array_equal(cnt, nint), "interaction counts differ from the single tree"
    assert e_ref < tol and e_single < tol
    # the test proves something: elements crossed the links ...
    assert all(i["let_imported"] > 0 for i in info)
    if v["theta"] == 0.5:
        # ... and not every remote particle came as a particle: pruned nodes were walked
        for r, i in enumerate(info):
            assert i["let_imported"] < pr.n - len(S.gid[r]), (r, i["let_imported"])
    return dev


@pytest.mark.parametrize("nshards", [2, 3, 8])
@pytest.mark.parametrize("name", list(TP.VARIANTS))
def test_walk_parity_on_shards(name, nshards):
    pr, old, _, _, _ = _reference(name)
    v = TP.VARIANTS[name]
    S = _shards(pr, nshards, old, v.get("adaptive", False))
    try:
        _check_walk(name, S, TP._pot_params(pr, v["theta"], pmgrid=v.get("pmgrid", 0)))
    finally:
        S.close()


def test_walk_parity_on_shards_that_own_several_pieces_of_the_curve():
    name = "ewald_rel"
    pr, old, _, _, _ = _reference(name)
    S = _shards(pr, 3, old, domains=4)
    try:
        _check_walk(name, S, TP._pot_params(pr, 0.0))
    finally:
        S.close()


def test_every_particle_is_a_target_whatever_the_active_list():
    """About 10 % of the particles are active and the step's GHIP_DD_GRAVITY has selected its locally
    essential trees for them: the potential of EVERY particle still matches (it would not if that
    selection were reused)."""
    name = "newton_rel"
    pr, old, _, _, _ = _reference(name)
    rng = np.random.default_rng(4)
    S = _shards(pr, 3, old)
    try:
        for r, fp in enumerate(S.fp):
            nl = len(S.gid[r])
            fp.set_active(np.sort(rng.choice(nl, max(1, nl // 10), replace=False)))
        S.run.gravity(pr.g_grav(0.0), B.WALK_NEWTON)
        _check_walk(name, S, TP._pot_params(pr, 0.0))
    finally:
        S.close()


def test_walk_parity_c2_on_eight_shards():
    """c2 size (2 x 64^3 particles) on 8 logical shards, periodic with the Ewald potential and the same
    positions without periodicity: 2048 sampled targets against the reference walk, counts exact.  Prints
    what crossed the links and the time of every phase per shard."""
    ic = ics.make_ics(64, gas=True)
    rng = np.random.default_rng(9)
    for periodic in (1, 0):
        pr = Problem(ic=ic, periodic=periodic)
        fp, old = TP._device(pr)
        tg = np.sort(rng.choice(pr.n, 2048, replace=False))
        w, nint = TP._ref_walk(fp, pr, 0.0, old, tg)
        fp.close()
        ref = R.finish(w, ic["pos"][tg], ic["mass"][tg], ic["type"][tg], pr.force_soft / 2.8, 1.0)
        S = _shards(pr, 8, old)
        try:
            params = TP._pot_params(pr, 0.0)
            S.run.potential(params)          # warm-up (allocations)
            ms = [[] for _ in S.fp]
            for f in S.fp:
                f.dd_begin(B.DD_POTENTIAL, params)
            while True:
                rcs = []
                for r, f in enumerate(S.fp):
                    f.sync()
                    t0 = time.perf_counter()
                    rcs.append(f.dd_step())
                    f.sync()
                    ms[r].append(round(1e3 * (time.perf_counter() - t0), 3))
                if rcs[0] == 0:
                    break
                B.dd_exchange_local(S.fp)
            dev = _gather(S, lambda f: f.get_potential())
            cnt = _gather(S, lambda f: f.get_potential_interactions(), np.int64)
            info = S.each(lambda f: f.dd_info())
            err = TP._err(dev[tg], ref)
            rec = dict(periodic=periodic, particles=[len(g) for g in S.gid],
                       imported=[i["let_imported"] for i in info], sent=[i["let_sent"] for i in info],
                       bytes_sent=S.each(lambda f: f.dd_bytes_sent(B.DD_POTENTIAL)),
                       merged_elements=[i["grav_elements"] for i in info], ms_phases=ms, err=err)
            print("\nPOTENTIAL_DD_C2 " + json.dumps(rec))
            assert len(np.unique(S.owner[tg])) == 8
            assert np.array_equal(cnt[tg], nint)
            assert err < TOL, periodic
            assert all(0 < i["let_imported"] < pr.n - len(g) for i, g in zip(info, S.gid))
        finally:
            S.close()


@pytest.mark.parametrize("case", ["pm16_comoving", "comoving_open", "lambda", "pm16"])
def test_finish_and_mesh_on_shards(case):
    periodic = case.startswith("pm")
    pmgrid = 16 if periodic else 0
    comoving = case in ("pm16_comoving", "comoving_open")
    pr = Problem(ng=8, periodic=int(periodic))
    fp, old = TP._device(pr)
    w, nint = TP._ref_walk(fp, pr, 0.0, old, np.arange(pr.n), pmgrid=pmgrid)
    fp.close()
    cosmo = dict(Omega0=0.3, OmegaLambda=0.7, Hubble=0.8)
    G = 0.7
    ic = pr.ic
    pm = dict(pmgrid=pmgrid, box=pr.box, asmth=1.25 * pr.box / pmgrid) if pmgrid else None
    ref = R.finish(w, ic["pos"], ic["mass"], ic["type"], pr.force_soft / 2.8, G, comoving=comoving,
                   periodic=periodic, pm=pm, **cosmo)
    bare = R.finish(w, ic["pos"], ic["mass"], ic["type"], pr.force_soft / 2.8, G)
    S = _shards(pr, 3, old)
    try:
        S.run.potential(TP._pot_params(pr, 0.0, G=G, pmgrid=pmgrid, comoving=comoving, **cosmo))
        dev = _gather(S, lambda f: f.get_potential())
        cnt = _gather(S, lambda f: f.get_potential_interactions(), np.int64)
        err = TP._err(dev, ref)
        print("%s on 3 shards: err %.3e" % (case, err))
        assert np.array_equal(cnt, nint)
        assert err < (TOL_MESH if pmgrid else TOL), case
        assert TP._err(dev, bare) > 1e-6      # every term matters
    finally:
        S.close()


def _gq_shards(pr, s, nshards):
    """shards holding the state s of tests/test_gpu_potential.py::_gq_state"""
    S = ShardSet(pr, nshards)
    for f, k in ((B.F_POS, "pos"), (B.F_VEL, "vel"), (B.F_MASS, "mass"), (B.F_TYPE, "ptype"),
                 (B.F_TIMEBIN, "timebin"), (B.F_TI_BEGSTEP, "ti_begstep"), (B.F_GRAVACCEL, "gravaccel"),
                 (B.F_HYDROACCEL, "hydroaccel"), (B.F_ENTROPY, "entropy"), (B.F_DTENTROPY, "dtentropy"),
                 (B.F_DENSITY, "density")):
        S.set_field(f, s[k])
    return S


@pytest.mark.parametrize("nshards", [3, 8])
@pytest.mark.parametrize("comoving", [0, 1])
def test_global_quantities_on_shards(comoving, nshards):
    pr = Problem(ng=8, periodic=1)
    ng = pr.ngas
    s = TP._gq_state(pr)
    rng = np.random.default_rng(3)
    gk = np.cumsum(0.01 + rng.random(1000) * 1e-3)
    hk = np.cumsum(0.02 + rng.random(1000) * 1e-3)
    tabs = dict(grav_kick_table=gk, hydro_kick_table=hk) if comoving else {}
    S = _gq_shards(pr, s, nshards)
    try:
        S.run.potential(TP._pot_params(pr, 0.5))
        pot = _gather(S, lambda f: f.get_potential())
        p = TP._gq_params(comoving)

        def run():
            built = [B.dd_global_args(p, len(S.gid[r]), old_photon_momentum=s["photon"][S.gid[r]], **tabs)
                     for r in range(nshards)]
            S.run.run(B.DD_GLOBAL_QUANTITIES, [b[0] for b in built])
            return [bytes(b[1]["out"]) for b in built], built[0][1]["out"].asdict()

        raw, dev = run()
        assert all(r == raw[0] for r in raw), "the shards hold different bytes"
        raw2, _ = run()
        assert raw2 == raw, "a second call gives other bytes"
        ref, scale = R.global_quantities(
            s["pos"], s["vel"], s["mass"], s["ptype"], s["timebin"], s["ti_begstep"], s["gravaccel"],
            p.Ti_Current, p.Timebase_interval, pot=pot, ngas=ng, hydroaccel=s["hydroaccel"],
            entropy=s["entropy"], dtentropy=s["dtentropy"], density=s["density"], comoving=comoving,
            time=p.Time, tables=(p.logTimeBegin, p.logTimeMax, gk, hk), photon=s["photon"], rad_fac=3.0)
        d = R.max_rel_diff(dev, ref, scale)
        print("global quantities on %d shards, comoving %d: %.3e" % (nshards, comoving, d))
        assert d < TP.TOL
        assert dev["EnergyRadComp"] > 0 and np.all(dev["EnergyPotComp"][ref["MassComp"] > 0] != 0)
        # the potential is the shards' own: without it the potential energy is another one
        zero, _ = R.global_quantities(
            s["pos"], s["vel"], s["mass"], s["ptype"], s["timebin"], s["ti_begstep"], s["gravaccel"],
            p.Ti_Current, p.Timebase_interval, pot=np.zeros(pr.n), ngas=ng, hydroaccel=s["hydroaccel"],
            entropy=s["entropy"], dtentropy=s["dtentropy"], density=s["density"], comoving=comoving,
            time=p.Time, tables=(p.logTimeBegin, p.logTimeMax, gk, hk), photon=s["photon"], rad_fac=3.0)
        assert np.all(zero["EnergyPotComp"] == 0)
        # the sharded-module form gives the same numbers
        again = S.run.global_quantities(p, tabs, [dict(old_photon_momentum=s["photon"][g]) for g in S.gid])
        for k in dev:
            assert all(np.array_equal(np.asarray(a[k]), np.asarray(dev[k])) for a in again), k
    finally:
        S.close()


def test_two_runs_give_identical_bytes():
    name = "ewald_rel"
    pr, old, _, _, _ = _reference(name)
    S = _shards(pr, 3, old)
    try:
        out = []
        for _ in range(2):
            S.run.potential(TP._pot_params(pr, 0.0))
            out.append((_gather(S, lambda f: f.get_potential()).tobytes(),
                        _gather(S, lambda f: f.get_potential_interactions(), np.int64).tobytes()))
        assert out[0] == out[1]
    finally:
        S.close()


def test_refusals_come_before_anything_runs():
    """Every argument is checked by ghip_dd_begin, before anything is launched or posted: an odd mesh, a mesh
    box that is not the walk's, a softening of zero, no parameters, no domain -- GHIP_EINVAL and the
    resident fields as they were.  Then the states in which results and trees stop being handed out."""
    pr, old, _, _, _ = _reference("ewald_rel")
    S = _shards(pr, 3, old)
    fields = (B.F_POS, B.F_VEL, B.F_MASS, B.F_OLDACC, B.F_HSML)
    try:
        before = [S.get_field(f) for f in fields]
        bad = []
        p = TP._pot_params(pr, 0.0, pmgrid=16)
        p.pm.pmgrid = 15                                   # odd mesh
        bad.append(p)
        p = TP._pot_params(pr, 0.0, pmgrid=16)
        p.pm.BoxSize = 2.0 * pr.box                        # another box than the walk's
        bad.append(p)
        p = TP._pot_params(pr, 0.0)
        p.SofteningTable[3] = 0.0
        bad.append(p)
        for p in bad:
            for fp in S.fp:
                with pytest.raises(B.GhipError) as e:
                    fp.dd_begin(B.DD_POTENTIAL, p)
                assert B.GHIP_ERRORS[e.value.code] == "GHIP_EINVAL"
        for f, b in zip(fields, before):
            assert np.array_equal(S.get_field(f), b)
        # (a field the walk reads cannot be missing on a context with particles: ghip_set_counts allocates
        # every resident field, zeroed.  The rule is ghip_potential's and shares its code; what the C-ABI
        # can reach of it is the operation without parameters and the shard without a domain)
        with pytest.raises(B.GhipError) as e:
            S.fp[0].dd_begin(B.DD_POTENTIAL, None)
        assert B.GHIP_ERRORS[e.value.code] == "GHIP_EINVAL"
        lone = B.ForcePath(0)
        lone.set_counts(64, 0)
        lone.set_field(B.F_POS, pr.ic["pos"][:64])
        lone.dd_init(0, 1)
        with pytest.raises(B.GhipError) as e:
            lone.dd_begin(B.DD_POTENTIAL, TP._pot_params(pr, 0.0))
        assert B.GHIP_ERRORS[e.value.code] == "GHIP_EINVAL"
        lone.close()
        # the one-context entry points stay refused on a shard and name the operation
        with pytest.raises(B.GhipError) as e:
            S.fp[0].potential(TP._pot_params(pr, 0.0))
        assert B.GHIP_ERRORS[e.value.code] == "GHIP_EINVAL" and "GHIP_DD_POTENTIAL" in str(e.value)
        with pytest.raises(B.GhipError):
            S.fp[0].get_potential()                        # nothing computed yet
        # the tree the potential leaves behind is not the step's gravity tree
        S.run.potential(TP._pot_params(pr, 0.0))
        for fp in S.fp:
            with pytest.raises(B.GhipError) as e:
                fp.dd_begin(B.DD_DENSITY, pr.g_dens())
            assert B.GHIP_ERRORS[e.value.code] == "GHIP_EINVAL"
        S.run.gravity(pr.g_grav(0.0), B.WALK_NEWTON)
        S.run.density(pr.g_dens())                         # works again after the next gravity call
        assert S.fp[0].get_potential().shape == (len(S.gid[0]),)
        # the result belongs to the particle set before a migration
        S.migrate()
        for fp in S.fp:
            with pytest.raises(B.GhipError) as e:
                fp.get_potential()
            assert B.GHIP_ERRORS[e.value.code] == "GHIP_EINVAL"
    finally:
        S.close()


def test_host_staged_transport_gives_the_same_bytes():
    """One case of the walk parity driven through ghip_dd_exchange_host: every shard in a thread of its own,
    the caller's all-gather a rendezvous of the threads."""
    name = "ewald_rel"
    pr, old, _, _, _ = _reference(name)
    nshards = 3
    S = _shards(pr, nshards, old)
    try:
        params = TP._pot_params(pr, 0.0)
        dev_local = _check_walk(name, S, params)
        cnt_local = _gather(S, lambda f: f.get_potential_interactions(), np.int64)
        bar = threading.Barrier(nshards, timeout=120)
        slots = [None] * nshards
        errors = []

        def worker(r):
            def allgather(data):
                slots[r] = data
                bar.wait()
                out = b"".join(slots)
                bar.wait()
                return out
            try:
                S.fp[r].dd_run_host(B.DD_POTENTIAL, params, allgather)
            except Exception as e:   # noqa: BLE001 -- reported by the main thread
                errors.append((r, repr(e)))
                bar.abort()

        threads = [threading.Thread(target=worker, args=(r,)) for r in range(nshards)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        dev = _gather(S, lambda f: f.get_potential())
        cnt = _gather(S, lambda f: f.get_potential_interactions(), np.int64)
        assert dev.tobytes() == dev_local.tobytes() and np.array_equal(cnt, cnt_local)
        assert all(f.dd_bytes_sent(B.DD_POTENTIAL) > 0 for f in S.fp)
    finally:
        S.close()
