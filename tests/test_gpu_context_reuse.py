"""One context through changing problems, as the product drives it (host/gadget_force.c binds one context for
the whole run): the sequences of tests/reuse_cases.py, each run through ONE context, stage after stage.

Every stage is held (a) to the oracle, with the assertions and bounds of tests/gpu_fuzz.py and of the existing
test of each pass -- node count, GRAVCOST, h-iteration count and pair count exactly, gravity and hydro to 1e-10
of the largest value, density and hsml to 1e-11, the mesh force to 1e-11, the potential as
tests/test_gpu_potential.py -- and (b) to a fresh context that runs this stage alone: every integer equal, every
floating-point result equal to the bit except the two sums whose order DESIGN documents as depending on history
(gravity accelerations, 4.2: the wavefronts per bucket follow the plan history; the mesh force, 4.8: fp64
atomics), which are held to their bound of (a).  What a stage leaves behind that the next one reads shows in
(b); what it corrupts shows in (a).

After a sequence the context synchronises without an error (ghip_sync reads the device's error words) and its
memory goes back when it is closed."""
import gc
import time

import numpy as np
import pytest

import reuse_cases as RC
from common import O, Problem, ShardSet, bindings, relerr

pytestmark = pytest.mark.gpu
B = bindings()
# results of a reused context that may differ from a fresh one's by summation order (see above)
ORDER_DEPENDENT = ("acc", "gravpm", "potmesh")


def _in_use():
    return int(B.lib().ghip_device_bytes_in_use())


def _check_potential(fp, st, p, pot, old):
    """tests/test_gpu_potential.py:test_walk_parity_all_targets on the tree this context built"""
    import potential_ref as R
    import test_gpu_potential as TP
    pr = st.pr
    theta, pmgrid = p[1], p[2]
    adaptive = bool(st.switches["adaptive"])
    w, nint = TP._ref_walk(fp, pr, theta, old, np.arange(pr.n), adaptive, pmgrid)
    ic = pr.ic
    pm = dict(pmgrid=pmgrid, box=pr.box, asmth=1.25 * pr.box / pmgrid) if pmgrid else None
    ref = R.finish(w, ic["pos"], ic["mass"], ic["type"], pr.force_soft / 2.8, 1.0, pm=pm)
    err = TP._err(pot, ref)
    print("      potential (theta %g, mesh %d): %.3e" % (theta, pmgrid, err))
    assert err < (1e-10 if pmgrid else TP.TOL), "%s: potential %.3e" % (st.name, err)
    assert fp.potential_interactions() == (int(nint.sum()), int(nint.max())), st.name


def _bits(a, b):
    """largest difference of two results in units of the largest value"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


@pytest.mark.parametrize("name", list(RC.SEQUENCES))
def test_one_context_through_a_sequence_of_problems(name):
    seq = RC.SEQUENCES[name]
    gc.collect()                                 # (contexts earlier tests dropped without closing)
    base = _in_use()
    failures = []
    fp = B.ForcePath(0)
    have = dict(RC.DEFAULTS)
    t_all = time.time()
    print()
    try:
        for st in seq:
            t0 = time.time()
            got, have = RC.device_stage(fp, st, have, on_potential=_check_potential)
            want = RC.oracle_stage(st)
            fresh = RC.fresh_stage(st)
            assert set(got) == set(fresh)
            a = RC.compare(got, want, 0)
            b = RC.compare(got, fresh, 1)
            # which results were not equal to the bit, and by how much of their largest value
            inexact = {k: _bits(got[k], fresh[k]) for k in got
                       if np.asarray(got[k]).shape == np.asarray(fresh[k]).shape and
                       not np.array_equal(got[k], fresh[k])}
            print("  %-30s n %4d gas %4d  %.2f s  not bit-equal to a fresh context: %s" % (
                st.name, st.pr.n, st.pr.ngas, time.time() - t0,
                ", ".join("%s %.1e" % kv for kv in sorted(inexact.items())) or "nothing"))
            for k in inexact:
                if not k.startswith(ORDER_DEPENDENT) and k not in b:
                    b[k] = "differs by %.3e" % inexact[k]
            failures += ["%s / oracle / %s: %s" % (st.name, k, v) for k, v in a.items()]
            failures += ["%s / fresh context / %s: %s" % (st.name, k, v) for k, v in b.items()]
        fp.sync()                                # raises on a set error word
    finally:
        fp.close()
    print("  %s: %.1f s" % (name, time.time() - t_all))
    assert _in_use() == base, "the closed context kept device memory"
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------
# three logical shards, reloaded
# ------------------------------------------------------------------------------------------------
def _shard_problem(which):
    if which == "A":
        return Problem(ic=RC.cosmo(8), periodic=1), None
    if which == "B":
        return Problem(ic=RC.plummer(2600, seed=11, a=0.03, gas_fraction=0.45, center=(0.4, 0.55, 0.5)), periodic=0,
                       unequal=True), None
    # C: 60 collisionless particles, 59 of them in one cell of the histogram the cut is made on and one far
    # away -- two occupied cells for three shards: one shard is left with nobody
    ic = RC.noise(60, 0, 31)
    ic["pos"][:59] = 0.2 + 1e-2 * ic["pos"][:59]
    ic["pos"][59] = 0.9
    return Problem(ic=ic, periodic=0, soft_frac=0.0004), None


def _shard_step(S, pr, old, shake):
    """gravity, density and hydro where there is gas, a shake with a migration and gravity again: against the
    oracle's single tree, as tests/gpu_ddfuzz.py:one does and with its bounds"""
    n, ng = pr.n, pr.ngas
    tg = np.arange(n, dtype=np.int32)
    theta = 0.5
    T = pr.oracle_tree()
    S.run.gravity(pr.g_grav(theta), B.WALK_NEWTON_EWALD if pr.periodic else B.WALK_NEWTON)
    oacc, ocost = T.gravity(pr.o_grav(theta), tg, old)
    if pr.periodic:
        T.gravity_ewald_add(pr.o_grav(theta), O.ewald_table(pr.box), tg, old, oacc, ocost)
    assert np.array_equal(S.get_field(B.F_GRAVCOST), ocost), "gravity counts"
    assert np.abs(S.get_field(B.F_GRAVACCEL) - oacc).max() < 1e-10 * (np.abs(oacc).max() + 1e-300), "gravity"
    if ng >= 40:
        act = np.arange(ng, dtype=np.int32)
        S.run.density(pr.g_dens())
        od = T.density(pr.o_dens(), act, pr.velpred, pr.entropy, pr.dtentropy, pr.timebin, pr.ti_begstep, pr.hsml0)
        assert relerr(S.get_field(B.F_HSML)[act], od["hsml"][act]) < 1e-9, "hsml"
        assert relerr(S.get_field(B.F_DENSITY)[act], od["density"][act]) < 1e-9, "density"
        assert sum(s["dens_neighbours"] for s in S.each(lambda fp: fp.stats())) == od["ngb_visits"]
        S.each(lambda fp: fp.update_hmax())
        T.update_hmax(act, od["hsml"], od["divvel"])
        S.run.hydro(pr.g_hydro())
        oh = T.hydro(pr.o_hydro(), act, pr.velpred, od["hsml"], od["density"], od["pressure"], od["dhsmlfac"],
                     od["divvel"], od["curlvel"], pr.timebin)
        assert sum(s["hydro_pairs"] for s in S.each(lambda fp: fp.stats())) == oh["npairs"], "pairs"
        want = oh["hydroaccel"][act]
        assert np.abs(S.get_field(B.F_HYDROACCEL)[act] - want).max() <= 1e-9 * (np.abs(want).max() + 1e-300), "hydro"
        assert relerr(S.get_field(B.F_MAXSIGNALVEL)[act], oh["maxsignalvel"][act]) < 1e-9, "MaxSignalVel"
    if shake:
        rng = np.random.default_rng(77)
        lo, ln = pr.extent[0], pr.extent[2]
        newpos = pr.ic["pos"] + 0.05 * ln * rng.standard_normal((n, 3))
        if pr.periodic:
            newpos = np.mod(newpos, pr.box)
            newpos[newpos >= pr.box] = 0.0
        newpos = np.clip(newpos, lo + 1e-9 * ln, lo + ln * (1 - 1e-9))
        S.set_field(B.F_POS, newpos)
        before = S.owner.copy()
        S.migrate()
        assert int((S.owner != before).sum()) > 0
        assert np.array_equal(np.sort(np.concatenate(S.gid)), np.arange(n)), "lost or doubled"
        assert np.array_equal(S.get_field(B.F_POS), newpos), "positions after migration"
        moved = Problem(ic=dict(pr.ic, pos=newpos), periodic=pr.periodic, unequal=bool(pr.unequal))
        moved.extent = pr.extent
        T2 = moved.oracle_tree()
        S.set_field(B.F_OLDACC, old)
        o2, c2 = T2.gravity(pr.o_grav(theta), tg, old)
        S.run.gravity(pr.g_grav(theta), B.WALK_NEWTON)
        assert np.array_equal(S.get_field(B.F_GRAVCOST), c2), "gravity counts after migration"
        assert np.abs(S.get_field(B.F_GRAVACCEL) - o2).max() < 1e-10 * (np.abs(o2).max() + 1e-300), \
            "gravity after migration"


def test_three_shards_reloaded_with_other_problems():
    """Problem A on three logical shards through gravity, SPH and a migration; then the same three contexts are
    given problem B (other n, ngas, domain, splits, softenings, open boundaries), then a problem whose cut
    leaves one of them with nobody."""
    gc.collect()
    base = _in_use()
    contexts = None
    S = None
    print()
    try:
        for which in "ABC":
            t0 = time.time()
            pr, work = _shard_problem(which)
            old = 0.2 + 3.0 * np.random.default_rng(5).random(pr.n)
            S = ShardSet(pr, 3, work=work, fields={"oldacc": old}, contexts=contexts)
            contexts = S.fp
            sizes = [len(g) for g in S.gid]
            if which == "C":
                assert min(sizes) == 0 and sum(sizes) == pr.n
            _shard_step(S, pr, old, shake=(which != "C"))
            print("  problem %s on shards of %r: %.2f s" % (which, sizes, time.time() - t0))
        S.each(lambda fp: fp.sync())
    finally:
        if S is not None:
            S.close()
    assert _in_use() == base


# ------------------------------------------------------------------------------------------------
# the bundle's integrator: flags and per-count fields across a change of counts
# ------------------------------------------------------------------------------------------------
def _load_kick_state(fp, s, fields):
    """tests/test_gpu_kick_bundle.py:device into an existing context"""
    import test_gpu_kick_bundle as TK
    n, ng = len(s["type"]), len(s["entropy"])
    fp.set_counts(n, ng)
    fp.set_field(B.F_POS, s.get("pos", np.zeros((n, 3))))
    fp.set_field(B.F_TI_CURRENT, np.zeros(n, np.int32))
    fp.set_field(B.F_DIVVEL, np.zeros(ng))
    fp.set_field(B.F_PRESSURE, np.zeros(ng))
    for f, k in TK.FIELDS:
        fp.set_field(getattr(B, f), s[k])
    if fields:
        fp.kick_set_fields(drag_accel=s["drag"], gas_dust_momentum=s["ddm"])


def _kick_and_drift(fp, p):
    import test_gpu_kick_bundle as TK
    fp.advance_timesteps(TK.kick_params(p))
    fp.drift(p["Ti_Current"] + (1 << 21), p["Timebase_interval"])
    return {f: fp.get_field(getattr(B, f)) for f in ("F_VEL", "F_VELPRED", "F_ENTROPY", "F_DTENTROPY", "F_TIMEBIN",
                                                      "F_TI_BEGSTEP", "F_POS")}


def test_integration_flags_and_kick_fields_do_not_outlive_their_problem():
    """The bundle's kick with DragAccel and DeltaDustMomentum on one problem, checked against tests/kick_ref.py as
    test_bundle_kick_and_drift_match_the_restatement does; then the flags reset with None and a problem of
    other counts in the same context: kick and drift equal, to the bit, a context that never had flags or fields,
    and the restatement under the minimal flag set."""
    import kick_ref as R
    import test_gpu_kick_bundle as TK
    from test_kick_bundle_cpu import problem
    gc.collect()
    base = _in_use()
    fp = B.ForcePath(0)
    try:
        p, s, tabs = problem(seed=11, ngas=1500, nother=1000)
        assert tabs is None
        f = R.bundle(OuterBoundary=300.0, FeedBackVelocity=10.0)
        _load_kick_state(fp, s, fields=True)
        fp.set_integration_flags(TK.flags_struct(f))
        fp.advance_timesteps(TK.kick_params(p))
        assert R.advance_timesteps(p, f, s)["rc"] == 0
        TK.check(fp, s)
        # other counts, no flags, no fields
        fp.set_integration_flags(None)
        p2, s2, _ = problem(seed=5, ngas=900, nother=700)
        _load_kick_state(fp, s2, fields=False)
        kept = _kick_and_drift(fp, p2)
        fp.sync()
    finally:
        fp.close()
    assert _in_use() == base
    fresh = B.ForcePath(0)
    try:
        _load_kick_state(fresh, s2, fields=False)
        alone = _kick_and_drift(fresh, p2)
    finally:
        fresh.close()
    for k in alone:
        assert np.array_equal(kept[k], alone[k]), k
    assert R.advance_timesteps(p2, R.flags(), s2)["rc"] == 0
    assert np.array_equal(kept["F_TIMEBIN"], s2["timebin"]) and np.array_equal(kept["F_TI_BEGSTEP"], s2["ti_begstep"])
    for fld, k in (("F_VEL", "vel"), ("F_ENTROPY", "entropy")):
        assert relerr(kept[fld], s2[k]) <= 1e-14, k


def test_a_kept_tree_of_another_particle_number_refuses_node_kicks_and_sub_steps():
    """ghip_set_dynamic_tree stays on while the counts change: until a full build has captured the new
    particles, the kept tree is the old set's -- its particle elements index planes sized for the counts of
    now.  Kicking its nodes or taking a sub-step on it is refused with a message; after the build both work,
    and the walk on the kept tree gives the oracle's counts."""
    small, big = RC.SEQUENCES["kept tree"][0], RC.SEQUENCES["kept tree"][1]
    assert small.pr.n < big.pr.n
    fp = B.ForcePath(0)
    try:
        have = RC.device_stage(fp, big, dict(RC.DEFAULTS))[1]
        assert have["dynamic"]
        small.pr.load(fp)                        # fewer particles, the switch still on, no build yet
        act, dv, dt, _ = RC._substep_draw(small, 1)
        for call in (lambda: fp.tree_kick_nodes(act, dv), lambda: fp.tree_substep(dt)):
            with pytest.raises(B.GhipError) as e:
                call()
            assert B.GHIP_ERRORS[e.value.code] == "GHIP_EINVAL" and "particle number changed" in str(e.value)
        got, have = RC.device_stage(fp, small, have)
        assert RC.compare(got, RC.oracle_stage(small), 0) == {}
        fp.sync()
    finally:
        fp.close()
