"""Who owns what: a context gives back every byte of device memory it took, whatever it was driven
through, and the state the library makes once per process survives the contexts that used it.

The yardstick is the library's own count of the bytes its DevBufs hold (ghip_device_bytes_in_use), compared
for equality: the card's free memory would also see every other process on it.  Two identical cycles in one
process -- one context through everything that allocates lazily, and a 2-shard set -- must each end at the
count they started from, and the second must reproduce the first bit for bit.

One result is not defined to the bit: the mesh force of ghip_pm_periodic, whose mass assignment adds with
fp64 atomics in whatever order the wavefronts arrive.  Two calls of it differ by that round-off
in any build, in one context as well as in two, so the cycles' GRAVPM are held to the bound DESIGN 4.8
documents for it -- 1e-11 of the largest component -- and everything else to equality."""
import gc

import numpy as np
import pytest

import test_gpu_potential as TP
from common import O, bindings
from test_gpu_dust import DustCase
from test_gpu_dust_dd import DdDust
from test_gpu_sink import _run_sink_op

pytestmark = pytest.mark.gpu
B = bindings()
TOL_MESH = 1e-11      # of the largest component: atomic-add order of the mass assignment


def _in_use():
    return int(B.lib().ghip_device_bytes_in_use())


def _single_context(out):
    """tree, Newton+Ewald pair, density, hydro, PM, time-bin counts, dust density and drag, potential,
    energy statistics, the kept tree on and off"""
    case = DustCase(1, ndust=300, ng=8)
    pr = case.pr
    n = pr.n
    _, fp = case.device()
    try:
        assert _in_use() > out["base"]          # (the count sees this context)
        fp.set_field(B.F_OLDACC, np.zeros(n))
        fp.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON_EWALD)
        fp.density(pr.g_dens())
        fp.update_hmax()
        fp.hydro(pr.g_hydro())
        out["gravaccel"] = fp.get_field(B.F_GRAVACCEL)
        out["gravcost"] = fp.get_field(B.F_GRAVCOST)
        out["density"] = fp.get_field(B.F_DENSITY)
        out["hydroaccel"] = fp.get_field(B.F_HYDROACCEL)
        fp.pm_periodic(16, pr.box, 1.0)
        out["gravpm"] = fp.get_field(B.F_GRAVPM)
        # the histogram against the arrays that were uploaded
        cnt, sph = fp.timebin_counts()
        typ = np.asarray(pr.ic["type"])
        assert np.array_equal(cnt, np.bincount(case.timebin, minlength=32))
        assert np.array_equal(sph, np.bincount(case.timebin[typ == 0], minlength=32))
        assert cnt.sum() == n and sph.sum() == pr.ngas
        out["timebins"] = np.concatenate([cnt, sph])
        d7 = fp.dust_density(case.gparams(), case.dust)
        drag = case.drag(fp, np.arange(len(case.dust)), d7)
        out["d7"] = d7
        for k, v in drag.items():
            out["drag_" + k] = v
        out["drag_heating"] = fp.dust_drag_heating()
        fp.potential(TP._pot_params(pr, 0.5))
        out["potential"] = fp.get_potential()
        gq = fp.global_quantities(TP._gq_params(0), old_photon_momentum=np.zeros(n))
        for k, v in gq.items():
            out["gq_" + k] = np.asarray(v)
        # the kept tree: captured by a full build, kicked, drifted by a sub-step, walked, released
        fp.set_dynamic_tree(True)
        pr.device_tree(fp)
        dt = 0.002 * pr.box / np.abs(pr.ic["vel"]).max()
        idx = np.arange(0, n, 7, dtype=np.int32)
        fp.tree_kick_nodes(idx, 1e-3 * np.ones((len(idx), 3)))
        fp.tree_substep(dt)
        held = _in_use()
        fp.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
        out["gravaccel_kept_tree"] = fp.get_field(B.F_GRAVACCEL)
        out["kept_tree"] = fp.tree_dump_dynamic()["xm"]
        fp.set_dynamic_tree(False)
        assert _in_use() < held                  # (released while the context lives)
        fp.sync()
    finally:
        fp.close()


def _two_shards(out):
    """gravity, density, the dust passes, a sink pass, the potential, a migration, gravity again"""
    case = DustCase(1, ndust=300, ng=8)
    pr, sp = case.pr, case.sp
    n = pr.n
    T = DdDust(case, 2)                          # GHIP_DD_GRAVITY and GHIP_DD_DENSITY of this step
    S = T.S
    try:
        out["dd_density"] = S.get_field(B.F_DENSITY)
        d7, _ = T.density()
        drag, _ = T.drag(d7)
        out["dd_d7"] = d7
        for k, v in drag.items():
            out["dd_drag_" + k] = v
        out["dd_drag_heating"] = T.heat()
        where = S.locate(sp.sinks)
        gd = pr.g_dens()
        res = _run_sink_op(S, B.DD_SINK_DENSITY, lambda r: B.dd_sink_args(
            where[r][0], dens=gd, ngb_factor=1.5, hsml=sp.hsml[sp.sinks][where[r][1]]))
        sink_rho = np.zeros(len(sp.sinks))
        for (_, pos), a in zip(where, res):
            sink_rho[pos] = a["density"]
        out["dd_sink_density"] = sink_rho
        S.run.potential(TP._pot_params(pr, 0.5))
        pot = np.zeros(n)
        for r, fp in enumerate(S.fp):
            pot[S.gid[r]] = fp.get_potential()
        out["dd_potential"] = pot
        # a shake that sends particles to the other shard
        rng = np.random.default_rng(21)
        newpos = np.mod(pr.ic["pos"] + 0.08 * pr.box * rng.standard_normal((n, 3)), pr.box)
        newpos[newpos >= pr.box] = 0.0
        S.set_field(B.F_POS, newpos)
        ext = O.domain_extent(newpos)
        S.each(lambda fp: fp.dd_set_domain(ext[0], ext[1], ext[2], pr.force_soft))
        before = S.owner.copy()
        S.migrate()
        assert int((S.owner != before).sum()) > 0
        S.run.gravity(pr.g_grav(pr.theta), B.WALK_NEWTON)
        out["dd_gravaccel_migrated"] = S.get_field(B.F_GRAVACCEL)
        S.each(lambda fp: fp.sync())
    finally:
        S.close()


def _cycle(base):
    out = {"base": base}
    _single_context(out)
    assert _in_use() == base, "a destroyed context kept device memory"
    _two_shards(out)
    assert _in_use() == base, "destroyed shards kept device memory"
    del out["base"]
    return out


def test_contexts_give_back_what_they_took_and_a_second_cycle_repeats_the_first():
    gc.collect()                                 # (contexts earlier tests dropped without closing)
    base = _in_use()
    first = _cycle(base)
    second = _cycle(base)
    assert first.keys() == second.keys() and len(first) > 20
    differ = [k for k in first if not np.array_equal(first[k], second[k])]
    mesh = np.abs(first["gravpm"] - second["gravpm"]).max() / np.abs(first["gravpm"]).max()
    print("\nresults that differ between the cycles: %r; GRAVPM by %.3e of its largest component" % (differ, mesh))
    assert [k for k in differ if k != "gravpm"] == []
    assert mesh < TOL_MESH
    # ... and the cycles computed something
    for k in ("gravaccel", "gravpm", "potential", "d7", "dd_d7", "dd_potential", "dd_sink_density",
              "dd_gravaccel_migrated", "gravaccel_kept_tree"):
        assert np.all(np.isfinite(first[k])) and np.abs(first[k]).max() > 0, k
