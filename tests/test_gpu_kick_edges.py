"""k_advance_timesteps (ghip_kick.hip) and k_drift (ghip_drift.hip, d_table_factor of ghip_timefac.h) on the inputs of
tests/kick_edges.py, which tests/test_kick_edges_cpu.py shows to carry every label of kick_ref's trace and to agree
with the oracle: old bin 0 at Ti_Current = 0, blocked and allowed raises at 2^27, TIMEBASE - 2^20, Ti_Current =
TIMEBASE (step and bin 0), all six particle types, MaxSizeTimestep and dt_displacement each winning, kick intervals in
the first two table cells, the interior and the end clamp; a drift with a third of the particles already at time1,
MinGasHsml between the drifted h, and coordinates on every edge of do_box_wrapping in boxes of 1 and 2.5.  The kick
runs through both entry forms -- the plain kernel and the bundle kernel -- and asserts what
test_timestep_and_kick_parity asserts; the drift holds test_drift_parity's bounds and bit equality where the
arithmetic is exact."""
import numpy as np
import pytest

import kick_edges as E
import kick_ref as R
from common import bindings, relerr
from test_gpu_kick_bundle import device, flags_struct, kick_params
from test_kick_edges_cpu import runs

pytestmark = pytest.mark.gpu

RUN_NAMES = ("t0", "mid-max", "mid-disp", "mid-adaptive", "mid-bundle", "late", "end")


def _where(trace, got, want, what, exact=True, tol=0.0):
    """the first particle whose `what` differs, with its labels"""
    got, want = np.asarray(got), np.asarray(want)
    if exact:
        bad = got != want
    else:
        bad = np.abs(got - want) > tol
    if bad.ndim == 2:
        bad = bad.any(axis=1)
    if not bad.any():
        return None
    i = int(np.argmax(bad))
    return "%s differs for %d particles; first %d: got %r, want %r, labels %s" % (
        what, int(bad.sum()), i, got[i], want[i], sorted(trace.get(i, ["inactive"])))


# the bundle's rules exist in the bundle kernel only
FORMS = [(name, form) for name in RUN_NAMES for form in ("plain", "bundle") if (name, form) != ("mid-bundle", "plain")]


@pytest.mark.parametrize("comoving", [False, True])
@pytest.mark.parametrize("name,form", FORMS)
def test_kick_edges_match_the_restatement(name, form, comoving):
    B = bindings()
    run, s, out, trace = [r for r in runs(comoving) if r[0]["name"] == name][0]
    assert run["flagfree"] == (name != "mid-bundle")
    b = run["s"]
    n, ng = len(b["type"]), len(b["entropy"])
    fp = device(b, fields=not run["flagfree"])
    try:
        if form == "bundle":        # with the flags the run needs: none for the flag-free ones (all switches 0)
            fp.set_integration_flags(flags_struct(run["f"]))
        if run["active"] is not None:
            fp.set_active(run["active"])
        tabs = run["tables"]
        cnt, sph = fp.advance_timesteps(kick_params(run["p"]), kick_tables=None if tabs is None else tabs[1:])
        g = fp.get_field
        for fid, k in ((B.F_TIMEBIN, "timebin"), (B.F_TI_BEGSTEP, "ti_begstep")):
            assert np.array_equal(g(fid), s[k]), _where(trace, g(fid), s[k], k)
        assert np.array_equal(cnt[:30], np.bincount(s["timebin"], minlength=30)) and cnt.sum() == n
        assert np.array_equal(sph[:30], np.bincount(s["timebin"][:ng], minlength=30)) and sph.sum() == ng
        bit_equal = [(B.F_VEL, "vel"), (B.F_VELPRED, "velpred")]
        if run["flagfree"]:
            if comoving:        # pow() enters through the MinEgySpec floor
                ent, dA = g(B.F_ENTROPY), g(B.F_DTENTROPY)
                print(name, form, "entropy %.1e dtentropy %.1e" % (
                    relerr(ent, s["entropy"]), np.abs(dA - s["dtentropy"]).max() / np.abs(s["dtentropy"]).max()))
                assert relerr(ent, s["entropy"]) < 1e-14, _where(
                    trace, ent, s["entropy"], "entropy", False, 1e-14 * np.abs(s["entropy"]))
                lim = 1e-14 * np.abs(s["dtentropy"]).max()
                assert np.abs(dA - s["dtentropy"]).max() <= lim, _where(trace, dA, s["dtentropy"], "dtentropy", False, lim)
            else:
                bit_equal += [(B.F_ENTROPY, "entropy"), (B.F_DTENTROPY, "dtentropy")]
            for fid, k in bit_equal:
                assert np.array_equal(g(fid), s[k]), _where(trace, g(fid), s[k], k)
        else:                   # the bundle's run: the levels test_gpu_kick_bundle holds it to
            for fid, k in bit_equal + [(B.F_ENTROPY, "entropy")]:
                assert relerr(g(fid), s[k]) <= 1e-14, _where(trace, g(fid), s[k], k)
            lim = 1e-14 * np.abs(s["dtentropy"]).max()
            assert np.abs(g(B.F_DTENTROPY) - s["dtentropy"]).max() <= lim
            assert np.array_equal(fp.kick_drag_accel(), s["drag"])
        if run["active"] is not None:       # inactive particles: bit-unchanged
            rest = np.setdiff1d(np.arange(n), run["active"])
            gas = rest[rest < ng]
            for fid, k in ((B.F_VEL, "vel"), (B.F_TIMEBIN, "timebin"), (B.F_TI_BEGSTEP, "ti_begstep")):
                assert np.array_equal(g(fid)[rest], b[k][rest]), k
            for fid, k in ((B.F_VELPRED, "velpred"), (B.F_ENTROPY, "entropy"), (B.F_DTENTROPY, "dtentropy")):
                assert np.array_equal(g(fid)[gas], b[k][gas]), k
    finally:
        fp.close()


@pytest.mark.parametrize("comoving", [False, True])
@pytest.mark.parametrize("box", [1.0, 2.5])
@pytest.mark.parametrize("when", E.DRIFT_WHEN)
def test_drift_edges_match_the_restatement(when, box, comoving):
    B = bindings()
    c = E.drift_edge_case(comoving, box, when)
    b = c["s"]
    s, p, (clamped, free) = E.drift_reference(c)
    assert clamped >= 8 and free >= 8
    n, ng = len(b["type"]), len(b["entropy"])
    fp = device(b, fields=False)
    try:
        for fid, k in ((B.F_POS, "pos"), (B.F_TI_CURRENT, "ti_current"), (B.F_DIVVEL, "divvel"),
                       (B.F_PRESSURE, "pressure")):
            fp.set_field(fid, b[k])
        fp.drift(c["time1"], p["Timebase_interval"], min_gas_hsml=p["MinGasHsml"], box_wrap=True, boxsize=box,
                 tables=c["tables"], log_time_begin=p["logTimeBegin"], log_time_max=p["logTimeMax"])
        g = fp.get_field
        pos = g(B.F_POS)
        assert np.array_equal(g(B.F_TI_CURRENT), s["ti_current"])
        err = dict(pos=float(np.abs(pos - s["pos"]).max()), velpred=relerr(g(B.F_VELPRED), s["velpred"]),
                   density=relerr(g(B.F_DENSITY), s["density"]), hsml=relerr(g(B.F_HSML), s["hsml"]),
                   pressure=relerr(g(B.F_PRESSURE), s["pressure"]))
        print(when, box, comoving, {k: "%.1e" % v for k, v in err.items()})
        assert err["pos"] < 1e-15 and err["velpred"] < 1e-14 and err["density"] < 1e-14
        assert err["hsml"] < 1e-14 and err["pressure"] < 1e-13
        assert (pos >= 0).all() and (pos < box).all()
        # the wrap set: bit-equal (its Vel * dt is exact, or its Vel is 0)
        w = c["wrapset"]
        assert np.array_equal(pos[w], s["pos"][w]), (pos[w][:, 0], s["pos"][w][:, 0])
        assert not pos[w[0]].any() and not pos[w[1]].any()      # -1e-17 and BoxSize: 0.0, not BoxSize
        # the clamp: the same particles sit at MinGasHsml, exactly
        h = g(B.F_HSML)[:ng]
        assert np.array_equal(h == p["MinGasHsml"], s["hsml"][:ng] == p["MinGasHsml"])
        # already at time1: bit-unchanged (the wrap set's positions are wrapped, nothing else)
        noop = c["noop"]
        plain = np.setdiff1d(noop, w)
        assert np.array_equal(pos[plain], b["pos"][plain])
        assert np.array_equal(g(B.F_TI_CURRENT)[noop], b["ti_current"][noop])
        assert np.array_equal(g(B.F_HSML)[noop], b["hsml"][noop])
        gas = noop[noop < ng]
        assert len(gas) >= 8
        for fid, k in ((B.F_VELPRED, "velpred"), (B.F_DENSITY, "density"), (B.F_PRESSURE, "pressure")):
            assert np.array_equal(g(fid)[gas], b[k][gas]), k
    finally:
        fp.close()
