"""The sinks on the resident state (ghip_sinks_set_table / _get_table / _density, ghip_blackhole_accretion,
ghip_sfr_form_sinks) against the per-pass path of today -- ghip_sink_density, ghip_blackhole_evaluate and
ghip_blackhole_swallow with host arrays, the Mdot step, the finish and the conversion done on the host by
tests/sink_accretion_ref.py -- and, on the inputs of tests/common.py, against tests/sink_ref.py (all pairs).

The two paths run the same kernels on the same inputs, and the new arithmetic is compiled without contraction,
so everything is compared bit for bit: MASS, VEL, HSML, SwallowID, Injected_BH_Energy, every column of the
table, the counts and the per-bin sums -- with one exception, bounded by its own rounding: the injected energy of
a gas particle that three or more sinks feed, whose atomic adds come in the order the hardware chooses
(_same_fields)."""
import numpy as np
import pytest

import sfr_ref
import sink_accretion_cases as AC
import sink_accretion_ref as AR
from common import SINK_CASES, SINK_SWITCHES, bindings, relerr, sink_case, sink_over, sink_reference

pytestmark = pytest.mark.gpu
EINVAL = -90002
NGB = AC.NGB_FACTOR


def _device(sp, gas_density=None):
    B = bindings()
    pr = sp.pr
    fp = pr.device()
    fp.set_field(B.F_HSML, sp.hsml)
    fp.set_field(B.F_ID, sp.ids.view(np.int32))
    fp.set_field(B.F_DENSITY, sp.gas_density if gas_density is None else gas_density)
    pr.device_tree(fp)
    return B, fp


def _gacc(B, acc):
    p = B.BhAccretionParams()
    for k, _ in p._fields_:
        setattr(p, k, getattr(acc, k))
    return p


def _state_of(B, rows):
    return dict(bh_mass=rows[:, B.SK_BH_MASS].copy(), accdisc=rows[:, B.SK_ACCDISC_MASS].copy(),
                mdot=rows[:, B.SK_BH_MDOT].copy(), dust_mass=rows[:, B.SK_DUST_MASS].copy(),
                total_mass=rows[:, B.SK_TOTAL_MASS].copy())


def _per_pass(B, fp, dens_params, gp, par, acc, sinks, ids5, rows):
    """blackhole_accretion() as a host drives it today, for the sinks `sinks` (particle indices in active-list
    order) whose rows [len(sinks)][SK_COUNT] the host keeps: the three passes through the library with host
    arrays, the Mdot step and the finish on the host.  Returns (rows, report)."""
    sinks = np.ascontiguousarray(sinks, np.int32)
    rows = rows.copy()
    if len(sinks) == 0:
        fp.sink_reset()
        return rows, dict(bin_mass=np.zeros(32), bin_dynmass=np.zeros(32), bin_mdot=np.zeros(32),
                          counts=np.zeros(3, np.int64), iterations=0)
    d = fp.sink_density(dens_params, NGB, sinks, fp.get_field(B.F_HSML)[sinks])
    tb = fp.get_field(B.F_TIMEBIN)[sinks]
    st, _ = AR.mdot_step(_state_of(B, rows), fp.get_field(B.F_MASS)[sinks], tb, par.dt_fac, acc)
    fp.sink_reset()
    fp.blackhole_evaluate(gp, sinks, ids5, st["mdot"], d["density"])
    go = fp.blackhole_swallow(gp, sinks, ids5, st["bh_mass"])
    st["bh_mass"] = go["bh_mass"]
    vel, mass = fp.get_field(B.F_VEL), fp.get_field(B.F_MASS)
    st, v5, m5, rep, _ = AR.finish(st, vel[sinks], mass[sinks], tb, go["acc_mass"], go["acc_bhmass"],
                                   go["acc_dustmass"], go["acc_momentum"], acc, par.dust)
    vel[sinks], mass[sinks] = v5, m5
    fp.set_field(B.F_VEL, vel)
    fp.set_field(B.F_MASS, mass)
    rows[:] = AC.rows_of(B, st, d)
    rows[:, B.SK_ACC_MASS] = go["acc_mass"]
    rows[:, B.SK_ACC_BHMASS] = go["acc_bhmass"]
    rows[:, B.SK_ACC_DUSTMASS] = go["acc_dustmass"]
    rows[:, B.SK_ACC_MOMENTUM:B.SK_ACC_MOMENTUM + 3] = go["acc_momentum"]
    rep["counts"] = go["counts"]
    rep["iterations"] = d["iterations"]
    return rows, rep


def _same_report(got, want):
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    for k in ("bin_mass", "bin_dynmass", "bin_mdot"):
        assert np.array_equal(got[k], want[k]), k


def _feeders(fp, B, sinks, box, periodic):
    """per gas particle, how many of the sinks `sinks` hold it inside their search sphere (r < h, with a margin of
    1e-9 so that a tie counts): an upper bound of the atomic adds its Injected_BH_Energy receives in one call"""
    pos, h = fp.get_field(B.F_POS), fp.get_field(B.F_HSML)
    k = np.zeros(fp.ngas, np.int64)
    for i in sinks:
        d = pos[:fp.ngas] - pos[i][None, :]
        if periodic:
            d -= box * np.round(d / box)
        k += np.sqrt((d * d).sum(axis=1)) < h[i] * (1 + 1e-9)
    return k


def _same_fields(B, fa, fb, fields, feeders=None):
    """Bit for bit, with one exception: a gas particle inside the spheres of THREE or more sinks gets
    its Injected_BH_Energy by as many atomic adds, whose order the hardware chooses -- one or two positive terms
    added to 0 give the same sum in any order, three need not.  Two orders of k positive terms differ by at most
    (k - 1) EPS x the sum ((k - 1) roundings of at most half an ulp of a partial sum each).  feeders [ngas]: k per
    gas particle (None: no call since the marks were compared last).  cooling_and_starformation spends the
    injection of an active particle into DtEntropy: there the bound of tests/test_gpu_sfr_cooling.py, 1e-13 A / dt."""
    many = np.zeros(fa.ngas, bool) if feeders is None else feeders >= 3
    for f in fields:
        a, b = fa.get_field(f), fb.get_field(f)
        if f == B.F_DTENTROPY and many.any():
            A, tb = fa.get_field(B.F_ENTROPY), fa.get_field(B.F_TIMEBIN)[:fa.ngas]
            dt = np.where(tb > 0, (1 << tb).astype(np.float64), 1.0) * 1e-3
            assert np.all(np.abs(a - b)[many] <= 1e-13 * ((np.abs(A) + np.abs(a) * dt) / dt)[many])
            a, b = a[~many], b[~many]
        assert np.array_equal(a, b), "field %d differs at %s" % (f, np.argwhere(a != b)[:5].tolist())
    (swa, inja), (swb, injb) = fa.sink_marks(), fb.sink_marks()
    assert np.array_equal(swa, swb), "SwallowID"
    bad = np.where((inja != injb) & ~many)[0]
    assert len(bad) == 0, "Injected_BH_Energy differs at %s: %s against %s" % (bad[:5], inja[bad[:5]], injb[bad[:5]])
    if many.any():
        k = feeders[many]
        assert np.all(np.abs(inja - injb)[many] <= (k - 1) * 2.0 ** -52 * np.maximum(inja, injb)[many])
        print("Injected_BH_Energy: %d particles with 3 or more feeders, %d of them differ, by at most %.2g"
              % (many.sum(), (inja != injb).sum(), (np.abs(inja - injb)[many] / np.maximum(injb[many], 1e-300)).max()))


# ------------------------------------------------------------------------------------------------
# a. the composite equals the per-pass path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic", [0, 1])
@pytest.mark.parametrize("switches", SINK_SWITCHES)
def test_composite_equals_the_per_pass_path(periodic, switches):
    sp = AC.stock(periodic)
    pr = sp.pr
    state = AC.state_for(sp)
    acc = AC.acc_for(sp, state)
    par = AC.ref_par(sp, switches)
    # chosen on the CPU: the reference path takes the clamp for some sinks and not for others
    _, br = AR.mdot_step(state, pr.ic["mass"][sp.sinks], pr.timebin[sp.sinks], par.dt_fac, acc)
    assert any("clamp" in b for b in br) and any("noclamp" in b for b in br)
    ids5 = sp.ids[sp.sinks]
    B, fa = _device(sp)
    _, fb = _device(sp)
    try:
        gp = sp.params(B.BhParams, **sink_over(*switches))
        rows_a, rep_a = _per_pass(B, fa, pr.g_dens(), gp, par, acc, sp.sinks, ids5, AC.rows_of(B, state))
        fb.sinks_set_table(ids5, AC.rows_of(B, state))
        it = fb.sinks_density(pr.g_dens(), NGB)
        rep_b = fb.blackhole_accretion(gp, _gacc(B, acc))
        assert it == rep_a["iterations"] >= 1 and rep_b["nactive"] == len(sp.sinks)
        assert rep_b["counts"].sum() > 10
        _same_report(rep_b, rep_a)
        _same_fields(B, fa, fb, (B.F_MASS, B.F_VEL, B.F_HSML, B.F_POS, B.F_TYPE),
                     _feeders(fb, B, sp.sinks, pr.box, periodic))
        ids_t, rows_b = fb.sinks_table()
        order = np.argsort(ids5)
        assert np.array_equal(ids_t, ids5[order])
        for c in range(B.SK_COUNT):
            assert np.array_equal(rows_b[:, c], rows_a[order, c]), "column %d" % c
        # something happened: sinks grew, the disc was drawn from, the masses of the victims are gone
        grew = rows_b[:, B.SK_ACC_MASS] > 0
        assert grew.sum() >= 2 and np.all(rows_b[:, B.SK_BH_MDOT] > 0)
        assert (fb.get_field(B.F_MASS) == 0).sum() == rep_b["counts"].sum()
    finally:
        fa.close()
        fb.close()


# ------------------------------------------------------------------------------------------------
# b. the inputs of SINK_CASES against all pairs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,periodic,switches", SINK_CASES)
def test_sink_inputs_against_all_pairs(name, periodic, switches):
    """Contested victims, chains, mutual claims, a swallowed sink that must not swallow, the central object, the
    branches of the h iteration.  Marks and counts exact; the masses of everybody but the sinks exact (victims at
    0); the columns that the Mdot step alone writes (AccDisc_Mass of a sink that accreted nothing, BH_Mdot) exact
    -- they are arithmetic on the inputs; sums with the tolerances of check_sink_passes (1e-13 of the largest,
    the density columns 1e-12: the order of the wave reductions against sink_ref's long-double sums)."""
    sp = sink_case(name, periodic)
    ref = sink_reference(name, periodic, *switches)
    pr, ic, sk = sp.pr, sp.pr.ic, sp.sinks
    state = AC.state_for(sp)
    acc = AC.acc_for(sp, state)
    r = AR.accretion(ic["pos"], ic["vel"], ic["mass"], ic["type"], sp.ids, sk, sp.dens["hsml"], pr.timebin,
                     sp.gas_density, sp.dens["density"], state, ref["par"], acc)
    assert np.array_equal(r["sw"], ref["sw"])          # (the Mdot step does not touch what the marks depend on)
    B, fp = _device(sp)
    try:
        gp = sp.params(B.BhParams, **ref["over"])
        ids5 = sp.ids[sk]
        fp.sinks_set_table(ids5, AC.rows_of(B, state))
        it = fp.sinks_density(pr.g_dens(), NGB)
        assert it == sp.dens["iterations"] >= 1
        assert relerr(fp.get_field(B.F_HSML)[sk], sp.dens["hsml"][sk]) < 1e-13
        rep = fp.blackhole_accretion(gp, _gacc(B, acc))
        sw, inj = fp.sink_marks()
        assert np.array_equal(sw, ref["sw"]), "SwallowID differs at %s" % np.where(sw != ref["sw"])[0][:10]
        assert np.array_equal(rep["counts"], r["report"]["counts"]) and rep["nactive"] == len(sk)
        top = np.abs(r["inj"]).max()
        assert top > 0 and np.abs(inj - r["inj"]).max() <= 1e-12 * top
        mass, vel = fp.get_field(B.F_MASS), fp.get_field(B.F_VEL)
        rest = np.setdiff1d(np.arange(pr.n), sk)
        assert np.array_equal(mass[rest], r["mass"][rest]) and np.array_equal(vel[rest], ic["vel"][rest])
        assert np.array_equal(mass[sk] == 0, r["mass"][sk] == 0)
        assert np.abs(mass[sk] - r["mass"][sk]).max() <= 1e-13 * r["mass"][sk].max()
        assert np.abs(vel[sk] - r["vel"][sk]).max() <= 1e-12 * np.abs(r["vel"][sk]).max()
        ids_t, rows = fp.sinks_table()
        order = np.argsort(ids5)
        assert np.array_equal(ids_t, ids5[order])
        rows = rows[np.argsort(order)]                 # back to list order
        st, so = r["state"], r["swallow"]
        assert np.array_equal(rows[:, B.SK_BH_MDOT], st["mdot"])
        quiet = so["acc_mass"] == 0
        assert np.array_equal(rows[quiet, B.SK_ACCDISC_MASS], st["accdisc"][quiet])
        assert np.array_equal(rows[quiet, B.SK_BH_MASS], st["bh_mass"][quiet])
        # BH_Mass of a sink is zeroed only if it really was swallowed, not if it was merely marked
        assert np.array_equal(rows[:, B.SK_BH_MASS] == 0, so["swallowed"][sk] | (st["bh_mass"] == 0))
        assert np.array_equal(rows[:, B.SK_ACC_MASS] > 0, so["acc_mass"] > 0)
        assert not rows[so["skipped"]][:, B.SK_ACC_MASS:].any()      # a claimed sink swept nothing
        for col, want in ((B.SK_BH_MASS, st["bh_mass"]), (B.SK_ACCDISC_MASS, st["accdisc"]),
                          (B.SK_DUST_MASS, st["dust_mass"]), (B.SK_TOTAL_MASS, st["total_mass"]),
                          (B.SK_ACC_MASS, so["acc_mass"]), (B.SK_ACC_BHMASS, so["acc_bhmass"]),
                          (B.SK_ACC_DUSTMASS, so["acc_dustmass"])):
            assert np.abs(rows[:, col] - want).max() <= 1e-13 * max(np.abs(want).max(), 1e-300), col
        mom = rows[:, B.SK_ACC_MOMENTUM:B.SK_ACC_MOMENTUM + 3]
        assert np.abs(mom - so["acc_momentum"]).max() <= 1e-13 * max(np.abs(so["acc_momentum"]).max(), 1e-300)
        assert relerr(rows[:, B.SK_BH_DENSITY], sp.dens["density"]) < 1e-12
        assert relerr(rows[:, B.SK_BH_ENTROPY], sp.dens["entropy"]) < 1e-12
        assert np.abs(rows[:, B.SK_NUMNGB] - sp.dens["numngb"]).max() < 1e-10
        for k in ("bin_mass", "bin_dynmass", "bin_mdot"):
            assert np.abs(rep[k] - r["report"][k]).max() <= 1e-13 * max(np.abs(r["report"][k]).max(), 1e-300), k
        if name == "pair":      # both sinks and all their victims keep their mass, the counts are 0
            assert not rep["counts"].any() and np.array_equal(mass, ic["mass"]) and (sw > 0).sum() >= 6
    finally:
        fp.close()


# ------------------------------------------------------------------------------------------------
# c. formation
# ------------------------------------------------------------------------------------------------
def _sfr_params(B, pr, crit):
    d = sfr_ref.params(cooling=sfr_ref.NONE, dust=0, Timebase_interval=pr.timebase, CritPhysDensity_code=crit,
                       OriginalGasMass=float(pr.ic["mass"][0]), MinEgySpec=1e-6)
    p = B.SfrParams()
    for k, v in d.items():
        if k == "smbh_pos":
            for c in range(3):
                p.smbh_pos[c] = float(v[c])
        else:
            setattr(p, k, v)
    return p


@pytest.mark.parametrize("limited", [1, 0])
def test_formation(limited):
    sp = AC.stock(1)
    pr = sp.pr
    n, ngas = pr.n, pr.ngas
    rng = np.random.default_rng(21)
    dens = 0.5 + rng.random(ngas)
    crit = float(np.quantile(dens, 0.95))              # about 5 % of the gas are candidates
    B, fp = _device(sp, gas_density=dens)
    try:
        state = AC.state_for(sp)
        ids5 = sp.ids[sp.sinks]
        fp.sinks_set_table(ids5, AC.rows_of(B, state))
        act = rng.permutation(n)[: (3 * n) // 4].astype(np.int32)      # an active subset, permuted
        fp.set_active(act)
        cand = fp.sfr_cooling(_sfr_params(B, pr, crit))
        assert 20 < len(cand) < ngas // 10
        u01 = rng.random(len(cand))
        want = AR.form_sinks(cand, u01, pr.ic["mass"], pr.ic["type"], pr.timebin, limited)

        def unchanged(ids_w, rows_w):
            assert np.array_equal(fp.get_field(B.F_TYPE), pr.ic["type"])
            assert np.array_equal(fp.get_field(B.F_MASS), pr.ic["mass"])
            ids_t, rows_t = fp.sinks_table()
            assert np.array_equal(ids_t, ids_w) and np.array_equal(rows_t, rows_w)
        ids0, rows0 = fp.sinks_table()
        with pytest.raises(B.GhipError) as e:
            fp.sfr_form_sinks(len(cand) + 1, np.r_[u01, 0.5], limited)
        assert e.value.code == EINVAL and str(len(cand)) in str(e.value)
        unchanged(ids0, rows0)
        rep = fp.sfr_form_sinks(len(cand), u01, limited)
        assert rep["stars_converted"] == len(cand) and rep["sum_mass_stars"] == want["sum_mass_stars"]
        assert np.array_equal(rep["converted_in_bin"], want["converted_in_bin"])
        typ, mass = fp.get_field(B.F_TYPE), fp.get_field(B.F_MASS)
        assert np.array_equal(typ, want["type"]) and np.array_equal(mass, want["mass"])
        assert (typ[:ngas] == 5).sum() == len(cand)
        all_ids = np.r_[ids5, sp.ids[cand]]
        all_rows = np.vstack([AC.rows_of(B, state), AC.rows_of(B, want["rows"])])
        order = np.argsort(all_ids)
        ids_t, rows_t = fp.sinks_table()
        assert np.array_equal(ids_t, all_ids[order]) and np.array_equal(rows_t, all_rows[order])
        # a second call: the candidates are consumed, and nothing changes
        pr_type, pr_mass = pr.ic["type"], pr.ic["mass"]
        pr.ic["type"], pr.ic["mass"] = typ, mass
        try:
            with pytest.raises(B.GhipError) as e:
                fp.sfr_form_sinks(len(cand) - 1, u01, limited)
            assert e.value.code == EINVAL
            unchanged(ids_t, rows_t)
        finally:
            pr.ic["type"], pr.ic["mass"] = pr_type, pr_mass
        # the records leave the gas block with ghip_rearrange as any converted gas does; the table stays
        res = fp.rearrange()
        assert (res.numpart, res.ngas, res.converted) == (n, ngas - len(cand), len(cand))
        ids_r, rows_r = fp.sinks_table()
        assert np.array_equal(ids_r, ids_t) and np.array_equal(rows_r, rows_t)
    finally:
        fp.close()


# ------------------------------------------------------------------------------------------------
# d. three steps in a row on one context
# ------------------------------------------------------------------------------------------------
def test_three_steps_on_one_context():
    """Per step: the active list from the time bins (bins 1 and 2 of 1..3: some sinks are inactive), tree,
    sinks_density, blackhole_accretion, sfr_cooling, sfr_form_sinks, rearrange, peano_order -- against the same
    steps on a second context through the per-pass calls, the host keeping the per-sink rows by particle index
    and permuting them by ghip_sequence_get_map."""
    sp = AC.stock(1)
    pr = sp.pr
    rng = np.random.default_rng(31)
    switches = (0, 0)
    par = AC.ref_par(sp, switches)
    dens0 = 0.5 + rng.random(pr.ngas)
    B, fa = _device(sp, gas_density=dens0)
    _, fb = _device(sp, gas_density=dens0)
    fields = (B.F_POS, B.F_VEL, B.F_MASS, B.F_TYPE, B.F_HSML, B.F_TIMEBIN, B.F_ID, B.F_DENSITY, B.F_ENTROPY,
              B.F_DTENTROPY)
    try:
        gp = sp.params(B.BhParams, **sink_over(*switches))
        state = AC.state_for(sp)
        acc = AC.acc_for(sp, state)
        gacc = _gacc(B, acc)
        # the host's per-sink arrays of path A: particle index, ID, row
        idx_a, ids_a, rows_a = sp.sinks.copy(), sp.ids[sp.sinks].copy(), AC.rows_of(B, state)
        fb.sinks_set_table(ids_a, rows_a)
        corner, dlen = pr.extent[0], pr.extent[2]
        formed_total = swallowed_sinks = 0
        for step in range(3):
            typ, tb = fa.get_field(B.F_TYPE), fa.get_field(B.F_TIMEBIN)
            ids_all = fa.get_field(B.F_ID).view(np.uint32)
            act = np.where(tb <= 2)[0].astype(np.int32)
            for fp in (fa, fb):
                fp.set_active(act)
                fp.tree_build(pr.extent[0], pr.extent[1], pr.extent[2], pr.force_soft)
            sinks = act[typ[act] == 5]
            slot = {int(i): k for k, i in enumerate(idx_a)}
            sel = np.array([slot[int(i)] for i in sinks], np.int64)
            inactive = np.setdiff1d(np.arange(len(idx_a)), sel)
            assert len(sel) >= 3 and len(inactive) >= 1
            ids_b0, rows_b0 = fb.sinks_table()
            # ---- path A ----
            new_rows, rep_a = _per_pass(B, fa, pr.g_dens(), gp, par, acc, sinks, ids_all[sinks], rows_a[sel])
            rows_a[sel] = new_rows
            # ---- path B ----
            it = fb.sinks_density(pr.g_dens(), NGB)
            rep_b = fb.blackhole_accretion(gp, gacc)
            assert it == rep_a["iterations"] and rep_b["nactive"] == len(sinks)
            _same_report(rep_b, rep_a)
            swallowed_sinks += int(rep_b["counts"][1])
            feeders = _feeders(fb, B, sinks, pr.box, 1)
            ids_b, rows_b = fb.sinks_table()
            order = np.argsort(ids_a)
            assert np.array_equal(ids_b, ids_a[order]) and np.array_equal(rows_b, rows_a[order])
            quiet = np.isin(ids_b, ids_a[inactive])    # the inactive sinks' rows: untouched, bit for bit
            assert quiet.sum() == len(inactive) and np.array_equal(rows_b[quiet], rows_b0[quiet])
            # ---- cooling and formation ----
            gas = np.where(typ[:fa.ngas] == 0)[0]
            crit = float(np.quantile(fa.get_field(B.F_DENSITY)[gas], 0.97))
            sfp = _sfr_params(B, pr, crit)
            cand_a, cand_b = fa.sfr_cooling(sfp), fb.sfr_cooling(sfp)
            assert np.array_equal(cand_a, cand_b) and len(cand_a) >= 5
            u01 = rng.random(len(cand_a))
            mass = fa.get_field(B.F_MASS)
            want = AR.form_sinks(cand_a, u01, mass, typ, tb, 1)
            fa.set_field(B.F_TYPE, want["type"])
            fa.set_field(B.F_MASS, want["mass"])
            idx_a = np.r_[idx_a, cand_a]
            ids_a = np.r_[ids_a, ids_all[cand_a]]
            rows_a = np.vstack([rows_a, AC.rows_of(B, want["rows"])])
            rep = fb.sfr_form_sinks(len(cand_b), u01, 1)
            assert rep["stars_converted"] == len(cand_a) and rep["sum_mass_stars"] == want["sum_mass_stars"]
            formed_total += len(cand_a)
            # ---- rearrange, peano order ----
            gone = fa.get_field(B.F_MASS)[idx_a] == 0
            ra, rb = fa.rearrange(), fb.rearrange()
            assert (ra.numpart, ra.ngas, ra.count_elim) == (rb.numpart, rb.ngas, rb.count_elim)
            new_of_old, old_of_new = fa.sequence_map()
            feeders = np.r_[feeders, np.zeros(len(new_of_old) - len(feeders), np.int64)][old_of_new][:fa.ngas]
            idx_a = new_of_old[idx_a]
            assert np.array_equal(idx_a < 0, gone)
            keep = idx_a >= 0
            idx_a, ids_a, rows_a = idx_a[keep], ids_a[keep], rows_a[keep]
            ids_b, rows_b = fb.sinks_table()
            order = np.argsort(ids_a)
            assert np.array_equal(ids_b, ids_a[order]) and np.array_equal(rows_b, rows_a[order])
            if fa.peano_order(corner, dlen):
                new_of_old, old_of_new = fa.sequence_map()
                feeders = feeders[old_of_new[:fa.ngas]]
                idx_a = new_of_old[idx_a]
            fb.peano_order(corner, dlen)
            assert fa.n == fb.n and fa.ngas == fb.ngas
            print("step", step, "sinks", len(idx_a), "formed", len(cand_a), "counts", rep_b["counts"])
            _same_fields(B, fa, fb, fields, feeders)
            assert np.array_equal(np.sort(idx_a), np.where(fa.get_field(B.F_TYPE) == 5)[0])
            ids_b2, rows_b2 = fb.sinks_table()         # neither call moved the table
            assert np.array_equal(ids_b2, ids_b) and np.array_equal(rows_b2, rows_b)
        assert formed_total >= 15
    finally:
        fa.close()
        fb.close()


# ------------------------------------------------------------------------------------------------
# e. errors and lifetime
# ------------------------------------------------------------------------------------------------
def test_errors_and_lifetime():
    import gc
    B = bindings()
    L = B.lib()
    gc.collect()              # (contexts that earlier tests dropped without closing go now, not in between)
    bytes0 = L.ghip_device_bytes_in_use()
    sp = AC.stock(1)
    pr = sp.pr
    state = AC.state_for(sp)
    acc = AC.acc_for(sp, state)
    ids5, rows = sp.ids[sp.sinks], AC.rows_of(bindings(), state)
    gp = sp.params(B.BhParams, **sink_over(0, 0))
    fp = pr.device()
    try:
        fp.set_field(B.F_HSML, sp.hsml)
        fp.set_field(B.F_DENSITY, sp.gas_density)
        # the table is keyed by ID: refused before GHIP_F_ID is given
        with pytest.raises(B.GhipError) as e:
            fp.sinks_set_table(ids5, rows)
        assert e.value.code == EINVAL and "GHIP_F_ID" in str(e.value)
        fp.set_field(B.F_ID, sp.ids.view(np.int32))
        pr.device_tree(fp)
        # no table yet
        for call in (lambda: fp.sinks_table(), lambda: fp.sinks_density(pr.g_dens(), NGB),
                     lambda: fp.blackhole_accretion(gp, _gacc(B, acc))):
            with pytest.raises(B.GhipError) as e:
                call()
            assert e.value.code == EINVAL and "no sink table" in str(e.value)
        # a duplicate ID is refused, and names it
        dup = ids5.copy()
        dup[3] = dup[5]
        with pytest.raises(B.GhipError) as e:
            fp.sinks_set_table(dup, rows)
        assert e.value.code == EINVAL and " %d " % dup[5] in str(e.value)
        # a Type-5 target without a row is refused, and the message names its ID; nothing was changed
        lost = 2
        fp.sinks_set_table(np.delete(ids5, lost), np.delete(rows, lost, axis=0))
        mass0, vel0 = fp.get_field(B.F_MASS), fp.get_field(B.F_VEL)
        for call in (lambda: fp.sinks_density(pr.g_dens(), NGB), lambda: fp.blackhole_accretion(gp, _gacc(B, acc))):
            with pytest.raises(B.GhipError) as e:
                call()
            assert e.value.code == EINVAL and "ID %d " % ids5[lost] in str(e.value)
        assert np.array_equal(fp.get_field(B.F_MASS), mass0) and np.array_equal(fp.get_field(B.F_VEL), vel0)
        ids_t, rows_t = fp.sinks_table()
        assert np.array_equal(rows_t, np.delete(rows, lost, axis=0)[np.argsort(np.delete(ids5, lost))])
        assert not fp.sink_marks()[0].any()
        # the rows come back in ascending ID order whatever order they were given in
        perm = np.random.default_rng(2).permutation(len(ids5))
        fp.sinks_set_table(ids5[perm], rows[perm])
        ids_t, rows_t = fp.sinks_table()
        assert np.array_equal(ids_t, np.sort(ids5)) and np.array_equal(rows_t, rows[np.argsort(ids5)])
        # refused after set_counts with other counts until it is given again
        fp.set_counts(pr.n - 1, pr.ngas)
        for call in (lambda: fp.sinks_table(), lambda: fp.sinks_density(pr.g_dens(), NGB),
                     lambda: fp.sfr_form_sinks(0, np.zeros(1), 1)):
            with pytest.raises(B.GhipError) as e:
                call()
            assert e.value.code == EINVAL
        pr.load(fp)
        fp.set_field(B.F_ID, sp.ids.view(np.int32))
        with pytest.raises(B.GhipError) as e:
            fp.sinks_table()
        assert e.value.code == EINVAL and "again" in str(e.value)
        fp.sinks_set_table(ids5, rows)
        assert len(fp.sinks_table()[0]) == len(ids5)
        fp.sinks_clear()
        with pytest.raises(B.GhipError):
            fp.sinks_table()
        fp.sinks_set_table(ids5, rows)
        # one GPU: refused on a replicated shard
        fp.set_shard(0, 2)
        for call in (lambda: fp.sinks_set_table(ids5, rows), lambda: fp.sinks_table(),
                     lambda: fp.sinks_density(pr.g_dens(), NGB), lambda: fp.blackhole_accretion(gp, _gacc(B, acc)),
                     lambda: fp.sfr_form_sinks(0, np.zeros(1), 1)):
            with pytest.raises(B.GhipError) as e:
                call()
            assert e.value.code == EINVAL and "shard" in str(e.value)
    finally:
        fp.close()
    assert L.ghip_device_bytes_in_use() == bytes0
