"""CPU checks of the sinks on the resident state (ghip_sinks_*, ghip_blackhole_accretion, ghip_sfr_form_sinks):
the symbols are exported and the structs have the sizes their Python mirrors assume, and the numpy restatement
the GPU tests compare against (tests/sink_accretion_ref.py: blackhole.c:119-286, 679-747, sfr_eff.c:602-629) is
pinned by what must hold of it -- conservation of mass and momentum, the disc + hole = mass invariant, the
branches its inputs reach, the rules of the conversion."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sink_accretion_cases as AC
import sink_accretion_ref as AR
from common import REPO, bindings, pkg, sink_case

EPS = 2.0 ** -52          # one ulp of a number in [1, 2): ulp(x) <= EPS |x|
LD = np.longdouble
SLACK = 1.001             # the check's own long-double sums (2^-64 relative each)


def test_libghip_exports_the_resident_sink_entry_points():
    L = C.CDLL(pkg.lib_path())
    B = bindings()
    for name in ("ghip_sinks_set_table", "ghip_sinks_get_table", "ghip_sinks_clear", "ghip_sinks_density",
                 "ghip_blackhole_accretion", "ghip_sfr_form_sinks"):
        assert hasattr(L, name), name
        assert name in B.EXPORTS
    B.lib()   # argtypes of every export resolve
    for name in ("sinks_set_table", "sinks_table", "sinks_density", "blackhole_accretion", "sfr_form_sinks"):
        assert hasattr(B.ForcePath, name), name


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ghip.h"
int main(void)
{
  printf("%d %zu %zu %zu %zu %zu %zu\n", (int) GHIP_SK_COUNT, sizeof(ghip_bh_accretion_params),
         offsetof(ghip_bh_accretion_params, medd_fac), sizeof(ghip_bh_accretion_report),
         offsetof(ghip_bh_accretion_report, swallowed), sizeof(ghip_sfr_form_report),
         offsetof(ghip_sfr_form_report, converted_in_bin));
  printf("%d %d %d %d %d\n", (int) GHIP_SK_BH_DENSITY, (int) GHIP_SK_GASVEL, (int) GHIP_SK_NUMNGB,
         (int) GHIP_SK_ACC_MASS, (int) GHIP_SK_ACC_MOMENTUM);
  return 0;
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    B = bindings()
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=gnu99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    a, b = subprocess.check_output([str(exe)]).decode().splitlines()
    assert [int(x) for x in a.split()] == [
        B.SK_COUNT, C.sizeof(B.BhAccretionParams), B.BhAccretionParams.medd_fac.offset,
        C.sizeof(B.BhAccretionReport), B.BhAccretionReport.swallowed.offset, C.sizeof(B.SfrFormReport),
        B.SfrFormReport.converted_in_bin.offset]
    assert [int(x) for x in b.split()] == [B.SK_BH_DENSITY, B.SK_GASVEL, B.SK_NUMNGB, B.SK_ACC_MASS,
                                           B.SK_ACC_MOMENTUM]
    assert B.SK_COUNT == 17


def _run(sp, switches, state, acc, mass=None, vel=None):
    ic, d = sp.pr.ic, sp.dens
    return AR.accretion(ic["pos"], ic["vel"] if vel is None else vel, ic["mass"] if mass is None else mass,
                        ic["type"], sp.ids, sp.sinks, d["hsml"], sp.pr.timebin, sp.gas_density, d["density"],
                        state, AC.ref_par(sp, switches), acc)


def _ldsum(x):
    return np.sum(np.asarray(x, np.float64).astype(LD), dtype=LD)


_INPUTS = {}


def _input(name):
    if name not in _INPUTS:
        _INPUTS[name] = sink_case("clump", 1) if name == "clump" else AC.stock(1)
    return _INPUTS[name]


@pytest.mark.parametrize("name", ["stock", "clump"])
def test_mass_and_momentum_of_sinks_and_victims_are_conserved(name):
    """{sinks + swallowed victims} before and after one call (shipped setting: limited accretion, not at the
    Eddington rate, where Mass is only ever added to).

    Mass.  A swallowing sink's new mass is fl(M + fl(sum of the victims' masses)): the sum is rounded once
    (tests/sink_ref.py adds in long double), the addition once -- two roundings of at most half an ulp of a
    number no larger than the new mass, so at most 1 ulp(M') <= EPS M' per sink and EPS x the total over all.

    Momentum, per component.  The sink's new momentum is v' M' with v' = fl(fl(fl(v M) + p) / M'), p = fl(sum of
    fl(m_j v_j)).  M' cancels; what remains is half an ulp each of v M, of every m_j v_j, of p, of the sum
    b = fl(v M) + p and of the quotient, i.e. at most (EPS / 2) (|v M| + 2 sum |m_j v_j| + 2 |b|) <=
    2.5 EPS (|v M| + sum |m_j v_j|): 2.5 EPS x the sum of |m v| over the set."""
    sp = _input(name)
    st = AC.state_for(sp)
    r = _run(sp, (0, 0), st, AC.acc_for(sp, st))
    ic = sp.pr.ic
    S = np.union1d(sp.sinks, np.where(r["swallow"]["swallowed"])[0])
    assert r["swallow"]["swallowed"].sum() > 10 and (r["swallow"]["acc_mass"] > 0).sum() >= 2
    m0, m1 = ic["mass"][S], r["mass"][S]
    M0, M1 = _ldsum(m0), _ldsum(m1)
    print(name, "mass", float(abs(M1 - M0) / M0))
    assert abs(M1 - M0) <= SLACK * EPS * max(M0, M1)
    assert np.all(r["mass"][np.where(r["swallow"]["swallowed"])[0]] == 0)
    for k in range(3):
        p0 = np.sum(m0.astype(LD) * ic["vel"][S, k].astype(LD), dtype=LD)
        p1 = np.sum(m1.astype(LD) * r["vel"][S, k].astype(LD), dtype=LD)
        scale = np.sum(np.abs(m0.astype(LD) * ic["vel"][S, k].astype(LD)), dtype=LD)
        print(name, "momentum", k, float(abs(p1 - p0) / scale))
        assert abs(p1 - p0) <= SLACK * 2.5 * EPS * scale
    # nobody outside the set was touched
    rest = np.setdiff1d(np.arange(sp.pr.n), S)
    assert np.array_equal(r["mass"][rest], ic["mass"][rest]) and np.array_equal(r["vel"][rest], ic["vel"][rest])


def test_disc_plus_hole_stays_the_mass_without_mergers():
    """Sinks formed under LIMITED_ACCRETION_AND_FEEDBACK (AccDisc_Mass = Mass, BH_Mass = 0) through three calls
    on an input without sink-sink mergers (asserted: a merger adds the victim's mass to the disc AND its BH_Mass
    to the hole).  e = AccDisc_Mass + BH_Mass - Mass starts at 0; per call the Mdot step rounds AccDisc - x and
    BH + x (the same x = fl(mdot dt) in both), the finish rounds AccDisc + a and Mass + a: four roundings of at
    most half an ulp of numbers no larger than the mass, 2 EPS Mass per call."""
    sp = _input("stock")
    ic = sp.pr.ic
    st = AR.new_state(len(sp.sinks))
    st["accdisc"] = ic["mass"][sp.sinks].copy()
    st["total_mass"] = ic["mass"][sp.sinks].copy()
    acc = AC.acc_for(sp, st)
    mass, vel = ic["mass"], ic["vel"]
    grown = 0
    for call in range(1, 4):
        r = _run(sp, (0, 0), st, acc, mass=mass, vel=vel)
        assert r["report"]["counts"][1] == 0, "the input has a sink-sink merger"
        st, mass, vel = r["state"], r["mass"], r["vel"]
        m = mass[sp.sinks]
        e = np.abs(st["accdisc"].astype(LD) + st["bh_mass"].astype(LD) - m.astype(LD))
        print(call, float((e / m).max()))
        assert np.all(e <= SLACK * 2 * call * EPS * m)
        grown += int((r["swallow"]["acc_mass"] > 0).sum())
    assert grown >= 2 and np.all(st["bh_mass"] > 0)


def test_the_mdot_step_alone_conserves_disc_plus_hole():
    """AccDisc_Mass - x and BH_Mass + x with the same x: two roundings, at most half an ulp each of numbers no
    larger than the sum, so 1 ulp: EPS x (AccDisc_Mass + BH_Mass).  Mass and the other columns are not written."""
    for name in ("stock", "clump"):
        sp = _input(name)
        st = AC.state_for(sp)
        m, tb = sp.pr.ic["mass"][sp.sinks], sp.pr.timebin[sp.sinks]
        st1, br = AR.mdot_step(st, m, tb, sp.par["dt_fac"], AC.acc_for(sp, st))
        s0 = st["accdisc"].astype(LD) + st["bh_mass"].astype(LD)
        s1 = st1["accdisc"].astype(LD) + st1["bh_mass"].astype(LD)
        assert np.all(np.abs(s1 - s0) <= SLACK * EPS * s0)
        moved = st1["bh_mass"] > st["bh_mass"]
        dt0 = np.array(["dt0" in b for b in br])
        assert moved.any() and np.array_equal(st1["dust_mass"], st["dust_mass"])
        assert np.array_equal(st1["accdisc"][dt0], st["accdisc"][dt0])      # dt == 0: nothing flows
        assert np.all(st1["mdot"][~dt0 & (st["accdisc"] > 0)] > 0)


def test_the_inputs_reach_every_branch():
    """the union over the runs the GPU tests make: a generator that stops reaching a branch fails here"""
    got = set()
    clump, stock = _input("clump"), _input("stock")
    st = AC.state_for(clump)
    r = _run(clump, (0, 0), st, AC.acc_for(clump, st))
    shipped = set().union(*r["branches"])
    assert {"dt0", "clamp", "noclamp", "accreted", "not_accreted", "mass0", "limited"} <= shipped, shipped
    got |= shipped
    st = AC.state_for(stock)
    r = _run(stock, (0, 0), st, AC.acc_for(stock, st))
    assert {"clamp", "noclamp", "accreted", "not_accreted"} <= set().union(*r["branches"])
    for over in (dict(limited_accretion=0), dict(accretion_at_eddington_rate=1)):
        r = _run(stock, (0, 0), st, AC.acc_for(stock, st, **over))
        got |= set().union(*r["branches"])
        if "accretion_at_eddington_rate" in over:      # :706-708: Mass = BH_Mass where something was accreted
            took = np.array(["accreted" in b for b in r["branches"]])
            assert took.any() and np.array_equal(r["mass"][stock.sinks][took], r["state"]["bh_mass"][took])
        else:
            assert not r["state"]["mdot"].any() and np.array_equal(r["state"]["accdisc"], st["accdisc"])
    assert got == set(AR.BRANCHES), set(AR.BRANCHES) - got


def test_formation():
    sp = _input("stock")
    pr = sp.pr
    rng = np.random.default_rng(8)
    cand = rng.permutation(pr.ngas)[:40]
    u01 = rng.random(40)
    u01[0], u01[1] = 0.0, (2.0 ** 32 - 1) / 2.0 ** 32      # the ends of gsl_rng_uniform's range [0, 1)
    mass, typ = pr.ic["mass"], pr.ic["type"]
    for limited in (1, 0):
        f = AR.form_sinks(cand, u01, mass, typ, pr.timebin, limited)
        ratio = f["mass"][cand] / mass[cand]
        assert np.all(f["mass"][cand] >= 0.995 * mass[cand]) and np.all(f["mass"][cand] < mass[cand])
        assert f["mass"][cand[0]] == 0.995 * mass[cand[0]]
        # the k-th candidate gets u01[k]: the draws are distinct, so are the ratios, in the same order
        assert np.array_equal(np.argsort(ratio), np.argsort(u01))
        assert np.array_equal(f["mass"][cand], mass[cand] * (0.995 + 0.005 * u01))
        assert np.all(f["type"][cand] == 5) and np.all(typ[cand] == 0)
        rest = np.setdiff1d(np.arange(pr.n), cand)
        assert np.array_equal(f["mass"][rest], mass[rest]) and np.array_equal(f["type"][rest], typ[rest])
        full, empty = ("accdisc", "bh_mass") if limited else ("bh_mass", "accdisc")
        assert np.array_equal(f["rows"][full], f["mass"][cand]) and not f["rows"][empty].any()
        assert f["stars_converted"] == 40 and f["converted_in_bin"].sum() == 40
        assert np.array_equal(f["converted_in_bin"], np.bincount(pr.timebin[cand], minlength=32))
        assert abs(f["sum_mass_stars"] - mass[cand].sum()) <= 40 * EPS * mass[cand].sum()
    f = AR.form_sinks(np.zeros(0, np.int64), np.zeros(0), mass, typ, pr.timebin, 1)
    assert np.array_equal(f["mass"], mass) and np.array_equal(f["type"], typ)
    assert f["stars_converted"] == 0 and f["sum_mass_stars"] == 0 and not f["converted_in_bin"].any()
