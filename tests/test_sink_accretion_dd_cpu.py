"""CPU checks of the sinks on the resident state of shards (GHIP_DD_SINK_DENSITY / GHIP_DD_BH_SWALLOW begun with
walk = GHIP_SINKS_RESIDENT_FORM): the symbol and the struct the Python mirror assumes, the methods of the shard
drivers, and a numpy restatement of the sharded finish -- per-shard partial sums over a partition of the
particles, added in rank order from 0.0, then the finish of tests/sink_accretion_ref.py -- held to conservation
of mass and momentum within bounds derived from its roundings."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import sink_accretion_cases as AC
import sink_accretion_ref as AR
import sink_ref
from common import REPO, SINK_PAIR_AT, bindings, pkg, sink_case

EPS = 2.0 ** -52
LD = np.longdouble
SLACK = 1.001             # the check's own long-double sums


def test_libghip_exports_the_args_size():
    L = C.CDLL(pkg.lib_path())
    B = bindings()
    assert hasattr(L, "ghip_dd_sinks_args_size") and "ghip_dd_sinks_args_size" in B.EXPORTS
    B.lib()
    L.ghip_dd_sinks_args_size.restype = C.c_size_t
    assert L.ghip_dd_sinks_args_size() == C.sizeof(B.DdSinksArgs)
    assert B.SINKS_RESIDENT_FORM == 1


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ghip.h"
int main(void)
{
  printf("%zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(ghip_dd_sinks_args), offsetof(ghip_dd_sinks_args, dens),
         offsetof(ghip_dd_sinks_args, ngb_factor), offsetof(ghip_dd_sinks_args, iterations),
         offsetof(ghip_dd_sinks_args, bh), offsetof(ghip_dd_sinks_args, acc), offsetof(ghip_dd_sinks_args, report),
         (int) GHIP_SINKS_RESIDENT_FORM);
  return 0;
}
"""


def test_struct_layout_matches_the_header(tmp_path):
    B = bindings()
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=gnu99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    A = B.DdSinksArgs
    assert got == [C.sizeof(A), A.dens.offset, A.ngb_factor.offset, A.iterations.offset, A.bh.offset, A.acc.offset,
                   A.report.offset, B.SINKS_RESIDENT_FORM]
    args, keep = B.dd_sinks_args(dens=B.DensParams(), ngb_factor=1.5, bh=B.BhParams(), acc=B.BhAccretionParams())
    assert args.ngb_factor == 1.5 and args.iterations and args.report and args.dens and args.bh and args.acc
    assert set(B.dd_sinks_report(keep)) == {"bin_mass", "bin_dynmass", "bin_mdot", "counts", "nactive"}


def test_the_shard_drivers_have_the_pair():
    sh = importlib.import_module("gadget-leicester_amd.sharded")
    for cls in (sh.DomainShards, sh.DomainRank):
        for name in ("sinks_density", "blackhole_accretion"):
            assert callable(getattr(cls, name, None)), (cls.__name__, name)


# ------------------------------------------------------------------------------------------------
# the sharded finish, restated
# ------------------------------------------------------------------------------------------------
def _only(typ, part, r):
    """the particle types as shard r sees its candidates: a particle of another shard is none (Type 1)"""
    return np.where(part == r, typ, 1)


def sharded_accretion(sp, switches, state, acc, part, nparts):
    """blackhole_accretion() as GHIP_DD_BH_SWALLOW runs it in its resident form, on the partition `part` [n] of
    the particles into nparts shards: the Mdot step per sink; the marking pass of every shard over its own
    particles (a victim is local to one shard, which sees every claim); the sweep of every shard over its own
    particles; the partial planes added in ascending rank order from 0.0 with plain adds; the finish."""
    ic, pr, d = sp.pr.ic, sp.pr, sp.dens
    par = AC.ref_par(sp, switches)
    sk = sp.sinks
    pos, vel, mass, typ = ic["pos"], ic["vel"], ic["mass"], ic["type"]
    st, _ = AR.mdot_step(state, mass[sk], pr.timebin[sk], par.dt_fac, acc)
    sw = np.zeros(pr.n, np.uint32)
    for r in range(nparts):
        s, _ = sink_ref.evaluate(pos, vel, mass, _only(typ, part, r), sp.ids, sk, d["hsml"], pr.timebin, st["mdot"],
                                 d["density"], sp.gas_density, par)
        assert not s[part != r].any()
        sw = np.maximum(sw, s)
    pbh = np.zeros(pr.n)
    pbh[sk] = st["bh_mass"]
    ns = len(sk)
    tot = dict(acc_mass=np.zeros(ns), acc_bhmass=np.zeros(ns), acc_dustmass=np.zeros(ns),
               acc_momentum=np.zeros((ns, 3)))
    counts = np.zeros(3, np.int64)
    swallowed = np.zeros(pr.n, bool)
    for r in range(nparts):                                  # ascending rank order, from 0.0
        so = sink_ref.swallow(pos, vel, mass, _only(typ, part, r), sp.ids, sk, d["hsml"], sw, pbh, par)
        for k in tot:
            tot[k] = tot[k] + so[k]
        counts += so["counts"]
        swallowed |= so["swallowed"]
    mass1 = np.where(swallowed, 0.0, mass)
    st["bh_mass"] = np.where(swallowed[sk], 0.0, st["bh_mass"])
    st, v5, m5, rep, _ = AR.finish(st, vel[sk], mass1[sk], pr.timebin[sk], tot["acc_mass"], tot["acc_bhmass"],
                                   tot["acc_dustmass"], tot["acc_momentum"], acc, par.dust)
    vel1 = vel.copy()
    vel1[sk], mass1[sk] = v5, m5
    return dict(state=st, vel=vel1, mass=mass1, sw=sw, swallowed=swallowed, counts=counts, sums=tot, report=rep)


def _ldsum(x):
    return np.sum(np.asarray(x, np.float64).astype(LD), dtype=LD)


def _partitions(n, nparts, seed):
    rng = np.random.default_rng(seed)
    yield "blocks", (np.arange(n) * nparts // n).astype(np.int64)
    yield "dealt", (np.arange(n) % nparts).astype(np.int64)
    yield "random", rng.integers(0, nparts, n)


@pytest.mark.parametrize("nparts", [1, 3, 8])
def test_the_sharded_finish_conserves_mass_and_momentum(nparts):
    """{sinks + swallowed victims} before and after, for any partition into P shards.

    Mass.  A swallowing sink's new mass is fl(M + s), s the rank-ordered sum of P partial sums, each rounded once
    from its exact value (tests/sink_ref.py adds in long double): P roundings of the partials, P - 1 of the chain
    (the first add, to 0.0, is exact), one of M + s -- 2 P roundings of at most half an ulp of numbers no larger
    than the new mass: P ulp(M') <= P EPS M' per sink, P EPS x the total.  (P = 1: the bound of
    tests/test_sink_accretion_cpu.py.)

    Momentum, per component.  As there, with p the rank-ordered sum: half an ulp each of v M, of every m_j v_j,
    of the sum b = fl(v M) + p and of the quotient, and now 2 P - 1 roundings in p (P partials, P - 1 adds) where
    one stood, each at most half an ulp of a number no larger than sum |m_j v_j|:
    (EPS / 2) (|v M| + 2 P sum |m_j v_j| + 2 |b|) <= (P + 1.5) EPS (|v M| + sum |m_j v_j|)."""
    sp = AC.stock(1)
    st = AC.state_for(sp)
    acc = AC.acc_for(sp, st)
    ic = sp.pr.ic
    one = None
    for name, part in _partitions(sp.pr.n, nparts, 40 + nparts):
        r = sharded_accretion(sp, (0, 0), st, acc, part, nparts)
        if one is None:
            one = sharded_accretion(sp, (0, 0), st, acc, np.zeros(sp.pr.n, np.int64), 1)
            whole = AR.accretion(ic["pos"], ic["vel"], ic["mass"], ic["type"], sp.ids, sp.sinks, sp.dens["hsml"],
                                 sp.pr.timebin, sp.gas_density, sp.dens["density"], st, AC.ref_par(sp, (0, 0)), acc)
            # one shard is the single-GPU call
            assert np.array_equal(one["mass"], whole["mass"]) and np.array_equal(one["vel"], whole["vel"])
            assert np.array_equal(one["sw"], whole["sw"])
        # the partition decides nothing: the same marks, the same victims, the same counts
        assert np.array_equal(r["sw"], one["sw"]) and np.array_equal(r["swallowed"], one["swallowed"])
        assert np.array_equal(r["counts"], one["counts"]) and r["swallowed"].sum() > 10
        S = np.union1d(sp.sinks, np.where(r["swallowed"])[0])
        m0, m1 = ic["mass"][S], r["mass"][S]
        M0, M1 = _ldsum(m0), _ldsum(m1)
        print(nparts, name, "mass", float(abs(M1 - M0) / M0))
        assert abs(M1 - M0) <= SLACK * nparts * EPS * max(M0, M1)
        assert not r["mass"][r["swallowed"]].any()
        for k in range(3):
            p0 = np.sum(m0.astype(LD) * ic["vel"][S, k].astype(LD), dtype=LD)
            p1 = np.sum(m1.astype(LD) * r["vel"][S, k].astype(LD), dtype=LD)
            scale = np.sum(np.abs(m0.astype(LD) * ic["vel"][S, k].astype(LD)), dtype=LD)
            print(nparts, name, "momentum", k, float(abs(p1 - p0) / scale))
            assert abs(p1 - p0) <= SLACK * (nparts + 1.5) * EPS * scale
        rest = np.setdiff1d(np.arange(sp.pr.n), S)
        assert np.array_equal(r["mass"][rest], ic["mass"][rest]) and np.array_equal(r["vel"][rest], ic["vel"][rest])


def test_the_partition_does_not_change_the_marks_of_the_pair():
    """two sinks that claim each other, with victims on other shards than themselves: whatever the partition,
    the marks are those of one shard, and neither sink swallows"""
    sp = sink_case("pair", 1, at=SINK_PAIR_AT)
    st = AC.state_for(sp)
    acc = AC.acc_for(sp, st)
    one = sharded_accretion(sp, (1, 1), st, acc, np.zeros(sp.pr.n, np.int64), 1)
    assert (one["sw"] > 0).sum() >= 6 and np.all(one["sw"][sp.sinks] > 0)
    for nparts in (3, 8):
        for name, part in _partitions(sp.pr.n, nparts, 7):
            r = sharded_accretion(sp, (1, 1), st, acc, part, nparts)
            assert np.array_equal(r["sw"], one["sw"]), (nparts, name)
            assert not r["counts"].any() and np.array_equal(r["mass"], sp.pr.ic["mass"])
            for g in sp.sinks:      # each sink's victims do not all lie with it
                marked = np.where(r["sw"] == sp.ids[g])[0]
                assert name == "blocks" or (part[marked] != part[g]).any()
