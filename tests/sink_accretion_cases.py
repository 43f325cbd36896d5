"""Inputs of the resident sink tests (tests/test_sink_accretion_cpu.py, tests/test_gpu_sink_accretion.py) on top
of the generators of tests/common.py: the per-sink state that goes into the sink table, and parameters of the
Mdot step chosen -- on the CPU, from the inputs alone -- so that about half of the sinks take the Eddington
clamp."""
import numpy as np

import sink_accretion_ref as AR
from common import SinkProblem, sink_over, sink_ref_density, sink_ref_par

NGB_FACTOR = 1.5


def stock(periodic=1, seed=5):
    """SinkProblem(ng=10, nsink=8, ndust=300) with what the marking pass reads besides: sp.gas_density, and
    sp.dens, the density pass of tests/sink_ref.py"""
    sp = SinkProblem(ng=10, periodic=periodic, nsink=8, ndust=300, seed=seed)
    sp.gas_density = 0.5 + np.random.default_rng(3).random(sp.pr.ngas)
    sp.dens = sink_ref_density(sp)
    return sp


def state_for(sp, seed=1):
    """the state of sp.sinks, in list order: BH_Mass as the generator has it, a disc of 10 to 90 % of the mass"""
    rng = np.random.default_rng(seed)
    m = sp.pr.ic["mass"][sp.sinks]
    ns = len(m)
    st = AR.new_state(ns)
    st["bh_mass"] = sp.bh_mass[sp.sinks].copy()
    st["accdisc"] = (0.1 + 0.8 * rng.random(ns)) * m
    st["dust_mass"] = 0.01 * rng.random(ns) * m
    st["total_mass"] = m.copy()
    return st


def acc_for(sp, state, **over):
    """tvisc = the median step; EddingtonFactor * medd_fac = the median of the unclamped mdot / Mass over the
    sinks with mass: those above it clamp, those below do not"""
    m = sp.pr.ic["mass"][sp.sinks]
    dt = AR.timestep(sp.pr.timebin[sp.sinks], sp.par["dt_fac"])
    tvisc = float(np.median(dt[dt > 0]))
    ok = m > 0
    q = state["accdisc"][ok] / (dt[ok] + tvisc) / m[ok]
    return AR.acc_params(**{**dict(medd_fac=float(np.median(q)), tvisc=tvisc, EddingtonFactor=1.0), **over})


def rows_of(B, state, dens=None):
    """rows [nsink][SK_COUNT] of the sink table from a state (and, where given, the density results)"""
    ns = len(state["bh_mass"])
    rows = np.zeros((ns, B.SK_COUNT))
    rows[:, B.SK_BH_MASS] = state["bh_mass"]
    rows[:, B.SK_ACCDISC_MASS] = state["accdisc"]
    rows[:, B.SK_BH_MDOT] = state["mdot"]
    rows[:, B.SK_DUST_MASS] = state["dust_mass"]
    rows[:, B.SK_TOTAL_MASS] = state["total_mass"]
    if dens is not None:
        rows[:, B.SK_BH_DENSITY] = dens["density"]
        rows[:, B.SK_BH_ENTROPY] = dens["entropy"]
        rows[:, B.SK_GASVEL:B.SK_GASVEL + 3] = dens["gasvel"]
        rows[:, B.SK_NUMNGB] = dens["numngb"]
    return rows


def ref_par(sp, switches):
    return sink_ref_par(sp, **sink_over(*switches))
