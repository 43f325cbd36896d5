"""The scalar bookkeeping of blackhole_accretion() and the BH_FORM conversion restated from the reference's
C text in numpy, one IEEE operation per C operation (no fused multiply-add, no reordering), for the flags
LIMITED_ACCRETION_AND_FEEDBACK + ACCRETION_RADIUS, ACCRETION_AT_EDDINGTON_RATE, ENFORCE_EDDINGTON_LIMIT,
BH_MASS_REAL, DUST.  Written from

    blackhole.c:119-286   the Mdot loop                          -> mdot_step()
    blackhole.c:679-735   the finish and the per-bin sums        -> finish()
    blackhole.c:70-791    the whole call, the two neighbour passes by tests/sink_ref.py (all pairs) -> accretion()
    sfr_eff.c:602-629     the conversion of a flagged gas particle into a sink              -> form_sinks()

No import of the oracle or of the library.  The per-sink state is a dict of arrays [nsink] in the order of the
sink list (the active Type-5 particles in active-list order): bh_mass, accdisc, mdot, dust_mass, total_mass.
Every function returns new arrays and the label of the branch each sink took:

    "dt0"       TimeBin == 0: dt = 0                      "clamp" / "noclamp"   the Eddington clamp taken / not
    "accreted"  BH_accreted_Mass > 0 / "not_accreted"     "mass0"  a sink of Mass == 0 (swallowed earlier)
    "limited" / "unlimited"  LIMITED_ACCRETION_AND_FEEDBACK on / off        "at_edd"  the at-Eddington form
"""
import types

import numpy as np

import sink_ref

STATE_KEYS = ("bh_mass", "accdisc", "mdot", "dust_mass", "total_mass")
BRANCHES = ("dt0", "clamp", "noclamp", "accreted", "not_accreted", "mass0", "limited", "unlimited", "at_edd")


def acc_params(limited_accretion=1, accretion_at_eddington_rate=0, enforce_eddington_limit=1, bh_mass_real=1,
               medd_fac=1.0, tvisc=0.0, EddingtonFactor=1.0):
    """the members of ghip_bh_accretion_params.  medd_fac = (4 pi GRAVITY C PROTONMASS / (0.1 C C THOMPSON)) *
    UnitTime_in_s (blackhole.c:149-159), tvisc = ViscousTimescale / UnitTime_in_s (:196)"""
    return types.SimpleNamespace(**locals())


def new_state(ns):
    return {k: np.zeros(ns) for k in STATE_KEYS}


def copy_state(st):
    return {k: np.array(st[k], np.float64) for k in STATE_KEYS}


def timestep(timebin, dt_fac):
    """dt = (TimeBin ? 1 << TimeBin : 0) * dt_fac (blackhole.c:124 with dt_fac = Timebase_interval / hubble_a)"""
    tb = np.asarray(timebin, np.int64)
    return np.where(tb != 0, (1 << tb).astype(np.float64), 0.0) * np.float64(dt_fac)


def mdot_step(state, mass, timebin, dt_fac, acc):
    """blackhole.c:119-286 for every sink of the list -> (state, branches [nsink] of sets)"""
    st = copy_state(state)
    mass = np.asarray(mass, np.float64)
    ns = len(mass)
    dt = timestep(timebin, dt_fac)
    br = [set() for _ in range(ns)]
    for a in range(ns):
        m = mass[a]
        medd = np.float64(acc.medd_fac) * (m if acc.bh_mass_real else st["bh_mass"][a])       # :149 / :158
        lim = np.float64(acc.EddingtonFactor) * medd
        mdot = np.float64(0.0)
        if dt[a] == 0:
            br[a].add("dt0")
        if m == 0:
            br[a].add("mass0")
        if acc.limited_accretion:
            br[a].add("limited")
            if not acc.accretion_at_eddington_rate:
                mdot = st["accdisc"][a] / (dt[a] + np.float64(acc.tvisc))                     # :196
                if acc.enforce_eddington_limit and mdot > lim:                                # :198-199
                    mdot = lim
                    br[a].add("clamp")
                else:
                    br[a].add("noclamp")
                st["accdisc"][a] = st["accdisc"][a] - mdot * dt[a]                            # :201
                st["bh_mass"][a] = st["bh_mass"][a] + mdot * dt[a]                            # :202
            else:
                br[a].add("at_edd")
                mdot = lim                                                                    # :205
                st["bh_mass"][a] = st["bh_mass"][a] + mdot * dt[a]                            # :206
        else:
            br[a].add("unlimited")
            if acc.enforce_eddington_limit and mdot > lim:                                    # :218-219
                mdot = lim
        st["mdot"][a] = mdot                                                                  # :237
    return st, br


def finish(state, vel, mass, timebin, acc_mass, acc_bhmass, acc_dustmass, acc_momentum, acc, dust):
    """blackhole.c:679-735: vel [nsink][3], mass [nsink] of the sinks -> (state, vel, mass, report, branches).
    report: dict(bin_mass, bin_dynmass, bin_mdot [32]) added in list order."""
    st = copy_state(state)
    vel = np.array(vel, np.float64)
    mass = np.array(mass, np.float64)
    ns = len(mass)
    br = [set() for _ in range(ns)]
    rep = dict(bin_mass=np.zeros(32), bin_dynmass=np.zeros(32), bin_mdot=np.zeros(32))
    for a in range(ns):
        am = np.float64(acc_mass[a])
        if am > 0:                                                                            # :691
            br[a].add("accreted")
            for k in range(3):
                vel[a, k] = (vel[a, k] * mass[a] + np.float64(acc_momentum[a][k])) / (mass[a] + am)   # :694-696
            mass[a] = mass[a] + am                                                            # :698
            st["bh_mass"][a] = st["bh_mass"][a] + np.float64(acc_bhmass[a])                   # :699
            if dust:
                st["dust_mass"][a] = st["dust_mass"][a] + np.float64(acc_dustmass[a])         # :701
            if acc.limited_accretion:
                st["accdisc"][a] = st["accdisc"][a] + am                                      # :705
                if acc.accretion_at_eddington_rate:
                    mass[a] = st["bh_mass"][a]                                                # :707
            if dust:
                st["total_mass"][a] = st["total_mass"][a] + am                                # :711
        else:
            br[a].add("not_accreted")
        b = int(timebin[a])
        rep["bin_mass"][b] += st["bh_mass"][a]                                                # :717-719
        rep["bin_dynmass"][b] += mass[a]
        rep["bin_mdot"][b] += st["mdot"][a]
    return st, vel, mass, rep, br


def accretion(pos, vel, mass, typ, ids, sinks, hsml, timebin, gas_density, bh_density, state, par, acc):
    """The whole of blackhole_accretion() for the sinks `sinks` (particle indices in active-list order), the
    marking pass and the swallow pass by tests/sink_ref.py over all pairs.  par: the members of ghip_bh_params.
    Nothing is modified.  Returns dict(state, vel [n][3], mass [n], sw, inj, swallow (sink_ref.swallow's dict),
    report (per-bin sums, counts), branches [nsink])."""
    sinks = np.asarray(sinks)
    vel, mass = np.array(vel, np.float64), np.array(mass, np.float64)
    st, br = mdot_step(state, mass[sinks], np.asarray(timebin)[sinks], par.dt_fac, acc)
    sw, inj = sink_ref.evaluate(pos, vel, mass, typ, ids, sinks, hsml, timebin, st["mdot"], bh_density,
                                gas_density, par)
    pbh = np.zeros(len(mass))
    pbh[sinks] = st["bh_mass"]
    so = sink_ref.swallow(pos, vel, mass, typ, ids, sinks, hsml, sw, pbh, par)
    st["bh_mass"] = so["bh_mass"][sinks].copy()          # P[j].BH_Mass = 0 of a swallowed sink (:1274)
    mass = so["mass"].copy()
    st, v5, m5, rep, br2 = finish(st, vel[sinks], mass[sinks], np.asarray(timebin)[sinks], so["acc_mass"],
                                  so["acc_bhmass"], so["acc_dustmass"], so["acc_momentum"], acc, par.dust)
    vel[sinks] = v5
    mass[sinks] = m5
    rep["counts"] = np.asarray(so["counts"], np.int64)
    return dict(state=st, vel=vel, mass=mass, sw=sw, inj=inj, swallow=so, report=rep,
                branches=[x | y for x, y in zip(br, br2)])


def form_sinks(cand, u01, mass, typ, timebin, limited_accretion):
    """sfr_eff.c:602-629 for the candidates `cand` (particle indices in active-list order), u01 [ncand] the
    gsl_rng_uniform draws in order -> dict(mass [n], type [n], rows: state of the new sinks in list order,
    stars_converted, sum_mass_stars, converted_in_bin [32])."""
    mass, typ = np.array(mass, np.float64), np.array(typ)
    cand = np.asarray(cand, np.int64)
    st = new_state(len(cand))
    out = dict(stars_converted=len(cand), sum_mass_stars=np.float64(0.0), converted_in_bin=np.zeros(32, np.int64))
    for k, i in enumerate(cand):
        out["sum_mass_stars"] = out["sum_mass_stars"] + mass[i]                               # :607
        typ[i] = 5                                                                            # :609
        mass[i] = mass[i] * (np.float64(0.995) + np.float64(0.005) * np.float64(u01[k]))      # :612
        if limited_accretion:
            st["accdisc"][k] = mass[i]                                                        # :622-623
        else:
            st["bh_mass"][k] = mass[i]                                                        # :615
        out["converted_in_bin"][int(timebin[i])] += 1                                         # :628
    out.update(mass=mass, type=typ, rows=st)
    return out
