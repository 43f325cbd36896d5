"""numpy restatement of cooling_and_starformation with the cooling function and the dust drag heating
(sfr_eff.c:183-597, DoCooling cooling.c:82-300) and of the position part of FindQuasars
(blackhole.c:1481-1530), as the shipped flag bundle selects them (COOLING, SFR, DUST, BH_FORM,
FIND_SMBH, EVAPORATION_RADIAL, CONSTANT_MEAN_MOLECULAR_WEIGHT, BLACK_HOLES + BH_THERMALFEEDBACK),
with the sibling closed forms of DoCooling.  One particle at a time, in active-list order, op by op
in IEEE fp64 like the reference's C (math.pow is the C library's pow).

GAMMA = 7/5 (allvars.h:64); PROTONMASS = 1.6726e-24 (allvars.h:89); BOLTZMANN = 1.3806e-16
(allvars.h:84)."""
import math

import numpy as np

GAMMA_MINUS1 = 7.0 / 5.0 - 1
PROTONMASS = 1.6726e-24
BOLTZMANN = 1.3806e-16
NONE, ISOTHERM, EVAPORATION, EVAPORATION_RADIAL, BETA = 0, 1, 2, 3, 4


def params(**over):
    """ghip_sfr_params as a dict; defaults are the shipped parameter file's values (MeanWeight 2.45,
    BetaCool 5, EquilibriumTemp 20, Evap_dens 2e-11, Cool_ind 0.5, units of 100 AU and a solar mass,
    MinGasTemp 1; rho_cool_ind, absent from that file, 2) with EVAPORATION_RADIAL"""
    ul, um, uv = 1.496e15, 1.989e33, 297837.66
    ut = ul / uv
    p = dict(cooling=EVAPORATION_RADIAL, beta_tapper_off=0, dust=1, comoving=0, Timebase_interval=1e-6,
             Time=1.0, hubble_a=1.0, CritPhysDensity_code=1.0 * ul ** 3 / um, OriginalGasMass=1e-6,
             MeanWeight=2.45, UnitEnergy_in_cgs=um * ul ** 2 / ut ** 2, UnitMass_in_g=um,
             UnitDensity_in_cgs=um / ul ** 3, EqTemp=20.0, BetaCool=5.0, Cool_ind=0.5, rho_cool_ind=2.0,
             Evap_dens=2e-11, smbh_pos=(0.0, 0.0, 0.0))
    p["MinEgySpec"] = 1 / p["MeanWeight"] * (1.0 / GAMMA_MINUS1) * (BOLTZMANN / PROTONMASS) * 1.0 * \
        (um / p["UnitEnergy_in_cgs"])                                   # begrun.c:382-383, MinGasTemp 1
    p.update(over)
    return p


def u_to_temp(p):
    """cooling.c:104-105, sfr_eff.c:127"""
    return p["MeanWeight"] * PROTONMASS / BOLTZMANN * GAMMA_MINUS1 * p["UnitEnergy_in_cgs"] / p["UnitMass_in_g"]


def do_cooling(p, u_old, rho, dt, r2):
    """DoCooling(u_old, rho, dt, &ne, r2): rho the proper density, dt the step dtime"""
    c = p["cooling"]
    u2t = u_to_temp(p)
    if c == NONE:
        return u_old
    if c == ISOTHERM:                                                   # cooling.c:170-173
        return p["EqTemp"] / u2t
    if c == EVAPORATION:                                                # :175-183
        u_eq = p["EqTemp"] / u2t
        tcool = p["BetaCool"]
        tcool *= (1. + math.pow(rho * p["UnitDensity_in_cgs"] / p["Evap_dens"], 5))
    elif c == EVAPORATION_RADIAL:                                       # :185-192
        u_eq = p["EqTemp"] / u2t / (math.pow(math.sqrt(r2), p["Cool_ind"]) + 1e-10)
        tcool = p["BetaCool"]
        tcool *= (1. + math.pow(rho * p["UnitDensity_in_cgs"] / p["Evap_dens"], p["rho_cool_ind"]))
    elif c == BETA:                                                     # :196-198, 218-222, 282
        u_eq = p["EqTemp"] / u2t / (math.pow(math.sqrt(r2), 0.5) + 1.e-10)
        tcool = p["BetaCool"] * math.pow(math.sqrt(r2), 1.5)
        if p["beta_tapper_off"]:
            tcool *= (1. + math.pow(rho * p["UnitDensity_in_cgs"] / 1.e-10, 2))
    else:
        raise ValueError("unknown cooling variant %r" % c)
    return (u_old + u_eq * dt / tcool) / (1. + dt / tcool)


def sfr_cooling(p, active, ngas, ptype, pos, mass, timebin, density, entropy, dtentropy, injected,
                dragheat=None):
    """the loop of sfr_eff.c:183-597 over `active` (particle indices, list order).  Returns a dict of
    copies: dtentropy, mass, injected, dragheat (None unless dust) and cand (the sink candidates'
    indices in list order)."""
    mass = np.array(mass, np.float64)
    dte = np.array(dtentropy, np.float64)
    inj = np.array(injected, np.float64)
    dh = None if not p["dust"] else (np.zeros(ngas) if dragheat is None else np.array(dragheat, np.float64))
    u2t = u_to_temp(p)
    if p["comoving"]:                                                   # :145-156
        a3inv = 1 / (p["Time"] * p["Time"] * p["Time"])
        time_hubble_a = p["Time"] * p["hubble_a"]
    else:
        a3inv = time_hubble_a = 1
    xbh, ybh, zbh = p["smbh_pos"]
    cand = []
    for i in (int(v) for v in active):
        if ptype[i] == 2:                                               # :185-187
            if mass[i] <= 1.e-5 * p["OriginalGasMass"]:
                mass[i] = 0.
        if ptype[i] != 0 or i >= ngas:
            continue
        tb = int(timebin[i])
        dt = float((1 << tb) if tb else 0) * p["Timebase_interval"]
        dtime = p["Time"] * dt / time_hubble_a if p["comoving"] else dt
        dx, dy, dz = pos[i][0] - xbh, pos[i][1] - ybh, pos[i][2] - zbh   # :215-224, not wrapped
        r2 = dx * dx + dy * dy + dz * dz
        flag = 1
        if density[i] >= p["CritPhysDensity_code"]:                     # :226-229
            flag = 0
        if mass[i] == 0:                                                # :459-462
            flag = 1
        if flag == 0:
            cand.append(i)
            continue
        rho = density[i] * a3inv
        unew = (entropy[i] + dte[i] * dt) / GAMMA_MINUS1 * math.pow(rho, GAMMA_MINUS1)
        unew = p["MinEgySpec"] if p["MinEgySpec"] > unew else unew     # DMAX, :486-488
        if dh is not None and dh[i] and mass[i] != 0:                   # :481-499
            unew += dh[i] / mass[i] * dt
            dh[i] = 0.
        if inj[i]:                                                      # :502-524
            if mass[i] == 0:
                inj[i] = 0
            else:
                unew += inj[i] / mass[i]
            if u2t * unew > 5.0e9:
                unew = 5.0e9 / u2t
            inj[i] = 0
        unew = do_cooling(p, unew, rho, dtime, r2)
        if tb and dt > 0:                                               # :572-595
            d = (unew * GAMMA_MINUS1 / math.pow(rho, GAMMA_MINUS1) - entropy[i]) / dt
            if d < -0.5 * entropy[i] / dt:
                d = -0.5 * entropy[i] / dt
            dte[i] = d
    return dict(dtentropy=dte, mass=mass, injected=inj, dragheat=dh, cand=np.array(cand, np.int32))


def find_smbh(active, ptype, mass, pos, smbh_mass):
    """FindQuasars' position part: the last active Type 5 with Mass > 0.9 SMBHmass, and the count"""
    out, count = np.zeros(3), 0
    for i in (int(v) for v in active):
        if ptype[i] == 5 and mass[i] > 0.9 * smbh_mass:
            count += 1
            out = np.array(pos[i], np.float64)
    return out, count
