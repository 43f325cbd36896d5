"""The creation of wind particles by the massive sinks, momentum_feedback.c:70-246 (-DVIRTUAL -DFB_MOMENTUM),
restated in numpy / Python floats op by op: every product, quotient and sum in the C text's order, one IEEE
double rounding each, acos / sin / cos from the platform's libm.  It reads nothing outside tests/.

The compile-time switches of the C text are keys of the parameter dict: fraction_of_ledd_feedback,
accretion_at_eddington_rate (read under the former), startup_luminosity, isotropic, accretion_radius,
fly_through_empty_space.  The term of :193 is multiplied by 0. and is left out; its three gsl draws per particle
are counted (gsl_draws).  force_add_star_to_tree (:230) and the time-bin lists (:202-213) are the caller's."""
import math

import numpy as np

C_LIGHT = 2.9979e10         # allvars.h:86
GRAVITY = 6.672e-8          # allvars.h:79
PROTONMASS = 1.6726e-24     # allvars.h:89
THOMPSON = 6.65245e-25      # allvars.h:91

# columns of a wind row (GHIP_WK_*)
(WK_STELLAR_AGE, WK_BIRTH_ENERGY, WK_OLD_MOMENTUM, WK_NEW_DENSITY, WK_DRMIN, WK_DT1, WK_DT2, WK_DT_JUMP,
 WK_DELTA_MOMENTUM, WK_DELETED, WK_COUNT) = range(11)


def params(**over):
    p = dict(Time=1.0, dt_fac=1e-3, SMBHmass=1.0, VirtualStart=0.0, VirtualFeedBack=1.0, VirtualMomentum=1e-3,
             VirtualMass=1e-3, FeedBackVelocity=1.0, UnitVelocity_in_cm_per_s=2.9979e10 / 50.0, UnitTime_in_s=3.0e10,
             SofteningBndryMaxPhys=0.01, InnerBoundary=0.02, NumCurrentTiStep=7, MaxPart=1 << 30,
             fraction_of_ledd_feedback=1, accretion_at_eddington_rate=0, startup_luminosity=0, isotropic=0,
             accretion_radius=1, fly_through_empty_space=1)
    p.update(over)
    return p


def l_edd_dimensionless(par):
    """:36-37 (pow(x, 2) is x * x)"""
    u = float(par["UnitVelocity_in_cm_per_s"])
    return (4 * math.pi * GRAVITY * C_LIGHT * PROTONMASS / THOMPSON) / (u * u) * float(par["UnitTime_in_s"])


def energy_wind_min(par):
    """:39"""
    return float(par["VirtualMomentum"]) * C_LIGHT / float(par["UnitVelocity_in_cm_per_s"])


def count(par, mass, timebin, bh_mass, bh_mdot):
    """:75-133 for one sink -> None if it does not count, else (dt, new_wind_exact, new_wind, correction_wind)"""
    mass, bh_mass, bh_mdot = float(mass), float(bh_mass), float(bh_mdot)
    if not (mass > 0.5 * float(par["SMBHmass"]) and float(par["Time"]) > float(par["VirtualStart"])):
        return None
    tb = int(timebin)
    dt = float((1 << tb) if tb else 0) * float(par["dt_fac"])
    vfb, ledd, ewm = float(par["VirtualFeedBack"]), l_edd_dimensionless(par), energy_wind_min(par)
    if par["fraction_of_ledd_feedback"]:
        m = bh_mass if par["accretion_at_eddington_rate"] else mass
        exact = vfb * ledd * m * dt / ewm
    else:
        cu = C_LIGHT / float(par["UnitVelocity_in_cm_per_s"])
        lum = vfb * 0.1 * bh_mdot * (cu * cu)
        if lum > ledd * mass:
            lum = ledd * mass
        exact = vfb * lum * dt / ewm
    if (exact > 1.e-4) if par["startup_luminosity"] else (exact > 0.):
        new_wind = int(exact) + 1
    else:
        new_wind = 0
    corr = exact / new_wind if new_wind > 0 else 1.
    return dt, exact, new_wind, corr


def direction(par, sink_id, bits, rnd):
    """:168-177 -> (dir[3], theta, phi)"""
    nrnd = len(rnd)
    step = int(par["NumCurrentTiStep"]) & 0xffffffff
    r1 = float(rnd[((int(sink_id) + 2 + bits + step) & 0xffffffff) % nrnd])
    r2 = float(rnd[((int(sink_id) + 3 + bits + step) & 0xffffffff) % nrnd])
    theta = math.acos(2. * r1 - 1.) if par["isotropic"] else math.acos(0.5 * r1 + 0.5)
    phi = 2 * math.pi * (r2 + float(par["Time"]))
    return [math.sin(theta) * math.cos(phi), math.sin(theta) * math.sin(phi), math.cos(theta)], theta, phi


def spawn(par, n, sinks, mass, timebin, hsml, ids, bh_mass, bh_mdot, bh_density, rnd):
    """The loop over the active sinks `sinks` (particle indices in active-list order) of a state of n particles.
    mass, timebin, hsml, ids: per particle; bh_mass, bh_mdot, bh_density: per listed sink.  Returns
      parent [total] (the sink each new particle copies, :158), bits [total], and of the new particles hsml, vel
      [total][3], dir [total][3], phi, id (uint32), mass, rows [total][WK_COUNT]; sink_mass: {sink: Mass after
      :89}; report: spawned, nsinks_emitting, first_index, new_wind_exact_sum, gsl_draws"""
    ewm = energy_wind_min(par)
    u, fbv = float(par["UnitVelocity_in_cm_per_s"]), float(par["FeedBackVelocity"])
    out = dict(parent=[], bits=[], hsml=[], vel=[], dir=[], phi=[], id=[], mass=[], rows=[], sink_mass={})
    rep = dict(spawned=0, nsinks_emitting=0, first_index=int(n), new_wind_exact_sum=0.0, gsl_draws=0)
    for a, i in enumerate(sinks):
        c = count(par, mass[i], timebin[i], bh_mass[a], bh_mdot[a])
        if c is None:
            continue
        dt, exact, new_wind, corr = c
        if par["fraction_of_ledd_feedback"] and par["accretion_at_eddington_rate"]:
            out["sink_mass"][int(i)] = float(bh_mass[a])     # :89
        if new_wind == 0:
            continue
        rep["nsinks_emitting"] += 1
        rep["new_wind_exact_sum"] += exact
        for bits in range(new_wind):
            j = n + rep["spawned"]
            if j >= par["MaxPart"]:
                raise OverflowError("endrun(8888): NumPart=%d, spawned %d, MaxPart=%d" % (n, rep["spawned"], par["MaxPart"]))
            h = float(hsml[i])
            h += float(par["SofteningBndryMaxPhys"])
            if par["accretion_radius"]:
                h += float(par["InnerBoundary"])
            d, theta, phi = direction(par, ids[i], bits, rnd)
            old = ewm / C_LIGHT * u * corr                   # :225
            birth = ewm * corr                               # :226
            row = np.zeros(WK_COUNT)
            row[WK_STELLAR_AGE] = float(par["Time"])
            row[WK_BIRTH_ENERGY] = birth
            row[WK_OLD_MOMENTUM] = old
            row[WK_DRMIN] = 0. if par["fly_through_empty_space"] else float(bh_density[a])
            row[WK_DT1] = dt
            out["parent"].append(int(i))
            out["bits"].append(bits)
            out["hsml"].append(h)
            out["vel"].append([C_LIGHT / u * d[k] / fbv for k in range(3)])     # :191
            out["dir"].append(d)
            out["phi"].append(phi)
            out["id"].append((int(ids[i]) + j) & 0xffffffff)                    # :215
            out["mass"].append(float(par["VirtualMass"]) * old)                 # :228
            out["rows"].append(row)
            rep["spawned"] += 1
    rep["gsl_draws"] = 3 * rep["spawned"]
    t = rep["spawned"]
    out["parent"] = np.array(out["parent"], np.int64)
    out["bits"] = np.array(out["bits"], np.int64)
    out["id"] = np.array(out["id"], np.uint32)
    for k in ("hsml", "phi", "mass"):
        out[k] = np.array(out[k], np.float64)
    for k in ("vel", "dir"):
        out[k] = np.array(out[k], np.float64).reshape(t, 3)
    out["rows"] = np.array(out["rows"], np.float64).reshape(t, WK_COUNT)
    out["report"] = rep
    return out
