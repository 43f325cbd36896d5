"""Independent numpy restatement of the physics switches of the reference's dust passes that
ghip_set_dust_model turns on (dust.c: DUST_REAL_PEBBLE_COLLISIONS :851-853, 479-490; DUST_EPSTEIN :415-416;
DUST_NO_FRICTION_HEATING :433-435; DUST_GROWTH :451-495, 551, 565-568; DUST_VAPORIZE :498-549, 590-609;
DUST_FE_AND_ICE_GRAINS :509-547, 596-605), with brute-force neighbour search.  Built on dust_ref.py; nothing
here imports the product.

Kept as the reference has them: t_coll uses the FINAL DustVcoll of the call (the value of :374 is overwritten
at :437-444 whenever dt > 0); the clamp to [0.1, 1e5] cm applies to every grain of the list, also with dt == 0
or behind a closed gate; the literal 3.1415 of :528; BOLTZMANN = 1.3806e-16 (allvars.h:84)."""
import numpy as np

import dust_ref as R

BOLTZMANN = 1.3806e-16
A_MIN, A_MAX = 0.1, 1.e5          # adust_min, adust_max [cm], dust.c:277
LATENT_ROCK, LATENT_ICE = 1.e11, 4.e10   # erg/g, dust.c:268, 270
SWITCHES = ("growth", "real_pebble_collisions", "vaporize", "fe_and_ice_grains", "epstein",
            "no_friction_heating")


def model(*on, **over):
    """the members of ghip_dust_model: the switches named in `on` set, the rest 0"""
    m = dict.fromkeys(SWITCHES, 0)
    for k in on:
        assert k in m, k
        m[k] = 1
    m.update(Time=1.0, VirtualTime=0.5, FragmentationVelocity=10.0, InitialDustRadius=1.0,
             UnitEnergy_in_cgs=1.989e33 * 6.674e-8 * 1.989e33 / 1.496e13)
    m.update(over)
    return m


def dust_density(pos, vel, mass, ptype, hsml, dust, box, periodic, m):
    """(d7, d9): d7 as dust_ref.dust_density; d9 [nd][3] the raw sums m_i W(r, h_i) Vel_j over the same
    neighbours (dust.c:851-853), None without real_pebble_collisions"""
    d7 = R.dust_density(pos, mass, ptype, hsml, dust, box, periodic)
    if not m["real_pebble_collisions"]:
        return d7, None
    cand = np.nonzero((ptype == 2) & (mass > 0))[0]
    d9 = np.zeros((len(dust), 3))
    for a, i in enumerate(dust):
        w, ok = R.weights(pos[i], pos[cand], hsml[i], box, periodic)
        d9[a] = np.sum((mass[i] * w[ok])[:, None] * vel[cand[ok]], axis=0)
    return d7, d9


def growth_rate(par, m, radius, d7, vcoll):
    """(t_coll, adot) of dust.c:463-490 for one grain behind an open gate with d7 > 0"""
    UL = par["UnitLength_in_cm"]
    t_coll = 4. * (R.RHO_GRAIN / par["UnitDensity_in_cgs"]) * (radius / UL) / d7 / \
        (vcoll * 1.e2 / par["UnitVelocity_in_cm_per_s"] + 1.e-20)
    adot = radius / UL / 3. / t_coll
    if m["real_pebble_collisions"]:
        if m["FragmentationVelocity"] < 0.1:
            adot = 0.
        else:
            x = vcoll / m["FragmentationVelocity"]
            adot *= (1 - x * x) / (1 + x * x)
    return t_coll, adot


def vapour(par, rho, ent, ice):
    """(T, pvap, term) of dust.c:502-528 for one grain: the dust temperature, the vapour pressure of rock
    (ice = False) or water ice, and what is subtracted from adot"""
    uv = par["UnitVelocity_in_cm_per_s"]
    cs = np.sqrt(8. / np.pi * ent * rho ** R.GAMMA_MINUS1)
    csu = cs * uv
    T = np.pi / 8. * (csu * csu) * par["MeanWeight"] * R.PROTONMASS / BOLTZMANN
    if not ice:
        pvap = 10. ** (-24605. / T + 13.176)
    elif T <= 600.:
        pvap = 10. ** (11.6 - 2104. / T)
    else:
        pvap = 5. + 5.2e-3 * T
    term = 1. / (R.RHO_GRAIN * np.sqrt(2. * 3.1415)) / cs / uv * pvap / uv
    return T, pvap, term


def latent_heat(m, a, ice):
    """dust.c:536-547: the latent heat per gram of a grain of radius a"""
    return (LATENT_ICE if ice else LATENT_ROCK) * (a - A_MIN) / (m["InitialDustRadius"] - A_MIN)


def grain_update(par, m, vel, mass, grav, dt, rho, ent, gasvel, radius, d7, d9, vcoll, ids=None, logr=None):
    """the per-grain part of dust_drag (dust.c:303-609) under the switches `m`, grains as rows.  Returns what
    dust_ref.grain_update returns plus radius, logr (the caller's value where :465 does not write) and, for the
    tests' census, gate (the gate passed with d7 > 0), x (DustVcoll / FragmentationVelocity, nan elsewhere), T,
    vap (the vapour term of adot, 0 where none), ice, adot, lo / hi (the clamps bound)."""
    n = len(rho)
    vel = np.array(vel, np.float64)
    d9 = np.array(d9, np.float64)
    vcoll = np.array(vcoll, np.float64)
    radius = np.array(radius, np.float64)
    logr = np.zeros(n) if logr is None else np.array(logr, np.float64)
    ids = np.zeros(n, np.int64) if ids is None else np.asarray(ids)
    dmom = np.zeros((n, 3))
    de = np.zeros(n)
    regime = np.full(n, R.NO_DT)
    gate = np.zeros(n, bool)
    lo, hi = np.zeros(n, bool), np.zeros(n, bool)
    ice = np.zeros(n, bool)
    x, T, vap, adots = np.full(n, np.nan), np.full(n, np.nan), np.zeros(n), np.zeros(n)
    UL, UM = par["UnitLength_in_cm"], par["UnitMass_in_g"]
    open_gate = m["Time"] > 0 and m["Time"] > m["VirtualTime"]
    for a in range(n):
        r = rho[a]
        cs = np.sqrt(8. / np.pi * ent[a] * r ** R.GAMMA_MINUS1)
        v = vel[a].copy()
        dv = np.sqrt(np.sum((v - gasvel[a]) ** 2))
        if d7[a] > 0.:
            d9[a] = d9[a] / d7[a]
            vcoll[a] = np.sqrt(np.sum((v - d9[a]) ** 2)) * par["UnitVelocity_in_cm_per_s"] / 1.e2 + 1.e-30
        if dt[a] > 0:
            Rg = radius[a]
            lam = par["MeanWeight"] * R.PROTONMASS / (par["UnitDensity_in_cgs"] * r) / 1.e-15 / UL
            rey = 6 * dv * Rg / UL / (lam * cs)
            if m["epstein"] or 3. / 2 * lam * UL >= Rg:
                ts = 1. / (r * cs / (R.RHO_GRAIN * Rg) * UM / UL / UL)
                regime[a] = R.EPSTEIN
            elif dv > 0:
                if rey >= 800.:
                    cd, regime[a] = 0.44, R.STOKES_HIGH
                elif rey >= 1.:
                    cd, regime[a] = 24. * rey ** -0.6, R.STOKES_MID
                else:
                    cd, regime[a] = 24. / rey, R.STOKES_LOW
                ts = R.RHO_GRAIN * Rg / (r * dv) / UM * UL * UL
                ts *= 8. / 3. / cd
            else:
                ts = 0.66667 / (r * cs / (R.RHO_GRAIN * Rg)) / UM * UL * Rg / lam
                regime[a] = R.STILL
            e1, e2 = np.exp(-dt[a] / ts), np.exp(-2. * dt[a] / ts)
            for k in range(3):
                vold = v[k]
                vs = (vold * d7[a] + gasvel[a][k] * r) / (d7[a] + r + 1.e-30)
                vel[a, k] = vs + (vold - vs) * e1 + grav[a][k] * ts * (1. - e1)
                dmom[a, k] = -mass[a] * (vold + grav[a][k] * dt[a] - vel[a, k])
                if not m["no_friction_heating"]:
                    de[a] += mass[a] * (vel[a, k] - vs) ** 2 * (1. - e2) / 2.
            vcoll[a] = np.sqrt(np.sum(np.asarray(grav[a]) ** 2)) * ts * par["UnitVelocity_in_cm_per_s"] / 1.e2
            vcoll[a] += 0.2
        if not m["growth"]:
            continue
        old_a = radius[a]
        adot = 0.
        if open_gate and d7[a] > 0.:
            gate[a] = True
            logr[a], adot = growth_rate(par, m, old_a, d7[a], vcoll[a])
            if m["real_pebble_collisions"] and not m["FragmentationVelocity"] < 0.1:
                x[a] = vcoll[a] / m["FragmentationVelocity"]
        if m["vaporize"]:
            ice[a] = bool(m["fe_and_ice_grains"]) and int(ids[a]) % 2 == 1
            if r > 0.:
                T[a], _, vap[a] = vapour(par, r, ent[a], ice[a])
                adot -= vap[a]
        adots[a] = adot
        new_a = old_a + (adot * dt[a]) * UL
        if new_a < A_MIN:
            new_a, lo[a] = A_MIN, True
        if new_a > A_MAX:
            new_a, hi[a] = A_MAX, True
        radius[a] = new_a
        if m["vaporize"]:
            de[a] += (latent_heat(m, new_a, ice[a]) - latent_heat(m, old_a, ice[a])) * mass[a] * UM / \
                m["UnitEnergy_in_cgs"]
    return dict(vel=vel, d9=d9, dmom=dmom, de=de, vcoll=vcoll, regime=regime, radius=radius, logr=logr,
                gate=gate, x=x, T=T, vap=vap, ice=ice, adot=adots, lo=lo, hi=hi)
