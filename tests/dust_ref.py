"""Independent numpy restatement of the reference's dust-gas drag passes for the shipped flag bundle
(dust.c: dust_density / dust_evaluate_density :60-261, 748-887; dust_drag :263-446; dust_evaluate_select
:889-1029; ngb_treefind_dust_active :1235-1333), with brute-force neighbour search.  Used by the dust
tests; nothing here imports the product.

Flags resolved: DUST, DUST_TIMESTEP, DUST_POWERLAW, DOUBLEPRECISION, CONSTANT_MEAN_MOLECULAR_WEIGHT;
GAMMA = 7/5 (allvars.h:64); rho_dust = 3 (dust.c:379); PROTONMASS = 1.6726e-24 (allvars.h:89)."""
import numpy as np

GAMMA_MINUS1 = 7.0 / 5.0 - 1
PROTONMASS = 1.6726e-24
RHO_GRAIN = 3.0
K1, K2, K5 = 2.546479089470, 15.278874536822, 5.092958178941

# regimes of the stopping time (dust.c:385-417) as grain_update labels them
EPSTEIN, STOKES_LOW, STOKES_MID, STOKES_HIGH, STILL, NO_DT = range(6)


def _wrap(d, box, periodic):
    if periodic:
        d = np.where(d > 0.5 * box, d - box, d)
        d = np.where(d < -0.5 * box, d + box, d)
    return d


def weights(p, q, h, box, periodic):
    """kernel weight W(|p - q|, h) of the grain at p for candidates q [m][3], 0 outside: the tree search
    keeps r <= h (dust.c:1253-1260), the evaluation u = r / h < 1 (:826-847, 971-983)"""
    d = _wrap(p[None, :] - q, box, periodic)
    r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    u = np.sqrt(r2) / h
    ok = (r2 <= h * h) & (u < 1)
    hinv = 1 / h
    hinv3 = hinv * hinv * hinv
    w = np.where(u < 0.5, hinv3 * (K1 + K2 * (u - 1) * u * u), hinv3 * K5 * (1.0 - u) * (1.0 - u) * (1.0 - u))
    return np.where(ok, w, 0.0), ok


def dust_density(pos, mass, ptype, hsml, dust, box, periodic):
    """d7.DUST_particle_density of the grains `dust` (dust.c:849): m_i * sum W over the Type-2
    neighbours with Mass > 0 -- the GRAIN's own mass m_i, as in the reference"""
    cand = np.nonzero((ptype == 2) & (mass > 0))[0]
    out = np.zeros(len(dust))
    for a, i in enumerate(dust):
        w, ok = weights(pos[i], pos[cand], hsml[i], box, periodic)
        out[a] = np.sum(mass[i] * w[ok])
    return out


def grain_update(par, vel, mass, grav, dt, rho, ent, gasvel, radius, d7, d9, vcoll):
    """the per-grain part of dust_drag (dust.c:303-446) for grains given as rows.  Returns dict(vel,
    d9, dmom, de, vcoll, regime); `dt` = bin * Timebase_interval / hubble_a per grain."""
    n = len(rho)
    vel = np.array(vel, np.float64)
    d9 = np.array(d9, np.float64)
    vcoll = np.array(vcoll, np.float64)
    dmom = np.zeros((n, 3))
    de = np.zeros(n)
    regime = np.full(n, NO_DT)
    UL, UM = par["UnitLength_in_cm"], par["UnitMass_in_g"]
    for a in range(n):
        r = rho[a]
        cs = np.sqrt(8. / np.pi * ent[a] * r ** GAMMA_MINUS1)
        v = vel[a].copy()
        dv = np.sqrt(np.sum((v - gasvel[a]) ** 2))
        if d7[a] > 0.:
            d9[a] = d9[a] / d7[a]
            vcoll[a] = np.sqrt(np.sum((v - d9[a]) ** 2)) * par["UnitVelocity_in_cm_per_s"] / 1.e2 + 1.e-30
        if dt[a] > 0:
            R = radius[a]
            lam = par["MeanWeight"] * PROTONMASS / (par["UnitDensity_in_cgs"] * r) / 1.e-15 / UL
            rey = 6 * dv * R / UL / (lam * cs)
            if 3. / 2 * lam * UL >= R:
                ts = 1. / (r * cs / (RHO_GRAIN * R) * UM / UL / UL)
                regime[a] = EPSTEIN
            elif dv > 0:
                if rey >= 800.:
                    cd, regime[a] = 0.44, STOKES_HIGH
                elif rey >= 1.:
                    cd, regime[a] = 24. * rey ** -0.6, STOKES_MID
                else:
                    cd, regime[a] = 24. / rey, STOKES_LOW
                ts = RHO_GRAIN * R / (r * dv) / UM * UL * UL
                ts *= 8. / 3. / cd
            else:
                ts = 0.66667 / (r * cs / (RHO_GRAIN * R)) / UM * UL * R / lam
                regime[a] = STILL
            e1, e2 = np.exp(-dt[a] / ts), np.exp(-2. * dt[a] / ts)
            for k in range(3):
                vold = v[k]
                vs = (vold * d7[a] + gasvel[a][k] * r) / (d7[a] + r + 1.e-30)
                vel[a, k] = vs + (vold - vs) * e1 + grav[a][k] * ts * (1. - e1)
                dmom[a, k] = -mass[a] * (vold + grav[a][k] * dt[a] - vel[a, k])
                de[a] += mass[a] * (vel[a, k] - vs) ** 2 * (1. - e2) / 2.
            vcoll[a] = np.sqrt(np.sum(np.asarray(grav[a]) ** 2)) * ts * par["UnitVelocity_in_cm_per_s"] / 1.e2
            vcoll[a] += 0.2
    return dict(vel=vel, d9=d9, dmom=dmom, de=de, vcoll=vcoll, regime=regime)


def gas_scatter(par, gpos, ghsml, grho, dmom, de, pos, mass, ptype, ngas, dt_gas, vel, entropy, heat,
                gas_idx=None):
    """dust_evaluate_select (dust.c:889-1029) applied serially, grain after grain in list order (rows of
    gpos ...), to the gas particles `gas_idx` (default: all of [0, ngas)).  vel [*][3], entropy, heat are
    indexed like gas_idx and updated in place.  Returns counts of the pair events where the 1.5 cap and
    the MinEgySpec floor bound, and the number of grains per gas particle."""
    box, periodic = par["BoxSize"], par["periodic"]
    gidx = np.arange(ngas) if gas_idx is None else np.asarray(gas_idx)
    live = (ptype[gidx] == 0) & (mass[gidx] > 0) & (dt_gas[gidx] > 0)
    touched = np.zeros(len(gidx), np.int64)
    caps = floors = 0
    for a in range(len(grho)):
        dens = grho[a]
        if not dens > 0.:
            continue
        w, ok = weights(gpos[a], pos[gidx], ghsml[a], box, periodic)
        sel = np.nonzero(ok & live)[0]
        if len(sel) == 0:
            continue
        wk = w[sel]
        touched[sel] += 1
        for k in range(3):
            vel[sel, k] -= dmom[a][k] / dens * wk
        u_raw = entropy[sel] / GAMMA_MINUS1 * dens ** GAMMA_MINUS1
        u_old = np.where(par["MinEgySpec"] > u_raw, par["MinEgySpec"], u_raw)
        floors += int(np.sum(par["MinEgySpec"] > u_raw))
        u_inc = (u_old + de[a] * wk / dens) / u_old
        caps += int(np.sum(u_inc > 1.5))
        u_inc = np.where(u_inc > 1.5, 1.5, u_inc)
        entropy[sel] *= u_inc
        j = gidx[sel]
        heat[sel] += 1.e-20 * (de[a] * wk / dens * mass[j] / dt_gas[j])
    return dict(caps=caps, floors=floors, touched=touched)


def params(box, periodic, timebase, **over):
    """a disc-like unit system (AU, solar mass; v unit sqrt(G M / L)) and the rest of ghip_dust_params"""
    UL, UM = 1.496e13, 1.989e33
    p = dict(periodic=int(periodic), BoxSize=float(box), dt_fac=timebase, dt_fac_gas=timebase,
             MinEgySpec=0.0, MeanWeight=2.3, UnitLength_in_cm=UL, UnitMass_in_g=UM,
             UnitDensity_in_cgs=UM / UL ** 3, UnitVelocity_in_cm_per_s=np.sqrt(6.674e-8 * UM / UL))
    p.update(over)
    return p


def mean_free_path(par, rho):
    """lambda_h2 in code units (dust.c:389)"""
    return par["MeanWeight"] * PROTONMASS / (par["UnitDensity_in_cgs"] * rho) / 1.e-15 / par["UnitLength_in_cm"]
