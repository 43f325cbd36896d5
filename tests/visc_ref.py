"""numpy restatement of the SPH pair loop with its viscosity switches, all pairs, O(N^2).

hydro_evaluate (hydra.c:1250-1621, mode 0) for -DTIME_DEP_ART_VISC, -DCONVENTIONAL_VISCOSITY,
-DNOVISCOSITYLIMITER and -DNO_SHEAR_VISCOSITY_LIMITER as run-time switches, the post-pass of hydro_force
(hydra.c:583, 735-744) and the alpha update of do_the_kick (timestep.c:530-533).  No tree: every gas
particle is tried against every other with the minimum image, so the neighbour search cannot hide
anything.  With every switch off and alpha = ArtBulkViscConst it is what oracle.Tree.hydro computes
(tests/test_visc_cpu.py pins the two together; the oracle itself may not change).

GAMMA = 7/5 (allvars.h:64); kernel coefficients of allvars.h:247-252.
"""
import numpy as np

GAMMA = 7.0 / 5.0
GAMMA_MINUS1 = GAMMA - 1
KERNEL_COEFF_3 = 45.836623610466
KERNEL_COEFF_4 = 30.557749073644
KERNEL_COEFF_6 = -15.278874536822


def params(**over):
    """ghip_visc_params as a dict: every switch off"""
    v = dict(time_dependent=0, conventional=0, no_limiter=0, no_shear_limiter=0, ArtBulkViscConst=0.8,
             AlphaMin=0.1, ViscSource=1.0, DecayTime=1.0, dtalpha_comoving_div=1.0)
    v.update(over)
    return v


def derive(visc_source0, decay_length):
    """begrun.c:132-133 as written"""
    return (visc_source0 / np.log((GAMMA + 1) / (GAMMA - 1)),
            1 / decay_length * np.sqrt((GAMMA - 1) / 2 * GAMMA))


def hydro(pr, dens_state, alpha, visc_params, hydro_params, act=None, raw=False):
    """pr: a common.Problem (positions, masses, VelPred, TimeBin, box); dens_state: dict of hsml, density,
    pressure, dhsmlfac, divvel, curlvel (first ngas entries read); alpha: [ngas]; visc_params: params();
    hydro_params: an object with the members of ghip_hydro_params / oracle.HydroParams; act: gas targets
    (None: all).  Returns dict(hydroaccel [ngas][3], dtentropy (raw sum or converted, hydra.c:583),
    maxsignalvel, npairs, napproach, nlimited); non-targets are zero."""
    ng = pr.ngas
    V, H = visc_params, hydro_params
    pos = np.asarray(pr.ic["pos"][:ng], np.float64)
    mass = np.asarray(pr.ic["mass"][:ng], np.float64)
    vel = np.asarray(pr.velpred[:ng], np.float64)
    hs, rho_, pres, dhf, divv, curl = (np.asarray(dens_state[k][:ng], np.float64) for k in
                                       ("hsml", "density", "pressure", "dhsmlfac", "divvel", "curlvel"))
    alpha = np.asarray(alpha, np.float64)
    tb = np.asarray(pr.timebin[:ng])
    tstep = np.where(tb > 0, np.left_shift(1, tb), 0).astype(np.float64)      # hydra.c:967
    box, boxhalf = H.BoxSize, 0.5 * H.BoxSize
    fac_mu, hubble_a2, fac_vsic_fix = H.fac_mu, H.hubble_a2, H.fac_vsic_fix
    out = dict(hydroaccel=np.zeros((ng, 3)), dtentropy=np.zeros(ng), maxsignalvel=np.zeros(ng))
    npairs = napproach = nlimited = 0
    p_over_rho2_all = pres / (rho_ * rho_)                                    # hydra.c:1271
    cs_all = np.sqrt(GAMMA * p_over_rho2_all * rho_)                          # hydra.c:1272
    f2_all = np.abs(divv) / (np.abs(divv) + curl + 0.0001 * cs_all / fac_mu / hs)   # hydra.c:1529-1531
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in (range(ng) if act is None else [int(a) for a in act]):
            h_i, rho, press = hs[i], rho_[i], pres[i]
            soundspeed_i = np.sqrt(GAMMA * press / rho)                       # hydra.c:968
            f1 = abs(divv[i]) / (abs(divv[i]) + curl[i] + 0.0001 * soundspeed_i / hs[i] / fac_mu)   # :970-977
            p_over_rho2_i = press / (rho * rho)                               # hydra.c:1154-1155
            p_over_rho2_i *= dhf[i]
            h_i2 = h_i * h_i
            d = pos[i] - pos                                                  # hydra.c:1247-1262
            if H.periodic:
                d = np.where(d > boxhalf, d - box, d)
                d = np.where(d < -boxhalf, d + box, d)
            dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
            r2 = dx * dx + dy * dy + dz * dz
            sel = ((r2 < h_i2) | (r2 < hs * hs)) & (r2 > 0)                   # hydra.c:1266-1269
            j = np.where(sel)[0]
            npairs += len(j)
            dx, dy, dz, r2 = dx[j], dy[j], dz[j], r2[j]
            r = np.sqrt(r2)
            h_j = hs[j]
            dv = vel[i] - vel[j]
            vdotr = dx * dv[:, 0] + dy * dv[:, 1] + dz * dv[:, 2]
            vdotr2 = vdotr + hubble_a2 * r2 if H.ComovingIntegrationOn else vdotr   # hydra.c:1276-1281

            def dwk(h, inside):                                               # hydra.c:1285-1352
                hinv = 1.0 / h
                hinv4 = hinv * hinv * hinv * hinv
                u = r * hinv
                w = np.where(u < 0.5, hinv4 * u * (KERNEL_COEFF_3 * u - KERNEL_COEFF_4),
                             hinv4 * KERNEL_COEFF_6 * (1.0 - u) * (1.0 - u))
                return np.where(inside, w, 0.0)
            dwk_i = dwk(h_i, r2 < h_i2)
            dwk_j = dwk(h_j, r2 < h_j * h_j)
            soundspeed_j = cs_all[j]
            vsig = soundspeed_i + soundspeed_j                                # hydra.c:1502
            maxsig = vsig.max() if len(j) else 0.0                            # hydra.c:1507-1508
            appr = vdotr2 < 0                                                 # hydra.c:1510
            if V["conventional"]:                                             # hydra.c:1516-1518
                c_ij = 0.5 * (soundspeed_i + soundspeed_j)
                h_ij = 0.5 * (h_i + h_j)
                mu_ij = fac_mu * h_ij * vdotr2 / (r2 + 0.0001 * h_ij * h_ij)
            else:                                                             # hydra.c:1514
                mu_ij = fac_mu * vdotr2 / r
            vsig2 = vsig - 3 * mu_ij                                          # hydra.c:1520
            if appr.any():
                maxsig = max(maxsig, vsig2[appr].max())                       # hydra.c:1523-1524
            rho_ij = 0.5 * (rho + rho_[j])                                    # hydra.c:1527
            f1_, f2_ = f1, f2_all[j]
            if V["no_shear_limiter"]:                                         # hydra.c:1538-1540
                f1_, f2_ = 1.0, 1.0
            if V["time_dependent"]:                                           # hydra.c:1541-1545
                bulk = 0.5 * (alpha[i] + alpha[j])
            else:
                bulk = H.ArtBulkViscConst
            if V["conventional"]:                                             # hydra.c:1549-1551
                visc = (-bulk * mu_ij * c_ij + 2 * bulk * mu_ij * mu_ij) / rho_ij * (f1_ + f2_) * 0.5
            else:                                                             # hydra.c:1547
                visc = 0.25 * bulk * vsig2 * (-mu_ij) / rho_ij * (f1_ + f2_)
            napproach += int(appr.sum())
            if not V["no_limiter"]:                                           # hydra.c:1583-1595
                dt = 2 * np.maximum(tstep[i], tstep[j]) * H.Timebase_interval
                can = appr & (dt > 0) & ((dwk_i + dwk_j) < 0)
                lim = 0.5 * fac_vsic_fix * vdotr2 / (0.5 * (mass[i] + mass[j]) * (dwk_i + dwk_j) * r * dt)
                hit = can & (lim < visc)
                nlimited += int(hit.sum())
                visc = np.where(hit, lim, visc)
            visc = np.where(appr, visc, 0.0)                                  # hydra.c:1597-1600
            p_over_rho2_j = p_over_rho2_all[j] * dhf[j]                       # hydra.c:1602
            hfc_visc = 0.5 * mass[j] * visc * (dwk_i + dwk_j) / r             # hydra.c:1604
            hfc = hfc_visc + mass[j] * (p_over_rho2_i * dwk_i + p_over_rho2_j * dwk_j) / r   # hydra.c:1606
            out["hydroaccel"][i] = [(-hfc * dx).sum(), (-hfc * dy).sum(), (-hfc * dz).sum()]   # :1616-1618
            de = (0.5 * hfc_visc * vdotr2).sum()                              # hydra.c:1621
            if not raw:                                                       # hydra.c:583
                de *= GAMMA_MINUS1 / (hubble_a2 * np.power(rho, GAMMA_MINUS1))
            out["dtentropy"][i] = de
            out["maxsignalvel"][i] = maxsig
    out.update(npairs=npairs, napproach=napproach, nlimited=nlimited)
    return out


def dtalpha(pressure, density, hsml, divvel, curlvel, maxsignalvel, alpha, visc_params, fac_mu=1.0,
            comoving=0):
    """hydra.c:736-743 with v.DivVel / r.CurlVel (the members the pair loop reads, hydra.c:1530; the
    u.s.* members named there exist only under -DNAVIERSTOKES, allvars.h:1454-1470)"""
    V = visc_params
    pressure, density, hsml, divvel, curlvel, maxsignalvel, alpha = (
        np.asarray(a, np.float64) for a in (pressure, density, hsml, divvel, curlvel, maxsignalvel, alpha))
    cs_h = np.sqrt(GAMMA * pressure / density) / hsml                         # hydra.c:736
    f = np.abs(divvel) / (np.abs(divvel) + curlvel + 0.0001 * cs_h / fac_mu)  # hydra.c:737-738
    da = -(alpha - V["AlphaMin"]) * V["DecayTime"] * 0.5 * maxsignalvel / (hsml * fac_mu) + \
        f * V["ViscSource"] * np.maximum(0.0, -divvel)                        # hydra.c:739-741
    if comoving:                                                              # hydra.c:742-743
        da = da / V["dtalpha_comoving_div"]
    return da


def kick_alpha(alpha, dtalpha_, dt_entr, visc_params):
    """timestep.c:530-533"""
    V = visc_params
    a = np.asarray(alpha, np.float64) + np.asarray(dtalpha_, np.float64) * dt_entr    # timestep.c:530
    a = np.where(a < V["ArtBulkViscConst"], a, V["ArtBulkViscConst"])         # timestep.c:531 (DMIN)
    return np.where(a < V["AlphaMin"], V["AlphaMin"], a)                      # timestep.c:532-533
