"""The wind particles of the shipped flag bundle (-DVIRTUAL -DFB_MOMENTUM, with VIRTUAL_FLY_THORUGH_EMPTY_SPACE,
VARIABLE_PHOTON_SEARCH_RADIUS and RAD_ACCEL as switches) restated directly from the reference's C text, all
pairs: every wind particle against all gas particles, plain numpy, no tree, no neighbour search and no import
of the oracle or of the library.  Written from

    momentum_feedback.c:283-568            the propagation loop, RAD_ACCEL, the elimination  -> feedback()
    virtual_density.c:79-127, 382-625      virtual_density / virtual_evaluate_select         -> density()
    virtual_density.c:628-664              ngb_treefind_virtual_active (gas, r2 <= h^2)
    virtual_spread_momentum.c:129-130, 310-469   virtual_spread_momentum / _evaluate_onthespot  -> spread()
    timestep.c:337-339, 497-500, 668-671, predict.c:190-192   RAD_ACCEL in the integrator -> the *_rad functions,
                                                               which call tests/kick_ref.py

Every per-pair and per-particle decision is taken with the C text's own fp64 expression, in its operation
order; every SUM (the density, the injected momentum over the whole loop, dt_total, the deleted momentum) is
accumulated in np.longdouble and rounded to fp64 once, so the restatement carries no summation-order error of
its own.

Every function also records the SMALLEST RELATIVE MARGIN over the discrete decisions it took (Margins): r
against the search radius, u against 1, the desired jump against the time cap, the 1 % depletion test, r
against OuterBoundary, the age against VirtualTime, dt_total against its floor.  Two implementations whose pow,
exp or summation order differ in the last bit agree on a decision only when its margin is far above 1e-16.

One deviation from the C text is kept, because the project takes it on purpose (ghip_wind.hip):
  (1) when the time cap of momentum_feedback.c:345-346 sets the jump, dt1 = dt_jump exactly and the particle
      ends the iteration with dt_jump = 0.  The reference recomputes dt1 = dr * U / C * FBV (:348) and subtracts
      it (:371-372); the residue of that round trip is 0 or +-1 ulp depending on the last bit of dt_jump, and on
      its sign hangs one more iteration of length ~1e-17 that spreads the previous DeltaPhotonMomentum again.
      feedback(round_trip=True) applies the reference's own rule; it exists only so that a test can show that
      the two rules differ.
"""
import numpy as np

KERNEL_COEFF_1 = 2.546479089470
KERNEL_COEFF_2 = 15.278874536822
KERNEL_COEFF_5 = 5.092958178941
C_LIGHT = 2.9979e10          # allvars.h:86
PROTONMASS = 1.6726e-24      # allvars.h:89
THOMPSON = 6.65245e-25       # allvars.h:91
LD = np.longdouble

PARAMS = ("periodic", "BoxSize", "Time", "dt_fac", "dt_fac_gas", "FeedBackVelocity", "UnitVelocity_in_cm_per_s",
          "UnitDensity_in_cgs", "UnitLength_in_cm", "VirtualCrosSection", "VirtualMass", "VirtualTime",
          "OuterBoundary", "DesNumNgb", "OriginalGasMass", "SofteningGas", "SofteningGasMaxPhys",
          "SofteningBulgeMaxPhys", "PhotonSearchRadius", "dt_total_floor", "fly_through_empty_space",
          "variable_search_radius", "rad_accel", "max_iter")


def params(**over):
    """ghip_wind_params as a dict; the defaults make every rule of the loop reachable in a unit box"""
    p = dict(periodic=0, BoxSize=1.0, Time=1.0, dt_fac=1e-3, dt_fac_gas=1e-3, FeedBackVelocity=1.0,
             UnitVelocity_in_cm_per_s=C_LIGHT / 50.0, UnitDensity_in_cgs=1.0, UnitLength_in_cm=1.0,
             VirtualCrosSection=PROTONMASS / THOMPSON, VirtualMass=1e-6, VirtualTime=10.0, OuterBoundary=10.0,
             DesNumNgb=33.0, OriginalGasMass=1e-3, SofteningGas=0.01, SofteningGasMaxPhys=0.01,
             SofteningBulgeMaxPhys=0.02, PhotonSearchRadius=0.5, dt_total_floor=0.0,
             fly_through_empty_space=1, variable_search_radius=1, rad_accel=0, max_iter=1000)
    assert set(over) <= set(p), set(over) - set(p)
    p.update(over)
    return p


class Margins:
    """the smallest relative margin |a - b| / |b| of every kind of decision taken"""

    def __init__(self):
        self.by_kind = {}

    def note(self, kind, a, b):
        a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
        if a.size == 0:
            return
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.abs(a - b) / np.abs(b)
        m = m[np.isfinite(m)]
        if m.size:
            self.by_kind[kind] = min(self.by_kind.get(kind, np.inf), float(m.min()))

    def smallest(self):
        return min(self.by_kind.values()) if self.by_kind else np.inf


def _pairs(par, gas, wpos, wh, M):
    """wind particles (rows) against the gas (columns): the candidates of ngb_treefind_virtual_active with
    Mass > 0 (virtual_density.c:495, 650-664), r and u = r / h_j (:497-524).  gas: dict(pos, hsml, mass, type)
    of the gas block."""
    d = wpos[:, None, :] - gas["pos"][None, :, :]
    if par["periodic"]:                                    # :500-513, the two comparisons
        box = par["BoxSize"]
        half = 0.5 * box
        d = np.where(d > half, d - box, d)
        d = np.where(d < -half, d + box, d)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    r2 = dx * dx + dy * dy + dz * dz
    ok = ((gas["type"] == 0) & (gas["mass"] > 0))[None, :]
    h2 = (wh * wh)[:, None]
    M.note("search_radius", np.where(ok, r2, np.nan), np.broadcast_to(h2, r2.shape))
    found = ok & ~(r2 > h2)
    r = np.sqrt(r2)
    u = r / gas["hsml"][None, :]
    M.note("u_vs_1", np.where(found, u, np.nan), 1.0)
    return found, r, u


def _wk(u, hj):
    """virtual_density.c:528-537"""
    hinv = 1 / hj
    hinv3 = hinv * hinv * hinv
    with np.errstate(invalid="ignore"):
        lo = hinv3 * (KERNEL_COEFF_1 + KERNEL_COEFF_2 * (u - 1) * u * u)
        hi = hinv3 * KERNEL_COEFF_5 * (1.0 - u) * (1.0 - u) * (1.0 - u)
    return np.where(u < 0.5, lo, hi)


def density(par, gas, wpos, wh, dt_jump, M=None):
    """one virtual_density(): (new_density, drmin) of the listed particles -- 0 and 1e40 for all (:107-127),
    evaluated where dt_jump > 0"""
    M = M if M is not None else Margins()
    nw = len(wh)
    rho, drmin = np.zeros(nw), np.full(nw, 1.e40)
    ev = np.flatnonzero(np.asarray(dt_jump) > 0)
    if len(ev) and len(gas["mass"]):
        found, r, u = _pairs(par, gas, wpos[ev], wh[ev], M)
        hj = gas["hsml"][None, :]
        drcheck = np.abs(r - hj) + 0.25 * hj                           # :519
        drmin[ev] = np.minimum(1.e40, np.where(found, drcheck, np.inf).min(axis=1))
        inside = found & (u < 1)
        mw = np.where(inside, gas["mass"][None, :] * _wk(u, hj), 0.0)   # :539, FLT(P[j].Mass * wk)
        rho[ev] = mw.astype(LD).sum(axis=1).astype(np.float64)
    return rho, drmin


def spread(par, gas, wpos, wh, wvel, dt_jump, new_density, delta_momentum, inj, M=None):
    """one virtual_spread_momentum(): adds to inj (np.longdouble [ngas][3], in place) what the gas receives
    from the listed particles with new_density > 0 && dt_jump > 0 (:129-130, 432, 447-448)"""
    M = M if M is not None else Margins()
    sp = np.flatnonzero((np.asarray(new_density) > 0) & (np.asarray(dt_jump) > 0))
    if not len(sp) or not len(gas["mass"]):
        return sp
    found, r, u = _pairs(par, gas, wpos[sp], wh[sp], M)
    hj = gas["hsml"][None, :]
    inside = found & (u < 1)
    v = wvel[sp]
    absol_vel = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])   # :391
    ddpm = delta_momentum[sp][:, None] * gas["mass"][None, :] * _wk(u, hj) / new_density[sp][:, None]   # :432
    ddpm = np.where(inside, ddpm, 0.0)
    for k in range(3):
        c = ddpm * v[:, k][:, None] / absol_vel[:, None]               # :448
        inj[:, k] += c.astype(LD).sum(axis=0)
    return sp


def gas_of(fields):
    """the gas block as _pairs reads it"""
    ng = int(fields["ngas"])
    return dict(pos=np.asarray(fields["pos"], np.float64)[:ng], hsml=np.asarray(fields["hsml"], np.float64)[:ng],
                mass=np.asarray(fields["mass"], np.float64)[:ng], type=np.asarray(fields["type"])[:ng])


def rad_accel(par, fields, active, injected):
    """momentum_feedback.c:497-538 for the active gas: (RadAccel of the active gas, others None-> untouched),
    returns (ra [ngas][3] with the rows of `touched` set, injected with those rows zeroed, touched mask)"""
    ng = int(fields["ngas"])
    ra = np.zeros((ng, 3))
    inj = np.array(injected, np.float64)
    touched = np.zeros(ng, bool)
    for i in (range(len(fields["type"])) if active is None else active):
        i = int(i)
        if i >= ng or fields["type"][i] != 0:
            continue
        tb = int(fields["timebin"][i])
        dt = ((1 << tb) if tb else 0) * par["dt_fac_gas"]
        m = float(fields["mass"][i])
        r = np.zeros(3)
        if dt != 0. and m > 0.:
            r = inj[i] / dt / m
            ac = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
            acmax = 1.e4 / dt
            if ac >= acmax:
                r = r * (acmax / ac)
        ra[i] = r
        inj[i] = 0.
        touched[i] = True
    return ra, inj, touched


def feedback(par, fields, wind, state, active=None, injected=None, rad_accel0=None, round_trip=False):
    """momentum_feedback.c:283-568.  fields: dict(pos [n][3], vel, hsml, mass, type, timebin, ngas) -- not
    modified; wind: the list; state: dict(stellar_age, birth_energy, old_momentum, new_density, drmin) in list
    order.  Returns a dict: pos, hsml, mass (copies, updated), the state arrays (old_momentum, new_density,
    drmin, dt1, dt2, dt_jump, delta_momentum, deleted), injected, rad_accel, iterations, bits, ndeleted,
    deleted_momentum, status ('ok', 'floor', 'noconv'), under_way, margins (Margins), ends (how each particle
    ended: sets of list positions by 'cap', 'hidden', 'fly')."""
    M = Margins()
    wind = np.asarray(wind, np.int64)
    nw = len(wind)
    ng = int(fields["ngas"])
    pos = np.array(fields["pos"], np.float64)
    hsml = np.array(fields["hsml"], np.float64)
    mass = np.array(fields["mass"], np.float64)
    vel = np.asarray(fields["vel"], np.float64)[wind]
    f64 = lambda k: np.array(state[k], np.float64)
    age, birth, old = f64("stellar_age"), f64("birth_energy"), f64("old_momentum")
    rho, drmin = f64("new_density"), f64("drmin")
    inj = np.zeros((ng, 3), LD) if injected is None else np.array(injected, LD)
    ra = np.zeros((ng, 3)) if rad_accel0 is None else np.array(rad_accel0, np.float64)
    U, FBV = par["UnitVelocity_in_cm_per_s"], par["FeedBackVelocity"]
    tb = np.asarray(fields["timebin"])[wind].astype(np.int64)
    dtj = np.where(tb > 0, (1 << tb).astype(np.float64), 0.0) * par["dt_fac"]   # :288
    dt1, dt2, dmom = np.zeros(nw), np.zeros(nw), np.zeros(nw)
    deleted = np.zeros(nw, np.int32)
    ends = dict(cap=set(), hidden=set(), fly=set(), grow=set(), hcap=set(), dtau_cap=set())
    out = dict(pos=pos, hsml=hsml, mass=mass, old_momentum=old, new_density=rho, drmin=drmin, dt1=dt1, dt2=dt2,
               dt_jump=dtj, delta_momentum=dmom, deleted=deleted, iterations=0, bits=0, ndeleted=0,
               deleted_momentum=0.0, status="ok", under_way=0, margins=M, ends=ends)
    dt_total = float(dtj.astype(LD).sum())
    M.note("dt_total_floor", dt_total, par["dt_total_floor"])
    if dt_total <= par["dt_total_floor"]:                              # :302
        out.update(status="floor", injected=inj.astype(np.float64), rad_accel=ra)
        return out

    def gas():
        return dict(pos=pos[:ng], hsml=hsml[:ng], mass=mass[:ng], type=np.asarray(fields["type"])[:ng])

    rho[:], drmin[:] = density(par, gas(), pos[wind], hsml[wind], dtj, M)   # :305
    lst = np.arange(nw)
    n_iter = bits = 0
    while True:
        n_iter += 1
        dtj[lst[dtj[lst] <= 0.]] = 0.                                  # :318-322
        A = lst[dtj[lst] > 0.]
        bits += len(A)
        if len(A):
            i = wind[A]
            dt_bh = dtj[A]
            h = hsml[i]
            desired = 0.2 * h                                          # :328
            if par["fly_through_empty_space"]:                         # :337-340
                lim = 0.5 * drmin[A] + 2. * par["SofteningGas"]
                ends["fly"].update(A[desired > lim].tolist())
                desired = np.where(desired > lim, lim, desired)
            cap = C_LIGHT * dt_bh / U / FBV                            # :345-346
            M.note("time_cap", desired, cap)
            capped = desired > cap
            desired = np.where(capped, cap, desired)
            d1 = desired * U / C_LIGHT * FBV                           # :348
            if not round_trip:
                d1 = np.where(capped, dt_bh, d1)                       # deviation (1)
            dtau_max = 10. * desired / h                               # :353-357
            dtau = par["VirtualCrosSection"] * THOMPSON / PROTONMASS * rho[A] * desired * \
                par["UnitDensity_in_cgs"] * par["UnitLength_in_cm"]
            ends["dtau_cap"].update(A[dtau > dtau_max].tolist())
            dtau = np.where(dtau > dtau_max, dtau_max, dtau)
            dm = old[A] * (1. - np.exp(-dtau))                         # :359-360
            o = old[A] - dm
            dmom[A] = dm
            old[A] = o
            mass[i] = par["VirtualMass"] * o                           # :364
            pos[i] = pos[i] + d1[:, None] * vel[A]                     # :367-368
            left = dt_bh - d1                                          # :371-375
            if not round_trip:
                left = np.where(capped, 0., left)
            ends["cap"].update(A[capped].tolist())
            t2 = dt2[A] + d1
            x = pos[i].copy()
            if par["periodic"]:                                        # :382-395
                box = par["BoxSize"]
                half = 0.5 * box
                x = np.where(x > half, x - box, x)
                x = np.where(x < -half, x + box, x)
            r2 = x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]
            dense = rho[A] > 0                                         # :398-405
            with np.errstate(divide="ignore"):
                hnew = np.where(dense, 3. * np.power(par["DesNumNgb"] * par["OriginalGasMass"] / (rho[A] + 1.e-38),
                                                     0.33333) + par["SofteningGasMaxPhys"], h * 1.2)
            ends["grow"].update(A[~dense].tolist())
            if par["variable_search_radius"]:                          # :409-410
                lim = par["PhotonSearchRadius"] * np.sqrt(r2) + par["SofteningBulgeMaxPhys"]
                ends["hcap"].update(A[hnew > lim].tolist())
                hnew = np.where(hnew > lim, lim, hnew)
            hsml[i] = hnew
            thr = 0.01 * birth[A] / C_LIGHT * U                        # :417-424
            M.note("depletion", o, thr)
            hide = o < thr
            ends["hidden"].update(A[hide].tolist())
            t2 = np.where(hide, t2 + left, t2)
            left = np.where(hide, 0., left)
            d1 = np.where(hide, 0., d1)
            dtj[A], dt2[A], dt1[A] = left, t2, d1
        rho[:], drmin[:] = density(par, gas(), pos[wind], hsml[wind], dtj, M)            # :431
        spread(par, gas(), pos[wind], hsml[wind], vel, dtj, rho, dmom, inj, M)           # :436
        lst = np.flatnonzero(dtj > 1.e-40)                             # :444-459
        if len(lst) == 0:
            break
        if n_iter >= par["max_iter"]:
            out.update(status="noconv", under_way=len(lst))
            break
    out.update(iterations=n_iter, bits=bits)
    injected_out = inj.astype(np.float64)
    if out["status"] == "ok":
        if par["rad_accel"]:                                           # :497-538
            f2 = dict(fields, mass=mass)
            r, injected_out, touched = rad_accel(par, f2, active, injected_out)
            ra[touched] = r[touched]
            out["rad_touched"] = touched
        # :550-568
        p = pos[wind]
        r = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2])
        alive = mass[wind] != 0.
        M.note("outer_boundary", r[alive], par["OuterBoundary"])
        M.note("virtual_time", (par["Time"] - age)[alive], par["VirtualTime"])
        first = alive & ((r > par["OuterBoundary"]) | (par["Time"] - age > par["VirtualTime"]))
        thr = 0.01 * birth / C_LIGHT * U
        rest = alive & ~first
        M.note("depletion", old[rest], thr[rest])
        second = rest & (old < thr)
        deleted[first] = 1
        deleted[second] = 2
        mass[wind[first | second]] = 0.
        out.update(ndeleted=int((first | second).sum()),
                   deleted_momentum=float(old[first].astype(LD).sum()))
    out.update(injected=injected_out, rad_accel=ra)
    return out


def round_trip_residue(dt_jump, U, FBV):
    """what the reference leaves of dt_jump after a capped jump: dt_jump - (C dt_jump / U / FBV) U / C FBV
    (momentum_feedback.c:346, 348, 372)"""
    dt_jump = np.asarray(dt_jump, np.float64)
    dr = C_LIGHT * dt_jump / U / FBV
    return dt_jump - dr * U / C_LIGHT * FBV


# ---- RAD_ACCEL in the integrator, on top of tests/kick_ref.py -------------------------------------------
def advance_timesteps_rad(p, f, s, ra, active=None):
    """kick_ref.advance_timesteps with RAD_ACCEL: the criterion adds fac2 RadAccel right after the hydro term
    (timestep.c:668-671), the kick adds RadAccel dt_hydrokick to Vel and then SETS VelPred = Vel - dt_hydrokick2
    RadAccel (:497-500).  Built on kick_ref's DragAccel slot, which enters the criterion in the same place with
    the same operations (:673-677): so no DragAccel of its own, no Type-2 particle, not comoving."""
    import kick_ref as K
    assert not p["ComovingIntegrationOn"] and not p.get("pmgrid", 0)
    assert not np.any(np.asarray(s["type"]) == 2) and not np.any(s["drag"])
    ng = len(s["entropy"])
    ra = np.asarray(ra, np.float64).reshape(ng, 3)
    s["drag"][:] = ra
    res = K.advance_timesteps(p, dict(f, dust=1), s, active=active)
    s["drag"][:] = 0.
    for i in np.flatnonzero(res["kick_flag"]):
        i = int(i)
        if not (s["type"][i] == 0 and i < ng):
            continue
        binold, binnew = int(res["binold"][i]), int(s["timebin"][i])
        old_step = (1 << binold) if binold else 0
        new_step = (1 << binnew) if binnew else 0
        tcurrent = int(s["ti_begstep"][i])
        tstart = tcurrent - old_step + old_step // 2
        tend = tcurrent + new_step // 2
        dt_hk = (tend - tstart) * p["Timebase_interval"]
        dt_hk2 = (tend - tcurrent) * p["Timebase_interval"]
        for j in range(3):
            res["kick_dv"][i, j] += ra[i, j] * dt_hk
            s["vel"][i, j] = s["vel"][i, j] + ra[i, j] * dt_hk
            s["velpred"][i, j] = s["vel"][i, j] - dt_hk2 * ra[i, j]
    return res


def drift_rad(p, f, s, ra, time1):
    """kick_ref.drift with RAD_ACCEL: VelPred += RadAccel dt_hydrokick (predict.c:190-192), through kick_ref's
    DragAccel slot, which does the same operation in the same place (:195-198)"""
    import kick_ref as K
    assert not p["ComovingIntegrationOn"] and not np.any(s["drag"])
    s["drag"][:] = np.asarray(ra, np.float64).reshape(len(s["entropy"]), 3)
    rc = K.drift(p, dict(f, dust=1), s, time1)
    s["drag"][:] = 0.
    return rc


def pm_kick_rad(s, gravpm, ra, ti_current, timebase, dt_gravkick, dt_gravkickB, rad=True):
    """the particle loop of the long-range kick (timestep.c:305-345, not comoving), in place: Vel += GravPM
    dt_gravkick; VelPred of the gas rebuilt (:333-335) and, with RAD_ACCEL, then SET to Vel + RadAccel dt_hydrokick
    (:337-339)"""
    ng = len(s["entropy"])
    s["vel"] += gravpm * dt_gravkick
    tb = s["timebin"][:ng].astype(np.int64)
    dt_step = np.where(tb > 0, 1 << tb, 0)
    dt_hk = ((ti_current - (s["ti_begstep"][:ng].astype(np.int64) + dt_step // 2)) * timebase)[:, None]
    gas = (s["type"][:ng] == 0)[:, None]
    vp = s["vel"][:ng] + s["grav"][:ng] * dt_hk + s["hyd"] * dt_hk + gravpm[:ng] * dt_gravkickB
    if rad:
        vp = s["vel"][:ng] + np.asarray(ra, np.float64) * dt_hk
    s["velpred"][:] = np.where(gas, vp, s["velpred"])
