"""numpy restatement of the integrator of the shipped flag bundle (-DDUST -DDUST_TIMESTEP
-DBLACK_HOLES -DACCRETION_RADIUS -DVIRTUAL -DSFR, ADAPTIVE_GRAVSOFT_FORGAS_HSML as a switch):
advance_and_find_timesteps' particle loop (timestep.c:142-260) with get_timestep (:607-1123,
TypeOfTimestepCriterion 0) and do_the_kick (:364-605), drift_particle (predict.c:129-259), the
per-bin sums of the loop (:183-210) and the type merge of find_dt_displacement_constraint
(:1160-1172, 1190-1194).  One particle at a time, in active-list order, op by op in IEEE fp64 like
the reference's C (math.pow is the C library's pow).  With every switch off it is the minimal flag
set that the oracle's orc_advance_timesteps restates (test_kick_bundle_cpu pins the two together).

GAMMA = 7/5 (allvars.h:64); C = 2.9979e10 (allvars.h:86); TIMEBASE = 1 << 29 (allvars.h:39-41);
DRIFT_TABLE_LENGTH = 1000 (allvars.h:136)."""
import math

import numpy as np

GAMMA = 7.0 / 5.0
GAMMA_MINUS1 = GAMMA - 1
C_LIGHT = 2.9979e10
TIMEBINS = 29
TIMEBASE = 1 << TIMEBINS
TABLE = 1000


def flags(**over):
    """ghip_integration_flags as a dict: every switch off (the minimal flag set)"""
    f = dict(dust=0, dust_timestep=0, black_holes=0, accretion_radius=0, virtual_particles=0,
             OuterBoundary=0.0, AccDtBlackHole=0.0, SMBHmass=0.0, InnerBoundary=0.0, SinkBoundary=0.0,
             FeedBackVelocity=0.0, UnitVelocity_in_cm_per_s=0.0)
    f.update(over)
    return f


def bundle(**over):
    """the shipped bundle's switches with parameters of its parameter file's kind"""
    f = flags(dust=1, dust_timestep=1, black_holes=1, accretion_radius=1, virtual_particles=1,
              OuterBoundary=3.0, AccDtBlackHole=0.05, SMBHmass=1.0, InnerBoundary=0.05,
              SinkBoundary=0.01, FeedBackVelocity=0.1, UnitVelocity_in_cm_per_s=2.97837e5)
    f.update(over)
    return f


def table_factor(tab, t0, t1, p):
    """driftfac.c:123-163 (get_drift_factor; the kick factors are the same with their own table)"""
    def one(t):
        a = p["logTimeBegin"] + t * p["Timebase_interval"]
        u = (a - p["logTimeBegin"]) / (p["logTimeMax"] - p["logTimeBegin"]) * TABLE
        i = int(u)
        if i >= TABLE:
            i = TABLE - 1
        return u * tab[0] if i <= 1 else tab[i - 1] + (tab[i] - tab[i - 1]) * (u - i)
    return one(t1) - one(t0)


def _factors(p):
    """timestep.c:52-63"""
    if p["ComovingIntegrationOn"]:
        t = p["Time"]
        return dict(fac1=1 / (t * t), fac2=1 / math.pow(t, 3 * GAMMA - 2),
                    fac3=math.pow(t, 3 * (1 - GAMMA) / 2.0), hubble_a=p["hubble_a"],
                    a3inv=1 / (t * t * t), atime=t)
    return dict(fac1=1.0, fac2=1.0, fac3=1.0, hubble_a=1.0, a3inv=1.0, atime=1.0)


CRITERIA = ("accel", "dust-dt", "adaptive", "courant", "virtual", "accretion", "max", "disp")
BIN_MOVES = ("down", "same", "up", "up-blocked", "end")
KICK_LABELS = CRITERIA + BIN_MOVES + ("binold0", "entropy-add", "entropy-halve", "minegy-floor",
                                      "dtentropy-limited")


def get_timestep(i, p, f, s, F, why=None):
    """get_timestep(i, &aphys, 0): the physical step before its integer mapping, or an endrun code
    (888 / 818) as a negative int.  s: the particle state (arrays), F: _factors(p).  why: a list that
    receives the criterion (CRITERIA) whose value dt ends with -- the last assignment that held."""
    w = ["accel"]
    ty = int(s["type"][i])
    ngas = len(s["entropy"])
    gas = ty == 0 and i < ngas
    g = s["grav"][i]
    ax, ay, az = F["fac1"] * g[0], F["fac1"] * g[1], F["fac1"] * g[2]
    if ty == 0:
        hy = s["hyd"][i] if gas else np.zeros(3)
        ax += F["fac2"] * hy[0]
        ay += F["fac2"] * hy[1]
        az += F["fac2"] * hy[2]
        if f["dust"] and gas:                                           # timestep.c:673-677
            d = s["drag"][i]
            ax += F["fac2"] * d[0]
            ay += F["fac2"] * d[1]
            az += F["fac2"] * d[2]
    ac = math.sqrt(ax * ax + ay * ay + az * az)
    if ac == 0:
        ac = 1.0e-30
    soft = p["SofteningTable"][ty]
    dt = math.sqrt(2 * p["ErrTolIntAccuracy"] * F["atime"] * soft / ac)
    m = float(s["mass"][i])
    if f["dust_timestep"] and ty == 0 and m > 0:                        # timestep.c:710-722
        d = s["ddm"][i] if gas else np.zeros(3)
        ax += d[0] / m / dt
        ay += d[1] / m / dt
        az += d[2] / m / dt
        ac = math.sqrt(ax * ax + ay * ay + az * az)
        if ac > 0:              # (ac == 0: the reference reads an uninitialised dt_new; dt stays)
            dt_new = math.sqrt(2 * p["ErrTolIntAccuracy"] * F["atime"] * soft / ac)
            if dt_new < dt:
                dt = dt_new
                w[0] = "dust-dt"
    if f["dust"] and ty == 2:                                           # timestep.c:725-726
        dt = dt / 2
    if p["AdaptiveGravsoftForGasHsml"] and ty == 0:                     # timestep.c:740-743: overwrites
        dt = math.sqrt(2 * p["ErrTolIntAccuracy"] * F["atime"] * s["hsml"][i] / 2.8 / ac) \
            if ac != 0 else math.inf
        w[0] = "adaptive"
    if gas:                                                             # timestep.c:768-772
        if p["ComovingIntegrationOn"]:
            dtc = 2 * p["CourantFac"] * p["Time"] * s["hsml"][i] / (F["fac3"] * s["vsig"][i])
        else:
            dtc = 2 * p["CourantFac"] * s["hsml"][i] / s["vsig"][i]
        if dtc < dt:
            dt = dtc
            w[0] = "courant"
    if f["virtual_particles"] and ty == 3:                              # timestep.c:887-897
        dt_abs = 0.03 * f["OuterBoundary"] / C_LIGHT * f["UnitVelocity_in_cm_per_s"] * f["FeedBackVelocity"]
        dt_ff = 1.0             # (NewDensity > 0: the reference divides by an uninitialised rho)
        if dt_abs > dt_ff:
            dt_abs = dt_ff
        if dt > dt_abs:
            dt = dt_abs
            w[0] = "virtual"
    if f["black_holes"] and ty == 5:                                    # timestep.c:908-947
        dt_accr = 0.03 * (f["OuterBoundary"] / 100.)
        if f["accretion_radius"]:
            dt_a = 1.e10
            h = float(s["hsml"][i])
            if m >= 0.45 * f["SMBHmass"] and f["InnerBoundary"] > 0:
                dt_a = f["AccDtBlackHole"] * math.pow((f["InnerBoundary"] + 0.5 * h), 1.5) / math.pow(m, 0.5)
            if m < 0.45 * f["SMBHmass"] and f["SinkBoundary"] > 0:
                dt_a = f["AccDtBlackHole"] * math.pow((f["SinkBoundary"] + 0.5 * h), 1.5) / math.pow(m, 0.5)
            if dt_accr > dt_a:
                dt_accr = dt_a
        if dt_accr < dt:
            dt = dt_accr
            w[0] = "accretion"
    dt *= F["hubble_a"]                                                 # timestep.c:1044-1058
    if dt >= p["MaxSizeTimestep"]:
        dt = p["MaxSizeTimestep"]
        w[0] = "max"
    if dt >= p["dt_displacement"]:
        dt = p["dt_displacement"]
        w[0] = "disp"
    if why is not None:
        why.append(w[0])
    if dt < p["MinSizeTimestep"]:
        return -888
    ti_step = int(dt / p["Timebase_interval"])
    if not (0 < ti_step < TIMEBASE):
        return -818
    return ti_step


def state(type, mass, vel, grav, hyd, velpred, entropy, dtentropy, density, hsml, vsig, timebin,
          ti_begstep, drag=None, ddm=None):
    """copies of the particle state, shaped as the reference holds it ([n][3] vectors)"""
    n, ngas = len(type), len(entropy)
    f = lambda a, shape: np.array(a, np.float64).reshape(shape).copy()
    return dict(type=np.array(type, np.int32), mass=f(mass, n), vel=f(vel, (n, 3)), grav=f(grav, (n, 3)),
                hyd=f(hyd, (ngas, 3)), velpred=f(velpred, (ngas, 3)), entropy=f(entropy, ngas),
                dtentropy=f(dtentropy, ngas), density=f(density, ngas), hsml=f(hsml, n), vsig=f(vsig, ngas),
                timebin=np.array(timebin, np.int32), ti_begstep=np.array(ti_begstep, np.int32),
                drag=np.zeros((ngas, 3)) if drag is None else f(drag, (ngas, 3)),
                ddm=np.zeros((ngas, 3)) if ddm is None else f(ddm, (ngas, 3)))


def advance_timesteps(p, f, s, active=None, tables=None, trace=None):
    """the loop of timestep.c:142-260 on the state s (modified in place).  p: the kick parameters
    (names of ghip_kick_params, SofteningTable a sequence, TimeBinActive a bit mask), f: flags(),
    tables: (gravkick, hydrokick) when comoving.  Returns dict(rc, kick_dv [n][3], kick_flag [n],
    binold [n]) -- rc 0 or the endrun code of the first failing particle in list order.
    trace: a dict that receives, per particle of the list that passed the checks, the set of labels
    (KICK_LABELS) of what the loop did with it: the criterion that set dt, the bin move ("end": the
    Ti_Current >= TIMEBASE block), "binold0", and for gas which way Entropy went (:553-557), the
    MinEgySpec floor (:574-583) and the DtEntropy limiter (:590-593)."""
    n, ngas = len(s["type"]), len(s["entropy"])
    F = _factors(p)
    kick_dv = np.zeros((n, 3))
    kick_flag = np.zeros(n, np.int32)
    binold_all = s["timebin"].copy()
    rc = 0
    for i in (range(n) if active is None else active):
        i = int(i)
        ty = int(s["type"][i])
        gas = ty == 0 and i < ngas
        why = []
        ti_step = get_timestep(i, p, f, s, F, why)
        if ti_step < 0:
            rc = rc or -ti_step
            continue
        ti_min = TIMEBASE                                               # timestep.c:148-152
        while ti_min > ti_step:
            ti_min >>= 1
        ti_step = ti_min
        if ti_step == 1:
            rc = rc or 112313
            continue
        bin = ti_step.bit_length() - 1 if ti_step else 0
        binold = int(s["timebin"][i])
        move = "down" if bin < binold else "same" if bin == binold else "up"
        if bin > binold and not (p["TimeBinActive"] >> bin) & 1:
            bin = binold
            ti_step = (1 << bin) if bin else 0
            move = "up-blocked"
        if p["Ti_Current"] >= TIMEBASE:
            ti_step = bin = 0
            move = "end"
        if TIMEBASE - p["Ti_Current"] < ti_step:
            rc = rc or 888
            continue
        lab = {why[0], move}
        if binold == 0:
            lab.add("binold0")
        if trace is not None:
            trace[i] = lab
        s["timebin"][i] = bin
        ti_step_old = (1 << binold) if binold else 0
        tb0 = int(s["ti_begstep"][i])
        tstart = tb0 + ti_step_old // 2
        tend = tb0 + ti_step_old + ti_step // 2
        tcurrent = tb0 + ti_step_old
        s["ti_begstep"][i] = tcurrent
        # ---- do_the_kick ----
        if f["virtual_particles"] and ty == 3:                          # timestep.c:375-377
            continue
        if p["ComovingIntegrationOn"]:
            gk, hk = tables
            dt_entr = (tend - tstart) * p["Timebase_interval"]
            dt_gk = table_factor(gk, tstart, tend, p)
            dt_hk = table_factor(hk, tstart, tend, p)
            dt_gk2 = table_factor(gk, tcurrent, tend, p)
            dt_hk2 = table_factor(hk, tcurrent, tend, p)
        else:
            dt_entr = dt_gk = dt_hk = (tend - tstart) * p["Timebase_interval"]
            dt_gk2 = dt_hk2 = (tend - tcurrent) * p["Timebase_interval"]
        g = s["grav"][i]
        dv = [g[j] * dt_gk for j in range(3)]                           # timestep.c:407-424
        if f["dust"] and ty == 2:
            dv = [0.0, 0.0, 0.0]
        for j in range(3):
            s["vel"][i, j] = s["vel"][i, j] + dv[j]
        if gas:
            hy = s["hyd"][i]
            for j in range(3):                                          # timestep.c:488-513
                dv[j] += hy[j] * dt_hk
                s["vel"][i, j] = s["vel"][i, j] + hy[j] * dt_hk
                s["velpred"][i, j] = s["vel"][i, j] - dt_gk2 * g[j] - dt_hk2 * hy[j]
                if f["dust"]:
                    s["drag"][i, j] = 0.
            A, dA = float(s["entropy"][i]), float(s["dtentropy"][i])
            if dA * dt_entr > -0.5 * A:                                 # timestep.c:553-557
                A += dA * dt_entr
                lab.add("entropy-add")
            else:
                A *= 0.5
                lab.add("entropy-halve")
            if p["MinEgySpec"]:                                         # timestep.c:574-583
                minentropy = p["MinEgySpec"] * GAMMA_MINUS1 / math.pow(s["density"][i] * F["a3inv"],
                                                                       GAMMA_MINUS1)
                if A < minentropy:
                    A, dA = minentropy, 0.0
                    lab.add("minegy-floor")
            dt_entr = ((1 << bin) if bin else 0) // 2 * p["Timebase_interval"]   # timestep.c:590-593
            if A + dA * dt_entr < 0.5 * A:
                dA = -0.5 * A / dt_entr
                lab.add("dtentropy-limited")
            s["entropy"][i], s["dtentropy"][i] = A, dA
        kick_dv[i] = dv                                                 # force_kick_node(i, dv)
        kick_flag[i] = 1
    return dict(rc=rc, kick_dv=kick_dv, kick_flag=kick_flag, binold=binold_all)


def drift(p, f, s, time1, tables=None):
    """drift_particle(i, time1) for every particle (predict.c:129-259), in place.  p: Timebase_interval,
    ComovingIntegrationOn, logTimeBegin, logTimeMax, MinGasHsml; s also carries pos, ti_current,
    divvel, pressure.  tables: (drift, gravkick, hydrokick) when comoving.  Returns 0 or 12."""
    ngas = len(s["entropy"])
    for i in range(len(s["type"])):
        ty = int(s["type"][i])
        if f["virtual_particles"] and ty == 3:                          # predict.c:134-136
            continue
        time0 = int(s["ti_current"][i])
        if time1 < time0:
            return 12
        if time1 == time0:
            continue
        if p["ComovingIntegrationOn"]:
            dt_drift = table_factor(tables[0], time0, time1, p)
            dt_gk = table_factor(tables[1], time0, time1, p)
            dt_hk = table_factor(tables[2], time0, time1, p)
        else:
            dt_drift = dt_gk = dt_hk = (time1 - time0) * p["Timebase_interval"]
        for j in range(3):
            s["pos"][i, j] += s["vel"][i, j] * dt_drift
        if ty == 0 and i < ngas:
            for j in range(3):
                s["velpred"][i, j] += s["grav"][i, j] * dt_gk + s["hyd"][i, j] * dt_hk
            if f["dust"]:                                               # predict.c:195-198
                for j in range(3):
                    s["velpred"][i, j] += s["drag"][i, j] * dt_hk
            dvv = s["divvel"][i]
            s["density"][i] *= math.exp(-dvv * dt_drift)
            h = s["hsml"][i] * math.exp(0.333333333333 * dvv * dt_drift)
            if h < p["MinGasHsml"]:
                h = p["MinGasHsml"]
            s["hsml"][i] = h
            tb = int(s["timebin"][i])
            dt_step = (1 << tb) if tb else 0
            dt_entr = (time1 - (int(s["ti_begstep"][i]) + dt_step // 2)) * p["Timebase_interval"]
            s["pressure"][i] = (s["entropy"][i] + s["dtentropy"][i] * dt_entr) * math.pow(s["density"][i], GAMMA)
        s["ti_current"][i] = time1
    if p.get("box_wrap"):
        box_wrap(s["pos"], p["BoxSize"])
    return 0


def box_wrap(pos, boxsize):
    """do_box_wrapping (predict.c:282-310) for every particle, in place: the two loops of :299-307.  They end
    only for finite coordinates of a moderate number of boxes."""
    for i in range(len(pos)):
        for j in range(3):
            x = float(pos[i, j])
            while x < 0:
                x += boxsize
            while x >= boxsize:
                x -= boxsize
            pos[i, j] = x


def bin_sums(order, ptype, binold, binnew, sfr=None, dust_mass=None, total_mass=None, mass=None,
             TimeBinSfr=None, TimeBin_BH_mass=None, TimeBin_BH_dynamicalmass=None, TimeBin_BH_Mdot=None):
    """timestep.c:183-210, in list order, where the bin changed (in place).  SFR: TimeBinSfr from the
    gas's Sfr; BLACK_HOLES + DUST: the three sink sums from Dust_Mass, Total_Mass and Mass."""
    for i in order:
        i = int(i)
        b0, b1 = int(binold[i]), int(binnew[i])
        if b0 == b1:
            continue
        if ptype[i] == 0 and TimeBinSfr is not None:
            TimeBinSfr[b0] -= sfr[i]
            TimeBinSfr[b1] += sfr[i]
        if ptype[i] == 5 and TimeBin_BH_mass is not None:
            TimeBin_BH_mass[b0] -= dust_mass[i]
            TimeBin_BH_dynamicalmass[b0] -= total_mass[i]
            TimeBin_BH_Mdot[b0] -= mass[i]
            TimeBin_BH_mass[b1] += dust_mass[i]
            TimeBin_BH_dynamicalmass[b1] += total_mass[i]
            TimeBin_BH_Mdot[b1] += mass[i]


def merge_displacement_sums(v_sum, count_sum, min_mass, sfr, black_holes):
    """timestep.c:1160-1172: under SFR gas and stars share one sum; under BLACK_HOLES as well the
    sinks, which take the gas's smallest mass.  Returns copies."""
    v, c, m = [float(x) for x in v_sum], [int(x) for x in count_sum], [float(x) for x in min_mass]
    if sfr:
        v[0] += v[4]
        c[0] += c[4]
        v[4] = v[0]
        c[4] = c[0]
        if black_holes:
            v[0] += v[5]
            c[0] += c[5]
            v[5] = v[0]
            c[5] = c[0]
            m[5] = m[0]
    return v, c, m
