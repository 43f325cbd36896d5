"""The sink (black-hole) passes of the shipped flag bundle restated directly from the reference's C
text, all pairs: every sink against all N particles, plain numpy, no tree, no neighbour search and
no import of the oracle or of the library.  Written from

    blackhole.c:794-1190    blackhole_evaluate          -> evaluate()
    blackhole.c:1201-1346   blackhole_evaluate_swallow  -> swallow()
    blackhole.c:528-532     its caller's filter            (a sink whose own SwallowID is not 0 is passed over)
    blackhole.c:1351-1474   ngb_treefind_blackhole         (types 0, 5 and, with DUST, 2; r2 <= h^2)
    density.c:521-652, 831-886, 972-978   the BLACK_HOLES branches of density()   -> sink_density()

Every per-pair decision is taken with the same fp64 expression as the C text (pow(r2, 0.5), r + 1.e-20,
the nearest image by the two comparisons of :896-907); every SUM (density, neighbour number, injected
energy, accreted mass and momentum) is accumulated in np.longdouble and rounded to fp64 once, so the
restatement carries no summation-order error of its own (MyLongDouble in the reference).

Two deviations from the C text are kept, because the project takes them on purpose (ghip_sink.hip,
gadget_oracle.c):
  (1) a victim claimed by several sinks goes to the LARGEST ID for all three kinds.  The reference says
      so for gas (:1071, 1092, 1111) and lets the last sink of the active list win for dust and sinks
      (:988-991, 1030), a result that depends on the list order.  evaluate(rule="last") and
      evaluate(rule="first") apply those other rules to ALL kinds; they exist only so that a test can show
      that its inputs tell the rules apart.
  (2) e_tot of a dust grain uses the grain's own r = sqrt(r2); the reference reads `r` there (:1024) before
      any assignment in that iteration.
"""
import numpy as np

KERNEL_COEFF_1 = 2.546479089470
KERNEL_COEFF_2 = 15.278874536822
KERNEL_COEFF_5 = 5.092958178941
NORM_COEFF = 4.188790204786
LD = np.longdouble


def _nearest(pos_i, pos, box, periodic):
    """dx = pos[0] - P[j].Pos[0] ... with the two comparisons of the C text; returns (dx, dy, dz, r2)"""
    d = pos_i[None, :] - pos
    if periodic:
        half = 0.5 * box
        d = np.where(d > half, d - box, d)
        d = np.where(d < -half, d + box, d)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    return dx, dy, dz, dx * dx + dy * dy + dz * dz


def _wk(r, h):
    """wk and hinv3 as density.c:859-871 / blackhole.c:1042-1055 form them"""
    hinv = 1.0 / h
    hinv3 = hinv * hinv * hinv
    u = r * hinv
    wk = np.where(u < 0.5, hinv3 * (KERNEL_COEFF_1 + KERNEL_COEFF_2 * (u - 1) * u * u),
                  hinv3 * KERNEL_COEFF_5 * (1.0 - u) * (1.0 - u) * (1.0 - u))
    return wk, hinv3


def _ldsum(x):
    return np.sum(np.asarray(x, np.float64).astype(LD), dtype=LD)


# ------------------------------------------------------------------------------------------------
# density() for Type-5 targets
# ------------------------------------------------------------------------------------------------
def sink_density(pos, mass, typ, velpred, entropy, sinks, hsml, des_ngb, ngb_factor, max_dev, min_gas_hsml,
                 box, periodic, maxiter=150):
    """The h iteration of density() for the sinks `sinks` against the gas (Type 0, Mass != 0:
    density.c:831-834), wanting DesNumNgb * BlackHoleNgbFactor neighbours (:548-551), without the Newton
    step (gas only, :612, 629).  hsml [n]: the first guesses at the sinks' indices.

    Returns dict(hsml [n], numngb, density, entropy, gasvel [nsink], iterations, passes [nsink],
    h_tried (per sink the h of every pass), branches): branches[a] is the set of iteration branches sink a took --
        "shrink"  h /= 1.26            (:627-641)        "grow"    h *= 1.26            (:610-624)
        "bisect"  Left, Right > 0      (:597-598)        "exit1e-3" (Right - Left) < 1e-3 Left (:566-573)
        "clamp"   h < MinGasHsml reset (:645-646)        "minh"    too many neighbours but h <= 1.01 MinGasHsml:
        "rho0"    a pass with no gas inside h (:524 false)          accepted by the second half of :559-561
    """
    pos = np.asarray(pos, np.float64)
    gas = np.where(np.asarray(typ) == 0)[0]
    gpos, gmass = pos[gas], np.asarray(mass, np.float64)[gas]
    gvel, gent = np.asarray(velpred, np.float64)[gas], np.asarray(entropy, np.float64)[gas]
    ns = len(sinks)
    h_all = np.asarray(hsml, np.float64).copy()
    out = dict(numngb=np.zeros(ns), density=np.zeros(ns), entropy=np.zeros(ns), gasvel=np.zeros((ns, 3)),
               passes=np.zeros(ns, np.int64), branches=[set() for _ in range(ns)],
               h_tried=[[] for _ in range(ns)])
    left, right = np.zeros(ns), np.zeros(ns)
    done = np.zeros(ns, bool)
    desnumngb = des_ngb * ngb_factor
    it = 0
    while True:
        npleft = 0
        for a, i in enumerate(sinks):
            if done[a]:
                continue
            br = out["branches"][a]
            out["passes"][a] += 1
            h = float(h_all[i])
            h2 = h * h
            out["h_tried"][a].append(h)
            _, _, _, r2 = _nearest(pos[i], gpos, box, periodic)
            m = (gmass != 0) & (r2 < h2)
            wk, hinv3 = _wk(np.sqrt(r2[m]), h)
            mj = gmass[m]
            rho = float(_ldsum(mj * wk))
            wn = float(_ldsum(NORM_COEFF * wk / hinv3))
            se = float(_ldsum(mj * wk * gent[m]))
            gv = [float(_ldsum(mj * wk * gvel[m, k])) for k in range(3)]
            if rho > 0:                                              # :524-530
                se /= rho
                gv = [v / rho for v in gv]
            else:
                br.add("rho0")
            out["numngb"][a], out["density"][a], out["entropy"][a] = wn, rho, se
            out["gasvel"][a] = gv
            few = wn < (desnumngb - max_dev)
            many = wn > (desnumngb + max_dev)
            if few or (many and h > (1.01 * min_gas_hsml)):          # :559-561
                npleft += 1
                if left[a] > 0 and right[a] > 0 and (right[a] - left[a]) < 1.0e-3 * left[a]:
                    npleft -= 1                                      # "this one should be ok"
                    done[a] = True
                    br.add("exit1e-3")
                    continue
                if few:
                    left[a] = max(h, left[a])
                elif right[a] != 0:
                    if h < right[a]:
                        right[a] = h
                else:
                    right[a] = h
                if right[a] > 0 and left[a] > 0:
                    h = (0.5 * (left[a] ** 3 + right[a] ** 3)) ** (1.0 / 3)
                    br.add("bisect")
                else:
                    if right[a] == 0 and left[a] > 0:
                        h *= 1.26
                        br.add("grow")
                    if right[a] > 0 and left[a] == 0:
                        h /= 1.26
                        br.add("shrink")
                if h < min_gas_hsml:
                    h = min_gas_hsml
                    br.add("clamp")
                h_all[i] = h
            else:
                if many:
                    br.add("minh")
                done[a] = True
        if npleft > 0:
            it += 1
            if it > maxiter:
                it = -1
                break
        else:
            break
    out["hsml"] = h_all
    out["iterations"] = it
    return out


# ------------------------------------------------------------------------------------------------
# blackhole_evaluate
# ------------------------------------------------------------------------------------------------
def _candidate_types(typ, dust):
    ok = (typ == 0) | (typ == 5)
    return ok | (typ == 2) if dust else ok


def claims(pos, vel, mass, typ, sinks, hsml, gas_density, par):
    """What each sink of the list wants: a list, in list order, of dict(sink=a, victims, kind-wise
    near-misses).  victims: particle indices the sink would mark.  `refused_unbound`: grains inside the
    accretion boundary with e_tot > 0 (:1030 false); `refused_heavier`: sinks inside the boundary that
    are heavier than this one (:988 false)."""
    pos, vel = np.asarray(pos, np.float64), np.asarray(vel, np.float64)
    mass, typ = np.asarray(mass, np.float64), np.asarray(typ)
    n = len(mass)
    gd = np.zeros(n)
    gd[:len(gas_density)] = gas_density
    cand_t = _candidate_types(typ, par.dust)
    out = []
    for a, i in enumerate(sinks):
        m_i, h = float(mass[i]), float(hsml[i])
        rec = dict(sink=a, victims=np.zeros(0, np.int64), refused_unbound=np.zeros(0, np.int64),
                   refused_heavier=np.zeros(0, np.int64), gas=np.zeros(0, np.int64), r=None)
        out.append(rec)
        if not m_i > 0:                                              # :890
            continue
        _, _, _, r2 = _nearest(pos[i], pos, par.BoxSize, par.periodic)
        inh = cand_t & (mass > 0) & (r2 < h * h)                     # :888, 911 (and :1392)
        w = vel - vel[i][None, :]
        vrel = np.sqrt(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2]) / par.ascale
        central = m_i > 0.95 * par.SMBHmass
        pr2 = np.power(r2, 0.5)
        r = np.sqrt(r2)
        # sinks, :934-1001
        inb = inh & (typ == 5) & (r2 > 0) & ~(pr2 > (par.InnerBoundary if central else par.SofteningBndry))
        bh = inb & (mass <= m_i)
        rec["refused_heavier"] = np.where(inb & ~(mass <= m_i))[0]
        # dust, :1005-1033 (deviation 2: the grain's own r)
        du = np.zeros(n, bool)
        if par.dust:
            inb = inh & (typ == 2) & (r2 > 0) & (pr2 < (par.InnerBoundary if central else par.SinkBoundary))
            etot = vrel * vrel / 2. - m_i / (r + 1.e-20)
            du = inb & (etot <= 0.)
            rec["refused_unbound"] = np.where(inb & ~(etot <= 0.))[0]
        # gas, :1038-1116
        g = inh & (typ == 0)
        etot = vrel * vrel / 2. - m_i / (r + 1.e-20)
        if central:
            ga = g & (r < par.InnerBoundary)
        elif par.accretion_of_dust_only:
            ga = np.zeros(n, bool)
        else:
            ga = g & (r < par.SinkBoundary) & ((gd >= par.CritDensity) if par.accretion_density else (etot < 0.))
        rec["victims"] = np.where(bh | du | ga)[0]
        rec["gas"] = np.where(g)[0]
        rec["r"] = r
    return out


def evaluate(pos, vel, mass, typ, ids, sinks, hsml, timebin, mdot, bh_density, gas_density, par, rule="max",
             swallow_id=None, injected=None):
    """blackhole_evaluate over the sinks in list order -> (swallow_id [n] uint32, injected [ngas]).
    rule: "max" -- the largest ID wins (the project's rule, deviation 1); "last" / "first" -- the last /
    the first claiming sink of the list wins."""
    assert rule in ("max", "last", "first")
    mass = np.asarray(mass, np.float64)
    n, ngas = len(mass), len(gas_density)
    sw = np.zeros(n, np.uint32) if swallow_id is None else np.asarray(swallow_id, np.uint32).copy()
    inj = np.zeros(ngas, LD)
    if injected is not None:
        inj += np.asarray(injected, np.float64)
    for rec in claims(pos, vel, mass, typ, sinks, hsml, gas_density, par):
        a = rec["sink"]
        i = sinks[a]
        v = rec["victims"]
        myid = np.uint32(ids[i])
        if rule == "max":
            sw[v] = np.maximum(sw[v], myid)
        elif rule == "last":
            sw[v] = myid
        else:
            v = v[sw[v] == 0]
            sw[v] = myid
        g = rec["gas"]
        if len(g):
            m_i, h = float(mass[i]), float(hsml[i])
            tb = int(timebin[i])
            dt = ((1 << tb) if tb else 0) * par.dt_fac              # :822
            energy = 0.
            if m_i < 0.95 * par.SMBHmass:                            # :1144-1149
                energy = par.FeedbackCoeff * (m_i * par.UnitMass_in_g) ** 0.6667 * mdot[a] * \
                    par.UnitMass_in_g * dt
            wk, _ = _wk(rec["r"][g], h)
            inj[g] += energy * mass[g] * wk / bh_density[a]          # :1154
    return sw, inj.astype(np.float64)


# ------------------------------------------------------------------------------------------------
# blackhole_evaluate_swallow under the filter of its caller
# ------------------------------------------------------------------------------------------------
def swallow(pos, vel, mass, typ, ids, sinks, hsml, swallow_id, bh_mass, par):
    """The swallow pass of blackhole_accretion(): for each sink of the list whose OWN SwallowID is 0
    (blackhole.c:528-532) every particle inside its search sphere that carries its ID is swallowed.  A sink
    that was itself claimed does nothing and reports zero sums -- what the union members hold after the
    reset of :713.  mass and bh_mass [n] are not modified; the results are returned:
    dict(acc_mass, acc_bhmass, acc_dustmass [nsink], acc_momentum [nsink][3], counts [3] = gas, sinks,
    dust, mass [n], bh_mass [n], skipped [nsink] bool, swallowed [n] bool)."""
    pos, vel = np.asarray(pos, np.float64), np.asarray(vel, np.float64)
    mass = np.asarray(mass, np.float64).copy()
    pbh = np.asarray(bh_mass, np.float64).copy()
    typ, sw = np.asarray(typ), np.asarray(swallow_id, np.uint32)
    ns = len(sinks)
    out = dict(acc_mass=np.zeros(ns), acc_bhmass=np.zeros(ns), acc_dustmass=np.zeros(ns),
               acc_momentum=np.zeros((ns, 3)), counts=np.zeros(3, np.int64), skipped=np.zeros(ns, bool),
               swallowed=np.zeros(len(mass), bool))
    cand_t = _candidate_types(typ, par.dust)
    for a, i in enumerate(sinks):
        if sw[i] != 0:                                               # :530
            out["skipped"][a] = True
            continue
        h = float(hsml[i])
        _, _, _, r2 = _nearest(pos[i], pos, par.BoxSize, par.periodic)
        v = np.where(cand_t & ~(r2 > h * h) & (sw == np.uint32(ids[i])))[0]      # :1392, 1255
        out["acc_mass"][a] = float(_ldsum(mass[v]))
        out["acc_bhmass"][a] = float(_ldsum(pbh[v[typ[v] == 5]]))
        out["acc_dustmass"][a] = float(_ldsum(mass[v[typ[v] == 2]]))
        for k in range(3):
            out["acc_momentum"][a, k] = float(_ldsum(mass[v] * vel[v, k]))
        out["counts"] += [(typ[v] == 0).sum(), (typ[v] == 5).sum(), (typ[v] == 2).sum()]
        mass[v] = 0
        pbh[v[typ[v] == 5]] = 0
        out["swallowed"][v] = True
    out["mass"], out["bh_mass"] = mass, pbh
    return out
