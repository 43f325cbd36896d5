"""density() for gas targets restated directly from the reference's C text, all pairs: every target against
every gas particle, plain numpy, no tree, no neighbour search and no import of the oracle or of the library
(hiter_case below, which builds the inputs, imports tests/common.py).  Written from

    density.c:711-1029   density_evaluate, mode 0, the plain-SPH members      -> _sums()
    density.c:831-834    the massless-gas rule (bit 0 of the oracle's set_massless_gas_rule)
    density.c:434-652    finalisation and the smoothing-length update         -> gas_density()

Every per-pair expression is the fp64 expression of the C text (the nearest image by the two comparisons of
:896-907); every SUM (rho, the weighted neighbour number, the dh term, div v, the three curl components) is
accumulated in np.longdouble and rounded to fp64 once, so the restatement carries no summation-order error of
its own.  The h rule is applied literally, one target at a time, the Newton step of :612 / :629 included, and
every branch a target takes is recorded under a label:

    accept         accepted inside the window              minh           too many neighbours but h <= 1.01 MinGasHsml
    exit1e-3       (Right - Left) < 1e-3 Left (:566-573)   few            too few neighbours (Left moves up)
    many-first     too many, Right was 0                   many-lower     too many, h < Right (Right moves down)
    many-keep      too many, h >= Right (Right stays)      bisect         Left, Right > 0: the cube mean
    grow-newton    Newton step up, fac < 1.26              grow-capped    Newton step up, capped at 1.26
    grow-far       |numngb - des| >= 0.5 des: h * 1.26     shrink-newton  Newton step down, fac > 1 / 1.26
    shrink-capped  Newton step down, capped at 1 / 1.26    shrink-far     |numngb - des| >= 0.5 des: h / 1.26
    clamp          the new h < MinGasHsml, reset to it     dhf-guard      dhf <= -0.9: DhsmlDensityFactor = 1
    rho0           a pass with rho == 0 (dhf stays the raw sum)

`many-keep` needs a too-many pass at h >= Right.  Right is only ever set to an h that had too many neighbours,
and every h that follows it is smaller: a bisection gives Left < h < Right, a step down multiplies h by
fac = 1 - (numngb - des) / (3 numngb) * dhf < 1 (dhf = 1 / (1 + x) > 0 for x > -0.9, else 1) or by 1 / 1.26, and a
reset to MinGasHsml ends with h <= 1.01 MinGasHsml, which accepts.  The one way to it is a target with rho == 0
(all neighbours massless) and too many neighbours: its raw dhf is 0, fac is 1, h never moves and the iteration
runs into MAXITER -- an input that fails rather than a branch that can be compared.  The label is kept because
the text has the branch; tests/test_density_hiter_cpu.py asserts that no terminating input carries it.
"""
import math

import numpy as np

KERNEL_COEFF_1 = 2.546479089470
KERNEL_COEFF_2 = 15.278874536822
KERNEL_COEFF_3 = 45.836623610466
KERNEL_COEFF_4 = 30.557749073644
KERNEL_COEFF_5 = 5.092958178941
KERNEL_COEFF_6 = -15.278874536822
NORM_COEFF = 4.188790204786
NUMDIMS = 3
GAMMA = 7.0 / 5.0
LD = np.longdouble

FIELDS = ("hsml", "numngb", "density", "dhsmlfac", "divvel", "curlvel", "pressure")
LABELS = ("accept", "minh", "exit1e-3", "few", "many-first", "many-lower", "many-keep", "bisect",
          "grow-newton", "grow-capped", "grow-far", "shrink-newton", "shrink-capped", "shrink-far",
          "clamp", "dhf-guard", "rho0")
UNREACHABLE = ("many-keep",)          # see the module text
CASES = ("base", "tight", "minh", "clamp", "small", "large", "mixed", "massless", "subset")
MARGIN = 1e-10


def _ldsum(x, m):
    return np.where(m, x, 0.0).astype(LD).sum(axis=1, dtype=LD).astype(np.float64)


def _sums(tpos, tvel, h, gpos, gvel, gmass, box, periodic, rule):
    """density_evaluate for the targets (tpos, tvel, h) against all gas -> the seven sums [nt][7] as fp64 and
    the number of neighbours with r2 < h2 per target (what the reference's loop counts as numngb)"""
    d = tpos[:, None, :] - gpos[None, :, :]
    if periodic:
        half = 0.5 * box
        d = np.where(d > half, d - box, d)
        d = np.where(d < -half, d + box, d)
    dx, dy, dz = d[:, :, 0], d[:, :, 1], d[:, :, 2]
    r2 = dx * dx + dy * dy + dz * dz
    h = h[:, None]
    m = r2 < h * h
    if rule & 1:
        m &= (gmass != 0)[None, :]
    hinv = 1.0 / h
    hinv3 = hinv * hinv * hinv
    hinv4 = hinv3 * hinv
    r = np.sqrt(r2)
    u = r * hinv
    with np.errstate(all="ignore"):
        wk = np.where(u < 0.5, hinv3 * (KERNEL_COEFF_1 + KERNEL_COEFF_2 * (u - 1) * u * u),
                      hinv3 * KERNEL_COEFF_5 * (1.0 - u) * (1.0 - u) * (1.0 - u))
        dwk = np.where(u < 0.5, hinv4 * u * (KERNEL_COEFF_3 * u - KERNEL_COEFF_4),
                       hinv4 * KERNEL_COEFF_6 * (1.0 - u) * (1.0 - u))
        mj = gmass[None, :]
        fac = np.where(r > 0, mj * dwk / np.where(r > 0, r, 1.0), 0.0)
    dv = tvel[:, None, :] - gvel[None, :, :]
    dvx, dvy, dvz = dv[:, :, 0], dv[:, :, 1], dv[:, :, 2]
    out = np.empty((len(tpos), 7))
    out[:, 0] = _ldsum(mj * wk, m)
    out[:, 1] = _ldsum(NORM_COEFF * wk / hinv3, m)
    out[:, 2] = _ldsum(-mj * (NUMDIMS * hinv * wk + u * dwk), m)
    out[:, 3] = _ldsum(-fac * (dx * dvx + dy * dvy + dz * dvz), m)
    out[:, 4] = _ldsum(fac * (dz * dvy - dy * dvz), m)
    out[:, 5] = _ldsum(fac * (dx * dvz - dz * dvx), m)
    out[:, 6] = _ldsum(fac * (dy * dvx - dx * dvy), m)
    return out, m.sum(axis=1)


def gas_density(pos, mass, typ, velpred, entropy, dtentropy, timebin, ti_begstep, hsml, active, des_ngb,
                max_dev, min_gas_hsml, box, periodic, ti_current, timebase, rule=0, maxiter=150):
    """density() for the gas targets `active` (indices < ngas = len(entropy); None: all gas).  hsml [n]: the
    first guesses.  rule: the massless-gas rule (bit 0: gas of mass 0 is nobody's neighbour).

    Returns dict(hsml, numngb, density, dhsmlfac, divvel, curlvel, pressure [n]: the targets' entries are
    results, the others hsml's input and zeros; passes, margin [n]; h_tried, branches (per particle: the h of
    every pass, the set of labels); iterations: the count of density(), -1 past maxiter; visits: neighbours with
    r2 < h2 over all passes).  margin: the smallest relative distance of any comparison the target made from its
    threshold -- numngb from both window edges (of DesNumNgb), (R - L) from 1e-3 L (of L), fac from 1.26 or
    1 / 1.26, |numngb - des| from 0.5 des (of des), dhf from -0.9, h from 1.01 MinGasHsml and the new h from
    MinGasHsml; an h that IS MinGasHsml because it was reset to it counts as 1."""
    pos = np.asarray(pos, np.float64)
    n, ngas = len(pos), len(entropy)
    assert np.all(np.asarray(typ)[:ngas] == 0), "the gas block comes first"
    gpos, gmass = pos[:ngas], np.asarray(mass, np.float64)[:ngas]
    gvel = np.asarray(velpred, np.float64)
    active = np.arange(ngas) if active is None else np.asarray(active, np.int64)
    out = {k: np.zeros(n) for k in FIELDS}
    out["hsml"] = np.asarray(hsml, np.float64).copy()
    out.update(passes=np.zeros(n, np.int64), margin=np.full(n, np.inf), h_tried=[[] for _ in range(n)],
               branches=[set() for _ in range(n)])
    hs = out["hsml"]
    left, right = np.zeros(n), np.zeros(n)
    done = np.ones(n, bool)
    done[active] = False
    lo, hi, mn = des_ngb - max_dev, des_ngb + max_dev, float(min_gas_hsml)
    it, visits = 0, 0

    def near(i, x, thr, scale):
        out["margin"][i] = min(out["margin"][i], abs(x - thr) / scale)

    def newton(i, numngb, dhf, br, up):
        if abs(numngb - des_ngb) < 0.5 * des_ngb:
            near(i, abs(numngb - des_ngb), 0.5 * des_ngb, des_ngb)
            fac = 1 - (numngb - des_ngb) / (NUMDIMS * numngb) * dhf
            cap = 1.26 if up else 1 / 1.26
            near(i, fac, cap, cap)
            if (fac < 1.26) if up else (fac > 1 / 1.26):
                br.add("grow-newton" if up else "shrink-newton")
                return hs[i] * fac
            br.add("grow-capped" if up else "shrink-capped")
        else:
            near(i, abs(numngb - des_ngb), 0.5 * des_ngb, des_ngb)
            br.add("grow-far" if up else "shrink-far")
        return hs[i] * 1.26 if up else hs[i] / 1.26

    while True:
        todo = np.where(~done)[0]
        sums, cnt = _sums(gpos[todo], gvel[todo], hs[todo], gpos, gvel, gmass, box, periodic, rule)
        visits += int(cnt.sum())
        npleft = 0
        for a, i in enumerate(todo):
            br = out["branches"][i]
            h = float(hs[i])
            out["passes"][i] += 1
            out["h_tried"][i].append(h)
            rho, numngb, dhf, divv = (float(x) for x in sums[a, :4])
            rot = [float(x) for x in sums[a, 4:]]
            curl = 0.0
            if rho > 0:                                              # :436-452
                dhf *= h / (NUMDIMS * rho)
                near(i, dhf, -0.9, 0.9)
                if dhf > -0.9:
                    dhf = 1 / (1 + dhf)
                else:
                    dhf = 1.0
                    br.add("dhf-guard")
                curl = math.sqrt(rot[0] * rot[0] + rot[1] * rot[1] + rot[2] * rot[2]) / rho
                divv /= rho
            else:
                br.add("rho0")
            tb = int(timebin[i])
            dt_step = (1 << tb) if tb else 0
            dt_entr = (ti_current - (int(ti_begstep[i]) + dt_step // 2)) * timebase        # :487-496
            out["numngb"][i], out["density"][i], out["dhsmlfac"][i] = numngb, rho, dhf
            out["divvel"][i], out["curlvel"][i] = divv, curl
            out["pressure"][i] = (entropy[i] + dtentropy[i] * dt_entr) * math.pow(rho, GAMMA)
            near(i, numngb, lo, des_ngb)
            near(i, numngb, hi, des_ngb)
            few, many = numngb < lo, numngb > hi
            if many and mn > 0:
                out["margin"][i] = min(out["margin"][i], 1.0 if h == mn else abs(h - 1.01 * mn) / (1.01 * mn))
            if few or (many and h > (1.01 * mn)):                    # :559-561
                npleft += 1
                L, R = left[i], right[i]
                if L > 0 and R > 0:
                    near(i, R - L, 1.0e-3 * L, L)
                    if (R - L) < 1.0e-3 * L:                         # :566-573
                        npleft -= 1
                        done[i] = True
                        br.add("exit1e-3")
                        continue
                if few:
                    br.add("few")
                    L = max(h, L)
                elif R != 0:
                    if h < R:
                        R = h
                        br.add("many-lower")
                    else:
                        br.add("many-keep")
                else:
                    R = h
                    br.add("many-first")
                hnew = h
                if R > 0 and L > 0:
                    hnew = math.pow(0.5 * (math.pow(L, 3) + math.pow(R, 3)), 1.0 / 3)
                    br.add("bisect")
                else:
                    if R == 0 and L > 0:
                        hnew = newton(i, numngb, dhf, br, True)
                    if R > 0 and L == 0:
                        hnew = newton(i, numngb, dhf, br, False)
                if mn > 0:
                    near(i, hnew, mn, mn)
                if hnew < mn:
                    hnew = mn
                    br.add("clamp")
                left[i], right[i], hs[i] = L, R, hnew
            else:
                br.add("minh" if many else "accept")
                done[i] = True
        if npleft > 0:
            it += 1
            if it > maxiter:
                it = -1
                break
        else:
            break
    out["iterations"], out["visits"] = it, visits
    return out


def reference(pr):
    """gas_density on a case of hiter_case"""
    ic = pr.ic
    return gas_density(ic["pos"], ic["mass"], ic["type"], pr.velpred, pr.entropy, pr.dtentropy, pr.timebin,
                       pr.ti_begstep, pr.hsml0, pr.active, pr.des_ngb, pr.max_dev, pr.min_gas_hsml, pr.box,
                       pr.periodic, pr.ti_current, pr.timebase, rule=pr.rule)


# ------------------------------------------------------------------------------------------------
# the inputs that send the gas targets down every branch of the rule
# ------------------------------------------------------------------------------------------------
HITER_TRIES = 20
# MaxNumNgbDeviation of the case `tight`.  A target that the Newton step brings inside the window is accepted
# there (about one in fifty does, whatever the width), and it can be MARGIN * DesNumNgb = 3.3e-9 away from both
# edges only in a window wider than 6.6e-9: at 1e-9 no seed can satisfy the margin.  1e-4 is a thousand times
# finer than what the exit (Right - Left) < 1e-3 Left resolves in numngb (about 0.1), so every target that
# bisects still ends by that exit, and a seed has one chance in fifty of an accepted target near an edge.
TIGHT_DEV = 1e-4
NG = 8                      # Problem(ng=8, gas=True): 512 gas + 512 others
_CACHE = {}


def _nearest_gas(pr, i):
    d = pr.ic["pos"][i][None, :] - pr.ic["pos"][:pr.ngas]
    if pr.periodic:
        d -= pr.box * np.round(d / pr.box)
    r = np.sqrt((d * d).sum(axis=1))
    r[i] = np.inf
    return float(r.min())


def _build(name, periodic, seed):
    from common import Problem
    pr = Problem(ng=NG, gas=True, periodic=periodic, seed=seed)
    pr.case, pr.seed, pr.rule, pr.active, pr.full = name, seed, 0, None, None
    ng = pr.ngas
    rng = np.random.default_rng(7000 + seed)
    if name == "base":
        pass
    elif name == "tight":
        pr.max_dev = TIGHT_DEV
    elif name in ("minh", "clamp"):
        conv = hiter_case("base", periodic)
        assert conv.seed == seed, "the converged h of the base case belong to another particle set"
        # 0.995, not 1: in the periodic box every first step is h0 / 1.26, so many targets are accepted at
        # that very number and the median IS it -- an exact tie of the new h with MinGasHsml
        pr.min_gas_hsml = (0.995 if name == "minh" else 1.05) * float(np.median(conv.ref["hsml"][:ng]))
    elif name == "small":
        pr.hsml0[:ng] *= 0.2
    elif name == "large":
        pr.hsml0[:ng] *= 3.0
    elif name == "mixed":
        pr.hsml0[:ng] *= 10.0 ** rng.uniform(-1.0, 0.6, ng)
    elif name == "massless":
        # 8 gas particles of mass 0, each with a first h of 0.8 of the distance to its nearest neighbour: under
        # rule 0 it is its own one neighbour there (numngb = NORM_COEFF KERNEL_COEFF_1 = 10.67, rho = 0, the raw
        # dhf sum 0), and it stays a neighbour of the others.  10 more are 1000 times heavier than the rest: at
        # its own place (u = 0) such a particle supplies nearly all of its rho and of its dh sum, so that
        # dhf * h / (3 rho) comes close to -1 and passes -0.9: the guard, in the pass that is accepted, so that
        # DhsmlDensityFactor = 1 is what comes out.  (`small` and `mixed` reach the guard too, with a first h that
        # holds the target alone, but only in passes that go on: there it shapes the Newton step.)
        pick = rng.choice(ng, 18, replace=False)
        mass = pr.ic["mass"].copy()
        mass[pick[:8]] = 0.0
        mass[pick[8:]] *= 1000.0
        pr.ic["mass"] = mass
        for i in pick[:8]:
            pr.hsml0[i] = 0.8 * _nearest_gas(pr, i)
        pr.massless, pr.heavy = np.sort(pick[:8]), np.sort(pick[8:])
    elif name == "subset":
        # sub-step: the state after a full pass of the base case, then 150 active targets with perturbed
        # predicted velocities and first guesses spread over 10^U(-1, 0.6) of their converged h
        conv = hiter_case("base", periodic)
        assert conv.seed == seed
        pr.full = {k: conv.ref[k].copy() for k in FIELDS}
        pr.hsml0 = conv.ref["hsml"].copy()
        pr.active = np.sort(rng.choice(ng, 150, replace=False)).astype(np.int32)
        pr.velpred = pr.velpred + 0.02 * rng.standard_normal(pr.velpred.shape)
        pr.hsml0[pr.active] *= 10.0 ** rng.uniform(-1.0, 0.6, len(pr.active))
    else:
        raise ValueError(name)
    pr.ref = reference(pr)
    return pr


def hiter_case(name, periodic, seed0=12345):
    """The input `name` (CASES) at Problem(ng=8, gas=True, periodic=periodic) from the first of the seeds seed0,
    seed0 + 1, ... whose reference converges and keeps every comparison of every target at least MARGIN away
    from its threshold; fails loudly after HITER_TRIES seeds.  minh, clamp and subset start from the base case's
    converged h and take its seed.  The Problem carries case, seed, rule (the massless-gas rule), active (None:
    all gas), full (subset: the seven fields before the sub-step) and ref, the reference's result.  Shared: no
    caller changes it."""
    key = (name, int(periodic))
    if key not in _CACHE:
        if name in ("minh", "clamp", "subset"):
            seed0 = hiter_case("base", periodic).seed
        for seed in range(seed0, seed0 + HITER_TRIES):
            pr = _build(name, int(periodic), seed)
            tg = np.arange(pr.ngas) if pr.active is None else pr.active
            if pr.ref["iterations"] >= 0 and pr.ref["margin"][tg].min() >= MARGIN:
                _CACHE[key] = pr
                break
            assert name not in ("minh", "clamp", "subset"), \
                "%s: a comparison within %g of its threshold at the base case's seed" % (name, MARGIN)
        else:
            raise AssertionError("hiter_case(%r): %d seeds from %d on all fail to converge or have a comparison "
                                 "within %g of its threshold" % (name, HITER_TRIES, seed0, MARGIN))
    return _CACHE[key]


def carriers(refs):
    """label -> the number of targets that carry it, summed over the references `refs`"""
    count = dict.fromkeys(LABELS, 0)
    for r in refs:
        for br in r["branches"]:
            for b in br:
                count[b] += 1
    return count
