"""numpy restatement of compute_potential() (potential.c:22-325) and its parts -- the potential walk
force_treeevaluate_potential / _shortrange (forcetree.c:3217-3530, 3752-4115) over a tree in the
reference's layout (nextnode / sibling / flags), ewald_psi and ewald_pot_corr (forcetree.c:4633-4720),
the finish and pmpotential_periodic (pm_periodic.c:808-1195) -- and of the particle loop of
compute_global_quantities_of_system() (global.c:18-238).  Operations are written in the reference's
order, so that the device kernels (built without floating-point contraction) can be compared with
them to rounding.
"""
import math

import numpy as np

EN = 64
NTAB = 1000
POT_ORIGIN = 2.8372975
GAMMA = 7.0 / 5.0
DRIFT_TABLE_LENGTH = 1000

try:
    from scipy.special import erfc as _erfc
except ImportError:   # (libm's erfc one value at a time)
    _erfc = np.vectorize(math.erfc, otypes=[np.float64])


# ---------------------------------------------------------------------------------------------
# Ewald potential correction
# ---------------------------------------------------------------------------------------------
def ewald_psi(x):
    """ewald_psi (forcetree.c:4686-4720) at the rows of x [m, 3] (box 1), terms in the reference's order"""
    x = np.atleast_2d(np.asarray(x, np.float64))
    x0, x1, x2 = x[:, 0], x[:, 1], x[:, 2]
    alpha = 2.0
    sum1 = np.zeros(len(x))
    for n0 in range(-4, 5):
        for n1 in range(-4, 5):
            for n2 in range(-4, 5):
                d0, d1, d2 = x0 - n0, x1 - n1, x2 - n2
                r = np.sqrt(d0 * d0 + d1 * d1 + d2 * d2)
                sum1 += _erfc(alpha * r) / r
    sum2 = np.zeros(len(x))
    for h0 in range(-4, 5):
        for h1 in range(-4, 5):
            for h2i in range(-4, 5):
                h2 = h0 * h0 + h1 * h1 + h2i * h2i
                if h2 > 0:
                    hdotx = x0 * h0 + x1 * h1 + x2 * h2i
                    sum2 += (1 / (math.pi * h2) * math.exp(-math.pi * math.pi * h2 / (alpha * alpha)) *
                             np.cos(2 * math.pi * hdotx))
    r = np.sqrt(x0 * x0 + x1 * x1 + x2 * x2)
    return math.pi / (alpha * alpha) - sum1 - sum2 + 1 / r


def pot_table(boxsize, idx=None):
    """potcorr of ewald_init divided by BoxSize (forcetree.c:4466-4525): [EN+1]^3, or the entries at the
    index rows idx [m, 3] only"""
    full = idx is None
    if full:
        g = np.arange(EN + 1)
        idx = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    idx = np.asarray(idx, np.int64)
    out = np.empty(len(idx))
    origin = idx.sum(axis=1) == 0
    x = 0.5 * idx[~origin].astype(np.float64) / EN
    out[~origin] = ewald_psi(x)
    out[origin] = POT_ORIGIN
    out = out / boxsize
    return out.reshape(EN + 1, EN + 1, EN + 1) if full else out


def ewald_pot_corr(tab, boxsize, dx, dy, dz):
    """ewald_pot_corr (forcetree.c:4633-4684), vectorised"""
    fac_intp = 2 * EN / boxsize
    ii, ww = [], []
    for a in (dx, dy, dz):
        u = np.abs(np.asarray(a, np.float64)) * fac_intp
        i = np.minimum(u.astype(np.int64), EN - 1)
        ii.append(i)
        ww.append(u - i)
    i, j, k = ii
    u, v, w = ww
    f1 = (1 - u) * (1 - v) * (1 - w)
    f2 = (1 - u) * (1 - v) * (w)
    f3 = (1 - u) * (v) * (1 - w)
    f4 = (1 - u) * (v) * (w)
    f5 = (u) * (1 - v) * (1 - w)
    f6 = (u) * (1 - v) * (w)
    f7 = (u) * (v) * (1 - w)
    f8 = (u) * (v) * (w)
    return (tab[i, j, k] * f1 + tab[i, j, k + 1] * f2 + tab[i, j + 1, k] * f3 + tab[i, j + 1, k + 1] * f4 +
            tab[i + 1, j, k] * f5 + tab[i + 1, j, k + 1] * f6 + tab[i + 1, j + 1, k] * f7 +
            tab[i + 1, j + 1, k + 1] * f8)


def shortrange_table_potential():
    """forcetree.c:4195-4202: erfc(u) at u = 3/NTAB (i + 1/2), a float table"""
    u = 3.0 / NTAB * (np.arange(NTAB) + 0.5)
    return np.array([math.erfc(x) for x in u], np.float32)


# ---------------------------------------------------------------------------------------------
# trees in the reference's layout
# ---------------------------------------------------------------------------------------------
class RefTree:
    """Elements [0, maxpart) are particles (next = Nextnode[]), [maxpart, maxpart + nnodes) nodes
    (open: nextnode, accept: sibling); -1 ends the walk.  soft: a particle's softening, a node's
    largest softening (maxsoft); mixed: the node opens for a target inside that softening."""

    def __init__(self, maxpart, pos, mass, psoft, p_next, nodes):
        n = len(pos)
        nn = len(nodes["len"])
        tot = maxpart + nn
        self.root = maxpart
        self.x = np.zeros((tot, 3))
        self.x[:n] = pos
        self.x[maxpart:] = nodes["s"]
        self.m = np.zeros(tot)
        self.m[:n] = mass
        self.m[maxpart:] = nodes["mass"]
        self.isnode = np.zeros(tot, bool)
        self.isnode[maxpart:] = True
        self.len = np.zeros(tot)
        self.len[maxpart:] = nodes["len"]
        self.cen = np.zeros((tot, 3))
        self.cen[maxpart:] = nodes["center"]
        self.nopen = np.full(tot, -1, np.int64)
        self.nacc = np.full(tot, -1, np.int64)
        self.nopen[:n] = p_next
        self.nacc[:n] = p_next
        self.nopen[maxpart:] = nodes["nextnode"]
        self.nacc[maxpart:] = nodes["sibling"]
        self.soft = np.zeros(tot)
        self.soft[:n] = psoft
        self.soft[maxpart:] = nodes["maxsoft"]
        self.mixed = np.zeros(tot, bool)
        self.mixed[maxpart:] = np.asarray(nodes["mixed"], bool)
        self.multi = np.ones(tot, bool)
        self.multi[maxpart:] = np.asarray(nodes["multi"], bool)

    @classmethod
    def from_oracle(cls, dump, pos, mass, psoft, adaptive=False):
        """O.Tree(...).dump() (MaxPart = N); adaptive: the dump of a tree after .adaptive_gravsoft()"""
        nodes = dict(len=dump["len"], center=dump["center"], s=dump["s"], mass=dump["mass"],
                     nextnode=dump["nextnode"], sibling=dump["sibling"], multi=dump["multi"],
                     maxsoft=dump["maxsoft"],
                     mixed=(np.ones(len(dump["len"]), bool) if adaptive else dump["mixedsoft"] != 0))
        return cls(len(pos), pos, mass, psoft, dump["p_nextnode"], nodes)

    @classmethod
    def from_export(cls, exported, maxpart, pos, mass, psoft, force_soft, unequal=False,
                    adaptive=False):
        """ForcePath.tree_export(...) = (Nodes, Extnodes, Nextnode, Father): bitflags bit 7 multiple
        particles, bits 2-4 the max-softening type, bit 5 mixed softenings; adaptive: NODE.maxsoft"""
        nd, _, nxt, _ = exported
        bf = nd["bitflags"].astype(np.int64)
        if adaptive:
            maxsoft = nd["maxsoft"]
            mixed = np.ones(len(nd), bool)
        elif unequal:
            maxsoft = np.asarray(force_soft)[(bf >> 2) & 7]
            mixed = ((bf >> 5) & 1) != 0
        else:
            maxsoft = np.zeros(len(nd))
            mixed = np.zeros(len(nd), bool)
        nodes = dict(len=nd["len"], center=nd["center"], s=nd["s"], mass=nd["mass"],
                     nextnode=nd["nextnode"], sibling=nd["sibling"], multi=((bf >> 7) & 1) != 0,
                     maxsoft=maxsoft, mixed=mixed)
        return cls(maxpart, pos, mass, psoft, nxt[:len(pos)], nodes)

    @classmethod
    def from_elements(cls, xm, cl, lk, aux=None):
        """a pre-order element list (ghip_tree_dump / ghip_tree_dump_dynamic): xm = (x, y, z, mass),
        cl = (centre, len), lk = (skip, particle index or -(level+1), ...); open = e + 1, accept = skip"""
        ne = len(xm)
        isn = lk[:, 1] < 0
        t = cls.__new__(cls)
        t.root = 0
        t.x = np.ascontiguousarray(xm[:, :3])
        t.m = np.ascontiguousarray(xm[:, 3])
        t.isnode = isn
        t.len = np.where(isn, cl[:, 3], 0.0)
        t.cen = np.ascontiguousarray(cl[:, :3])
        e1 = np.arange(1, ne + 1)
        t.nopen = np.where(e1 >= ne, -1, e1)
        nacc = np.where(isn, lk[:, 0], e1)
        t.nacc = np.where(nacc >= ne, -1, nacc)
        a = np.zeros(ne) if aux is None else np.asarray(aux, np.float64)
        t.soft = np.abs(a)
        t.mixed = isn & (a < 0)
        t.multi = np.ones(ne, bool)
        return t


def _nearest(x, box):
    half = 0.5 * box
    return np.where(x > half, x - box, np.where(x < -half, x + box, x))


def pot_term(mass, r, h):
    """forcetree.c:3492-3511: -m / r outside h, the spline potential m / h wp(r / h) inside"""
    mass = np.broadcast_to(np.asarray(mass, np.float64), r.shape)
    h = np.broadcast_to(np.asarray(h, np.float64), r.shape)
    out = np.empty_like(r)
    far = r >= h
    out[far] = -mass[far] / r[far]
    nf = ~far
    if nf.any():
        h_inv = 1.0 / h[nf]
        u = r[nf] * h_inv
        with np.errstate(divide="ignore", invalid="ignore"):
            wp = np.where(u < 0.5, -2.8 + u * u * (5.333333333333 + u * u * (6.4 * u - 9.6)),
                          -3.2 + 0.066666666667 / u +
                          u * u * (10.666666666667 + u * (-16.0 + u * (9.6 - 2.133333333333 * u))))
        out[nf] = mass[nf] * h_inv * wp
    return out


def walk_potential(T, tpos, tsoft, toldacc, theta, errtol=0.005, periodic=False, box=1.0,
                   unequal=False, potcorr=None, rcut=None, asmth=None):
    """The potential of the targets (positions tpos, softening tsoft -- Hsml for gas with adaptive
    softening --, OldAcc toldacc), each walk in the reference's order.  Returns (pot, interactions)."""
    tpos = np.asarray(tpos, np.float64)
    m = len(tpos)
    no = np.full(m, T.root, np.int64)
    pot = np.zeros(m)
    nint = np.zeros(m, np.int64)
    aold_all = errtol * np.asarray(toldacc, np.float64)
    th_all = np.asarray(tsoft, np.float64)
    short = rcut is not None
    if short:
        asmthfac = 0.5 / asmth * (NTAB / 3.0)
        srpot = shortrange_table_potential()
    while True:
        act = np.nonzero(no >= 0)[0]
        if len(act) == 0:
            break
        e = no[act]
        px, py, pz = tpos[act, 0], tpos[act, 1], tpos[act, 2]
        isn = T.isnode[e]
        nomulti = isn & ~T.multi[e]
        dx, dy, dz = T.x[e, 0] - px, T.x[e, 1] - py, T.x[e, 2] - pz
        if periodic:
            dx, dy, dz = _nearest(dx, box), _nearest(dy, box), _nearest(dz, box)
        r2 = dx * dx + dy * dy + dz * dz
        h = th_all[act].copy()
        if unequal:
            h = np.where(~isn & (h < T.soft[e]), T.soft[e], h)
        L = T.len[e]
        cx, cy, cz = T.cen[e, 0] - px, T.cen[e, 1] - py, T.cen[e, 2] - pz
        drop = np.zeros(len(act), bool)
        if short:
            eff = rcut + 0.5 * L
            if periodic:
                ux, uy, uz = _nearest(cx, box), _nearest(cy, box), _nearest(cz, box)
            else:
                ux, uy, uz = cx, cy, cz
            drop = isn & ~nomulti & ((ux < -eff) | (ux > eff) | (uy < -eff) | (uy > eff) |
                                     (uz < -eff) | (uz > eff))
        if theta:
            crit = L * L > r2 * theta * theta
        else:
            crit = T.m[e] * L * L > r2 * r2 * aold_all[act]
            crit |= (np.abs(cx) < 0.60 * L) & (np.abs(cy) < 0.60 * L) & (np.abs(cz) < 0.60 * L)
        opn = isn & ~drop & (nomulti | crit)
        if unequal:
            ms = T.soft[e]
            up = isn & ~drop & ~opn & (h < ms)
            h = np.where(up, ms, h)
            opn |= up & T.mixed[e] & (r2 < h * h)
        inter = ~opn & ~drop
        nxt = np.where(opn, T.nopen[e], T.nacc[e])
        ii = np.nonzero(inter)[0]
        if len(ii):
            r = np.sqrt(r2[ii])
            mm = T.m[e[ii]]
            tgt = act[ii]
            if short:
                ti = (r * asmthfac).astype(np.int64)
                ok = ti < NTAB
                fac = srpot[np.minimum(ti, NTAB - 1)].astype(np.float64)
                term = pot_term(fac * mm, r, h[ii])
                pot[tgt[ok]] += term[ok]
                nint[tgt[ok]] += 1
            else:
                pot[tgt] += pot_term(mm, r, h[ii])
                if periodic:
                    pot[tgt] += mm * ewald_pot_corr(potcorr, box, dx[ii], dy[ii], dz[ii])
                nint[tgt] += 1
        no[act] = nxt
    return pot, nint


def direct_potential(pos, mass, tsoft, ssoft, targets, unequal=False):
    """O(N^2) sum of the same pair potential over all particles (the r = 0 term included), index order"""
    pos = np.asarray(pos, np.float64)
    mass = np.asarray(mass, np.float64)
    out = np.zeros(len(targets))
    for a, i in enumerate(targets):
        d = pos - pos[i]
        r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        h = np.full(len(pos), tsoft[i])
        if unequal:
            h = np.maximum(h, ssoft)
        out[a] = pot_term(mass, r, h).sum()
    return out


# ---------------------------------------------------------------------------------------------
# finish and mesh part (potential.c:235-325, pm_periodic.c:808-1195)
# ---------------------------------------------------------------------------------------------
def pm_potential(pos, mass, box, G, N, asmth):
    """pmpotential_periodic: CIC deposit, Green's function -exp(-k^2 asmth^2)/k^2 with the CIC
    deconvolution to the fourth power, CIC read-out, times fac = G / (pi BoxSize)"""
    pos = np.asarray(pos, np.float64)
    mass = np.asarray(mass, np.float64)
    to_slab = N / box
    p = to_slab * pos
    s = p.astype(np.int64)
    d = p - s
    s = np.minimum(s, N - 1)
    corners = [(xx, yy, zz) for xx in (0, 1) for yy in (0, 1) for zz in (0, 1)]

    def weight(c):
        return ((d[:, 0] if c[0] else 1.0 - d[:, 0]) * (d[:, 1] if c[1] else 1.0 - d[:, 1]) *
                (d[:, 2] if c[2] else 1.0 - d[:, 2]))
    rho = np.zeros((N, N, N))
    for c in corners:
        g = (s + np.array(c)) % N
        np.add.at(rho, (g[:, 0], g[:, 1], g[:, 2]), mass * weight(c))
    fk = np.fft.rfftn(rho)
    kx = np.arange(N)
    kx = np.where(kx > N // 2, kx - N, kx).astype(np.float64)
    kz = np.arange(N // 2 + 1).astype(np.float64)
    KX, KY, KZ = np.meshgrid(kx, kx, kz, indexing="ij")
    k2 = KX * KX + KY * KY + KZ * KZ
    asmth2 = (2 * math.pi) * asmth / box
    asmth2 *= asmth2

    def sinc(k):
        f = (math.pi * k) / N
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(k != 0, np.sin(f) / f, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        smth = -np.exp(-k2 * asmth2) / k2
    ff = 1 / (sinc(KX) * sinc(KY) * sinc(KZ))
    smth = smth * (ff * ff * ff * ff)
    smth[k2 == 0] = 0.0
    phi = np.fft.irfftn(fk * smth, s=(N, N, N), axes=(0, 1, 2)) * float(N) ** 3   # (unnormalised, as FFTW / hipFFT)
    v = np.zeros(len(pos))
    for c in corners:
        g = (s + np.array(c)) % N
        v += phi[g[:, 0], g[:, 1], g[:, 2]] * weight(c)
    return G / (math.pi * box) * v


def finish(walk, pos, mass, ptype, soft_table, G, comoving=0, periodic=0, Omega0=0.0,
           OmegaLambda=0.0, Hubble=0.0, pm=None):
    """potential.c:235-325 in order: + m / SofteningTable[type], the comoving periodic background,
    * G, + the PM potential, the r^2 term.  pm: dict(pmgrid, box, asmth) or None."""
    pos = np.asarray(pos, np.float64)
    mass = np.asarray(mass, np.float64)
    p = walk + mass / np.asarray(soft_table, np.float64)[ptype]
    if comoving and periodic:
        bg = (Omega0 * 3 * Hubble * Hubble / (8 * math.pi * G)) ** (1.0 / 3)
        p = p - POT_ORIGIN * mass ** (2.0 / 3) * bg
    p = p * G
    if pm is not None:
        p = p + pm_potential(pos, mass, pm["box"], G, pm["pmgrid"], pm["asmth"])
    fac = 0.0
    if comoving:
        if not periodic:
            fac = -0.5 * Omega0 * Hubble * Hubble
    else:
        fac = -0.5 * OmegaLambda * Hubble * Hubble
    if fac != 0:
        r2 = pos[:, 0] * pos[:, 0] + pos[:, 1] * pos[:, 1] + pos[:, 2] * pos[:, 2]
        p = p + fac * r2
    return p


# ---------------------------------------------------------------------------------------------
# compute_global_quantities_of_system (global.c:18-238)
# ---------------------------------------------------------------------------------------------
def table_factor(tab, t0, t1, logTimeBegin, logTimeMax, timebase):
    """get_gravkick_factor / get_hydrokick_factor (driftfac.c:166-247), vectorised over t0, t1"""
    tab = np.asarray(tab, np.float64)

    def one(t):
        a = logTimeBegin + np.asarray(t, np.float64) * timebase
        u = (a - logTimeBegin) / (logTimeMax - logTimeBegin) * DRIFT_TABLE_LENGTH
        i = np.minimum(u.astype(np.int64), DRIFT_TABLE_LENGTH - 1)
        lo = np.maximum(i - 1, 0)
        return np.where(i <= 1, u * tab[0], tab[lo] + (tab[i] - tab[lo]) * (u - i))
    return one(t1) - one(t0)


def global_quantities(pos, vel, mass, ptype, timebin, ti_begstep, gravaccel, Ti_Current, timebase,
                      pot=None, ngas=0, hydroaccel=None, entropy=None, dtentropy=None, density=None,
                      comoving=0, time=1.0, tables=None, gravpm=None, dt_gravkick_pm=0.0,
                      photon=None, rad_fac=1.0):
    """the per-type sums of state_of_system and, per sum, the sum of the magnitudes of its terms
    (the scale a comparison is relative to); tables = (logTimeBegin, logTimeMax, grav, hydro)"""
    pos, vel, mass, gravaccel = (np.asarray(a, np.float64) for a in (pos, vel, mass, gravaccel))
    ptype = np.asarray(ptype)
    n = len(pos)
    a1, a2, a3 = (time, time * time, time * time * time) if comoving else (1.0, 1.0, 1.0)
    tb = np.asarray(timebin, np.int64)
    tbeg = np.asarray(ti_begstep, np.int64)
    dt_step = np.where(tb > 0, np.left_shift(1, tb), 0)
    mid = tbeg + dt_step // 2
    if comoving:
        lb, lm, gk, hk = tables
        dt_entr = (Ti_Current - mid) * timebase
        dt_g = table_factor(gk, tbeg, Ti_Current, lb, lm, timebase) - \
            table_factor(gk, tbeg, mid, lb, lm, timebase)
        dt_h = table_factor(hk, tbeg, Ti_Current, lb, lm, timebase) - \
            table_factor(hk, tbeg, mid, lb, lm, timebase)
    else:
        dt_entr = dt_g = dt_h = (Ti_Current - mid) * timebase
    gas = (ptype == 0) & (np.arange(n) < ngas)
    v = vel + gravaccel * dt_g[:, None]
    if ngas:
        v[:ngas] += np.where(gas[:ngas, None], np.asarray(hydroaccel) * dt_h[:ngas, None], 0.0)
    if gravpm is not None:
        v = v + gravpm * dt_gravkick_pm
    q = {"MassComp": mass,
         "EnergyPotComp": 0.5 * mass * pot / a1 if pot is not None else np.zeros(n),
         "EnergyKinComp": 0.5 * mass * (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]) / a2}
    eint = np.zeros(n)
    if ngas:
        entr = np.asarray(entropy) + np.asarray(dtentropy) * dt_entr[:ngas]
        eint[:ngas] = np.where(gas[:ngas], mass[:ngas] * (entr / (GAMMA - 1) *
                                                          (np.asarray(density) / a3) ** (GAMMA - 1)), 0.0)
    q["EnergyIntComp"] = eint
    mom = mass[:, None] * v
    com = mass[:, None] * pos
    ang = np.stack([mass * (pos[:, 1] * v[:, 2] - pos[:, 2] * v[:, 1]),
                    mass * (pos[:, 2] * v[:, 0] - pos[:, 0] * v[:, 2]),
                    mass * (pos[:, 0] * v[:, 1] - pos[:, 1] * v[:, 0])], axis=1)
    out, scale = {}, {}
    for k in ("MassComp", "EnergyPotComp", "EnergyKinComp", "EnergyIntComp"):
        out[k] = np.array([q[k][ptype == t].sum() for t in range(6)])
        scale[k] = np.array([np.abs(q[k][ptype == t]).sum() for t in range(6)])
    for k, a in (("MomentumComp", mom), ("CenterOfMassComp", com), ("AngMomentumComp", ang)):
        o = np.zeros((6, 4))
        s = np.zeros((6, 4))
        for t in range(6):
            o[t, :3] = a[ptype == t].sum(axis=0)
            s[t, :3] = np.abs(a[ptype == t]).sum(axis=0)
        out[k], scale[k] = o, s
    rad = np.zeros(n)
    if photon is not None:
        sel = (ptype == 3) & (mass != 0.)
        rad[sel] = np.asarray(photon, np.float64)[sel] * rad_fac
    out["EnergyRadComp"] = float(rad.sum())
    scale["EnergyRadComp"] = float(np.abs(rad).sum())
    return out, scale


def max_rel_diff(dev, ref, scale):
    """largest |dev - ref| over all per-type sums, relative to the magnitudes summed into each"""
    worst = 0.0
    for k, r in ref.items():
        d = np.asarray(dev[k], np.float64)
        s = np.maximum(np.asarray(scale[k], np.float64), 1e-300)
        worst = max(worst, float(np.max(np.abs(d - np.asarray(r)) / s)))
    return worst
