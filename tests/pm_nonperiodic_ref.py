"""numpy restatement of the non-periodic particle-mesh code for mesh 0 (pm_nonperiodic.c, GRIDBOOST 2, no
PLACEHIGHRESREGION / SCALARFIELD / ENLARGEREGION) and of the tail of long_range_force (longrange.c:117-138):
pm_init_regionsize (:91-212), pm_setup_nonperiodic_kernel (:371-438, 500-558), pmforce_nonperiodic(0)
(:576-1175) and pmpotential_nonperiodic(0) (:1354-1750).  FFTs are np.fft.rfftn / irfftn; irfftn divides by
GRID^3 where FFTW does not, so the inverse is multiplied by GRID^3 to keep the reference's prefactors.

Cells of the force mesh that the reference leaves unwritten (outside 2 <= x, y, z < GRID/2 - 2, :1005-1008) are
zero here.  No particle of the allowed region reads them.
"""
import math

import numpy as np

ASMTH = 1.25   # allvars.h:122
RCUT = 4.5     # allvars.h:128

try:
    from scipy.special import erf as _erf
except ImportError:   # (libm's erf one value at a time)
    _erf = np.vectorize(math.erf, otypes=[np.float64])


def region_from_extremes(xmin, xmax, pmgrid):
    """pm_init_regionsize :121-159 from the extremes of :98-119, operation for operation in double"""
    GRID = 2 * int(pmgrid)
    xmin = [float(v) for v in xmin]
    xmax = [float(v) for v in xmax]
    tms = xmax[0] - xmin[0]                                   # :123-125
    tms = max(tms, xmax[1] - xmin[1])
    tms = max(tms, xmax[2] - xmin[2])
    Xmintot, Xmaxtot = [0.0] * 3, [0.0] * 3
    for i in range(3):                                        # :131-135
        Xmintot[i] = (xmin[i] + xmax[i]) / 2 - tms / 2
        Xmaxtot[i] = Xmintot[i] + tms
    meshinner = tms
    tms *= 2.001 * GRID / float(GRID - 2 - 8)                 # :144
    Corner, Upper = [0.0] * 3, [0.0] * 3
    for i in range(3):                                        # :152-153
        Corner[i] = Xmintot[i] - 2.0005 * tms / GRID
        Upper[i] = Corner[i] + (GRID // 2 - 1) * (tms / GRID)
    Asmth = ASMTH * tms / GRID                                # :158-159
    Rcut = RCUT * Asmth
    return dict(pmgrid=int(pmgrid), Xmintot=np.array(Xmintot), Xmaxtot=np.array(Xmaxtot), meshinner=meshinner,
                TotalMeshSize=tms, Corner=np.array(Corner), UpperCorner=np.array(Upper), Asmth=Asmth, Rcut=Rcut)


def region(pos, pmgrid):
    """pm_init_regionsize (:91-212) for the particles pos [n, 3]"""
    pos = np.asarray(pos, np.float64)
    return region_from_extremes(pos.min(axis=0), pos.max(axis=0), pmgrid)


def range_slack(reg):
    """The rounding of :133-134 can leave a bound 1 ulp inside the particle that defines the extent, which the
    reference then refuses for good (endrun(68687)).  The library's range check allows 4 eps max(|Xmintot|,
    |Xmaxtot|) per axis, twice the bound of the three roundings; this is that rule, not the reference's."""
    return 4 * np.finfo(np.float64).eps * np.maximum(np.abs(reg["Xmintot"]), np.abs(reg["Xmaxtot"]))


def in_region(pos, reg, slack=True):
    """the range check of :614-647: True where a particle lies inside [Xmintot, Xmaxtot] (slack: widened by
    range_slack, as the library checks; False: the reference's own comparison)"""
    pos = np.asarray(pos, np.float64)
    tol = range_slack(reg) if slack else 0.0
    return np.all((pos >= reg["Xmintot"] - tol) & (pos <= reg["Xmaxtot"] + tol), axis=1)


_KERNELS = {}


def kernel_table(pmgrid):
    """fft_of_kernel[0] (:396-434, 500-558) in the layout of rfftn: [GRID][GRID][GRID/2 + 1].  Depends on
    PMGRID only: ASMTH / GRID is in mesh units."""
    pmgrid = int(pmgrid)
    if pmgrid in _KERNELS:
        return _KERNELS[pmgrid]
    GRID = 2 * pmgrid
    c = np.arange(GRID, dtype=np.float64) / GRID              # :400-409
    c = np.where(c >= 0.5, c - 1.0, c)
    xx, yy, zz = np.meshgrid(c, c, c, indexing="ij")
    r = np.sqrt(xx * xx + yy * yy + zz * zz)
    u = 0.5 * r / (ASMTH / GRID)                              # :413
    fac = _erf(u)                                             # :415, 1 - erfc(u)
    with np.errstate(divide="ignore", invalid="ignore"):
        kern = -fac / r
    kern[0, 0, 0] = -1 / (math.sqrt(math.pi) * (ASMTH / GRID))   # :420-421
    fk = np.fft.rfftn(kern)
    k = np.arange(GRID, dtype=np.float64)                     # :504-515
    k = np.where(k > GRID // 2, k - GRID, k)
    kz = np.arange(GRID // 2 + 1, dtype=np.float64)

    def sinc(kk):
        f = np.ones_like(kk)
        nz = kk != 0
        a = (math.pi * kk[nz]) / GRID
        f[nz] = np.sin(a) / a
        return f
    fx, fy, fz = sinc(k)[:, None, None], sinc(k)[None, :, None], sinc(kz)[None, None, :]
    ff = 1 / (fx * fy * fz)                                   # :537-538 (k = 0: all three are 1, ff = 1)
    ff = ff * ff * ff * ff
    fk = fk * ff
    _KERNELS[pmgrid] = fk
    return fk


def _cic(pos, reg):
    """slab indices and offsets of :766-772"""
    GRID = 2 * reg["pmgrid"]
    to_slab_fac = GRID / reg["TotalMeshSize"]                 # :609
    p = to_slab_fac * (np.asarray(pos, np.float64) - reg["Corner"])
    s = p.astype(np.int64)
    return s, p - s


def cells(pos, reg):
    """the eight mesh cells of each particle [n, 8, 3] (:672-690)"""
    s, _ = _cic(pos, reg)
    off = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)])
    return s[:, None, :] + off[None, :, :]


def deposit(pos, mass, reg):
    """the density mesh [GRID]^3 (:757-790), zero outside the lower octant"""
    GRID = 2 * reg["pmgrid"]
    s, d = _cic(pos, reg)
    mass = np.asarray(mass, np.float64)
    rho = np.zeros((GRID, GRID, GRID))
    for xx in (0, 1):
        for yy in (0, 1):
            for zz in (0, 1):
                w = (mass * (d[:, 0] if xx else 1.0 - d[:, 0]) * (d[:, 1] if yy else 1.0 - d[:, 1]) *
                     (d[:, 2] if zz else 1.0 - d[:, 2]))
                np.add.at(rho, (s[:, 0] + xx, s[:, 1] + yy, s[:, 2] + zz), w)
    return rho


def potential_mesh(rho, pmgrid):
    """:856-895: forward transform, product with the table, unnormalised inverse transform"""
    GRID = 2 * int(pmgrid)
    return np.fft.irfftn(np.fft.rfftn(rho) * kernel_table(pmgrid), s=(GRID, GRID, GRID), axes=(0, 1, 2)) * float(GRID) ** 3


def _readout(mesh, pos, reg):
    """CIC read-out in the corner order of :1143-1151 / :1722-1730"""
    s, d = _cic(pos, reg)
    out = np.zeros(len(s))
    for xx in (0, 1):
        for yy in (0, 1):
            for zz in (0, 1):
                out = out + (mesh[s[:, 0] + xx, s[:, 1] + yy, s[:, 2] + zz] * (d[:, 0] if xx else 1.0 - d[:, 0]) *
                             (d[:, 1] if yy else 1.0 - d[:, 1]) * (d[:, 2] if zz else 1.0 - d[:, 2]))
    return out


def force_mesh(phi, reg, G):
    """:1000-1051: the three components [3][GRID/2]^3 of the lower octant, zero where the reference does not write"""
    pm = reg["pmgrid"]
    GRID = 2 * pm
    tms = reg["TotalMeshSize"]
    fac = G / tms ** 4 * (tms / GRID) ** 3                    # :606
    fac *= 1 / (2 * tms / GRID)                               # :607
    lo, hi = 2, GRID // 2 - 2
    out = np.zeros((3, pm, pm, pm))
    c = np.arange(lo, hi)
    for dim in range(3):
        def sh(o):
            idx = [c[:, None, None], c[None, :, None], c[None, None, :]]
            idx[dim] = idx[dim] + o
            return phi[idx[0], idx[1], idx[2]]
        out[dim, lo:hi, lo:hi, lo:hi] = fac * ((4.0 / 3) * (sh(-1) - sh(+1)) - (1.0 / 6) * (sh(-2) - sh(+2)))
    return out


def tail(gravpm, pos, comoving=0, Omega0=0.0, OmegaLambda=0.0, Hubble=0.0):
    """longrange.c:117-138"""
    fac = 0.5 * Hubble * Hubble * Omega0 if comoving else OmegaLambda * Hubble * Hubble
    return gravpm + fac * np.asarray(pos, np.float64)


def pm_force(pos, mass, reg, G, comoving=0, Omega0=0.0, OmegaLambda=0.0, Hubble=0.0):
    """GravPM [n, 3] of long_range_force for the non-periodic mesh 0; raises if a particle is out of range
    (the reference returns 1 there, :646)"""
    if not np.all(in_region(pos, reg)):
        raise ValueError("a particle lies outside the allowed region")
    phi = potential_mesh(deposit(pos, mass, reg), reg["pmgrid"])
    fm = force_mesh(phi, reg, G)
    acc = np.stack([_readout(fm[dim], pos, reg) for dim in range(3)], axis=1)
    return tail(acc, pos, comoving, Omega0, OmegaLambda, Hubble)


def pm_potential(pos, mass, reg, G):
    """the mesh potential of pmpotential_nonperiodic(0) at the particles, times the fac of :1378 that the
    fork computes and never applies (without it the mesh part is not in the units of the tree part)"""
    if not np.all(in_region(pos, reg)):
        raise ValueError("a particle lies outside the allowed region")
    GRID = 2 * reg["pmgrid"]
    tms = reg["TotalMeshSize"]
    fac = G / tms ** 4 * (tms / GRID) ** 3                    # :1378
    phi = potential_mesh(deposit(pos, mass, reg), reg["pmgrid"])
    return fac * _readout(phi, pos, reg)


# ---------------------------------------------------------------------------------------------
# what the mesh approximates: the exact long-range parts of the force split
# ---------------------------------------------------------------------------------------------
def exact_longrange(pos, mass, asmth, G):
    """G sum m d (erf(r/2a) - r/(a sqrt(pi)) exp(-r^2/4a^2)) / r^3 over all other particles, and the Newtonian
    force, both [n, 3]"""
    pos = np.asarray(pos, np.float64)
    d = pos[None, :, :] - pos[:, None, :]
    r = np.sqrt((d * d).sum(axis=2))
    np.fill_diagonal(r, 1.0)
    u = r / (2 * asmth)
    f = _erf(u) - r / (asmth * math.sqrt(math.pi)) * np.exp(-u * u)
    np.fill_diagonal(f, 0.0)
    w = mass[None, :] / r ** 3
    np.fill_diagonal(w, 0.0)
    return G * ((w * f)[:, :, None] * d).sum(axis=1), G * (w[:, :, None] * d).sum(axis=1)


def exact_longrange_potential(pos, mass, asmth, G):
    """-G sum m erf(r/2a) / r over all other particles plus the self term -G m / (sqrt(pi) a)"""
    pos = np.asarray(pos, np.float64)
    d = pos[None, :, :] - pos[:, None, :]
    r = np.sqrt((d * d).sum(axis=2))
    np.fill_diagonal(r, 1.0)
    t = _erf(r / (2 * asmth)) / r
    np.fill_diagonal(t, 0.0)
    return -G * (t * mass[None, :]).sum(axis=1) - G * mass / (math.sqrt(math.pi) * asmth)
