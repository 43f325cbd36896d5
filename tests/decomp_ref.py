"""NumPy restatement of GHIP_DD_DECOMPOSE (include/ghip.h): the extent rule of domain_findExtent
(domain.c:1972-2014), the Peano-Hilbert cell of a position, the integer weights of
domain_particle_costfactor (domain.c:378-384) and domain_findSplit_work_balanced (domain.c:1075-1113).
Uses nothing from the library; the curve is the oracle's table-driven peano_hilbert_key."""
import numpy as np

BITS = 21
TIMEBINS = 29


def histogram_level(ntot, nranks):
    """about 32 particles of the whole run per cell, level 1..7, at least nranks cells"""
    level = 1
    while level < 7 and 8 ** level * 32 < ntot:
        level += 1
    while 8 ** level < nranks:
        level += 1
    return level


def extent(pos):
    """(corner[3], center[3], len): len = 1.001 max_j(xmax_j - xmin_j), center_j = 0.5 (xmin_j + xmax_j),
    corner_j = center_j - 0.5 len, in double and in this order"""
    pos = np.asarray(pos, np.float64) + 0.0
    xmin, xmax = pos.min(axis=0), pos.max(axis=0)
    ln = 0.0
    for j in range(3):
        if xmax[j] - xmin[j] > ln:
            ln = float(xmax[j] - xmin[j])
    ln *= 1.001
    center = np.array([0.5 * (xmin[j] + xmax[j]) for j in range(3)])
    corner = np.array([0.5 * (xmin[j] + xmax[j]) - 0.5 * ln for j in range(3)])
    return corner, center, ln


def integer_coordinates(pos, corner, ln):
    """(int) ((x - corner) * DomainFac), DomainFac = 1 / len * 2^21, clamped to the cube's cells"""
    fac = 1.0 / ln * float(1 << BITS)
    c = (np.asarray(pos, np.float64) - np.asarray(corner)) * fac
    return np.clip(c, 0, (1 << BITS) - 1).astype(np.int64)


def keys_of(pos, corner, ln):
    from oracle import oracle as O
    ip = integer_coordinates(pos, corner, ln)
    return np.array([O.peano_hilbert_key(*p) for p in ip], dtype=np.uint64)


def effective_bins(timebin):
    tb = np.asarray(timebin, np.int64)
    return np.where(tb == 0, TIMEBINS, tb)


def ceil_log2(n):
    c = 0
    while (1 << c) < n:
        c += 1
    return c


def excess_shift(bmin, bmax, ntot):
    """s: (1 + GravCost) < 2^32, shifted by at most bmax - bmin, summed over at most 2^ceil(log2 N)
    particles, must stay below 2^63"""
    return max(0, (bmax - bmin) + 32 + ceil_log2(ntot) - 63)


def integer_weights(gravcost, timebin, ntot=None, bmin=None, bmax=None):
    """w = ((1 + GravCost) << (bmax - b)) >> s, at least 1, as uint64 (exact: Python integers)"""
    b = effective_bins(timebin)
    bmin = int(b.min()) if bmin is None else bmin
    bmax = int(b.max()) if bmax is None else bmax
    ntot = len(b) if ntot is None else ntot
    s = excess_shift(bmin, bmax, ntot)
    w = [max(1, ((1 + int(c)) << (bmax - int(bi))) >> s) for c, bi in zip(np.asarray(gravcost), b)]
    assert max(w) < 1 << 64
    return np.array(w, dtype=np.uint64), s


def find_split(ncpu, work):
    """domain_findSplit_work_balanced with equal speed factors: (start[ncpu], end[ncpu]), sums in the
    reference's order"""
    work = [float(w) for w in work]
    ndomain = len(work)
    total = 0.0
    for w in work:
        total += w
    avg = total / ncpu
    before = avg_before = 0.0
    start, end, s = [], [], 0
    for i in range(ncpu):
        e = s
        w = work[e]
        while (w + before < avg + avg_before) or (i == ncpu - 1 and e < ndomain - 1):
            if ndomain - e > ncpu - i:
                e += 1
            else:
                break
            w += work[e]
        start.append(s)
        end.append(e)
        before += w
        avg_before += avg
        s = e + 1
    return start, end


def splits_from_cells(cell, weight, nranks, level):
    """cells (ints in [0, 8^level)) and uint64 weights -> splits[nranks+1] uint64"""
    hist = np.zeros(8 ** level, np.uint64)
    np.add.at(hist, np.asarray(cell, np.int64), np.asarray(weight, np.uint64))
    start, _ = find_split(nranks, hist.astype(np.float64))
    shift = 63 - 3 * level
    splits = np.array([s << shift for s in start] + [1 << 63], dtype=np.uint64)
    splits[0] = 0
    return splits


def decompose(pos, nranks, level=0, gravcost=None, timebin=None, domain=None):
    """The whole operation on the global arrays.  domain = (corner, center, len): the kept cube; None:
    the extent of the particles.  gravcost / timebin None: every particle weighs 1.
    Returns (splits, (corner, center, len), keys)."""
    pos = np.asarray(pos, np.float64)
    n = len(pos)
    dom = extent(pos) if domain is None else domain
    if level == 0:
        level = histogram_level(n, nranks)
    keys = keys_of(pos, dom[0], dom[2])
    cell = (keys >> np.uint64(63 - 3 * level)).astype(np.int64)
    if gravcost is None:
        w = np.ones(n, np.uint64)
    else:
        w, _ = integer_weights(gravcost, timebin)
    return splits_from_cells(cell, w, nranks, level), dom, keys
