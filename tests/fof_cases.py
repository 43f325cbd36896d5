"""Inputs of the friends-of-friends tests (tests/test_fof_cpu.py, tests/test_gpu_fof.py): dicts with the particle
arrays and the call's parameters, small enough for tests/fof_ref.py to take a second each.  Particle order as the
library expects it: the gas block first (allvars.h:1384)."""
import numpy as np

PRIMARY = 2                 # FOF_PRIMARY_LINK_TYPES: halo particles
SECONDARY = 1 + 16 + 32     # FOF_SECONDARY_LINK_TYPES: gas, stars, black holes


def _finish(pos, ptype, box, periodic, linkl, seed, **par):
    rng = np.random.default_rng(seed + 77)
    n = len(pos)
    ptype = np.asarray(ptype, np.int32)
    ngas = int((ptype == 0).sum())
    assert np.all(ptype[:ngas] == 0)
    mass = np.where(ptype == 1, 1.0, 0.17) * (1 + 0.1 * rng.random(n))
    hsml = np.zeros(n)
    hsml[:ngas] = linkl * rng.uniform(0.3, 3.0, ngas)
    c = dict(pos=np.ascontiguousarray(pos, np.float64), vel=rng.standard_normal((n, 3)), mass=mass, type=ptype,
             ids=(rng.permutation(n) * 3 + 7).astype(np.int32), hsml=hsml, density=0.5 + rng.random(ngas), ngas=ngas,
             box=float(box), periodic=bool(periodic), linkl=float(linkl), primary_types=PRIMARY,
             secondary_types=SECONDARY, group_min_len=1, max_iter=150)
    c.update(par)
    return c


def ref_args(c, **over):
    """the keyword arguments of fof_ref.fof for a case"""
    a = dict(pos=c["pos"], vel=c["vel"], mass=c["mass"], ptype=c["type"], ids=c["ids"], hsml=c["hsml"],
             density=c["density"], ngas=c["ngas"], linkl=c["linkl"], primary_types=c["primary_types"],
             secondary_types=c["secondary_types"], group_min_len=c["group_min_len"], box=c["box"],
             periodic=c["periodic"], max_iter=c["max_iter"])
    a.update(over)
    return a


def clumps(n, periodic, seed=1, box=1.0):
    """Gaussian clumps on a uniform background: a quarter gas, half halo particles, the rest stars, a few black
    holes and a few Type-2 particles that are neither primary nor secondary.  LinkL = 0.2 mean halo spacings, the
    clumps 1.5 LinkL wide with about 60 halo particles each: a handful of neighbours per particle in the cores."""
    rng = np.random.default_rng(seed)
    ngas = n // 4
    ndm = max(1, n // 2)
    nrest = n - ngas - ndm
    ptype = np.r_[np.zeros(ngas), np.ones(ndm), np.where(np.arange(nrest) % 9 == 0, 5, np.where(np.arange(nrest) % 11 == 0, 2, 4))]
    linkl = 0.2 * box * (1.0 / ndm) ** (1.0 / 3)
    nc = max(1, ndm // 100)
    centre = rng.random((nc, 3)) * box
    centre[0] = (0.001 * box, 0.999 * box, 0.5 * box)          # one clump across two faces
    inclump = rng.random(n) < 0.6
    which = rng.integers(0, nc, n)
    pos = np.where(inclump[:, None], centre[which] + 1.5 * linkl * rng.standard_normal((n, 3)), rng.random((n, 3)) * box)
    if periodic:
        pos = np.mod(pos, box)
        pos[pos >= box] = 0.0
    return _finish(pos, ptype, box, periodic, linkl, seed)


def lattice(linkl):
    """a 4^3 lattice of spacing 0.25 in a periodic box of 1: every coordinate and every r2 is exact"""
    g = np.arange(4) * 0.25
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return _finish(pos, np.ones(64), 1.0, True, linkl, 3, secondary_types=0)


def chain(across_face, n=4097, seed=4):
    """n primaries on a line, 0.9 LinkL apart, in random index order: one group, whatever the bucket of a link"""
    rng = np.random.default_rng(seed)
    box = 1.0
    linkl = 0.8 * box / n / 0.9
    x = (0.05 if not across_face else 0.55) * box + 0.9 * linkl * np.arange(n)
    pos = np.stack([x, np.full(n, 0.37 * box), np.full(n, 0.61 * box)], axis=1)
    if across_face:
        pos = np.mod(pos, box)
    pos = pos[rng.permutation(n)]
    return _finish(pos, np.ones(n), box, True, linkl, seed, secondary_types=0)


def bridge(with_bridge, seed=5):
    """two clumps of 40 whose nearest members are 1.6 LinkL apart, joined by one particle halfway"""
    rng = np.random.default_rng(seed)
    linkl = 0.01
    a = np.array([0.3, 0.3, 0.3]) + 0.8 * linkl * rng.random((40, 3))
    b = a + np.array([0.8 * linkl + 1.6 * linkl, 0, 0])
    a[0] = (0.3 + 0.8 * linkl, 0.3 + 0.4 * linkl, 0.3 + 0.4 * linkl)
    b[0] = a[0] + np.array([1.6 * linkl, 0, 0])
    b[1:, 0] = np.maximum(b[1:, 0], b[0, 0])
    a[1:, 0] = np.minimum(a[1:, 0], a[0, 0])
    pos = np.r_[a, b]
    if with_bridge:
        pos = np.r_[pos, [0.5 * (a[0] + b[0])]]
    return _finish(pos, np.ones(len(pos)), 1.0, False, linkl, seed, secondary_types=0)


def coincident(seed=6):
    """three primaries at one position (and a few others): the tree holds them in one leaf or, with a table of
    random numbers bound, in randomised subnodes"""
    rng = np.random.default_rng(seed)
    pos = rng.random((40, 3))
    pos[11] = pos[23] = pos[5]
    return _finish(pos, np.ones(40), 1.0, True, 0.02, seed, secondary_types=0)


def secondary_rounds(doublings, seed=7):
    """A close pair of primaries (one group), a second group far away, and per entry of `doublings` one star whose
    nearest primary lies at 0.1 LinkL * 2^k * 0.75: found in round k exactly (0.1 LinkL 2^(k-1) < d < 0.1 LinkL 2^k).
    One gas particle whose Hsml already reaches a primary comes first."""
    linkl = 1.0e-4
    prim = np.array([[0.5, 0.5, 0.5], [0.5 + 0.5 * linkl, 0.5, 0.5], [0.1, 0.1, 0.1]])
    stars = [prim[0] - np.array([0, 0.1 * linkl * 2.0 ** k * 0.75, 0]) for k in doublings]
    gas = [prim[2] + np.array([0, 0, 0.3 * linkl])]
    pos = np.r_[gas, prim, stars]
    ptype = np.r_[[0], [1, 1, 1], np.full(len(stars), 4)]
    c = _finish(pos, ptype, 1.0, True, linkl, seed)
    c["hsml"][0] = 0.5 * linkl
    c["doublings"] = max(doublings) if len(doublings) else 0
    return c


def equidistant(seed=8):
    """one star exactly between two primaries of different groups (coordinates exact in binary): the smaller ID"""
    pos = np.array([[0.5, 0.5, 0.5], [0.25, 0.5, 0.5], [0.75, 0.5, 0.5], [0.25, 0.5, 0.5 + 2.0 ** -10]])
    c = _finish(pos, [4, 1, 1, 1], 1.0, False, 2.0 ** -9, seed, secondary_types=16)
    c["ids"] = np.array([50, 30, 20, 40], np.int32)     # groups {1, 3} (MinID 30) and {2} (MinID 20)
    return c


def equal_len(seed=9):
    """six groups of 5 and three of 3, far apart, one of them around the periodic corner"""
    rng = np.random.default_rng(seed)
    linkl = 0.01
    centres = np.r_[[[0.0, 0.0, 0.0]], 0.1 + 0.8 * rng.random((8, 3))]
    sizes = [5, 5, 5, 5, 5, 5, 3, 3, 3]
    pos = np.concatenate([c + 0.4 * linkl * (rng.random((s, 3)) - 0.5) for c, s in zip(centres, sizes)])
    pos = np.mod(pos, 1.0)
    return _finish(pos, np.ones(len(pos)), 1.0, True, linkl, seed, secondary_types=0)
