"""fof.c restated in NumPy: the serial list merging of fof_find_groups, the nearest-primary search of the
secondary types, the catalogue and the group properties.  Test infrastructure only: the reference every device
result of ghip_fof is compared with (tests/test_gpu_fof.py), itself pinned against an independent construction
(tests/test_fof_cpu.py).

What is restated, with the places in the reference:
  link_pairs          ngb_treefind_fof_primary (ngb.c:351-368): two primaries are neighbours when the
                      nearest-image distance satisfies r2 <= LinkL^2 (the loop continues on r2 > LinkL^2)
  find_groups         fof_find_dmparticles_evaluate, mode 0 (fof.c:645-680): Head / Tail / Next / Len lists, the
                      shorter list is appended to the longer, MinID of the head is the minimum of both
  linklength_rule     fof.c:112-124
  nearest_primary     fof_find_nearest_dmparticle(_evaluate) (fof.c:1434-1776): h = Hsml (gas) or 0.1 LinkL,
                      nearest primary with r2 < h^2, h doubled for those that found none, iter > MAXITER fails
  catalogue           fof_compile_catalogue (fof.c:710-898), fof_compute_group_properties (fof.c:900-974),
                      fof_finish_group_properties (fof.c:1081-1119), GrNr / Offset as fof_save_groups assigns them
                      (fof.c:1122-1250: groups by Len descending, the ID list by (GrNr, ID))

Two deliberate deviations, the same the device library makes:
  1. equally distant primaries of a secondary: the one with the smaller ID (the reference keeps the first in the
     order of its tree traversal, fof.c:1734);
  2. the reference position of the periodic centre of mass is the member that carries MinID (the reference reads
     P[start], fof.c:921 / 968, with `start` an index into the sorted FOF_PList: some unrelated particle).
Groups of equal Len are ordered by MinID (the reference leaves them to qsort).  The search radii are doubles (the
reference keeps them in floats, fof.c:1446-1447).

The neighbour search itself (which pairs to test) stands for the reference's tree walk and uses scipy's cKDTree
with a slightly enlarged radius; every candidate pair is then decided by the arithmetic above.
"""
import numpy as np
from scipy.spatial import cKDTree


class NoConvergence(RuntimeError):
    """endrun(1159): failed to converge in fof-nearest"""


def nearest(d, box, periodic):
    """the nearest image of a coordinate difference (ngb.c NGB_PERIODIC_LONG / fof.c:1719-1732)"""
    d = np.array(d, dtype=np.float64, copy=True)
    if periodic:
        half = 0.5 * box
        d[d > half] -= box
        d[d < -half] += box
    return d


def fof_periodic(d, box):
    """fof.c:2273-2280"""
    d = np.array(d, dtype=np.float64, copy=True)
    d[d >= 0.5 * box] -= box
    d[d < -0.5 * box] += box
    return d


def fof_periodic_wrap(x, box):
    """fof.c:2283-2290"""
    x = float(x)
    while x >= box:
        x -= box
    while x < 0:
        x += box
    return x


def _kdtree(pos, box, periodic):
    if periodic:
        p = np.mod(pos, box)
        p[p >= box] = 0.0
        return cKDTree(p, boxsize=box)
    return cKDTree(pos)


def primaries(ptype, primary_types):
    ptype = np.asarray(ptype)
    return np.where(((1 << ptype) & primary_types) != 0)[0]


def secondaries(ptype, primary_types, secondary_types):
    ptype = np.asarray(ptype)
    return np.where((((1 << ptype) & secondary_types) != 0) & (((1 << ptype) & primary_types) == 0))[0]


def link_pairs(pos, prim, linkl, box, periodic):
    """all pairs (i < j) of primaries (particle indices) with r2 <= LinkL^2, sorted by (i, j)"""
    if len(prim) < 2:
        return np.zeros((0, 2), np.int64)
    pp = pos[prim]
    cand = _kdtree(pp, box, periodic).query_pairs(linkl * (1 + 1e-9) + 1e-300, output_type="ndarray")
    if len(cand) == 0:
        return np.zeros((0, 2), np.int64)
    d = nearest(pp[cand[:, 0]] - pp[cand[:, 1]], box, periodic)
    r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    keep = ~(r2 > linkl * linkl)          # ngb.c:366: `if(r2 > hsml * hsml) continue;`
    pairs = np.sort(prim[cand[keep]], axis=1)
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    return pairs[order].astype(np.int64)


def find_groups(n, ids, pairs):
    """fof.c:153-160 and 645-680 over the neighbour pairs -> (Head, MinID): MinID[Head[i]] labels particle i"""
    Head = list(range(n))
    Tail = list(range(n))
    Next = [-1] * n
    Len = [1] * n
    MinID = [int(x) for x in ids]
    for target, j in pairs.tolist():
        if Head[target] != Head[j]:                      # only if not yet linked
            if Len[Head[target]] > Len[Head[j]]:         # p group is longer
                p, s = target, j
            else:
                p, s = j, target
            hp, hs = Head[p], Head[s]
            Next[Tail[hp]] = hs
            Tail[hp] = Tail[hs]
            Len[hp] += Len[hs]
            ss = hs
            while ss >= 0:
                Head[ss] = hp
                ss = Next[ss]
            if MinID[hs] < MinID[hp]:
                MinID[hp] = MinID[hs]
    return np.array(Head, np.int64), np.array(MinID, np.int64)


def linklength_rule(mass, ptype, primary_types, linklength, rhodm):
    """fof.c:112-124"""
    prim = primaries(ptype, primary_types)
    masstot = 0.0
    for m in np.asarray(mass, np.float64)[prim]:
        masstot += m
    return linklength * (masstot / len(prim) / rhodm) ** (1.0 / 3)


def nearest_primary(pos, ptype, ids, hsml, prim, sec, label, linkl, box, periodic, max_iter):
    """labels of the secondaries -> (label, iterations); raises NoConvergence when iter > max_iter"""
    label = label.copy()
    if len(sec) == 0:
        return label, 0
    h = np.where(ptype[sec] == 0, hsml[sec], 0.1 * linkl).astype(np.float64)    # fof.c:1454-1457
    tree = _kdtree(pos[prim], box, periodic)
    todo = np.arange(len(sec))
    it = 0
    while True:
        todo = np.asarray(todo, np.int64)
        q = np.mod(pos[sec[todo]], box) if periodic else pos[sec[todo]]
        if periodic:
            q[q >= box] = 0.0
        # (a periodic search reaches at most half a box: beyond that every primary is a candidate)
        r = h[todo] * (1 + 1e-9) + 1e-300
        far = r >= 0.5 * box if periodic else np.zeros(len(todo), bool)
        cands = tree.query_ball_point(q, np.where(far, 0.0, r))
        everybody = list(range(len(prim)))
        cands = [everybody if fr else cl for cl, fr in zip(cands, far.tolist())]
        cnt = np.array([len(cl) for cl in cands], np.int64)
        kk = np.repeat(todo, cnt)                                   # the secondary of every candidate pair
        jj = prim[np.concatenate([np.asarray(cl, np.int64) for cl in cands])] if cnt.sum() else np.zeros(0, np.int64)
        d = nearest(pos[sec[kk]] - pos[jj], box, periodic)
        r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        ok = r2 < h[kk] * h[kk]                                      # fof.c:1734
        kk, jj, r2 = kk[ok], jj[ok], r2[ok]
        order = np.lexsort((ids[jj], r2, kk))                        # per secondary: nearest first, then smaller ID
        kk, jj = kk[order], jj[order]
        first = np.r_[True, kk[1:] != kk[:-1]] if len(kk) else np.zeros(0, bool)
        label[sec[kk[first]]] = label[jj[first]]                     # fof.c:1760: MinID[Head[index]]
        found = np.zeros(len(sec), bool)
        found[kk[first]] = True
        left = todo[~found[todo]]
        h[left] *= 2.0                                               # fof.c:1625
        left = left.tolist()
        if not left:
            return label, it
        it += 1
        if it > max_iter:                                # fof.c:1647-1652
            raise NoConvergence("failed to converge in fof-nearest")
        todo = left


def fof(pos, vel, mass, ptype, ids, hsml=None, density=None, ngas=0, linkl=0.0, linklength=0.2, rhodm=0.0,
        primary_types=2, secondary_types=0, group_min_len=32, box=0.0, periodic=False, max_iter=150):
    """fof_fof(): dict(LinkL, label [n], grnr [n], Ngroups, Nids, largest, nearest_iterations, ids [Nids],
    groups = dict of arrays per kept group in GrNr order)"""
    pos = np.asarray(pos, np.float64)
    vel = np.asarray(vel, np.float64)
    mass = np.asarray(mass, np.float64)
    ptype = np.asarray(ptype, np.int64)
    ids = np.asarray(ids, np.int64)
    n = len(pos)
    hsml = np.zeros(n) if hsml is None else np.asarray(hsml, np.float64)
    density = np.zeros(ngas) if density is None else np.asarray(density, np.float64)
    if not linkl > 0:
        linkl = linklength_rule(mass, ptype, primary_types, linklength, rhodm)
    prim = primaries(ptype, primary_types)
    sec = secondaries(ptype, primary_types, secondary_types)
    pairs = link_pairs(pos, prim, linkl, box, periodic)
    Head, MinID = find_groups(n, ids, pairs)
    label = MinID[Head]                                  # fof.c:183-187
    label, iters = nearest_primary(pos, ptype, ids, hsml, prim, sec, label, linkl, box, periodic, max_iter)
    out = catalogue(pos, vel, mass, ptype, ids, density, ngas, label, group_min_len, box, periodic)
    out.update(LinkL=linkl, nearest_iterations=iters)
    return out


def catalogue(pos, vel, mass, ptype, ids, density, ngas, label, group_min_len, box, periodic):
    n = len(pos)
    order = np.lexsort((ids, label))                     # FOF_PList by MinID (fof.c:716), members by ID
    lab_s = label[order]
    start = np.r_[0, np.where(lab_s[1:] != lab_s[:-1])[0] + 1]
    length = np.diff(np.r_[start, n])
    minid = lab_s[start]
    keep = np.where(length >= max(1, group_min_len))[0]  # fof.c:876-892
    rank = keep[np.lexsort((minid[keep], -length[keep]))]   # Len descending, MinID ascending
    ng = len(rank)
    G = dict(Len=np.zeros(ng, np.int64), Offset=np.zeros(ng, np.int64), MinID=np.zeros(ng, np.int64),
             GrNr=np.arange(ng), LenType=np.zeros((ng, 6), np.int64), MassType=np.zeros((ng, 6)), Mass=np.zeros(ng),
             CM=np.zeros((ng, 3)), Vel=np.zeros((ng, 3)), MaxDens=np.zeros(ng), index_maxdens=np.full(ng, -1, np.int64))
    grnr = np.full(n, -1, np.int64)
    idlist = []
    off = 0
    for g, s in enumerate(rank):
        mem = order[start[s]:start[s] + length[s]]       # sorted by ID: mem[0] carries MinID
        G["Len"][g], G["Offset"][g], G["MinID"][g] = length[s], off, minid[s]
        off += length[s]
        grnr[mem] = g
        idlist.append(ids[mem])
        m, t = mass[mem], ptype[mem]
        for k in range(6):
            G["LenType"][g, k] = int((t == k).sum())
            G["MassType"][g, k] = m[t == k].sum()
        G["Mass"][g] = m.sum()
        ref = pos[mem[0]]                                # deviation 2 (the reference: P[start], fof.c:921)
        x = fof_periodic(pos[mem] - ref, box) if periodic else pos[mem]   # fof.c:964-970
        cm = (m[:, None] * x).sum(axis=0) / G["Mass"][g]
        if periodic:
            cm = np.array([fof_periodic_wrap(cm[k] + ref[k], box) for k in range(3)])   # fof.c:1094-1098
        G["CM"][g] = cm
        G["Vel"][g] = (m[:, None] * vel[mem]).sum(axis=0) / G["Mass"][g]
        gas = mem[(t == 0) & (mem < ngas)]
        if len(gas):                                     # fof.c:950-961, starting from MaxDens = 0
            d = density[gas]
            if d.max() > 0:
                G["MaxDens"][g] = d.max()
                G["index_maxdens"][g] = int(gas[d == d.max()].min())
    return dict(label=label, grnr=grnr, Ngroups=ng, Nids=int(off), largest=int(G["Len"].max()) if ng else 0,
                ids=np.concatenate(idlist) if idlist else np.zeros(0, np.int64), groups=G)


def same_partition(a, b):
    """do two label arrays describe the same partition?"""
    a, b = np.asarray(a), np.asarray(b)
    if len(a) != len(b):
        return False
    _, ia = np.unique(a, return_inverse=True)
    _, ib = np.unique(b, return_inverse=True)
    fa = {}
    fb = {}
    for x, y in zip(ia.tolist(), ib.tolist()):
        if fa.setdefault(x, y) != y or fb.setdefault(y, x) != x:
            return False
    return True
