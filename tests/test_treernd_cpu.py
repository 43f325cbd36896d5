"""CPU checks of the randomised-subnode tree (the reference without -DNOTREERND): the trie of digit strings
of tests/treernd_ref.py -- the definition the device build follows (ghip_set_rnd_table) --
against the oracle's insertion tree, whose `tiny_rng(index + depth)` is the table `tiny_rng(j)` read with
ID = index; and the properties the oracle cannot express (any IDs, the table's modulus and wrap).
"""
import numpy as np
import pytest

import treernd_ref as R
from common import O, Problem

NTABLE = 262144
SCALES = [1.0, 1.0e-3, 1.0e-6]


def _state():
    ic, pick = R.standard_state()
    return Problem(ic=ic, periodic=0), pick


def _oracle_cells(pr, soft, toplevels=0):
    ic = pr.ic
    T = O.Tree(ic["pos"], ic["vel"], ic["mass"], ic["type"], soft, hsml=pr.hsml0, extent=pr.extent,
               toplevels=toplevels)
    od = T.dump()
    cells = np.column_stack([od["len"], od["center"]])
    return T, od, cells


def _assert_same_tree(tr, pr, od, cells):
    n = pr.n
    mine = np.asarray(tr.cells)
    assert len(mine) == len(cells)
    om, oo = np.lexsort(mine.T[::-1]), np.lexsort(cells.T[::-1])
    assert np.array_equal(mine[om], cells[oo])                         # identical cells, bit for bit
    # fathers of the particles: the same cell
    assert np.array_equal(tr.father_cells(), cells[od["p_father"] - n])
    # fathers of the nodes
    o2m = np.empty(len(cells), np.int64)
    o2m[oo] = om                                                       # oracle rank -> trie index
    nf = np.asarray(tr.node_father)
    of = od["father"]
    want = np.where(of >= 0, o2m[np.maximum(of - n, 0)], -1)
    assert np.array_equal(nf[o2m], want)
    # per-cell particle sets: the oracle's follow from the fathers
    count = np.zeros(len(cells), np.int64)
    f = od["p_father"] - n
    alive = np.ones(n, bool)
    while alive.any():
        np.add.at(count, f[alive], 1)
        nxt = of[f] - n
        alive &= of[f] >= 0
        f = np.where(alive, nxt, f)
    assert np.array_equal(np.array([len(m) for m in tr.members])[o2m], count)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("toplevels", [0, 2])
def test_trie_is_the_oracles_insertion_tree(scale, toplevels):
    pr, _ = _state()
    soft = pr.force_soft * scale
    T, od, cells = _oracle_cells(pr, soft, toplevels)
    tr = R.build(pr.ic["pos"], np.arange(pr.n), pr.ic["type"], soft, R.tiny_table(NTABLE), pr.extent,
                 toplevels=toplevels)
    print("softening x %g, toplevels %d: %d nodes, deepest level %d" % (scale, toplevels, tr.numnodes, tr.maxdepth))
    assert tr.maxdepth < 42                                            # inside the device's two key words
    _assert_same_tree(tr, pr, od, cells)


def test_the_state_has_cells_only_the_randomisation_separates():
    """without the rule (softening 0: no cell is ever small enough) the coincident groups never part"""
    pr, _ = _state()
    with pytest.raises(RuntimeError):
        R.build(pr.ic["pos"], np.arange(pr.n), pr.ic["type"], np.zeros(6), R.tiny_table(NTABLE), pr.extent,
                maxdepth=80)


def test_trie_does_not_depend_on_the_particle_order():
    pr, _ = _state()
    rng = np.random.default_rng(3)
    ids = rng.permutation(pr.n).astype(np.uint32) * np.uint32(977) + np.uint32(5)
    table = rng.random(NTABLE)
    soft = pr.force_soft * 1.0e-3
    a = R.build(pr.ic["pos"], ids, pr.ic["type"], soft, table, pr.extent)
    p = rng.permutation(pr.n)
    b = R.build(pr.ic["pos"][p], ids[p], pr.ic["type"][p], soft, table, pr.extent)
    ca, cb = np.asarray(a.cells), np.asarray(b.cells)
    oa, ob = np.lexsort(ca.T[::-1]), np.lexsort(cb.T[::-1])
    assert np.array_equal(ca[oa], cb[ob])
    assert np.array_equal(a.father_cells()[p], b.father_cells())
    # ... and the members, named by ID
    for ka, kb in zip(oa[::17], ob[::17]):
        assert np.array_equal(np.sort(ids[a.members[ka]]), np.sort(ids[p][b.members[kb]]))


def test_modulus_and_wrap_of_the_table_index():
    """IDs >= ntable: (ID + d) % (ntable + (d & 3)) % ntable.  Three coincident particles, a table of 8
    entries: the digits are checked against the formula written out by hand."""
    ntable = 8
    table = (np.arange(ntable) + 0.5) / ntable                          # digit = index
    pos = np.array([[0.3, 0.3, 0.3]] * 3 + [[0.9, 0.1, 0.5], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    ids = np.array([8, 11, 2 ** 32 - 1, 1, 2, 3], np.uint64)
    extent = (np.zeros(3), np.full(3, 0.5), 1.0)
    soft = np.full(6, 1.0e3 * 2.0 ** -3)                                # cells of len < 2^-3 randomise: depth >= 4
    tr = R.build(pos, ids, np.ones(6, np.int32), soft, table, extent)
    cells = np.asarray(tr.cells)

    def digit(i, d):
        u = (int(ids[i]) + d) % 2 ** 32
        return (u % (ntable + (d & 3))) % ntable

    # walk the three down by hand from depth 4 on: they part where their digits first differ
    for a, b in ((0, 1), (0, 2), (1, 2)):
        d = 4
        while digit(a, d) == digit(b, d):
            d += 1
        shared = [k for k in range(len(cells)) if a in tr.members[k] and b in tr.members[k]]
        assert max(tr.depth[k] for k in shared) == d
    # d & 3 == 0 wraps at ntable, the others do not: ID 8 at depth 4 reads entry 4, ID 11 at depth 5 entry
    # (16 % 9) = 7, ID 2^32 - 1 at depth 5 entry (4 % 9) = 4 (the sum wraps in 32 bits)
    assert digit(0, 4) == 4 and digit(1, 5) == 7 and digit(2, 5) == 4
