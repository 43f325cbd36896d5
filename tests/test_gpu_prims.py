"""The device scans, selections and the 32-bit pair sort (ghip_prim.hip) on their own, through
ghip_debug_prim: exact against numpy at the sizes where an offset can go wrong -- the edges of a
wavefront (64), of one block of 16 x 64 items, and of the 64 blocks that one round of the
block-offsets loop covers.  Both forms of the scan and of the selection are held to the same numpy
result, and so to each other.
"""
import numpy as np
import pytest

from common import bindings

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 65536, 65537]
DENSITIES = [0.0, 0.03, 0.5, 1.0]


@pytest.fixture(scope="module")
def fp():
    f = bindings().ForcePath(0)
    yield f
    f.close()


def _flags(n, density, seed):
    rng = np.random.default_rng(seed)
    if density in (0.0, 1.0):
        return np.full(n, int(density), np.int32)
    return (rng.random(n) < density).astype(np.int32)


@pytest.mark.parametrize("n", SIZES)
def test_both_scans_are_the_shifted_cumsum(fp, n):
    B = bindings()
    rng = np.random.default_rng(1000 + n)
    inputs = [rng.integers(0, 8, n).astype(np.int32)] + [_flags(n, d, 2000 + n) for d in DENSITIES]
    for v in inputs:
        want = np.concatenate(([0], np.cumsum(v, dtype=np.int64)[:-1])).astype(np.int32)
        for prim in (B.PRIM_SCAN, B.PRIM_WSCAN):
            got = fp.debug_prim(prim, v)
            assert np.array_equal(got, want), "prim %d, n %d: first difference at %d" % (
                prim, n, int(np.flatnonzero(got != want)[0]))


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("n", SIZES)
def test_both_selections_are_flatnonzero_in_order(fp, n, density):
    B = bindings()
    f = _flags(n, density, 3000 + n)
    want = np.flatnonzero(f).astype(np.int32)
    vals = np.random.default_rng(4000 + n).integers(0, 2 ** 31 - 1, n).astype(np.int32)
    for prim in (B.PRIM_SELECT, B.PRIM_WSELECT):
        got, cnt = fp.debug_prim(prim, None, f)          # the indices 0..n-1
        assert cnt == int(f.sum()) == len(want), "prim %d: count word %d of %d flags" % (prim, cnt, f.sum())
        assert np.array_equal(got, want), "prim %d, n %d, density %g" % (prim, n, density)
        got, cnt = fp.debug_prim(prim, vals, f)          # a list of the caller's
        assert cnt == len(want)
        assert np.array_equal(got, vals[want]), "prim %d, n %d, density %g (values)" % (prim, n, density)


@pytest.mark.parametrize("end_bit", [12, 30])
@pytest.mark.parametrize("n", [4097, 65537])
def test_pair_sort_returns_the_stable_permutation(fp, n, end_bit):
    B = bindings()
    rng = np.random.default_rng(5000 + n + end_bit)
    # many duplicates: a few hundred distinct keys, spread over all of [0, 2^end_bit)
    pool = rng.integers(0, 2 ** end_bit, 300)
    pool[:2] = (0, 2 ** end_bit - 1)
    keys = pool[rng.integers(0, len(pool), n)].astype(np.int32)
    assert len(np.unique(keys)) < n // 8
    perm = fp.debug_prim(B.PRIM_SORT_U32, keys, end_bit=end_bit)
    assert np.array_equal(perm, np.argsort(keys, kind="stable").astype(np.int32))


def test_debug_prim_refuses_what_it_cannot_run(fp):
    B = bindings()
    one = np.ones(4, np.int32)
    for call in (lambda: fp.debug_prim(17, one),
                 lambda: fp.debug_prim(B.PRIM_SORT_U32, one, end_bit=0),
                 lambda: fp.debug_prim(B.PRIM_SCAN, np.zeros(0, np.int32))):
        with pytest.raises(B.GhipError):
            call()
