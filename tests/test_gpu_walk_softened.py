"""The spline-softened branch of the monopole kernel (r < h, forcetree.c:2150-2171) lives out of
line (ghip_walk.h, d_grav_fac_inside).  The bench's box and the parity sets of test_gpu_parity.py
hardly ever enter it, so these sets are softened over several particle spacings: most particle
pairs of the 1 024 are inside each other's softening length, in both pieces of the spline.  Same
bounds as test_gpu_parity.py: interaction counts exact, fp64 within TOL = 1e-11 of the oracle.
"""
import numpy as np
import pytest

from common import O, Problem, bindings, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-11      # tests/test_gpu_parity.py


def _spline_pieces(pr):
    """number of particle pairs with r < h/2 and with h/2 <= r < h (h: the larger softening of the
    two, nearest image in a periodic box): numpy on the positions, no device involved"""
    pos = pr.ic["pos"]
    h = pr.force_soft[pr.ic["type"]]
    d = pos[:, None, :] - pos[None, :, :]
    if pr.periodic:
        d -= pr.box * np.round(d / pr.box)
    r = np.sqrt((d * d).sum(axis=2))
    hh = np.maximum(h[:, None], h[None, :])
    iu = np.triu_indices(pr.n, 1)
    r, hh = r[iu], hh[iu]
    return int((r < 0.5 * hh).sum()), int(((r >= 0.5 * hh) & (r < hh)).sum())


@pytest.mark.parametrize("unequal", [False, True])
@pytest.mark.parametrize("periodic", [0, 1])
def test_softened_walks_match_the_oracle(periodic, unequal):
    B = bindings()
    pr = Problem(ng=8, gas=True, soft_frac=1.5, periodic=periodic, unequal=unequal)
    assert pr.n == 1024
    inner, outer = _spline_pieces(pr)
    print("pairs with r < h/2: %d, with h/2 <= r < h: %d" % (inner, outer))
    assert inner > 1000 and outer > 1000       # both pieces of the spline are populated
    fp = pr.device()
    pr.device_tree(fp)
    T = pr.oracle_tree()
    tg = np.arange(pr.n, dtype=np.int32)
    # the two passes of test_gravity_two_pass_parity: Barnes-Hut, then the relative criterion
    tab = O.ewald_table(pr.box) if periodic else None
    old = np.zeros(pr.n)
    for theta in (pr.theta, 0.0):
        fp.set_field(B.F_OLDACC, old)
        fp.gravity(pr.g_grav(theta), B.WALK_NEWTON)
        oacc, ocost = T.gravity(pr.o_grav(theta), tg, old)
        assert np.array_equal(fp.get_field(B.F_GRAVCOST), ocost)
        e = relerr(fp.get_field(B.F_GRAVACCEL), oacc)
        print("theta %g newton relerr %.3e" % (theta, e))
        assert e < TOL
        if periodic:
            fp.gravity(pr.g_grav(theta), B.WALK_EWALD)
            T.gravity_ewald_add(pr.o_grav(theta), tab, tg, old, oacc, ocost)
            assert np.array_equal(fp.get_field(B.F_GRAVCOST), ocost)
            e = relerr(fp.get_field(B.F_GRAVACCEL), oacc)
            print("theta %g newton + ewald relerr %.3e" % (theta, e))
            assert e < TOL
        fp.gravity_finish(pr.G)
        old = np.linalg.norm(oacc, axis=1)
    # the short-range walk as test_shortrange_walk_parity sets it up: it also consumes the branch's r
    asmth = 1.25 * pr.box / 16
    rcut = 4.5 * asmth
    old = np.full(pr.n, 3.0)
    for theta in (pr.theta, 0.0):
        fp.set_field(B.F_OLDACC, old)
        fp.gravity(pr.g_grav(theta, rcut, asmth), B.WALK_SHORTRANGE)
        oacc, ocost = T.gravity(pr.o_grav(theta, rcut=rcut, asmth=asmth), tg, old, kind="shortrange")
        assert np.array_equal(fp.get_field(B.F_GRAVCOST), ocost)
        e = relerr(fp.get_field(B.F_GRAVACCEL), oacc)
        print("theta %g shortrange relerr %.3e" % (theta, e))
        assert e < TOL
