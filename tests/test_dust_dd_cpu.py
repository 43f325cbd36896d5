"""CPU checks of the dust passes on domain-decomposed shards (GHIP_DD_DUST_DENSITY / GHIP_DD_DUST_DRAG):
the constants and the argument struct of include/ghip.h match their Python mirrors, and the per-rank
order restatement of tests/dust_dd_ref.py reduces to the single-rank order on one rank."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import dust_dd_ref as DR
import dust_ref as R
from common import REPO, bindings

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ghip.h"
int main(void)
{
  printf("%d %d %zu %zu %zu %zu %zu %zu %zu\n", GHIP_DD_DUST_DENSITY, GHIP_DD_DUST_DRAG,
         sizeof(ghip_dd_dust_args), offsetof(ghip_dd_dust_args, ndust), offsetof(ghip_dd_dust_args, dust_idx),
         offsetof(ghip_dd_dust_args, particle_density), offsetof(ghip_dd_dust_args, dust_radius),
         offsetof(ghip_dd_dust_args, vcoll), offsetof(ghip_dd_dust_args, counts));
  return 0;
}
"""


def test_dd_dust_args_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no C compiler to build the layout probe")
    src = tmp_path / "probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    B = bindings()
    A = B.DdDustArgs
    assert got == [B.DD_DUST_DENSITY, B.DD_DUST_DRAG, C.sizeof(A), A.ndust.offset, A.dust_idx.offset,
                   A.particle_density.offset, A.dust_radius.offset, A.vcoll.offset, A.counts.offset]
    assert got[:2] == [9, 10] and got[2] == 104


def test_dd_dust_args_helper_points_into_its_arrays():
    B = bindings()
    p = B.DustParams()
    dust = np.array([4, 1, 7], np.int32)
    A, a = B.dd_dust_args(p, dust, particle_density=[1.0, 2.0, 3.0], dust_gasvel=np.ones((3, 3)))
    assert A.ndust == 3 and A.dust_idx == a["dust_idx"].ctypes.data
    assert A.particle_density == a["particle_density"].ctypes.data and a["particle_density"][2] == 3.0
    assert A.counts == a["counts"].ctypes.data and a["counts"].shape == (4,)
    assert A.dust_gasvel == a["dust_gasvel"].ctypes.data and a["dust_gasvel"].shape == (3, 3)


def test_one_rank_order_is_the_list_order():
    lst = np.array([5, 2, 9, 0, 3])
    loc = np.array([40, 10, 30, 20, 0])
    (o,) = DR.rank_orders([lst], [loc])
    assert np.array_equal(o, lst)


def test_rank_order_own_list_then_ranks_by_local_index():
    lists = [np.array([3, 0]), np.array([1, 4, 2]), np.array([5])]
    local = [np.array([7, 2]), np.array([9, 1, 5]), np.array([0])]
    o = DR.rank_orders(lists, local)
    assert o[0].tolist() == [3, 0, 4, 2, 1, 5]        # own list, rank 1 by index 1 < 5 < 9, rank 2
    assert o[1].tolist() == [1, 4, 2, 0, 3, 5]        # rank 0 by index 2 < 7
    assert o[2].tolist() == [5, 0, 3, 4, 2, 1]


def test_shard_scatter_on_one_rank_is_gas_scatter():
    rng = np.random.default_rng(3)
    par = R.params(1.0, 1, 1e-3, MinEgySpec=0.5)
    ng, nd = 40, 12
    pos = rng.random((ng + nd, 3))
    mass = np.ones(ng + nd)
    ptype = np.r_[np.zeros(ng, np.int32), np.full(nd, 2, np.int32)]
    dt = np.full(ng + nd, 1e-3)
    gpos, gh = pos[ng:], np.full(nd, 0.4)
    grho, dmom, de = 1 + rng.random(nd), rng.standard_normal((nd, 3)), 5 * rng.random(nd)
    ent0 = rng.random(ng)
    v1, e1, h1 = np.zeros((ng, 3)), ent0.copy(), np.zeros(ng)
    c1 = R.gas_scatter(par, gpos, gh, grho, dmom, de, pos, mass, ptype, ng, dt, v1, e1, h1)
    v2, e2, h2 = np.zeros((ng, 3)), ent0.copy(), np.zeros(ng)
    (c2,) = DR.shard_scatter(par, gpos, gh, grho, dmom, de, pos, mass, ptype, ng, dt, v2, e2, h2,
                             DR.rank_orders([np.arange(nd)], [np.arange(nd)]), [np.arange(ng)])
    assert np.array_equal(v1, v2) and np.array_equal(e1, e2) and np.array_equal(h1, h2)
    assert c1["caps"] == c2["caps"] > 0
