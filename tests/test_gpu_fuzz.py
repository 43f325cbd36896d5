"""Slices of tests/gpu_fuzz.py and tests/gpu_ddfuzz.py inside the GPU suite: seeded random problems (distribution, size,
boundaries, softening variant, walk variant, active list) through tree, walks, density and hydro
against the oracle.  `python tests/gpu_fuzz.py N` runs more seeds."""
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(1000, 1010))
def test_random_problem_matches_the_oracle(seed):
    import gpu_fuzz
    gpu_fuzz.one(seed)


@pytest.mark.parametrize("seed", range(10, 15))
def test_random_problems_through_one_context(seed):
    """gpu_fuzz.chain: six random problems (the seeds 100 seed ... 100 seed + 5) one after the other through ONE
    context, each held to the oracle exactly as a problem in a fresh context is"""
    import gpu_fuzz
    infos = gpu_fuzz.chain(seed, 6)
    assert len(infos) == 6
    print(infos)


@pytest.mark.parametrize("seed", [5000, 5003, 5011, 5027, 5036, 6017, 6101, 6204, 5006, 5058])
def test_random_problem_on_random_shards_matches_the_oracle(seed):
    """tests/gpu_ddfuzz.py: the same kind of random problem cut into 2..8 logical shards (some nearly
    empty), gravity + SPH + a shake with migration, against the oracle's single tree.  The last two seeds
    draw converted and swallowed gas records: 5006 under the rule of a sink build (3), 5058 under that of a
    dust build (1)."""
    import gpu_ddfuzz
    gpu_ddfuzz.one(seed)
