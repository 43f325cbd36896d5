"""The keyed row table under the resident sink table (key: P[].ID) and the resident wind table (key: particle
index), driven through the public entry points only: one script, run on both.  Every double of a row is
key * 64 + column, so a row that ends up under another key, or a column that moved, names where it came from;
rows are compared as integers (their bit patterns).

The state is tests/sequence_cases.py's with 1000 records, 300 of them gas and the others Type 3 or Type 5 by the
parity of their ID, so that either table can hold 257 rows: the key column and the rows x columns gather then
cross a 256-thread block for both row widths.  The eliminations are made as tests/test_gpu_sequence.py makes
them (Mass == 0), and the maps the tables must follow are those that tests/sequence_ref.py restates."""
import numpy as np
import pytest

import sequence_cases as SC
import sequence_ref as R
from common import bindings

pytestmark = pytest.mark.gpu
B = bindings()
EINVAL = -90002
N, NGAS, M = 1000, 300, 257
KINDS = ("sinks", "winds")
_MADE = {}


def _case():
    if "case" not in _MADE:
        case = SC.Case(n=N, ngas=NGAS)
        other = case.ids[NGAS:]
        case.type_of[other] = np.where(other % 2, 3, 5)
        _MADE["case"] = case
    return _MADE["case"]


class Table:
    """one of the two tables on a context that holds _case()"""

    def __init__(self, kind):
        self.kind, self.case = kind, _case()
        case = self.case
        self.fp = SC.load(B.ForcePath(0), case)
        self.type = case.type_of[case.ids]
        sinks = kind == "sinks"
        self.what, self.key_what, self.nc = ("sink", "ID", B.SK_COUNT) if sinks else ("wind", "index", B.WK_COUNT)
        self.set, self.get = (self.fp.sinks_set_table, self.fp.sinks_table) if sinks else (
            self.fp.winds_set_table, self.fp.winds_table)
        self.owners = np.nonzero(self.type == (5 if sinks else 3))[0]      # slots, ascending
        assert len(self.owners) >= M + 20
        self.spare, self.owners = self.owners[M:], self.owners[:M]         # particles of the type without a row

    def keys(self, slots):
        slots = np.asarray(slots, np.int64)
        return (self.case.ids[slots] if self.kind == "sinks" else slots).astype(np.int64)

    def rows(self, keys):
        return np.asarray(keys, np.float64)[:, None] * 64.0 + np.arange(self.nc)[None, :]

    def give(self, keys, seed=1):
        keys = np.asarray(keys, np.int64)
        p = np.random.default_rng(seed).permutation(len(keys))
        self.set(keys[p], self.rows(keys)[p])

    def holds(self, keys, content=None):
        """the table has exactly `keys`, ascending, and under keys[r] the row made for content[r]"""
        keys = np.asarray(keys, np.int64)
        content = keys if content is None else np.asarray(content, np.int64)
        got_k, got_r = self.get()
        assert got_r.shape == (len(keys), self.nc)
        assert np.array_equal(got_k.astype(np.int64), keys), (got_k[:8], keys[:8])
        assert (np.diff(got_k.astype(np.int64)) > 0).all()
        want = np.ascontiguousarray(self.rows(content)).view(np.int64)
        got = np.ascontiguousarray(got_r).view(np.int64)
        assert np.array_equal(got, want), "rows differ at %s" % np.argwhere(got != want)[:5].tolist()

    def close(self):
        self.fp.close()


@pytest.fixture(params=KINDS)
def tab(request):
    t = Table(request.param)
    yield t
    t.close()


@pytest.mark.parametrize("m", [0, 1, 2, M])
def test_shuffled_rows_come_back_sorted_under_their_keys(tab, m):
    keys = tab.keys(tab.owners[:m])
    tab.give(keys, seed=m)
    tab.holds(np.sort(keys))


@pytest.mark.parametrize("where", ["first pair", "last pair", "across 256"])
def test_a_duplicate_key_is_refused_and_named(tab, where):
    keys = np.sort(tab.keys(tab.owners))
    dup = int(keys[{"first pair": 0, "last pair": M - 1, "across 256": 255}[where]])
    both = np.r_[keys, dup]
    at = np.nonzero(np.sort(both) == dup)[0]
    assert at.tolist() == {"first pair": [0, 1], "last pair": [M - 1, M], "across 256": [255, 256]}[where]
    tab.give(keys)
    with pytest.raises(B.GhipError, match=r"two rows of the %s table have the %s %d \(the context holds no table now\)"
                       % (tab.what, tab.key_what, dup)) as e:
        tab.give(both, seed=7)
    assert e.value.code == EINVAL
    with pytest.raises(B.GhipError, match="no %s table" % tab.what) as e:
        tab.get()
    assert e.value.code == EINVAL


@pytest.mark.parametrize("which", ["first", "last", "all", "none"])
def test_rearrange_drops_the_rows_of_eliminated_particles(tab, which):
    case, fp = tab.case, tab.fp
    keys = tab.keys(tab.owners)
    by_key = tab.owners[np.argsort(keys)]                  # the rows' particles in the order of their keys
    gone = {"first": by_key[:1], "last": by_key[-1:], "all": by_key, "none": by_key[:0]}[which]
    # every case eliminates particles without a row as well (gas, the other type, the table's type): the map is
    # never the identity, and both tables go through their filter
    others = np.r_[[0, 5, NGAS - 1], tab.spare[:3], np.nonzero(tab.type == (3 if tab.kind == "sinks" else 5))[0][:3]]
    mass = case.mass_of[case.ids].copy()
    mass[np.r_[gone, others].astype(np.int64)] = 0.0
    fp.set_field(B.F_MASS, mass)
    tab.give(keys, seed=3)
    spec = R.spec_rearrange(tab.type, mass, NGAS)
    res = fp.rearrange()
    assert res.count_elim == len(gone) + len(others) == spec["count_elim"] and res.changed
    new_of_old = fp.sequence_map()[0]
    assert np.array_equal(new_of_old, spec["new_of_old"])
    alive = np.setdiff1d(tab.owners, gone)
    assert len(alive) == M - len(gone)
    old = tab.keys(alive)
    if tab.kind == "sinks":                                # keyed by ID: the surviving rows as they were
        order = np.argsort(old)
        tab.holds(old[order])
    else:                                                  # keyed by index: under the new index of their particle
        new = spec["new_of_old"][alive].astype(np.int64)
        assert (new >= 0).all()
        order = np.argsort(new)
        tab.holds(new[order], content=old[order])
        assert (fp.get_field(B.F_TYPE)[new] == 3).all()


def test_peano_order_moves_the_index_keys_and_not_the_id_keys(tab):
    case, fp = tab.case, tab.fp
    keys = tab.keys(tab.owners)
    tab.give(keys, seed=4)
    old_of_new = R.spec_peano_order(case.key_of()[case.ids], NGAS)
    assert fp.peano_order(SC.CORNER, SC.DLEN) is True
    assert np.array_equal(fp.sequence_map()[1], old_of_new)
    if tab.kind == "sinks":
        tab.holds(np.sort(keys))
    else:
        new_of_old = np.empty(N, np.int64)
        new_of_old[old_of_new] = np.arange(N)
        new = new_of_old[tab.owners]
        order = np.argsort(new)
        assert not np.array_equal(order, np.arange(M)), "the order of the rows changes"
        tab.holds(new[order], content=keys[order])


def test_a_smaller_table_after_a_larger_one(tab):
    """2 rows, then 257, then 1: the buffers keep the capacity of the largest, the table is the last one given"""
    for m, seed in ((2, 1), (M, 2), (1, 3)):
        keys = tab.keys(tab.owners[-m:])
        tab.give(keys, seed=seed)
        tab.holds(np.sort(keys))


@pytest.mark.parametrize("kind", KINDS)
def test_growth_keeps_the_old_rows_and_the_order(kind):
    """one ghip_sfr_form_sinks / one ghip_wind_spawn on the set-ups of test_formation and
    test_spawn_maxpart_tables_and_the_grown_state"""
    if kind == "sinks":
        import sink_accretion_cases as AC
        from test_gpu_sink_accretion import _device, _sfr_params
        sp = AC.stock(1)
        rng = np.random.default_rng(21)
        dens = 0.5 + rng.random(sp.pr.ngas)
        _, fp = _device(sp, gas_density=dens)
        try:
            fp.sinks_set_table(sp.ids[sp.sinks], AC.rows_of(B, AC.state_for(sp)))
            k0, r0 = fp.sinks_table()
            cand = fp.sfr_cooling(_sfr_params(B, sp.pr, float(np.quantile(dens, 0.95))))
            assert len(cand) > 20
            fp.sfr_form_sinks(len(cand), rng.random(len(cand)), 1)
            k1, r1 = fp.sinks_table()
        finally:
            fp.close()
        grown = len(cand)
    else:
        from test_gpu_wind_resident import SpawnCase
        sc = SpawnCase(1)
        fp = sc.device(B)
        try:
            k0, r0 = fp.winds_table()
            grown = fp.wind_spawn(sc.gparams(B), sc.rnd)["spawned"]
            assert grown > 256
            k1, r1 = fp.winds_table()
        finally:
            fp.close()
    assert len(k0) > 0 and len(k1) == len(k0) + grown
    assert (np.diff(k1.astype(np.int64)) > 0).all()
    at = np.searchsorted(k1, k0)
    assert np.array_equal(k1[at], k0)
    assert np.array_equal(np.ascontiguousarray(r1[at]).view(np.int64), np.ascontiguousarray(r0).view(np.int64))
