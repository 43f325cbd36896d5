"""What the wind rows' way through GHIP_DD_MIGRATE rests on, without a GPU: a numpy restatement of the migration's
renumbering (kept gas, received gas, kept others, received others: k_mig_move_old / k_mig_move_new) with the row keys
that follow from it (k_wkm_rekey, k_wkm_pack, k_wkm_unpack of ghip_wind.hip), against a brute-force permutation for
random destination masks on 2, 3 and 8 owners; and the constants and the struct of the new form."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from common import REPO, bindings

HEADER = open(os.path.join(REPO, "include", "ghip.h")).read()


def _exclusive(v):
    return np.concatenate([[0], np.cumsum(v)])[:-1]


def migrate_keys(owner, P, states):
    """states[s] = dict(ngas, type [n], dest [n] (owner of each particle's key), keys (ascending local indices with a
    row), tag [n] (what a test follows a particle by)).  -> per owner: (new tags, new row keys, tag of each row), by
    the scans the device uses.  A row travels as (ordinal in the sender's run for its destination, row)."""
    # the send runs: per destination, the leaving particles in index order (multi_select); a header in front
    runs = [[np.where((st["dest"] == d) & (d != s))[0] for d in range(P)] for s, st in enumerate(states)]
    out = []
    for me, st in enumerate(states):
        n, ng = len(st["type"]), st["ngas"]
        stay = st["dest"] == me
        gas = np.arange(n) < ng
        ro_gas, ro_oth = _exclusive(stay & gas), _exclusive(stay & ~gas)
        kg, ko = int((stay & gas).sum()), int((stay & ~gas).sum())
        # the receive buffer: sender ascending, [header] + its run for me
        rec = []                                             # (sender, ordinal or -1 for the header)
        first = {}
        for s in range(P):
            if s == me:
                continue
            rec.append((s, -1))
            first[s] = len(rec)
            rec += [(s, o) for o in range(len(runs[s][me]))]
        isgas = np.array([o >= 0 and runs[s][me][o] < states[s]["ngas"] for s, o in rec], bool)
        isoth = np.array([o >= 0 and not runs[s][me][o] < states[s]["ngas"] for s, o in rec], bool)
        rn_gas, rn_oth = _exclusive(isgas), _exclusive(isoth)
        rg, ro_n = int(isgas.sum()), int(isoth.sum())
        nn, ngn = kg + ko + rg + ro_n, kg + rg
        tag = np.full(nn, -1, np.int64)
        for i in np.where(stay)[0]:
            tag[ro_gas[i] if gas[i] else ngn + ro_oth[i]] = st["tag"][i]
        for q, (s, o) in enumerate(rec):
            if o >= 0:
                tag[kg + rn_gas[q] if isgas[q] else ngn + ko + rn_oth[q]] = states[s]["tag"][runs[s][me][o]]
        # the rows: staying ones re-keyed, arriving ones keyed through (first[sender] + ordinal)
        keys, rowtag = [], []
        for i in st["keys"]:
            if stay[i]:
                keys.append(ngn + ro_oth[i])
                rowtag.append(st["tag"][i])
        for s in range(P):
            if s == me:
                continue
            have = set(states[s]["keys"].tolist())
            for o, i in enumerate(runs[s][me]):
                if states[s]["type"][i] == 3 and int(i) in have:
                    q = first[s] + o
                    assert isoth[q]
                    keys.append(ngn + ko + rn_oth[q])
                    rowtag.append(states[s]["tag"][i])
        order = np.argsort(keys, kind="stable")
        out.append((tag, np.array(keys, np.int64)[order], np.array(rowtag, np.int64)[order], ngn))
    return out


def _random_states(P, rng, mode):
    states, next_tag = [], 0
    for s in range(P):
        ng, no = int(rng.integers(0, 40)), int(rng.integers(1, 60))
        n = ng + no
        typ = np.concatenate([np.zeros(ng, np.int32), rng.choice([1, 3, 3, 5], no).astype(np.int32)])
        if mode == "empty":
            dest = np.full(n, s)
        elif mode == "all_leave" and s == 0:
            dest = rng.integers(1, P, n)
        else:
            dest = np.where(rng.random(n) < 0.6, s, rng.integers(0, P, n))
        w = np.where(typ == 3)[0]
        keys = w[rng.random(len(w)) < 0.8] if s != P - 1 else w[:0]       # some without rows; one empty table
        states.append(dict(ngas=ng, type=typ, dest=dest, keys=keys, tag=np.arange(next_tag, next_tag + n)))
        next_tag += n
    return states


@pytest.mark.parametrize("P", [2, 3, 8])
@pytest.mark.parametrize("mode", ["random", "empty", "all_leave"])
def test_renumbering_and_row_keys_against_a_brute_force_permutation(P, mode):
    rng = np.random.default_rng(100 * P + len(mode))
    for _ in range(5):
        states = _random_states(P, rng, mode)
        got = migrate_keys(None, P, states)
        had_row = {int(st["tag"][i]) for st in states for i in st["keys"]}
        seen = set()
        for me in range(P):
            # brute force: everybody whose key names me, gas first; within a block the kept ones in their order,
            # then the arrivals by sender and by their order there
            gas, oth = [], []
            for s in [me] + [s for s in range(P) if s != me]:
                st = states[s]
                for i in np.where(st["dest"] == me)[0]:
                    (gas if i < st["ngas"] else oth).append((st["tag"][i], st["type"][i]))
            want = gas + oth
            tag, keys, rowtag, ngn = got[me]
            assert ngn == len(gas) and np.array_equal(tag, [t for t, _ in want])
            assert np.all(np.diff(keys) > 0)
            for k, t in zip(keys, rowtag):
                assert tag[k] == t and want[k][1] == 3 and k >= ngn
                seen.add(int(t))
            if mode == "empty":
                assert np.array_equal(keys, states[me]["keys"])
        assert seen == had_row                                # no row lost, none made
        if mode == "all_leave":
            assert len(got[0][1]) == sum(1 for s in range(1, P) for i in states[s]["keys"]
                                         if states[s]["dest"][i] == 0)


def _define(name):
    m = re.search(r"#define\s+%s\s+(\d+)" % name, HEADER)
    assert m, name
    return int(m.group(1))


def test_the_form_constants():
    B = bindings()
    assert _define("GHIP_WINDS_RESIDENT_FORM") == 32 == B.WINDS_RESIDENT_FORM
    assert _define("GHIP_WINDS_SPAWN_FORM") == 33 == B.WINDS_SPAWN_FORM
    assert (_define("GHIP_WIND_FORM"), _define("GHIP_WIND_DENSITY_FORM"), _define("GHIP_WIND_SPREAD_FORM")) == (16, 17, 18)
    assert (B.WIND_FORM, B.WIND_DENSITY_FORM, B.WIND_SPREAD_FORM) == (16, 17, 18)
    # GHIP_WIND_SPREAD_FORM + 1 is still not a form: no name of ghip.h or of the bindings has the value 19
    forms = {n: int(v) for n, v in re.findall(r"#define\s+(GHIP_\w*FORM)\s+(\d+)", HEADER)}
    assert 19 not in forms.values(), forms
    assert all(getattr(B, k) != 19 for k in dir(B) if k.endswith("_FORM"))
    # no operation code was added
    assert _define("GHIP_DD_PM_NONPERIODIC") == 15 and "GHIP_DD_DUST_DRAG" in re.search(
        r"#define\s+GHIP_DD_WIND\s+(\w+)", HEADER).group(1)


def test_the_args_struct_has_the_library_size():
    B = bindings()
    L = B.lib()
    assert L.ghip_dd_winds_args_size() == C.sizeof(B.DdWindsArgs) == 6 * C.sizeof(C.c_void_p)
