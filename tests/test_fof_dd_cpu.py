"""CPU-side checks of the friends-of-friends groups on shards (GHIP_DD_GLOBAL_QUANTITIES begun with walk =
GHIP_FOF_FORM): include/ghip.h, the version script csrc/ghip.map, the library and gadget-leicester_amd/bindings.py
agree on the form, the argument struct and the two new symbols; no operation code was added; the sharded module
offers the operation.  No compute entry point is called."""
import ctypes as C
import fnmatch
import importlib
import os
import re

import numpy as np

from common import REPO, bindings, pkg

NEW_SYMBOLS = ("ghip_fof_get_maxdens_task", "ghip_dd_fof_args_size")


def _header():
    return open(os.path.join(REPO, "include", "ghip.h")).read()


def test_the_form_is_a_walk_value_not_an_operation():
    B = bindings()
    h = _header()
    m = re.search(r"#define\s+GHIP_FOF_FORM\s+(\d+)\b", h)
    assert m and int(m.group(1)) == 1 == B.FOF_FORM
    ops = dict((k, int(v)) for k, v in re.findall(r"#define\s+GHIP_DD_([A-Z_]+)\s+(\d+)\b", h))
    assert "FOF" not in ops and "FOF_FORM" not in ops
    assert len(set(ops.values())) == len(ops), "two operations share a code"
    assert max(ops.values()) < 16 and len(ops) == 15          # codes 1..15, as before
    assert ops["GLOBAL_QUANTITIES"] == 12 == B.DD_GLOBAL_QUANTITIES
    for name, code in ops.items():
        assert getattr(B, "DD_" + name) == code, name


def test_new_symbols_are_declared_exported_and_bound():
    B = bindings()
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    globs = re.findall(r"^\s*([A-Za-z_*][A-Za-z0-9_*]*);", open(os.path.join(pkg.CSRC, "ghip.map")).read().split(
        "local:")[0].split("global:")[1], flags=re.M)
    assert globs, "csrc/ghip.map lists no global symbols"
    L = C.CDLL(pkg.lib_path())
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), "%s is not declared in ghip.h" % name
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), "%s is not exported by ghip.map" % name
        assert hasattr(L, name), "libghip.so does not export %s" % name
        assert name in B.EXPORTS
        assert getattr(B.lib(), name).argtypes is not None, "%s has no argument types in bindings.py" % name


def test_argument_struct():
    B = bindings()
    m = re.search(r"typedef struct\s*\{([^}]*)\}\s*ghip_dd_fof_args;", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S))
    assert m, "ghip_dd_fof_args is not declared"
    members = re.findall(r"\*\s*([a-z_]+)\s*;", m.group(1))
    assert members == ["p", "out", "counts"] == [k for k, _ in B.DdFofArgs._fields_]
    assert C.sizeof(B.DdFofArgs) == 3 * C.sizeof(C.c_void_p) == B.lib().ghip_dd_fof_args_size()
    A, keep = B.dd_fof_args(link_length=0.25, primary_types=2, secondary_types=49, group_min_len=7, boxsize=2.0,
                            periodic=True, max_iter=11)
    p = A.p.contents
    assert (p.LinkL, p.primary_types, p.secondary_types, p.group_min_len, p.BoxSize, p.periodic, p.MaxIter) == \
        (0.25, 2, 49, 7, 2.0, 1, 11)
    assert C.addressof(A.out.contents) == C.addressof(keep["out"])
    assert C.addressof(A.counts.contents) == keep["counts"].ctypes.data
    assert keep["counts"].dtype == np.int64 and len(keep["counts"]) == 8 == len(B.FOF_COUNTS)


def test_sharded_module_offers_the_operation():
    sh = importlib.import_module("gadget-leicester_amd.sharded")
    for cls in (sh.DomainShards, sh.DomainRank):
        assert callable(getattr(cls, "fof"))
    assert callable(bindings().ForcePath.fof_maxdens_task)
