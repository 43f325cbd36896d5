"""CPU-side checks of GHIP_DD_POTENTIAL / GHIP_DD_GLOBAL_QUANTITIES: include/ghip.h, the version script
csrc/ghip.map, the library and gadget-leicester_amd/bindings.py agree on the new symbols, constants and the
argument struct, and the sharded module offers the two operations.  No compute entry point is called."""
import ctypes as C
import fnmatch
import importlib
import os
import re

import numpy as np

from common import REPO, bindings, pkg

NEW_SYMBOLS = ("ghip_get_potential_interactions", "ghip_dd_bytes_sent")


def _header():
    return open(os.path.join(REPO, "include", "ghip.h")).read()


def test_operation_codes_of_header_and_bindings_agree():
    B = bindings()
    ops = dict((k, int(v)) for k, v in re.findall(r"#define\s+GHIP_DD_([A-Z_]+)\s+(\d+)\b", _header()))
    assert ops["POTENTIAL"] == 11 and ops["GLOBAL_QUANTITIES"] == 12
    assert len(set(ops.values())) == len(ops), "two operations share a code"
    assert max(ops.values()) < 16          # (the per-operation traffic counters)
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


def test_argument_struct_of_the_sums():
    B = bindings()
    m = re.search(r"typedef struct\s*\{([^}]*)\}\s*ghip_dd_global_args;", _header())
    assert m, "ghip_dd_global_args is not declared"
    members = re.findall(r"\*\s*([a-z_]+)\s*;", m.group(1))
    assert members == ["p", "out"] == [k for k, _ in B.DdGlobalArgs._fields_]
    assert C.sizeof(B.DdGlobalArgs) == 2 * C.sizeof(C.c_void_p)
    p = B.GlobalParams()
    p.Ti_Current, p.rad_fac = 7, 3.0
    ph = np.arange(5.0)
    A, keep = B.dd_global_args(p, 5, old_photon_momentum=ph)
    assert A.p.contents.Ti_Current == 7 and A.p.contents.rad_fac == 3.0
    assert A.p.contents.OldPhotonMomentum == keep["OldPhotonMomentum"].ctypes.data
    assert not A.p.contents.Potential and not p.OldPhotonMomentum      # the caller's struct keeps no pointers
    assert C.addressof(A.out.contents) == C.addressof(keep["out"])
    assert C.sizeof(B.GlobalSums) % 8 == 0      # (the shards' sums are added as an array of doubles)
    try:
        B.dd_global_args(p, 4, old_photon_momentum=ph)
    except ValueError:
        pass
    else:
        raise AssertionError("a photon array of the wrong length was accepted")


def test_sharded_module_offers_both_operations():
    sh = importlib.import_module("gadget-leicester_amd.sharded")
    for cls in (sh.DomainShards, sh.DomainRank):
        assert callable(getattr(cls, "potential")) and callable(getattr(cls, "global_quantities"))
