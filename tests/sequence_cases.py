"""States for the tests of ghip_rearrange / ghip_peano_order: every value of every field and of every optional
resident array is a function of (ID, component), so that a misplaced value names the record it came from.  A
state is (ids in slot order, ngas) plus per-ID tables of Type, Mass and Pos; what a call must leave behind is
the same function of the expected ID sequence."""
import numpy as np

from common import O, Problem, bindings

B = bindings()
N, NGAS = 4099, 2053
CORNER, DLEN = np.zeros(3), 1.0
OPTIONAL = ("heat", "visc", "inj", "ra", "sink", "drag", "ddm", "newdens")
_PRIME = 1000003


def u(ids, code, c=0):
    """[0, 1), distinct per ID for one (code, c)"""
    return ((np.asarray(ids, np.int64) * 131 + code * 7919 + c * 104729) % _PRIME) / float(_PRIME)


def name(ids, code, c=0):
    """a double that names (ID, code, component) exactly"""
    return np.asarray(ids, np.float64) * 64.0 + code + 0.25 * c


class Case:
    def __init__(self, n=N, ngas=NGAS, converted=(), massless=(), seed=3, tied=False, shuffle=True):
        rng = np.random.default_rng(seed)
        self.n, self.ngas = n, ngas
        self.ids = (rng.permutation(n) if shuffle else np.arange(n)).astype(np.int64)   # slot -> ID
        slot_of = np.empty(n, np.int64)
        slot_of[self.ids] = np.arange(n)
        allid = np.arange(n)
        self.type_of = np.where(slot_of < ngas, 0, 1 + allid % 5).astype(np.int32)
        self.type_of[self.ids[list(converted)]] = 4
        self.mass_of = (1.0 + u(allid, 3)) / max(n, 1)
        self.mass_of[self.ids[list(massless)]] = 0.0
        pos = np.stack([u(allid, 1, c) for c in range(3)], axis=1)
        if tied:   # many records per cell: 4 x 4 x 4 cell centres
            pos = (np.floor(pos * 4) + 0.5) / 4
        self.pos_of = 0.01 + 0.98 * pos
        self._keys = None
        self.h0 = 1.2 * (3.0 * 33.0 / (4 * np.pi * max(ngas, 1))) ** (1.0 / 3.0)

    def key_of(self):
        """domain.c's Key[] per ID in the cube (CORNER, DLEN), from the oracle's table-driven curve"""
        if self._keys is None:
            ip = ((self.pos_of - CORNER) * ((1 << 21) / DLEN)).astype(np.int64)
            self._keys = np.array([O.peano_hilbert_key(*p) for p in ip], dtype=np.uint64)
        return self._keys

    # ---- the state as a function of the ID sequence ----
    def fields(self, ids, ngas):
        I, G = np.asarray(ids, np.int64), np.asarray(ids[:ngas], np.int64)

        def v3(fn, J, code):
            return np.stack([fn(J, code, c) for c in range(3)], axis=1).reshape(len(J), 3)
        vel = 0.01 * (v3(u, I, 2) - 0.5)
        f = {
            B.F_POS: self.pos_of[I].reshape(len(I), 3), B.F_VEL: vel, B.F_MASS: self.mass_of[I],
            B.F_TYPE: self.type_of[I], B.F_OLDACC: 0.2 + u(I, 4), B.F_HSML: self.h0 * (1 + 0.1 * u(I, 5)),
            B.F_TIMEBIN: (1 + I % 3).astype(np.int32), B.F_TI_BEGSTEP: (I % 2).astype(np.int32),
            B.F_VELPRED: vel[:ngas] + 1e-3 * (v3(u, G, 8) - 0.5), B.F_ENTROPY: 0.05 * (1 + 0.2 * u(G, 9)),
            B.F_DTENTROPY: 1e-3 * (u(G, 10) - 0.5), B.F_GRAVACCEL: v3(name, I, 11),
            B.F_GRAVCOST: (I * 64 + 12).astype(np.int32), B.F_NUMNGB: name(G, 13), B.F_DENSITY: name(G, 14),
            B.F_DHSMLFAC: name(G, 15), B.F_DIVVEL: name(G, 16), B.F_CURLVEL: name(G, 17), B.F_PRESSURE: name(G, 18),
            B.F_HYDROACCEL: v3(name, G, 19), B.F_MAXSIGNALVEL: name(G, 20),
            B.F_TI_CURRENT: (I * 64 + 21).astype(np.int32), B.F_GRAVPM: v3(name, I, 22), B.F_ID: I.astype(np.int32)}
        return f

    def optional(self, ids, ngas):
        I, G = np.asarray(ids, np.int64), np.asarray(ids[:ngas], np.int64)

        def v3(J, code):
            return np.stack([name(J, code, c) for c in range(3)], axis=1).reshape(len(J), 3)
        return dict(heat=name(G, 30), alpha=name(G, 31), dtalpha=name(G, 32), inj=v3(G, 33), ra=v3(G, 34),
                    swallow=(I * 64 + 35).astype(np.uint32), injected=name(G, 36), drag=v3(G, 37), ddm=v3(G, 38),
                    newdens=name(I, 39))

    def problem(self, ids, ngas, periodic=0):
        """run-time parameters for walks over the records `ids` (tests/common.py:Problem), the cube fixed"""
        f = self.fields(ids, ngas)
        ic = dict(pos=f[B.F_POS], vel=f[B.F_VEL], mass=f[B.F_MASS], type=f[B.F_TYPE], ngas=ngas, boxsize=1.0,
                  spacing=1.0 / max(len(ids), 1) ** (1.0 / 3.0))
        pr = Problem(ic=ic, periodic=periodic)
        pr.extent = (CORNER.copy(), CORNER + 0.5 * DLEN, DLEN)
        return pr


def load(fp, case, ids=None, ngas=None, opts=()):
    ids = case.ids if ids is None else ids
    ngas = case.ngas if ngas is None else ngas
    fp.set_counts(len(ids), ngas)
    for field, a in case.fields(ids, ngas).items():
        if len(a):
            fp.set_field(field, a)
    o = case.optional(ids, ngas)
    if "heat" in opts:
        fp.set_dust_drag_heating(o["heat"])
    if "visc" in opts:
        fp.visc_set_alpha(o["alpha"], o["dtalpha"])
    if "inj" in opts:
        fp.set_wind_injected(o["inj"])
    if "ra" in opts:
        fp.set_wind_rad_accel(o["ra"])
    if "sink" in opts:
        fp.set_sink_marks(o["swallow"], o["injected"])
    if {"drag", "ddm", "newdens"} & set(opts):
        fp.kick_set_fields(o["drag"] if "drag" in opts else None, o["ddm"] if "ddm" in opts else None,
                           o["newdens"] if "newdens" in opts else None)
    return fp


def read(fp, opts=()):
    """everything the context holds, as {name: array}"""
    out = {("F", f): fp.get_field(f) for f in range(B.F_COUNT)}
    if "heat" in opts:
        out["heat"] = fp.dust_drag_heating()
    if "visc" in opts:
        out["alpha"], out["dtalpha"] = fp.visc_get()
    if "inj" in opts:
        out["inj"] = fp.wind_injected()
    if "ra" in opts:
        out["ra"] = fp.wind_rad_accel()
    if "sink" in opts:
        out["swallow"], out["injected"] = fp.sink_marks()
    out["drag"], out["ddm"], out["newdens"] = fp.kick_fields()
    return out


def expected(case, ids, ngas, opts=()):
    out = {("F", f): a for f, a in case.fields(ids, ngas).items()}
    o = case.optional(ids, ngas)
    for k, names in (("heat", ("heat",)), ("visc", ("alpha", "dtalpha")), ("inj", ("inj",)), ("ra", ("ra",)),
                     ("sink", ("swallow", "injected"))):
        if k in opts:
            for nm in names:
                out[nm] = o[nm]
    for k in ("drag", "ddm", "newdens"):
        out[k] = o[k] if k in opts else None
    return out


def assert_same_bits(got, want, what=""):
    assert set(got) == set(want), (sorted(map(str, got)), sorted(map(str, want)))
    for k, w in want.items():
        g = got[k]
        if w is None or g is None:
            assert g is None and w is None, "%s %s: held / not held" % (what, k)
            continue
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, "%s %s: %r %s, want %r %s" % (
            what, k, g.shape, g.dtype, w.shape, w.dtype)
        if g.tobytes() != w.tobytes():
            bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
            raise AssertionError("%s %s: %d records differ, first at slot %d: %r, want %r"
                                 % (what, k, len(bad), bad[0], g[bad[0]], w[bad[0]]))
