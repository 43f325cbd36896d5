"""The whole-record (AoS) path on its own, through the C-ABI: uploads, the three downloads, the split
upload and the gas-block word against a numpy restatement that reads and writes the record bytes
through the offsets table.  Every comparison is bit for bit.  (ghip_gravity_to_records needs a walk:
tests/test_gpu_boundary.py and the overlap_sph sequences of tests/test_gpu_parity.py.)"""
import ctypes as C
import importlib
import itertools

import numpy as np
import pytest

from common import bindings
from test_gpu_boundary import bundle_layouts

pytestmark = pytest.mark.gpu

B = bindings()
SENTINEL = 0xA5
# one record; one lane past a wavefront with a gas block that fills one; past a 256-thread
# workgroup with a gas block past two wavefronts
COUNTS = [(1, 0), (1, 1), (65, 64), (257, 130)]
EINVAL = -90002

# record member, resident field, format in the record, components, block (P: all n records of P[];
# PGAS: the records [0, ngas) of P[]; S: SphP[]), transfers.  Hsml / NumNgb come back in the block
# that holds Hsml (the PPP macro): `dens_rows`.
ROWS = [
    ("p_pos", B.F_POS, "f8", 3, "P", {"UP"}),
    ("p_vel", B.F_VEL, "f8", 3, "P", {"UP", "KICK"}),
    ("p_mass", B.F_MASS, "f8", 1, "P", {"UP"}),
    ("p_type", B.F_TYPE, "i2", 1, "P", {"UP"}),
    ("p_timebin", B.F_TIMEBIN, "i2", 1, "P", {"UP", "KICK"}),
    ("p_ti_begstep", B.F_TI_BEGSTEP, "i4", 1, "P", {"UP", "KICK"}),
    ("p_ti_current", B.F_TI_CURRENT, "i4", 1, "P", {"UP"}),
    ("p_oldacc", B.F_OLDACC, "f8", 1, "P", {"UP", "GRAV"}),
    ("p_gravaccel", B.F_GRAVACCEL, "f8", 3, "P", {"UP", "GRAV"}),
    ("p_gravpm", B.F_GRAVPM, "f8", 3, "P", {"UP", "GRAV"}),
    ("p_gravcost", B.F_GRAVCOST, "f4", 1, "P", {"GRAV"}),
    ("p_hsml", B.F_HSML, "f8", 1, "P", {"UP"}),
    ("p_hsml", B.F_HSML, "f8", 1, "PGAS", {"DENS"}),
    ("p_numngb", B.F_NUMNGB, "f8", 1, "PGAS", {"DENS"}),
    ("s_hsml", B.F_HSML, "f8", 1, "S", {"UP", "DENS"}),
    ("s_numngb", B.F_NUMNGB, "f8", 1, "S", {"DENS"}),
    ("s_velpred", B.F_VELPRED, "f8", 3, "S", {"UP", "KICK"}),
    ("s_entropy", B.F_ENTROPY, "f8", 1, "S", {"UP", "KICK"}),
    ("s_dtentropy", B.F_DTENTROPY, "f8", 1, "S", {"UP", "HYDRO", "KICK"}),
    ("s_density", B.F_DENSITY, "f8", 1, "S", {"UP", "DENS"}),
    ("s_dhsmlfac", B.F_DHSMLFAC, "f8", 1, "S", {"UP", "DENS"}),
    ("s_divvel", B.F_DIVVEL, "f8", 1, "S", {"UP", "DENS"}),
    ("s_curlvel", B.F_CURLVEL, "f8", 1, "S", {"UP", "DENS"}),
    ("s_pressure", B.F_PRESSURE, "f8", 1, "S", {"UP", "DENS"}),
    ("s_hydroaccel", B.F_HYDROACCEL, "f8", 3, "S", {"UP", "HYDRO"}),
    ("s_maxsignalvel", B.F_MAXSIGNALVEL, "f8", 1, "S", {"UP", "HYDRO"}),
]
RESULT_FIELDS = sorted({r[1] for r in ROWS if r[5] - {"UP"}})


def rows_of(lay, sets):
    """the rows a transfer of `sets` moves with this layout"""
    for row in ROWS:
        key, block, rsets = row[0], row[4], row[5]
        if getattr(lay, key) < 0 or not (rsets & sets):
            continue
        if key in ("p_hsml", "p_numngb", "s_hsml", "s_numngb") and not (rsets & sets - {"DENS"}):
            # (taken for DENS alone: only in the block that holds Hsml)
            if (block == "PGAS") != (lay.p_hsml >= 0):
                continue
        yield row


def minimal_layout():
    """the 112 / 184-byte records of the minimal flag set, Hsml in SphP"""
    H = importlib.import_module("gadget-leicester_amd.hostapi")
    lay = B.Layout()
    H.lib().gadget_force_layout(C.byref(lay))
    assert (lay.p_stride, lay.s_stride, lay.p_hsml) == (112, 184, -1) and lay.s_hsml >= 0
    return lay


def bundle_layout():
    """the shipped bundle's 536 / 264-byte records, Hsml in P"""
    lay, _ = bundle_layouts(B, importlib.import_module("gadget-leicester_amd.hostapi"))
    assert (lay.p_stride, lay.s_stride, lay.s_hsml) == (536, 264, -1) and lay.p_hsml >= 0
    return lay


def sparse_layout():
    """a layout of this test's own: GravPM present; TimeBin, GravCost, Ti_current, NumNgb, Pressure and
    CurlVel absent; Hsml in P"""
    lay = B.Layout()
    C.memset(C.byref(lay), 0xff, C.sizeof(lay))
    for k, v in dict(p_stride=152, p_pos=0, p_vel=24, p_mass=48, p_type=56, p_gravaccel=64, p_gravpm=88,
                     p_hsml=112, p_oldacc=120, p_ti_begstep=128,
                     s_stride=104, s_entropy=0, s_velpred=8, s_density=32, s_dtentropy=40, s_hydroaccel=48,
                     s_dhsmlfac=72, s_divvel=80, s_maxsignalvel=88).items():
        setattr(lay, k, v)
    assert lay.p_timebin == lay.p_gravcost == lay.p_ti_current == lay.p_numngb == lay.s_numngb == -1
    return lay


LAYOUTS = {"minimal": minimal_layout, "bundle": bundle_layout, "sparse": sparse_layout}


@pytest.fixture(scope="module")
def fp():
    path = B.ForcePath(0)
    yield path
    path.close()


@pytest.fixture(params=sorted(LAYOUTS))
def lay(request):
    return LAYOUTS[request.param]()


def member(img, off, fmt, ncomp):
    """the member at byte offset `off` of every record of an image, as a writable [n][ncomp] view"""
    dt = np.dtype(fmt)
    if img.shape[0] == 0:
        return np.empty((0, ncomp), dt)
    return np.ndarray((img.shape[0], ncomp), dt, buffer=img, offset=off, strides=(img.shape[1], dt.itemsize))


def draw(rng, shape, fmt, top=None):
    """finite doubles; small integers (int -> i16 and, below 2^24, int -> f32 are exact)"""
    dt = np.dtype(fmt)
    if dt.kind == "f" and dt.itemsize == 8:
        return rng.standard_normal(shape) * 1e3
    return rng.integers(0, top or 30, shape).astype(dt)


def fill_records(lay, n, ng, seed):
    """both blocks with every byte defined: the sentinel, then values in the members the layout names;
    the gas block is gas, the rest is not"""
    rng = np.random.default_rng(seed)
    P = np.full((n, lay.p_stride), SENTINEL, np.uint8)
    S = np.full((ng, lay.s_stride), SENTINEL, np.uint8)
    for key, _, fmt, ncomp, block, _ in ROWS:
        if getattr(lay, key) >= 0:
            m = member(S if block == "S" else P, getattr(lay, key), fmt, ncomp)
            m[...] = draw(rng, m.shape, fmt)
    if lay.p_type >= 0:
        t = member(P, lay.p_type, "i2", 1)
        t[:ng] = 0
        t[ng:] = rng.integers(1, 6, (n - ng, 1))
    return P, S


def vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def upload(fp, P, S, lay):
    fp.upload_aos(P, S if len(S) else None, lay)   # (no gas block: a null SphP is accepted)


def check_uploaded_fields(fp, P, S, lay):
    ng = len(S)
    for key, field, fmt, ncomp, block, _ in rows_of(lay, {"UP"}):
        want = member(S if block == "S" else P, getattr(lay, key), fmt, ncomp)
        got = fp.get_field(field).reshape(-1, ncomp)
        if block == "S":
            got = got[:ng]   # (Hsml is sized n, SphP[] holds its first ngas entries)
        assert got.dtype == (np.int32 if np.dtype(fmt).kind == "i" else np.float64)
        assert np.array_equal(got, want), key


def set_results(fp, seed):
    """new values in every field a download writes back; returns them by field"""
    rng = np.random.default_rng(seed)
    new = {}
    for field in RESULT_FIELDS:
        like = fp.get_field(field)
        top = {B.F_TIMEBIN: 30, B.F_GRAVCOST: 1 << 24}.get(field, 1 << 30)
        new[field] = draw(rng, like.shape, like.dtype, top)
        fp.set_field(field, new[field])
    return new


def expected(P, S, lay, sets, new):
    """the uploaded images with the members of `sets` replaced by the new values: nothing else moves"""
    P, S = P.copy(), S.copy()
    ng = len(S)
    for key, field, fmt, ncomp, block, _ in rows_of(lay, sets):
        cnt = len(P) if block == "P" else ng
        m = member(S if block == "S" else P, getattr(lay, key), fmt, ncomp)
        m[:cnt] = new[field].reshape(-1, ncomp)[:cnt]
    return P, S


def download(fp, entry, P, S, lay, *want):
    """one of the download entry points into P and S (S is passed also without a gas block: the
    library must leave it alone)"""
    rc = getattr(fp.L, entry)(fp.h, vp(P), vp(S), C.byref(lay), *[C.c_int(int(w)) for w in want])
    if rc == 0 and entry == "ghip_download_aos_async":
        fp.sync()
    return rc


def fresh_host_copies(P, S, lay):
    # (without a gas block SphP is one record of sentinels that must stay as it is)
    return P.copy(), (S.copy() if len(S) else np.full((1, lay.s_stride), SENTINEL, np.uint8))


def same_bytes(got, want):
    return got.shape[0] >= want.shape[0] and np.array_equal(got[:len(want)], want) and \
        np.all(got[len(want):] == SENTINEL)


def test_upload_unpacks_every_member_into_its_field(fp, lay):
    for seed, (n, ng) in enumerate(COUNTS):
        P, S = fill_records(lay, n, ng, 100 + seed)
        P0, S0 = P.copy(), S.copy()
        upload(fp, P, S, lay)
        check_uploaded_fields(fp, P, S, lay)
        assert np.array_equal(P, P0) and np.array_equal(S, S0)   # (the host's records are only read)


def test_split_upload_gives_the_same_fields(fp, lay):
    for seed, (n, ng) in enumerate(COUNTS):
        P, S = fill_records(lay, n, ng, 200 + seed)
        assert fp.L.ghip_upload_aos_particles(fp.h, vp(P), C.byref(lay), C.c_int(n), C.c_int(ng)) == 0
        assert fp.L.ghip_upload_aos_gas(fp.h, vp(S) if ng else None, C.byref(lay)) == 0
        fp.n, fp.ngas = n, ng
        check_uploaded_fields(fp, P, S, lay)


def test_split_upload_is_refused_when_the_softenings_live_in_sphp():
    lay = minimal_layout()
    P, S = fill_records(lay, 65, 64, 300)
    path = B.ForcePath(0)
    try:
        path.set_adaptive_gravsoft(True)
        rc = path.L.ghip_upload_aos_particles(path.h, vp(P), C.byref(lay), C.c_int(65), C.c_int(64))
        msg = path.L.ghip_last_error(path.h).decode()
        assert rc == EINVAL
        assert msg == ("ghip_upload_aos_particles: with adaptive gravitational softening the smoothing "
                       "lengths of SphP[] are needed first: use ghip_upload_aos")
        # (with Hsml in P[] the block is all the walks need)
        lay = bundle_layout()
        P, S = fill_records(lay, 65, 64, 301)
        assert path.L.ghip_upload_aos_particles(path.h, vp(P), C.byref(lay), C.c_int(65), C.c_int(64)) == 0
    finally:
        path.close()


@pytest.mark.parametrize("entry", ["ghip_download_aos", "ghip_download_aos_async"])
def test_download_writes_the_chosen_sets_and_no_other_byte(fp, lay, entry):
    combos = [c for c in itertools.product((0, 1), repeat=3) if any(c)]
    assert len(combos) == 7
    for seed, (n, ng) in enumerate(COUNTS):
        P, S = fill_records(lay, n, ng, 400 + seed)
        for g, d, h in combos:
            upload(fp, P, S, lay)   # (the device image is the uploaded one again)
            new = set_results(fp, 500 + seed)
            sets = {name for name, on in (("GRAV", g), ("DENS", d), ("HYDRO", h)) if on}
            if ng == 0:
                sets -= {"DENS", "HYDRO"}
            wantP, wantS = expected(P, S, lay, sets, new)
            gotP, gotS = fresh_host_copies(P, S, lay)
            assert download(fp, entry, gotP, gotS, lay, g, d, h) == 0
            assert np.array_equal(gotP, wantP), (n, ng, g, d, h)
            assert same_bytes(gotS, wantS), (n, ng, g, d, h)


def test_kick_download_writes_its_six_members_and_no_other_byte(fp, lay):
    kick = {r[0] for r in ROWS if "KICK" in r[5]}
    assert kick == {"p_vel", "p_timebin", "p_ti_begstep", "s_velpred", "s_entropy", "s_dtentropy"}
    for seed, (n, ng) in enumerate(COUNTS):
        P, S = fill_records(lay, n, ng, 600 + seed)
        upload(fp, P, S, lay)
        new = set_results(fp, 700 + seed)
        wantP, wantS = expected(P, S, lay, {"KICK"}, new)
        gotP, gotS = fresh_host_copies(P, S, lay)
        assert download(fp, "ghip_download_aos_kick", gotP, gotS, lay) == 0
        assert np.array_equal(gotP, wantP), (n, ng)
        assert same_bytes(gotS, wantS), (n, ng)
        assert not np.array_equal(gotP, P)   # (something was written)


def test_gas_block_word_tells_a_record_of_another_type(fp, lay):
    mixed = lambda: fp.L.ghip_gas_block_mixed(fp.h)
    for seed, (n, ng) in enumerate(COUNTS):
        P, S = fill_records(lay, n, ng, 800 + seed)
        upload(fp, P, S, lay)
        assert mixed() == 0   # (the records behind the gas block have other types: they do not count)
        if ng == 0:
            continue
        for at in {0, ng - 1}:
            Q = P.copy()
            member(Q, lay.p_type, "i2", 1)[at] = 3
            upload(fp, Q, S, lay)
            assert mixed() == 1, (n, ng, at)
        # the same records through a layout without Type
        blind = LAYOUTS["sparse"]()
        blind.p_type = -1
        Q = np.full((n, blind.p_stride), 1, np.uint8)
        upload(fp, Q, np.zeros((ng, blind.s_stride), np.uint8), blind)
        assert mixed() == 0
        upload(fp, P, S, lay)
        assert mixed() == 0


def test_download_without_a_device_image_fails_with_its_message(lay):
    path = B.ForcePath(0)
    try:
        path.set_counts(3, 2)
        P = np.zeros((3, lay.p_stride), np.uint8)
        S = np.zeros((2, lay.s_stride), np.uint8)
        for entry, want in (("ghip_download_aos", (1, 1, 1)), ("ghip_download_aos_async", (1, 1, 1)),
                            ("ghip_download_aos_kick", ())):
            assert download(path, entry, P, S, lay, *want) == EINVAL, entry
            msg = path.L.ghip_last_error(path.h).decode()
            assert msg.endswith(": no device image (call ghip_upload_aos)") and msg.startswith("ghip_download_aos"), msg
        assert not P.any() and not S.any()
    finally:
        path.close()
