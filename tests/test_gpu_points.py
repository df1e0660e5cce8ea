"""Point validation on the device: gm_g1_check / gm_g2_check, their _bases_ forms, gm_g1_bases_from_bytes, gm_g1_powers_check and
CommitterKey.check.

Inputs are valid or invalid BY CONSTRUCTION, so the expected status of every index is known without a per-point ladder: valid points
are multiples of the generators, invalid ones come from a handful of distinct bad points, each verified once on the CPU with the
`[r] P` ladder of tests/points_ref.py (which tests/test_points_cpu.py holds against the endomorphism tests).  Every compare is exact:
the whole status array, first_bad and ok.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from gemini_amd import g2 as G2
from gemini_amd import capi, wire
from gemini_amd.capi import GeminiHipError
from gemini_amd.fr import R_MOD
from gemini_amd.kzg import CommitterKey, VerifierKey, g1_generator_mont, g2_records
from gemini_amd.points import PointStatus, check_g1, check_g2, check_powers, g1_bases_from_bytes
from oracle import oracle as orc
from tests import g2_ref
from tests import points_ref as pr
from tests.points_cases import g1_bytes, rejection_cases

pytestmark = pytest.mark.gpu

OK, BAD_ENCODING, NONCANONICAL, NOT_ON_CURVE, NOT_IN_SUBGROUP = (int(s) for s in PointStatus)
GM_EINVAL, GM_EHANDLE = -1, -3
NMAX = 1000


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


# ---- inputs, built once ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def g1_valid() -> np.ndarray:
    """(NMAX, 12): G, -G, then random multiples of G"""
    orc.build()
    out = orc.g1_fixed_base_mul(orc.g1_generator(), orc.random_fr(0x9017, NMAX))
    out[0] = pr.g1_record(pr.G1_GEN)
    out[1] = pr.g1_record(pr.g1_neg(pr.G1_GEN))
    return out


@functools.lru_cache(maxsize=None)
def g1_bad():
    """[(record, status)]: every bad point checked ONCE against the ladder"""
    G, t = pr.G1_GEN, pr.G1_ORDER3
    assert pr.g1_mul_raw(t, pr.R) == t  # order 3 and r = 1 mod 3
    outside = [t, pr.g1_neg(t), pr.g1_add(G, t), pr.g1_add(pr.g1_mul_raw(G, 0xC0FFEE), pr.g1_neg(t))] + list(pr.g1_random_curve_points(2))
    out = []
    for p in outside:
        assert pr.g1_on_curve(p) and not pr.g1_in_subgroup_ladder(p)
        out.append((pr.g1_record(p), NOT_IN_SUBGROUP))
    k5 = pr.g1_mul_raw(G, 5)
    off = (k5[0], (k5[1] + 1) % pr.Q)
    assert not pr.g1_on_curve(off)
    out.append((pr.g1_record(off), NOT_ON_CURVE))
    out.append((pr.noncanonical(pr.g1_record(k5), 0), NONCANONICAL))
    out.append((pr.noncanonical(pr.g1_record(k5), 1), NONCANONICAL))
    return out


@functools.lru_cache(maxsize=None)
def g2_valid() -> np.ndarray:
    pts = list(g2_ref.chain(130))
    pts[0], pts[1] = pr.G2_GEN, pr.g2_neg(pr.G2_GEN)
    return np.array([pr.g2_record(p) for p in pts], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def g2_bad():
    out = []
    for c in pr.g2_random_curve_points(2):
        for p in (c, pr.g2_add(g2_ref.chain(130)[7], c)):
            assert pr.g2_on_curve(p) and not pr.g2_in_subgroup_ladder(p)
            out.append((pr.g2_record(p), NOT_IN_SUBGROUP))
    H = pr.G2_GEN
    off = (H[0], ((H[1][0] + 1) % pr.Q, H[1][1]))
    assert not pr.g2_on_curve(off)
    out.append((pr.g2_record(off), NOT_ON_CURVE))
    out.append((pr.noncanonical(pr.g2_record(H), 0), NONCANONICAL))  # x.c0
    out.append((pr.noncanonical(pr.g2_record(H), 3), NONCANONICAL))  # y.c1
    return out


def plant(valid: np.ndarray, bad, n: int, flag: bool, boundaries):
    """n records (with the infinity word when `flag`) and the expected status array: bad points at 0, n - 1 and the lane boundaries,
    an all-zero identity, and with `flag` the infinity byte set over live coordinates -- a valid point's and a bad point's"""
    limbs = valid.shape[1]
    rec = np.zeros((n, limbs + 1 if flag else limbs), dtype=np.uint64)
    rec[:, :limbs] = valid[:n]
    want = np.zeros(n, dtype=np.uint8)
    spots = sorted({i for i in [0, n - 1] + list(boundaries) if 0 <= i < n})
    for k, i in enumerate(spots):
        r, st = bad[(k + n) % len(bad)]
        rec[i, :limbs] = np.array(r, dtype=np.uint64)
        want[i] = st
    free = [i for i in range(n) if i not in spots]
    if len(free) >= 3:
        rec[free[len(free) // 3], :limbs] = 0  # the identity as the all-zero record
        if flag:
            rec[free[len(free) // 2], limbs] = 1  # infinity over the coordinates of a valid point
            j = free[2 * len(free) // 3]
            rec[j, :limbs] = np.array(bad[-1][0], dtype=np.uint64)  # ... and over non-canonical ones: registration reads the identity
            rec[j, limbs] = 1
    return rec, want


def expect(res, want):
    bad = np.flatnonzero(want)
    assert (res.status == want).all(), (np.flatnonzero(res.status != want)[:8], res.status[res.status != want][:8], want[res.status != want][:8])
    assert res.first_bad == (int(bad[0]) if len(bad) else len(want))
    assert res.ok == (len(bad) == 0)


# ---- gm_g1_check / gm_g2_check ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", [False, True], ids=["stride96", "stride104"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_g1_check(gm, n, flag):
    rec, want = plant(g1_valid(), g1_bad(), n, flag, (63, 64, 255, 256))
    assert len(np.flatnonzero(want)) == len({0, n - 1} | {i for i in (63, 64, 255, 256) if i < n})
    expect(check_g1(rec), want)
    good = np.zeros_like(rec)
    good[:, :12] = g1_valid()[:n]
    res = check_g1(good)
    assert res.ok and res.first_bad == n and not res.status.any()


def test_g1_check_every_bad_class(gm):
    """each bad point on its own, in the middle of a wave, reports its own status"""
    bad = g1_bad()
    rec = g1_valid()[:3 * len(bad)].copy()
    want = np.zeros(len(rec), dtype=np.uint8)
    for k, (r, st) in enumerate(bad):
        rec[3 * k + 1] = np.array(r, dtype=np.uint64)
        want[3 * k + 1] = st
    expect(check_g1(rec), want)


@pytest.mark.parametrize("flag", [False, True], ids=["stride192", "stride200"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_g2_check(gm, n, flag):
    rec, want = plant(g2_valid(), g2_bad(), n, flag, (63, 64))
    expect(check_g2(rec), want)
    good = np.zeros_like(rec)
    good[:, :24] = g2_valid()[:n]
    res = check_g2(good)
    assert res.ok and res.first_bad == n and not res.status.any()


def test_g2_check_every_bad_class(gm):
    bad = g2_bad()
    rec = g2_valid()[:3 * len(bad)].copy()
    want = np.zeros(len(rec), dtype=np.uint8)
    for k, (r, st) in enumerate(bad):
        rec[3 * k + 1] = np.array(r, dtype=np.uint64)
        want[3 * k + 1] = st
    expect(check_g2(rec), want)


def test_check_misuse(gm):
    lib = capi.load()
    rec = g1_valid()[:4].copy()
    st = np.zeros(4, dtype=np.uint8)
    fb, ok = C.c_size_t(0), C.c_int(0)
    assert lib.gm_g1_check(capi.ptr(rec), C.c_size_t(88), C.c_size_t(4), capi.ptr(st), C.byref(fb), C.byref(ok)) == GM_EINVAL
    assert lib.gm_g1_check(capi.ptr(rec), C.c_size_t(100), C.c_size_t(3), capi.ptr(st), C.byref(fb), C.byref(ok)) == GM_EINVAL
    assert lib.gm_g2_check(capi.ptr(rec), C.c_size_t(96), C.c_size_t(2), capi.ptr(st), C.byref(fb), C.byref(ok)) == GM_EINVAL
    assert lib.gm_g1_check(None, C.c_size_t(96), C.c_size_t(4), capi.ptr(st), C.byref(fb), C.byref(ok)) == GM_EINVAL
    assert lib.gm_g1_check(capi.ptr(rec), C.c_size_t(96), C.c_size_t(4), capi.ptr(st), C.byref(fb), None) == GM_EINVAL
    # status and first_bad are optional; no points is a pass
    assert lib.gm_g1_check(capi.ptr(rec), C.c_size_t(96), C.c_size_t(4), None, None, C.byref(ok)) == 0 and ok.value == 1
    assert lib.gm_g1_check(None, C.c_size_t(96), C.c_size_t(0), None, C.byref(fb), C.byref(ok)) == 0 and ok.value == 1 and fb.value == 0


def test_every_entry_fails_closed(gm):
    """a negative return value comes with *ok = 0 whatever the caller had put there: one GM_EINVAL and (where the entry takes a handle)
    one GM_EHANDLE case per entry, *ok preset to 1 -- and *handle preset for the decoder"""
    lib = capi.load()
    rec, rec2 = g1_valid()[:4].copy(), g2_valid()[:4].copy()
    st = np.zeros(4, dtype=np.uint8)
    fb, ok, h = C.c_size_t(0), C.c_int(1), C.c_uint64(0xFEEDFACE)
    tail = (capi.ptr(st), C.byref(fb), C.byref(ok))

    def closed(rc, want):
        assert rc == want and ok.value == 0, (rc, want, ok.value)
        ok.value = 1

    closed(lib.gm_g1_check(capi.ptr(rec), C.c_size_t(88), C.c_size_t(4), *tail), GM_EINVAL)     # bad stride
    closed(lib.gm_g2_check(capi.ptr(rec2), C.c_size_t(196), C.c_size_t(4), *tail), GM_EINVAL)
    closed(lib.gm_g1_check(None, C.c_size_t(96), C.c_size_t(4), *tail), GM_EINVAL)              # null records
    g1 = gm.G1Bases.register(rec)
    g2 = gm.G2Bases.register(rec2)
    try:
        closed(lib.gm_g1_bases_check(C.c_uint64(g1.handle), C.c_size_t(3), C.c_size_t(2), *tail), GM_EINVAL)   # range
        closed(lib.gm_g1_bases_check(C.c_uint64(0xDEAD0011), C.c_size_t(0), C.c_size_t(1), *tail), GM_EHANDLE)
        closed(lib.gm_g2_bases_check(C.c_uint64(g2.handle), C.c_size_t(5), C.c_size_t(0), *tail), GM_EINVAL)
        closed(lib.gm_g2_bases_check(C.c_uint64(g1.handle), C.c_size_t(0), C.c_size_t(1), *tail), GM_EHANDLE)  # a G1 handle is no G2 handle
        g2p = g2_powers()
        rho, zero = np.ones(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        pw = lambda hh, off, n, r: lib.gm_g1_powers_check(C.c_uint64(hh), C.c_size_t(off), C.c_size_t(n), capi.ptr(g2p[0]), capi.ptr(g2p[1]), capi.ptr(r), C.byref(ok))  # noqa: E731
        closed(pw(g1.handle, 0, 4, zero), GM_EINVAL)            # rho = 0
        closed(pw(g1.handle, 2, 3, rho), GM_EINVAL)             # range
        closed(pw(0xDEAD0012, 0, 2, rho), GM_EHANDLE)
    finally:
        g1.free()
        g2.free()
    data = np.frombuffer(g1_bytes(pr.G1_GEN, True, 0), dtype=np.uint8)
    dec = lambda n, enc: lib.gm_g1_bases_from_bytes(capi.ptr(data), C.c_size_t(n), C.c_int(1), C.c_int(enc), C.c_int(1), C.byref(h), *tail)  # noqa: E731
    for n, enc in ((1, 2), ((1 << 64) // 96 + 1, 0)):           # unknown framing; a size that overflows
        h.value = 0xFEEDFACE
        closed(dec(n, enc), GM_EINVAL)
        assert h.value == 0


# ---- the _bases_check forms -------------------------------------------------------------------------------------------------------
def _resident_bad(bad):
    """registration keeps curve and subgroup failures as they are; a non-canonical record has no defined resident form"""
    return [b for b in bad if b[1] != NONCANONICAL]


def test_g1_bases_check(gm):
    n = 300
    rec, want = plant(g1_valid(), _resident_bad(g1_bad()), n, False, (63, 64, 255, 256))
    host = check_g1(rec)
    expect(host, want)
    reg = gm.G1Bases.register(rec)
    try:
        res = reg.check()
        expect(res, want)
        assert (res.status == host.status).all() and res.first_bad == host.first_bad
        win = reg.check(65, 190)  # [65, 255): between the planted points
        assert win.ok and win.first_bad == 190 and not win.status.any()
        win = reg.check(60, 10)
        expect(win, want[60:70])
        assert reg.check(300, 0).ok
        for off, cnt in ((0, 301), (301, 0), (299, 2)):
            with pytest.raises(GeminiHipError) as e:
                reg.check(off, cnt)
            assert e.value.code == GM_EINVAL
    finally:
        reg.free()
    with pytest.raises(GeminiHipError) as e:
        gm.G1Bases(0xDEAD0001, 4).check()
    assert e.value.code == GM_EHANDLE


def test_g2_bases_check(gm):
    n = 130
    rec, want = plant(g2_valid(), _resident_bad(g2_bad()), n, False, (63, 64))
    host = check_g2(rec)
    expect(host, want)
    reg = gm.G2Bases.register(rec)
    try:
        res = reg.check()
        expect(res, want)
        assert (res.status == host.status).all() and res.first_bad == host.first_bad
        win = reg.check(65, 64)
        assert win.ok and win.first_bad == 64 and not win.status.any()
        for off, cnt in ((0, 131), (131, 0), (129, 2)):
            with pytest.raises(GeminiHipError) as e:
                reg.check(off, cnt)
            assert e.value.code == GM_EINVAL
    finally:
        reg.free()
    with pytest.raises(GeminiHipError) as e:
        gm.G2Bases(0xDEAD0002, 4).check()
    assert e.value.code == GM_EHANDLE


# ---- gm_g1_bases_from_bytes -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decode_points():
    """257 affine points: multiples of G with both y signs, and the identity"""
    pts = [orc.affine_to_ints(r) for r in g1_valid()[:257]]
    pts[3] = None
    pts[5] = pr.g1_neg(pts[4])
    larger = [wire._y_is_larger(p[1]) for p in pts if p is not None]
    assert any(larger) and not all(larger)
    return pts


@pytest.mark.parametrize("enc", [wire.G1Encoding.ARKWORKS, wire.G1Encoding.ZCASH], ids=["arkworks", "zcash"])
@pytest.mark.parametrize("compress", [True, False], ids=["compressed", "uncompressed"])
@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_from_bytes(gm, n, compress, enc):
    pts = decode_points()[:n] if n > 1 else decode_points()[4:5]
    data = b"".join(g1_bytes(p, compress, enc) for p in pts)
    size = wire.g1_size(compress)
    # what wire.py reads from the same bytes, point for point (validate=False: the points are in G1 by construction, and the device
    # validates below); 18-limb images (x, y, Z = R) -> the 12-limb records a download gives, the identity all zero
    images = np.stack([wire.g1_deserialize(data, i * size, compress, enc, validate=False)[0] for i in range(n)])
    want = images[:, :12].copy()
    want[~images[:, 12:].any(axis=1)] = 0
    assert (want == np.array([pr.g1_record(p) for p in pts], dtype=np.uint64)).all()  # ... which is what the bytes were made from
    bases, res = g1_bases_from_bytes(data, n, compress, enc, validate=True)
    assert res.ok and res.first_bad == n and not res.status.any() and bases is not None and bases.handle != 0
    try:
        assert (bases.download() == want).all()
        if n == 257:  # the handle serves an MSM like a registered one
            sc = orc.random_fr(0x515, n)
            old = gm.G1Bases.register(want)
            try:
                assert (bases.msm_bigint(sc) == old.msm_bigint(sc)).all()
            finally:
                old.free()
    finally:
        bases.free()


@pytest.mark.parametrize("enc", [wire.G1Encoding.ARKWORKS, wire.G1Encoding.ZCASH], ids=["arkworks", "zcash"])
@pytest.mark.parametrize("compress", [True, False], ids=["compressed", "uncompressed"])
def test_from_bytes_rejections(gm, compress, enc):
    n, mid = 65, 32
    size = wire.g1_size(compress)
    good = [g1_bytes(p, compress, enc) for p in decode_points()[:n]]
    cases = rejection_cases(compress, enc)
    assert {c[2] for c in cases} == {PointStatus.BAD_ENCODING, PointStatus.NONCANONICAL, PointStatus.NOT_ON_CURVE, PointStatus.NOT_IN_SUBGROUP}
    lib = capi.load()
    for name, one, status in cases:
        with pytest.raises(wire.WireError):
            wire.g1_deserialize(one, 0, compress, enc, validate=True)
        data = b"".join(good[:mid] + [one] + good[mid + 1:])
        assert len(data) == n * size
        # the C entry itself: *handle comes back 0 whatever it held, and nothing stays registered (the bytes of resident keys
        # and the device memory in use are what they were)
        before = capi.mem_stats()
        buf = np.frombuffer(data, dtype=np.uint8)
        h, fb, ok = C.c_uint64(0xFEEDFACE), C.c_size_t(n + 1), C.c_int(1)
        rc = lib.gm_g1_bases_from_bytes(capi.ptr(buf), C.c_size_t(n), C.c_int(int(compress)), C.c_int(int(enc)), C.c_int(1), C.byref(h), None, C.byref(fb), C.byref(ok))
        assert rc == 0 and ok.value == 0 and fb.value == mid and h.value == 0, name
        after = capi.mem_stats()
        assert after["keys"] == before["keys"] and after["in_use"] == before["in_use"], (name, before, after)
        bases, res = g1_bases_from_bytes(data, n, compress, enc, validate=True)
        want = np.zeros(n, dtype=np.uint8)
        want[mid] = int(status)
        assert bases is None and not res.ok and res.first_bad == mid, name
        assert (res.status == want).all(), (name, res.status[mid])
        if status == PointStatus.NOT_IN_SUBGROUP:  # the same bytes pass without validation, as in wire.py
            wire.g1_deserialize(one, 0, compress, enc, validate=False)
            bases, res = g1_bases_from_bytes(data, n, compress, enc, validate=False)
            assert res.ok and res.first_bad == n and bases is not None
            try:
                assert (bases.download(mid, 1)[0] == np.array(pr.g1_record(pr.g1_random_curve_points(1)[0]), dtype=np.uint64)).all()
            finally:
                bases.free()


def test_from_bytes_misuse(gm):
    lib = capi.load()
    data = np.frombuffer(g1_bytes(pr.G1_GEN, True, 0), dtype=np.uint8)
    st = np.zeros(1, dtype=np.uint8)
    h, fb, ok = C.c_uint64(7), C.c_size_t(0), C.c_int(0)
    args = (capi.ptr(st), C.byref(fb), C.byref(ok))
    assert lib.gm_g1_bases_from_bytes(capi.ptr(data), C.c_size_t(1), C.c_int(1), C.c_int(2), C.c_int(1), C.byref(h), *args) == GM_EINVAL
    assert lib.gm_g1_bases_from_bytes(None, C.c_size_t(1), C.c_int(1), C.c_int(0), C.c_int(1), C.byref(h), *args) == GM_EINVAL
    assert lib.gm_g1_bases_from_bytes(capi.ptr(data), C.c_size_t(1), C.c_int(1), C.c_int(0), C.c_int(1), None, *args) == GM_EINVAL
    assert lib.gm_g1_bases_from_bytes(capi.ptr(data), C.c_size_t((1 << 64) // 96 + 1), C.c_int(1), C.c_int(0), C.c_int(1), C.byref(h), *args) == GM_EINVAL
    # a stride that wraps n * stride
    assert lib.gm_g1_check(capi.ptr(data), C.c_size_t(1 << 63), C.c_size_t(2), *args) == GM_EINVAL
    assert lib.gm_g2_check(capi.ptr(data), C.c_size_t(1 << 62), C.c_size_t(4), *args) == GM_EINVAL


# ---- gm_g1_powers_check -----------------------------------------------------------------------------------------------------------
TAU = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100ABCD % R_MOD


@functools.lru_cache(maxsize=None)
def g2_powers():
    """g2, tau g2, tau^2 g2 as 24-limb records, from gm_vk_from_trapdoor"""
    vk = VerifierKey.from_trapdoor(orc.ints_to_limbs([TAU], 4)[0], 2)
    try:
        raw = vk.powers_of_g2_bytes(enc=0)
    finally:
        vk.free()
    pts = [G2.deserialize_uncompressed(raw[8 + 192 * i: 8 + 192 * (i + 1)], 0) for i in range(3)]
    assert pts[0] == G2.generator()
    return g2_records(pts)


def srs(gm, n):
    return gm.G1Bases.srs(g1_generator_mont(), orc.ints_to_limbs([TAU], 4)[0], n)


@pytest.mark.parametrize("n", [2, 3, 64, 257, 4097])
def test_powers_check_accepts_an_srs(gm, n):
    g2p = g2_powers()
    key = srs(gm, n)
    try:
        assert key.check().ok
        assert check_powers(key, g2p[0], g2p[1], rho=0x1234567 + n)
        assert check_powers(key, g2p[0], g2p[1])  # rho drawn here
        assert not check_powers(key, g2p[0], g2p[2], rho=0x1234567 + n)  # the wrong tau g2
        assert check_powers(key, g2p[0], g2p[2], rho=5, offset=n - 1, n=1)  # one point is a power sequence of any tau
        with pytest.raises(GeminiHipError) as e:
            check_powers(key, g2p[0], g2p[1], rho=0)
        assert e.value.code == GM_EINVAL
        with pytest.raises(GeminiHipError) as e:
            check_powers(key, g2p[0], g2p[1], rho=3, offset=1, n=n)
        assert e.value.code == GM_EINVAL
    finally:
        key.free()


@pytest.mark.parametrize("where", [0, 128, 256])
def test_powers_check_rejects_a_doubled_element(gm, where):
    n = 257
    g2p = g2_powers()
    key = srs(gm, n)
    rec = key.download()
    key.free()
    rec[where] = orc.g1_to_affine(orc.g1_mul(rec[where], orc.ints_to_limbs([2], 4)[0]))
    reg = gm.G1Bases.register(rec)
    try:
        assert reg.check().ok  # still points of G1: only the powers check can tell
        assert not check_powers(reg, g2p[0], g2p[1], rho=0xABCDEF)
        for off, cnt in ((0, where), (where + 1, n - where - 1)):  # the windows on either side of it
            assert check_powers(reg, g2p[0], g2p[1], rho=0xABCDEF, offset=off, n=cnt)
        if 0 < where < n - 1:
            assert not check_powers(reg, g2p[0], g2p[1], rho=0xABCDEF, offset=where - 1, n=2)
    finally:
        reg.free()
    with pytest.raises(GeminiHipError) as e:
        check_powers(gm.G1Bases(0xDEAD0003, 4), g2p[0], g2p[1], rho=3)
    assert e.value.code == GM_EHANDLE


def test_powers_check_refuses_a_cyclic_share(gm):
    """a share of a sharded key holds powers of tau^world: not a bad key, and not one this check is built for"""
    g2p = g2_powers()
    h = C.c_uint64(0)
    capi.check(capi.load().gm_g1_srs_register_cyclic(capi.ptr(capi.u64(g1_generator_mont())), capi.ptr(orc.ints_to_limbs([TAU], 4)[0]), C.c_size_t(64), C.c_int(1),
                                                     C.c_int(2), C.byref(h)))
    share = gm.G1Bases(h.value, 32)
    try:
        assert share.check().ok  # the per-point checks do not care
        with pytest.raises(GeminiHipError) as e:
            check_powers(share, g2p[0], g2p[1], rho=7)
        assert e.value.code == GM_EINVAL and "cyclic share" in str(e.value)
        with pytest.raises(GeminiHipError):
            CommitterKey(share, 2, [G2.generator(), G2.mul(G2.generator(), TAU)]).check()
    finally:
        share.free()


# ---- CommitterKey.check -----------------------------------------------------------------------------------------------------------
def test_committer_key_check(gm):
    tau = orc.ints_to_limbs([TAU], 4)[0]
    ck = CommitterKey.new(63, 2, tau)
    vk = VerifierKey.from_committer_key(ck)
    try:
        assert ck.check() and ck.check(vk)
        rec = ck.powers_of_g.download()
    finally:
        vk.free()
        ck.powers_of_g.free()
    rec[40] = np.array(pr.g1_record(pr.g1_add(orc.affine_to_ints(rec[40]), pr.G1_ORDER3)), dtype=np.uint64)  # tau^40 g + a point of order 3
    bad = CommitterKey.from_powers(rec, 2, ck.powers_of_g2)
    try:
        res = bad.powers_of_g.check()
        assert not res.ok and res.first_bad == 40 and res.status[40] == NOT_IN_SUBGROUP
        assert not bad.check()
    finally:
        bad.powers_of_g.free()
