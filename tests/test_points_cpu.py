"""CPU: the reference side of the point-validation tests is itself right, the new entry points exist and fail cleanly without a
device, and the decode status table covers every way wire.g1_deserialize rejects a point."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from gemini_amd import capi, wire
from gemini_amd.points import WIRE_ERROR_STATUS, PointStatus
from tests import points_ref as pr


def test_constants():
    assert pr.BETA != 1 and pow(pr.BETA, 3, pr.Q) == 1
    # sigma has the eigenvalue -x^2 on G1, a root of lambda^2 + lambda + 1 mod r
    lam = (-pr.X_ABS * pr.X_ABS) % pr.R
    assert (lam * lam + lam + 1) % pr.R == 0
    assert pr.g1_sigma(pr.G1_GEN) == pr.g1_mul_raw(pr.G1_GEN, lam)
    # psi is the untwist-Frobenius-twist map: it acts on G2 as multiplication by q = x (mod r)
    assert pr.Q % pr.R == (-pr.X_ABS) % pr.R
    assert pr.g2_psi(pr.G2_GEN) == pr.g2_mul_raw(pr.G2_GEN, pr.Q % pr.R)
    assert pr.C_X[0] == 0  # the device multiplies by c_x with two products because of this


def g1_adversarial():
    G = pr.G1_GEN
    k7 = pr.g1_mul_raw(G, 7)
    t = pr.G1_ORDER3
    return [t, pr.g1_neg(t), pr.g1_add(G, t), pr.g1_add(k7, pr.g1_neg(t))] + list(pr.g1_random_curve_points(3))


def test_g1_endomorphism_test_agrees_with_the_ladder():
    G = pr.G1_GEN
    assert pr.g1_mul_raw(pr.G1_ORDER3, pr.R) == pr.G1_ORDER3  # r = 1 mod 3: [r] fixes the points of order 3
    for p in [None, G, pr.g1_neg(G), pr.g1_mul_raw(G, 0xDEADBEEF12345), pr.g1_mul_raw(G, pr.R - 1)]:
        assert pr.g1_on_curve(p) and pr.g1_in_subgroup_ladder(p) and pr.g1_in_subgroup_endo(p)
    for p in g1_adversarial():
        assert pr.g1_on_curve(p)
        assert not pr.g1_in_subgroup_ladder(p) and not pr.g1_in_subgroup_endo(p)


def test_g2_endomorphism_test_agrees_with_the_ladder():
    H = pr.G2_GEN
    for p in [None, H, pr.g2_neg(H), pr.g2_mul_raw(H, 0xDEADBEEF12345)]:
        assert pr.g2_on_curve(p) and pr.g2_in_subgroup_ladder(p) and pr.g2_in_subgroup_endo(p)
    for c in pr.g2_random_curve_points(2):
        for p in (c, pr.g2_add(H, c)):
            assert pr.g2_on_curve(p)
            assert not pr.g2_in_subgroup_ladder(p) and not pr.g2_in_subgroup_endo(p)


def test_f2_sqrt():
    for x in [(3, 5), (0, 7), (11, 0), (pr.Q - 1, 2)]:
        sq = pr.f2_mul(x, x)
        r = pr.f2_sqrt(sq)
        assert r is not None and pr.f2_mul(r, r) == sq


def test_record_builders():
    rec = pr.g1_record(pr.G1_GEN)
    assert rec == [int(v) for v in wire.g1_from_affine_ints(pr.G1_GEN)[:12]]
    bad = pr.noncanonical(rec, 1)
    y = sum(w << (64 * i) for i, w in enumerate(bad[6:]))
    assert y >= pr.Q and y % pr.Q == pr.fq_mont(pr.G1_GEN[1]) and bad[:6] == rec[:6]


def test_new_entries_need_init():
    """every new entry answers GM_ENOTINIT before gm_init (this process never initialises a device) -- and fails closed: a caller's
    *ok = 1 (and *handle) is overwritten with 0 even on this earliest of error returns"""
    lib = capi.load()
    rec = np.zeros((1, 13), dtype=np.uint64)
    rec2 = np.zeros((1, 25), dtype=np.uint64)
    st = np.zeros(1, dtype=np.uint8)
    fb, ok, h = C.c_size_t(0), C.c_int(1), C.c_uint64(7)
    tail = (C.c_size_t(1), capi.ptr(st), C.byref(fb), C.byref(ok))

    def closed(rc):
        assert rc == -2 and ok.value == 0
        ok.value = 1

    closed(lib.gm_g1_check(capi.ptr(rec), C.c_size_t(104), *tail))
    closed(lib.gm_g2_check(capi.ptr(rec2), C.c_size_t(200), *tail))
    closed(lib.gm_g1_bases_check(C.c_uint64(1), C.c_size_t(0), *tail))
    closed(lib.gm_g2_bases_check(C.c_uint64(1), C.c_size_t(0), *tail))
    data = np.zeros(48, dtype=np.uint8)
    closed(lib.gm_g1_bases_from_bytes(capi.ptr(data), C.c_size_t(1), C.c_int(1), C.c_int(0), C.c_int(1), C.byref(h), capi.ptr(st), C.byref(fb), C.byref(ok)))
    assert h.value == 0
    g2 = np.zeros(24, dtype=np.uint64)
    rho = np.ones(4, dtype=np.uint64)
    closed(lib.gm_g1_powers_check(C.c_uint64(1), C.c_size_t(0), C.c_size_t(2), capi.ptr(g2), capi.ptr(g2), capi.ptr(rho), C.byref(ok)))
    assert b"gm_init" in lib.gm_last_error()


def test_status_table_covers_every_wire_error():
    """every WireError a G1 point can raise in wire.py (g1_deserialize and the _check_point it calls) has a row, and no row is stale"""
    src = inspect.getsource(wire.g1_deserialize) + inspect.getsource(wire._check_point)
    raised = set(re.findall(r'raise WireError\("([^"]+)"\)', src))
    raised.discard("not enough bytes for a G1 point")  # the length of the input, the caller's to check: not a property of a point
    assert raised and raised == set(WIRE_ERROR_STATUS)
    want = {"flags": PointStatus.BAD_ENCODING, "flag": PointStatus.BAD_ENCODING, "infinity with non-zero": PointStatus.BAD_ENCODING,
            "not a canonical field element": PointStatus.NONCANONICAL, "x coordinate is not on the curve": PointStatus.NOT_ON_CURVE,
            "is not on the curve": PointStatus.NOT_ON_CURVE, "not in the prime-order subgroup": PointStatus.NOT_IN_SUBGROUP}
    for msg, st in WIRE_ERROR_STATUS.items():
        hits = {v for k, v in want.items() if k in msg}
        assert hits == {st}, (msg, st, hits)


@pytest.mark.parametrize("compress", [True, False])
@pytest.mark.parametrize("enc", [wire.G1Encoding.ARKWORKS, wire.G1Encoding.ZCASH])
def test_wire_rejections_used_by_the_gpu_tests(compress, enc):
    """the planted encodings of tests/test_gpu_points.py are rejected by wire.py with the message the table maps"""
    from tests.points_cases import rejection_cases

    for name, data, status in rejection_cases(compress, enc):
        with pytest.raises(wire.WireError) as e:
            wire.g1_deserialize(data, 0, compress, enc, validate=True, strict=True)
        assert WIRE_ERROR_STATUS[str(e.value)] == status, (name, str(e.value))
