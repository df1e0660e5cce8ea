"""No GPU: the key-generation reference itself (tests/keygen_ref.py) -- the clearings land in the subgroups, the skip rules hold in
their order -- and the new entries of the C ABI in the export list and, uninitialised, failing closed."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import keygen_ref as kr
from tests import points_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["gm_g2_fixed_base_register", "gm_g2_srs_register", "gm_g1_bases_from_candidates", "gm_g2_bases_from_candidates", "gm_crs_truncate", "gm_crs_halve",
       "gm_crs_fold", "gm_crs_to_bases"]


def test_g1_clearing_lands_in_the_subgroup():
    for p in pr.g1_random_curve_points(3):
        assert pr.g1_on_curve(p) and not pr.g1_in_subgroup_ladder(p)
        c = kr.g1_clear(p)
        assert c is not None and pr.g1_on_curve(c) and pr.g1_in_subgroup_ladder(c) and pr.g1_in_subgroup_endo(c)
        assert c == pr.g1_add(pr.g1_mul_raw(p, pr.X_ABS), p)  # [|x|] P + P, as the device adds it up


def test_g2_clearing_lands_in_the_subgroup():
    for p in pr.g2_random_curve_points(2):
        assert pr.g2_on_curve(p) and not pr.g2_in_subgroup_ladder(p)
        c = kr.g2_clear(p)
        assert c is not None and pr.g2_on_curve(c) and pr.g2_in_subgroup_ladder(c) and pr.g2_in_subgroup_endo(c)
        # the two ladders of the device: U = [|x| + 1] P, then [|x|] U - P - psi(U) + psi^2([2] P)
        u = pr.g2_add(pr.g2_mul_raw(p, pr.X_ABS), p)
        dev = pr.g2_add(pr.g2_add(pr.g2_add(pr.g2_mul_raw(u, pr.X_ABS), pr.g2_neg(p)), pr.g2_neg(pr.g2_psi(u))), pr.g2_psi(pr.g2_psi(pr.g2_add(p, p))))
        assert dev == c


def test_a_member_is_multiplied_not_moved_out():
    """on the subgroup the G1 clearing is multiplication by 1 - x, a unit mod r"""
    g = pr.G1_GEN
    assert kr.g1_clear(g) == pr.g1_mul_raw(g, (1 + pr.X_ABS) % pr.R)
    assert pr.g2_in_subgroup_ladder(kr.g2_clear(pr.G2_GEN))


def test_order_three_point_is_skipped():
    assert pr.g1_on_curve(pr.G1_ORDER3) and pr.g1_mul_raw(pr.G1_ORDER3, 3) is None
    assert kr.g1_clear(pr.G1_ORDER3) is None
    for larger in (False, True):  # both points at x = 0
        assert kr.g1_curve_point(kr.g1_candidate_bytes(0, larger))[0] == kr.OK
        assert kr.g1_from_candidate(kr.g1_candidate_bytes(0, larger)) == (kr.IDENTITY, None)


def _g1_non_square_x():
    x = 1
    while pr.fq_sqrt((x**3 + 4) % pr.Q) is not None:
        x += 1
    return x


def test_skip_order_and_format_g1():
    q = pr.Q
    assert q < 1 << 381
    # rule 1 before rule 2: q + x is >= q whatever x^3 + 4 is -- not reduced first
    assert kr.g1_from_candidate(kr.g1_candidate_bytes(q + 2, False))[0] == kr.GE_Q
    assert kr.g1_from_candidate(kr.g1_candidate_bytes(q, True))[0] == kr.GE_Q  # x = q is not x = 0
    assert kr.g1_from_candidate(kr.g1_candidate_bytes((1 << 381) - 1, False))[0] == kr.GE_Q
    assert kr.g1_from_candidate(kr.g1_candidate_bytes(_g1_non_square_x(), True))[0] == kr.NO_SQUARE
    x = pr.g1_random_curve_points(1)[0][0]
    st0, p0 = kr.g1_curve_point(kr.g1_candidate_bytes(x, False))
    st1, p1 = kr.g1_curve_point(kr.g1_candidate_bytes(x, True))
    assert st0 == st1 == kr.OK and p0[0] == p1[0] == x and p0[1] + p1[1] == q and p1[1] > p0[1]  # the choice bit: the larger y
    for ignored in (1, 2, 3):  # bits 381 and 382 change nothing
        assert kr.g1_from_candidate(kr.g1_candidate_bytes(x, True, ignored)) == kr.g1_from_candidate(kr.g1_candidate_bytes(x, True))
    st, c = kr.g1_from_candidate(kr.g1_candidate_bytes(x, True))
    assert st == kr.OK and c == pr.g1_neg(kr.g1_from_candidate(kr.g1_candidate_bytes(x, False))[1])


def test_skip_order_and_format_g2():
    q = pr.Q
    x = pr.g2_random_curve_points(1)[0][0]
    assert kr.g2_from_candidate(kr.g2_candidate_bytes((q, x[1]), False))[0] == kr.GE_Q  # each half
    assert kr.g2_from_candidate(kr.g2_candidate_bytes((x[0], q + 1), False))[0] == kr.GE_Q
    bad = (1, 1)
    while pr.g2_point_from_x(bad) is not None:
        bad = (bad[0] + 1, 1)
    assert kr.g2_from_candidate(kr.g2_candidate_bytes(bad, True))[0] == kr.NO_SQUARE
    assert kr.g2_from_candidate(kr.g2_candidate_bytes((q, bad[1]), True))[0] == kr.GE_Q  # rule 1 first
    (st0, p0), (st1, p1) = kr.g2_curve_point(kr.g2_candidate_bytes(x, False)), kr.g2_curve_point(kr.g2_candidate_bytes(x, True))
    assert st0 == st1 == kr.OK and p0 == pr.g2_neg(p1) and pr.g2_on_curve(p0)
    assert (p1[1][1], p1[1][0]) > (p0[1][1], p0[1][0])  # ark-ff's order of Fq2: c1 first
    # the choice bit is bit 383 of the c1 half; that of the c0 half and bits 381 / 382 of both change nothing
    assert kr.g2_curve_point(kr.g2_candidate_bytes(x, False, (3, 1), c0_top=True)) == (st0, p0)
    st, c = kr.g2_from_candidate(kr.g2_candidate_bytes(x, True))
    assert st == kr.OK and pr.g2_in_subgroup_ladder(c)


def test_stream_semantics():
    """used, found, the shortfall and n = 0"""
    x = pr.g1_random_curve_points(3)
    ns = _g1_non_square_x()
    cands = b"".join(kr.g1_candidate_bytes(v, False) for v in (ns, x[0][0], 0, pr.Q, x[1][0], x[2][0]))
    pts, used, found = kr.from_candidates(1, cands, 2)
    assert (used, found) == (5, 2) and pts == [kr.g1_clear(x[0]), kr.g1_clear(x[1])]
    assert kr.from_candidates(1, cands, 3)[1:] == (6, 3)
    assert kr.from_candidates(1, cands, 4) == (None, 6, 3)
    assert kr.from_candidates(1, cands, 0) == ([], 0, 0)
    assert kr.accepted(1, cands) == [1, 2, 4, 5]  # square roots only: x = 0 passes rules 1 and 2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(os.path.join(ROOT, "gemini_amd", "libgemini_hip.so")):
        ge.build()
    from gemini_amd import capi

    return capi.load()


def test_exports_include_the_new_entries(lib):
    from gemini_amd import capi

    hdr = open(os.path.join(ROOT, "include", "gemini_hip.h")).read()
    for s in NEW:
        assert s in capi.SYMBOLS and hasattr(lib, s) and f"int {s}(" in hdr, s
    assert lib.gm_abi_version() == 1


def test_new_entries_fail_closed_without_init(lib):
    """no gm_init (no GPU here): GM_ENOTINIT, and every output handle is 0 already"""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible; this test is about the CPU-only box")
    from gemini_amd import capi

    rec, sc = np.zeros(24, dtype=np.uint64), np.ones(4, dtype=np.uint64)
    cand = np.zeros(96, dtype=np.uint8)
    z = C.c_size_t
    for call in (lambda h: lib.gm_g2_fixed_base_register(capi.ptr(rec), capi.ptr(sc), z(1), C.byref(h)),
                 lambda h: lib.gm_g2_srs_register(capi.ptr(rec), capi.ptr(sc), z(1), C.byref(h))):
        assert call(C.c_uint64(7)) == -2
    for fn in (lib.gm_g1_bases_from_candidates, lib.gm_g2_bases_from_candidates):
        h, used, found = C.c_uint64(7), z(), z()
        assert fn(capi.ptr(cand), z(1), z(1), C.byref(h), C.byref(used), C.byref(found)) == -2 and h.value == 0
    for call in (lambda h: lib.gm_crs_truncate(C.c_uint64(1), z(1), C.byref(h)), lambda h: lib.gm_crs_halve(C.c_uint64(1), C.byref(h)),
                 lambda h: lib.gm_crs_fold(C.c_uint64(1), capi.ptr(sc), C.byref(h))):
        h = C.c_uint64(7)
        assert call(h) == -2 and h.value == 0
    h1, h2 = C.c_uint64(7), C.c_uint64(7)
    assert lib.gm_crs_to_bases(C.c_uint64(1), C.byref(h1), C.byref(h2)) == -2 and h1.value == 0 and h2.value == 0
