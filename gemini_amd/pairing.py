"""Host mirror of the pairing surface herring uses: `P::multi_pairing` behind PModule::ip (src/herring/module.rs:60-79) and the
multi-pairings of Vrs::from (src/herring/ipa.rs:215-247).  All arithmetic happens in libgemini_hip.so (gm_pairing_*, gm_gt_*).

Data conventions (numpy uint64): G1 records (n, 12) / (n, 13) as in gemini_amd.msm, G2 records (n, 24) / (n, 25) as in
gemini_amd.g2msm; a GT element is (72,) limbs = 12 Fq values in Montgomery form, tower order c0.c0.c0, c0.c0.c1, c0.c1.c0, ...,
c1.c2.c1 of Fq12 = Fq6[w] / (w^2 - v), Fq6 = Fq2[v] / (v^3 - (1 + u)), Fq2 = Fq[u] / (u^2 + 1).  GT is written multiplicatively:
what herring calls "+" on GT is `gt_mul`.  The value is the reduced ate pairing as ark-ec states it for BLS12 with the exponent
(q^12 - 1) / r.  InnerProductProof with Crs and Vrs is gemini_amd/ipa.py; InnerProductProof::generic and CrsStream are out of scope.
"""
from __future__ import annotations

import ctypes as C
import enum

import numpy as np

from . import capi
from .g2msm import G2Bases, _fq_int, _fq_limbs, _records as _g2_records
from .points import CheckResult


def gt_from_ints(coeffs) -> np.ndarray:
    """12 canonical integers in tower order -> (72,) limbs"""
    assert len(coeffs) == 12
    return np.array([w for c in coeffs for w in _fq_limbs(int(c))], dtype=np.uint64)


def gt_to_ints(gt) -> list:
    """(72,) limbs -> 12 canonical integers in tower order"""
    g = capi.u64(gt).reshape(12, 6)
    return [_fq_int(row) for row in g]


def gt_one() -> np.ndarray:
    out = np.empty(72, dtype=np.uint64)
    capi.check(capi.load().gm_gt_one(capi.ptr(out)))
    return out


def gt_mul(a, b) -> np.ndarray:
    """a b on the host (no GPU needed)"""
    out = np.empty(72, dtype=np.uint64)
    capi.check(capi.load().gm_gt_mul(capi.ptr(capi.u64(a).reshape(72)), capi.ptr(capi.u64(b).reshape(72)), capi.ptr(out)))
    return out


def gt_pow(a, scalar: int) -> np.ndarray:
    """a^scalar for 0 <= scalar < 2^256 on the host (no GPU needed)"""
    assert 0 <= scalar < (1 << 256)
    s = np.array([(scalar >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)
    out = np.empty(72, dtype=np.uint64)
    capi.check(capi.load().gm_gt_pow(capi.ptr(capi.u64(a).reshape(72)), capi.ptr(s), capi.ptr(out)))
    return out


def gt_multi_pow(x, scalars) -> np.ndarray:
    """prod_i x_i^scalars_i on the device (gm_gt_multi_pow): x is (n, 72) limbs, scalars n integers 0 <= s < 2^256 taken as they
    are (not reduced mod r) or an (n, 4) uint64 array of canonical limbs; the shorter input ends the product, n = 0 gives 1.
    No final exponentiation, no membership check: bit for bit the composition of gt_pow / gt_mul on any reduced coefficients."""
    capi.ensure_init()
    xs = capi.u64(x).reshape(-1, 72)
    if isinstance(scalars, np.ndarray) and scalars.dtype == np.uint64:
        sc = capi.u64(scalars).reshape(-1, 4)
    else:
        ints = [int(s) for s in scalars]
        assert all(0 <= s < (1 << 256) for s in ints)
        sc = np.array([[(s >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for s in ints], dtype=np.uint64).reshape(-1, 4)
    n = min(len(xs), len(sc))
    out = np.empty(72, dtype=np.uint64)
    capi.check(capi.load().gm_gt_multi_pow(capi.ptr(xs), C.c_size_t(n), capi.ptr(sc), capi.ptr(out)))
    return out


def gt_multi_pow_many(x, scalars, offsets) -> np.ndarray:
    """S = len(offsets) - 1 independent products in one launch (gm_gt_multi_pow_many): out[s] = prod of x_i^scalars_i over
    offsets[s] <= i < offsets[s + 1], an empty product is 1; -> (S, 72).  x and scalars as gt_multi_pow takes them.  Each row is bit
    for bit gt_multi_pow on its range."""
    capi.ensure_init()
    xs = capi.u64(x).reshape(-1, 72)
    if isinstance(scalars, np.ndarray) and scalars.dtype == np.uint64:
        sc = capi.u64(scalars).reshape(-1, 4)
    else:
        ints = [int(s) for s in scalars]
        assert all(0 <= s < (1 << 256) for s in ints)
        sc = np.array([[(s >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for s in ints], dtype=np.uint64).reshape(-1, 4)
    off = np.ascontiguousarray(offsets, dtype=np.uintp)
    S = len(off) - 1
    assert S >= 0 and (S == 0 or int(off.max()) <= min(len(xs), len(sc))), "the offsets run past the terms"
    out = np.empty((max(S, 0), 72), dtype=np.uint64)
    capi.check(capi.load().gm_gt_multi_pow_many(capi.ptr(xs) if len(xs) else None, capi.ptr(sc) if len(sc) else None, capi.ptr(off), C.c_size_t(S), capi.ptr(out) if S else None))
    return out


def gt_final_exp(f) -> np.ndarray:
    """f^((q^12 - 1) / r) for any Fq12 element, no conjugation: a test and integration aid (gm_gt_final_exp)"""
    out = np.empty(72, dtype=np.uint64)
    capi.check(capi.load().gm_gt_final_exp(capi.ptr(capi.u64(f).reshape(72)), capi.ptr(out)))
    return out


def gt_final_exp_many(f) -> np.ndarray:
    """out[i] = f[i]^((q^12 - 1) / r) on the device (gm_gt_final_exp_many): (n, 72) limbs in and out, no conjugation; bit for bit
    `gt_final_exp` element by element on any reduced coefficients"""
    capi.ensure_init()
    fs = capi.u64(f).reshape(-1, 72)
    out = np.empty_like(fs)
    capi.check(capi.load().gm_gt_final_exp_many(capi.ptr(fs), C.c_size_t(len(fs)), capi.ptr(out)))
    return out


class GtStatus(enum.IntEnum):
    """the GM_PT_* values gm_gt_check reports: the FIRST test of an element that fails, in this order"""
    OK = 0
    NONCANONICAL = 2       # a coefficient >= q
    NOT_CYCLOTOMIC = 5     # f = 0 or f^(q^4) f != f^(q^2)
    NOT_IN_SUBGROUP = 4    # f^q != f^x


def gt_check(x) -> CheckResult:
    """gm_gt_check: is every element of x ((n, 72) limbs) a member of GT, the order-r subgroup of Fq12*?  A points.CheckResult whose
    status holds GtStatus values; a bad element is a result, not an exception."""
    capi.ensure_init()
    xs = capi.u64(x).reshape(-1, 72)
    status = np.zeros(len(xs), dtype=np.uint8)
    first_bad, ok = C.c_size_t(0), C.c_int(0)
    capi.check(capi.load().gm_gt_check(capi.ptr(xs), C.c_size_t(len(xs)), capi.ptr(status), C.byref(first_bad), C.byref(ok)))
    return CheckResult(bool(ok.value), first_bad.value, status)


def debug_gt_op(op: int, x) -> np.ndarray:
    """gm_debug_gt_op, a test aid: ONE device function per element of x ((n, 72) limbs).  op 0: x^q, 1: x^(q^2), 2: 1 / x,
    3: the cyclotomic squaring, 4: x^|x_BLS| by cyclotomic squarings (3 and 4 are valid on the cyclotomic subgroup only)"""
    capi.ensure_init()
    xs = capi.u64(x).reshape(-1, 72)
    out = np.empty_like(xs)
    capi.check(capi.load().gm_debug_gt_op(C.c_int(op), capi.ptr(xs), C.c_size_t(len(xs)), capi.ptr(out)))
    return out


(GT_OP2_MUL, GT_OP2_SQR, GT_OP2_CONJ, GT_OP2_MUL_014, GT_OP2_FQ6_MUL, GT_OP2_FQ6_MUL_V, GT_OP2_FQ6_MUL_01, GT_OP2_FQ6_MUL_1, GT_OP2_FQ2_MUL_XI,
 GT_OP2_FQ2_MUL12, GT_OP2_FQ2_MUL_FQ, GT_OP2_FQ2_CONJ) = range(12)
MILLER_OP_DBL, MILLER_OP_ADD = range(2)


def debug_gt_op2(op: int, a, b=None) -> np.ndarray:
    """gm_debug_gt_op2, a test aid: ONE tower function of gt.cuh per element of a ((n, 72) limbs); b ((n, 72)) is the second operand
    of the GT_OP2_* that take one (include/gemini_hip.h: a line in its first three Fq2 slots, an Fq scalar in the c0 of a slot)"""
    capi.ensure_init()
    xs = capi.u64(a).reshape(-1, 72)
    pb = None
    if b is not None:
        ys = capi.u64(b).reshape(-1, 72)
        assert len(ys) == len(xs)
        pb = capi.ptr(ys)
    out = np.empty_like(xs)
    capi.check(capi.load().gm_debug_gt_op2(C.c_int(op), capi.ptr(xs), pb, C.c_size_t(len(xs)), capi.ptr(out)))
    return out


def debug_miller_step(op: int, T, Q, P):
    """gm_debug_miller_step, a test aid: ONE miller_dbl_step (op 0) or miller_add_step (op 1) per row.  T is (n, 36) limbs (X | Y | Z
    over Fq2, any Z), Q (n, 24) (x | y over Fq2), P (n, 12) (two field elements, not checked against the curve) -> the new T (n, 36)
    and the line (l0 | l1 | l4) (n, 36)"""
    capi.ensure_init()
    t, q, p = capi.u64(T).reshape(-1, 36), capi.u64(Q).reshape(-1, 24), capi.u64(P).reshape(-1, 12)
    assert len(t) == len(q) == len(p)
    rec = np.ascontiguousarray(np.concatenate([t, q, p], axis=1))
    out = np.empty_like(rec)
    capi.check(capi.load().gm_debug_miller_step(C.c_int(op), capi.ptr(rec), C.c_size_t(len(rec)), capi.ptr(out)))
    return out[:, :36].copy(), out[:, 36:].copy()


def debug_miller_each(g1, g2) -> np.ndarray:
    """gm_debug_miller_each, a test aid: out[i] = the Miller value of pair i as the loop leaves it ((n, 72) limbs): no conjugation, no
    product, no final exponentiation.  Records as for `pairing_each`; the shorter input ends the vector."""
    capi.ensure_init()
    r1, r2 = _g1_records(g1), _g2_records(g2)
    m = min(len(r1), len(r2))
    out = np.empty((m, 72), dtype=np.uint64)
    capi.check(capi.load().gm_debug_miller_each(capi.ptr(r1), C.c_size_t(r1.shape[1] * 8), capi.ptr(r2), C.c_size_t(r2.shape[1] * 8), C.c_size_t(m), capi.ptr(out)))
    return out


def _g1_records(bases) -> np.ndarray:
    bases = capi.u64(bases)
    assert bases.ndim == 2 and bases.shape[1] in (12, 13)
    return bases


def multi_pairing(g1_records, g2_records) -> np.ndarray:
    """prod_i e(P_i, Q_i) over the shorter input (zip); records with an infinity flag or all-zero coordinates contribute 1"""
    capi.ensure_init()
    g1 = _g1_records(g1_records)
    g2 = _g2_records(g2_records)
    n = min(len(g1), len(g2))
    out = np.empty(72, dtype=np.uint64)
    capi.check(capi.load().gm_pairing_multi(capi.ptr(g1), C.c_size_t(g1.shape[1] * 8), capi.ptr(g2), C.c_size_t(g2.shape[1] * 8), C.c_size_t(n),
                                            capi.ptr(out)))
    return out


def multi_pairing_many(g1_records, g2_records, offsets) -> np.ndarray:
    """gm_pairing_multi_many: S = len(offsets) - 1 independent products, out[s] = prod e(P_t, Q_t) over offsets[s] <= t < offsets[s + 1],
    (S, 72) limbs; each equals `multi_pairing` on that slice bit for bit, an empty product is 1.  One segmented Miller launch and one
    launch of final exponentiations whatever S is."""
    capi.ensure_init()
    g1 = _g1_records(g1_records)
    g2 = _g2_records(g2_records)
    off = np.ascontiguousarray(offsets, dtype=np.uintp)
    S = len(off) - 1
    assert S >= 0 and (S == 0 or int(off[-1]) <= min(len(g1), len(g2)))
    out = np.empty((max(S, 0), 72), dtype=np.uint64)
    capi.check(capi.load().gm_pairing_multi_many(capi.ptr(g1), C.c_size_t(g1.shape[1] * 8), capi.ptr(g2), C.c_size_t(g2.shape[1] * 8), capi.ptr(off),
                                                 C.c_size_t(S), capi.ptr(out)))
    return out


def multi_pairing_many_h(g1_bases, g2_bases: G2Bases, offsets, off1: int = 0, off2: int = 0) -> np.ndarray:
    """the same over registered bases: product s pairs g1[off1 + t] with g2[off2 + t], offsets[s] <= t < offsets[s + 1]"""
    off = np.ascontiguousarray(offsets, dtype=np.uintp)
    S = len(off) - 1
    out = np.empty((max(S, 0), 72), dtype=np.uint64)
    capi.check(capi.load().gm_pairing_multi_many_h(C.c_uint64(g1_bases.handle), C.c_size_t(off1), C.c_uint64(g2_bases.handle), C.c_size_t(off2), capi.ptr(off),
                                                   C.c_size_t(S), capi.ptr(out)))
    return out


def multi_pairing_h(g1_bases, g2_bases: G2Bases, n: int, off1: int = 0, step1: int = 1, off2: int = 0, step2: int = 1) -> np.ndarray:
    """prod_i e(g1[off1 + step1 i], g2[off2 + step2 i]), i < n, over registered bases (gemini_amd.msm.G1Bases, g2msm.G2Bases)"""
    out = np.empty(72, dtype=np.uint64)
    capi.check(capi.load().gm_pairing_multi_h(C.c_uint64(g1_bases.handle), C.c_size_t(off1), C.c_size_t(step1), C.c_uint64(g2_bases.handle),
                                              C.c_size_t(off2), C.c_size_t(step2), C.c_size_t(n), capi.ptr(out)))
    return out


def pairing_each(g1, g2, n: int | None = None, off1: int = 0, step1: int = 1, off2: int = 0, step2: int = 1) -> np.ndarray:
    """out[i] = e(P_i, Q_i), (n, 72) limbs: one launch of Miller loops and one of final exponentiations (gm_pairing_each).  g1 / g2
    are host records (zip: the shorter input ends the vector) or BOTH registered handles (G1Bases, G2Bases), then
    out[i] = e(g1[off1 + step1 i], g2[off2 + step2 i]) for i < n (gm_pairing_each_h)."""
    capi.ensure_init()
    if isinstance(g2, G2Bases):
        assert hasattr(g1, "handle") and n is not None, "handles on both sides, and n"
        out = np.empty((n, 72), dtype=np.uint64)
        capi.check(capi.load().gm_pairing_each_h(C.c_uint64(g1.handle), C.c_size_t(off1), C.c_size_t(step1), C.c_uint64(g2.handle), C.c_size_t(off2),
                                                 C.c_size_t(step2), C.c_size_t(n), capi.ptr(out)))
        return out
    r1, r2 = _g1_records(g1), _g2_records(g2)
    m = min(len(r1), len(r2)) if n is None else n
    assert m <= min(len(r1), len(r2))
    out = np.empty((m, 72), dtype=np.uint64)
    capi.check(capi.load().gm_pairing_each(capi.ptr(r1), C.c_size_t(r1.shape[1] * 8), capi.ptr(r2), C.c_size_t(r2.shape[1] * 8), C.c_size_t(m), capi.ptr(out)))
    return out
