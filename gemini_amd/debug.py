"""The element-wise test aids of the C ABI (include/gemini_hip.h, "A test aid"): ONE device function of field.cuh / field30.cuh /
g1.cuh / g2.cuh per lane, on records in device form, read and written as they are.

Records are uint32 arrays: an Fq element is 12 words holding a * 2^390 mod q, a loose Fq30 element 13 limbs of 30 bits (the top one
up to 26), an Fq2 element 24 words (c0 | c1), a G1 XYZZ point 48 words, a G2 one 96, an Acc30 accumulator 52 limbs.  The helpers at
the bottom convert Python integers to and from these layouts and do nothing else (no reduction, no Montgomery factor): the caller
decides the limbs."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

Q = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R390 = 1 << 390

FQ_MUL, FQ_SQR, FQ_ADD, FQ_SUB, FQ_DBL, FQ_NEG, FQ_IMPORT, FQ_EXPORT, FQ_INV, FQ_RAW_GE_Q, FQ_PACK_UNPACK = range(11)
FQ30_MUL_ASM, FQ30_SQR_ASM, FQ30_MUL_C, FQ30_LOOSE_TO_CANONICAL, FQ30_CANONICAL_TAIL = range(5)
FQ2_MUL, FQ2_SQR, FQ2_ADD, FQ2_SUB, FQ2_NEG, FQ2_INV = range(6)
G1_MADD, G1_ADD, G1_DBL, G1_DBL_AFFINE, G1_STORE_LOAD30 = range(5)
G2_MADD, G2_ADD, G2_DBL, G2_DBL_AFFINE, G2_TO_AFFINE = range(5)
ACC30_MADD, ACC30_ADD = range(2)


def _u32(a, width: int) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint32)
    assert a.ndim == 2 and a.shape[1] == width, (a.shape, width)
    return a


def _binary(entry: str, op: int, a, b, aw: int, bw: int, ow: int) -> np.ndarray:
    a = _u32(a, aw)
    out = np.zeros((len(a), ow), dtype=np.uint32)
    pb = None
    if b is not None:
        b = _u32(b, bw)
        assert len(b) == len(a)
        pb = capi.ptr(b)
    capi.check(getattr(capi.load(), entry)(C.c_int(op), capi.ptr(a), pb, C.c_size_t(len(a)), capi.ptr(out)))
    return out


def fq_op(op: int, a, b=None) -> np.ndarray:
    """gm_debug_fq_op: (n, 12) words -> (n, 12)"""
    return _binary("gm_debug_fq_op", op, a, b, 12, 12, 12)


def fq30_op(op: int, a, b=None) -> np.ndarray:
    """gm_debug_fq30_op: (n, 13) loose limbs -> (n, 13)"""
    return _binary("gm_debug_fq30_op", op, a, b, 13, 13, 13)


def fq2_op(op: int, a, b=None) -> np.ndarray:
    """gm_debug_fq2_op: (n, 24) words -> (n, 24)"""
    return _binary("gm_debug_fq2_op", op, a, b, 24, 24, 24)


def g1_op(op: int, p, q=None) -> np.ndarray:
    """gm_debug_g1_op: p (n, 48); q (n, 24) for G1_MADD, (n, 48) for G1_ADD -> (n, 48)"""
    return _binary("gm_debug_g1_op", op, p, q, 48, 24 if op == G1_MADD else 48, 48)


def g2_op(op: int, p, q=None) -> np.ndarray:
    """gm_debug_g2_op: p (n, 96); q (n, 48) for G2_MADD, (n, 96) for G2_ADD -> (n, 96)"""
    return _binary("gm_debug_g2_op", op, p, q, 96, 48 if op == G2_MADD else 96, 96)


def acc30_op(op: int, acc, other, neg=None):
    """gm_debug_acc30_op: acc (n, 52) loose limbs; other (n, 24) words + neg (n,) for ACC30_MADD, (n, 52) limbs for ACC30_ADD ->
    (the 52 limbs the statement leaves, acc30_to_canonical of them (n, 48))"""
    acc = _u32(acc, 52)
    other = _u32(other, 24 if op == ACC30_MADD else 52)
    n = len(acc)
    assert len(other) == n
    pn = None
    if neg is not None:
        neg = np.ascontiguousarray(neg, dtype=np.uint32)
        assert neg.shape == (n,)
        pn = capi.ptr(neg)
    out = np.zeros((n, 52), dtype=np.uint32)
    canon = np.zeros((n, 48), dtype=np.uint32)
    capi.check(capi.load().gm_debug_acc30_op(C.c_int(op), capi.ptr(acc), capi.ptr(other), pn, C.c_size_t(n), capi.ptr(out), capi.ptr(canon)))
    return out, canon


# ---- integers <-> records -------------------------------------------------------------------------------------------------------
def words(v: int, n: int = 12) -> list:
    """the integer v as n little-endian 32-bit words"""
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def limbs30(v: int) -> list:
    """the integer v < 2^386 as 13 normalised 30-bit limbs"""
    assert 0 <= v < 1 << 386
    return [(v >> (30 * i)) & 0x3FFFFFFF for i in range(12)] + [v >> 360]


def from_words(row) -> int:
    return sum(int(w) << (32 * i) for i, w in enumerate(row))


def from_limbs30(row) -> int:
    return sum(int(w) << (30 * i) for i, w in enumerate(row))


def rows_words(vals, per: int = 1) -> np.ndarray:
    """a list of integers (per = 1) or of per-tuples of integers -> (n, 12 per) words"""
    if per == 1:
        vals = [(v,) for v in vals]
    return np.array([[w for v in t for w in words(v)] for t in vals], dtype=np.uint32).reshape(len(vals), 12 * per)


def rows_limbs30(vals, per: int = 1) -> np.ndarray:
    if per == 1:
        vals = [(v,) for v in vals]
    return np.array([[w for v in t for w in limbs30(v)] for t in vals], dtype=np.uint32).reshape(len(vals), 13 * per)


def ints_of_words(a: np.ndarray) -> list:
    """(n, 12 k) words -> n tuples of k integers"""
    k = a.shape[1] // 12
    return [tuple(from_words(r[12 * j:12 * j + 12]) for j in range(k)) for r in a]


def ints_of_limbs30(a: np.ndarray) -> list:
    k = a.shape[1] // 13
    return [tuple(from_limbs30(r[13 * j:13 * j + 13]) for j in range(k)) for r in a]
