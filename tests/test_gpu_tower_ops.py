"""GPU: the Miller-loop half of gt.cuh and pairing.hip one device function per lane -- fq12_mul, fq12_sqr, fq12_conj, fq12_mul_014, fq6_mul,
fq6_mul_v, fq6_mul_01, fq6_mul_1, fq2_mul_xi, fq2_mul12, fq2_mul_fq, fq2_conj (gm_debug_gt_op2), miller_dbl_step, miller_add_step
(gm_debug_miller_step) and miller_lane (gm_debug_miller_each).

Operands and expected values are the Python integers of tests/tower_cases.py, which tests/test_tower_cases_cpu.py validates without a
GPU; every compare is bit for bit on the 72 limbs of a record.  The steps and the raw Miller values are ALSO held against independent
statements: the new T against the affine chord and tangent of tests/g2_ref.py, the line against oracle.pairing._line up to c w^3 with
c in Fq2*, the Miller value against oracle.pairing.miller_loop up to a factor in Fq4 (tower_cases.py says why Fq4).

Sizes: every op runs its whole list and then n in {1, 63, 64, 65, 130} rows of it, cycling from row n: one lane, the block edge, a
second block, a block with a two-lane tail (64 lanes per block).  The all-pairs product supplies the many-block shape.

Not here on purpose: miller_add_step at T = +-Q (outside its contract), a twist point with y = 0 (there is none: no 2-torsion), the
block products (commutative, covered through multi_pow / multi_pairing), and fq2_conj's canonical zero as raw device words -- the
entries exchange host records, whose export reduces; fq_sub(0, 0) on raw words is in tests/test_gpu_field_ops.py.
"""
import ctypes as C

import numpy as np
import pytest

from gemini_amd import pairing as gp
from gemini_amd.g2msm import _fq_int, _fq_limbs, g2_points_to_affine
from oracle import pairing as OP
from tests import g2_ref
from tests import tower_cases as tc
from tests.test_gpu_pairing import g1_points_to_affine

pytestmark = pytest.mark.gpu

Q = tc.Q
SIZES = (1, 63, 64, 65, 130)
GM_EINVAL = -1


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


def limbs(rows) -> np.ndarray:
    """rows of k canonical integers -> (n, 6 k) limbs of host records, read-only"""
    a = np.array([[w for c in r for w in _fq_limbs(c)] for r in rows], dtype=np.uint64)
    a.setflags(write=False)
    return a


def ints(row) -> tuple:
    return tuple(_fq_int(row[6 * k:6 * k + 6]) for k in range(len(row) // 6))


def flat(*f2s):
    return tuple(c for v in f2s for c in v)


def tiled(a, n: int):
    """n rows of `a`, cycling from row n"""
    return a[(np.arange(n) + n) % len(a)]


def same(got, want, names, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want)} rows differ, the first is {names[bad[0] % len(names)]}"


def run_op2(op, a, b, want, names, what):
    """the whole list, then the lane shapes"""
    same(gp.debug_gt_op2(op, a, b), want, names, what)
    for n in SIZES:
        got = gp.debug_gt_op2(op, tiled(a, n), None if b is None else tiled(b, n))
        assert got.shape == (n, 72)
        same(got, tiled(want, n), [names[(i + n) % len(names)] for i in range(len(names))], f"{what} at n = {n}")


# ---- the module's expected values: computed once, read-only ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def elements():
    el = tc.elements()
    return [n for n, _ in el], [v for _, v in el], limbs([v for _, v in el])


@pytest.fixture(scope="module")
def products():
    pc = tc.product_cases()
    return [f"{na} * {nb}" for (na, nb), _, _, _ in pc], limbs([a for _, a, _, _ in pc]), limbs([b for _, _, b, _ in pc]), limbs([w for _, _, _, w in pc])


@pytest.fixture(scope="module")
def lines():
    mc = tc.mul014_cases()
    return ([f"{na} by line {nl}" for (na, nl), _, _, _ in mc], [c[1] for c in mc], [c[2] for c in mc], limbs([c[1] for c in mc]),
            limbs([tc.line_record(*c[2]) for c in mc]), limbs([tc.embed_line(*c[2]) for c in mc]), limbs([c[3] for c in mc]))


# ---- gm_debug_gt_op2: the tower ----------------------------------------------------------------------------------------------------
def test_products_of_every_ordered_pair(gm, products):
    names, a, b, want = products
    assert len(a) >= 1156  # 19 blocks and more
    run_op2(gp.GT_OP2_MUL, a, b, want, names, "fq12_mul")


def test_squares(gm, elements):
    """against the oracle's a a, and bit for bit the device's own fq12_mul(a, a)"""
    names, vals, x = elements
    want = limbs([tc.ref_mul(v, v) for v in vals])
    run_op2(gp.GT_OP2_SQR, x, None, want, names, "fq12_sqr")
    same(gp.debug_gt_op2(gp.GT_OP2_SQR, x), gp.debug_gt_op2(gp.GT_OP2_MUL, x, x), names, "fq12_sqr against fq12_mul(a, a)")


def test_conjugation(gm, elements):
    names, vals, x = elements
    run_op2(gp.GT_OP2_CONJ, x, None, limbs([tc.ref_conj(v) for v in vals]), names, "fq12_conj")


def test_product_by_a_line(gm, lines):
    """fq12_mul_014 against the oracle's dense product by l0 + l1 v + l4 v w, and bit for bit the device's dense fq12_mul by it"""
    names, _, _, a, rec, emb, want = lines
    run_op2(gp.GT_OP2_MUL_014, a, rec, want, names, "fq12_mul_014")
    same(gp.debug_gt_op2(gp.GT_OP2_MUL_014, a, rec), gp.debug_gt_op2(gp.GT_OP2_MUL, a, emb), names, "fq12_mul_014 against fq12_mul")


def test_fq6_products(gm, elements, lines):
    """fq6_mul and fq6_mul_v on both halves of the element list; fq6_mul_01 / fq6_mul_1 by the (l0, l1) / the l4 of every line case"""
    names, vals, x = elements
    m = len(vals)
    pairs = [(i, (7 * i + 3) % m) for i in range(m)] + [(i, j) for i in range(m) for j in range(m) if names[i] in tc.MUL014_A and names[j] in tc.MUL014_A]
    pn = [f"{names[i]} * {names[j]}" for i, j in pairs]
    a, b = x[[i for i, _ in pairs]], x[[j for _, j in pairs]]
    run_op2(gp.GT_OP2_FQ6_MUL, a, b, limbs([tc.ref_fq6(vals[i], vals[j]) for i, j in pairs]), pn, "fq6_mul")
    run_op2(gp.GT_OP2_FQ6_MUL_V, x, None, limbs([tc.ref_fq6(v, tc.V6) for v in vals]), names, "fq6_mul_v")
    lnames, la, ll, a, rec, _, _ = lines
    run_op2(gp.GT_OP2_FQ6_MUL_01, a, rec, limbs([tc.ref_fq6(v, tc.b01(l[0], l[1])) for v, l in zip(la, ll)]), lnames, "fq6_mul_01")
    rec1 = limbs([tc.line_record(l[2], l[0], l[1]) for l in ll])  # b1 = l4 in the first slot; the other slots are not read
    run_op2(gp.GT_OP2_FQ6_MUL_1, a, rec1, limbs([tc.ref_fq6(v, tc.b1v(l[2])) for v, l in zip(la, ll)]), lnames, "fq6_mul_1")


def test_fq2_helpers(gm):
    """fq2_mul_xi with a borrow, a carry, a0 = a1; fq2_mul12 and fq2_mul_fq at 0, 1, q - 1 and the halves; fq2_conj of c1 = 0"""
    recs = tc.pack_slots(tc.fq2_values())
    names = [f"fq2_values()[{6 * i}:{6 * i + 6}]" for i in range(len(recs))]
    x = limbs(recs)
    run_op2(gp.GT_OP2_FQ2_MUL_XI, x, None, limbs([tc.map_slots(r, tc.f2_mul_xi) for r in recs]), names, "fq2_mul_xi")
    run_op2(gp.GT_OP2_FQ2_MUL12, x, None, limbs([tc.map_slots(r, tc.f2_mul12) for r in recs]), names, "fq2_mul12")
    run_op2(gp.GT_OP2_FQ2_CONJ, x, None, limbs([tc.map_slots(r, tc.f2_conj) for r in recs]), names, "fq2_conj")
    a, b, want, nm = [], [], [], []
    for s in tc.FQ_SCALARS:
        for r, n in zip(recs, names):
            a.append(r)
            b.append(tc.from_slots([(s, Q - 1)] * 6))  # the scalar is the c0 of the slot; its c1 is not read
            want.append(tc.map_slots(r, lambda v: tc.f2_mul_fq(v, s)))
            nm.append(f"{n} by {s:#x}")
    run_op2(gp.GT_OP2_FQ2_MUL_FQ, limbs(a), limbs(b), limbs(want), nm, "fq2_mul_fq")


# ---- gm_debug_miller_step ----------------------------------------------------------------------------------------------------------
def run_steps(op, cases, step, law, other):
    names = [c.name for c in cases]
    T, Qr, Pr = limbs([flat(*c.T) for c in cases]), limbs([flat(*c.Q) for c in cases]), limbs([c.P for c in cases])
    exp = [step(c) for c in cases]
    want_t, want_l = limbs([flat(*t) for t, _ in exp]), limbs([flat(*l) for _, l in exp])
    got_t, got_l = gp.debug_miller_step(op, T, Qr, Pr)
    for c, rt, rl in zip(cases, got_t, got_l):  # the independent statements, on what the device returned
        t, l = tc.slots(ints(rt)), tc.slots(ints(rl))
        assert t[2] != (0, 0), c.name
        assert tc.normalise(t) == law(c), c.name
        assert tc.is_w3_times_fq2(tc.ratio_w(tc.embed_line(*l), tc.geometric_line(c.t_affine, other(c), c.P))), c.name
    same(got_t, want_t, names, "the new T")
    same(got_l, want_l, names, "the line")
    for n in SIZES:
        gt, gl = gp.debug_miller_step(op, tiled(T, n), tiled(Qr, n), tiled(Pr, n))
        assert gt.shape == gl.shape == (n, 36)
        assert (gt == tiled(want_t, n)).all() and (gl == tiled(want_l, n)).all(), n


def test_doubling_step(gm):
    """miller_dbl_step: T = k Q at five Z, a twist point outside the r-torsion, four (x_P, y_P) -- the new T is 2 T, the line the
    tangent up to c w^3, and both equal the transliteration bit for bit"""
    run_steps(gp.MILLER_OP_DBL, tc.dbl_cases(), lambda c: tc.dbl_step(c.T, c.P), lambda c: g2_ref.add(c.t_affine, c.t_affine), lambda c: c.t_affine)


def test_addition_step(gm):
    """miller_add_step for T != +-Q (its contract): the new T is T + Q, the line the chord up to c w^3, bit for bit the transliteration"""
    run_steps(gp.MILLER_OP_ADD, tc.add_cases(), lambda c: tc.add_step(c.T, c.Q, c.P), lambda c: g2_ref.add(c.t_affine, c.Q), lambda c: c.Q)


# ---- gm_debug_miller_each ----------------------------------------------------------------------------------------------------------
def test_raw_miller_values(gm):
    """the lane's column after miller_lane, n in {1, 2, 65} pairs: bit for bit the restated loop; against oracle.pairing.miller_loop up
    to a factor in Fq4; exactly 1 with a point at infinity; and its conjugate's final exponentiation is the library's pairing"""
    pairs = tc.miller_pairs()
    names = [n for n, _, _ in pairs]
    r1 = g1_points_to_affine([p for _, p, _ in pairs], flag=True)
    r2 = g2_points_to_affine([q for _, _, q in pairs], flag=True)
    want = limbs(tc.miller_expected())
    got = gp.debug_miller_each(r1, r2)
    same(got, want, names, "miller_lane")
    one = gp.gt_one()
    for (name, p1, q2), row in zip(pairs, got):
        if p1 is None or q2 is None:
            assert (row == one).all(), name
        else:
            assert tc.is_in_fq4(tc.ratio_w(ints(row), OP.miller_loop(q2, p1))), name
    for n in (1, 2, 65):
        same(gp.debug_miller_each(tiled(r1, n), tiled(r2, n)), tiled(want, n), [names[(i + n) % len(names)] for i in range(len(names))], f"miller_lane at n = {n}")
    each = gp.pairing_each(r1, r2)
    conj = gp.debug_gt_op2(gp.GT_OP2_CONJ, got)
    for i, name in enumerate(names):
        assert (gp.gt_final_exp(conj[i]) == each[i]).all(), name


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(gm):
    lib, x = gm.capi.load(), np.zeros((1, 72), dtype=np.uint64)
    p, n1, n0 = gm.capi.ptr(x), C.c_size_t(1), C.c_size_t(0)
    for op in (-1, 12):
        assert lib.gm_debug_gt_op2(C.c_int(op), p, p, n1, p) == GM_EINVAL
    for op in (gp.GT_OP2_MUL, gp.GT_OP2_MUL_014, gp.GT_OP2_FQ6_MUL, gp.GT_OP2_FQ6_MUL_01, gp.GT_OP2_FQ6_MUL_1, gp.GT_OP2_FQ2_MUL_FQ):
        assert lib.gm_debug_gt_op2(C.c_int(op), p, None, n1, p) == GM_EINVAL  # a binary op without its second operand
    assert lib.gm_debug_gt_op2(C.c_int(0), None, p, n1, p) == GM_EINVAL
    assert lib.gm_debug_gt_op2(C.c_int(0), p, p, n1, None) == GM_EINVAL
    assert lib.gm_debug_gt_op2(C.c_int(0), None, None, n0, None) == 0
    for op in (-1, 2):
        assert lib.gm_debug_miller_step(C.c_int(op), p, n1, p) == GM_EINVAL
    assert lib.gm_debug_miller_step(C.c_int(0), None, n1, p) == GM_EINVAL
    assert lib.gm_debug_miller_step(C.c_int(0), None, n0, None) == 0
    assert lib.gm_debug_miller_each(None, C.c_size_t(96), p, C.c_size_t(192), n1, p) == GM_EINVAL
    assert lib.gm_debug_miller_each(p, C.c_size_t(96), p, C.c_size_t(192), n1, None) == GM_EINVAL
    assert lib.gm_debug_miller_each(None, C.c_size_t(96), None, C.c_size_t(192), n0, None) == 0
