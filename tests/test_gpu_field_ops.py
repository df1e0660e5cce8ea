"""GPU: the device's field arithmetic element by element, at the edges, against Python integers (gm_debug_fq_op, gm_debug_fq30_op,
gm_debug_fq2_op; gemini_amd/debug.py).

Every function is applied to records the test spells limb by limb and the limbs it leaves are compared bit for bit with the
integer result: the unique residue in device form for the canonical layers (a b 2^-390 mod q for the product), the exact Montgomery
quotient (ab + (-ab q^-1 mod 2^390) q) >> 390 with normalised limbs for the loose products.  The reference is tests/field_cases.py:
`pow`, `%`, nothing else.  The operands are the named lists there: 0, 1, q - 1, all-ones limbs in both radices, single limbs at every
position, pairs solved so that the raw product lands in [q, 1.002 q), a - b with a borrow out of every word, loose values at 2^386 - 1.

Sizes: every op runs once over its whole list (a few thousand lanes, many blocks), and the binary / unary kernels run again at
n in {1, 63, 64, 65, 130} -- the block edge (64 lanes per block), a second block, a two-lane tail -- on the list tiled with a shift,
so that edge operands sit in partial waves next to the harmless operand the idle lanes run.
"""
import ctypes as C

import numpy as np
import pytest

from gemini_amd import debug as D
from tests import field_cases as fc

pytestmark = pytest.mark.gpu

Q = fc.Q
SIZES = [1, 63, 64, 65, 130]
GM_EINVAL = -1


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


def tiled(a, n: int, shift: int = 0):
    """n rows of `a`, cycling from row `shift`"""
    return a[(np.arange(n) + shift) % len(a)]


def frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


def same(got: np.ndarray, want: np.ndarray, names):
    """bit for bit; on a mismatch name the first case"""
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (f"{len(bad)} of {len(got)} lanes differ; first: lane {bad[0]} ({names[bad[0] % len(names)]})",
                           [hex(int(w)) for w in got[bad[0]]], [hex(int(w)) for w in want[bad[0]]])


# ---- the integer references, computed once ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fq_binary():
    """(names, a (m, 12), b (m, 12), {op: expected (m, 12)}) over FQ_PAIRS"""
    names = [n for n, _, _ in fc.FQ_PAIRS]
    a = frozen(D.rows_words([a for _, a, _ in fc.FQ_PAIRS]))
    b = frozen(D.rows_words([b for _, _, b in fc.FQ_PAIRS]))
    exp = {D.FQ_MUL: frozen(D.rows_words([fc.mm(x, y) for _, x, y in fc.FQ_PAIRS])),
           D.FQ_ADD: frozen(D.rows_words([(x + y) % Q for _, x, y in fc.FQ_PAIRS])),
           D.FQ_SUB: frozen(D.rows_words([(x - y) % Q for _, x, y in fc.FQ_PAIRS]))}
    return names, a, b, exp


@pytest.fixture(scope="module")
def fq_unary():
    """over every value that occurs in FQ_PAIRS (the solved operands included: a square has its own conditional subtraction)"""
    vals = list(fc.FQ_VALUES) + [b for n, _, b in fc.FQ_PAIRS if n.startswith(("solved", "product"))]
    # squares solved for a small result: a^2 2^-390 = t  <=>  a = sqrt(t 2^390), q = 3 mod 4
    for t in range(1, 400):
        r = pow(t * fc.R390 % Q, (Q + 1) // 4, Q)
        if fc.mm(r, r) == t:
            vals.append(r)
    names = [fc.FQ_NAME.get(v, hex(v)) for v in vals]
    a = frozen(D.rows_words(vals))
    exp = {D.FQ_SQR: [fc.mm(v, v) for v in vals], D.FQ_DBL: [2 * v % Q for v in vals], D.FQ_NEG: [-v % Q for v in vals],
           D.FQ_IMPORT: [fc.mm(v, fc.CIN) for v in vals], D.FQ_EXPORT: [fc.mm(v, fc.COUT) for v in vals], D.FQ_PACK_UNPACK: vals}
    return names, a, {k: frozen(D.rows_words(v)) for k, v in exp.items()}


@pytest.fixture(scope="module")
def loose_binary():
    names = [n for n, _, _ in fc.LOOSE_PAIRS]
    a = frozen(D.rows_limbs30([a for _, a, _ in fc.LOOSE_PAIRS]))
    b = frozen(D.rows_limbs30([b for _, _, b in fc.LOOSE_PAIRS]))
    quot = [fc.mont_quotient(x, y) for _, x, y in fc.LOOSE_PAIRS]
    assert all(v % Q == fc.mm(x, y) and v < Q + (x * y >> 390) + 1 for v, (_, x, y) in zip(quot, fc.LOOSE_PAIRS))
    return names, a, b, frozen(D.rows_limbs30(quot))  # rows_limbs30 asserts the value fits normalised limbs


# ---- Fq: the canonical layer --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [D.FQ_MUL, D.FQ_ADD, D.FQ_SUB])
def test_fq_binary_whole_list(gm, fq_binary, op):
    names, a, b, exp = fq_binary
    same(D.fq_op(op, a, b), exp[op], names)


@pytest.mark.parametrize("n", SIZES)
def test_fq_binary_block_edges(gm, fq_binary, n):
    """the edge-heavy tail of the list (solved pairs, products 0 / 1 / q - 1, the borrows) and its head, tiled with a shift"""
    names, a, b, exp = fq_binary
    for op in (D.FQ_MUL, D.FQ_ADD, D.FQ_SUB):
        for shift in (n, len(a) - 345 + n):
            got = D.fq_op(op, tiled(a, n, shift), tiled(b, n, shift))
            same(got, tiled(exp[op], n, shift), np.roll(names, -shift))


@pytest.mark.parametrize("op", [D.FQ_SQR, D.FQ_DBL, D.FQ_NEG, D.FQ_IMPORT, D.FQ_EXPORT, D.FQ_PACK_UNPACK])
def test_fq_unary_whole_list(gm, fq_unary, op):
    names, a, exp = fq_unary
    same(D.fq_op(op, a), exp[op], names)


@pytest.mark.parametrize("n", SIZES)
def test_fq_unary_block_edges(gm, fq_unary, n):
    names, a, exp = fq_unary
    for op in exp:
        got = D.fq_op(op, tiled(a, n, n))
        same(got, tiled(exp[op], n, n), np.roll(names, -n))


def test_fq_neg_of_zero_is_zero(gm):
    """-0 stays the exact zero of the identity record, not q"""
    got = D.fq_op(D.FQ_NEG, D.rows_words([0, 0, 1]))
    assert not got[:2].any() and D.from_words(got[2]) == Q - 1


def test_fq_square_is_the_product_with_itself(gm, fq_unary):
    _, a, exp = fq_unary
    same(D.fq_op(D.FQ_MUL, a, a), exp[D.FQ_SQR], ["mul(a, a)"])


def test_fq_inverse(gm):
    """fq_inv is Fermat's a^(q - 2): the inverse, and 0 for 0 (the ladder multiplies the operand in at its first step and
    0 stays 0) -- 0, 1, q - 1 and the rest of the list, a partial second block"""
    names = [n for n, _ in fc.FQ]
    a = D.rows_words(fc.FQ_VALUES)
    want = D.rows_words([fc.fq_inv_expected(v) for v in fc.FQ_VALUES])
    assert fc.fq_inv_expected(0) == 0 and fc.mm(fc.fq_inv_expected(Q - 1), Q - 1) == fc.ONE
    same(D.fq_op(D.FQ_INV, a), want, names)
    same(D.fq_op(D.FQ_INV, a[:1]), want[:1], names)


def test_raw_ge_q(gm):
    """the only function that takes words >= q: q - 1, q, q + 1, 2^384 - 1, q +- 2^(32 k) for every word k"""
    names = [n for n, _ in fc.RAW_GE_Q]
    vals = [v for _, v in fc.RAW_GE_Q]
    want = np.zeros((len(vals), 12), dtype=np.uint32)
    want[:, 0] = [int(v >= Q) for v in vals]
    assert want[:, 0].sum() == 15
    a = D.rows_words(vals)
    same(D.fq_op(D.FQ_RAW_GE_Q, a), want, names)
    for n in (1, 65):
        same(D.fq_op(D.FQ_RAW_GE_Q, tiled(a, n, 1)), tiled(want, n, 1), np.roll(names, -1))


# ---- Fq30: the loose products -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [D.FQ30_MUL_ASM, D.FQ30_MUL_C])
def test_fq30_product_is_the_exact_quotient(gm, loose_binary, op):
    """the asm statement and the plain-C statement: the same 13 limbs, the integer quotient's"""
    names, a, b, want = loose_binary
    same(D.fq30_op(op, a, b), want, names)


def test_fq30_square_is_the_exact_quotient(gm):
    names = [n for n, _ in fc.LOOSE]
    vals = [v for _, v in fc.LOOSE]
    a = D.rows_limbs30(vals)
    want = D.rows_limbs30([fc.mont_quotient(v, v) for v in vals])
    same(D.fq30_op(D.FQ30_SQR_ASM, a), want, names)
    same(D.fq30_op(D.FQ30_MUL_ASM, a, a), want, names)
    same(D.fq30_op(D.FQ30_MUL_C, a, a), want, names)


@pytest.mark.parametrize("n", SIZES)
def test_fq30_block_edges(gm, loose_binary, n):
    names, a, b, want = loose_binary
    L = len(fc.LOOSE)
    shift = L + n  # row L on: 2^386 - 1 against the whole list
    for op in (D.FQ30_MUL_ASM, D.FQ30_MUL_C):
        same(D.fq30_op(op, tiled(a, n, shift), tiled(b, n, shift)), tiled(want, n, shift), np.roll(names, -shift))
    d = tiled(a[::L], n, n)  # every value of the list once
    sq = D.rows_limbs30([fc.mont_quotient(v, v) for _, v in fc.LOOSE])
    same(D.fq30_op(D.FQ30_SQR_ASM, d), tiled(sq, n, n), np.roll([m for m, _ in fc.LOOSE], -n))


def test_fq30_loose_to_canonical(gm):
    """every loose representative -- residue + j q up to 2^386, 2^386 - 1 -- gives its residue: 12 words and a zero"""
    names = [n for n, _ in fc.LOOSE]
    vals = [v for _, v in fc.LOOSE]
    want = np.zeros((len(vals), 13), dtype=np.uint32)
    want[:, :12] = D.rows_words([v % Q for v in vals])
    a = D.rows_limbs30(vals)
    same(D.fq30_op(D.FQ30_LOOSE_TO_CANONICAL, a), want, names)
    for n in (1, 65):
        same(D.fq30_op(D.FQ30_LOOSE_TO_CANONICAL, tiled(a, n, 3)), tiled(want, n, 3), np.roll(names, -3))


def test_fq30_canonical_tail(gm):
    """alone, on q - 1, q, q + 1 and the largest value fq30_loose_to_canonical can hand it (1.0625 q): one subtraction of q when the
    value is >= q, none below"""
    names = [n for n, _ in fc.TAIL]
    vals = [v for _, v in fc.TAIL]
    want = D.rows_limbs30([v - Q if v >= Q else v for v in vals])
    a = D.rows_limbs30(vals)
    same(D.fq30_op(D.FQ30_CANONICAL_TAIL, a), want, names)
    same(D.fq30_op(D.FQ30_CANONICAL_TAIL, tiled(a, 65, 2)), tiled(want, 65, 2), np.roll(names, -2))


# ---- Fq2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fq2_binary():
    names = [n for n, _, _ in fc.FQ2_PAIRS]
    a = frozen(D.rows_words([a for _, a, _ in fc.FQ2_PAIRS], 2))
    b = frozen(D.rows_words([b for _, _, b in fc.FQ2_PAIRS], 2))
    exp = {D.FQ2_MUL: [fc.fq2_mul(x, y) for _, x, y in fc.FQ2_PAIRS],
           D.FQ2_ADD: [((x[0] + y[0]) % Q, (x[1] + y[1]) % Q) for _, x, y in fc.FQ2_PAIRS],
           D.FQ2_SUB: [((x[0] - y[0]) % Q, (x[1] - y[1]) % Q) for _, x, y in fc.FQ2_PAIRS]}
    return names, a, b, {k: frozen(D.rows_words(v, 2)) for k, v in exp.items()}


@pytest.mark.parametrize("op", [D.FQ2_MUL, D.FQ2_ADD, D.FQ2_SUB])
def test_fq2_binary_whole_list(gm, fq2_binary, op):
    names, a, b, exp = fq2_binary
    same(D.fq2_op(op, a, b), exp[op], names)


@pytest.mark.parametrize("n", SIZES)
def test_fq2_block_edges(gm, fq2_binary, n):
    names, a, b, exp = fq2_binary
    for op in exp:
        same(D.fq2_op(op, tiled(a, n, n), tiled(b, n, n)), tiled(exp[op], n, n), np.roll(names, -n))


def test_fq2_unary(gm):
    """square, negation, inverse over the list: c0 = 0, c1 = 0, a and its conjugate, a^2 real, u, u + 1, norm 1, the Fq list in
    either coefficient.  The inverse is (a0 - a1 u) / (a0^2 + a1^2) on integers (tests/g2_ref.py); 0 is not its input."""
    names = [n for n, _ in fc.FQ2]
    vals = [v for _, v in fc.FQ2]
    a = D.rows_words(vals, 2)
    same(D.fq2_op(D.FQ2_SQR, a), D.rows_words([fc.fq2_mul(v, v) for v in vals], 2), names)
    same(D.fq2_op(D.FQ2_NEG, a), D.rows_words([(-v[0] % Q, -v[1] % Q) for v in vals], 2), names)
    nz = [(n, v) for n, v in fc.FQ2 if v != (0, 0)]
    inv = [fc.fq2_inv(v) for _, v in nz]
    assert all(fc.fq2_mul(v, i) == (fc.ONE, 0) for (_, v), i in zip(nz, inv))
    for sl in (slice(None), slice(0, 1), slice(5, 70)):
        same(D.fq2_op(D.FQ2_INV, D.rows_words([v for _, v in nz][sl], 2)), D.rows_words(inv[sl], 2), [n for n, _ in nz][sl])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,width,nops", [("gm_debug_fq_op", 12, 11), ("gm_debug_fq30_op", 13, 5), ("gm_debug_fq2_op", 24, 6),
                                              ("gm_debug_g1_op", 48, 5), ("gm_debug_g2_op", 96, 5)])
def test_refusals(gm, entry, width, nops):
    f = getattr(gm.capi.load(), entry)
    x, out = np.ones((1, width), dtype=np.uint32), np.zeros((1, width), dtype=np.uint32)
    p, o = gm.capi.ptr(x), gm.capi.ptr(out)
    assert f(C.c_int(nops), p, p, C.c_size_t(1), o) == GM_EINVAL
    assert f(C.c_int(-1), p, p, C.c_size_t(1), o) == GM_EINVAL
    assert f(C.c_int(0), None, p, C.c_size_t(1), o) == GM_EINVAL
    assert f(C.c_int(0), p, None, C.c_size_t(1), o) == GM_EINVAL  # op 0 reads its second operand everywhere
    assert f(C.c_int(0), p, p, C.c_size_t(1), None) == GM_EINVAL
    assert f(C.c_int(0), None, None, C.c_size_t(0), None) == 0
    assert not out.any()


def test_acc30_refusals(gm):
    f = gm.capi.load().gm_debug_acc30_op
    acc, oth, neg = np.zeros((1, 52), dtype=np.uint32), np.ones((1, 52), dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    out, canon = np.zeros((1, 52), dtype=np.uint32), np.zeros((1, 48), dtype=np.uint32)
    p = gm.capi.ptr
    assert f(C.c_int(2), p(acc), p(oth), p(neg), C.c_size_t(1), p(out), p(canon)) == GM_EINVAL
    assert f(C.c_int(-1), p(acc), p(oth), p(neg), C.c_size_t(1), p(out), p(canon)) == GM_EINVAL
    assert f(C.c_int(0), None, p(oth), p(neg), C.c_size_t(1), p(out), p(canon)) == GM_EINVAL
    assert f(C.c_int(0), p(acc), None, p(neg), C.c_size_t(1), p(out), p(canon)) == GM_EINVAL
    assert f(C.c_int(0), p(acc), p(oth), None, C.c_size_t(1), p(out), p(canon)) == GM_EINVAL
    assert f(C.c_int(0), p(acc), p(oth), p(neg), C.c_size_t(1), None, p(canon)) == GM_EINVAL
    assert f(C.c_int(0), p(acc), p(oth), p(neg), C.c_size_t(1), p(out), None) == GM_EINVAL
    assert f(C.c_int(0), None, None, None, C.c_size_t(0), None, None) == 0
