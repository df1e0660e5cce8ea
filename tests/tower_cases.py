"""The operands and the integer references of tests/test_gpu_tower_ops.py: the Fq12 tower of gt.cuh and the Miller-loop steps of
pairing.hip, one device function per lane.  tests/test_tower_cases_cpu.py validates every list and reference here without a GPU.

Everything is Python integers.  An Fq2 value is a pair (c0, c1), an Fq12 element 12 integers in tower order (index 6 h + 2 j + k is
the coefficient of u^k v^j w^h, tests/test_pairing_cpu.py), a twist point ((x0, x1), (y0, y1)).

References.
  the tower     oracle/pairing.py's f12_mul on polynomials in w over Fq, through tower_to_w / w_to_tower: it shares no structure with the
                Karatsuba layers of gt.cuh.  Sparse operands (a line, an Fq6 half, v) are embedded and multiplied densely.
  the steps     `dbl_step` / `add_step` are LITERAL transliterations of miller_dbl_step / miller_add_step, statement by statement, so the
                device can be compared with them bit for bit.  What makes them a reference is checked against independent statements:
                the new T, divided by its Z, is 2 T / T + Q by the affine chord and tangent of tests/g2_ref.py, and the line relates to
                oracle.pairing._line as described next.
  the subfield  The device's line l0 + l1 v + l4 v w equals the oracle's affine line through the untwisted points, evaluated at the
                embedded (x_P, y_P), times c w^3 with c a non-zero element of Fq2 (c = 2 Y Z for the tangent, -(X - x_Q Z) for the chord:
                the untwisting divides x by w^2 and y by w^3).  w^3 is not in Fq2 or Fq6 but in Fq4 = Fq2(w^3) (w^6 = xi), and
                (q^4 - 1) divides (q^12 - 1) / r, so the final exponentiation removes the factor.  In the w basis `is_w3_times_fq2`
                (only w^3 and w^9) states the property of one line, `is_in_fq4` (only w^0, w^3, w^6, w^9) that of a whole Miller value,
                where the factors of 131 lines multiply.

The lists are built once, deterministically, and never modified."""
import collections
import functools
import random

from gemini_amd import g2
from oracle import pairing as OP
from oracle import pyref as P
from tests import g2_ref
from tests import gt_check_ref as ref
from tests.test_pairing_cpu import tower_to_w, w_to_tower

Q, R = OP.Q, OP.R
HALF_LO, HALF_HI = (Q - 1) // 2, (Q + 1) // 2
ZERO12, ONE12 = (0,) * 12, (1,) + (0,) * 11


# ---- Fq2 on integers -------------------------------------------------------------------------------------------------------------
def f2_add(a, b):
    return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)


def f2_sub(a, b):
    return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def f2_sqr(a):
    return f2_mul(a, a)


def f2_dbl(a):
    return f2_add(a, a)


def f2_neg(a):
    return ((-a[0]) % Q, (-a[1]) % Q)


def f2_inv(a):
    d = pow(a[0] * a[0] + a[1] * a[1], -1, Q)
    return (a[0] * d % Q, -a[1] * d % Q)


# the four helpers of gt.cuh, stated from their definitions (not from the device's formulas)
def f2_mul_xi(a):
    return f2_mul(a, (1, 1))


def f2_mul12(a):
    return (12 * a[0] % Q, 12 * a[1] % Q)


def f2_mul_fq(a, s):
    return (a[0] * s % Q, a[1] * s % Q)


def f2_conj(a):
    return (a[0], (-a[1]) % Q)


# ---- the tower through the oracle ------------------------------------------------------------------------------------------------
def ref_mul(a, b):
    return tuple(w_to_tower(OP.f12_mul(tower_to_w(a), tower_to_w(b))))


def ref_conj(a):
    return tuple(w_to_tower(ref.conj_w(tower_to_w(a))))


def slots(a):
    """2 k integers -> k Fq2 values in order (12 integers: the six Fq2 of an Fq12 in tower order)"""
    return [(a[2 * k], a[2 * k + 1]) for k in range(len(a) // 2)]


def from_slots(s):
    return tuple(c for v in s for c in v)


def embed_line(l0, l1, l4):
    """l0 + l1 v + l4 v w"""
    return from_slots([l0, l1, (0, 0), (0, 0), l4, (0, 0)])


def line_record(l0, l1, l4):
    """the operand b of GT_OP2_MUL_014: the line in the first three Fq2 slots"""
    return from_slots([l0, l1, l4, (0, 0), (0, 0), (0, 0)])


def ref_mul_014(a, l0, l1, l4):
    """a l0 + (a l1) v + (a l4) v w, term by term: tests/test_tower_cases_cpu.py checks it equals ref_mul(a, embed_line(...))"""
    z = (0, 0)
    t0 = tower_to_w(ref_mul(a, embed_line(l0, z, z)))
    t1 = tower_to_w(ref_mul(a, embed_line(z, l1, z)))
    t4 = tower_to_w(ref_mul(a, embed_line(z, z, l4)))
    return tuple(w_to_tower(OP.f12_add(OP.f12_add(t0, t1), t4)))


def _half(a, h):
    """the Fq6 half c_h of a as an Fq12 element with c1 = 0"""
    return tuple(a[6 * h:6 * h + 6]) + (0,) * 6


def ref_fq6(a, b):
    """(a.c0 b.c0, a.c1 b.c1): what GT_OP2_FQ6_MUL and its sparse forms return, b an embedded Fq6 operand per half"""
    out = ()
    for h in range(2):
        r = ref_mul(_half(a, h), _half(b, h))
        assert r[6:] == (0,) * 6
        out += r[:6]
    return out


V6 = from_slots([(0, 0), (1, 0), (0, 0)] * 2)  # v in both halves


def b01(b0, b1):
    return from_slots([b0, b1, (0, 0)] * 2)


def b1v(b1):
    return from_slots([(0, 0), b1, (0, 0)] * 2)


# ---- Fq12 elements ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def elements():
    """((name, 12 integers), ...): the edge elements, the sparse ones, and the values the library meets; unique by value (1 is also
    the basis element 1 with coefficient 1, -1 the one with coefficient q - 1)"""
    rnd = random.Random(0x746F776572)
    adv = {n: tuple(c) for n, c, _ in ref.adversarial()}
    out = [("0", ZERO12), ("1", ONE12), ("-1", (Q - 1,) + (0,) * 11)]
    for k in range(12):
        for cn, c in (("1", 1), ("q-1", Q - 1)):
            out.append((f"basis{k}*{cn}", tuple(c if i == k else 0 for i in range(12))))
    out += [("all q-1", (Q - 1,) * 12), ("all (q-1)/2", (HALF_LO,) * 12), ("all (q+1)/2", (HALF_HI,) * 12)]
    out.append(("in Fq2", (rnd.randrange(Q), rnd.randrange(Q)) + (0,) * 10))
    out.append(("in Fq6", tuple(rnd.randrange(Q) for _ in range(6)) + (0,) * 6))
    out.append(("c0 = 0", (0,) * 6 + tuple(rnd.randrange(Q) for _ in range(6))))
    out += [("GT member", adv["member0"]), ("Miller value", adv["miller0"]), ("cyclotomic non-member", adv["cyclotomic_non_member"])]
    out += [(f"random{i}", tuple(rnd.randrange(Q) for _ in range(12))) for i in range(2)]
    seen, uniq = set(), []
    for n, v in out:
        if v not in seen:
            seen.add(v)
            uniq.append((n, v))
    return tuple(uniq)


def element(name):
    return dict(elements())[name]


@functools.lru_cache(maxsize=None)
def product_cases():
    """every ordered pair of the list: ((name a, name b), a, b, a b)"""
    el = elements()
    w = [tower_to_w(v) for _, v in el]
    return tuple(((na, nb), a, b, tuple(w_to_tower(OP.f12_mul(w[i], w[j])))) for i, (na, a) in enumerate(el) for j, (nb, b) in enumerate(el))


# ---- lines for fq12_mul_014 ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def line_triples():
    """((name, l0, l1, l4), ...): each slot from {0, 1, (q-1) + (q-1) u, random}, all 64 combinations; l1 + l4 wrapping past q in both
    components; l1 = -l4 (the Karatsuba middle term fq2_add(l1, l4) is zero)"""
    rnd = random.Random(0x6C696E65)
    r2 = lambda: (rnd.randrange(Q), rnd.randrange(Q))
    vals = (("0", (0, 0)), ("1", (1, 0)), ("-1-u", (Q - 1, Q - 1)), ("rnd", r2()))
    out = [(f"{a[0]},{b[0]},{c[0]}", a[1], b[1], c[1]) for a in vals for b in vals for c in vals]
    out.append(("l1+l4 wraps", r2(), (HALF_HI, Q - 1), (HALF_HI, 2)))
    l4 = r2()
    out.append(("l1=-l4", r2(), f2_neg(l4), l4))
    return tuple(out)


MUL014_A = ("random0", "1", "all q-1", "in Fq6", "c0 = 0")


@functools.lru_cache(maxsize=None)
def mul014_cases():
    """((name a, name line), a, (l0, l1, l4), a (l0 + l1 v + l4 v w)) for the five a crossed with every triple"""
    out = []
    for na in MUL014_A:
        a = element(na)
        for nl, l0, l1, l4 in line_triples():
            out.append(((na, nl), a, (l0, l1, l4), ref_mul(a, embed_line(l0, l1, l4))))
    return tuple(out)


# ---- the Fq2 helpers -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fq2_values():
    """{0, 1, q-1, (q-1)/2, (q+1)/2} in either component -- a0 < a1 (fq2_mul_xi borrows), a0 + a1 >= q (it carries; = q exactly for
    (q-1, 1) and ((q+1)/2, (q-1)/2)), a0 = a1, c1 = 0 (fq2_conj must give 0) -- and random values of each of the three kinds"""
    rnd = random.Random(0x667132)
    s = (0, 1, Q - 1, HALF_LO, HALF_HI)
    out = [(a, b) for a in s for b in s]
    lo, hi = rnd.randrange(Q // 2), rnd.randrange(Q // 2, Q)
    out += [(lo, hi), (hi, rnd.randrange(Q // 2, Q)), (lo, lo), (hi, hi), (hi, 0), (0, hi)]
    assert any(a < b for a, b in out) and any(a + b >= Q for a, b in out) and any(a + b == Q for a, b in out)
    return tuple(out)


FQ_SCALARS = (0, 1, Q - 1, HALF_HI, 0x123456789ABCDEF0FEDCBA9876543210 << 200)


def pack_slots(vals):
    """Fq2 values -> records of six (the last one filled by cycling)"""
    vals = list(vals)
    vals += [vals[i % len(vals)] for i in range(-len(vals) % 6)]
    return [from_slots(vals[i:i + 6]) for i in range(0, len(vals), 6)]


def map_slots(rec, fn):
    return from_slots([fn(v) for v in slots(rec)])


# ---- the steps: literal transliterations of pairing.hip --------------------------------------------------------------------------
def dbl_step(T, Pxy):
    """miller_dbl_step: (new T, (l0, l1, l4))"""
    X, Y, Z = T
    a = f2_mul(X, Y)
    b = f2_sqr(Y)
    c = f2_sqr(Z)
    e = f2_mul12(f2_mul_xi(c))
    f = f2_add(f2_dbl(e), e)
    g = f2_add(b, f)
    h = f2_sub(f2_sub(f2_sqr(f2_add(Y, Z)), b), c)
    j = f2_sqr(X)
    l0 = f2_sub(e, b)
    l1 = f2_mul_fq(f2_add(f2_dbl(j), j), Pxy[0])
    l4 = f2_mul_fq(f2_neg(h), Pxy[1])
    X3 = f2_dbl(f2_mul(a, f2_sub(b, f)))
    Y3 = f2_sub(f2_sqr(g), f2_mul12(f2_sqr(e)))
    Z3 = f2_dbl(f2_dbl(f2_mul(b, h)))
    return (X3, Y3, Z3), (l0, l1, l4)


def add_step(T, Qa, Pxy):
    """miller_add_step (T != +-Q): (new T, (l0, l1, l4))"""
    X, Y, Z = T
    theta = f2_sub(Y, f2_mul(Qa[1], Z))
    lam = f2_sub(X, f2_mul(Qa[0], Z))
    c = f2_sqr(theta)
    d = f2_sqr(lam)
    e = f2_mul(lam, d)
    f = f2_mul(Z, c)
    g = f2_mul(X, d)
    h = f2_sub(f2_add(e, f), f2_dbl(g))
    l0 = f2_sub(f2_mul(theta, Qa[0]), f2_mul(lam, Qa[1]))
    l1 = f2_mul_fq(f2_neg(theta), Pxy[0])
    l4 = f2_mul_fq(lam, Pxy[1])
    Y3 = f2_sub(f2_mul(theta, f2_sub(g, h)), f2_mul(e, Y))
    X3 = f2_mul(lam, h)
    Z3 = f2_mul(Z, e)
    return (X3, Y3, Z3), (l0, l1, l4)


def normalise(T):
    """(X, Y, Z) with Z != 0 -> the affine point (X / Z, Y / Z)"""
    zi = f2_inv(T[2])
    return (f2_mul(T[0], zi), f2_mul(T[1], zi))


def on_twist(p) -> bool:
    return g2.on_curve(p)


def geometric_line(p1, p2, Pxy):
    """oracle.pairing._line through the untwisted twist points p1, p2 (the tangent when equal) at the embedded (x_P, y_P); the pair
    need not be a point of the curve"""
    return OP._line(OP.untwist(p1), OP.untwist(p2), (OP.f12(Pxy[0]), OP.f12(Pxy[1])))


def ratio_w(x_tower, y_w):
    """x / y in the w basis"""
    return OP.f12_mul(tower_to_w(x_tower), OP.f12_inv(y_w))


def is_w3_times_fq2(x_w) -> bool:
    """non-zero and c w^3 for c in Fq2: only the coefficients at w^3 and w^9"""
    return any(x_w) and all(v == 0 for k, v in enumerate(x_w) if k not in (3, 9))


def is_in_fq4(x_w) -> bool:
    """non-zero and in Fq4 = Fq2(w^3): only the coefficients at w^0, w^3, w^6, w^9"""
    return any(x_w) and all(v == 0 for k, v in enumerate(x_w) if k % 3)


StepCase = collections.namedtuple("StepCase", "name T Q P t_affine")


@functools.lru_cache(maxsize=None)
def outside_point():
    """a point of the twist y^2 = x^3 + 4 (1 + u) OUTSIDE the r-torsion: the first x = k (k = 1, 2, ...) with a root"""
    for k in range(1, 100):
        x = (k, 0)
        y = g2.f2_sqrt(f2_add(f2_mul(f2_sqr(x), x), (4, 4)))
        if y is not None:
            p = (x, y)
            assert g2.on_curve(p) and not g2.in_prime_order_subgroup(p)
            return p
    raise AssertionError("no point found")


K255 = 0x5A3C9E17F0B2D4C6A8E1F3057192B4D6F8A0C2E4061728394A5B6C7D8E9FA0B1 % R
STEP_KS = (1, 2, 3, K255)


@functools.lru_cache(maxsize=None)
def _step_parts():
    rnd = random.Random(0x73746570)
    zs = (("Z=1", (1, 0)), ("Z=q-1", (Q - 1, 0)), ("Z=u", (0, 1)), ("Z real", (rnd.randrange(2, Q), 0)), ("Z rnd", (rnd.randrange(Q), rnd.randrange(Q))))
    g1 = P.g1_mul(P.G1_GEN, 0x1D2C3B4A59687766)
    ps = (("P in G1", (g1[0], g1[1])), ("P=(0,1)", (0, 1)), ("P=(1,0)", (1, 0)), ("P=(q-1,q-1)", (Q - 1, Q - 1)))
    return zs, ps, tuple(g2_ref.chain(2))


def _with_z(t, z):
    return (f2_mul(t[0], z), f2_mul(t[1], z), z)


@functools.lru_cache(maxsize=None)
def dbl_cases():
    """T = k Q for k in STEP_KS and two Q of the chain, and one twist point outside the r-torsion (the formulas do not depend on the
    subgroup, and no pairing test can supply it), each written (x Z, y Z, Z) for five Z, for four (x_P, y_P).  No twist point has
    y = 0 (the curve has no 2-torsion), so there is no such case."""
    zs, ps, qs = _step_parts()
    ts = [(f"T={k if k < 4 else 'k255'}*Q{i}", g2.mul(q, k), q) for i, q in enumerate(qs) for k in STEP_KS]
    ts.append(("T outside the r-torsion", outside_point(), qs[0]))
    return tuple(StepCase(f"{tn}, {zn}, {pn}", _with_z(t, z), q, p, t) for tn, t, q in ts for zn, z in zs for pn, p in ps)


@functools.lru_cache(maxsize=None)
def add_cases():
    """as dbl_cases for T = k Q, k in {2, 3, a 255-bit value}.  T = +-Q is outside miller_add_step's contract (1 < k < r - 1, its
    comment says so) and is left out: the chord through T and Q is not defined there."""
    zs, ps, qs = _step_parts()
    ts = [(f"T={k if k < 4 else 'k255'}*Q{i}", g2.mul(q, k), q) for i, q in enumerate(qs) for k in STEP_KS if k != 1]
    return tuple(StepCase(f"{tn}, {zn}, {pn}", _with_z(t, z), q, p, t) for tn, t, q in ts for zn, z in zs for pn, p in ps)


# ---- raw Miller values -----------------------------------------------------------------------------------------------------------
def miller_restated(q2, p1):
    """miller_lane restated: the loop over |x| with the transliterated steps and the oracle's product, in tower order; 1 when either
    point is the identity (None)"""
    if q2 is None or p1 is None:
        return ONE12
    f = OP.ONE
    T = (q2[0], q2[1], (1, 0))
    for bit in range(62, -1, -1):
        T, l = dbl_step(T, p1)
        f = OP.f12_mul(OP.f12_mul(f, f), tower_to_w(embed_line(*l)))
        if (OP.ATE_LOOP >> bit) & 1:
            T, l = add_step(T, q2, p1)
            f = OP.f12_mul(f, tower_to_w(embed_line(*l)))
    return tuple(w_to_tower(f))


@functools.lru_cache(maxsize=None)
def miller_pairs():
    """((name, G1 point | None, G2 point | None), ...): the generators, their negatives, a point at infinity on either side,
    generic points"""
    g1, gq = P.G1_GEN, g2_ref.G
    ch = g2_ref.chain(3)
    a = [P.g1_mul(P.G1_GEN, 0x3C6EF372FE94F82BE54FF53A5F1D36F1 + 977 * i) for i in range(3)]
    return (("(G1, G2)", g1, gq), ("((r-1) G1, G2)", P.g1_mul(g1, R - 1), gq), ("(G1, (r-1) G2)", g1, g2.mul(gq, R - 1)),
            ("(inf, Q)", None, ch[0]), ("(P, inf)", a[0], None), ("generic0", a[0], ch[0]), ("generic1", a[1], ch[1]), ("generic2", a[2], ch[2]))


@functools.lru_cache(maxsize=None)
def miller_expected():
    """miller_restated of every pair of miller_pairs()"""
    return tuple(miller_restated(q2, p1) for _, p1, q2 in miller_pairs())
