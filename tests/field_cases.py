"""The operands and the integer references of tests/test_gpu_field_ops.py and tests/test_gpu_group_ops.py.

Everything here is Python integers: `pow`, `%`, and the curve laws of oracle/pyref.py (G1, affine chord and tangent) and
tests/g2_ref.py (G2, the same over Fq2).  No host C++ arithmetic and no device function is ever the reference.

Device form.  A field element at rest on the device is the canonical residue a * 2^390 mod q; the lists below hold those residues
(what the 12 words of a record spell), so "1" is the residue 1 -- the field element 2^-390 -- and `ONE` is the field's one.  The
Montgomery product of two residues is mm(a, b) = a b 2^-390 mod q.  Loose values (field30.cuh) are integers below 2^386 standing for
their residue.

The lists are built once at import, deterministically, named, and never modified (tuples)."""
import random

from oracle import pyref
from tests import g2_ref

Q = pyref.Q_MOD
R390 = 1 << 390
RI = pow(R390, -1, Q)
ONE = R390 % Q                 # the field's one
CIN = (1 << 396) % Q           # fqe_import's constant: ark-ff form a 2^384 -> a 2^390
COUT = (1 << 384) % Q          # fqe_export's
MASK30 = (1 << 30) - 1
LOOSE_LIMIT = 1 << 386
QINV390 = pow(Q, -1, R390)
assert Q % 4 == 3


def mm(a: int, b: int) -> int:
    return a * b * RI % Q


def mont_quotient(a: int, b: int) -> int:
    """the exact integer the lazy radix-2^30 product leaves: (ab + (-ab q^-1 mod 2^390) q) >> 390 (gen_field_mul30.selftest_loose)"""
    ab = a * b
    return (ab + (-ab * QINV390 % R390) * Q) >> 390


def dev(v: int) -> int:
    """the device residue of the field element v"""
    return v * R390 % Q


def val(d: int) -> int:
    """the field element of a device residue (or of a loose representative)"""
    return d * RI % Q


def _unique(named, limit: int):
    """the first name of every value, in order (1 is also 2^(30*0))"""
    seen, out = set(), []
    for n, v in named:
        assert 0 <= v < limit, n
        if v not in seen:
            seen.add(v)
            out.append((n, v))
    return tuple(out)


# ---- Fq: canonical residues --------------------------------------------------------------------------------------------------------
def _fq_values():
    rnd = random.Random(0xF9)
    q11 = Q >> 352
    out = [("0", 0), ("1", 1), ("2", 2), ("q-1", Q - 1), ("q-2", Q - 2), ("(q-1)/2", (Q - 1) // 2), ("(q+1)/2", (Q + 1) // 2),
           ("one", ONE), ("CIN", CIN), ("COUT", COUT), ("2^380-1", (1 << 380) - 1),
           ("limbs30 all ones below q's top limb", ((Q >> 360) << 360) - 1), ("2^360-1", (1 << 360) - 1),
           ("words32 all ones below q's top word", (q11 << 352) - 1), ("2^352-1", (1 << 352) - 1),
           ("q's top word alone", q11 << 352)]
    for i in range(13):
        out.append((f"2^(30*{i})", 1 << (30 * i)))
    for i in range(12):
        out.append((f"limb30 {i} all ones", MASK30 << (30 * i)))
    out.append(("limb30 12 at q's top limb - 1", ((Q >> 360) - 1) << 360))
    for i in range(12):
        out.append((f"2^(32*{i})", 1 << (32 * i)))
    for i in range(11):
        out.append((f"word32 {i} all ones", 0xFFFFFFFF << (32 * i)))
    for k in range(8):
        out.append((f"q-1-rand200[{k}]", Q - 1 - rnd.getrandbits(200)))
    for k in range(6):
        out.append((f"random[{k}]", rnd.randrange(Q)))
    return _unique(out, Q)


FQ = _fq_values()
FQ_VALUES = tuple(v for _, v in FQ)
FQ_NAME = {v: n for n, v in FQ}


def _fq_pairs():
    """(name, a, b) for the binary ops: the whole list against itself, pairs solved for a small canonical product (the raw product
    of the multiplier is then the result or the result + q: the conditional subtraction's edge, gen_field_mul30.selftest's recipe),
    pairs with product 0 / 1 / q - 1 / one, and a - b with a borrow out of every word"""
    rnd = random.Random(0xFA)
    out = [(f"{na} . {nb}", a, b) for na, a in FQ for nb, b in FQ]
    for k in range(300):
        a = rnd.randrange(1, Q)
        t = rnd.randrange(0, Q >> 9)
        out.append((f"solved small[{k}]", a, t * pow(a, -1, Q) * R390 % Q))
    for k in range(8):
        a = rnd.randrange(1, Q)
        for t, nt in ((0, "0"), (1, "1"), (Q - 1, "q-1"), (ONE, "one")):
            out.append((f"product {nt}[{k}]", a, t * pow(a, -1, Q) * R390 % Q))
    words_q = [(Q >> (32 * i)) & 0xFFFFFFFF for i in range(12)]
    out.append(("borrow every word: (q-1 minus 1 per word) - (q-1)", sum((w - 1 - (i == 0)) << (32 * i) for i, w in enumerate(words_q)), Q - 1))
    for k in range(8):
        bw = [rnd.randrange(1, 1 << 32) for _ in range(11)] + [rnd.randrange(1, words_q[11])]
        aw = [rnd.randrange(0, w) for w in bw]
        a, b = (sum(w << (32 * i) for i, w in enumerate(ws)) for ws in (aw, bw))
        assert a < b < Q and all(x < y for x, y in zip(aw, bw))
        out.append((f"borrow every word[{k}]", a, b))
    return tuple(out)


FQ_PAIRS = _fq_pairs()

# pt_raw_ge_q: the ONLY function that takes words >= q
RAW_GE_Q = tuple([("q-1", Q - 1), ("q", Q), ("q+1", Q + 1), ("2^384-1", (1 << 384) - 1), ("0", 0)]
                 + [(f"q+2^(32*{k})", Q + (1 << (32 * k))) for k in range(12)] + [(f"q-2^(32*{k})", Q - (1 << (32 * k))) for k in range(12)]
                 + list(FQ))
assert all(0 <= v < 1 << 384 for _, v in RAW_GE_Q)


def fq_inv_expected(a: int) -> int:
    """fq_inv: a^(q - 2) in the field, i.e. the inverse, and 0 for 0 (Fermat's ladder multiplies 0 in at its first step)"""
    return dev(pow(val(a), Q - 2, Q))


# ---- Fq30: loose 13-limb values -----------------------------------------------------------------------------------------------------
def _loose_values():
    rnd = random.Random(0xFB)
    out = [("0", 0), ("2^386-1", LOOSE_LIMIT - 1), ("10q", 10 * Q), ("10q-1", 10 * Q - 1), ("top limb at its 26-bit maximum", ((1 << 26) - 1) << 360),
           ("top limb at its maximum, low limbs random", (((1 << 26) - 1) << 360) | rnd.getrandbits(360)), ("q", Q), ("q-1", Q - 1), ("q+1", Q + 1)]
    for nr, r in (("0", 0), ("1", 1), ("q-1", Q - 1), ("one", ONE), ("random a", rnd.randrange(Q)), ("random b", rnd.randrange(Q))):
        j = 1
        while r + j * Q < LOOSE_LIMIT:
            if j in (1, 2, 6, 7, 15, 16, 31, 32) or r + (j + 1) * Q >= LOOSE_LIMIT:
                out.append((f"{nr} + {j} q", r + j * Q))
            j += 1
    for i in range(13):
        out.append((f"2^(30*{i})", 1 << (30 * i)))
        out.append((f"limb {i} all ones", (MASK30 if i < 12 else (1 << 26) - 1) << (30 * i)))
    for k in range(8):
        out.append((f"2^386-1-rand300[{k}]", LOOSE_LIMIT - 1 - rnd.getrandbits(300)))
    for k in range(6):
        out.append((f"random386[{k}]", rnd.getrandbits(386)))
    return _unique(out, LOOSE_LIMIT)


LOOSE = _loose_values()
LOOSE_PAIRS = tuple((f"{na} . {nb}", a, b) for na, a in LOOSE for nb, b in LOOSE)
# what fq30_loose_to_canonical hands fq30_canonical_tail: quotient(v, one) <= q + floor(v one / 2^390), v < 2^386
TAIL_MAX = Q + ((LOOSE_LIMIT - 1) * ONE >> 390)
TAIL = (("0", 0), ("1", 1), ("q-1", Q - 1), ("q", Q), ("q+1", Q + 1), ("the largest value loose_to_canonical can hand it", TAIL_MAX),
        ("the quotient of (2^386-1) . one", mont_quotient(LOOSE_LIMIT - 1, ONE)), ("q + 2^360", Q + (1 << 360)), ("q with limb 0 zeroed", Q - (Q & MASK30)),
        ("q + 2^30 - q_0", Q + (1 << 30) - (Q & MASK30)))
assert all(v < 2 * Q for _, v in TAIL) and TAIL_MAX < Q + Q // 16 + 1


# ---- Fq2 = Fq[u] / (u^2 + 1), device residues (c0, c1) -------------------------------------------------------------------------------
def fq2_mul(a, b):
    return ((mm(a[0], b[0]) - mm(a[1], b[1])) % Q, (mm(a[0], b[1]) + mm(a[1], b[0])) % Q)


def fq2_inv(a):
    """on field elements by g2_ref's statement, back in device form"""
    i0, i1 = g2_ref._inv((val(a[0]), val(a[1])))
    return (dev(i0), dev(i1))


def _fq2_values():
    rnd = random.Random(0xFC)
    a = (rnd.randrange(1, Q), rnd.randrange(1, Q))
    t = rnd.randrange(2, Q)
    d = pow(1 + t * t, -1, Q)
    out = [("0", (0, 0)), ("c1 = 0", (a[0], 0)), ("c0 = 0 (its square is real)", (0, a[1])), ("a", a), ("conj a", (a[0], Q - a[1])),
           ("u", (0, ONE)), ("u + 1", (ONE, ONE)), ("one", (ONE, 0)), ("-one", (Q - ONE, 0)), ("c0 = c1 (its square is imaginary)", (a[0], a[0])),
           ("norm 1", (dev((1 - t * t) * d % Q), dev(2 * t * d % Q))), ("(q-1, q-1)", (Q - 1, Q - 1)), ("(1, q-1)", (1, Q - 1))]
    fixed = rnd.randrange(1, Q)
    for n, v in FQ:
        out.append((f"c0 = {n}", (v, fixed)))
        out.append((f"c1 = {n}", (fixed, v)))
    return tuple(out)


FQ2 = _fq2_values()
_FQ2_CORE = FQ2[:13] + tuple(x for x in FQ2[13:] if any(k in x[0] for k in ("= q-1", "= 0", "= 1", "= (q+1)/2", "= 2^380-1")))
FQ2_PAIRS = tuple([(f"{na} . {nb}", a, b) for na, a in _FQ2_CORE for nb, b in _FQ2_CORE]
                  + [(f"{FQ2[i][0]} . {FQ2[(7 * i + 3) % len(FQ2)][0]}", FQ2[i][1], FQ2[(7 * i + 3) % len(FQ2)][1]) for i in range(len(FQ2))])


# ---- G1 points and their XYZZ representations -------------------------------------------------------------------------------------------
G1_SCALARS = (1, 2, 3, 5, 7, 11, 0x1234567, 0xDEADBEEFCAFE, pyref.R_MOD - 1, pyref.R_MOD - 2, (pyref.R_MOD + 1) // 2,
              0x0F1E2D3C4B5A69788796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF)
G1_POINTS = tuple(pyref.g1_mul(pyref.G1_GEN, k) for k in G1_SCALARS)
assert all(P is not None and P[1] != 0 and pyref.g1_is_on_curve(P) for P in G1_POINTS)
# A point with y = 0 would have order 2.  #E(Fq) = h r with h = (x - 1)^2 / 3, x = -0xd201000000010000: both factors are odd, so the
# curve has no such point and no y = 0 input is built (the twist's order h2 r is odd as well: h2 = (x^8 - 4 x^7 + ... + 13) / 9, x even).
assert ((0xD201000000010000 + 1) ** 2 // 3) % 2 == 1 and pyref.R_MOD % 2 == 1


def g1_xyzz(P, lam: int):
    """device residues (X, Y, ZZ, ZZZ) of the affine point P in the representation ZZ = lam^2, ZZZ = lam^3; None is the identity"""
    if P is None:
        return (0, 0, 0, 0)
    l2, l3 = lam * lam % Q, lam * lam * lam % Q
    return (dev(P[0] * l2 % Q), dev(P[1] * l3 % Q), dev(l2), dev(l3))


def g1_affine_dev(P):
    return (dev(P[0]), dev(P[1]))


def g1_point_of(rec):
    """(X, Y, ZZ, ZZZ) device residues or loose values -> the affine point on field elements; ZZ == 0 EXACTLY is the identity.
    Asserts ZZ^3 == ZZZ^2 in the field."""
    X, Y, ZZ, ZZZ = rec
    if ZZ == 0:
        return None
    x, y, zz, zzz = val(X), val(Y), val(ZZ), val(ZZZ)
    assert zz != 0, "ZZ is a non-zero multiple of q: neither the identity's encoding nor a point"
    assert pow(zz, 3, Q) == zzz * zzz % Q, "ZZ^3 != ZZZ^2"
    return (x * pow(zz, -1, Q) % Q, y * pow(zzz, -1, Q) % Q)


# ---- G2 -------------------------------------------------------------------------------------------------------------------------------
G2_SCALARS = (1, 2, 3, 5, 0x1234567, pyref.R_MOD - 1, pyref.R_MOD - 2, 0x0F1E2D3C4B5A69788796A5B4C3D2E1F00112233445566778899AABBCCDDEEFF)
G2_POINTS = tuple(g2_ref.g2.mul(g2_ref.G, k) for k in G2_SCALARS)


def f2v(a):
    return (val(a[0]), val(a[1]))


def f2d(a):
    return (dev(a[0]), dev(a[1]))


def g2_xyzz(P, lam):
    """lam in Fq2 (field elements)"""
    if P is None:
        return ((0, 0),) * 4
    l2 = g2_ref._mul(lam, lam)
    l3 = g2_ref._mul(l2, lam)
    return (f2d(g2_ref._mul(P[0], l2)), f2d(g2_ref._mul(P[1], l3)), f2d(l2), f2d(l3))


def g2_point_of(rec):
    X, Y, ZZ, ZZZ = rec
    if ZZ == (0, 0):
        return None
    x, y, zz, zzz = f2v(X), f2v(Y), f2v(ZZ), f2v(ZZZ)
    assert g2_ref._mul(g2_ref._mul(zz, zz), zz) == g2_ref._mul(zzz, zzz), "ZZ^3 != ZZZ^2"
    return (g2_ref._mul(x, g2_ref._inv(zz)), g2_ref._mul(y, g2_ref._inv(zzz)))
