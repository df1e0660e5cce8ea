"""Reference side of the point-validation tests (test infrastructure, Python integers).

The two endomorphism subgroup tests the device runs (gemini_amd/csrc/points.hip), stated on integers, with their constants DERIVED
here rather than copied, the `[r] P` ladders they are checked against, and the square roots that build adversarial inputs.

  G1   sigma(P) = (beta x, y) == -[x^2] P      |x| = 0xd201000000010000, beta^3 = 1, beta != 1
  G2   psi(Q) = (conj(x) c_x, conj(y) c_y) == [x] Q = -[|x|] Q      c_x = (1 + u)^-((q - 1) / 3), c_y = (1 + u)^-((q - 1) / 2)

The ladders are this module's own: `gemini_amd.g2.mul` reduces its scalar mod r, so `mul(P, r)` is None for EVERY point and says
nothing about membership.  G1 points are (x, y) or None, G2 points ((x0, x1), (y0, y1)) or None.
"""
import functools

from gemini_amd import g2
from gemini_amd.g2 import f2_add, f2_inv, f2_mul, f2_neg, f2_sub

Q = g2.Q
R = g2.R_ORDER
X_ABS = 0xD201000000010000  # the curve parameter is x = -X_ABS
G1_GEN = (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
          0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)
G2_GEN = g2.generator()
assert (X_ABS**4 - X_ABS**2 + 1) == R and ((X_ABS + 1) ** 2 * R) % 3 == 0 and (X_ABS + 1) ** 2 * R // 3 + (-X_ABS) == Q


# ---- G1 on integers ------------------------------------------------------------------------------------------------------
def g1_on_curve(p) -> bool:
    return p is None or (p[1] * p[1] - p[0] ** 3 - 4) % Q == 0


def g1_neg(p):
    return None if p is None else (p[0], (-p[1]) % Q)


def g1_add(p, q):
    """affine chord-and-tangent; complete"""
    if p is None:
        return q
    if q is None:
        return p
    (x1, y1), (x2, y2) = p, q
    if x1 == x2:
        if (y1 + y2) % Q == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, Q) % Q
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, Q) % Q
    x3 = (lam * lam - x1 - x2) % Q
    return (x3, (lam * (x1 - x3) - y1) % Q)


def g1_mul_raw(p, k: int):
    """[k] p for ANY integer k >= 0 -- no reduction mod r"""
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = g1_add(acc, acc)
        if bit == "1":
            acc = g1_add(acc, p)
    return acc


def g1_in_subgroup_ladder(p) -> bool:
    """the truth: [r] P == O"""
    return g1_mul_raw(p, R) is None


def _derive_beta() -> int:
    """The two non-trivial cube roots of unity are g^((q - 1) / 3) and its square for any non-cube g; sigma acts on G1 as one of
    the two roots of lambda^2 + lambda + 1 mod r, which are x^2 - 1 and -x^2.  BETA is the root for which sigma(G) = -[x^2] G."""
    g = 2
    while pow(g, (Q - 1) // 3, Q) == 1:
        g += 1
    b = pow(g, (Q - 1) // 3, Q)
    target = g1_neg(g1_mul_raw(G1_GEN, X_ABS * X_ABS))
    for cand in (b, b * b % Q):
        if (cand * G1_GEN[0] % Q, G1_GEN[1]) == target:
            return cand
    raise AssertionError("no cube root of unity gives sigma(G) = -[x^2] G")


BETA = _derive_beta()


def g1_sigma(p):
    return None if p is None else (BETA * p[0] % Q, p[1])


def g1_in_subgroup_endo(p) -> bool:
    """what k_pt_check<PtG1> computes: sigma(P) == -[x^2] P as two multiplications by |x|; the identity is a member"""
    if p is None:
        return True
    return g1_sigma(p) == g1_neg(g1_mul_raw(g1_mul_raw(p, X_ABS), X_ABS))


def fq_sqrt(a: int):
    """q = 3 mod 4"""
    s = pow(a, (Q + 1) // 4, Q)
    return s if s * s % Q == a % Q else None


def g1_point_from_x(x: int):
    """(x, y) on the curve with the smaller y, or None when x^3 + 4 is no square"""
    y = fq_sqrt((x**3 + 4) % Q)
    return None if y is None else (x, min(y, Q - y))


# ---- G2 on integers ------------------------------------------------------------------------------------------------------
def f2_pow(a, e: int):
    out = (1, 0)
    for bit in bin(e)[2:] if e else "":
        out = f2_mul(out, out)
        if bit == "1":
            out = f2_mul(out, a)
    return out


def f2_conj(a):
    return (a[0], (-a[1]) % Q)


C_X = f2_inv(f2_pow((1, 1), (Q - 1) // 3))
C_Y = f2_inv(f2_pow((1, 1), (Q - 1) // 2))


def g2_on_curve(p) -> bool:
    return g2.on_curve(p)


def g2_neg(p):
    return None if p is None else (p[0], f2_neg(p[1]))


def g2_add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    (x1, y1), (x2, y2) = p, q
    if x1 == x2:
        if f2_add(y1, y2) == (0, 0):
            return None
        xx = f2_mul(x1, x1)
        lam = f2_mul(f2_add(f2_add(xx, xx), xx), f2_inv(f2_add(y1, y1)))
    else:
        lam = f2_mul(f2_sub(y2, y1), f2_inv(f2_sub(x2, x1)))
    x3 = f2_sub(f2_sub(f2_mul(lam, lam), x1), x2)
    return (x3, f2_sub(f2_mul(lam, f2_sub(x1, x3)), y1))


def g2_mul_raw(p, k: int):
    """[k] p for ANY integer k >= 0 -- no reduction mod r (Jacobian inside: one inversion at the end)"""
    if p is None or k == 0:
        return None
    acc = (g2.ONE2, g2.ONE2, g2.ZERO2)
    for bit in bin(k)[2:]:
        acc = g2._jdbl(acc)
        if bit == "1":
            acc = g2._jadd_affine(acc, p)
    X, Y, Z = acc
    if Z == g2.ZERO2:
        return None
    zi = f2_inv(Z)
    zi2 = f2_mul(zi, zi)
    return (f2_mul(X, zi2), f2_mul(Y, f2_mul(zi2, zi)))


def g2_in_subgroup_ladder(p) -> bool:
    return g2_mul_raw(p, R) is None


def g2_psi(p):
    return None if p is None else (f2_mul(f2_conj(p[0]), C_X), f2_mul(f2_conj(p[1]), C_Y))


def g2_in_subgroup_endo(p) -> bool:
    """what k_pt_check<PtG2> computes: psi(Q) == -[|x|] Q; the identity is a member"""
    if p is None:
        return True
    return g2_psi(p) == g2_neg(g2_mul_raw(p, X_ABS))


def f2_sqrt(a):
    """a square root in Fq2 = Fq[u] / (u^2 + 1) or None: with n = a0^2 + a1^2 and s = sqrt(n), x0^2 = (a0 +- s) / 2, x1 = a1 / (2 x0)"""
    if a == (0, 0):
        return (0, 0)
    a0, a1 = a
    if a1 == 0:
        s = fq_sqrt(a0)
        if s is not None:
            return (s, 0)
        s = fq_sqrt((-a0) % Q)
        return None if s is None else (0, s)
    s = fq_sqrt((a0 * a0 + a1 * a1) % Q)
    if s is None:
        return None
    inv2 = pow(2, -1, Q)
    for cand in ((a0 + s) * inv2 % Q, (a0 - s) * inv2 % Q):
        x0 = fq_sqrt(cand)
        if x0:
            r = (x0, a1 * pow(2 * x0, -1, Q) % Q)
            if f2_mul(r, r) == (a0 % Q, a1 % Q):
                return r
    return None


def g2_point_from_x(x):
    """a point of E'(Fq2) with this x, or None"""
    y = f2_sqrt(f2_add(f2_mul(f2_mul(x, x), x), (4, 4)))
    return None if y is None else (x, y)


# ---- the adversarial sets of the tests -----------------------------------------------------------------------------------
G1_ORDER3 = (0, 2)  # on the curve (4 = 0 + 4), order 3: the tangent at x = 0 is horizontal


@functools.lru_cache(maxsize=None)
def g1_random_curve_points(count: int = 3, seed: int = 0x5EED):
    """points of E(Fq) from x = seed, seed + 1, ...: the cofactor is ~2^126, so none is in G1 (checked by the callers' ladder)"""
    out, x = [], seed
    while len(out) < count:
        p = g1_point_from_x(x)
        if p is not None:
            out.append(p)
        x += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def g2_random_curve_points(count: int = 2, seed: int = 0x5EED):
    out, x = [], seed
    while len(out) < count:
        p = g2_point_from_x((x, 1))
        if p is not None:
            out.append(p)
        x += 1
    return tuple(out)


# ---- points as the host records of the C ABI (ark-ff Montgomery limbs, a * 2^384 mod q) -------------------------------------
def fq_limbs(raw: int) -> list:
    """the six u64 limbs of an integer < 2^384, as it stands"""
    assert 0 <= raw < 1 << 384
    return [(raw >> (64 * i)) & (2**64 - 1) for i in range(6)]


def fq_mont(v: int) -> int:
    return (v << 384) % Q


def g1_record(p) -> list:
    """12 limbs; the identity is the all-zero record"""
    return [0] * 12 if p is None else fq_limbs(fq_mont(p[0])) + fq_limbs(fq_mont(p[1]))


def g2_record(p) -> list:
    """24 limbs: x.c0 | x.c1 | y.c0 | y.c1"""
    return [0] * 24 if p is None else sum((fq_limbs(fq_mont(c)) for c in (p[0][0], p[0][1], p[1][0], p[1][1])), [])


def noncanonical(limbs: list, coord: int) -> list:
    """the same record with coordinate `coord` replaced by itself + q: the same residue, limbs >= q (2^384 / q > 9, so it fits)"""
    out = list(limbs)
    v = sum(w << (64 * i) for i, w in enumerate(limbs[6 * coord: 6 * coord + 6])) + Q
    out[6 * coord: 6 * coord + 6] = fq_limbs(v)
    return out
