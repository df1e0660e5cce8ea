"""Reference side of the key-generation tests (test infrastructure, Python integers): the candidate format of
gm_g1_bases_from_candidates / gm_g2_bases_from_candidates, the skip rules in their order, and both cofactor clearings, stated from
their formulas on the curve arithmetic of tests/points_ref.py and gemini_amd/g2.py.

  G1 candidate   48 bytes, one little-endian integer: bits 0 .. 380 x, bits 381 / 382 ignored, bit 383 chooses the larger of y, -y
  G2 candidate   96 bytes, x.c0 | x.c1, each masked the same way; the choice bit is bit 383 of the c1 half
  skipped when   (1) a coordinate >= q   (2) x^3 + 4 (on the twist x^3 + 4 (1 + u)) is no square   (3) the cleared point is the identity
  clearing       G1  P -> [1 - x] P = [|x|] P + P
                 G2  P -> [x^2 - x - 1] P + [x - 1] psi(P) + psi^2([2] P), x = -|x|

Points are those of points_ref: (x, y) / ((x0, x1), (y0, y1)) or None.
"""
from gemini_amd import g2
from gemini_amd.g2 import f2_add, f2_mul, f2_neg
from tests import points_ref as pr

Q = pr.Q
X_ABS = pr.X_ABS
OK, GE_Q, NO_SQUARE, IDENTITY = 0, 1, 2, 3
_X_MASK = (1 << 381) - 1


def parse_coord(b: bytes):
    """48 bytes -> (the low 381 bits, bit 383)"""
    assert len(b) == 48
    v = int.from_bytes(b, "little")
    return v & _X_MASK, bool(v >> 383)


def g1_candidate_bytes(x: int, larger: bool, ignored: int = 0) -> bytes:
    """x < 2^381 (NOT reduced: x >= q is a candidate to skip); ignored: the two bits 381, 382"""
    assert 0 <= x < 1 << 381 and 0 <= ignored < 4
    return (x | (ignored << 381) | (int(larger) << 383)).to_bytes(48, "little")


def g2_candidate_bytes(x, larger: bool, ignored=(0, 0), c0_top: bool = False) -> bytes:
    """c0_top: bit 383 of the c0 half, which nothing reads"""
    assert all(0 <= c < 1 << 381 for c in x)
    return (x[0] | (ignored[0] << 381) | (int(c0_top) << 383)).to_bytes(48, "little") + (x[1] | (ignored[1] << 381) | (int(larger) << 383)).to_bytes(48, "little")


# ---- clearing ------------------------------------------------------------------------------------------------------------
def g1_clear(p):
    """[1 - x] P, x = -X_ABS"""
    return pr.g1_mul_raw(p, 1 + X_ABS)


def g2_clear(p):
    """[x^2 - x - 1] P + [x - 1] psi(P) + psi^2([2] P) with x = -X_ABS: x^2 - x - 1 = X^2 + X - 1 and [x - 1] T = -[X + 1] T"""
    a = pr.g2_mul_raw(p, X_ABS * X_ABS + X_ABS - 1)
    b = pr.g2_neg(pr.g2_mul_raw(pr.g2_psi(p), X_ABS + 1))
    c = pr.g2_psi(pr.g2_psi(pr.g2_add(p, p)))
    return pr.g2_add(pr.g2_add(a, b), c)


# ---- one candidate -------------------------------------------------------------------------------------------------------
def g1_curve_point(cand: bytes):
    """rules 1 and 2 -> (status, the curve point with the chosen y or None): square roots only, no clearing"""
    x, larger = parse_coord(cand)
    if x >= Q:
        return GE_Q, None
    y = pr.fq_sqrt((x**3 + 4) % Q)
    if y is None:
        return NO_SQUARE, None
    lo, hi = min(y, Q - y), max(y, Q - y)
    return OK, (x, hi if larger else lo)


def g2_curve_point(cand: bytes):
    assert len(cand) == 96
    x0, _ = parse_coord(cand[:48])
    x1, larger = parse_coord(cand[48:])
    if x0 >= Q or x1 >= Q:
        return GE_Q, None
    x = (x0, x1)
    y = pr.f2_sqrt(f2_add(f2_mul(f2_mul(x, x), x), (4, 4)))
    if y is None:
        return NO_SQUARE, None
    ny = f2_neg(y)
    hi, lo = (y, ny) if g2._f2_gt(y, ny) else (ny, y)  # ark-ff's order of Fq2: c1 first, then c0
    return OK, (x, hi if larger else lo)


def g1_from_candidate(cand: bytes):
    """-> (status, the cleared point or None), the skip rules in their order"""
    st, p = g1_curve_point(cand)
    if st != OK:
        return st, None
    c = g1_clear(p)
    return (IDENTITY, None) if c is None else (OK, c)


def g2_from_candidate(cand: bytes):
    st, p = g2_curve_point(cand)
    if st != OK:
        return st, None
    c = g2_clear(p)
    return (IDENTITY, None) if c is None else (OK, c)


# ---- a stream of candidates ------------------------------------------------------------------------------------------------
def from_candidates(group: int, cands: bytes, n: int):
    """what gm_g{group}_bases_from_candidates returns: (the first n survivors or None on a shortfall, used, found)"""
    size, one = (48, g1_from_candidate) if group == 1 else (96, g2_from_candidate)
    m = len(cands) // size
    out = []
    if n == 0:
        return out, 0, 0
    for i in range(m):
        st, p = one(cands[size * i: size * (i + 1)])
        if st == OK:
            out.append(p)
            if len(out) == n:
                return out, i + 1, n
    return None, m, len(out)


def accepted(group: int, cands: bytes):
    """indices of the candidates that pass rules 1 and 2 (square roots only: rule 3 needs the clearing, and no candidate drawn at
    random meets it -- the points of small order are a handful)"""
    size, one = (48, g1_curve_point) if group == 1 else (96, g2_curve_point)
    return [i for i in range(len(cands) // size) if one(cands[size * i: size * (i + 1)])[0] == OK]
