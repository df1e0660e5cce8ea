"""Reference side of the G2 tests (test infrastructure, Python integers).

An AFFINE chord-and-tangent statement of the group law on y^2 = x^3 + 4 (1 + u) over Fq2 = Fq[u] / (u^2 + 1) -- deliberately not
the Jacobian formulas of gemini_amd/g2.py, so the two are independent statements (tests/test_g2_ref_cpu.py pins them against each
other) --, a naive MSM, the chain of points b0 G, (b0 + d) G, (b0 + 2d) G, ... whose discrete logs are known, and a restatement
of herring's TimeProver over G2Module (src/herring/time_prover.rs:72-137, module.rs:104-125).

A point is ((x0, x1), (y0, y1)) or None, as in gemini_amd/g2.py.
"""
import functools
import os
import re

from gemini_amd import g2

Q = g2.Q
R = g2.R_ORDER
G = g2.generator()
B0 = 0x1F3A9C5D77E2B4A6908D1C3E5F7A9B2D4C6E8F0A1B3D5F79
D = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA5


def _mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def _sub(a, b):
    return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)


def _inv(a):
    d = pow(a[0] * a[0] + a[1] * a[1], -1, Q)
    return (a[0] * d % Q, -a[1] * d % Q)


def neg(p):
    return None if p is None else (p[0], ((-p[1][0]) % Q, (-p[1][1]) % Q))


def add(p, q):
    """p + q by the chord (p != +-q) or the tangent (p == q) through the affine points"""
    if p is None:
        return q
    if q is None:
        return p
    (x1, y1), (x2, y2) = p, q
    if x1 == x2:
        if y1 != y2 or y1 == (0, 0):
            return None
        xx = _mul(x1, x1)
        lam = _mul(((3 * xx[0]) % Q, (3 * xx[1]) % Q), _inv(((2 * y1[0]) % Q, (2 * y1[1]) % Q)))
    else:
        lam = _mul(_sub(y2, y1), _inv(_sub(x2, x1)))
    x3 = _sub(_sub(_mul(lam, lam), x1), x2)
    return (x3, _sub(_mul(lam, _sub(x1, x3)), y1))


def msm_naive(points, scalars):
    """sum_i s_i P_i over the shorter input (zip): one g2.mul per pair, summed by affine additions"""
    acc = None
    for p, s in zip(points, scalars):
        acc = add(acc, g2.mul(p, s))
    return acc


@functools.lru_cache(maxsize=None)
def chain(n: int):
    """[(B0 + i D) G for i < n] by n - 1 affine additions"""
    out = [g2.mul(G, B0)]
    step = g2.mul(G, D)
    for _ in range(n - 1):
        out.append(add(out[-1], step))
    return out


def chain_log(i: int) -> int:
    return (B0 + i * D) % R


def ceil_log2(n: int) -> int:
    return (n - 1).bit_length()


class HerringG2TimeProver:
    """TimeProver<G2Module>: f in Fr (ints), g in G2; the twist rides on the f side (time_prover.rs:83-88)"""

    def __init__(self, f, g, twist):
        self.f = [x % R for x in f]
        self.g = list(g)
        self.twist = twist % R
        self.round = 0
        self.tot_rounds = ceil_log2(min(len(self.f), len(self.g)))  # :36-39

    def fold(self, r):  # :83-88, split_fold :72-76 with unwrap_or(zero) for an odd tail
        rt = r * self.twist % R
        self.f = [(self.f[i] + (self.f[i + 1] if i + 1 < len(self.f) else 0) * rt) % R for i in range(0, len(self.f), 2)]
        self.g = [add(self.g[i], g2.mul(self.g[i + 1], r) if i + 1 < len(self.g) else None) for i in range(0, len(self.g), 2)]
        self.twist = self.twist * self.twist % R

    def next_message(self, vm=None):  # :91-123; G2Module::ip(f, g) = msm(g, f)
        if vm is not None:
            self.fold(vm)
        if self.round == self.tot_rounds:
            return None
        fe, fo = self.f[0::2], self.f[1::2]
        ge, go = self.g[0::2], self.g[1::2]
        a = msm_naive(ge, fe)
        b = add(msm_naive(go, fe), msm_naive(ge, fo))
        self.round += 1
        return (a, b)

    def final_foldings(self):  # :135-137
        return (self.f[0], self.g[0]) if self.round == self.tot_rounds else None


def source_thresholds() -> dict:
    """The size thresholds of the G2 MSM, read from the sources: the window steps of g2msm.hip (G2_C*_MIN_N), the length above which
    a call is cut into pieces (G2_CALL_MAX_N, lowered by the environment variable GM_G2_CALL_MAX_N) and the step from
    the flat to the block sort in msm_sort_plain (msm.hip: n W <= 2^21 entries and W 2^(c-1) <= 2^18 buckets take the flat one)."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gemini_amd", "csrc")
    src = open(os.path.join(csrc, "g2msm.hip")).read()
    out = {}
    for c in (8, 12, 16):
        m = re.search(r"constexpr\s+size_t\s+G2_C%d_MIN_N\s*=\s*([^;]+);" % c, src)
        assert m, f"G2_C{c}_MIN_N not found in g2msm.hip"
        out[c] = int(eval(re.sub(r"\(size_t\)", "", m.group(1)), {"__builtins__": {}}))
    assert re.search(r"return n >= G2_C16_MIN_N \? 16 : n >= G2_C12_MIN_N \? 12 : n >= G2_C8_MIN_N \? 8 : 4;", src), "g2_choose_window changed"
    m = re.search(r"constexpr\s+size_t\s+G2_CALL_MAX_N\s*=\s*\(size_t\)1 << (\d+);", src)
    assert m, "G2_CALL_MAX_N not found in g2msm.hip"
    out["cut"] = 1 << int(m.group(1))
    assert 'getenv("GM_G2_CALL_MAX_N")' in src, "the override of the call cut is gone from g2msm.hip"
    msm = open(os.path.join(csrc, "msm.hip")).read()
    body = msm[msm.index("int msm_sort_plain("):]
    m = re.search(r"if \(N <= \(\(uint64_t\)1 << (\d+)\) && nbuckets <= \(\(size_t\)1 << (\d+)\)\) \{", body)
    assert m, "the flat / block sort rule of msm_sort_plain not found in msm.hip"
    out["flat_entries"], out["flat_buckets"] = 1 << int(m.group(1)), 1 << int(m.group(2))
    return out


def window_of(n: int, th: dict) -> int:
    return 16 if n >= th[16] else 12 if n >= th[12] else 8 if n >= th[8] else 4


def flat_sort(n: int, th: dict) -> bool:
    c = window_of(n, th)
    W = (256 + c - 1) // c
    return n * W <= th["flat_entries"] and (W << (c - 1)) <= th["flat_buckets"]
