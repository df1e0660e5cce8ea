"""GT on the host (no GPU): gm_gt_mul / gm_gt_pow / gm_gt_one / gm_gt_final_exp against oracle/pairing.py.

The library's Fq12 is the tower Fq12 = Fq6[w] / (w^2 - v), Fq6 = Fq2[v] / (v^3 - (1 + u)), Fq2 = Fq[u] / (u^2 + 1), twelve Fq values in
the order c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1: index 6 h + 2 j + k is the coefficient of u^k v^j w^h.  The oracle's is
Fq[w] / (w^12 - 2 w^6 + 2) with u = w^6 - 1 and v = w^2.  The Fq2 coefficient a + b u at v^j w^h is therefore
a + b (w^6 - 1) times w^(2 j + h): (a - b) at w^(2 j + h) and b at w^(2 j + h + 6).  `tower_to_w` states this map, `w_to_tower` its
inverse; tests/test_gpu_pairing.py imports both.
"""
import random

import numpy as np
import pytest

from gemini_amd import capi
from gemini_amd import pairing as gp
from oracle import pairing as OP
from oracle import pyref as P
from oracle.psnark_ref import G2_GEN, g2_mul

Q = OP.Q


def tower_to_w(c):
    out = [0] * 12
    for h in range(2):
        for j in range(3):
            a, b = c[6 * h + 2 * j], c[6 * h + 2 * j + 1]
            out[2 * j + h] = (a - b) % Q
            out[2 * j + h + 6] = b % Q
    return out


def w_to_tower(x):
    c = [0] * 12
    for h in range(2):
        for j in range(3):
            b = x[2 * j + h + 6]
            c[6 * h + 2 * j] = (x[2 * j + h] + b) % Q
            c[6 * h + 2 * j + 1] = b % Q
    return c


def gt_of_w(x) -> np.ndarray:
    """oracle element -> (72,) limbs"""
    return gp.gt_from_ints(w_to_tower(x))


def w_of_gt(gt):
    """(72,) limbs -> oracle element"""
    return tower_to_w(gp.gt_to_ints(gt))


@pytest.fixture(scope="module")
def elements():
    rng = random.Random(0x6774)
    return [[rng.randrange(Q) for _ in range(12)] for _ in range(10)]


def test_exports_and_abi():
    lib = capi.load()
    for s in ("gm_pairing_multi", "gm_pairing_multi_h", "gm_gt_mul", "gm_gt_pow", "gm_gt_one", "gm_gt_final_exp", "gm_hp_new", "gm_hp_round",
              "gm_hp_fold", "gm_hp_rounds", "gm_hp_final", "gm_hp_free"):
        assert hasattr(lib, s), s
        assert s in capi.SYMBOLS
    assert lib.gm_abi_version() == 1
    import gemini_amd
    from gemini_amd import herring

    assert gemini_amd.multi_pairing is gp.multi_pairing and hasattr(herring, "PModuleTimeProver")


def test_basis_map_round_trips(elements):
    for c in elements:
        assert w_to_tower(tower_to_w(c)) == c
        assert tower_to_w(w_to_tower(c)) == c  # the same list read as an oracle element
    assert tower_to_w([1] + [0] * 11) == OP.ONE
    # u^2 = -1, v^3 = 1 + u, w^2 = v in the oracle's basis
    u, v, w = ([0] * 12 for _ in range(3))
    u[1], v[2], w[6] = 1, 1, 1
    U, V, W = tower_to_w(u), tower_to_w(v), tower_to_w(w)
    assert OP.f12_mul(U, U) == OP.f12(-1)
    assert OP.f12_mul(V, OP.f12_mul(V, V)) == OP.f12_add(OP.ONE, U)
    assert OP.f12_mul(W, W) == V


def test_limb_conversion_round_trips(elements):
    for c in elements:
        assert gp.gt_to_ints(gp.gt_from_ints(c)) == c


def test_gt_one():
    assert w_of_gt(gp.gt_one()) == OP.ONE


def test_gt_mul(elements):
    for a, b in zip(elements, elements[1:] + elements[:1]):
        assert w_of_gt(gp.gt_mul(gt_of_w(a), gt_of_w(b))) == OP.f12_mul(a, b)
    assert w_of_gt(gp.gt_mul(gt_of_w(elements[0]), gp.gt_one())) == elements[0]


def test_gt_pow(elements):
    rng = random.Random(0x706F77)
    for a in elements:
        e = rng.randrange(1 << 256)
        assert w_of_gt(gp.gt_pow(gt_of_w(a), e)) == OP.f12_pow(a, e)
    assert w_of_gt(gp.gt_pow(gt_of_w(elements[0]), 0)) == OP.ONE
    assert w_of_gt(gp.gt_pow(gt_of_w(elements[1]), 1)) == elements[1]
    assert w_of_gt(gp.gt_pow(gt_of_w(elements[2]), (1 << 256) - 1)) == OP.f12_pow(elements[2], (1 << 256) - 1)


def test_final_exponentiation():
    """the host final exponentiation on the unconjugated product of two oracle Miller loops, and on a random element"""
    rng = random.Random(0x66696E)
    f = OP.ONE
    for _ in range(2):
        p1 = P.g1_mul(P.G1_GEN, rng.randrange(1, OP.R))
        q2 = g2_mul(G2_GEN, rng.randrange(1, OP.R))
        f = OP.f12_mul(f, OP.miller_loop(q2, p1))
    exp = OP.final_exponentiation(f)
    assert exp != OP.ONE and OP.f12_pow(exp, OP.R) == OP.ONE
    assert w_of_gt(gp.gt_final_exp(gt_of_w(f))) == exp
    x = [rng.randrange(Q) for _ in range(12)]
    assert w_of_gt(gp.gt_final_exp(gt_of_w(x))) == OP.final_exponentiation(x)
    assert w_of_gt(gp.gt_final_exp(gp.gt_one())) == OP.ONE
