"""GT membership stated twice on Python integers over oracle/pairing.py (TEST INFRASTRUCTURE ONLY), and the adversarial elements
the GT tests share.

An element is 12 integers in tower order (tests/test_pairing_cpu.py); arithmetic runs in the oracle's basis through its
tower_to_w / w_to_tower.  GT is the subgroup of order r of Fq12*.

  status_literal   the definition: every coefficient < q, f != 0, f^r = 1.  It cannot tell WHY a non-member fails, so it answers
                   OK / NONCANONICAL / "not a member".
  status_tests     the three tests gm_gt_check runs, Frobenius as f12_pow(f, q): a coefficient >= q; f = 0 or f^(q^4) f != f^(q^2);
                   f^q != f^x.  Tests 2 and 3 give f^(x^4 - x^2 + 1) = f^r = 1 because r = x^4 - x^2 + 1 for BLS12.
"""
import functools
import random

from oracle import pairing as OP
from oracle import pyref as P
from oracle.psnark_ref import G2_GEN
from tests.test_pairing_cpu import tower_to_w, w_to_tower

Q, R = OP.Q, OP.R
X_ABS = OP.ATE_LOOP  # the curve parameter is x = -X_ABS
OK, NONCANONICAL, NOT_IN_SUBGROUP, NOT_CYCLOTOMIC = 0, 2, 4, 5  # GM_PT_* of include/gemini_hip.h
ZERO = [0] * 12


def conj_w(x):
    """x^(q^6): w -> -w"""
    return [(-v) % Q if k & 1 else v for k, v in enumerate(x)]


def status_literal(c) -> int:
    """OK, NONCANONICAL, or NOT_IN_SUBGROUP for every other non-member (the definition does not name a reason)"""
    if any(v >= Q for v in c):
        return NONCANONICAL
    f = tower_to_w(c)
    if f == ZERO:
        return NOT_IN_SUBGROUP
    return OK if OP.f12_pow(f, R) == OP.ONE else NOT_IN_SUBGROUP


def status_tests(c) -> int:
    """the first of gm_gt_check's three tests that fails"""
    if any(v >= Q for v in c):
        return NONCANONICAL
    f = tower_to_w(c)
    f2 = OP.f12_pow(f, Q * Q)
    if f == ZERO or OP.f12_mul(OP.f12_pow(f2, Q * Q), f) != f2:
        return NOT_CYCLOTOMIC
    if OP.f12_pow(f, Q) != conj_w(OP.f12_pow(f, X_ABS)):
        return NOT_IN_SUBGROUP
    return OK


@functools.lru_cache(maxsize=None)
def E():
    """e(G1, G2) as the library defines it (tests/test_gpu_pairing.py), in the oracle's basis"""
    return OP.f12_inv(OP.pairing(G2_GEN, P.G1_GEN))


@functools.lru_cache(maxsize=None)
def cyclotomic_non_member():
    """g = f^((q^6 - 1)(q^2 + 1)) for a random f: in the cyclotomic subgroup, of order dividing r h and (checked in
    tests/test_gt_device_cpu.py) not r"""
    rng = random.Random(0x6779)
    f = [rng.randrange(Q) for _ in range(12)]
    a = OP.f12_mul(conj_w(f), OP.f12_inv(f))
    return OP.f12_mul(OP.f12_pow(a, Q * Q), a)


@functools.lru_cache(maxsize=None)
def adversarial():
    """[(name, 12 integers in tower order, expected status)]: members and non-members of known membership, host-representable
    (every coefficient < q).  Built once; callers do not modify it."""
    rng = random.Random(0x6774636B)
    g = cyclotomic_non_member()
    gr = OP.f12_pow(g, R)  # order divides h = (q^4 - q^2 + 1) / r
    out = []
    for i in range(3):
        out.append((f"random{i}", [rng.randrange(Q) for _ in range(12)], NOT_CYCLOTOMIC))
    for i in range(2):
        m = OP.miller_loop(OP.g2_mul(G2_GEN, rng.randrange(1, R)), P.g1_mul(P.G1_GEN, rng.randrange(1, R)))
        out.append((f"miller{i}", w_to_tower(m), NOT_CYCLOTOMIC))
    out.append(("one", [1] + [0] * 11, OK))
    out.append(("zero", list(ZERO), NOT_CYCLOTOMIC))
    out.append(("minus_one", [Q - 1] + [0] * 11, NOT_CYCLOTOMIC))  # order 2, and q^4 - q^2 + 1 is odd
    out.append(("fq_element", [rng.randrange(2, Q)] + [0] * 11, NOT_CYCLOTOMIC))
    beta = pow(2, (Q - 1) // 3, Q)
    assert beta != 1 and pow(beta, 3, Q) == 1
    out.append(("cube_root_of_unity", [beta] + [0] * 11, NOT_CYCLOTOMIC))
    out.append(("all_q_minus_1", [Q - 1] * 12, NOT_CYCLOTOMIC))
    for i in range(4):
        out.append((f"member{i}", w_to_tower(OP.f12_pow(E(), rng.randrange(1, R))), OK))
    out.append(("cyclotomic_non_member", w_to_tower(g), NOT_IN_SUBGROUP))
    out.append(("order_divides_h", w_to_tower(gr), NOT_IN_SUBGROUP))
    out.append(("member_times_order_h", w_to_tower(OP.f12_mul(OP.f12_pow(E(), rng.randrange(1, R)), gr)), NOT_IN_SUBGROUP))
    return out


def noncanonical_cases():
    """host-only: [(name, 12 integers, NONCANONICAL)]: a member with one coefficient replaced by q, and by 2^384 - 1, in each position"""
    base = w_to_tower(OP.f12_pow(E(), 0x1234567))
    out = []
    for k in range(12):
        for name, v in (("q", Q), ("ones", (1 << 384) - 1)):
            c = list(base)
            c[k] = v
            out.append((f"{name}_at_{k}", c, NONCANONICAL))
    return out
