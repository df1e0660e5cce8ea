"""CPU-only G2 checks: the pins of the reference side (tests/g2_ref.py against gemini_amd/g2.py, two independent statements of the
group law) and the host arithmetic of the library behind gm_g2_sum (host_field.hpp: Fq2, Jacobian G2), which the G2 MSM uses for
its window Horner and normalisation.  No device compute happens here."""
import os

import numpy as np
import pytest

from gemini_amd import g2
from tests import g2_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    if not os.path.exists(os.path.join(ROOT, "gemini_amd", "libgemini_hip.so")):
        ge.build()
    from gemini_amd import capi

    return capi.load()


def test_generator_on_curve():
    assert g2.on_curve(g2_ref.G)
    assert g2.on_curve(g2_ref.add(g2_ref.G, g2_ref.G))


def test_order_minus_one_is_negation():
    assert g2.mul(g2_ref.G, g2.R_ORDER - 1) == g2_ref.neg(g2_ref.G)


def test_affine_chain_meets_scalar_multiplication():
    """2^14 - 1 affine additions against one Jacobian double-and-add"""
    n = 1 << 14
    pts = g2_ref.chain(n + 3)  # the length the GPU tests share
    assert pts[n - 1] == g2.mul(g2_ref.G, g2_ref.B0 + (n - 1) * g2_ref.D)
    assert pts[n - 1] == g2.mul(g2_ref.G, g2_ref.chain_log(n - 1))


def test_affine_and_jacobian_statements_agree():
    P = g2.mul(g2_ref.G, 0xDEADBEEF)
    assert g2_ref.add(P, P) == g2.mul(P, 2)
    assert g2_ref.add(P, g2_ref.neg(P)) is None and g2.mul(P, g2.R_ORDER) is None
    assert g2_ref.add(P, None) == P and g2_ref.add(None, P) == P
    assert g2_ref.add(g2.mul(P, 2), P) == g2.mul(P, 3)


def _scaled(p, z):
    """an un-normalised Jacobian representative (X z^2, Y z^3, z) of the affine point p, as 36 Montgomery limbs"""
    from gemini_amd.g2msm import _fq_limbs

    zz = g2.f2_mul(z, z)
    X, Y = g2.f2_mul(p[0], zz), g2.f2_mul(p[1], g2.f2_mul(zz, z))
    return np.array(sum((_fq_limbs(c) for v in (X, Y, z) for c in v), []), dtype=np.uint64)


def _identity_unnormalised():
    from gemini_amd.g2msm import _fq_limbs

    return np.array(sum((_fq_limbs(c) for c in (5, 7, 11, 13, 0, 0)), []), dtype=np.uint64)


def _g2_sum_cases():
    P, Qp, S = (g2.mul(g2_ref.G, k) for k in (3, 0x1234567, g2.R_ORDER - 5))
    z1, z2 = (0x1111, 0x2222), (0x33333, 0x5)
    return {
        0: [],
        1: [P],
        2: [P, g2_ref.neg(P)],
        7: [None, P, Qp, P, g2_ref.neg(Qp), None, S],  # the identity first and inside, P twice, Q and -Q
    }, (z1, z2)


@pytest.mark.parametrize("k", [0, 1, 2, 7])
def test_g2_sum_host(lib, k):
    """gm_g2_sum is pure host code; fails on a library without the symbol"""
    from gemini_amd.g2msm import g2_jac_to_point, g2_point_to_jac, g2_sum

    cases, zs = _g2_sum_cases()
    pts = cases[k]
    jac = np.zeros((len(pts), 36), dtype=np.uint64)
    for i, p in enumerate(pts):
        jac[i] = _identity_unnormalised() if p is None else (_scaled(p, zs[i % 2]) if i % 3 != 1 else g2_point_to_jac(p))
    got = g2_sum(jac)
    exp = None
    for p in pts:
        exp = g2_ref.add(exp, p)
    assert g2_jac_to_point(got) == exp
    assert (got == g2_point_to_jac(exp)).all()  # normalised: Z = 1, or (1, 1, 0) for the identity
    if k == 1:  # a doubling through the general addition
        assert g2_jac_to_point(g2_sum(np.stack([jac[0], g2_point_to_jac(pts[0])]))) == g2.mul(pts[0], 2)
