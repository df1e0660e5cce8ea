"""GT on the device, the parts that need no GPU: the two statements of membership of tests/gt_check_ref.py agree on the adversarial
list, the exponent identity behind k_gt_final_exp holds on integers, the generator reproduces the committed constants, and the
exports are there.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from gemini_amd import capi
from oracle import pairing as OP
from tests import gt_check_ref as ref
from tests.test_pairing_cpu import tower_to_w

Q, R = OP.Q, OP.R
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gemini_amd", "csrc")
NAMES = ("gm_gt_final_exp_many", "gm_pairing_each", "gm_pairing_each_h", "gm_gt_check", "gm_hgt_check", "gm_ipa_check_gt", "gm_debug_gt_op",
         "gm_debug_gt_op2", "gm_debug_miller_step", "gm_debug_miller_each")


def test_chain_identity_on_integers():
    """(q^12 - 1) / r = (q^6 - 1)(q^2 + 1) h with h = ((x - 1)^2 / 3)(x + q)(x^2 + q^2 - 1) + 1 exactly: the chain of k_gt_final_exp
    raises to the library's exponent, not to its triple"""
    x = -ref.X_ABS
    assert R == x**4 - x**2 + 1
    assert (Q**4 - Q**2 + 1) % R == 0
    h = (Q**4 - Q**2 + 1) // R
    assert (x - 1) ** 2 % 3 == 0 and x % 3 == 1
    assert h == ((x - 1) ** 2 // 3) * (x + Q) * (x * x + Q * Q - 1) + 1
    assert OP.FINAL_EXP == (Q**6 - 1) * (Q**2 + 1) * h
    e3 = (ref.X_ABS + 1) // 3
    assert 3 * e3 == ref.X_ABS + 1 and e3 == 0x460055555555AAAB and e3.bit_length() == 63 and bin(e3).count("1") == 28
    assert (x - 1) ** 2 // 3 == e3 * (ref.X_ABS + 1)
    assert ref.X_ABS.bit_length() == 64 and bin(ref.X_ABS).count("1") == 6  # 63 squarings, 5 products


def test_the_two_statements_agree():
    """on every element of the list: the literal f^r = 1 and the three tests accept the same elements, and the tests name the
    reason the list expects"""
    for name, c, want in ref.adversarial():
        lit, tst = ref.status_literal(c), ref.status_tests(c)
        assert (lit == ref.OK) == (tst == ref.OK), name
        assert tst == want, (name, tst, want)
    for name, c, want in ref.noncanonical_cases()[::5]:
        assert ref.status_literal(c) == ref.status_tests(c) == want == ref.NONCANONICAL, name


def test_cyclotomic_non_member_is_what_it_says():
    g = ref.cyclotomic_non_member()
    g2 = OP.f12_pow(g, Q * Q)
    assert OP.f12_mul(OP.f12_pow(g2, Q * Q), g) == g2         # cyclotomic
    assert OP.f12_pow(g, R) != OP.ONE                          # not a member
    assert OP.f12_pow(g, Q) != ref.conj_w(OP.f12_pow(g, ref.X_ABS))  # g^q != g^x
    e = ref.E()
    assert e != OP.ONE and OP.f12_pow(e, R) == OP.ONE


def _generator():
    spec = importlib.util.spec_from_file_location("gen_gt_consts", os.path.join(CSRC, "gen_gt_consts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_generator_reproduces_the_committed_constants():
    gen = _generator()
    assert gen.Q == Q
    with open(os.path.join(CSRC, "gt_consts_gen.inc")) as f:
        assert f.read() == gen.render()


def test_generated_constants_are_the_frobenius_maps():
    """w^k -> w^(k q) = xi^(k (q - 1) / 6) w^k in the oracle's field, for the constants the generator computes"""
    gen = _generator()
    f1, f2 = gen.frob1_consts(), gen.frob2_consts()
    for k in range(6):
        wk = [0] * 12
        wk[k] = 1
        c = [0] * 12
        c[0], c[1] = f1[k]
        assert OP.f12_pow(wk, Q) == OP.f12_mul(tower_to_w(c), wk)
        assert OP.f12_pow(wk, Q * Q) == OP.f12_scalar(wk, f2[k])
    assert f2[1] == 0x5F19672FDF76CE51BA69C6076A0F77EADDB3A93BE6F89688DE17D813620A00022E01FFFFFFFEFFFF  # DELTA of host_field.hpp


def test_exports_and_abi():
    lib = capi.load()
    for s in NAMES:
        assert hasattr(lib, s), s
        assert s in capi.SYMBOLS
    import gemini_amd
    from gemini_amd import herring, ipa
    from gemini_amd import pairing as gp

    assert gemini_amd.gt_final_exp_many is gp.gt_final_exp_many and gemini_amd.pairing_each is gp.pairing_each and gemini_amd.gt_check is gp.gt_check
    assert hasattr(herring.GtModuleTimeProver, "check") and hasattr(ipa.InnerProductProof, "check_messages")
    assert int(gp.GtStatus.NOT_CYCLOTOMIC) == 5
    with open(os.path.join(os.path.dirname(CSRC), "..", "include", "gemini_hip.h")) as f:
        assert "GM_PT_NOT_CYCLOTOMIC = 5" in f.read()


def test_entries_fail_closed_before_init():
    """no entry answers without gm_init, and the check entries clear *ok first (on the CPU-only box no process calls gm_init)"""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible; this test is about the CPU-only box")
    lib = capi.load()
    x = np.zeros((2, 72), dtype=np.uint64)
    out = np.zeros((2, 72), dtype=np.uint64)
    st = np.zeros(2, dtype=np.uint8)
    NOTINIT = -2
    assert lib.gm_gt_final_exp_many(capi.ptr(x), C.c_size_t(2), capi.ptr(out)) == NOTINIT
    assert lib.gm_gt_final_exp_many(None, C.c_size_t(0), None) == NOTINIT
    assert lib.gm_pairing_each(capi.ptr(x), C.c_size_t(96), capi.ptr(x), C.c_size_t(192), C.c_size_t(1), capi.ptr(out)) == NOTINIT
    assert lib.gm_pairing_each_h(C.c_uint64(1), C.c_size_t(0), C.c_size_t(1), C.c_uint64(2), C.c_size_t(0), C.c_size_t(1), C.c_size_t(1), capi.ptr(out)) == NOTINIT
    assert lib.gm_debug_gt_op(C.c_int(0), capi.ptr(x), C.c_size_t(2), capi.ptr(out)) == NOTINIT
    assert lib.gm_debug_gt_op2(C.c_int(0), capi.ptr(x), capi.ptr(x), C.c_size_t(2), capi.ptr(out)) == NOTINIT
    assert lib.gm_debug_gt_op2(C.c_int(99), None, None, C.c_size_t(0), None) == NOTINIT
    assert lib.gm_debug_miller_step(C.c_int(0), capi.ptr(x), C.c_size_t(2), capi.ptr(out)) == NOTINIT
    assert lib.gm_debug_miller_each(capi.ptr(x), C.c_size_t(96), capi.ptr(x), C.c_size_t(192), C.c_size_t(1), capi.ptr(out)) == NOTINIT
    for call in (lambda fb, ok: lib.gm_gt_check(capi.ptr(x), C.c_size_t(2), capi.ptr(st), fb, ok),
                 lambda fb, ok: lib.gm_hgt_check(C.c_uint64(1), fb, ok),
                 lambda fb, ok: lib.gm_ipa_check_gt(C.c_uint64(1), fb, ok)):
        fb, ok = C.c_size_t(7), C.c_int(1)
        assert call(C.byref(fb), C.byref(ok)) == NOTINIT and ok.value == 0
        assert call(None, None) == NOTINIT
