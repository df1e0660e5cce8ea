"""GtModule without a GPU: the two statements of TimeProver<GtModule> on Python integers (tests/gt_module_ref.py) agree, the C ABI
exports the GtModule entries, and without gm_init they fail loudly instead of computing on the host."""
import ctypes as C
import random

import numpy as np
import pytest

from gemini_amd import capi
from oracle import pairing as OP
from tests import gt_module_ref as GR

R = GR.R
NAMES = ("gm_gt_multi_pow", "gm_hgt_new", "gm_hgt_round", "gm_hgt_fold", "gm_hgt_rounds", "gm_hgt_final", "gm_hgt_free")


@pytest.mark.parametrize("nf,ng", [(4, 4), (3, 2)])
def test_literal_and_exponent_statements_agree(nf, ng):
    rng = random.Random(0x6774 + 16 * nf + ng)
    E = GR.E()
    k = [rng.randrange(R) for _ in range(nf)]
    g = [rng.randrange(R) for _ in range(ng)]
    tw = rng.randrange(2, R)
    ch = [rng.randrange(R) for _ in range(4)]
    L = GR.GtProverLiteral([OP.f12_pow(E, x) for x in k], g, tw)
    X = GR.GtProverOnLogs(k, g, tw)
    assert L.tot_rounds == X.tot_rounds == GR.ceil_log2(min(nf, ng))
    assert L.final_foldings() is None and X.final_foldings() is None
    vm, rounds = None, 0
    while True:
        ml, mx = L.next_message(vm), X.next_message(vm)
        if mx is None:
            assert ml is None
            break
        assert ml == (OP.f12_pow(E, mx[0]), OP.f12_pow(E, mx[1])), (nf, ng, rounds)
        vm = ch[rounds]
        rounds += 1
    assert rounds == L.tot_rounds
    (fl, gl), (fx, gx) = L.final_foldings(), X.final_foldings()
    assert fl == OP.f12_pow(E, fx) and gl == gx
    # a fold after the last round goes on folding (against nothing, on one side or both): the two still agree
    L.fold(ch[3])
    X.fold(ch[3])
    assert L.next_message() is None and X.next_message() is None
    assert L.final_foldings() == (OP.f12_pow(E, X.f[0]), X.g[0])


def test_exports():
    lib = capi.load()
    for s in NAMES:
        assert hasattr(lib, s), s
        assert s in capi.SYMBOLS
    assert lib.gm_abi_version() == 1
    import gemini_amd
    from gemini_amd import herring
    from gemini_amd import pairing as gp

    assert gemini_amd.gt_multi_pow is gp.gt_multi_pow and hasattr(herring, "GtModuleTimeProver")


def test_no_host_fallback_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible; this test is about the CPU-only box")
    lib = capi.load()
    x = np.zeros((2, 72), dtype=np.uint64)
    s = np.ones((2, 4), dtype=np.uint64)
    out = np.zeros(72, dtype=np.uint64)
    h = C.c_uint64()
    assert lib.gm_gt_multi_pow(capi.ptr(x), C.c_size_t(2), capi.ptr(s), capi.ptr(out)) == -2  # GM_ENOTINIT
    assert b"gm_init" in lib.gm_last_error()
    assert lib.gm_gt_multi_pow(None, C.c_size_t(0), None, capi.ptr(out)) == -2  # n = 0 too: no entry answers without gm_init
    assert lib.gm_hgt_new(capi.ptr(x), C.c_size_t(2), capi.ptr(s), C.c_size_t(2), capi.ptr(s[0]), C.byref(h)) == -2
    assert b"gm_init" in lib.gm_last_error()
    assert lib.gm_hgt_round(C.c_uint64(1), None, capi.ptr(out), capi.ptr(out), C.byref(C.c_int())) == -2
    assert lib.gm_hgt_fold(C.c_uint64(1), capi.ptr(s[0])) == -2
    assert lib.gm_hgt_rounds(C.c_uint64(1), None, None) == -2
    assert lib.gm_hgt_final(C.c_uint64(1), capi.ptr(out), capi.ptr(s[0]), C.byref(C.c_int())) == -2
    assert lib.gm_hgt_free(C.c_uint64(1)) == -2
    assert not out.any()
