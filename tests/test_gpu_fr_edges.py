"""GPU: Fr at the edges, through the entries that exist -- hadamard, ip, fold_polynomial and the TimeProver's round messages --
against Python integers (oracle/pyref.py), bit for bit.

The vectors' Montgomery LIMBS are drawn from the values where a 32-bit-limb multiplier, its conditional subtraction and the 17-limb
lazy accumulator of the round kernel (fp_mac_wide) can go wrong: 0, 1, r - 1, r - 2, all-ones words below the top, single words at
every position.  What the device is given is the limbs m; the field element they stand for is m 2^-256 mod r, and the reference
computes on those.  All-(r - 1) vectors are the accumulator's worst case: every product is (r - 1)^2.

Lengths: 1, 2, 3, 255, 256, 257 (one block of the element-wise kernels is 256 threads), and 2^20 + 1: the round kernel runs at most
2^17 threads (gemini_amd/csrc/fr.hip:1005-1008, sc_prepare: `while (lt < 17 && ((size_t)1 << lt) < A.npairs) lt++`) and thread t takes the
pairs t, t + 2^17, ..., so a thread accumulates 5 pairs first when there are 4 * 2^17 + 1 of them -- 2^20 + 1 elements.  At that
length only the first message is compared (the reference is Python: two seconds of big integers for 2^19 pairs)."""
import numpy as np
import pytest

from gemini_amd import fr as F
from oracle import pyref
from tests.fr_cases import EDGE, EDGE_CANON, EDGE_LIMBS, R_MINUS_1, Vec, canon, edge_limbs, limbs, mont, vectors  # noqa: F401

pytestmark = pytest.mark.gpu

R = pyref.R_MOD
RINV = pow(1 << 256, -1, R)
LENGTHS = [1, 2, 3, 255, 256, 257]
FIVE_PAIRS = (1 << 20) + 1


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


CASES = [(n, s) for n in LENGTHS for s in (0, 2)] + [(len(EDGE) ** 2, 1)]  # the last: every value against every value


@pytest.mark.parametrize("n,shift", CASES)
def test_hadamard_and_ip(gm, n, shift):
    f, g = vectors(n, shift)
    if n == len(EDGE) ** 2:
        assert len(set(zip(f.idx.tolist(), g.idx.tolist()))) == n
    h = F.hadamard(f.limbs, g.limbs)
    try:
        assert (h.to_host() == mont(pyref.hadamard(f.canon, g.canon))).all()
    finally:
        h.free()
    assert (F.ip(f.limbs, g.limbs) == mont([pyref.ip(f.canon, g.canon)])[0]).all()


@pytest.mark.parametrize("n", LENGTHS + [1000])
def test_all_r_minus_1(gm, n):
    """the largest products there are, in every slot"""
    f = Vec([R_MINUS_1] * n)
    h = F.hadamard(f.limbs, f.limbs)
    try:
        assert (h.to_host() == mont(pyref.hadamard(f.canon, f.canon))).all()
    finally:
        h.free()
    assert (F.ip(f.limbs, f.limbs) == mont([pyref.ip(f.canon, f.canon)])[0]).all()


@pytest.mark.parametrize("n,shift", CASES[:-1])
def test_fold_polynomial(gm, n, shift):
    f, _ = vectors(n, shift)
    for r in (0, 1, R - 1, EDGE[5], 0x1234567 << 200):
        out = F.fold_polynomial(f.limbs, limbs([r])[0])
        try:
            assert (out.to_host() == mont(pyref.fold_polynomial(f.canon, canon([r])[0]))).all(), hex(r)
        finally:
            out.free()


def run_rounds(gm, f, g, twist_m, challenges_m, max_messages=None):
    """the device's messages and final foldings against pyref.TimeProver on the elements the limbs stand for"""
    O = pyref.TimeProver(f.canon, g.canon, canon([twist_m])[0])
    G = gm.TimeProver(f.limbs, g.limbs, limbs([twist_m])[0])
    try:
        assert G.rounds() == O.tot_rounds
        vm_o = vm_g = None
        k = 0
        while max_messages is None or k < max_messages:
            mo, mg = O.next_message(vm_o), G.next_message(vm_g)
            if mo is None:
                assert mg is None
                break
            want = mont(mo)
            assert (mg[0] == want[0]).all() and (mg[1] == want[1]).all(), f"round {k}"
            c = challenges_m[k % len(challenges_m)]
            vm_o, vm_g = canon([c])[0], limbs([c])[0]
            k += 1
        if max_messages is None:
            assert k == O.tot_rounds
            fo, fg = O.final_foldings(), G.final_foldings()
            assert (fg[0] == mont([fo[0]])[0]).all() and (fg[1] == mont([fo[1]])[0]).all()
    finally:
        G.free()


ONE_M = (1 << 256) % R          # the limbs of the field's one: the twist that takes the TW1 kernels
TWIST_M = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
CHALLENGES_M = (R - 1, 0x1F3A9C5D77E2B4A6908D1C3E5F7A9B2D4C6E8F0A1B3D5F79, 1, (1 << 224) - 1, R - 2, 0x0123456789ABCDEF << 190)


@pytest.mark.parametrize("twist", [TWIST_M, ONE_M, R - 1], ids=["twist", "twist=1", "twist=r-1 limbs"])
@pytest.mark.parametrize("n,shift", CASES[:-1])
def test_time_prover_messages(gm, n, shift, twist):
    f, g = vectors(n, shift)
    run_rounds(gm, f, g, twist, CHALLENGES_M)


@pytest.mark.parametrize("twist", [TWIST_M, ONE_M], ids=["twist", "twist=1"])
@pytest.mark.parametrize("n", LENGTHS + [1000])
def test_time_prover_all_r_minus_1(gm, n, twist):
    f = Vec([R_MINUS_1] * n)
    run_rounds(gm, f, f, twist, (R - 1, R - 2))


@pytest.mark.parametrize("twist", [TWIST_M, ONE_M], ids=["twist", "twist=1"])
@pytest.mark.parametrize("kind", ["edge list", "all r-1"])
def test_time_prover_five_pairs_per_thread(gm, kind, twist):
    """2^20 + 1 elements: 2^19 + 1 pairs over 2^17 threads, thread 0 accumulates five products per inner product before its one
    reduction (fr.hip:1005-1008, sc_prepare: log_threads is capped at 17).  The first message only: the reference walks 2^19 pairs in Python."""
    if kind == "all r-1":
        f = g = Vec([R_MINUS_1] * FIVE_PAIRS)
    else:
        f, g = vectors(FIVE_PAIRS, 1)
    run_rounds(gm, f, g, twist, (R - 1,), max_messages=1)
