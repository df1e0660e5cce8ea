"""GPU: gm_g1_lincomb_many -- S short linear combinations in a fixed number of launches (k_g1_term_mul: one lane per term,
k_g1_seg_sum: one lane per segment).  The oracles are gm_g1_msm on every segment and the CPU restatement (oracle.msm_pippenger /
oracle.msm_naive); every compare is exact, on canonical affine integers."""
import numpy as np
import pytest

from tests.util import jac_to_affine_ints, rand_bases

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 33, 300)


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


def _is_identity(jac) -> bool:
    return not np.asarray(jac, dtype=np.uint64).reshape(3, 6)[2].any()


def _same(oracle, got, want):
    if _is_identity(want):
        assert _is_identity(got)
    else:
        assert not _is_identity(got) and jac_to_affine_ints(oracle, got) == jac_to_affine_ints(oracle, want)


def _segment_lengths(S):
    """lengths mixed from LENGTHS; from S = 3 on the terms span several 256-lane blocks and a 300-term segment straddles a block edge"""
    if S == 1:
        return [33]
    order = (2, 300, 0, 33, 1)
    return [order[i % 5] for i in range(S)]


@pytest.mark.parametrize("S", [1, 3, 70])
def test_lincomb_many_against_the_msm_and_the_oracle(gm, oracle, S):
    from gemini_amd.msm import g1_lincomb_many

    lens = _segment_lengths(S)
    assert set(lens) <= set(LENGTHS)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    T = int(off[-1])
    assert S < 3 or (T > 256 and any(int(a) // 256 != (int(b) - 1) // 256 for a, b in zip(off[:-1], off[1:]) if b > a))
    bases = rand_bases(oracle, 7100 + S, T)
    sc = oracle.random_fr(7200 + S, T)
    got = g1_lincomb_many(bases, sc, off)
    assert got.shape == (S, 18)
    for s in range(S):
        lo, hi = int(off[s]), int(off[s + 1])
        if lo == hi:
            assert _is_identity(got[s])
            continue
        _same(oracle, got[s], gm.VariableBaseMSM.msm_bigint(bases[lo:hi], sc[lo:hi]))
        _same(oracle, got[s], oracle.msm_pippenger(bases[lo:hi], sc[lo:hi]))


def test_lincomb_many_edge_segments(gm, oracle, pyref):
    """what an adversarial proof can put into a segment: equal terms (a doubling), opposite terms (the identity), the scalars 0, 1,
    r - 1 and one of 2^254, an identity record among the points, all terms equal"""
    from gemini_amd.msm import g1_lincomb_many

    from oracle import pairing as OP

    R = pyref.R_MOD
    pts = rand_bases(oracle, 7300, 4)
    P, P2 = pts[0], pts[1]
    x, y = oracle.affine_to_ints(P)
    negP = oracle.ints_to_affine((x, OP.Q - y))
    zero = np.zeros(12, dtype=np.uint64)
    s = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % R
    big = (1 << 254) + 12345
    assert big < R
    segments = {
        "scalar 0": [(P, 0)],
        "scalar 1": [(P, 1)],
        "scalar r - 1": [(P, R - 1)],
        "scalar 2^254": [(P, big), (P2, 1)],
        "identity record": [(P, 5), (zero, 7), (P2, 11)],
        "only identity records": [(zero, 1), (zero, R - 1)],
        "P + P": [(P, 1), (P, 1)],
        "s P + (r - s) P": [(P, s), (P, R - s)],
        "P + (-P)": [(P, 1), (negP, 1)],
        "P + (-P) + P2": [(P, 1), (negP, 1), (P2, 3)],
        "all terms equal": [(P2, s)] * 5,
        "empty": [],
    }
    names = list(segments)
    bases = np.array([p for n in names for p, _ in segments[n]], dtype=np.uint64).reshape(-1, 12)
    sc = oracle.ints_to_limbs([k for n in names for _, k in segments[n]], 4)
    off = np.concatenate([[0], np.cumsum([len(segments[n]) for n in names])]).astype(np.uint64)
    got = g1_lincomb_many(bases, sc, off)
    for i, n in enumerate(names):
        lo, hi = int(off[i]), int(off[i + 1])
        want = gm.VariableBaseMSM.msm_bigint(bases[lo:hi], sc[lo:hi]) if hi > lo else None
        if want is None or _is_identity(want):
            assert _is_identity(got[i]), n
        else:
            _same(oracle, got[i], want)
        if not any(not p.any() for p, _ in segments[n]) and hi > lo:  # the CPU restatement has no identity record
            _same(oracle, got[i], oracle.msm_naive(bases[lo:hi], sc[lo:hi]))
    for n in ("scalar 0", "only identity records", "s P + (r - s) P", "P + (-P)", "empty"):
        assert _is_identity(got[names.index(n)]), n
    one = oracle.ints_to_limbs([1], 4)[0]
    p_jac = oracle.g1_mul(P, one)
    _same(oracle, got[names.index("P + P")], oracle.g1_add(p_jac, p_jac))
    _same(oracle, got[names.index("scalar r - 1")], oracle.g1_mul(negP, one))


def test_lincomb_many_no_segments_and_misuse(gm, oracle):
    import ctypes as C

    from gemini_amd.msm import g1_lincomb_many

    assert g1_lincomb_many(np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64), [0]).shape == (0, 18)
    bases = rand_bases(oracle, 7400, 3)
    sc = oracle.random_fr(7401, 3)
    out = np.zeros((2, 18), dtype=np.uint64)
    descending = np.array([0, 3, 2], dtype=np.uintp)
    lib = gm.capi.load()
    assert lib.gm_g1_lincomb_many(gm.capi.ptr(bases), C.c_size_t(96), gm.capi.ptr(sc), gm.capi.ptr(descending), C.c_size_t(2), gm.capi.ptr(out)) == -1
    assert lib.gm_g1_lincomb_many(gm.capi.ptr(bases), C.c_size_t(96), gm.capi.ptr(sc), None, C.c_size_t(2), gm.capi.ptr(out)) == -1
