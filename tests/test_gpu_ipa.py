"""herring's InnerProductProof on the device (gm_crs_*, gm_vrs_*, gm_ipa_*; gemini_amd/csrc/ipa.hip) against the exponent restatement
of tests/ipa_exponent_ref.py: field by field and bit for bit on canonical integers.

The shapes are the smallest at which each part of the segmented Miller kernel can go wrong (64 pairs per block):
    d = 2     CRS 4      the round loop runs zero times
    d = 4     CRS 8
    d = 5     CRS 16     odd tails in the F, G1 and G2 provers; rounds = 3
    d = 64    CRS 128    segments of 16 ... 1 pairs sharing one wave with several provers live
    d = 512   CRS 1024   segments of 128 pairs crossing wave and block boundaries (one reduction level)
    d = 1024  CRS 2048   the reference's test_correctness shape
"""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

from gemini_amd import pairing as gp
from gemini_amd.fr import fr_from_int, fr_to_int
from gemini_amd.g2msm import g2_jac_to_point, g2_points_to_affine
from oracle import pyref as P
from tests import ipa_exponent_ref as X
from tests.test_gpu_pairing import g1_jac_to_point, g1_points_to_affine

pytestmark = pytest.mark.gpu

R = X.R
GM_EINVAL, GM_EHANDLE = -1, -3
LABEL = b"gemini-tests"
SHAPES = [(2, 4), (4, 8), (5, 16), (64, 128), (512, 1024), (1024, 2048)]


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


def mont(v) -> np.ndarray:
    return np.stack([fr_from_int(x) for x in v])


def scalars(seed: int, n: int, zeros=()):
    rng = P.SplitMix64(seed)
    v = [rng.fr() for _ in range(n)]
    for i in zeros:
        v[i] = 0
    return v


@functools.lru_cache(maxsize=None)
def reference(d: int, n: int, special: bool = False):
    """the inputs and the restatement's proof of one shape: computed once, never modified.  special: points at infinity in the CRS
    and zeros among the scalars"""
    p1, s, p2, t = X.crs(n, infinity_at=(1, 6) if special else ())
    zeros = (0, 3) if special else ()
    a, b = scalars(1000 + d, d, zeros), scalars(2000 + d, d, zeros[:1])
    tr = P.GeminiTranscript(LABEL)
    proof = X.prove(tr, s, t, a, b)
    out = {"s": s, "t": t, "a": a, "b": b, "r1": g1_points_to_affine(p1, flag=special), "r2": g2_points_to_affine(p2, flag=special), "a_mont": mont(a),
           "b_mont": mont(b), "proof": proof, "next": tr.get_challenge(b"next"), "comm_a": X.commit(s, a), "comm_b": X.commit(t, b), "y": X.ip(a, b)}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def prove_on_device(gm, ref):
    """-> (Crs, transcript after the proof, InnerProductProof)"""
    crs = gm.Crs(ref["r1"], ref["r2"])
    tr = gm.Transcript(LABEL)
    return crs, tr, gm.InnerProductProof.new(tr, crs, ref["a_mont"], ref["b_mont"])


def assert_fields_equal(f, exp):
    """the device proof's fields against the restatement's logs"""
    k = exp["rounds"]
    assert f.rounds == k
    assert [fr_to_int(c) for c in f.challenges] == exp["challenges"]
    assert [fr_to_int(c) for c in f.batch_challenges] == exp["batch_challenges"]
    for i, (a, b) in enumerate(exp["messages"]):
        assert gp.gt_to_ints(f.messages[i, 0]) == X.gt_ints(a), ("message a", i)
        assert gp.gt_to_ints(f.messages[i, 1]) == X.gt_ints(b), ("message b", i)
    assert len(f.final_lhs) == len(f.final_rhs) == len(exp["final_foldings"]) == 2 * (k - 1)
    for p, (l, r) in enumerate(exp["final_foldings"]):
        assert g1_jac_to_point(f.final_lhs[p]) == X.g1_point(l), ("final lhs", p)
        assert g2_jac_to_point(f.final_rhs[p]) == X.g2_point(r), ("final rhs", p)
    assert (fr_to_int(f.foldings_ff[0]), fr_to_int(f.foldings_ff[1])) == exp["foldings_ff"]
    assert (g1_jac_to_point(f.foldings_fg1[0]), fr_to_int(f.foldings_fg1[1])) == (X.g1_point(exp["foldings_fg1"][0]), exp["foldings_fg1"][1])
    assert (fr_to_int(f.foldings_fg2[0]), g2_jac_to_point(f.foldings_fg2[1])) == (exp["foldings_fg2"][0], X.g2_point(exp["foldings_fg2"][1]))


@pytest.mark.parametrize("d,n", SHAPES, ids=[f"d{d}" for d, _ in SHAPES])
def test_proof_equals_the_exponent_restatement(gm, d, n):
    """gm_ipa_new field by field, the transcript it leaves behind, the commitments, and gm_ipa_verify on the result"""
    ref = reference(d, n)
    crs, tr, proof = prove_on_device(gm, ref)
    assert_fields_equal(proof.fields(), ref["proof"])
    assert fr_to_int(tr.get_challenge(b"next")) == ref["next"]  # handed on: the same next challenge as the restatement's
    comm_a, comm_b = crs.commit_g1(ref["a_mont"]), crs.commit_g2(ref["b_mont"])
    assert g1_jac_to_point(comm_a) == X.g1_point(ref["comm_a"]) and g2_jac_to_point(comm_b) == X.g2_point(ref["comm_b"])
    vrs = gm.Vrs(crs)
    assert vrs.levels == X.ceil_log2(n) - 1
    assert proof.verify_transcript(vrs, comm_a, comm_b, fr_from_int(ref["y"]))
    assert not proof.verify_transcript(vrs, comm_a, comm_b, fr_from_int((ref["y"] + 1) % R))
    for o in (proof, vrs, tr, crs):
        o.free()


@pytest.mark.parametrize("d,n", [(5, 16), (64, 128)])
def test_verifier_rejects(gm, d, n):
    """a tampered message, a swapped commitment, a tampered final folding and the Vrs of another CRS"""
    ref = reference(d, n)
    crs, tr, proof = prove_on_device(gm, ref)
    vrs = gm.Vrs(crs)
    comm_a, comm_b, y = crs.commit_g1(ref["a_mont"]), crs.commit_g2(ref["b_mont"]), fr_from_int(ref["y"])
    f = proof.fields()
    same = gm.InnerProductProof.from_fields(f)
    assert same.verify_transcript(vrs, comm_a, comm_b, y)
    same.free()
    e2 = gp.gt_from_ints(X.gt_ints(2))
    for i, h in ((0, 0), (f.rounds - 1, 1), (1, 0)):
        g = proof.fields()
        g.messages[i, h] = gp.gt_mul(g.messages[i, h], e2)
        bad = gm.InnerProductProof.from_fields(g)
        assert not bad.verify_transcript(vrs, comm_a, comm_b, y), (i, h)
        bad.free()
    g = proof.fields()
    g.final_lhs[0] = g.final_lhs[1]
    bad = gm.InnerProductProof.from_fields(g)
    assert not bad.verify_transcript(vrs, comm_a, comm_b, y)
    bad.free()
    other = crs.commit_g1(ref["b_mont"])
    assert not proof.verify_transcript(vrs, other, comm_b, y)
    # another CRS: the same points in another order
    crs2 = gm.Crs(ref["r1"][::-1].copy(), ref["r2"][::-1].copy())
    vrs2 = gm.Vrs(crs2)
    assert not proof.verify_transcript(vrs2, comm_a, comm_b, y)
    for o in (vrs2, crs2, proof, vrs, tr, crs):
        o.free()


@pytest.mark.parametrize("n", [8, 11, 128])
def test_vrs_equals_the_products_one_by_one(gm, n):
    """gm_vrs_from_crs (one segmented launch) against gm_pairing_multi_h called product by product and against the logs; n = 11:
    a CRS that is no power of two (the zips end early), n = 128: segments of 2 ... 64 pairs in one launch"""
    p1, s, p2, t = X.crs(n)
    r1, r2 = g1_points_to_affine(p1), g2_points_to_affine(p2)
    crs, b1, b2 = gm.Crs(r1, r2), gm.G1Bases.register(r1), gm.G2Bases.register(r2)
    vrs = gm.Vrs(crs)
    vk1, vk2 = X.vrs(s, t)
    assert vrs.levels == len(vk1) == X.ceil_log2(n) - 1
    for l in range(vrs.levels):
        size = 2 << l
        got1, got2 = vrs.level(l)
        one = [gm.multi_pairing_h(b1, b2, min(size, (n + 1) // 2), off1=0, step1=2), gm.multi_pairing_h(b1, b2, min(size, n // 2), off1=1, step1=2),
               gm.multi_pairing_h(b1, b2, min(size, (n + 1) // 2), off2=0, step2=2), gm.multi_pairing_h(b1, b2, min(size, n // 2), off2=1, step2=2)]
        assert (got1[0] == one[0]).all() and (got1[1] == one[1]).all() and (got2[0] == one[2]).all() and (got2[1] == one[3]).all(), l
        assert [gp.gt_to_ints(g) for g in (got1[0], got1[1], got2[0], got2[1])] == [X.gt_ints(x) for x in vk1[l] + vk2[l]], l
    for o in (vrs, b1, b2, crs):
        o.free()


def test_infinity_in_the_crs_and_zero_scalars(gm):
    """points at infinity (flagged (n, 13) / (n, 25) records) among the points every round folds and pairs, zeros among the scalars"""
    ref = reference(8, 16, True)
    crs, tr, proof = prove_on_device(gm, ref)
    assert_fields_equal(proof.fields(), ref["proof"])
    vrs = gm.Vrs(crs)
    assert proof.verify_transcript(vrs, crs.commit_g1(ref["a_mont"]), crs.commit_g2(ref["b_mont"]), fr_from_int(ref["y"]))
    for o in (proof, vrs, tr, crs):
        o.free()


def test_refusals_and_stale_handles(gm):
    lib, ptr = gm.capi.load(), gm.capi.ptr
    ref = reference(4, 8)
    crs = gm.Crs(ref["r1"], ref["r2"])
    tr = gm.Transcript(LABEL)
    h = C.c_uint64()

    def new(crs_handle, d, a=ref["a_mont"], b=ref["b_mont"]):
        return lib.gm_ipa_new(C.c_uint64(tr.handle), C.c_uint64(crs_handle), ptr(np.array(a)), ptr(np.array(b)), C.c_size_t(d), C.byref(h))

    assert new(crs.handle, 1) == GM_EINVAL and new(crs.handle, 0) == GM_EINVAL  # d < 2
    short = gm.Crs(ref["r1"][:4], ref["r2"][:4])  # d = 4 needs d + 1 = 5 points
    assert new(short.handle, 4) == GM_EINVAL
    five = gm.Crs(np.array(reference(5, 16)["r1"][:6]), np.array(reference(5, 16)["r2"][:6]))  # d = 5 needs 2^3 = 8 points, d + 1 = 6 is not enough
    assert new(five.handle, 5, reference(5, 16)["a_mont"], reference(5, 16)["b_mont"]) == GM_EINVAL
    out = np.zeros(36, dtype=np.uint64)
    a8 = mont(scalars(1, 8))
    assert lib.gm_crs_commit_g1(C.c_uint64(crs.handle), ptr(a8), C.c_size_t(8), ptr(out)) == GM_EINVAL  # the CRS must be LONGER than the scalars
    assert lib.gm_crs_commit_g2(C.c_uint64(crs.handle), ptr(a8), C.c_size_t(8), ptr(out)) == GM_EINVAL
    assert lib.gm_crs_commit_g1(C.c_uint64(crs.handle), ptr(a8), C.c_size_t(7), ptr(out)) == 0
    # nothing above consumed the transcript: a proof made now is the restatement's
    proof = gm.InnerProductProof.new(tr, crs, ref["a_mont"], ref["b_mont"])
    assert_fields_equal(proof.fields(), ref["proof"])
    vrs = gm.Vrs(crs)
    comm_a, comm_b, y, ok = crs.commit_g1(ref["a_mont"]), crs.commit_g2(ref["b_mont"]), fr_from_int(ref["y"]), C.c_int()
    short_vrs = gm.Vrs(short)  # 1 level; a proof of 2 rounds needs 1: fine.  A Vrs without levels is refused
    tiny = gm.Crs(ref["r1"][:2], ref["r2"][:2])
    tiny_vrs = gm.Vrs(tiny)
    assert short_vrs.levels == 1 and tiny_vrs.levels == 0
    assert lib.gm_ipa_verify(C.c_uint64(proof.handle), C.c_uint64(tiny_vrs.handle), ptr(comm_a), ptr(comm_b), ptr(y), C.byref(ok)) == GM_EINVAL
    # handles of other kinds and stale ones
    assert lib.gm_ipa_verify(C.c_uint64(vrs.handle), C.c_uint64(vrs.handle), ptr(comm_a), ptr(comm_b), ptr(y), C.byref(ok)) == GM_EHANDLE
    assert lib.gm_ipa_verify(C.c_uint64(proof.handle), C.c_uint64(crs.handle), ptr(comm_a), ptr(comm_b), ptr(y), C.byref(ok)) == GM_EHANDLE
    assert lib.gm_vrs_from_crs(C.c_uint64(proof.handle), C.byref(h)) == GM_EHANDLE
    ph, vh, ch = proof.handle, vrs.handle, crs.handle
    assert proof.verify_transcript(vrs, comm_a, comm_b, y)
    proof.free()
    assert lib.gm_ipa_verify(C.c_uint64(ph), C.c_uint64(vh), ptr(comm_a), ptr(comm_b), ptr(y), C.byref(ok)) == GM_EHANDLE
    assert lib.gm_ipa_rounds(C.c_uint64(ph), C.byref(C.c_size_t())) == GM_EHANDLE and lib.gm_ipa_free(C.c_uint64(ph)) == GM_EHANDLE
    vrs.free()
    assert lib.gm_vrs_levels(C.c_uint64(vh), C.byref(C.c_size_t())) == GM_EHANDLE and lib.gm_vrs_free(C.c_uint64(vh)) == GM_EHANDLE
    crs.free()
    assert new(ch, 4) == GM_EHANDLE and lib.gm_crs_free(C.c_uint64(ch)) == GM_EHANDLE
    assert lib.gm_crs_len(C.c_uint64(ch), None, None) == GM_EHANDLE
    for o in (short_vrs, tiny_vrs, short, tiny, five, tr):
        o.free()


def test_two_proofs_from_two_threads(gm):
    """two provers at once on one context, over one CRS: each thread's proof is the restatement's"""
    refs = [reference(64, 128), reference(5, 16)]
    crs = [gm.Crs(r["r1"], r["r2"]) for r in refs]
    got, errs = [None, None], []

    def run(k):
        try:
            tr = gm.Transcript(LABEL)
            p = gm.InnerProductProof.new(tr, crs[k], refs[k]["a_mont"], refs[k]["b_mont"])
            got[k] = (p.fields(), fr_to_int(tr.get_challenge(b"next")))
            p.free()
            tr.free()
        except Exception as e:  # noqa: BLE001 -- reported below with the thread index
            errs.append((k, e))

    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errs, errs
    for k in range(2):
        assert_fields_equal(got[k][0], refs[k]["proof"])
        assert got[k][1] == refs[k]["next"]
    for c in crs:
        c.free()
