"""herring's inner-product argument without a GPU: the exponent restatement (tests/ipa_exponent_ref.py) accepts its own proofs and
rejects changed ones, and the framing of GT elements in the transcript (gm_transcript_append_gt, host code of the library) is the
576-byte image the restatement absorbs."""
import copy

import numpy as np
import pytest

from oracle import pyref as P
from tests import ipa_exponent_ref as X

R = X.R


def scalars(seed: int, n: int, zeros=()):
    rng = P.SplitMix64(seed)
    v = [rng.fr() for _ in range(n)]
    for i in zeros:
        v[i] = 0
    return v


@pytest.fixture(scope="module", params=[(2, 4), (5, 16), (8, 16)], ids=lambda p: f"d{p[0]}")
def case(request):
    """(logs of the CRS, a, b, the proof of the restatement, its Vrs, comm_a, comm_b, y): computed once, never modified"""
    d, n = request.param
    s, t = [X.g1_log(i) for i in range(n)], [X.g2_log(i) for i in range(n)]
    a, b = scalars(100 + d, d), scalars(200 + d, d)
    proof = X.prove(P.GeminiTranscript(b"gemini-tests"), s, t, a, b)
    return s, t, a, b, proof, X.vrs(s, t), X.commit(s, a), X.commit(t, b), X.ip(a, b)


def test_accepts_its_own_proof(case):
    s, t, a, b, proof, vk, ca, cb, y = case
    d = len(a)
    assert proof["rounds"] == X.ceil_log2(d) == len(proof["messages"]) == len(proof["challenges"])
    assert len(proof["batch_challenges"]) == 2 * proof["rounds"] + 1 and len(proof["final_foldings"]) == 2 * (proof["rounds"] - 1)
    assert X.verify(proof, vk, ca, cb, y)


def test_rejects_changed_values(case):
    s, t, a, b, proof, vk, ca, cb, y = case
    assert not X.verify(proof, vk, ca, cb, (y + 1) % R)
    assert not X.verify(proof, vk, (ca + 1) % R, cb, y)
    assert not X.verify(proof, vk, ca, (cb + 1) % R, y)
    for i in range(proof["rounds"]):
        for h in range(2):
            bad = copy.deepcopy(proof)
            m = list(bad["messages"][i])
            m[h] = (m[h] + 1) % R
            bad["messages"][i] = tuple(m)
            assert not X.verify(bad, vk, ca, cb, y), (i, h)
    for name in ("foldings_ff", "foldings_fg1", "foldings_fg2"):
        bad = copy.deepcopy(proof)
        bad[name] = (bad[name][0], (bad[name][1] + 1) % R)
        assert not X.verify(bad, vk, ca, cb, y), name
    for k in range(len(proof["final_foldings"])):  # the foldings that depend on the challenges of the rounds
        bad = copy.deepcopy(proof)
        l, r = bad["final_foldings"][k]
        bad["final_foldings"][k] = ((l + 1) % R, r)
        assert not X.verify(bad, vk, ca, cb, y), k


def test_transcript_goes_on_differently_after_a_different_proof(case):
    s, t, a, b, proof, *_ = case
    t1, t2 = P.GeminiTranscript(b"gemini-tests"), P.GeminiTranscript(b"gemini-tests")
    assert X.prove(t1, s, t, a, b) == proof
    X.prove(t2, s, t, a, [(b[0] + 1) % R] + b[1:])
    assert t1.get_challenge(b"next") != t2.get_challenge(b"next")


def test_gt_framing_is_576_bytes_and_round_trips():
    from gemini_amd import pairing as gp
    from gemini_amd.transcript import Transcript

    xs = [0, 1, 5, R - 1, scalars(7, 1)[0]]
    for x in xs:
        b = X.gt_bytes(x)
        assert len(b) == 576 and X.gt_ints_from_bytes(b) == X.gt_ints(x)
    assert X.gt_ints(0) == [1] + [0] * 11 and X.gt_ints(R) == X.gt_ints(0)  # E has order r
    # the library frames a GT element the same way: same next challenge as Merlin over the restatement's bytes
    for count in (1, 2):
        lib_t, ref_t = Transcript(b"gemini-tests"), P.GeminiTranscript(b"gemini-tests")
        vals = xs[2: 2 + count]
        lib_t.append_gt(b"sumcheck-round", np.stack([gp.gt_from_ints(X.gt_ints(x)) for x in vals]))
        ref_t.append_message(b"sumcheck-round", b"".join(X.gt_bytes(x) for x in vals))
        assert lib_t.challenge_bytes(b"c", 32) == ref_t.challenge_bytes(b"c", 32)
        lib_t.free()
