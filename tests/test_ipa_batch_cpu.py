"""The batch inner-product argument without a GPU (tests/ipa_batch_ref.py): the literal 3 K-prover `generic` and the collapsed
prover the device runs give the same proof field for field, the generalised verifier accepts it and rejects every single
alteration, and K = 1 is `prove` / `verify` of tests/ipa_exponent_ref.py."""
import copy

import pytest

from oracle import pyref as P
from tests import ipa_batch_ref as B
from tests import ipa_exponent_ref as X

R = X.R
CASES = [(K, d, n, ()) for K, d, n in B.SHAPES] + [(2, 8, 16, (3,))]


@pytest.fixture(scope="module", params=CASES, ids=lambda p: f"K{p[0]}-d{p[1]}-n{p[2]}" + ("-inf" if p[3] else ""))
def case(request):
    """(s, t, claims, the collapsed proof, the Vrs, comm_a, comm_b, y): computed once, never modified"""
    K, d, n, inf = request.param
    _, s, _, t = X.crs(n, infinity_at=inf)
    claims = B.claims_for(K, d, seed=K * 100 + d, zero_a=K - 1 if K > 1 else None)  # one a_i = 0
    proof = B.prove_collapsed(P.GeminiTranscript(b"gemini-tests"), s, t, claims)
    ca, cb, y = B.statement(s, t, claims)
    return s, t, claims, proof, X.vrs(s, t), ca, cb, y


def test_literal_equals_collapsed_in_every_field(case):
    s, t, claims, proof, *_ = case
    K = len(claims)
    t1, t2 = P.GeminiTranscript(b"gemini-tests"), P.GeminiTranscript(b"gemini-tests")
    lit = B.prove_literal(t1, s, t, claims)
    assert B.prove_collapsed(t2, s, t, claims) == proof
    assert set(lit) == set(proof)
    for name in lit:
        assert lit[name] == proof[name], name
    assert t1.get_challenge(b"next") == t2.get_challenge(b"next")
    R_ = proof["rounds"]
    assert len(proof["batch_challenges"]) == 3 * K + 2 * (R_ - 1) and len(proof["final_foldings"]) == 2 * (R_ - 1)
    assert len(proof["foldings_ff"]) == len(proof["foldings_fg1"]) == len(proof["foldings_fg2"]) == K


def test_verifier_accepts(case):
    s, t, claims, proof, vk, ca, cb, y = case
    assert B.verify_batch(proof, vk, ca, cb, y)


def test_verifier_rejects_single_alterations(case):
    s, t, claims, proof, vk, ca, cb, y = case
    K = len(claims)
    for i in range(K):
        bad_y = list(y)
        bad_y[i] = (bad_y[i] + 1) % R
        assert not B.verify_batch(proof, vk, ca, cb, bad_y), ("y", i)
    if K >= 2:  # commitments swapped between two claims
        sw = lambda v: [v[1], v[0]] + list(v[2:])
        assert ca[0] != ca[1] and cb[0] != cb[1]
        assert not B.verify_batch(proof, vk, sw(ca), cb, y)
        assert not B.verify_batch(proof, vk, ca, sw(cb), y)
    for i in range(proof["rounds"]):
        for h in range(2):
            bad = copy.deepcopy(proof)
            m = list(bad["messages"][i])
            m[h] = (m[h] + 1) % R
            bad["messages"][i] = tuple(m)
            assert not B.verify_batch(bad, vk, ca, cb, y), ("message", i, h)
    for i in range(K):
        bad = copy.deepcopy(proof)
        l, r = bad["foldings_ff"][i]
        bad["foldings_ff"][i] = ((l + 1) % R, r)  # the side that counts when a_i = 0 (then lhs = 0 and rhs is free)
        assert not B.verify_batch(bad, vk, ca, cb, y), ("ff", i)
        bad = copy.deepcopy(proof)
        l, r = bad["foldings_fg1"][i]
        bad["foldings_fg1"][i] = (l, (r + 1) % R)
        assert not B.verify_batch(bad, vk, ca, cb, y), ("fg1", i)
        bad = copy.deepcopy(proof)
        l, r = bad["foldings_fg2"][i]
        bad["foldings_fg2"][i] = ((l + 1) % R, r)
        assert not B.verify_batch(bad, vk, ca, cb, y), ("fg2", i)


@pytest.mark.parametrize("d,n", [(8, 16), (5, 16), (2, 4)])
def test_one_claim_is_the_single_proof(d, n):
    _, s, _, t = X.crs(n)
    (a, b), = B.claims_for(1, d, seed=d)
    t1, t2, t3 = (P.GeminiTranscript(b"gemini-tests") for _ in range(3))
    single = X.prove(t1, s, t, a, b)
    for batch, tr in ((B.prove_collapsed(t2, s, t, [(a, b)]), t2), (B.prove_literal(t3, s, t, [(a, b)]), t3)):
        for name in ("rounds", "messages", "challenges", "batch_challenges", "final_foldings"):
            assert batch[name] == single[name], name
        for name in ("foldings_ff", "foldings_fg1", "foldings_fg2"):
            assert batch[name] == [single[name]], name
    assert t1.get_challenge(b"next") == t2.get_challenge(b"next") == t3.get_challenge(b"next")
    vk, ca, cb, y = X.vrs(s, t), X.commit(s, a), X.commit(t, b), X.ip(a, b)
    for yy in (y, (y + 1) % R):
        assert B.verify_batch(batch, vk, [ca], [cb], [yy]) == X.verify(single, vk, ca, cb, yy)
