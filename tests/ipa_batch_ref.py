"""The oracle of the batch inner-product argument (test infrastructure, Python integers).

`InnerProductProof::generic` (src/herring/ipa.rs:345-531) restated IN THE EXPONENT with the provers of tests/ipa_exponent_ref.py,
for the statement `new_batch` fixes: K claims <a_i, b_i> = y_i, <a_i, crs.g1> = comm_a_i, <b_i, crs.g2> = comm_b_i, every twist one,
every vector of the same length d.

  prove_literal    3 K LogProvers, as `generic` runs them: K FModule, K G1Module over the CRS, K G2Module over the CRS
  prove_collapsed  what the device runs: K FModule provers, ONE G1Module prover over sum_i bc^(K+i) a_i and ONE G2Module prover
                   over sum_i bc^(2K+i) b_i.  The batch weights of the initial provers are fixed for the whole proof and fold and
                   message are linear in the scalar side, so the two proofs are equal field for field.
  verify_batch     `verify_transcript` (ipa.rs:250-343) with the constant 3 replaced by 3 K.  The reference has no verifier for
                   `generic`; this one is the library's own.

A proof is the dict of tests/ipa_exponent_ref.py with `foldings_ff`, `foldings_fg1`, `foldings_fg2` lists of K pairs.
"""
from tests import ipa_exponent_ref as X

R = X.R


def _powers(x: int, n: int) -> list:
    out, p = [], 1
    for _ in range(n):
        out.append(p)
        p = p * x % R
    return out


def _run(transcript, s, t, K, make_initial):
    """The round loop of `generic`.  `make_initial(bc)` gives the initial provers and the weights of their messages once the first
    batch challenge is known; the PModule provers take batch_challenges[3 K + p]."""
    messages, challenges = [], []
    bc = transcript.get_challenge(b"batch-chal")
    K3 = 3 * K
    initial, w = make_initial(bc)
    assert len(w) == len(initial)
    batch_challenges = _powers(bc, K3)
    ms = [p.next_message() for p in initial]
    msg = tuple(sum(m[h] * x for m, x in zip(ms, w)) % R for h in range(2))
    transcript.append_message(b"prover_message", X.gt_bytes(msg[0]) + X.gt_bytes(msg[1]))
    messages.append(msg)
    rounds = max(p.tot_rounds for p in initial)
    assert all(p.tot_rounds == rounds for p in initial)  # generic unwraps a message from every prover in every round
    chop = (s[: 1 << rounds], t[: 1 << rounds])
    provers_gg = []
    for _ in range(rounds - 1):
        c = transcript.get_challenge(b"sumcheck-chal")
        bc = transcript.get_challenge(b"batch-chal")
        challenges.append(c)
        batch_challenges += [bc, bc * bc % R]
        fold = (X.split_fold(chop[0], c), X.split_fold(chop[1], c))
        chop = (chop[0][: (len(chop[0]) + 1) // 2], chop[1][: (len(chop[1]) + 1) // 2])
        g1fold, g2fold = X.LogProver(fold[0], chop[1]), X.LogProver(chop[0], fold[1])
        ms = [p.next_message(c) for p in initial]
        new = [g1fold.next_message(), g2fold.next_message()]
        gg = [p.next_message(c) for p in provers_gg] + new
        assert all(m is not None for m in ms + gg)
        provers_gg += [g1fold, g2fold]
        msg = tuple((sum(m[h] * x for m, x in zip(ms, w)) + sum(m[h] * x for m, x in zip(gg, batch_challenges[K3:]))) % R for h in range(2))
        transcript.append_message(b"sumcheck-round", X.gt_bytes(msg[0]) + X.gt_bytes(msg[1]))
        messages.append(msg)
    c = transcript.get_challenge(b"sumcheck-chal")
    challenges.append(c)
    finals = []
    for p in provers_gg + initial:
        p.fold(c)
        finals.append(p.final_foldings())
    assert all(f is not None for f in finals)
    k = len(provers_gg)
    return {"rounds": rounds, "messages": messages, "challenges": challenges, "batch_challenges": batch_challenges, "final_foldings": finals[:k]}, finals[k:]


def prove_literal(transcript, s, t, claims):
    """`generic` with f_ip = [(a_i, b_i)], g1_ip = [(crs.g1s, a_i)], g2_ip = [(b_i, crs.g2s)]: 3 K provers"""
    K = len(claims)
    assert K >= 1
    initial = [X.LogProver(a, b) for a, b in claims] + [X.LogProver(s, a) for a, _ in claims] + [X.LogProver(b, t) for _, b in claims]
    proof, fin = _run(transcript, s, t, K, lambda bc: (initial, _powers(bc, 3 * K)))
    proof["foldings_ff"], proof["foldings_fg1"], proof["foldings_fg2"] = fin[:K], fin[K: 2 * K], fin[2 * K:]
    return proof


def prove_collapsed(transcript, s, t, claims):
    """K FModule provers and one module prover a group, over the weighted sums of the scalar vectors"""
    K = len(claims)
    assert K >= 1
    d = len(claims[0][0])
    assert all(len(a) == d and len(b) == d for a, b in claims)

    def make_initial(bc):
        w = _powers(bc, 3 * K)
        ca = [sum(w[K + i] * claims[i][0][j] for i in range(K)) % R for j in range(d)]
        cb = [sum(w[2 * K + i] * claims[i][1][j] for i in range(K)) % R for j in range(d)]
        provers = [X.LogProver(a, b) for a, b in claims] + [X.LogProver(s, ca), X.LogProver(cb, t)]
        return provers, w[:K] + [1, 1]  # the module messages carry their weights in the scalars

    proof, fin = _run(transcript, s, t, K, make_initial)
    ff = fin[:K]
    point1, point2 = fin[K][0], fin[K + 1][1]  # the folded CRS: the same for every claim
    proof["foldings_ff"] = ff
    proof["foldings_fg1"] = [(point1, ff[i][0]) for i in range(K)]
    proof["foldings_fg2"] = [(ff[i][1], point2) for i in range(K)]
    return proof


def verify_batch(proof, vk, comm_a, comm_b, y) -> bool:
    """verify_transcript with 3 K initial claims, on logs"""
    vk1, vk2 = vk
    K = len(y)
    if not (K >= 1 and len(comm_a) == K and len(comm_b) == K and len(proof["foldings_ff"]) == K and len(proof["foldings_fg1"]) == K and len(proof["foldings_fg2"]) == K):
        return False
    ch, bch, msgs = proof["challenges"], proof["batch_challenges"], proof["messages"]
    rev = list(reversed(ch))[1:]
    g1s = [(e + o * c) % R for (e, o), c in zip(vk1, rev)][::-1] + [0]
    g2s = [(e + o * c) % R for (e, o), c in zip(vk2, rev)][::-1] + [0]
    claim = X.ip([v % R for v in y] + list(comm_a) + list(comm_b), bch[: 3 * K])
    rounds = len(msgs)
    assert rounds == len(ch)
    for i in range(rounds - 1):
        a, b = msgs[i]
        claim = (a + b * ch[i] + (claim - a) * ch[i] * ch[i] + g1s[i] * bch[3 * K + 2 * i] + g2s[i] * bch[3 * K + 2 * i + 1]) % R
    a, b = msgs[rounds - 1]
    claim = (a + b * ch[-1] + (claim - a) * ch[-1] * ch[-1]) % R
    finals = list(proof["foldings_ff"]) + list(proof["foldings_fg1"]) + list(proof["foldings_fg2"]) + list(proof["final_foldings"])
    assert len(finals) == len(bch)
    return claim == X.ip([l * r % R for l, r in finals], bch)


def statement(s, t, claims):
    """-> (comm_a, comm_b, y), lists of K logs"""
    return [X.commit(s, a) for a, _ in claims], [X.commit(t, b) for _, b in claims], [X.ip(a, b) for a, b in claims]


SHAPES = [(1, 8, 16), (2, 8, 16), (3, 5, 16), (4, 13, 32), (2, 2, 4), (3, 3, 8)]  # (K, d, n)


def claims_for(K: int, d: int, seed: int = 1, zero_a=None):
    """K deterministic claims of length d; claim `zero_a` has a = 0"""
    out = []
    x = (0x9E3779B97F4A7C15 * (seed + 1) + 0x1234567) % R
    for i in range(K):
        a, b = [], []
        for _ in range(d):
            x = (x * x + 0xB5AD4ECEDA1CE2A9 + i) % R
            a.append(x)
            x = (x * 3 + 0x2545F4914F6CDD1D) % R
            b.append(x)
        if zero_a == i:
            a = [0] * d
        out.append((a, b))
    return out
