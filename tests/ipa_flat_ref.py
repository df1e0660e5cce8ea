"""The stated form of `InnerProductProof::verify_transcript` (src/herring/ipa.rs:250-343) on Python integers (test infrastructure).

verify_transcript is linear in the claim: round i maps claim -> a_i + b_i ch_i + (claim - a_i) ch_i^2 (+ the folded verifier key).
Unrolled over the R rounds, with w[i] = prod_{j > i} ch[j]^2 (w[R - 1] = 1) and W = w[0] ch[0]^2, "claim == expected" is ONE
relation: the sum of log x exponent over the terms below is 0 mod r.  gemini_amd/csrc/ipa.hip (ipa_state) states the same exponents
in C++, in the same order, and gm_ipa_verify_many evaluates the relation as one product in GT.

  GT terms, 6 R - 4        for every round i:          a_i ^ ((1 - ch_i^2) w_i),  b_i ^ (ch_i w_i)
                           for every round i < R - 1, level l = R - 2 - i of the Vrs:
                                                       vk1_even[l] ^ (bch[3+2i] w_i), vk1_odd[l] ^ (bch[3+2i] w_i ch_i),
                                                       vk2_even[l] ^ (bch[4+2i] w_i), vk2_odd[l] ^ (bch[4+2i] w_i ch_i)
  pairing terms, 2 R + 4   e(G1, G2) ^ (y bch0 W), e(comm_a, G2) ^ (bch1 W), e(G1, comm_b) ^ (bch2 W),
                           e(G1, G2) ^ (-ff.lhs ff.rhs bch0), e(fg1.f0, G2) ^ (-fg1.g0 bch1), e(G1, fg2.g0) ^ (-fg2.f0 bch2),
                           e(lhs_p, rhs_p) ^ (-bch[3+p]) for each of the 2 (R - 1) final foldings

A proof is the dict of logs of tests/ipa_exponent_ref.py, whose `verify` is the round-by-round statement this one is held against.
"""
from tests.ipa_exponent_ref import R


def exponents(proof, y: int):
    """-> (the 6 R - 4 exponents of the GT terms, the 2 R + 4 exponents of the pairing terms), canonical, in the order above"""
    ch, bch = proof["challenges"], proof["batch_challenges"]
    rounds = len(ch)
    w = [1] * rounds
    for i in range(rounds - 2, -1, -1):
        w[i] = w[i + 1] * ch[i + 1] * ch[i + 1] % R
    W = w[0] * ch[0] * ch[0] % R
    gt = []
    for i in range(rounds):
        gt += [(1 - ch[i] * ch[i]) * w[i] % R, ch[i] * w[i] % R]
    for i in range(rounds - 1):
        for v in range(2):
            e = bch[3 + 2 * i + v] * w[i] % R
            gt += [e, e * ch[i] % R]
    ff, fg1, fg2 = proof["foldings_ff"], proof["foldings_fg1"], proof["foldings_fg2"]
    pair = [y * bch[0] * W % R, bch[1] * W % R, bch[2] * W % R, -ff[0] * ff[1] * bch[0] % R, -fg1[1] * bch[1] % R, -fg2[0] * bch[2] % R]
    pair += [-bch[3 + p] % R for p in range(2 * (rounds - 1))]
    return gt, pair


def logs(proof, vk, comm_a: int, comm_b: int):
    """the logs (to the base E = e(G1, G2)) of the elements the exponents above belong to, in the same order"""
    vk1, vk2 = vk
    rounds = len(proof["challenges"])
    assert len(vk1) >= rounds - 1 and len(vk2) >= rounds - 1, "the Vrs is too shallow for this proof"
    gt = []
    for a, b in proof["messages"]:
        gt += [a, b]
    for i in range(rounds - 1):
        l = rounds - 2 - i
        gt += [vk1[l][0], vk1[l][1], vk2[l][0], vk2[l][1]]
    pair = [1, comm_a, comm_b, 1, proof["foldings_fg1"][0], proof["foldings_fg2"][1]] + [lhs * rhs % R for lhs, rhs in proof["final_foldings"]]
    return gt, pair


def verify(proof, vk, comm_a: int, comm_b: int, y: int) -> bool:
    ge, pe = exponents(proof, y)
    gl, pl = logs(proof, vk, comm_a, comm_b)
    assert len(ge) == len(gl) and len(pe) == len(pl)
    return (sum(x * e for x, e in zip(gl, ge)) + sum(x * e for x, e in zip(pl, pe))) % R == 0
