"""TEST INFRASTRUCTURE: InnerProductProof::generic (src/herring/ipa.rs:345-531) for K claims over one CRS as the literal composition
of 3 K single provers of the library -- K FModuleTimeProver, K G1ModuleTimeProver, K G2ModuleTimeProver, every module prover folding
its own copy of the CRS, no collapse -- plus one PModuleTimeProver per folded claim, with gm_gt_mul / gm_gt_pow, gm_pairing_multi and
a transcript handle.  The byte-for-byte cross-check of gm_ipa_new_batch, which runs one module prover a group over weighted sums.

The helpers and the fold of the CRS on Python integers are those of tests/stepwise/ipa.py.
"""
import numpy as np

from gemini_amd import g2
from gemini_amd import herring
from gemini_amd import pairing as gp
from gemini_amd.fr import fr_from_int, fr_to_int
from gemini_amd.g2msm import g2_jac_to_point, g2_points_to_affine
from oracle import pyref as P
from tests.stepwise.ipa import R, _fold, _g1_jac_to_point, _g1_records, _g2_add, _ip


def new_batch(transcript, g1_points, g2_points, claims):
    """claims: [(a_i, b_i)] as integers, all of one length.
    -> the fields as limbs: rounds, messages (rounds, 2, 72), challenges, batch_challenges (lists of (4,)), final_foldings
    [((18,), (36,))], foldings_ff / fg1 / fg2 (lists of K pairs)"""
    K = len(claims)
    one = fr_from_int(1)
    G1, G2 = _g1_records([P.G1_GEN]), g2_points_to_affine([g2.generator()])
    E = gp.multi_pairing(G1, G2)
    po_fr = lambda m: (gp.gt_pow(E, fr_to_int(m[0])), gp.gt_pow(E, fr_to_int(m[1])))  # noqa: E731  scalarfieldsm_to_posm
    po_g1 = lambda m: tuple(gp.multi_pairing(_g1_records([_g1_jac_to_point(x)]), G2) for x in m)  # noqa: E731  g1sm_to_posm
    po_g2 = lambda m: tuple(gp.multi_pairing(G1, g2_points_to_affine([g2_jac_to_point(x)])) for x in m)  # noqa: E731  g2sm_to_posm
    am = [np.stack([fr_from_int(x) for x in a]) for a, _ in claims]
    bm = [np.stack([fr_from_int(x) for x in b]) for _, b in claims]
    r1, r2 = _g1_records(g1_points), g2_points_to_affine(g2_points)
    provers_ff = [herring.FModuleTimeProver(am[i], bm[i], one) for i in range(K)]
    provers_fg1 = [herring.G1ModuleTimeProver(r1, am[i], one) for i in range(K)]
    provers_fg2 = [herring.G2ModuleTimeProver(bm[i], r2, one) for i in range(K)]

    def initial_messages(vm):
        return ([po_fr(p.next_message(vm)) for p in provers_ff] + [po_g1(p.next_message(vm)) for p in provers_fg1] +
                [po_g2(p.next_message(vm)) for p in provers_fg2])

    messages, challenges = [], []
    bc = transcript.get_challenge(b"batch-chal")
    bci = fr_to_int(bc)
    batch = [pow(bci, i, R) for i in range(3 * K)]  # powers(batch_challenge, 3 K)
    batch_challenges = [fr_from_int(x) for x in batch]
    msg = _ip(initial_messages(None), batch)
    transcript.append_gt(b"prover_message", np.stack(msg))
    messages.append(msg)
    rounds = provers_ff[0].rounds()
    assert all(p.rounds() == rounds for p in provers_ff + provers_fg1 + provers_fg2)
    chop1, chop2 = list(g1_points[: 1 << rounds]), list(g2_points[: 1 << rounds])
    provers_gg = []
    for _ in range(rounds - 1):
        c = transcript.get_challenge(b"sumcheck-chal")
        bc = transcript.get_challenge(b"batch-chal")
        ci, bci = fr_to_int(c), fr_to_int(bc)
        challenges.append(c)
        batch += [bci, bci * bci % R]
        batch_challenges += [bc, fr_from_int(batch[-1])]
        fold1, fold2 = _fold(chop1, ci, P.g1_add, P.g1_mul), _fold(chop2, ci, _g2_add, g2.mul)
        chop1, chop2 = chop1[: (len(chop1) + 1) // 2], chop2[: (len(chop2) + 1) // 2]
        g1fold = herring.PModuleTimeProver(_g1_records(fold1), g2_points_to_affine(chop2), one)
        g2fold = herring.PModuleTimeProver(_g1_records(chop1), g2_points_to_affine(fold2), one)
        msgs = initial_messages(c)
        new_msgs = [g1fold.next_message(), g2fold.next_message()]
        msgs += [p.next_message(c) for p in provers_gg] + new_msgs
        provers_gg += [g1fold, g2fold]
        msg = _ip(msgs, batch)
        transcript.append_gt(b"sumcheck-round", np.stack(msg))
        messages.append(msg)
    c = transcript.get_challenge(b"sumcheck-chal")
    challenges.append(c)
    finals = []
    for p in provers_gg + provers_ff + provers_fg1 + provers_fg2:
        p.fold(c)
        finals.append(p.final_foldings())
        p.free()
    k = len(provers_gg)
    return {"rounds": rounds, "messages": np.array(messages), "challenges": challenges, "batch_challenges": batch_challenges, "final_foldings": finals[:k],
            "foldings_ff": finals[k: k + K], "foldings_fg1": finals[k + K: k + 2 * K], "foldings_fg2": finals[k + 2 * K:]}
