"""TEST INFRASTRUCTURE: InnerProductProof::new (src/herring/ipa.rs:533-685) as the literal composition of the module provers the
library already had -- FModuleTimeProver, G1ModuleTimeProver, G2ModuleTimeProver, one PModuleTimeProver per folded claim -- with
gm_gt_mul / gm_gt_pow, gm_pairing_multi and a transcript handle: one FFI call per step, two Miller products and two final
exponentiations per PModule prover and round.  The byte-for-byte cross-check of gm_ipa_new's batched kernels, and the baseline of
tools/ipa_bench.py.

The folded CRS of step 2b (Crs::fold, ipa.rs:203-212) is the witness of a NEW prover and has no entry point of its own in the
per-prover path; it is folded here on Python integers (oracle/pyref.py, gemini_amd/g2.py).
"""
import time

import numpy as np

from gemini_amd import g2
from gemini_amd import herring
from gemini_amd import pairing as gp
from gemini_amd.fr import fr_from_int, fr_to_int
from gemini_amd.g2msm import g2_jac_to_point, g2_points_to_affine
from oracle import pyref as P

R = P.R_MOD


def _g1_records(points) -> np.ndarray:
    from gemini_amd.g2msm import _fq_limbs

    out = np.zeros((len(points), 12), dtype=np.uint64)
    for i, p in enumerate(points):
        if p is not None:
            out[i] = _fq_limbs(p[0]) + _fq_limbs(p[1])
    return out


def _g1_jac_to_point(jac):
    from gemini_amd.g2msm import _fq_int

    X, Y, Z = (_fq_int(r) for r in np.asarray(jac).reshape(3, 6))
    if Z == 0:
        return None
    zi = pow(Z, -1, P.Q_MOD)
    return (X * zi * zi % P.Q_MOD, Y * zi * zi * zi % P.Q_MOD)


def _g2_add(p, q):
    from tests import g2_ref

    return g2_ref.add(p, q)


def _fold(points, c, add, mul):
    """Crs::fold on one group: out[i] = p[2i] + c p[2i+1]"""
    return [add(points[i], mul(points[i + 1], c)) if i + 1 < len(points) else points[i] for i in range(0, len(points), 2)]


def _ip(messages, scalars):
    """SumcheckMsg::ip over GT (prover.rs:35-43): zip, fold from the identity"""
    a, b = gp.gt_one(), gp.gt_one()
    for (ma, mb), s in zip(messages, scalars):
        a, b = gp.gt_mul(a, gp.gt_pow(ma, s)), gp.gt_mul(b, gp.gt_pow(mb, s))
    return a, b


def new(transcript, g1_points, g2_points, a, b, timers=None):
    """timers: a dict whose "fold_s" collects the seconds spent folding the CRS on Python integers (tools/ipa_bench.py takes them
    out of the baseline).
    -> the fields of the proof as limbs: rounds, messages (rounds, 2, 72), challenges, batch_challenges (lists of (4,)),
    final_foldings [((18,), (36,))], foldings_ff / fg1 / fg2.  g1_points / g2_points: the CRS as integer points, a / b: integers"""
    one = fr_from_int(1)
    G1, G2 = _g1_records([P.G1_GEN]), g2_points_to_affine([g2.generator()])
    E = gp.multi_pairing(G1, G2)
    po_fr = lambda m: (gp.gt_pow(E, fr_to_int(m[0])), gp.gt_pow(E, fr_to_int(m[1])))  # noqa: E731  scalarfieldsm_to_posm
    po_g1 = lambda m: tuple(gp.multi_pairing(_g1_records([_g1_jac_to_point(x)]), G2) for x in m)  # noqa: E731  g1sm_to_posm
    po_g2 = lambda m: tuple(gp.multi_pairing(G1, g2_points_to_affine([g2_jac_to_point(x)])) for x in m)  # noqa: E731  g2sm_to_posm
    am, bm = np.stack([fr_from_int(x) for x in a]), np.stack([fr_from_int(x) for x in b])
    prover_ff = herring.FModuleTimeProver(am, bm, one)
    prover_fg1 = herring.G1ModuleTimeProver(_g1_records(g1_points), am, one)
    prover_fg2 = herring.G2ModuleTimeProver(bm, g2_points_to_affine(g2_points), one)
    messages, challenges, batch_challenges = [], [], []
    bc = transcript.get_challenge(b"batch-chal")
    bci = fr_to_int(bc)
    batch = [1, bci, bci * bci % R]
    batch_challenges += [one, bc, fr_from_int(batch[2])]
    msg = _ip([po_fr(prover_ff.next_message()), po_g1(prover_fg1.next_message()), po_g2(prover_fg2.next_message())], batch)
    transcript.append_gt(b"prover_message", np.stack(msg))
    messages.append(msg)
    rounds = prover_ff.rounds()
    assert rounds == prover_fg1.rounds() == prover_fg2.rounds()
    chop1, chop2 = list(g1_points[: 1 << rounds]), list(g2_points[: 1 << rounds])
    provers_gg = []
    for _ in range(rounds - 1):
        c = transcript.get_challenge(b"sumcheck-chal")
        bc = transcript.get_challenge(b"batch-chal")
        ci, bci = fr_to_int(c), fr_to_int(bc)
        challenges.append(c)
        batch += [bci, bci * bci % R]
        batch_challenges += [bc, fr_from_int(batch[-1])]
        t0 = time.perf_counter()
        fold1, fold2 = _fold(chop1, ci, P.g1_add, P.g1_mul), _fold(chop2, ci, _g2_add, g2.mul)
        if timers is not None:
            timers["fold_s"] = timers.get("fold_s", 0.0) + time.perf_counter() - t0
        chop1, chop2 = chop1[: (len(chop1) + 1) // 2], chop2[: (len(chop2) + 1) // 2]
        g1fold = herring.PModuleTimeProver(_g1_records(fold1), g2_points_to_affine(chop2), one)
        g2fold = herring.PModuleTimeProver(_g1_records(chop1), g2_points_to_affine(fold2), one)
        msgs = [po_fr(prover_ff.next_message(c)), po_g1(prover_fg1.next_message(c)), po_g2(prover_fg2.next_message(c))]
        new_msgs = [g1fold.next_message(), g2fold.next_message()]
        msgs += [p.next_message(c) for p in provers_gg] + new_msgs
        provers_gg += [g1fold, g2fold]
        msg = _ip(msgs, batch)
        transcript.append_gt(b"sumcheck-round", np.stack(msg))
        messages.append(msg)
    c = transcript.get_challenge(b"sumcheck-chal")
    challenges.append(c)
    finals = []
    for p in provers_gg + [prover_ff, prover_fg1, prover_fg2]:
        p.fold(c)
        finals.append(p.final_foldings())
        p.free()
    return {"rounds": rounds, "messages": np.array(messages), "challenges": challenges, "batch_challenges": batch_challenges, "final_foldings": finals[:-3],
            "foldings_ff": finals[-3], "foldings_fg1": finals[-2], "foldings_fg2": finals[-1]}
