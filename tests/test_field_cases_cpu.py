"""CPU: the case lists and the comparison code of tests/test_gpu_field_ops.py and tests/test_gpu_group_ops.py do what they say --
without a GPU.  The generator's interpreter stands in for the device on a few lanes of every kind, so the checks that the GPU
tests apply are seen to accept the right result and to reject a subtly wrong one; the committed false-positive vectors are seen to
visit the cold block of their statement and to leave it as ordinary lanes."""
import numpy as np
import pytest

from gemini_amd import debug as D
from oracle import pyref
from tests import acc30_cases as ac
from tests import field_cases as fc
from tests.test_gpu_field_ops import same
from tests.test_gpu_group_ops import g1_cases, g1_expected, g2_cases, g2_expected

Q = fc.Q


def test_the_comparison_rejects_a_wrong_product():
    """an expected value off by q in one lane, or by one bit in one limb, is a failure"""
    want = D.rows_words([fc.mm(3, 5), fc.mm(7, 9)])
    same(want.copy(), want, ["a", "b"])
    for wrong in (D.rows_words([fc.mm(3, 5), fc.mm(7, 9) + Q]), want ^ np.eye(2, 12, 7, dtype=np.uint32)):
        with pytest.raises(AssertionError):
            same(wrong, want, ["a", "b"])


def test_solved_pairs_hit_the_conditional_subtraction():
    """the solved pairs fall on both sides of the subtraction's edge: 74 of the 300 leave the raw product in [q, 1.002 q), the others
    below q with a canonical result under q / 512"""
    solved = [(a, b) for n, a, b in fc.FQ_PAIRS if n.startswith("solved")]
    above = sum(1 for a, b in solved if fc.mont_quotient(a, b) >= Q)
    assert len(solved) == 300 and 50 <= above <= 250, above
    assert all(fc.mm(a, b) < Q >> 9 for a, b in solved)


def test_the_lists_are_what_the_functions_accept():
    assert all(a < Q and b < Q for _, a, b in fc.FQ_PAIRS)
    assert all(a < fc.LOOSE_LIMIT and b < fc.LOOSE_LIMIT for _, a, b in fc.LOOSE_PAIRS)
    assert fc.mm(fc.ONE, fc.ONE) == fc.ONE and fc.val(fc.ONE) == 1
    # the constants of field30.cuh, spelled there as limbs
    assert fc.mm(fc.dev(5) * pow(64, -1, Q) % Q, fc.CIN) == fc.dev(5) and fc.mm(fc.dev(5), fc.COUT) == fc.dev(5) * pow(64, -1, Q) % Q
    borrows = [(a, b) for n, a, b in fc.FQ_PAIRS if n.startswith("borrow")]
    assert len(borrows) == 9
    for a, b in borrows:
        assert all(((a >> (32 * i)) & 0xFFFFFFFF) < ((b >> (32 * i)) & 0xFFFFFFFF) for i in range(12))


def test_quotient_is_what_the_generator_asserts():
    """fc.mont_quotient against the interpreted loose product, on the extreme pairs (the GPU test compares the device with the former)"""
    import sys

    sys.path.insert(0, ac.CSRC)
    try:
        import gen_field_mul30 as g
    finally:
        sys.path.pop(0)
    p = g.gen(False, loose=True)
    for a, b in ((fc.LOOSE_LIMIT - 1, fc.LOOSE_LIMIT - 1), (10 * Q, 10 * Q - 1), (Q - 1, 1), (0, fc.LOOSE_LIMIT - 1)):
        regs = {f"v{i}": 0 for i in range(72)}
        regs.update({f"s{i}": 0 for i in range(32)})
        for i, (x, y) in enumerate(zip(D.limbs30(a), D.limbs30(b))):
            regs[f"v{i}"], regs[f"v{13 + i}"] = x, y
        p.run(regs)
        assert D.limbs30(fc.mont_quotient(a, b)) == [regs[f"v{i}"] for i in range(13)]


# ---- the Acc30 lanes: the interpreter in the device's place ----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["madd", "add"])
def test_committed_false_positives_visit_the_cold_block(which):
    fps = ac.false_positives()[which]
    assert len(fps) >= 8 and {e["low_limb"] for e in fps} == {"q0", "0"}
    for e in fps:
        assert all(v < m * Q for v, m in zip(e["acc"], ac.MULT))
        out, cold, exceptional = ac.interpret(which, e["acc"], e["other"], e["neg"])
        assert cold and not exceptional
        assert tuple(v % Q for v in out) == tuple(ac.model(which, e["acc"], e["other"], e["neg"]))


@pytest.mark.parametrize("which", ["madd", "add"])
def test_ordinary_lanes_do_not_visit_the_cold_block_and_exceptional_ones_do(which):
    lanes = ac.build(which, ["ordinary", "ordinary!", "double", "cancel"], seed=5)
    seen = [ac.interpret(which, l["acc"], l["other"], l["neg"])[1:] for l in lanes]
    assert seen == [(False, False), (False, False), (True, True), (True, True)]


@pytest.mark.parametrize("which", ["madd", "add"])
def test_lane_check_accepts_the_interpreter_and_rejects_a_wrong_law(which):
    """every kind of lane through check_lane with the interpreter's output; then the same with one thing wrong at a time"""
    bnd = ac.bounds(which)
    kinds = ["ordinary", "ordinary!", "fp"] + [k for k in ac.EXCEPTIONAL[which]] + [k + "!" for k in ac.EXCEPTIONAL[which] if "identity" not in k]
    lanes = ac.build(which, kinds * 3, seed=9)
    outs = []
    for lane in lanes:
        out, _, _ = ac.interpret(which, lane["acc"], lane["other"], lane["neg"])
        canon = (0, 0, 0, 0) if out[2] == 0 else tuple(v % Q for v in out)
        ac.check_lane(which, lane, out, canon, bnd)
        outs.append((out, canon))
    rejected = 0
    for lane, (out, canon) in zip(lanes, outs):
        wrong = []
        if lane["kind"] == "ordinary":  # the sign of the base swapped: the model's P - B in the place of P + B
            wrong.append((dict(lane, point=pyref.g1_neg(lane["point"])), out, canon))
        if lane["kind"] == "double":    # doubling answered as cancellation
            wrong.append((lane, (out[0], out[1], 0, out[3]), (0, 0, 0, 0)))
        if lane["kind"] == "cancel":    # ZZ = q in the place of ZZ = 0: the same residue, not the identity's encoding
            wrong.append((lane, (out[0], out[1], Q, out[3]), canon))
        if lane["kind"] == "fp":        # the lane left as an exceptional one
            wrong.append((lane, (out[0], out[1], 0, out[3]), canon))
        if out[2] != 0:
            wrong.append((lane, (out[0] + 7 * Q, out[1], out[2], out[3]), canon))           # the right residue beyond its bound
            wrong.append((lane, out, (canon[0], canon[1] ^ 1, canon[2], canon[3])))          # acc30_to_canonical off by a bit
            wrong.append((lane, (out[0], (out[1] + 1) % Q, out[2], out[3]), canon))          # off the curve
        for args in wrong:
            with pytest.raises(AssertionError):
                ac.check_lane(which, *args, bnd)
            rejected += 1
    assert rejected > 40


@pytest.mark.parametrize("which", ["madd", "add"])
def test_waves_state_their_composition(which):
    names = [n for n, _ in ac.waves(which)]
    for must in ("all ordinary", "all double", "all cancel", "all identity", "one double lane at lane 0", "one cancel lane at lane 63", "interleaved",
                 "false positives beside ordinary and exceptional lanes"):
        assert must in names
    w = dict(ac.waves(which))
    assert w["one identity lane at lane 63"][63] == "identity" and set(w["one identity lane at lane 63"][:63]) == {"ordinary"}
    assert {"double", "cancel", "identity", "ordinary"} <= set(w["interleaved"])


# ---- the canonical group law: the reference against itself ---------------------------------------------------------------------------------------
def test_g1_case_kinds_and_expectations():
    kinds = {c["kind"] for c in g1_cases()}
    assert kinds == {"generic", "equal", "negatives", "identity + Q", "P + identity", "identity + identity"}
    for c in g1_cases():
        P, B = fc.g1_point_of(c["acc"]), c["B"]
        assert g1_expected(c) == pyref.g1_add(P, B)
        if c["kind"] == "equal":
            assert P == B and c["acc"][2] != fc.ONE  # a non-trivial representation
        if c["kind"] == "negatives":
            assert g1_expected(c) is None


def test_g2_case_kinds_and_expectations():
    from tests import g2_ref

    kinds = {c["kind"] for c in g2_cases()}
    assert kinds == {"generic", "equal", "negatives", "identity + Q", "P + identity", "identity + identity"}
    for c in g2_cases():
        assert g2_expected(c) == g2_ref.add(fc.g2_point_of(c["acc"]), c["B"])
