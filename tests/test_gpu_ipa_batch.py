"""GPU: gm_ipa_new_batch and gm_ipa_verify_batch -- ONE inner-product proof for K claims over the same CRS (gemini_amd/csrc/ipa.hip:
ipa_prove_batch, ipa_verify_batch) -- against the exponent oracle of tests/ipa_batch_ref.py, against the literal 3 K-prover
composition of tests/stepwise/ipa_generic.py, and, for K = 1, against gm_ipa_new.

Shapes (K, d, n): d = 2 has one round and no PModule prover; 3, 5 and 13 are no powers of two (odd tails on the Fr side and in the
sums the module provers run on); K = 4 at d = 64 has Miller segments of 16 .. 1 pairs with several provers live; K = 23 crosses the
22-prover launch split of the multi-prover sumcheck round.  One claim of every K > 1 case has a = 0, so its comm_a is the identity.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from gemini_amd import pairing as gp
from gemini_amd.fr import fr_from_int, fr_to_int
from gemini_amd.g2msm import g2_jac_to_point, g2_points_to_affine
from oracle import pyref as P
from tests import ipa_batch_ref as B
from tests import ipa_exponent_ref as X
from tests.test_gpu_pairing import g1_jac_to_point, g1_points_to_affine

pytestmark = pytest.mark.gpu

R = X.R
GM_EINVAL, GM_EHANDLE, GM_ENOMEM = -1, -3, -5
LABEL = b"gemini-tests"
CASES = [(K, d, n, ()) for K, d, n in B.SHAPES] + [(2, 8, 16, (3,))]
IDS = [f"K{K}-d{d}-n{n}" + ("-inf" if inf else "") for K, d, n, inf in CASES]


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


def mont(v) -> np.ndarray:
    return np.stack([fr_from_int(x) for x in v])


@functools.lru_cache(maxsize=None)
def reference(K: int, d: int, n: int, inf=()):
    """the inputs and the oracle's proof of one case: computed once, never modified"""
    p1, s, p2, t = X.crs(n, infinity_at=inf)
    claims = B.claims_for(K, d, seed=K * 100 + d, zero_a=K - 1 if K > 1 else None)
    tr = P.GeminiTranscript(LABEL)
    proof = B.prove_collapsed(tr, s, t, claims)
    ca, cb, y = B.statement(s, t, claims)
    return {"s": s, "t": t, "claims": claims, "r1": g1_points_to_affine(p1, flag=bool(inf)), "r2": g2_points_to_affine(p2, flag=bool(inf)), "proof": proof,
            "next": tr.get_challenge(b"next"), "comm_a": ca, "comm_b": cb, "y": y, "vk": X.vrs(s, t), "a_mont": [mont(a) for a, _ in claims],
            "b_mont": [mont(b) for _, b in claims]}


def statement_on_device(crs, ref):
    """-> (comm_a (K, 18), comm_b (K, 36), y (K, 4)) through the library's commitments"""
    return (np.stack([crs.commit_g1(a) for a in ref["a_mont"]]), np.stack([crs.commit_g2(b) for b in ref["b_mont"]]), np.stack([fr_from_int(v) for v in ref["y"]]))


def assert_fields_equal(f, exp, K):
    """the K-long fields of a device proof against the oracle's logs"""
    k = exp["rounds"]
    assert f.rounds == k and f.claims == K
    assert [fr_to_int(c) for c in f.challenges] == exp["challenges"]
    assert [fr_to_int(c) for c in f.batch_challenges] == exp["batch_challenges"] and len(f.batch_challenges) == 3 * K + 2 * (k - 1)
    for i, (a, b) in enumerate(exp["messages"]):
        assert gp.gt_to_ints(f.messages[i, 0]) == X.gt_ints(a), ("message a", i)
        assert gp.gt_to_ints(f.messages[i, 1]) == X.gt_ints(b), ("message b", i)
    assert len(f.final_lhs) == len(f.final_rhs) == len(exp["final_foldings"]) == 2 * (k - 1)
    for p, (l, r) in enumerate(exp["final_foldings"]):
        assert g1_jac_to_point(f.final_lhs[p]) == X.g1_point(l), ("final lhs", p)
        assert g2_jac_to_point(f.final_rhs[p]) == X.g2_point(r), ("final rhs", p)
    for i in range(K):
        assert (fr_to_int(f.foldings_ff[i, 0]), fr_to_int(f.foldings_ff[i, 1])) == exp["foldings_ff"][i], ("ff", i)
        l, r = exp["foldings_fg1"][i]
        assert (g1_jac_to_point(f.foldings_fg1[0][i]), fr_to_int(f.foldings_fg1[1][i])) == (X.g1_point(l), r), ("fg1", i)
        l, r = exp["foldings_fg2"][i]
        assert (fr_to_int(f.foldings_fg2[0][i]), g2_jac_to_point(f.foldings_fg2[1][i])) == (l, X.g2_point(r)), ("fg2", i)


@pytest.mark.parametrize("K,d,n,inf", CASES, ids=IDS)
def test_bytes_against_the_exponent_oracle(gm, K, d, n, inf):
    """messages, points, scalars, batch challenges and the transcript afterwards; then the verifier on the result"""
    ref = reference(K, d, n, inf)
    crs, tr = gm.Crs(ref["r1"], ref["r2"]), gm.Transcript(LABEL)
    proof = gm.InnerProductProof.new_batch(tr, crs, ref["a_mont"], ref["b_mont"])
    assert proof.claims == K
    assert_fields_equal(proof.batch_fields(), ref["proof"], K)
    assert fr_to_int(tr.get_challenge(b"next")) == ref["next"]
    vrs = gm.Vrs(crs)
    ca, cb, y = statement_on_device(crs, ref)
    for i in range(K):
        assert g1_jac_to_point(ca[i]) == X.g1_point(ref["comm_a"][i]) and g2_jac_to_point(cb[i]) == X.g2_point(ref["comm_b"][i])
    assert proof.verify_batch(vrs, ca, cb, y)
    assert proof.check_points().ok and proof.check_messages().ok
    for o in (proof, vrs, tr, crs):
        o.free()


@pytest.mark.parametrize("K,d,n", [(2, 8, 16), (3, 5, 16), (4, 64, 128)])
def test_bytes_against_the_literal_composition(gm, K, d, n):
    """3 K single provers of the library, every module prover folding its own copy of the CRS: the same bytes in every field"""
    from tests.stepwise import ipa_generic as steps

    p1, _, p2, _ = X.crs(n)
    claims = B.claims_for(K, d, seed=7 * K + d)
    t_steps, t_lib = gm.Transcript(LABEL), gm.Transcript(LABEL)
    exp = steps.new_batch(t_steps, p1, p2, claims)
    crs = gm.Crs(g1_points_to_affine(p1), g2_points_to_affine(p2))
    proof = gm.InnerProductProof.new_batch(t_lib, crs, [mont(a) for a, _ in claims], [mont(b) for _, b in claims])
    f = proof.batch_fields()
    assert f.rounds == exp["rounds"] == X.ceil_log2(d)
    assert f.messages.tobytes() == exp["messages"].tobytes()
    assert f.challenges.tobytes() == np.stack(exp["challenges"]).tobytes()
    assert f.batch_challenges.tobytes() == np.stack(exp["batch_challenges"]).tobytes()
    assert len(exp["final_foldings"]) == 2 * (f.rounds - 1)
    for p, (l, r) in enumerate(exp["final_foldings"]):
        assert f.final_lhs[p].tobytes() == l.tobytes() and f.final_rhs[p].tobytes() == r.tobytes(), p
    for i in range(K):
        assert f.foldings_ff[i].tobytes() == np.stack(exp["foldings_ff"][i]).tobytes(), i
        assert f.foldings_fg1[0][i].tobytes() == exp["foldings_fg1"][i][0].tobytes() and f.foldings_fg1[1][i].tobytes() == exp["foldings_fg1"][i][1].tobytes(), i
        assert f.foldings_fg2[0][i].tobytes() == exp["foldings_fg2"][i][0].tobytes() and f.foldings_fg2[1][i].tobytes() == exp["foldings_fg2"][i][1].tobytes(), i
    assert t_lib.challenge_bytes(b"next", 32) == t_steps.challenge_bytes(b"next", 32)
    for o in (proof, crs, t_lib, t_steps):
        o.free()


@pytest.mark.parametrize("d,n", [(8, 16), (64, 128)])
def test_one_claim_is_gm_ipa_new(gm, d, n):
    """equal in every field and in the transcript afterwards; accepted by gm_ipa_verify and gm_ipa_verify_many; the single-claim
    getters answer as for gm_ipa_new's proof"""
    from tests.test_gpu_ipa_new_many import fields_equal

    p1, _, p2, _ = X.crs(n)
    (a, b), = B.claims_for(1, d, seed=900 + d)
    crs = gm.Crs(g1_points_to_affine(p1), g2_points_to_affine(p2))
    t1, t2 = gm.Transcript(LABEL), gm.Transcript(LABEL)
    single = gm.InnerProductProof.new(t1, crs, mont(a), mont(b))
    batch = gm.InnerProductProof.new_batch(t2, crs, [mont(a)], [mont(b)])
    assert batch.claims == 1 and single.claims == 1
    assert fields_equal(batch.fields(), single.fields())
    assert t1.challenge_bytes(b"next", 32) == t2.challenge_bytes(b"next", 32)
    vrs = gm.Vrs(crs)
    ca, cb, y = crs.commit_g1(mont(a)), crs.commit_g2(mont(b)), fr_from_int(X.ip(a, b))
    assert batch.verify_transcript(vrs, ca, cb, y) and not batch.verify_transcript(vrs, ca, cb, fr_from_int((X.ip(a, b) + 1) % R))
    assert gm.InnerProductProof.verify_many([batch, single], vrs, [ca, ca], [cb, cb], [y, y]) == [True, True]
    assert batch.verify_batch(vrs, [ca], [cb], [y]) and single.verify_batch(vrs, [ca], [cb], [y])
    assert batch.host_times()["call_ms"] > 0
    for o in (batch, single, vrs, t1, t2, crs):
        o.free()


def _single_claim_getters(gm, proof):
    """gm_ipa_foldings_ff / _fg1 / _fg2 -> their three return codes and (ff (8,), fg1 (22,), fg2 (40,))"""
    lib, ptr, h = gm.capi.load(), gm.capi.ptr, C.c_uint64(proof.handle)
    ff, fg1, fg2 = (np.zeros(w, dtype=np.uint64) for w in (8, 22, 40))
    codes = (lib.gm_ipa_foldings_ff(h, ptr(ff)), lib.gm_ipa_foldings_fg1(h, ptr(fg1), ptr(fg1[18:])), lib.gm_ipa_foldings_fg2(h, ptr(fg2), ptr(fg2[4:])))
    return codes, (ff, fg1, fg2)


def _foldings_batch(gm, proof, K):
    """gm_ipa_foldings_batch -> ff (K, 8), fg1 (K, 22), fg2 (K, 40)"""
    out = tuple(np.zeros((K, w), dtype=np.uint64) for w in (8, 22, 40))
    gm.capi.check(gm.capi.load().gm_ipa_foldings_batch(C.c_uint64(proof.handle), *(gm.capi.ptr(x) for x in out)))
    return out


@pytest.mark.parametrize("d,n", [(2, 4), (5, 16)])
def test_one_claim_has_one_storage(gm, d, n):
    """a proof of gm_ipa_new and one of gm_ipa_new_batch at K = 1, each rebuilt through from_fields(fields()) and through
    from_fields_batch(batch_fields()): the same bytes from fields() and from batch_fields() whichever way a proof was made, the
    single-claim getters are row 0 of gm_ipa_foldings_batch, and every verifier and check accepts every one.  d = 2 has one round,
    no PModule prover and empty final foldings; d = 5 has three rounds and odd tails."""
    from tests.test_gpu_ipa_new_many import fields_equal

    p1, _, p2, _ = X.crs(n)
    (a, b), = B.claims_for(1, d, seed=1200 + d)
    crs = gm.Crs(g1_points_to_affine(p1), g2_points_to_affine(p2))
    t1, t2 = gm.Transcript(LABEL), gm.Transcript(LABEL)
    IP = gm.InnerProductProof
    made = [IP.new(t1, crs, mont(a), mont(b)), IP.new_batch(t2, crs, [mont(a)], [mont(b)])]
    rebuilt = [q for p in made for q in (IP.from_fields(p.fields()), IP.from_fields_batch(p.batch_fields()))]
    f0, b0 = rebuilt[0].fields(), rebuilt[0].batch_fields()
    k = 2 * (X.ceil_log2(d) - 1)
    assert f0.rounds == X.ceil_log2(d) and f0.final_lhs.shape == (k, 18) and f0.final_rhs.shape == (k, 36) and f0.batch_challenges.shape == (3 + k, 4)
    assert f0.foldings_ff.shape == (2, 4) and [x.shape for x in f0.foldings_fg1 + f0.foldings_fg2] == [(18,), (4,), (4,), (36,)]
    assert b0.foldings_ff.shape == (1, 2, 4) and [x.shape for x in b0.foldings_fg1 + b0.foldings_fg2] == [(1, 18), (1, 4), (1, 4), (1, 36)]
    vrs = gm.Vrs(crs)
    ca, cb, y = crs.commit_g1(mont(a)), crs.commit_g2(mont(b)), fr_from_int(X.ip(a, b))
    for i, p in enumerate(made + rebuilt):
        assert p.claims == 1, i
        assert fields_equal(p.fields(), f0) and fields_equal(p.batch_fields(), b0), i
        codes, single = _single_claim_getters(gm, p)
        assert codes == (0, 0, 0), i
        for one, rows in zip(single, _foldings_batch(gm, p, 1)):
            assert one.tobytes() == rows[0].tobytes(), i
        assert single[0].tobytes() == f0.foldings_ff.tobytes() and single[1].tobytes() == np.concatenate(f0.foldings_fg1).tobytes(), i
        assert single[2].tobytes() == np.concatenate(f0.foldings_fg2).tobytes(), i
        assert p.verify_transcript(vrs, ca, cb, y) and p.verify_batch(vrs, [ca], [cb], [y]), i
        assert p.check_points().ok and p.check_messages().ok, i
    for o in made + rebuilt + [vrs, t1, t2, crs]:
        o.free()


def test_three_claims_round_trip(gm):
    """K = 3 at d = 5 through from_fields_batch(batch_fields()): the same bytes, and the single-claim getters refuse both proofs"""
    from tests.test_gpu_ipa_new_many import fields_equal

    K = 3
    ref = reference(K, 5, 16)
    crs, tr = gm.Crs(ref["r1"], ref["r2"]), gm.Transcript(LABEL)
    proof = gm.InnerProductProof.new_batch(tr, crs, ref["a_mont"], ref["b_mont"])
    rebuilt = gm.InnerProductProof.from_fields_batch(proof.batch_fields())
    f = proof.batch_fields()
    assert f.claims == K and f.foldings_ff.shape == (K, 2, 4) and f.batch_challenges.shape == (3 * K + 4, 4)
    for p in (proof, rebuilt):
        assert p.claims == K
        assert fields_equal(p.batch_fields(), f) and fields_equal(p.fields(), f)
        assert _single_claim_getters(gm, p)[0] == (GM_EINVAL, GM_EINVAL, GM_EINVAL)
        for rows, exp in zip(_foldings_batch(gm, p, K), (f.foldings_ff.reshape(K, 8), np.concatenate(f.foldings_fg1, axis=1), np.concatenate(f.foldings_fg2, axis=1))):
            assert rows.tobytes() == exp.tobytes()
    for o in (proof, rebuilt, tr, crs):
        o.free()


def _oracle_with(exp, **changes):
    bad = copy.deepcopy(exp)
    bad.update(changes)
    return bad


@pytest.mark.parametrize("K,d,n", [(3, 5, 16), (2, 2, 4)])
def test_verify_batch_verdicts_equal_the_oracle(gm, K, d, n):
    """accepts; rejects each single alteration -- y_i, swapped comm_a, swapped comm_b, a message, a folding scalar, a folding point, a
    batch challenge; accepts the one alteration the oracle accepts (ff.rhs of the claim with a = 0: its lhs is 0); a proof rebuilt
    by from_fields_batch gets the same verdict.  The identity commitment of the claim with a = 0 goes through."""
    ref = reference(K, d, n)
    exp, vk = ref["proof"], ref["vk"]
    crs, tr = gm.Crs(ref["r1"], ref["r2"]), gm.Transcript(LABEL)
    proof = gm.InnerProductProof.new_batch(tr, crs, ref["a_mont"], ref["b_mont"])
    vrs = gm.Vrs(crs)
    ca, cb, y = statement_on_device(crs, ref)
    oca, ocb, oy = ref["comm_a"], ref["comm_b"], ref["y"]
    assert not ca[K - 1][12:].any()  # a = 0: the commitment is the identity
    verdicts = []

    def both(device_proof, oracle_proof, dev_stmt, log_stmt, what):
        got = device_proof.verify_batch(vrs, *dev_stmt)
        assert got == B.verify_batch(oracle_proof, vk, *log_stmt), what
        verdicts.append((what, got))
        return got

    assert both(proof, exp, (ca, cb, y), (oca, ocb, oy), "honest")
    rebuilt = gm.InnerProductProof.from_fields_batch(proof.batch_fields())
    assert rebuilt.claims == K and both(rebuilt, exp, (ca, cb, y), (oca, ocb, oy), "rebuilt")
    rebuilt.free()
    for i in range(K):
        y2, oy2 = y.copy(), list(oy)
        oy2[i] = (oy2[i] + 1) % R
        y2[i] = fr_from_int(oy2[i])
        assert not both(proof, exp, (ca, cb, y2), (oca, ocb, oy2), ("y", i))
    sw = [1, 0] + list(range(2, K))
    assert not both(proof, exp, (ca[sw], cb, y), ([oca[j] for j in sw], ocb, oy), "swapped comm_a")
    assert not both(proof, exp, (ca, cb[sw], y), (oca, [ocb[j] for j in sw], oy), "swapped comm_b")

    def altered(edit_fields, oracle_proof, what, expect):
        f = proof.batch_fields()
        edit_fields(f)
        bad = gm.InnerProductProof.from_fields_batch(f)
        assert both(bad, oracle_proof, (ca, cb, y), (oca, ocb, oy), what) == expect
        bad.free()

    e2 = gp.gt_from_ints(X.gt_ints(2))
    for i, h in ((0, 0), (exp["rounds"] - 1, 1)):
        def edit(f, i=i, h=h):
            f.messages[i, h] = gp.gt_mul(f.messages[i, h], e2)
        msgs = list(exp["messages"])
        m = list(msgs[i])
        m[h] = (m[h] + 2) % R
        msgs[i] = tuple(m)
        altered(edit, _oracle_with(exp, messages=msgs), ("message", i, h), False)
    for i in range(K):  # a folding scalar: the lhs of ff_i
        def edit(f, i=i):
            f.foldings_ff[i, 0] = fr_from_int((fr_to_int(f.foldings_ff[i, 0]) + 1) % R)
        ff = list(exp["foldings_ff"])
        ff[i] = ((ff[i][0] + 1) % R, ff[i][1])
        altered(edit, _oracle_with(exp, foldings_ff=ff), ("ff lhs", i), False)

    def edit_free(f):  # lhs = 0, so rhs does not count
        f.foldings_ff[K - 1, 1] = fr_from_int((fr_to_int(f.foldings_ff[K - 1, 1]) + 1) % R)
    ff = list(exp["foldings_ff"])
    assert ff[K - 1][0] == 0
    ff[K - 1] = (0, (ff[K - 1][1] + 1) % R)
    altered(edit_free, _oracle_with(exp, foldings_ff=ff), "ff rhs of the zero claim", True)

    def edit_scalar(f):
        f.foldings_fg2[0][0] = fr_from_int((fr_to_int(f.foldings_fg2[0][0]) + 1) % R)
    fg2 = list(exp["foldings_fg2"])
    fg2[0] = ((fg2[0][0] + 1) % R, fg2[0][1])
    altered(edit_scalar, _oracle_with(exp, foldings_fg2=fg2), "fg2 scalar", False)

    other1, olog1 = ca[0], oca[0]  # a folding point: the G1 point of fg1_0 becomes another member of G1
    def edit_point(f):
        f.foldings_fg1[0][0] = other1
    fg1 = list(exp["foldings_fg1"])
    fg1[0] = (olog1, fg1[0][1])
    altered(edit_point, _oracle_with(exp, foldings_fg1=fg1), "fg1 point", False)

    for j in (0, K, 3 * K - 1):  # the weights of ff_0, fg1_0 and fg2_{K-1}: none belongs to the zero side of the claim with a = 0
        def edit_bch(f, j=j):
            f.batch_challenges[j] = fr_from_int((fr_to_int(f.batch_challenges[j]) + 1) % R)
        bch = list(exp["batch_challenges"])
        bch[j] = (bch[j] + 1) % R
        altered(edit_bch, _oracle_with(exp, batch_challenges=bch), ("batch challenge", j), False)
    assert sum(1 for _, v in verdicts if v) == 3
    for o in (proof, vrs, tr, crs):
        o.free()


def test_launch_counts_do_not_depend_on_K(gm):
    """gm_debug_ipa_new_batch_path at d = 64 for K = 1 and K = 5: split-fold launches, MSM calls, Miller launches"""
    from gemini_amd import ipa
    from tests.test_gpu_ipa_new_many import canon
    from tests.test_gpu_ipa import scalars

    crs = gm.Crs.from_scalars(canon(scalars(41, 128)), canon(scalars(42, 128)))
    seen = {}
    for K in (1, 5):
        claims = B.claims_for(K, 64, seed=40 + K)
        tr = gm.Transcript(LABEL)
        proof = gm.InnerProductProof.new_batch(tr, crs, [mont(a) for a, _ in claims], [mont(b) for _, b in claims])
        seen[K] = ipa.new_batch_path()
        proof.free()
        tr.free()
    assert seen[1] == seen[5]
    rounds = 6
    # per round after the first: two arena folds and the point folds of the two module provers; the last fold once more
    assert seen[1] == (4 * (rounds - 1) + 4, 4 * rounds, rounds)
    crs.free()


def test_refusals(gm):
    """every refusal of gm_ipa_new_batch leaves the transcript as a fresh one and makes no handle; gm_ipa_verify_batch refuses
    another K, a short Vrs and scalars that are not reduced; the single-claim entries refuse a proof of two claims"""
    lib, ptr = gm.capi.load(), gm.capi.ptr
    ref = reference(2, 8, 16)
    K, d = 2, 8
    crs, tr, twin = gm.Crs(ref["r1"], ref["r2"]), gm.Transcript(LABEL), gm.Transcript(LABEL)
    a, b = np.ascontiguousarray(np.stack(ref["a_mont"])), np.ascontiguousarray(np.stack(ref["b_mont"]))
    h = C.c_uint64(0)

    def new(t_handle, crs_handle, d_, K_, a_=a, b_=b, out=h):
        return lib.gm_ipa_new_batch(C.c_uint64(t_handle), C.c_uint64(crs_handle), ptr(a_) if a_ is not None else None, ptr(b_) if b_ is not None else None, C.c_size_t(d_),
                                    C.c_size_t(K_), C.byref(out) if out is not None else None)

    gone = gm.Transcript(b"gone")
    gone_handle = gone.handle
    gone.free()
    short = gm.Crs(ref["r1"][:8], ref["r2"][:8])  # d = 8 needs d + 1 = 9 points
    assert new(tr.handle, crs.handle, d, 0) == GM_EINVAL
    assert new(tr.handle, crs.handle, 1, K) == GM_EINVAL and new(tr.handle, crs.handle, 0, K) == GM_EINVAL
    assert new(tr.handle, short.handle, d, K) == GM_EINVAL
    assert new(tr.handle, crs.handle, d, K, a_=None) == GM_EINVAL
    assert new(tr.handle, crs.handle, d, K, b_=None) == GM_EINVAL
    assert new(tr.handle, crs.handle, d, K, out=None) == GM_EINVAL
    assert new(gone_handle, crs.handle, d, K) == GM_EHANDLE
    assert new(tr.handle, gone_handle, d, K) == GM_EHANDLE  # no CRS of that handle
    # 2^40 claims of d = 8 are 2^50 bytes of scalars: refused before a vector is read
    assert new(tr.handle, crs.handle, d, 1 << 40) == GM_ENOMEM
    msg = lib.gm_last_error().decode()
    import re
    assert len(re.findall(r"\d{4,}", msg)) >= 2, msg  # both numbers
    assert h.value == 0
    assert tr.challenge_bytes(b"after", 32) == twin.challenge_bytes(b"after", 32)

    tr2 = gm.Transcript(LABEL)
    proof = gm.InnerProductProof.new_batch(tr2, crs, ref["a_mont"], ref["b_mont"])
    vrs = gm.Vrs(crs)
    ca, cb, y = statement_on_device(crs, ref)
    ok = C.c_int(7)

    def verify(p_handle, v_handle, K_, y_=y):
        return lib.gm_ipa_verify_batch(C.c_uint64(p_handle), C.c_uint64(v_handle), ptr(ca), ptr(cb), ptr(np.ascontiguousarray(y_)), C.c_size_t(K_), C.byref(ok))

    assert verify(proof.handle, vrs.handle, K) == 0 and ok.value == 1
    assert verify(proof.handle, vrs.handle, 1) == GM_EINVAL and verify(proof.handle, vrs.handle, 3) == GM_EINVAL
    tiny = gm.Crs(ref["r1"][:4], ref["r2"][:4])
    tiny_vrs = gm.Vrs(tiny)  # 1 level; a proof of 3 rounds needs 2
    assert tiny_vrs.levels == 1 and verify(proof.handle, tiny_vrs.handle, K) == GM_EINVAL
    big = y.copy()
    big[1] = np.array([2**64 - 1] * 4, dtype=np.uint64)  # above the modulus
    assert verify(proof.handle, vrs.handle, K, big) == GM_EINVAL
    f = proof.batch_fields()
    f.foldings_ff[0, 1] = big[1]
    bad = gm.InnerProductProof.from_fields_batch(f)
    assert verify(bad.handle, vrs.handle, K) == GM_EINVAL
    bad.free()
    f = proof.batch_fields()
    f.batch_challenges[2] = big[1]
    bad = gm.InnerProductProof.from_fields_batch(f)
    assert verify(bad.handle, vrs.handle, K) == GM_EINVAL
    bad.free()
    assert verify(vrs.handle, vrs.handle, K) == GM_EHANDLE and verify(proof.handle, crs.handle, K) == GM_EHANDLE
    # the single-claim entries
    ph, buf = C.c_uint64(proof.handle), np.zeros(64, dtype=np.uint64)
    assert lib.gm_ipa_verify(ph, C.c_uint64(vrs.handle), ptr(ca), ptr(cb), ptr(y), C.byref(ok)) == GM_EINVAL
    hs, oks = np.array([proof.handle], dtype=np.uint64), np.zeros(1, dtype=np.intc)
    assert lib.gm_ipa_verify_many(ptr(hs), C.c_uint64(vrs.handle), ptr(ca), ptr(cb), ptr(y), C.c_size_t(1), ptr(oks)) == GM_EINVAL
    assert lib.gm_ipa_foldings_ff(ph, ptr(buf)) == GM_EINVAL
    assert lib.gm_ipa_foldings_fg1(ph, ptr(buf), ptr(buf[32:])) == GM_EINVAL
    assert lib.gm_ipa_foldings_fg2(ph, ptr(buf), ptr(buf[8:])) == GM_EINVAL
    assert lib.gm_debug_ipa_stated_terms(ph, ptr(y), ptr(np.zeros((64, 4), dtype=np.uint64)), ptr(np.zeros((64, 4), dtype=np.uint64))) == GM_EINVAL
    assert lib.gm_ipa_host_times(ph, (C.c_double * 3)()) == GM_EINVAL
    n = C.c_size_t()
    assert lib.gm_ipa_rounds(ph, C.byref(n)) == 0 and n.value == 3 and lib.gm_ipa_claims(ph, C.byref(n)) == 0 and n.value == 2
    for o in (proof, vrs, tiny_vrs, tiny, short, tr, tr2, twin, crs):
        o.free()


def test_twenty_three_claims(gm):
    """K = 23 at d = 8: one more FModule prover than a launch of the multi-prover sumcheck round takes"""
    K, d, n = 23, 8, 16
    ref = reference(K, d, n)
    crs, tr = gm.Crs(ref["r1"], ref["r2"]), gm.Transcript(LABEL)
    proof = gm.InnerProductProof.new_batch(tr, crs, ref["a_mont"], ref["b_mont"])
    assert_fields_equal(proof.batch_fields(), ref["proof"], K)
    assert fr_to_int(tr.get_challenge(b"next")) == ref["next"]
    vrs = gm.Vrs(crs)
    ca, cb, y = statement_on_device(crs, ref)
    assert proof.verify_batch(vrs, ca, cb, y)
    y[22] = fr_from_int((ref["y"][22] + 1) % R)
    assert not proof.verify_batch(vrs, ca, cb, y)
    for o in (proof, vrs, tr, crs):
        o.free()
