"""GPU: many proofs in one call -- gm_kzg_verify_multi_points_many, gm_snark_verify_many, gm_psnark_verify_many.  The verdict of every
proof of a batch is what the single entry answers for it, on both sides of gm_set_verify_many_min, and what the restatement on
Python integers (oracle/verifier_ref.py) answers.  A rejected proof is False in the list, never an exception or an error code."""
import ctypes as C

import numpy as np
import pytest

from tests import test_gpu_verifier as TV
from tests.test_gpu_verifier import _double, _limbs, _mont, _verdict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


@pytest.fixture()
def knob(gm):
    """gm_set_verify_many_min for one test; the default comes back afterwards"""
    from gemini_amd.kzg import set_verify_many_min

    yield set_verify_many_min
    set_verify_many_min(DEFAULT_MIN)


DEFAULT_MIN = 3  # Context::verify_many_min (gemini_amd/csrc/ctx.hpp)


# ---- KZG ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kzg_batch(gm, oracle, pyref):
    """The honest case of tests/test_gpu_verifier.py (polynomials of 33, 17 and 9 coefficients at 3 points, the key from a trapdoor), its
    four altered variants, the same polynomials opened at a point set that holds 0, and a constant polynomial (its proof element is the
    identity).  Each entry: (name, device arguments, oracle arguments, expected verdict)."""
    from gemini_amd.kzg import CommitterKey, VerifierKey
    from oracle import verifier_ref as V
    from tests.util import jac_to_affine_ints

    R = pyref.R_MOD
    tau = 0x1F2E3D4C5B6A79880123456789ABCDEF % R
    rng = pyref.SplitMix64(5)
    polys = [[rng.fr() for _ in range(n)] for n in (33, 17, 9)]
    pts = [rng.fr() for _ in range(3)]
    chal = rng.fr()
    ck = CommitterKey.new(40, 5, _limbs(oracle, tau))
    vk, ovk = VerifierKey.from_committer_key(ck), V.VerifierKey.from_trapdoor(tau, 5)
    vecs = [gm.FrVec.from_host(_mont(gm, p)) for p in polys]
    comms = ck.batch_commit(vecs)
    evals = [[pyref.evaluate_le(p, x) for x in pts] for p in polys]
    proof = ck.batch_open_multi_points(vecs, _mont(gm, pts), gm.fr.fr_from_int(chal))
    pts0 = [pts[0], 0, pts[2]]
    evals0 = [[pyref.evaluate_le(p, x) for x in pts0] for p in polys]
    proof0 = ck.batch_open_multi_points(vecs, _mont(gm, pts0), gm.fr.fr_from_int(chal))
    const = gm.FrVec.from_host(_mont(gm, [polys[0][0]]))
    const_comm = ck.batch_commit([const])
    const_proof = ck.batch_open_multi_points([const], _mont(gm, pts), gm.fr.fr_from_int(chal))
    assert not np.asarray(const_proof, dtype=np.uint64).reshape(3, 6)[2].any()  # the quotient is zero: the identity
    for v in vecs + [const]:
        v.free()
    aff = lambda p: jac_to_affine_ints(oracle, p)  # noqa: E731

    def entry(name, want, comms=comms, pts=pts, evals=evals, proof=proof, chal=chal):
        dev = (list(comms), _mont(gm, pts), np.stack([_mont(gm, e) for e in evals]), proof, gm.fr.fr_from_int(chal))
        return name, dev, ([aff(c) for c in comms], pts, evals, aff(proof), chal), want

    bad_evals = [list(e) for e in evals]
    bad_evals[1][2] = (bad_evals[1][2] + 1) % R
    batch = [entry("honest", True), entry("evaluation", False, evals=bad_evals), entry("proof", False, proof=_double(proof)),
             entry("open_chal", False, chal=(chal + 1) % R), entry("count", False, comms=comms[:2]),
             entry("point 0", True, pts=pts0, evals=evals0, proof=proof0), entry("point 0, first proof", False, pts=pts0, evals=evals0),
             entry("constant", True, comms=const_comm, evals=[[polys[0][0]] * 3], proof=const_proof)]
    yield {"vk": vk, "ovk": ovk, "batch": batch}
    vk.free()
    ck.powers_of_g.free()


def test_kzg_batch_equals_the_single_calls_and_the_oracle(gm, kzg_batch, knob):
    from oracle import verifier_ref as V

    vk, batch = kzg_batch["vk"], kzg_batch["batch"]
    want = [w for _, _, _, w in batch]
    singles = [_verdict(vk.verify_multi_points, *dev) for _, dev, _, _ in batch]
    assert singles == want
    assert [_verdict(V.verify_multi_points, kzg_batch["ovk"], *o) for _, _, o, _ in batch] == want
    checks = [dev for _, dev, _, _ in batch]
    for minimum in (DEFAULT_MIN, 1, len(batch) + 1):  # the batched path, forced on, and the per-check path
        knob(minimum)
        assert vk.verify_multi_points_many(checks) == want, minimum
        assert vk.verify_multi_points_many(checks[::-1]) == want[::-1], minimum
    knob(1)
    assert vk.verify_multi_points_many([]) == []
    for dev, w in zip(checks, want):  # S = 1, through the batched path
        assert vk.verify_multi_points_many([dev]) == [w]
    knob(DEFAULT_MIN)
    assert vk.verify_multi_points_many(checks[:1]) == want[:1]  # S = 1, below the default: the per-check path


def test_kzg_batch_misuse_is_an_error_code(gm, kzg_batch):
    """more points than the key holds powers for fails the call, as it fails the single entry; a stale handle is GM_EHANDLE"""
    vk, batch = kzg_batch["vk"], kzg_batch["batch"]
    comms, _, _, proof, chal = batch[0][1]
    too_many = (comms, _mont(gm, [3, 4, 5, 6, 7, 8]), np.zeros((3, 6, 4), dtype=np.uint64), proof, chal)
    with pytest.raises(gm.capi.GeminiHipError) as e:
        vk.verify_multi_points_many([batch[0][1], too_many])
    assert e.value.code == -1
    ok = (C.c_int * 1)()
    z = np.zeros(32, dtype=np.uint64)
    off = np.array([0, 1], dtype=np.uintp)
    p = gm.capi.ptr
    lib = gm.capi.load()
    assert lib.gm_kzg_verify_multi_points_many(C.c_uint64(1 << 40), C.c_size_t(1), p(z), p(off), p(z), p(off), p(z), p(off), p(z), p(z), ok) == -3
    assert lib.gm_kzg_verify_multi_points_many(C.c_uint64(vk.handle), C.c_size_t(1), p(z), None, p(z), p(off), p(z), p(off), p(z), p(z), ok) == -1


# ---- snark ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def snark_batch(gm, oracle, pyref):
    """n = 32.  dummy_r1cs has A = B = C = diag(1 / e), so z is satisfying iff every entry is 0 or e: two witnesses with different
    public inputs under ONE set of matrices."""
    from gemini_amd.circuit import R1cs
    from gemini_amd.snark import Proof

    n = 32
    K = TV._snark_case(gm, oracle, pyref, "dummy", n)
    e = K["inst"]["z"][0]
    z2 = [0 if i % 3 == 0 else e for i in range(n)]
    inst2 = dict(K["inst"], z=z2, w=z2[1:], x=z2[:1])
    r = K["r1cs"]
    r2 = R1cs(r.a, r.b, r.c, r.at, r.bt, r.ct, gm.FrVec.from_host(_mont(gm, z2)), gm.FrVec.from_host(_mont(gm, z2[1:])), gm.FrVec.from_host(_mont(gm, z2[:1])))
    proof2 = Proof.new_time(r2, K["ck"])
    T = lambda slot: TV._snark_tamper(gm, pyref, K["proof"], slot)  # noqa: E731
    # (name, proof, instance it was made for, expected verdict)
    batch = [("honest", K["proof"], 0, True), ("first sumcheck message", T("first_sumcheck_msgs:message"), 0, False), ("honest, other x", proof2, 1, True),
             ("fold evaluation", T("folded_evaluation"), 0, False), ("evaluation proof", T("evaluation_proof"), 0, False),
             ("fold commitment", T("folded_commitment"), 0, False), ("other x, wrong input", proof2, 0, False),
             ("other x, evaluation proof", TV._snark_tamper(gm, pyref, proof2, "evaluation_proof"), 1, False)]
    yield {"K": K, "r1cs": [r, r2], "inst": [K["inst"], inst2], "batch": batch}
    for v in (r2.z, r2.w, r2.x):
        v.free()


def test_snark_batch_equals_proof_verify_one_by_one(gm, oracle, pyref, snark_batch, knob):
    from gemini_amd.snark import Proof
    from oracle import verifier_ref as V
    from tests.util import snark_proof_to_ints

    K, rs, batch = snark_batch["K"], snark_batch["r1cs"], snark_batch["batch"]
    want = [w for *_, w in batch]
    assert [_verdict(p.verify, rs[i], K["vk"]) for _, p, i, _ in batch] == want
    for k in (0, 4):  # the honest proof and the one only the pairing rejects: the Python-integer pairing is slow
        _, p, i, w = batch[k]
        assert _verdict(V.snark_verify, snark_proof_to_ints(gm, oracle, p), snark_batch["inst"][i], K["ovk"]) == w
    proofs, xs = [p for _, p, _, _ in batch], [rs[i].x for _, _, i, _ in batch]
    for minimum in (DEFAULT_MIN, 1, len(batch) + 1):
        knob(minimum)
        assert Proof.verify_many(proofs, rs[0], K["vk"], x_vecs=xs) == want, minimum
    knob(1)
    assert Proof.verify_many([], rs[0], K["vk"]) == []
    assert Proof.verify_many(proofs[:1], rs[0], K["vk"]) == [True] and Proof.verify_many(proofs[4:5], rs[0], K["vk"]) == [False]
    assert Proof.verify_many(proofs[:2], rs[0], K["vk"]) == want[:2]  # x_vecs defaults to the instance's
    other = TV._other_g2_key(gm, pyref, K["ck"], 12345)
    assert Proof.verify_many(proofs, rs[0], other, x_vecs=xs) == [False] * len(batch)
    other.free()


def test_snark_batch_misuse_is_an_error_code(gm, oracle, pyref, snark_batch):
    from gemini_amd.snark import _GmSnarkProof, _pack_native

    K, r = snark_batch["K"], snark_batch["r1cs"][0]
    lib = gm.capi.load()
    packed = [_pack_native(K["proof"]) for _ in range(2)]
    recs = (_GmSnarkProof * 2)(*[P for P, _ in packed])
    xh = (C.c_uint64 * 2)(r.x.handle, r.x.handle)
    mats = (C.c_uint64 * 3)(r.a.handle, r.b.handle, r.c.handle)
    ok = (C.c_int * 2)(-7, -7)
    assert lib.gm_snark_verify_many(mats, xh, C.c_uint64(K["vk"].handle), C.c_int(0), recs, C.c_size_t(2), ok) == 0 and list(ok) == [1, 1]
    assert lib.gm_snark_verify_many(mats, xh, C.c_uint64(r.z.handle), C.c_int(0), recs, C.c_size_t(2), ok) == -3  # a vector is no key
    assert lib.gm_snark_verify_many(mats, None, C.c_uint64(K["vk"].handle), C.c_int(0), recs, C.c_size_t(2), ok) == -1
    foreign = (C.c_uint64 * 3)(r.a.handle, r.z.handle, r.c.handle)
    assert lib.gm_snark_verify_many(foreign, xh, C.c_uint64(K["vk"].handle), C.c_int(0), recs, C.c_size_t(2), ok) == -3


# ---- psnark --------------------------------------------------------------------------------------------------------------------
def test_psnark_batch_equals_verify_one_by_one(gm, oracle, pyref, knob):
    """the smallest instance of tests/test_gpu_verifier.py.  Doubling ralpha_star_acc_mu_proof fails only the FIRST of the two KZG
    checks, doubling evaluation_proof only the second; a bumped third-sumcheck message is rejected on the host behind the first check"""
    from gemini_amd.psnark import Proof

    K = TV._psnark_case(gm, oracle, pyref, "dummy", 1 << 3)
    alt = dict(TV._psnark_alterations(gm, pyref, K["proof"]))
    batch = [(K["proof"], True), (alt["ralpha_star_acc_mu_proof"], False), (alt["tensorcheck.evaluation_proof"], False), (alt["third_sumcheck_msgs:message"], False),
             (K["proof"], True)]
    proofs, want = [p for p, _ in batch], [w for _, w in batch]
    assert [_verdict(p.verify, K["r1cs"], K["vk"], K["index"], K["nnz"]) for p in proofs] == want
    for minimum in (DEFAULT_MIN, 1, 2 * len(batch) + 1):
        knob(minimum)
        assert Proof.verify_many(proofs, K["r1cs"], K["vk"], K["index"], K["nnz"]) == want, minimum
    knob(1)
    assert Proof.verify_many(proofs[1:2], K["r1cs"], K["vk"], K["index"]) == [False]  # the number of non-zero entries from the instance
    assert Proof.verify_many([], K["r1cs"], K["vk"], K["index"], K["nnz"]) == []


def test_psnark_batch_error_behind_a_failed_first_check(gm, oracle, pyref, knob):
    """An unknown public-input handle is read only BEHIND the first KZG check.  The single entry rejects a proof whose first check fails
    and never reaches the handle; for the honest proof it answers GM_EHANDLE.  A batch does the same, proof by proof in order."""
    from gemini_amd.circuit import R1cs
    from gemini_amd.psnark import Proof

    class Unknown:
        handle = 1 << 40

    K = TV._psnark_case(gm, oracle, pyref, "dummy", 1 << 3)
    alt = dict(TV._psnark_alterations(gm, pyref, K["proof"]))
    r = K["r1cs"]
    lost = R1cs(r.a, r.b, r.c, r.at, r.bt, r.ct, r.z, r.w, Unknown())
    bad_first = alt["ralpha_star_acc_mu_proof"]
    assert not _verdict(bad_first.verify, lost, K["vk"], K["index"], K["nnz"])
    with pytest.raises(gm.capi.GeminiHipError) as e:
        K["proof"].verify(lost, K["vk"], K["index"], K["nnz"])
    assert e.value.code == -3
    for minimum in (1, 100):
        knob(minimum)
        assert Proof.verify_many([bad_first, K["proof"], bad_first], r, K["vk"], K["index"], K["nnz"], x_vecs=[Unknown(), r.x, Unknown()]) == [False, True, False]
        with pytest.raises(gm.capi.GeminiHipError) as e:
            Proof.verify_many([bad_first, K["proof"]], r, K["vk"], K["index"], K["nnz"], x_vecs=[Unknown(), Unknown()])
        assert e.value.code == -3
