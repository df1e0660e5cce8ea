"""GPU: the verifiers of the library (gemini_amd/csrc/verifier.cpp) -- kzg::VerifierKey::{verify, verify_multi_points}, Subclaim::{new,
new_batch}, snark::Proof::verify, psnark::Proof::verify -- on proofs of the device provers.  An honest proof is accepted, every single
altered element is rejected, and the verdicts are those of the independent restatement on Python integers (oracle/verifier_ref.py).
A rejection is a result (`VerificationError` in the mirrors, *ok = 0 in the C ABI), never an error code."""
import copy
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


def _limbs(oracle, v):
    return oracle.ints_to_limbs([v], 4)[0]


def _mont(gm, ints):
    return np.stack([gm.fr.fr_from_int(v) for v in ints]) if len(ints) else np.empty((0, 4), dtype=np.uint64)


def _bump(gm, pyref, x):
    """an Fr element + 1"""
    return gm.fr.fr_from_int((gm.fr.fr_to_int(x) + 1) % pyref.R_MOD)


def _double(p):
    """a G1 point (Jacobian limbs) replaced by its double"""
    from gemini_amd.msm import g1_sum

    return g1_sum(np.stack([np.asarray(p, dtype=np.uint64), np.asarray(p, dtype=np.uint64)]))


def _verdict(fn, *args) -> bool:
    """True: accepted, False: rejected -- whichever VerificationError class the callee raises"""
    from gemini_amd.kzg import VerificationError
    from oracle import verifier_ref as V

    try:
        fn(*args)
        return True
    except (VerificationError, V.VerificationError):
        return False


def _device_instance(gm, inst, n):
    """an instance in the layout of oracle/snark_ref.py on the device"""
    from gemini_amd.circuit import R1cs, SparseMatrix

    dev = lambda rows: [[(gm.fr.fr_from_int(v), col) for v, col in row] for row in rows]  # noqa: E731
    mats = [SparseMatrix.from_rows(dev(inst[k]), n) for k in "abc"] + [SparseMatrix.from_rows(dev(inst[k]), n, transpose=True) for k in "abc"]
    return R1cs(*mats, gm.FrVec.from_host(_mont(gm, inst["z"])), gm.FrVec.from_host(_mont(gm, inst["w"])), gm.FrVec.from_host(_mont(gm, inst["x"])))


def _other_g2_key(gm, pyref, ck, other_tau):
    """the G1 half of `ck` with the G2 powers of another trapdoor"""
    from gemini_amd import g2 as G2
    from gemini_amd.kzg import VerifierKey, g2_records

    k = ck.max_eval_points()
    return VerifierKey.from_powers(ck.powers_of_g.download(0, k), g2_records([G2.mul(G2.generator(), pow(other_tau, i, pyref.R_MOD)) for i in range(k + 1)]))


# ---- KZG ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kzg_case(gm, oracle, pyref):
    """3 polynomials of 33, 17, 9 coefficients committed and opened at 3 points by the device CommitterKey"""
    from gemini_amd.fr import evaluate_le
    from gemini_amd.kzg import CommitterKey, VerifierKey
    from oracle import verifier_ref as V
    from tests.util import jac_to_affine_ints

    tau = 0x1F2E3D4C5B6A79880123456789ABCDEF % pyref.R_MOD
    rng = pyref.SplitMix64(5)
    polys = [[rng.fr() for _ in range(n)] for n in (33, 17, 9)]
    pts = [rng.fr() for _ in range(3)]
    chal = rng.fr()
    ck = CommitterKey.new(40, 5, _limbs(oracle, tau))
    vecs = [gm.FrVec.from_host(_mont(gm, p)) for p in polys]
    case = {"tau": tau, "ck": ck, "vk": VerifierKey.from_committer_key(ck), "ovk": V.VerifierKey.from_trapdoor(tau, 5), "pts": pts, "chal": chal,
            "comms": ck.batch_commit(vecs), "evals": [[pyref.evaluate_le(p, x) for x in pts] for p in polys],
            "proof": ck.batch_open_multi_points(vecs, _mont(gm, pts), gm.fr.fr_from_int(chal))}
    # single point: the first polynomial at the first point
    ev, single = ck.open(vecs[0], gm.fr.fr_from_int(pts[0]))
    assert gm.fr.fr_to_int(ev) == case["evals"][0][0] and (evaluate_le(vecs[0], _mont(gm, pts[:1]))[0] == ev).all()
    case["single"] = single
    case["aff"] = lambda p: jac_to_affine_ints(oracle, p)
    for v in vecs:
        v.free()
    yield case
    case["vk"].free()
    ck.powers_of_g.free()


def test_vk_halves_and_the_g2_bytes(gm, oracle, pyref, kzg_case):
    """From<&CommitterKey> keeps max_eval_points G1 powers and all G2 powers; gm_vk_from_trapdoor builds the same key; the bytes psnark
    absorbs as b"ck" are CommitterKey.powers_of_g2_bytes() in both framings"""
    from gemini_amd.kzg import VerifierKey

    ck, vk = kzg_case["ck"], kzg_case["vk"]
    n1, n2 = C.c_size_t(), C.c_size_t()
    lib = gm.capi.load()
    assert lib.gm_vk_len(C.c_uint64(vk.handle), C.byref(n1), C.byref(n2)) == 0 and (n1.value, n2.value) == (5, 6)
    from gemini_amd import g2 as G2

    for enc in (0, 1):
        assert vk.powers_of_g2_bytes(enc) == G2.serialize_vec_uncompressed(ck.powers_of_g2, enc)
    vt = VerifierKey.from_trapdoor(_limbs(oracle, kzg_case["tau"]), 5)
    assert vt.powers_of_g2_bytes(0) == vk.powers_of_g2_bytes(0)
    vt.verify_multi_points(kzg_case["comms"], _mont(gm, kzg_case["pts"]), np.stack([_mont(gm, e) for e in kzg_case["evals"]]), kzg_case["proof"],
                           gm.fr.fr_from_int(kzg_case["chal"]))
    vt.free()


@pytest.mark.parametrize("case", ["honest", "evaluation", "proof", "open_chal", "g2_key", "count"])
def test_kzg_verify_multi_points(gm, oracle, pyref, kzg_case, case):
    from oracle import verifier_ref as V

    K, aff, R = kzg_case, kzg_case["aff"], pyref.R_MOD
    comms, evals, proof, chal, vk, ovk = list(K["comms"]), [list(e) for e in K["evals"]], K["proof"], K["chal"], K["vk"], K["ovk"]
    if case == "evaluation":
        evals[1][2] = (evals[1][2] + 1) % R
    elif case == "proof":
        proof = _double(proof)
    elif case == "open_chal":
        chal = (chal + 1) % R
    elif case == "g2_key":
        vk = _other_g2_key(gm, pyref, K["ck"], 12345)
        ovk = V.VerifierKey(ovk.powers_of_g, V.VerifierKey.from_trapdoor(12345, 5).powers_of_g2)
    elif case == "count":  # one evaluation row per commitment: a mismatch is a rejection, as the oracle states it
        comms = comms[:2]
    got = _verdict(vk.verify_multi_points, comms, _mont(gm, K["pts"]), np.stack([_mont(gm, e) for e in evals]), proof, gm.fr.fr_from_int(chal))
    want = _verdict(V.verify_multi_points, ovk, [aff(c) for c in comms], K["pts"], evals, aff(proof), chal)
    assert got == want == (case == "honest")
    if case == "g2_key":
        vk.free()


@pytest.mark.parametrize("case", ["honest", "evaluation", "proof", "point", "g2_key"])
def test_kzg_verify_single_point(gm, oracle, pyref, kzg_case, case):
    from oracle import verifier_ref as V

    K, aff, R = kzg_case, kzg_case["aff"], pyref.R_MOD
    comm, alpha, ev, proof, vk, ovk = K["comms"][0], K["pts"][0], K["evals"][0][0], K["single"], K["vk"], K["ovk"]
    if case == "evaluation":
        ev = (ev + 1) % R
    elif case == "proof":
        proof = _double(proof)
    elif case == "point":
        alpha = (alpha + 1) % R
    elif case == "g2_key":
        vk = _other_g2_key(gm, pyref, K["ck"], 12345)
        ovk = V.VerifierKey(ovk.powers_of_g, V.VerifierKey.from_trapdoor(12345, 5).powers_of_g2)
    got = _verdict(vk.verify, comm, gm.fr.fr_from_int(alpha), gm.fr.fr_from_int(ev), proof)
    want = _verdict(V.verify, ovk, aff(comm), alpha, ev, aff(proof))
    assert got == want == (case == "honest")
    if case == "g2_key":
        vk.free()


def test_more_points_than_the_key_holds_is_misuse(gm, oracle, pyref, kzg_case):
    """6 points against a key of 5 G1 / 6 G2 powers: GM_EINVAL, not a verdict"""
    K = kzg_case
    pts = _mont(gm, [3, 4, 5, 6, 7, 8])
    ev = np.zeros((3, 6, 4), dtype=np.uint64)
    with pytest.raises(gm.capi.GeminiHipError) as e:
        K["vk"].verify_multi_points(K["comms"], pts, ev, K["proof"], gm.fr.fr_from_int(K["chal"]))
    assert e.value.code == -1


# ---- Subclaim ----------------------------------------------------------------------------------------------------------------
def _twisted_ip(pyref, f, g, tw):
    return sum(a * b % pyref.R_MOD * pow(tw, i, pyref.R_MOD) for i, (a, b) in enumerate(zip(f, g))) % pyref.R_MOD


def test_subclaim_new_on_a_device_sumcheck(gm, pyref):
    from gemini_amd.kzg import VerificationError
    from gemini_amd.sumcheck import Subclaim, Sumcheck
    from gemini_amd.transcript import Transcript

    rng = pyref.SplitMix64(901)
    f, g, tw = [rng.fr() for _ in range(32)], [rng.fr() for _ in range(32)], rng.fr()
    sc = Sumcheck.new_time(Transcript(), _mont(gm, f), _mont(gm, g), gm.fr.fr_from_int(tw))
    assert len(sc.messages) == 5
    claim = gm.fr.fr_from_int(_twisted_ip(pyref, f, g, tw))
    sub = Subclaim.new(Transcript(), sc.messages, sc.final_foldings, claim)
    assert all((a == b).all() for a, b in zip(sub.challenges, sc.challenges)) and len(sub.challenges) == 5
    bad = list(sc.messages)
    bad[2] = (bad[2][0], _bump(gm, pyref, bad[2][1]))
    with pytest.raises(VerificationError):
        Subclaim.new(Transcript(), bad, sc.final_foldings, claim)
    with pytest.raises(VerificationError):
        Subclaim.new(Transcript(), sc.messages, [(_bump(gm, pyref, sc.final_foldings[0][0]), sc.final_foldings[0][1])], claim)
    with pytest.raises(VerificationError):
        Subclaim.new(Transcript(), sc.messages, sc.final_foldings, _bump(gm, pyref, claim))


def test_subclaim_new_batch_on_a_device_batch_sumcheck(gm, pyref):
    from gemini_amd.kzg import VerificationError
    from gemini_amd.sumcheck import Subclaim, Sumcheck, TimeProver
    from gemini_amd.transcript import Transcript

    rng = pyref.SplitMix64(902)
    shapes = [(32, rng.fr()), (32, 1), (8, rng.fr())]
    data = [([rng.fr() for _ in range(n)], [rng.fr() for _ in range(n)], tw) for n, tw in shapes]
    provers = [TimeProver(_mont(gm, f), _mont(gm, g), gm.fr.fr_from_int(tw)) for f, g, tw in data]
    sc = Sumcheck.prove_batch(Transcript(), provers)
    for p in provers:
        p.free()
    assert len(sc.messages) == 6 and len(sc.final_foldings) == 3  # max rounds + 1
    sums = _mont(gm, [_twisted_ip(pyref, f, g, tw) for f, g, tw in data])
    sub = Subclaim.new_batch(Transcript(), sc.messages, sc.final_foldings, sums)
    assert all((a == b).all() for a, b in zip(sub.challenges, sc.challenges)) and len(sub.challenges) == 6
    bad = list(sc.messages)
    bad[0] = (_bump(gm, pyref, bad[0][0]), bad[0][1])
    with pytest.raises(VerificationError):
        Subclaim.new_batch(Transcript(), bad, sc.final_foldings, sums)
    ff = list(sc.final_foldings)
    ff[2] = (ff[2][0], _bump(gm, pyref, ff[2][1]))
    with pytest.raises(VerificationError):
        Subclaim.new_batch(Transcript(), sc.messages, ff, sums)


# ---- snark ---------------------------------------------------------------------------------------------------------------------
_SNARK_CACHE = {}


def _snark_case(gm, oracle, pyref, kind, n):
    """(instance as integers, device instance, key, verifier key, oracle key, device proof), built once per module"""
    from gemini_amd.circuit import dummy_r1cs
    from gemini_amd.kzg import CommitterKey, VerifierKey
    from gemini_amd.snark import Proof
    from oracle import snark_ref as sr
    from oracle import verifier_ref as V
    from tests.util import random_r1cs_instance

    if (kind, n) not in _SNARK_CACHE:
        if kind == "dummy":
            e = oracle.limbs_to_ints(oracle.random_fr(3100 + n, 1))[0]
            tau = oracle.limbs_to_ints(oracle.random_fr(3200 + n, 1))[0]
            inst, r1cs = sr.dummy_r1cs(e, n), dummy_r1cs(e, n)
        else:
            inst, tau = random_r1cs_instance(pyref, sr, n, 99, nx=2)
            r1cs = _device_instance(gm, inst, n)
        ck = CommitterKey.new(2 * n, 5, _limbs(oracle, tau))
        _SNARK_CACHE[(kind, n)] = {"inst": inst, "r1cs": r1cs, "ck": ck, "vk": VerifierKey.from_committer_key(ck), "ovk": V.VerifierKey.from_trapdoor(tau, 5),
                                   "proof": Proof.new_time(r1cs, ck), "tau": tau}
    return _SNARK_CACHE[(kind, n)]


@pytest.mark.parametrize("kind,n", [("dummy", 1 << 3), ("dummy", 1 << 8), ("dummy", 1 << 12), ("random", 16)])
def test_snark_device_proofs_are_accepted(gm, oracle, pyref, kind, n):
    """time and (<= 2^8) elastic proofs; the verdict is the oracle's; a proof that went through serialize / deserialize -- the verifier
    that did not run the prover -- is accepted as well"""
    from gemini_amd.circuit import R1csStream
    from gemini_amd.kzg import CommitterKeyStream
    from gemini_amd.snark import Proof
    from oracle import verifier_ref as V
    from tests.util import snark_proof_to_ints

    K = _snark_case(gm, oracle, pyref, kind, n)
    K["proof"].verify(K["r1cs"], K["vk"])
    assert _verdict(V.snark_verify, snark_proof_to_ints(gm, oracle, K["proof"]), K["inst"], K["ovk"])
    for compress in (True, False):
        Proof.deserialize(K["proof"].serialize(compress), compress).verify(K["r1cs"], K["vk"])
    if n <= 1 << 8:
        stream = R1csStream(K["r1cs"])
        elastic = Proof.new_elastic(stream, CommitterKeyStream.from_committer_key(K["ck"]), 1 << 5)
        elastic.verify(K["r1cs"], K["vk"])
        stream.free()


def _snark_tamper(gm, pyref, proof, slot):
    p = copy.deepcopy(proof)
    tc = p.tensorcheck_proof
    B = lambda x: _bump(gm, pyref, x)  # noqa: E731
    if slot == "zc_alpha":
        p.zc_alpha = B(p.zc_alpha)
    elif slot == "witness_commitment":
        p.witness_commitment = _double(p.witness_commitment)
    elif slot == "folded_commitment":
        tc.folded_polynomials_commitments[0] = _double(tc.folded_polynomials_commitments[0])
    elif slot == "folded_evaluation":
        e = np.array(tc.folded_polynomials_evaluations[1], dtype=np.uint64).reshape(2, 4)
        e[0] = B(e[0])
        tc.folded_polynomials_evaluations[1] = e
    elif slot == "base_evaluation":
        e = np.array(tc.base_polynomials_evaluations[0], dtype=np.uint64).reshape(3, 4)
        e[0] = B(e[0])
        tc.base_polynomials_evaluations[0] = e
    elif slot == "evaluation_proof":
        tc.evaluation_proof = _double(tc.evaluation_proof)
    else:
        which, part = slot.split(":")
        msgs, ff = getattr(p, which)
        msgs, ff = list(msgs), list(ff)
        if part == "message":
            msgs[1] = (msgs[1][0], B(msgs[1][1]))
        else:
            ff[0] = (B(ff[0][0]), ff[0][1])
        setattr(p, which, (msgs, ff))
    return p


SNARK_SLOTS = ["zc_alpha", "witness_commitment", "folded_commitment", "folded_evaluation", "base_evaluation", "evaluation_proof",
               "first_sumcheck_msgs:message", "first_sumcheck_msgs:final", "second_sumcheck_msgs:message", "second_sumcheck_msgs:final"]


@pytest.mark.parametrize("slot", SNARK_SLOTS)
def test_snark_rejects_every_altered_slot(gm, oracle, pyref, slot):
    """the tamper list of tests/test_oracle_verifier.py, slot by slot, on the 2^3 instance; the oracle gives the same verdict"""
    from gemini_amd.kzg import VerificationError
    from oracle import verifier_ref as V
    from tests.util import snark_proof_to_ints

    K = _snark_case(gm, oracle, pyref, "dummy", 1 << 3)
    bad = _snark_tamper(gm, pyref, K["proof"], slot)
    with pytest.raises(VerificationError):
        bad.verify(K["r1cs"], K["vk"])
    assert not _verdict(V.snark_verify, snark_proof_to_ints(gm, oracle, bad), K["inst"], K["ovk"])
    K["proof"].verify(K["r1cs"], K["vk"])  # the copy was altered, not the proof


def test_snark_rejects_a_wrong_g2_key_and_another_public_input(gm, oracle, pyref):
    from gemini_amd.circuit import R1cs
    from gemini_amd.kzg import VerificationError

    K = _snark_case(gm, oracle, pyref, "random", 16)
    other = _other_g2_key(gm, pyref, K["ck"], 12345)
    with pytest.raises(VerificationError):
        K["proof"].verify(K["r1cs"], other)
    other.free()
    r = K["r1cs"]
    x = r.x.to_host()
    x[1] = _bump(gm, pyref, x[1])
    x2 = gm.FrVec.from_host(x)
    with pytest.raises(VerificationError):
        K["proof"].verify(R1cs(r.a, r.b, r.c, r.at, r.bt, r.ct, r.z, r.w, x2), K["vk"])
    x2.free()


def test_gm_snark_verify_reports_a_rejection_as_a_result(gm, oracle, pyref):
    """through ctypes: return value 0 with ok = 0 for a rejected proof, 0 with ok = 1 for the honest one; stale and foreign handles
    are GM_EHANDLE"""
    from gemini_amd.kzg import VerifierKey
    from gemini_amd.snark import _pack_native

    K = _snark_case(gm, oracle, pyref, "dummy", 1 << 3)
    lib = gm.capi.load()
    r = K["r1cs"]
    mats = (C.c_uint64 * 3)(r.a.handle, r.b.handle, r.c.handle)
    for proof, want in ((K["proof"], 1), (_snark_tamper(gm, pyref, K["proof"], "folded_evaluation"), 0), (_snark_tamper(gm, pyref, K["proof"], "zc_alpha"), 0)):
        P, keep = _pack_native(proof)
        ok = C.c_int(-7)
        assert lib.gm_snark_verify(mats, C.c_uint64(r.x.handle), C.c_uint64(K["vk"].handle), C.c_int(0), C.byref(P), C.byref(ok)) == 0
        assert ok.value == want
    P, keep = _pack_native(K["proof"])
    ok = C.c_int(-7)
    stale = VerifierKey.from_committer_key(K["ck"])
    h = stale.handle
    stale.free()
    assert lib.gm_vk_free(C.c_uint64(h)) == -3
    assert lib.gm_snark_verify(mats, C.c_uint64(r.x.handle), C.c_uint64(h), C.c_int(0), C.byref(P), C.byref(ok)) == -3
    assert lib.gm_snark_verify(mats, C.c_uint64(r.x.handle), C.c_uint64(r.z.handle), C.c_int(0), C.byref(P), C.byref(ok)) == -3  # a vector is no key
    foreign = (C.c_uint64 * 3)(r.a.handle, r.z.handle, r.c.handle)
    assert lib.gm_snark_verify(foreign, C.c_uint64(r.x.handle), C.c_uint64(K["vk"].handle), C.c_int(0), C.byref(P), C.byref(ok)) == -3
    out = np.zeros(18, dtype=np.uint64)
    assert lib.gm_kzg_verify(C.c_uint64(h), gm.capi.ptr(out), gm.capi.ptr(out), gm.capi.ptr(out), gm.capi.ptr(out), C.byref(ok)) == -3
    assert ok.value == -7


def test_two_threads_verify_two_proofs_at_once(gm, oracle, pyref):
    from gemini_amd.kzg import VerificationError

    cases = [_snark_case(gm, oracle, pyref, "dummy", 1 << 8), _snark_case(gm, oracle, pyref, "random", 16)]
    bad = [_snark_tamper(gm, pyref, K["proof"], "base_evaluation") for K in cases]
    results, errors = {}, []

    def work(i):
        try:
            K = cases[i]
            for it in range(4):
                K["proof"].verify(K["r1cs"], K["vk"])
                try:
                    bad[i].verify(K["r1cs"], K["vk"])
                    results[(i, it)] = "accepted an altered proof"
                except VerificationError:
                    results[(i, it)] = "ok"
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert results == {(i, it): "ok" for i in range(2) for it in range(4)}


def test_snark_verify_at_2p20_constraints(gm, oracle, pyref):
    """the size at which the Python verifier needs the C restatement of the matrix evaluations: device only"""
    from gemini_amd.circuit import dummy_r1cs
    from gemini_amd.kzg import CommitterKey, VerificationError, VerifierKey
    from gemini_amd.snark import Proof

    n = 1 << 20
    e, tau = 0x1D2C3B4A59687766554433221100FFEE % pyref.R_MOD, 0x0123456789ABCDEF0FEDCBA987654321 % pyref.R_MOD
    ck = CommitterKey.new(2 * n, 5, _limbs(oracle, tau))
    vk = VerifierKey.from_committer_key(ck)
    r1cs = dummy_r1cs(e, n)
    proof = Proof.new_time(r1cs, ck)
    proof.verify(r1cs, vk)
    fe = proof.tensorcheck_proof.folded_polynomials_evaluations
    last = np.array(fe[-1], dtype=np.uint64).reshape(2, 4)
    last[1] = _bump(gm, pyref, last[1])
    fe[-1] = last
    with pytest.raises(VerificationError):
        proof.verify(r1cs, vk)
    r1cs.free()
    vk.free()
    ck.powers_of_g.free()


# ---- psnark --------------------------------------------------------------------------------------------------------------------
_PSNARK_CACHE = {}


def _psnark_case(gm, oracle, pyref, kind, n):
    from gemini_amd.circuit import dummy_r1cs
    from gemini_amd.kzg import CommitterKey, VerifierKey
    from gemini_amd.psnark import Proof
    from oracle import psnark_ref as pr
    from oracle import snark_ref as sr
    from oracle import verifier_ref as V
    from tests.util import jac_to_affine_ints, random_r1cs_instance

    if (kind, n) not in _PSNARK_CACHE:
        if kind == "dummy":
            e, tau = 987654321987654321, 1234567890123456789012345
            inst, r1cs = sr.dummy_r1cs(e, n), dummy_r1cs(e, n)
        else:
            inst, tau = random_r1cs_instance(pyref, sr, n, 2024)
            r1cs = _device_instance(gm, inst, n)
        jm = pr.sum_matrices(inst["a"], inst["b"], inst["c"], n)
        nnz = len(pr.joint_matrices(jm, inst["a"], inst["b"], inst["c"])[0])
        ck = CommitterKey.new(nnz + 2 * n + 1, 3, _limbs(oracle, tau))  # nnz + 2 n + 2 powers
        index = Proof.index(ck, r1cs)
        _PSNARK_CACHE[(kind, n)] = {"inst": inst, "r1cs": r1cs, "ck": ck, "vk": VerifierKey.from_committer_key(ck), "ovk": V.VerifierKey.from_trapdoor(tau, 3),
                                    "index": index, "index_ints": [jac_to_affine_ints(oracle, c) for c in index], "nnz": nnz,
                                    "proof": Proof.new_time(ck, r1cs, index), "tau": tau}
    return _PSNARK_CACHE[(kind, n)]


@pytest.mark.parametrize("kind,n", [("dummy", 1 << 3), ("dummy", 1 << 6), ("random", 8)])
def test_psnark_device_proofs_are_accepted(gm, oracle, pyref, kind, n):
    from gemini_amd.psnark import Proof
    from oracle import verifier_ref as V
    from tests.util import psnark_proof_to_ints

    K = _psnark_case(gm, oracle, pyref, kind, n)
    K["proof"].verify(K["r1cs"], K["vk"], K["index"], K["nnz"])
    K["proof"].verify(K["r1cs"], K["vk"], K["index"])  # the number of non-zero entries computed from the instance
    assert _verdict(V.psnark_verify, psnark_proof_to_ints(gm, oracle, K["proof"]), K["inst"], K["ovk"], K["index_ints"], K["nnz"])
    Proof.deserialize(K["proof"].serialize(True), True).verify(K["r1cs"], K["vk"], K["index"], K["nnz"])


def _psnark_alterations(gm, pyref, proof):
    """(name, altered copy): one altered element of every field of a psnark::Proof (the keys of tests.util.psnark_proof_to_ints)"""
    B = lambda x: _bump(gm, pyref, x)  # noqa: E731

    def altered(fn):
        p = copy.deepcopy(proof)
        fn(p)
        return p

    def at(container, i, f):
        def go(p):
            c = container(p)
            c[i] = f(c[i])
        return go

    def row(i, f):
        def go(x):
            x = np.array(x, dtype=np.uint64).reshape(-1, 4)
            x[i] = f(x[i])
            return x
        return go

    for name in ("witness_commitment", "z_star_commitment", "sorted_r_commitment", "sorted_alpha_commitment", "sorted_z_commitment", "ralpha_star_acc_mu_proof"):
        yield name, altered(lambda p, name=name: setattr(p, name, _double(getattr(p, name))))
    for name in ("zc_alpha", "set_r_ep", "subset_r_ep", "set_alpha_ep", "subset_alpha_ep", "set_z_ep", "subset_z_ep"):
        yield name, altered(lambda p, name=name: setattr(p, name, B(getattr(p, name))))
    for name in ("first_sumcheck_msgs", "second_sumcheck_msgs", "third_sumcheck_msgs"):
        def message(p, name=name):
            msgs, ff = getattr(p, name)
            msgs = list(msgs)
            msgs[1] = (msgs[1][0], B(msgs[1][1]))
            setattr(p, name, (msgs, ff))

        def final(p, name=name):
            msgs, ff = getattr(p, name)
            ff = list(ff)
            ff[-1] = (ff[-1][0], B(ff[-1][1]))
            setattr(p, name, (msgs, ff))

        yield name + ":message", altered(message)
        yield name + ":final", altered(final)
    yield "r_star_commitments", altered(at(lambda p: p.r_star_commitments, 1, _double))
    yield "ep_msgs.acc_v_commitments", altered(at(lambda p: p.ep_msgs.acc_v_commitments, 8, _double))
    yield "ep_msgs.claimed_sumchecks", altered(at(lambda p: p.ep_msgs.claimed_sumchecks, 4, B))
    yield "ralpha_star_acc_mu_evals", altered(at(lambda p: p.ralpha_star_acc_mu_evals, 3, B))
    yield "rstars_vals", altered(at(lambda p: p.rstars_vals, 1, B))
    yield "tensorcheck.folded_commitments", altered(at(lambda p: p.tensorcheck_proof.folded_polynomials_commitments, 0, _double))
    yield "tensorcheck.folded_evaluations", altered(at(lambda p: p.tensorcheck_proof.folded_polynomials_evaluations, 0, row(1, B)))
    yield "tensorcheck.base_evaluations", altered(at(lambda p: p.tensorcheck_proof.base_polynomials_evaluations, 17, row(2, B)))
    yield "tensorcheck.evaluation_proof", altered(lambda p: setattr(p.tensorcheck_proof, "evaluation_proof", _double(p.tensorcheck_proof.evaluation_proof)))


def test_psnark_rejects_one_altered_element_of_every_field(gm, oracle, pyref):
    from gemini_amd.kzg import VerificationError
    from tests.util import psnark_proof_to_ints

    K = _psnark_case(gm, oracle, pyref, "random", 8)
    seen = set()
    for name, bad in _psnark_alterations(gm, pyref, K["proof"]):
        assert bad != K["proof"], name
        with pytest.raises(VerificationError):
            bad.verify(K["r1cs"], K["vk"], K["index"], K["nnz"])
        seen.add(name.split(":")[0].split(".")[0].replace("tensorcheck", "tensorcheck_proof"))
    assert seen == set(psnark_proof_to_ints(gm, oracle, K["proof"]).keys())  # no field of the proof was left out
    K["proof"].verify(K["r1cs"], K["vk"], K["index"], K["nnz"])


def test_psnark_verdicts_equal_the_oracle_on_altered_proofs(gm, oracle, pyref):
    """three alterations that are caught at three different places (second sumcheck, the opening at mu, the tensor check)"""
    from oracle import verifier_ref as V
    from tests.util import psnark_proof_to_ints

    K = _psnark_case(gm, oracle, pyref, "dummy", 1 << 3)
    picked = {"second_sumcheck_msgs:final", "ralpha_star_acc_mu_evals", "tensorcheck.base_evaluations"}
    for name, bad in _psnark_alterations(gm, pyref, K["proof"]):
        if name in picked:
            got = _verdict(bad.verify, K["r1cs"], K["vk"], K["index"], K["nnz"])
            assert got == _verdict(V.psnark_verify, psnark_proof_to_ints(gm, oracle, bad), K["inst"], K["ovk"], K["index_ints"], K["nnz"]) == False  # noqa: E712


def test_psnark_rejects_a_wrong_index_commitment_and_a_wrong_count(gm, oracle, pyref):
    from gemini_amd.kzg import VerificationError

    K = _psnark_case(gm, oracle, pyref, "random", 8)
    swapped = [K["index"][1], K["index"][0]] + list(K["index"][2:])
    with pytest.raises(VerificationError):
        K["proof"].verify(K["r1cs"], K["vk"], swapped, K["nnz"])
    with pytest.raises(VerificationError):
        K["proof"].verify(K["r1cs"], K["vk"], K["index"], K["nnz"] + 1)


def test_psnark_example_key_is_one_power_short(gm, oracle, pyref):
    """examples/psnark.rs:76: 2 n + 1 powers for dummy_r1cs(n) drop the top coefficient of three commitments and the proof is REJECTED;
    one more power and it is accepted (the oracle finds the same: tests/test_oracle_verifier.py)"""
    from gemini_amd.circuit import dummy_r1cs
    from gemini_amd.kzg import CommitterKey, VerifierKey
    from gemini_amd.psnark import Proof

    import warnings

    n = 16
    e, tau = 987654321987654321, 1234567890123456789012345
    r1cs = dummy_r1cs(e, n)
    verdict = {}
    for max_degree in (2 * n, 2 * n + 1):
        ck = CommitterKey.new(max_degree, 5, _limbs(oracle, tau))
        vk = VerifierKey.from_committer_key(ck)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            index = Proof.index(ck, r1cs)
            proof = Proof.new_time(ck, r1cs, index)
        verdict[max_degree] = _verdict(proof.verify, r1cs, vk, index, n)
        vk.free()
        ck.powers_of_g.free()
    assert verdict == {2 * n: False, 2 * n + 1: True}
    r1cs.free()
