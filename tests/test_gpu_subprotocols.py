"""GPU: the sub-protocols as stand-alone entries of the library -- the device-built extended frequency (gm_idx_extend_frequency), plookup
(gm_plookup_new_time), the entry product (gm_entryproduct_new_time_batch) and the tensor check (gm_tensorcheck_new_time) -- through the
product-side Python surface (gemini_amd.plookup / .entryproduct / .tensorcheck) and the C++ mirror, against numpy, the CPU restatements
(oracle/psnark_ref.py, oracle/snark_ref.py) and the reference verifier's restatement (oracle/verifier_ref.py)."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests.util import jac_to_affine_ints, random_r1cs_instance

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GM_EINVAL = -1
PROTOCOL = b"LTAPS-2019"  # tensorcheck/tests.rs:13
TAU_SEED, SRS_LEN = 4201, 1100


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


@pytest.fixture(scope="module")
def key(gm, oracle):
    """(tau, the oracle's SRS of SRS_LEN powers, the device key over the same trapdoor)"""
    from gemini_amd.kzg import CommitterKey
    from oracle import snark_ref as sr

    tau = oracle.limbs_to_ints(oracle.random_fr(TAU_SEED, 1))[0]
    ck = CommitterKey.new(SRS_LEN - 1, 5, oracle.ints_to_limbs([tau], 4)[0])
    yield tau, sr.srs(tau, SRS_LEN), ck
    ck.powers_of_g.free()


def _M(orc, ints):
    return orc.fr_to_mont(orc.ints_to_limbs(ints, 4)) if len(ints) else np.empty((0, 4), dtype=np.uint64)


def _I(orc, mont):
    return orc.limbs_to_ints(orc.fr_from_mont(np.asarray(mont, dtype=np.uint64).reshape(-1, 4)))


def _rand_ints(orc, seed, n):
    return orc.limbs_to_ints(orc.random_fr(seed, n)) if n else []


# ---- 1. extend_frequency --------------------------------------------------------------------------------------------------------
def _expected_ext(index, set_len):
    return np.repeat(np.arange(set_len, dtype=np.uint32), 1 + np.bincount(index, minlength=set_len))


def _indices(set_len, k, seed):
    """the index distributions of one size: uniform random, every entry the first / the last set element, sorted, reversed"""
    if k == 0:
        return {"empty": np.empty(0, dtype=np.uint32)}
    uni = np.random.default_rng(seed).integers(0, set_len, size=k).astype(np.uint32)
    srt = np.sort(uni)
    return {"uniform": uni, "all_first": np.zeros(k, dtype=np.uint32), "all_last": np.full(k, set_len - 1, dtype=np.uint32), "sorted": srt,
            "reversed": np.ascontiguousarray(srt[::-1])}


@pytest.mark.parametrize("set_len,k", [(1, 0), (1, 5), (5, 3), (7, 1 << 20), (1000, 3000), ((1 << 16) + 3, 1 << 18), (1 << 20, 1 << 10), (1 << 20, 1 << 22)])
def test_extend_frequency_matches_numpy(gm, set_len, k):
    from gemini_amd.fr import IdxVec
    from gemini_amd.plookup import extend_frequency_device

    for name, index in _indices(set_len, k, 17 * set_len + k).items():
        didx = IdxVec.from_host(index)
        ext = extend_frequency_device(didx, set_len)
        got = ext.to_host()
        want = _expected_ext(index, set_len)
        assert len(ext) == set_len + k == len(want), name
        assert np.array_equal(got, want), (name, int(np.flatnonzero(got != want)[0]))
        ext.free()
        didx.free()


def test_extend_frequency_of_nothing(gm):
    from gemini_amd.fr import IdxVec
    from gemini_amd.plookup import extend_frequency_device

    didx = IdxVec.from_host(np.empty(0, dtype=np.uint32))
    ext = extend_frequency_device(didx, 0)
    assert len(ext) == 0 and ext.to_host().size == 0
    ext.free()
    didx.free()


def test_extend_frequency_equals_preprocess(gm, oracle, pyref):
    """the ext_fre_row / ext_fre_col that gm_psnark_preprocess builds with its host loop for a random general R1CS, entry for entry"""
    from gemini_amd.circuit import R1cs, SparseMatrix
    from gemini_amd.fr import IdxVec
    from gemini_amd.plookup import extend_frequency_device
    from gemini_amd.psnark import _joint_native
    from oracle import snark_ref as sr

    n = 96
    inst, _ = random_r1cs_instance(pyref, sr, n, 8100)
    dev = lambda rows: [[(gm.fr.fr_from_int(v), col) for v, col in row] for row in rows]  # noqa: E731
    mats = [SparseMatrix.from_rows(dev(inst[k]), n) for k in "abc"] + [SparseMatrix.from_rows(dev(inst[k]), n, transpose=True) for k in "abc"]
    r1cs = R1cs(*mats, gm.FrVec.from_host(_M(oracle, inst["z"])), gm.FrVec.from_host(_M(oracle, inst["w"])), gm.FrVec.from_host(_M(oracle, inst["x"])))
    rec = _joint_native(r1cs).rec
    nnz = rec.nnz
    for index_h, ext_h, ext_len in ((rec.row_index, rec.ext_fre_row, rec.ext_fre_row_len), (rec.col_index, rec.ext_fre_col, rec.ext_fre_col_len)):
        index, host_built = IdxVec(index_h, nnz), IdxVec(ext_h, ext_len)  # views: the handles stay the instance's
        assert len(index) == nnz and len(host_built) == ext_len
        ext = extend_frequency_device(index, ext_len - nnz)
        assert np.array_equal(ext.to_host(), host_built.to_host())
        ext.free()
    r1cs.free()


def test_extend_frequency_rejects_out_of_range(gm):
    """an entry == set_len or 2^32 - 1 is GM_EINVAL, registers nothing and leaves the context usable.  Safe by construction: the kernel
    compares every entry with set_len before it is used as an address and skips the ones that fail."""
    from gemini_amd import capi
    from gemini_amd.fr import IdxVec
    from gemini_amd.plookup import extend_frequency_device

    lib = capi.load()
    for set_len, k in ((1000, 3000), ((1 << 16) + 3, 5000)):  # the LDS-privatised and the global counting kernel
        good = np.random.default_rng(5).integers(0, set_len, size=k).astype(np.uint32)
        for bad_value in (set_len, 0xFFFFFFFF):
            index = good.copy()
            index[k // 2] = bad_value
            didx = IdxVec.from_host(index)
            in_use = capi.mem_stats()["in_use"]
            h, n = C.c_uint64(0), C.c_size_t(0)
            assert lib.gm_idx_extend_frequency(C.c_uint64(didx.handle), C.c_size_t(set_len), C.byref(h), C.byref(n)) == GM_EINVAL
            assert b"outside the set" in lib.gm_last_error()
            assert h.value == 0 and capi.mem_stats()["in_use"] == in_use
            with pytest.raises(capi.GeminiHipError):
                extend_frequency_device(didx, set_len)
            didx.free()
            dgood = IdxVec.from_host(good)
            ext = extend_frequency_device(dgood, set_len)
            assert np.array_equal(ext.to_host(), _expected_ext(good, set_len))
            ext.free()
            dgood.free()


# ---- 2. plookup -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nset,nidx", [(6, 4), (1000, 3000), ((1 << 12) + 1, 1 << 14)])
def test_plookup_matches_the_restatement(gm, oracle, pyref, nset, nidx):
    from gemini_amd import capi
    from gemini_amd.fr import FrVec, IdxVec
    from gemini_amd.plookup import extend_frequency_device, plookup
    from oracle import psnark_ref as pr

    R = pyref.R_MOD
    if (nset, nidx) == (6, 4):  # plookup/time_prover.rs:114-148 test_plookup_relation
        set_, index, y, z = [10, 12, 13, 14, 15, 42], np.array([0, 2, 4, 5], dtype=np.uint32), 47, 52
        zeta = oracle.limbs_to_ints(oracle.random_fr(77, 1))[0]
    else:
        set_ = _rand_ints(oracle, 100 + nset, nset)
        index = np.random.default_rng(nset).integers(0, nset, size=nidx).astype(np.uint32)
        y, z, zeta = _rand_ints(oracle, 200 + nset, 3)
    subset = pr.lookup(set_, index.tolist())
    dset, dsub, didx = FrVec.from_host(_M(oracle, set_)), FrVec.from_host(_M(oracle, subset)), IdxVec.from_host(index)
    kept = extend_frequency_device(didx, nset)
    lib = capi.load()

    def product(v):
        out = np.zeros(4, dtype=np.uint64)
        capi.check(lib.gm_fr_product(C.c_uint64(v.handle), capi.ptr(out)))
        return gm.fr.fr_to_int(out)

    for zt in (0, zeta):
        mont = lambda v: _M(oracle, [v])[0]  # noqa: E731
        got = plookup(dsub, dset, didx, mont(y), mont(z), mont(zt))
        want = pr.plookup(subset, set_, index.tolist(), y, z, zt)
        host = [v.to_host() for v in got]
        assert [len(h) for h in host] == [nset + 1, nidx, nset + nidx + 1]
        for k in range(3):
            assert _I(oracle, host[k]) == want[k], (zt != 0, k)
        assert product(got[2]) == product(got[0]) * product(got[1]) % R * pow(1 + z, nidx, R) % R
        again = plookup(dsub, dset, didx, mont(y), mont(z), mont(zt), ext_fre=kept)  # a caller-held extended frequency: identical vectors
        for k in range(3):
            assert np.array_equal(again[k].to_host(), host[k])
        for v in got + again:
            v.free()
    # the zip of the reference: with zeta != 0 a subset longer than the index is cut to the index, with zeta = 0 it is not
    longer = FrVec.from_host(_M(oracle, subset + [5, 6]))
    cut = plookup(longer, dset, didx, _M(oracle, [y])[0], _M(oracle, [z])[0], _M(oracle, [zeta])[0])
    whole = plookup(longer, dset, didx, _M(oracle, [y])[0], _M(oracle, [z])[0], _M(oracle, [0])[0])
    assert len(cut[1]) == nidx and len(whole[1]) == nidx + 2
    for v in cut + whole + [longer, dset, dsub]:
        v.free()
    kept.free()
    didx.free()


# ---- 3. entry product -----------------------------------------------------------------------------------------------------------
def _entry_product_case(gm, oracle, pyref, key, lens, seed, single):
    from gemini_amd.entryproduct import EntryProduct
    from gemini_amd.fr import FrVec, accumulated_product_monic
    from gemini_amd.transcript import Transcript
    from oracle import psnark_ref as pr
    from oracle import verifier_ref as V

    _, srs, ck = key
    vs = [_rand_ints(oracle, seed + i, n) for i, n in enumerate(lens)]
    products = [pr.product(v) for v in vs]
    tr = pyref.GeminiTranscript(PROTOCOL)
    want_msgs, want_chal, _ = pr.entry_product_new_time_batch(tr, srs, vs, products)
    J = lambda p: jac_to_affine_ints(oracle, p)  # noqa: E731
    F = gm.fr.fr_to_int

    def same_as_oracle(ep):
        assert [J(c) for c in ep.msgs.acc_v_commitments] == want_msgs["acc_v_commitments"]
        assert [F(s) for s in ep.msgs.claimed_sumchecks] == want_msgs["claimed_sumchecks"]
        assert F(ep.chal) == want_chal

    # (a) the accumulated vectors built inside the call; the inputs are freed BEFORE the sumcheck runs: the provers own their data
    dvs = [FrVec.from_host(_M(oracle, v)) for v in vs]
    t = Transcript(PROTOCOL)
    cps = [_M(oracle, [p])[0] for p in products]
    ep = EntryProduct.new_time(t, ck, dvs[0], cps[0]) if single else EntryProduct.new_time_batch(t, ck, dvs, cps)
    same_as_oracle(ep)
    for v in dvs:
        v.free()
    scratch = [FrVec.alloc(max(lens) + 1) for _ in range(4)]  # the pool hands the freed blocks out again: overwrite them
    for s in scratch:
        s.fill(_M(oracle, [7])[0])
    sc = gm.Sumcheck.prove_batch(t, ep.provers)
    msgs = [(F(a), F(b)) for a, b in sc.messages]
    finals = [(F(a), F(b)) for a, b in sc.final_foldings]
    V.subclaim_new_batch(tr, msgs, finals, want_msgs["claimed_sumchecks"])  # the oracle's transcript, after its own entry product
    assert F(t.get_challenge(b"next")) == tr.get_challenge(b"next")
    tr2 = pyref.GeminiTranscript(PROTOCOL)
    pr.entry_product_new_time_batch(tr2, srs, vs, products)
    with pytest.raises(V.VerificationError):  # (the verifier is not vacuous: a wrong claimed sum is refused)
        V.subclaim_new_batch(tr2, msgs, finals, [(s + 1) % pyref.R_MOD for s in want_msgs["claimed_sumchecks"]])
    ep.free()
    for s in scratch:
        s.free()
    t.free()
    # (b) the caller holds the accumulated vectors already: identical outputs, and the transcript's next challenge is the oracle's
    dvs = [FrVec.from_host(_M(oracle, v)) for v in vs]
    accs = [accumulated_product_monic(v) for v in dvs]
    t = Transcript(PROTOCOL)
    ep2 = EntryProduct.new_time_batch(t, ck, dvs, cps, acc_vs=accs)
    same_as_oracle(ep2)
    tr3 = pyref.GeminiTranscript(PROTOCOL)
    pr.entry_product_new_time_batch(tr3, srs, vs, products)
    assert F(t.get_challenge(b"next")) == tr3.get_challenge(b"next")
    ep2.free()
    for v in dvs + accs:
        v.free()
    t.free()
    return want_msgs, want_chal


def test_entry_product_batch(gm, oracle, pyref, key):
    _entry_product_case(gm, oracle, pyref, key, (1000, 257, 1), 3100, single=False)


def test_entry_product_new_time(gm, oracle, pyref, key):
    _entry_product_case(gm, oracle, pyref, key, (1000,), 3200, single=True)  # the reference's test size (entryproduct/tests.rs)


# ---- 4. tensor check ------------------------------------------------------------------------------------------------------------
def _tensorcheck_shape(oracle, shape):
    """(base polynomials, [(indices of the body's polynomials, challenges)]) as integers"""
    if shape == "a":  # tensorcheck/tests.rs:16-86: d = 8, one base, one body
        polys = [_rand_ints(oracle, 5100, 8)]
        bodies = [([0], _rand_ints(oracle, 5101, 3))]
    elif shape == "b":  # three bases of unequal lengths, two bodies: 7 + 5 foldings
        polys = [_rand_ints(oracle, 5200 + i, n) for i, n in enumerate((256, 200, 64))]
        bodies = [([0, 1], _rand_ints(oracle, 5210, 8)), ([2], _rand_ints(oracle, 5211, 6))]
    else:  # a body that folds nothing (one challenge: no batched polynomial, no level) in front of one that folds twice
        polys = [_rand_ints(oracle, 5400, 8), _rand_ints(oracle, 5401, 5)]
        bodies = [([0], _rand_ints(oracle, 5410, 1)), ([0, 1], _rand_ints(oracle, 5411, 3))]
    return polys, bodies


def _tc_to_ints(gm, oracle, tc):
    F = gm.fr.fr_to_int
    J = lambda p: jac_to_affine_ints(oracle, p)  # noqa: E731
    return {"folded_polynomials_commitments": [J(c) for c in tc.folded_polynomials_commitments],
            "folded_polynomials_evaluations": [[F(x) for x in e2] for e2 in tc.folded_polynomials_evaluations],
            "evaluation_proof": J(tc.evaluation_proof),
            "base_polynomials_evaluations": [[F(x) for x in e3] for e3 in tc.base_polynomials_evaluations]}


@pytest.mark.parametrize("shape", ["a", "b", "c"])
def test_tensorcheck_prove_verify(gm, oracle, pyref, key, shape):
    from gemini_amd import capi, wire
    from gemini_amd.fr import FrVec
    from gemini_amd.tensorcheck import TensorcheckProof
    from gemini_amd.transcript import Transcript
    from oracle import snark_ref as sr
    from oracle import verifier_ref as V

    R = pyref.R_MOD
    tau, srs, ck = key
    polys, bodies = _tensorcheck_shape(oracle, shape)
    dpolys = [FrVec.from_host(_M(oracle, p)) for p in polys]
    dbodies = [([dpolys[i] for i in idx], _M(oracle, ch)) for idx, ch in bodies]
    nfold = sum(len(ch) - 1 for _, ch in bodies)
    assert nfold == {"a": 2, "b": 12, "c": 2}[shape]
    t = Transcript(PROTOCOL)
    tc = TensorcheckProof.new_time(t, ck, dpolys, dbodies)
    tr = pyref.GeminiTranscript(PROTOCOL)
    want = sr.tensorcheck_new_time(tr, srs, polys, [([polys[i] for i in idx], ch) for idx, ch in bodies])
    got = _tc_to_ints(gm, oracle, tc)
    for field in ("folded_polynomials_commitments", "folded_polynomials_evaluations", "evaluation_proof", "base_polynomials_evaluations"):
        assert got[field] == want[field], field
    assert gm.fr.fr_to_int(t.get_challenge(b"next")) == tr.get_challenge(b"next")
    t.free()
    # (shape c is the prover's path alone: its first body pairs 8 coefficients with the tensor of ONE challenge, which no verifier is handed)
    if shape != "c":
        # the verifier (tensorcheck/mod.rs:286-392, pairing check included), driven as tensorcheck/tests.rs:45-85 drives it
        vk = V.VerifierKey.from_trapdoor(tau, 5)
        trv = pyref.GeminiTranscript(PROTOCOL)
        batch_challenge = trv.get_challenge(b"batch_challenge")
        for c in got["folded_polynomials_commitments"]:
            trv.append_message(b"commitment", pyref.g1_serialize_uncompressed(c))
        eval_chal = trv.get_challenge(b"evaluation-chal")
        asserted, direct = [], []
        for idx, ch in bodies:
            tensor = pyref.tensor(ch)
            asserted.append([pyref.ip(polys[i], tensor[:len(polys[i])]) for i in idx])
            e0 = e1 = 0
            for j, i in enumerate(idx):
                w = pow(batch_challenge, j, R)
                e0 = (e0 + w * got["base_polynomials_evaluations"][i][1]) % R
                e1 = (e1 + w * got["base_polynomials_evaluations"][i][2]) % R
            direct.append([e0, e1])
        base_commitments = [sr.commit(srs, p) for p in polys]
        V.tensorcheck_verify(got, trv, vk, asserted, base_commitments, direct, [ch for _, ch in bodies], eval_chal, batch_challenge)
    # the proof record round-trips through the wire schema
    for compress in (True, False):
        back = wire.deserialize(wire.TENSORCHECK_PROOF, wire.serialize(wire.TENSORCHECK_PROOF, tc, compress=compress), compress=compress)
        assert wire.equal(wire.TENSORCHECK_PROOF, tc, back)
    # room for one folding too few: GM_EINVAL, and nothing is left allocated
    in_use = capi.mem_stats()["in_use"]
    t = Transcript(PROTOCOL)
    with pytest.raises(capi.GeminiHipError) as err:
        TensorcheckProof.new_time(t, ck, dpolys, dbodies, cap_folds=nfold - 1)
    assert err.value.code == GM_EINVAL
    t.free()
    assert capi.mem_stats()["in_use"] == in_use
    for v in dpolys:
        v.free()


def test_tensorcheck_rejects_empty_bodies(gm, oracle, key):
    from gemini_amd import capi
    from gemini_amd.fr import FrVec
    from gemini_amd.tensorcheck import TensorcheckProof
    from gemini_amd.transcript import Transcript

    _, _, ck = key
    p = FrVec.from_host(_M(oracle, _rand_ints(oracle, 5300, 8)))
    t = Transcript(PROTOCOL)
    for bodies in ([], [([], _M(oracle, [1, 2, 3]))]):
        with pytest.raises(capi.GeminiHipError) as err:
            TensorcheckProof.new_time(t, ck, [p], bodies)
        assert err.value.code == GM_EINVAL
    # a body with ONE challenge folds nothing (strip_last): no commitments, the opening covers the base alone
    tc = TensorcheckProof.new_time(t, ck, [p], [([p], _M(oracle, [5]))])
    assert tc.folded_polynomials_commitments == [] and len(tc.base_polynomials_evaluations) == 1
    t.free()
    p.free()


# ---- 5. the product surface alone -----------------------------------------------------------------------------------------------
_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
import numpy as np
import gemini_amd as gm
from gemini_amd.entryproduct import EntryProduct
from gemini_amd.fr import FrVec
from gemini_amd.kzg import CommitterKey
from gemini_amd.tensorcheck import TensorcheckProof
from gemini_amd.transcript import Transcript
gm.capi.init()
d = np.load({inputs!r})
ck = CommitterKey.new({srs_len} - 1, 5, d["tau"])
t = Transcript({protocol!r})
ep = EntryProduct.new_time(t, ck, FrVec.from_host(d["v"]), d["product"])
print("ep", ep.msgs.acc_v_commitments[0].tobytes().hex(), ep.msgs.claimed_sumchecks[0].tobytes().hex())
t = Transcript({protocol!r})
p = FrVec.from_host(d["poly"])
tc = TensorcheckProof.new_time(t, ck, [p], [([p], d["randomness"])])
print("tc", b"".join(c.tobytes() for c in tc.folded_polynomials_commitments).hex(), tc.evaluation_proof.tobytes().hex())
assert not any(m == "tests" or m.startswith("tests.") for m in sys.modules), "the tests package was imported"
"""


def test_product_surface_without_the_tests_package(gm, oracle, pyref, key, tmp_path):
    """one entry product and one tensor check through gemini_amd alone, in a child interpreter that never sees tests.*"""
    from oracle import psnark_ref as pr
    from oracle import snark_ref as sr

    tau, srs, _ = key
    v = _rand_ints(oracle, 6100, 300)
    polys, bodies = _tensorcheck_shape(oracle, "a")
    inputs = str(tmp_path / "inputs.npz")
    np.savez(inputs, tau=oracle.ints_to_limbs([tau], 4)[0], v=_M(oracle, v), product=_M(oracle, [pr.product(v)])[0], poly=_M(oracle, polys[0]),
             randomness=_M(oracle, bodies[0][1]))
    out = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", _CHILD.format(root=ROOT, inputs=inputs, srs_len=SRS_LEN, protocol=PROTOCOL)],
                         capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith(("ep ", "tc "))}
    J = lambda hexs: jac_to_affine_ints(oracle, np.frombuffer(bytes.fromhex(hexs), dtype=np.uint64))  # noqa: E731
    want_msgs, _, _ = pr.entry_product_new_time_batch(pyref.GeminiTranscript(PROTOCOL), srs, [v], [pr.product(v)])
    assert J(lines["ep"][0]) == want_msgs["acc_v_commitments"][0]
    assert gm.fr.fr_to_int(np.frombuffer(bytes.fromhex(lines["ep"][1]), dtype=np.uint64)) == want_msgs["claimed_sumchecks"][0]
    want = sr.tensorcheck_new_time(pyref.GeminiTranscript(PROTOCOL), srs, polys, [([polys[0]], bodies[0][1])])
    fc = np.frombuffer(bytes.fromhex(lines["tc"][0]), dtype=np.uint64).reshape(-1, 18)
    assert [jac_to_affine_ints(oracle, c) for c in fc] == want["folded_polynomials_commitments"]
    assert J(lines["tc"][1]) == want["evaluation_proof"]


# ---- 6. the C++ mirror ----------------------------------------------------------------------------------------------------------
def _wvec(fh, arr):
    arr = np.ascontiguousarray(arr)
    fh.write(struct.pack("<Q", arr.shape[0]))
    fh.write(arr.tobytes())


def test_cpp_mirror(gm, oracle, pyref, key, tmp_path):
    """tests/cpp/test_subprotocols.cpp, built against include/gemini_hip.hpp only: entry product + Sumcheck::prove_batch, the tensor check of
    shape (a), plookup with a device-built and a caller-held extended frequency"""
    from oracle import psnark_ref as pr
    from oracle import snark_ref as sr
    from oracle import verifier_ref as V

    exe = str(tmp_path / "test_subprotocols")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_subprotocols.cpp"),
                           "-L", os.path.join(ROOT, "gemini_amd"), "-lgemini_hip", "-Wl,-rpath," + os.path.join(ROOT, "gemini_amd"), "-o", exe])
    _, srs, _ = key
    srs_rust = np.zeros((len(srs), 13), dtype=np.uint64)
    srs_rust[:, :12] = srs
    vs = [_rand_ints(oracle, 7100, 600), _rand_ints(oracle, 7101, 33)]
    products = [pr.product(v) for v in vs]
    polys, bodies = _tensorcheck_shape(oracle, "a")
    set_ = _rand_ints(oracle, 7200, 50)
    index = np.random.default_rng(72).integers(0, 50, size=120).astype(np.uint32)
    y, z, zeta = _rand_ints(oracle, 7201, 3)
    inp = str(tmp_path / "in.bin")
    with open(inp, "wb") as fh:
        for a in (srs_rust, _M(oracle, vs[0]), _M(oracle, vs[1]), _M(oracle, products), _M(oracle, polys[0]), _M(oracle, bodies[0][1]), _M(oracle, set_), index,
                  _M(oracle, [y, z, zeta])):
            _wvec(fh, a)
    out = subprocess.run(["timeout", "-k", "10", "300", exe, inp], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    vals = {}
    for line in out.stdout.splitlines():
        parts = line.split()
        vals.setdefault(parts[0], []).append(parts[1:])
    assert "FAILED" not in vals, out.stdout
    L = lambda key_, k=0: np.array([int(x, 16) for x in vals[key_][k]], dtype=np.uint64)  # noqa: E731
    A = lambda key_, k=0: jac_to_affine_ints(oracle, L(key_, k))  # noqa: E731
    F = lambda key_, k=0: gm.fr.fr_to_int(L(key_, k))  # noqa: E731
    tr = pyref.GeminiTranscript(pyref.PROTOCOL_NAME)
    want_msgs, want_chal, _ = pr.entry_product_new_time_batch(tr, srs, vs, products)
    assert [A("ep_acc_v", k) for k in range(2)] == want_msgs["acc_v_commitments"]
    assert [F("ep_claimed", k) for k in range(2)] == want_msgs["claimed_sumchecks"] and F("ep_chal") == want_chal
    msgs = [(F("ep_msg_a", k), F("ep_msg_b", k)) for k in range(len(vals["ep_msg_a"]))]
    finals = [(F("ep_ff_lhs", k), F("ep_ff_rhs", k)) for k in range(2)]
    V.subclaim_new_batch(tr, msgs, finals, want_msgs["claimed_sumchecks"])
    assert F("ep_after") == tr.get_challenge(b"after")
    tr = pyref.GeminiTranscript(pyref.PROTOCOL_NAME)
    want = sr.tensorcheck_new_time(tr, srs, polys, [([polys[0]], bodies[0][1])])
    assert [A("tc_fc", k) for k in range(len(vals["tc_fc"]))] == want["folded_polynomials_commitments"]
    assert [[F("tc_fe", 2 * k), F("tc_fe", 2 * k + 1)] for k in range(len(vals["tc_fe"]) // 2)] == want["folded_polynomials_evaluations"]
    assert A("tc_open") == want["evaluation_proof"]
    assert [[F("tc_be", k) for k in range(3)]] == want["base_polynomials_evaluations"]
    assert F("tc_after") == tr.get_challenge(b"after")
    assert vals["plookup_ext_equal"][0] == ["1"]
    want_sorted = pr.plookup(pr.lookup(set_, index.tolist()), set_, index.tolist(), y, z, zeta)[2]
    assert [F("plookup_sorted", k) for k in range(len(vals["plookup_sorted"]))] == want_sorted
    assert vals["error_path"][0] == [str(GM_EINVAL)]
