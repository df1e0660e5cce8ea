"""GPU: the key-generation part of the C++ host mirror (gm::G2Bases::{fixed_base, srs, from_candidates},
CommitterKey::from_candidates, Crs::{from_scalars, from_candidates, truncate, halve, fold, bases, len} in include/gemini_hip.hpp)
compiled with g++ against libgemini_hip.so.  Every value it prints must equal what the Python mirror returns for the same call -- the
Python mirror itself is checked against integers in tests/test_gpu_keygen.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wvec(fh, arr):
    arr = np.ascontiguousarray(arr)
    fh.write(struct.pack("<Q", arr.shape[0]))
    fh.write(arr.tobytes())


def _words(arr) -> list:
    return [f"{int(w):016x}" for w in np.asarray(arr, dtype=np.uint64).reshape(-1)]


def test_cpp_keygen_layer(tmp_path):
    import gemini_amd as gm
    from gemini_amd.fr import fr_from_int
    from gemini_amd.points import candidate_stream
    from tests.test_gpu_keygen import LABEL, canon, g1_gen_record, g2_gen_record, mont, scalars

    exe = str(tmp_path / "test_keygen_api")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_keygen_api.cpp"),
                           "-L", os.path.join(ROOT, "gemini_amd"), "-lgemini_hip", "-Wl,-rpath," + os.path.join(ROOT, "gemini_amd"), "-o", exe])
    n, d = 5, 8
    a, b = scalars(301, n), scalars(302, n)
    b[1] = 0
    tau, c = scalars(303, 1), scalars(304, 1)[0]
    va, vb = mont(scalars(305, d)), mont(scalars(306, d))
    c1, c2 = candidate_stream(b"cpp", 1, 0, 128), candidate_stream(b"cpp", 2, 0, 128)
    inp = str(tmp_path / "in.bin")
    with open(inp, "wb") as fh:
        for arr in (g1_gen_record(), g2_gen_record(), canon(a), canon(b), canon(tau), np.frombuffer(c1, dtype=np.uint8), np.frombuffer(c2, dtype=np.uint8),
                    fr_from_int(c).reshape(1, 4), va, vb):
            _wvec(fh, arr)
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True, timeout=120).stdout
    got = {ln.split()[0]: ln.split()[1:] for ln in out.strip().splitlines()}
    ints = lambda tag: [int(x) for x in got[tag]]  # noqa: E731

    gm.capi.init()
    fb = gm.G2Bases.fixed_base(g2_gen_record(), canon(b))
    assert got["fixed_base"] == _words(fb.download()) and not fb.download()[1].any()
    srs = gm.G2Bases.srs(g2_gen_record(), canon(tau), 5)
    assert got["srs"] == _words(srs.download()) and ints("srs_check") == [1]
    k1, used, found = gm.G1Bases.from_candidates(c1, 6)
    assert ints("g1_cand") == [1, used, found] and got["g1_cand_points"] == _words(k1.download())
    k2, used, found = gm.G2Bases.from_candidates(c2, 6)
    assert ints("g2_cand") == [1, used, found] and got["g2_cand_points"] == _words(k2.download())
    none, used, found = gm.G2Bases.from_candidates(c2, 128)
    assert none is None and ints("g2_short") == [0, used, found] and used == 128 and found < 128

    def same_crs(tag, crs):
        p1, p2 = crs.bases()
        assert ints(tag + "_len") == [crs.n1, crs.n2] and got[tag + "_g1"] == _words(p1.download()) and got[tag + "_g2"] == _words(p2.download()), tag
        p1.free()
        p2.free()

    crs = gm.Crs.from_scalars(canon(a), canon(b))
    same_crs("crs", crs)
    for tag, new in (("fold", crs.fold(fr_from_int(c))), ("halve", crs.halve()), ("truncate", crs.truncate(1))):
        same_crs(tag, new)
        new.free()
    assert ints("truncate_all") == [n]
    same_crs("crs_after", crs)
    assert got["crs_after_g1"] == got["crs_g1"] and got["crs_after_g2"] == got["crs_g2"]
    # Crs::from_candidates is what Crs.new does with the stream of its seed
    fresh = gm.Crs.new(b"cpp", 16)
    assert ints("crs_from_candidates") == [1] and ints("fresh_check") == [1, 16, 16] and ints("crs_too_short") == [0]
    tr = gm.Transcript(LABEL)
    proof = gm.InnerProductProof.new(tr, fresh, va, vb)
    assert got["msg0"] == _words(proof.fields().messages[0, 0])
    for o in (proof, tr, fresh, crs, k1, k2, srs, fb):
        o.free()
