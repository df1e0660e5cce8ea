"""GPU: the verifiers of the C++ host mirror (gm::VerifierKey, gm::SnarkProof::verify, gm::PsnarkProof::verify in include/gemini_hip.hpp)
compiled with g++ against libgemini_hip.so: prove, verify, flip a limb, verify -- through gemini_hip.hpp only.  The key bytes it
prints must be the ones the Python mirror absorbs as b"ck"."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_verifier_layer(tmp_path, oracle, pyref):
    from gemini_amd import g2 as G2
    from gemini_amd.fr import fr_from_int
    from gemini_amd.kzg import g1_generator_mont, g2_records

    exe = str(tmp_path / "test_verifier")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_verifier.cpp"),
                           "-L", os.path.join(ROOT, "gemini_amd"), "-lgemini_hip", "-Wl,-rpath," + os.path.join(ROOT, "gemini_amd"), "-o", exe])
    n = 16
    e, tau = 987654321987654321, 1234567890123456789012345
    words = np.concatenate([np.array([n], dtype=np.uint64), fr_from_int(e), fr_from_int(pow(e, -1, pyref.R_MOD)), oracle.ints_to_limbs([tau], 4)[0],
                            g1_generator_mont(), g2_records([G2.generator()])[0]]).astype(np.uint64)
    inp = str(tmp_path / "in.bin")
    words.tofile(inp)
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True, timeout=120).stdout
    got = dict(line.split(" ", 1) for line in out.strip().splitlines())
    want = {"snark": "1", "snark_elastic": "1", "snark_zc_alpha": "0", "snark_fold_evaluation": "0", "snark_restored": "1", "snark_other_key": "0",
            "psnark": "1", "psnark_rstars": "0", "psnark_base_evaluation": "0", "psnark_count": "0", "psnark_restored": "1", "stale": "-3"}
    assert {k: v for k, v in got.items() if k != "g2_bytes"} == want
    ck_g2 = [G2.mul(G2.generator(), pow(tau, i, pyref.R_MOD)) for i in range(4)]
    assert bytes.fromhex(got["g2_bytes"]) == G2.serialize_vec_uncompressed(ck_g2, 0)
