"""GPU: many proofs in one call through the C++ host mirror (gm::g1_lincomb_many, gm::multi_pairing_many,
gm::VerifierKey::verify_multi_points_many, gm::SnarkProof::verify_many in include/gemini_hip.hpp), compiled with g++ against
libgemini_hip.so: one KZG batch and one snark batch, each beside the single calls on the same inputs."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_verify_many_layer(tmp_path, oracle, pyref):
    from gemini_amd import g2 as G2
    from gemini_amd.fr import fr_from_int
    from gemini_amd.kzg import g1_generator_mont, g2_records

    exe = str(tmp_path / "test_verify_many")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_verify_many.cpp"),
                           "-L", os.path.join(ROOT, "gemini_amd"), "-lgemini_hip", "-Wl,-rpath," + os.path.join(ROOT, "gemini_amd"), "-o", exe])
    n = 16
    e, tau = 987654321987654321, 1234567890123456789012345
    words = np.concatenate([np.array([n], dtype=np.uint64), fr_from_int(e), fr_from_int(pow(e, -1, pyref.R_MOD)), oracle.ints_to_limbs([tau], 4)[0],
                            g1_generator_mont(), g2_records([G2.generator()])[0]]).astype(np.uint64)
    inp = str(tmp_path / "in.bin")
    words.tofile(inp)
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True, timeout=120).stdout
    got = dict(line.split(" ", 1) for line in out.strip().splitlines())
    want = {"lincomb": "11", "pairing": "111", "kzg_many": "1001", "kzg_singles": "1001", "kzg_none": "none",
            "snark_many": "1001", "snark_many_min_1": "1001", "snark_many_min_100": "1001", "snark_singles": "1001", "snark_none": "none",
            "snark_other_key": "0000"}
    assert got == want
