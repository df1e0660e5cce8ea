"""GPU: gm::InnerProductProof::new_many and gm::g2_lincomb_many of the C++ host mirror (include/gemini_hip.hpp) compiled with g++
against libgemini_hip.so.  The program goes through gemini_hip.hpp only: three proofs at d = 5 made in one call must equal the ones
made one by one, every proof must be accepted by verify_transcript and by verify_many, and a G2 commitment made as a short
combination must be commit_g2's."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import ipa_exponent_ref as X
from tests.test_gpu_ipa import mont, scalars
from tests.test_gpu_pairing import g1_points_to_affine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wvec(fh, arr):
    arr = np.ascontiguousarray(arr)
    fh.write(struct.pack("<Q", arr.shape[0]))
    fh.write(arr.tobytes())


def test_cpp_ipa_new_many_layer(tmp_path):
    from gemini_amd.fr import fr_from_int
    from gemini_amd.g2msm import g2_points_to_affine

    exe = str(tmp_path / "test_ipa_new_many_api")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_ipa_new_many_api.cpp"),
                           "-L", os.path.join(ROOT, "gemini_amd"), "-lgemini_hip", "-Wl,-rpath," + os.path.join(ROOT, "gemini_amd"), "-o", exe])
    n, d, S = 16, 5, 3
    p1, _, p2, _ = X.crs(n)
    g1, g2 = g1_points_to_affine(p1, flag=True), g2_points_to_affine(p2, flag=True)  # the 104- and 200-byte Rust records
    vecs = [(scalars(5100 + s, d), scalars(6100 + s, d)) for s in range(S)]
    y = np.stack([fr_from_int(X.ip(a, b)) for a, b in vecs])
    b0 = np.array([[(v >> (64 * i)) & (2**64 - 1) for i in range(4)] for v in vecs[0][1]], dtype=np.uint64)
    inp = str(tmp_path / "in.bin")
    with open(inp, "wb") as fh:
        _wvec(fh, g1)
        _wvec(fh, g2)
        for a, b in vecs:
            _wvec(fh, mont(a))
            _wvec(fh, mont(b))
        _wvec(fh, y)
        _wvec(fh, b0)
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True, timeout=120).stdout
    got = {ln.split()[0]: ln.split()[1:] for ln in out.strip().splitlines()}
    assert got["path"] == ["3", "0"] and got["made"] == ["3"]
    assert got["equal"] == ["1", "1", "1"]
    assert got["verify"] == ["1", "1", "1"] and got["verify_many"] == ["1", "1", "1"]
    assert got["none"] == ["0"] and got["refused"] == ["-1"]
    assert got["lincomb"] == ["1", "1"]
