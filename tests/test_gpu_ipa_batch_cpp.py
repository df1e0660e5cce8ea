"""GPU: gm::InnerProductProof::new_batch / verify_batch / claims of the C++ host mirror (include/gemini_hip.hpp) compiled with g++
against libgemini_hip.so.  The program goes through gemini_hip.hpp only: one proof for three claims at d = 5 must verify, must be
rejected for an altered y and for swapped commitments, one claim in a batch call must be the constructor's proof, and the refusals
must carry their codes."""
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


def test_cpp_ipa_batch_layer(tmp_path):
    from gemini_amd.fr import fr_from_int
    from gemini_amd.g2msm import g2_points_to_affine

    exe = str(tmp_path / "test_ipa_batch_api")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_ipa_batch_api.cpp"),
                           "-L", os.path.join(ROOT, "gemini_amd"), "-lgemini_hip", "-Wl,-rpath," + os.path.join(ROOT, "gemini_amd"), "-o", exe])
    n, d, K = 16, 5, 3
    p1, _, p2, _ = X.crs(n)
    g1, g2 = g1_points_to_affine(p1, flag=True), g2_points_to_affine(p2, flag=True)  # the 104- and 200-byte Rust records
    vecs = [(scalars(5300 + i, d), scalars(6300 + i, d)) for i in range(K)]
    ys = [X.ip(a, b) for a, b in vecs]
    y = np.stack([fr_from_int(v) for v in ys])
    y_bad = y.copy()
    y_bad[1] = fr_from_int((ys[1] + 1) % X.R)
    inp = str(tmp_path / "in.bin")
    with open(inp, "wb") as fh:
        _wvec(fh, g1)
        _wvec(fh, g2)
        for a, b in vecs:
            _wvec(fh, mont(a))
            _wvec(fh, mont(b))
        _wvec(fh, y)
        _wvec(fh, y_bad)
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True, timeout=120).stdout
    got = {ln.split()[0]: ln.split()[1:] for ln in out.strip().splitlines()}
    rounds = 3
    assert got["claims"] == ["3"]
    assert got["lengths"] == [str(rounds), str(3 * K + 2 * (rounds - 1)), "3", "3", "3"]
    assert got["shared"] == ["1"]
    assert got["verify"] == ["1"] and got["bad_y"] == ["0"] and got["swapped"] == ["0"]
    assert got["points"] == ["1", "messages", "1"]
    assert got["path"] == [str(4 * (rounds - 1) + 4), str(4 * rounds), str(rounds)]
    assert got["one"] == ["1", "1"] and got["one_verify"] == ["1", "1"]
    assert got["refused"] == ["-1", "-1", "-1", "1"]
