"""GPU: gm::InnerProductProof::verify_many and gm::gt_multi_pow_many of the C++ host mirror (include/gemini_hip.hpp) compiled with g++
against libgemini_hip.so.  The program goes through gemini_hip.hpp only; its verdicts must be the single entry's and the expected
pattern, its GT products what the Python mirror returns for the same call (tests/test_gpu_gt_multi_pow_many.py checks those)."""
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


def test_cpp_ipa_verify_many_layer(tmp_path):
    import gemini_amd as gm
    from gemini_amd.fr import fr_from_int
    from gemini_amd.g2msm import g2_points_to_affine

    exe = str(tmp_path / "test_ipa_verify_many_api")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_ipa_verify_many_api.cpp"),
                           "-L", os.path.join(ROOT, "gemini_amd"), "-lgemini_hip", "-Wl,-rpath," + os.path.join(ROOT, "gemini_amd"), "-o", exe])
    n = 16
    p1, _, p2, _ = X.crs(n)
    g1, g2 = g1_points_to_affine(p1, flag=True), g2_points_to_affine(p2, flag=True)  # the 104- and 200-byte Rust records
    a0, b0, a1, b1 = scalars(5000, 5), scalars(6000, 5), scalars(5001, 2), scalars(6001, 2)  # 3 rounds and 1 round
    y = np.stack([fr_from_int(X.ip(a0, b0)), fr_from_int(X.ip(a1, b1)), fr_from_int((X.ip(a0, b0) + 1) % X.R)])
    rng = np.random.default_rng(0xC99)
    nx = 2 * 3 + 2 * 1  # the messages of both proofs
    exps = rng.integers(0, 1 << 63, size=(nx, 4), dtype=np.uint64)
    exps[2] = 0
    exps[5] = 0xFFFFFFFFFFFFFFFF
    offs = np.array([0, 3, 3, 4, nx], dtype=np.uint64)
    inp = str(tmp_path / "in.bin")
    with open(inp, "wb") as fh:
        for arr in (g1, g2, mont(a0), mont(b0), mont(a1), mont(b1), y, exps, offs):
            _wvec(fh, arr)
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True, timeout=120).stdout
    got = {}
    for ln in (line.split() for line in out.strip().splitlines()):
        val = ln[1:] if ln[0] in ("rounds", "single", "many", "none", "refused") else np.array([int(x, 16) for x in ln[1:]], dtype=np.uint64)
        got.setdefault(ln[0], []).append(val)
    assert got["rounds"] == [["3", "1"]]
    assert got["single"] == got["many"] == [["1", "0", "1", "0"]]
    assert got["none"] == [["0"]] and got["refused"] == [["-1"]]
    gm.capi.init()
    x = np.stack(got["x"])
    assert x.shape == (nx, 72)
    assert (np.stack(got["prod"]) == gm.gt_multi_pow_many(x, exps, offs)).all()
