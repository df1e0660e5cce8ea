"""GPU: the inner-product argument of the C++ host mirror (gm::Crs, gm::Vrs, gm::InnerProductProof in include/gemini_hip.hpp) compiled
with g++ against libgemini_hip.so: it proves and verifies through gemini_hip.hpp only, and every value it prints must equal what the
Python mirror returns for the same call -- which tests/test_gpu_ipa.py checks against the exponent restatement."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import ipa_exponent_ref as X
from tests.test_gpu_ipa import LABEL, mont, scalars
from tests.test_gpu_pairing import g1_points_to_affine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wvec(fh, arr):
    arr = np.ascontiguousarray(arr)
    fh.write(struct.pack("<Q", arr.shape[0]))
    fh.write(arr.tobytes())


def test_cpp_ipa_layer(tmp_path):
    import gemini_amd as gm
    from gemini_amd.fr import fr_from_int
    from gemini_amd.g2msm import g2_points_to_affine

    exe = str(tmp_path / "test_ipa_api")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_ipa_api.cpp"),
                           "-L", os.path.join(ROOT, "gemini_amd"), "-lgemini_hip", "-Wl,-rpath," + os.path.join(ROOT, "gemini_amd"), "-o", exe])
    d, n = 5, 16
    p1, _, p2, _ = X.crs(n)
    g1, g2 = g1_points_to_affine(p1, flag=True), g2_points_to_affine(p2, flag=True)  # the 104- and 200-byte Rust records
    a, b = scalars(5000, d), scalars(6000, d)
    am, bm = mont(a), mont(b)
    y = np.stack([fr_from_int(X.ip(a, b)), fr_from_int((X.ip(a, b) + 1) % X.R)])
    inp = str(tmp_path / "in.bin")
    with open(inp, "wb") as fh:
        for arr in (g1, g2, am, bm, y):
            _wvec(fh, arr)
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True, timeout=120).stdout
    got = {}
    for ln in (line.split() for line in out.strip().splitlines()):
        val = ln[1] if ln[0] in ("levels", "rounds", "verify", "verify_wrong_y", "refused") else np.array([int(x, 16) for x in ln[1:]], dtype=np.uint64)
        got.setdefault(ln[0], []).append(val)

    gm.capi.init()
    crs = gm.Crs(g1, g2)
    vrs = gm.Vrs(crs)
    tr = gm.Transcript(LABEL)
    proof = gm.InnerProductProof.new(tr, crs, am, bm)
    f = proof.fields()
    assert got["levels"] == [str(vrs.levels)] == ["3"] and got["rounds"] == [str(f.rounds)] == ["3"]
    for l in range(vrs.levels):
        vk1, vk2 = vrs.level(l)
        for key, exp in (("vk1e", vk1[0]), ("vk1o", vk1[1]), ("vk2e", vk2[0]), ("vk2o", vk2[1])):
            assert (got[key][l] == exp).all(), (key, l)
    assert (np.stack(got["a"]) == f.messages[:, 0]).all() and (np.stack(got["b"]) == f.messages[:, 1]).all()
    assert (np.stack(got["challenge"]) == f.challenges).all() and (np.stack(got["batch"]) == f.batch_challenges).all()
    assert (np.stack(got["lhs"]) == f.final_lhs).all() and (np.stack(got["rhs"]) == f.final_rhs).all()
    assert (got["ff0"][0] == f.foldings_ff[0]).all() and (got["ff1"][0] == f.foldings_ff[1]).all()
    assert (got["fg1f"][0] == f.foldings_fg1[0]).all() and (got["fg1g"][0] == f.foldings_fg1[1]).all()
    assert (got["fg2f"][0] == f.foldings_fg2[0]).all() and (got["fg2g"][0] == f.foldings_fg2[1]).all()
    assert (got["next"][0] == tr.get_challenge(b"next")).all()
    assert (got["comm_a"][0] == crs.commit_g1(am)).all() and (got["comm_b"][0] == crs.commit_g2(bm)).all()
    assert got["verify"] == ["1"] and got["verify_wrong_y"] == ["0"] and got["refused"] == ["-1"]
    for o in (proof, tr, vrs, crs):
        o.free()
