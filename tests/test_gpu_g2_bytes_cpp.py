"""GPU: the byte and check part of the C++ host mirror (gm::G2Bases::{from_bytes, to_bytes}, CommitterKey::to_bytes, Crs::{from_bases,
check}, VerifierKey::check, InnerProductProof::check_points in include/gemini_hip.hpp) compiled with g++ against libgemini_hip.so.
Every value it prints must equal what the Python definition (gemini_amd/g2.py, wire.py) or the Python mirror gives for the same call
-- the Python mirror itself is checked in tests/test_gpu_g2_bytes.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import points_ref as pr
from tests.g2_cases import g2_bytes
from tests.points_cases import g1_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wvec(fh, arr):
    arr = np.ascontiguousarray(arr)
    fh.write(struct.pack("<Q", arr.shape[0]))
    fh.write(arr.tobytes())


def test_cpp_g2_bytes_layer(tmp_path):
    from gemini_amd.points import g2_bases_from_bytes
    from tests.test_gpu_g2_bytes import g1_members, g2_members, outsiders, records_of
    from tests.test_gpu_ipa import mont, scalars

    exe = str(tmp_path / "test_g2_bytes_api")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_g2_bytes_api.cpp"),
                           "-L", os.path.join(ROOT, "gemini_amd"), "-lgemini_hip", "-Wl,-rpath," + os.path.join(ROOT, "gemini_amd"), "-o", exe])
    n, d, where = 8, 4, 5
    rec1, pts1 = g1_members()
    rec1, pts1 = rec1[8: 8 + n], pts1[8: 8 + n]  # no identity among them
    pts2 = list(g2_members()[8: 8 + n])
    g1 = np.zeros((n, 13), dtype=np.uint64)  # the 104- / 200-byte records of the mirror
    g1[:, :12] = rec1
    g2 = np.zeros((n, 25), dtype=np.uint64)
    g2[:, :24] = records_of(pts2)
    good = b"".join(g2_bytes(p, True, 1) for p in pts2)
    swapped = [p if i != where else outsiders()[1] for i, p in enumerate(pts2)]
    bad = b"".join(g2_bytes(p, True, 1) for p in swapped)
    inp = str(tmp_path / "in.bin")
    with open(inp, "wb") as fh:
        for arr in (g1, g2, np.frombuffer(good, dtype=np.uint8), np.frombuffer(bad, dtype=np.uint8), mont(scalars(71, d)), mont(scalars(72, d))):
            _wvec(fh, arr)
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True, timeout=120).stdout
    got = {ln.split()[0]: ln.split()[1:] for ln in out.strip().splitlines()}
    ints = lambda tag: [int(x) for x in got[tag]]  # noqa: E731

    def same(tag, res):
        assert ints(tag) == [int(res.ok), res.first_bad] + [int(s) for s in res.status], tag

    import gemini_amd as gm

    gm.capi.init()
    b, res = g2_bases_from_bytes(good, n, True, 1)
    same("from_bytes", res)
    b.free()
    b, res = g2_bases_from_bytes(bad, n, True, 1)
    same("from_bad_bytes", res)
    assert b is None and res.first_bad == where and res.status[where] == 4
    assert ints("key") == [1, n] and ints("bad_key") == [0] and ints("same_records") == [1]
    assert got["g2_compressed_zcash"] == [good.hex()]
    assert got["g2_uncompressed_ark"] == [b"".join(g2_bytes(p, False, 0) for p in pts2[1:3]).hex()]
    assert got["g1_compressed_ark"] == [b"".join(g1_bytes(p, True, 0) for p in pts1).hex()]
    assert got["g1_uncompressed_zcash"] == [b"".join(g1_bytes(p, False, 1) for p in pts1[1:3]).hex()]
    assert ints("crs_check") == [1, n, n] and ints("same_proof") == [1] and ints("ipa_check") == [1, 2 * (1 + 2)]
    assert ints("unchecked_key") == [1] and ints("unchecked_points")[:2] == [0, where] and ints("bad_crs_check") == [0, n, where]
    assert ints("vk_check") == [1, 2, 3]
    assert pr.g2_on_curve(outsiders()[1])
