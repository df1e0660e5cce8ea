"""GPU: the point-validation part of the C++ host mirror (gm::check_g1 / check_g2, CommitterKey::{check_points, check_powers,
from_bytes}, G2Bases::check_points in include/gemini_hip.hpp) compiled with g++ against libgemini_hip.so.  Every value it prints must
equal what the Python mirror returns for the same call -- the Python mirror itself is checked in tests/test_gpu_points.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import points_ref as pr
from tests.points_cases import g1_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wvec(fh, arr):
    arr = np.ascontiguousarray(arr)
    fh.write(struct.pack("<Q", arr.shape[0]))
    fh.write(arr.tobytes())


def test_cpp_points_layer(tmp_path):
    import gemini_amd as gm
    from gemini_amd.fr import fr_from_int
    from gemini_amd.kzg import g1_generator_mont
    from gemini_amd.points import check_g1, check_g2, check_powers, g1_bases_from_bytes
    from oracle import oracle as orc
    from tests.test_gpu_points import TAU, g1_bad, g1_valid, g2_bad, g2_powers, g2_valid, plant

    exe = str(tmp_path / "test_points_api")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_points_api.cpp"),
                           "-L", os.path.join(ROOT, "gemini_amd"), "-lgemini_hip", "-Wl,-rpath," + os.path.join(ROOT, "gemini_amd"), "-o", exe])
    gm.capi.init()
    g1, _ = plant(g1_valid(), g1_bad(), 70, True, (63, 64))       # the 104-byte Rust records
    # the G2 list is also registered: curve and subgroup failures only (a non-canonical record has no defined resident form)
    g2, _ = plant(g2_valid(), [b for b in g2_bad() if b[1] != 2], 70, True, (63, 64))
    npow = 40
    key = gm.G1Bases.srs(g1_generator_mont(), orc.ints_to_limbs([TAU], 4)[0], npow)
    try:
        powers = np.zeros((npow, 13), dtype=np.uint64)
        powers[:, :12] = key.download()
        pts = [orc.affine_to_ints(r) for r in powers[:, :12]]
        good = b"".join(g1_bytes(p, True, 1) for p in pts)
        bad = b"".join(g1_bytes(p if i != 17 else pr.g1_random_curve_points(1)[0], True, 1) for i, p in enumerate(pts))
        pair = np.zeros((2, 25), dtype=np.uint64)
        pair[:, :24] = g2_powers()[:2]
        rho = fr_from_int(0x77AA55)
        inp = str(tmp_path / "in.bin")
        with open(inp, "wb") as fh:
            for arr in (g1, g2, powers, pair, rho.reshape(1, 4), np.frombuffer(good, dtype=np.uint8), np.frombuffer(bad, dtype=np.uint8)):
                _wvec(fh, arr)
        out = subprocess.run([exe, inp], check=True, capture_output=True, text=True, timeout=120).stdout
        got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out.strip().splitlines()}

        def same(tag, res):
            assert got[tag] == [int(res.ok), res.first_bad] + [int(s) for s in res.status], tag

        same("g1", check_g1(g1))
        same("g2", check_g2(g2))
        reg = gm.G2Bases.register(g2)
        try:
            same("g2_bases", reg.check())
            same("g2_window", reg.check(0, 2))
        finally:
            reg.free()
        assert not check_g1(g1).ok and not check_g2(g2).ok  # the lists do hold bad points
        same("ck", key.check())
        pw = g2_powers()
        assert got["powers"] == [1] == [int(check_powers(key, pw[0], pw[1], rho=0x77AA55))]
        assert got["powers_swapped"] == [0] == [int(check_powers(key, pw[1], pw[0], rho=0x77AA55))]
        b, res = g1_bases_from_bytes(good, npow, True, 1)
        same("from_bytes", res)
        assert got["key"] == [1, npow] and got["key_powers"] == [1] and b is not None
        b.free()
        b, res = g1_bases_from_bytes(bad, npow, True, 1)
        same("from_bad_bytes", res)
        assert got["bad_key"] == [0] and b is None and res.first_bad == 17 and res.status[17] == 4
        assert got["bad_handle"] == [0, 0, 17]
    finally:
        key.free()
