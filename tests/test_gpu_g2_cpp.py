"""GPU: the G2 part of the C++ host mirror (gm::G2Bases, gm::HerringG2, g2_add in include/gemini_hip.hpp) compiled with g++
against libgemini_hip.so.  Every value it prints must equal what the Python mirror returns for the same call -- the Python mirror
itself is checked against the reference side in tests/test_gpu_g2.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import g2_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wvec(fh, arr):
    arr = np.ascontiguousarray(arr)
    fh.write(struct.pack("<Q", arr.shape[0]))
    fh.write(arr.tobytes())


def test_cpp_g2_layer(tmp_path):
    import gemini_amd as gm
    from gemini_amd.fr import fr_from_int
    from gemini_amd.g2msm import g2_points_to_affine, g2_sum
    from gemini_amd.herring import G2ModuleTimeProver

    exe = str(tmp_path / "test_g2_api")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_g2_api.cpp"),
                           "-L", os.path.join(ROOT, "gemini_amd"), "-lgemini_hip", "-Wl,-rpath," + os.path.join(ROOT, "gemini_amd"), "-o", exe])
    n, nf = 200, 13
    pts = g2_ref.chain(n)
    pts = pts[:9] + [None] + pts[10:]
    rust = g2_points_to_affine(pts, flag=True)  # the 200-byte Rust records, entry 9 flagged as the identity
    rng = np.random.default_rng(77)

    def rand(k):
        sc = rng.integers(0, 1 << 64, size=(k, 4), dtype=np.uint64)
        sc[:, 3] &= np.uint64((1 << 62) - 1)
        return sc

    ints = lambda a: [sum(int(w) << (64 * i) for i, w in enumerate(r)) for r in a]  # noqa: E731
    mont = lambda a: np.stack([fr_from_int(v) for v in ints(a)])  # noqa: E731
    sc = rand(n)
    f, tw, ch = mont(rand(nf)), mont(rand(1)), mont(rand(6))
    inp = str(tmp_path / "in.bin")
    with open(inp, "wb") as fh:
        for arr in (rust, sc, mont(sc), f, tw, ch):
            _wvec(fh, arr)
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True, timeout=120).stdout
    lines = [ln.split() for ln in out.strip().splitlines()]
    hexes = lambda ln: np.array([int(x, 16) for x in ln[1:]], dtype=np.uint64)  # noqa: E731
    got = {}
    msgs = []
    for ln in lines:
        if ln[0] in ("a", "b"):
            msgs.append(hexes(ln))
        else:
            got[ln[0]] = ln[1:] if ln[0] in ("size", "rounds", "final") else hexes(ln)

    gm.capi.init()
    reg = gm.G2Bases.register(rust)
    try:
        assert got["size"] == [str(n)]
        assert (got["msm_bigint"] == reg.msm_bigint(sc)).all()
        rev = reg.msm_bigint(sc[:50], offset=120, reversed_=True)
        assert (got["msm_bigint_rev"] == rev).all()
        assert (got["msm_unchecked"] == reg.msm_bigint(sc)).all()  # the same scalars in Montgomery form
        assert (got["download"] == reg.download(3, 2).reshape(-1)).all()
        assert (got["zero"] == g2_sum(np.empty((0, 36), dtype=np.uint64))).all()
        assert (got["add"] == g2_sum(np.stack([reg.msm_bigint(sc[:50]), rev]))).all()
    finally:
        reg.free()
    P = G2ModuleTimeProver(f, rust[:16], tw[0])
    assert got["rounds"] == [str(P.rounds())]
    vm, k = None, 0
    while True:
        m = P.next_message(vm)
        if m is None:
            break
        assert (msgs[2 * k] == m[0]).all() and (msgs[2 * k + 1] == m[1]).all(), k
        vm = ch[k]
        k += 1
    assert len(msgs) == 2 * k and k == P.rounds()
    ff = P.final_foldings()
    assert got["final"] == ["1"] and (got["f0"] == ff[0]).all() and (got["g0"] == ff[1]).all()
    P.free()
