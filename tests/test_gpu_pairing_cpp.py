"""GPU: the pairing part of the C++ host mirror (gm::multi_pairing, the gm::Gt helpers, gm::HerringP in include/gemini_hip.hpp)
compiled with g++ against libgemini_hip.so.  Every value it prints must equal the bytes the C ABI gives the Python mirror for the
same call -- the Python mirror itself is checked against the oracle in tests/test_gpu_pairing.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import pyref as P
from tests import g2_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wvec(fh, arr):
    arr = np.ascontiguousarray(arr)
    fh.write(struct.pack("<Q", arr.shape[0]))
    fh.write(arr.tobytes())


def test_cpp_pairing_layer(tmp_path):
    import gemini_amd as gm
    from gemini_amd import pairing as gp
    from gemini_amd.fr import fr_from_int
    from gemini_amd.g2msm import _fq_limbs, g2_points_to_affine
    from gemini_amd.herring import PModuleTimeProver

    exe = str(tmp_path / "test_pairing_api")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_pairing_api.cpp"),
                           "-L", os.path.join(ROOT, "gemini_amd"), "-lgemini_hip", "-Wl,-rpath," + os.path.join(ROOT, "gemini_amd"), "-o", exe])
    n = 8
    p1 = [P.g1_mul(P.G1_GEN, 0xA5A5A5A5A5A5A5A5A5A5 + 977 * i) for i in range(n)]
    g1 = np.zeros((n, 13), dtype=np.uint64)  # the 104-byte Rust records, entry 5 flagged as the identity over live coordinates
    for i, p in enumerate(p1):
        g1[i, :12] = _fq_limbs(p[0]) + _fq_limbs(p[1])
    g1[5, 12] = 1
    p2 = list(g2_ref.chain(n))
    g2 = g2_points_to_affine(p2[:2] + [None] + p2[3:], flag=True)  # the 200-byte Rust records, entry 2 the identity
    rng = np.random.default_rng(78)

    def rand(k):
        sc = rng.integers(0, 1 << 64, size=(k, 4), dtype=np.uint64)
        sc[:, 3] &= np.uint64((1 << 62) - 1)
        return sc

    ints = lambda a: [sum(int(w) << (64 * i) for i, w in enumerate(r)) for r in a]  # noqa: E731
    mont = lambda a: np.stack([fr_from_int(v) for v in ints(a)])  # noqa: E731
    tw, ch, k = mont(rand(1)), mont(rand(4)), rand(1)
    inp = str(tmp_path / "in.bin")
    with open(inp, "wb") as fh:
        for arr in (g1, g2, tw, ch, k):
            _wvec(fh, arr)
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True, timeout=120).stdout
    lines = [ln.split() for ln in out.strip().splitlines()]
    hexes = lambda ln: np.array([int(x, 16) for x in ln[1:]], dtype=np.uint64)  # noqa: E731
    got, msgs = {}, []
    for ln in lines:
        if ln[0] in ("a", "b"):
            msgs.append(hexes(ln))
        else:
            got[ln[0]] = ln[1:] if ln[0] in ("rounds", "final") else hexes(ln)

    gm.capi.init()
    whole, head = gm.multi_pairing(g1, g2), gm.multi_pairing(g1[:3], g2)
    assert (got["multi"] == whole).all() and (got["head"] == head).all()
    assert (got["one"] == gm.gt_one()).all() and (got["empty"] == gm.gt_one()).all()
    assert not (whole == gm.gt_one()).all()
    assert (got["mul"] == gm.gt_mul(whole, head)).all()
    assert (got["pow"] == gm.gt_pow(head, ints(k)[0])).all()
    B1, B2 = gm.G1Bases.register(g1), gm.G2Bases.register(g2)
    try:
        assert (got["strided"] == gp.multi_pairing_h(B1, B2, 3, 1, 2, 0, 1)).all()
    finally:
        B1.free()
        B2.free()
    Pv = PModuleTimeProver(g1, g2, tw[0])
    assert got["rounds"] == [str(Pv.rounds())] == ["3"]
    vm, r = None, 0
    while True:
        m = Pv.next_message(vm)
        if m is None:
            break
        assert (msgs[2 * r] == m[0]).all() and (msgs[2 * r + 1] == m[1]).all(), r
        vm = ch[r]
        r += 1
    assert len(msgs) == 2 * r and r == Pv.rounds()
    ff = Pv.final_foldings()
    assert got["final"] == ["1"] and (got["f0"] == ff[0]).all() and (got["g0"] == ff[1]).all()
    Pv.free()
