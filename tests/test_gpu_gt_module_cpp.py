"""GPU: the GtModule part of the C++ host mirror (gm::gt_multi_pow, gm::HerringGt in include/gemini_hip.hpp) compiled with g++
against libgemini_hip.so.  Every value it prints must equal the bytes the C ABI gives the Python mirror for the same call -- the
Python mirror itself is checked against its statements in tests/test_gpu_gt_module.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import gt_module_ref as GR
from tests.test_pairing_cpu import gt_of_w

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wvec(fh, arr):
    arr = np.ascontiguousarray(arr)
    fh.write(struct.pack("<Q", arr.shape[0]))
    fh.write(arr.tobytes())


def test_cpp_gt_module_layer(tmp_path):
    import gemini_amd as gm
    from gemini_amd import pairing as gp
    from gemini_amd.fr import fr_from_int
    from gemini_amd.herring import GtModuleTimeProver

    exe = str(tmp_path / "test_gt_module_api")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_gt_module_api.cpp"),
                           "-L", os.path.join(ROOT, "gemini_amd"), "-lgemini_hip", "-Wl,-rpath," + os.path.join(ROOT, "gemini_amd"), "-o", exe])
    rng = np.random.default_rng(79)

    def rand(k):
        sc = rng.integers(0, 1 << 64, size=(k, 4), dtype=np.uint64)
        sc[:, 3] &= np.uint64((1 << 62) - 1)
        return sc

    ints = lambda a: [sum(int(w) << (64 * i) for i, w in enumerate(r)) for r in a]  # noqa: E731
    mont = lambda a: np.stack([fr_from_int(v) for v in ints(a)])  # noqa: E731
    e12 = gt_of_w(GR.E())
    pows = np.stack([gp.gt_pow(e12, v) for v in ints(rand(13))])  # host entry: no GPU yet in this process
    x, f = pows[:5], pows[5:]
    e = rng.integers(0, 1 << 64, size=(5, 4), dtype=np.uint64)  # 256-bit exponents, taken as they are
    g, tw, ch = mont(rand(8)), mont(rand(1)), mont(rand(4))
    inp = str(tmp_path / "in.bin")
    with open(inp, "wb") as fh:
        for arr in (x, e, f, g, tw, ch):
            _wvec(fh, arr)
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True, timeout=120).stdout
    lines = [ln.split() for ln in out.strip().splitlines()]
    hexes = lambda ln: np.array([int(v, 16) for v in ln[1:]], dtype=np.uint64)  # noqa: E731
    got, msgs = {}, []
    for ln in lines:
        if ln[0] in ("a", "b"):
            msgs.append(hexes(ln))
        else:
            got[ln[0]] = ln[1:] if ln[0] in ("rounds", "final") else hexes(ln)

    gm.capi.init()
    whole = gm.gt_multi_pow(x, e)
    assert (got["multi"] == whole).all() and (got["head"] == gm.gt_multi_pow(x[:2], e)).all()
    assert (got["empty"] == gm.gt_one()).all() and not (whole == gm.gt_one()).all()
    Pv = GtModuleTimeProver(f, g, tw[0])
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
