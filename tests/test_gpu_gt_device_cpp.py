"""GPU: the element-wise GT part of the C++ host mirror (gm::gt_final_exp_many, gm::pairing_each, gm::check_gt, gm::HerringGt::check,
gm::InnerProductProof::check_messages in include/gemini_hip.hpp) compiled with g++ against libgemini_hip.so.  Every value it prints
must equal what the C ABI gives the Python mirror for the same call -- the Python mirror itself is checked against its statements
in tests/test_gpu_gt_device.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import gt_check_ref as ref
from tests import ipa_exponent_ref as X
from tests.test_gpu_pairing import g1_points_to_affine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wvec(fh, arr):
    arr = np.ascontiguousarray(arr)
    fh.write(struct.pack("<Q", arr.shape[0]))
    fh.write(arr.tobytes())


def test_cpp_gt_device_layer(tmp_path):
    import gemini_amd as gm
    from gemini_amd import pairing as gp
    from gemini_amd.fr import fr_from_int
    from gemini_amd.g2msm import g2_points_to_affine
    from gemini_amd.herring import GtModuleTimeProver

    exe = str(tmp_path / "test_gt_device_api")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_gt_device_api.cpp"),
                           "-L", os.path.join(ROOT, "gemini_amd"), "-lgemini_hip", "-Wl,-rpath," + os.path.join(ROOT, "gemini_amd"), "-o", exe])
    lst = {n: c for n, c, _ in ref.adversarial()}
    x = np.stack([gp.gt_from_ints(lst[n]) for n in ("cyclotomic_non_member", "member0", "random0", "zero", "one", "member1", "order_divides_h")])
    want_status = [ref.NOT_IN_SUBGROUP, ref.OK, ref.NOT_CYCLOTOMIC, ref.NOT_CYCLOTOMIC, ref.OK, ref.OK, ref.NOT_IN_SUBGROUP]
    good = np.stack([gp.gt_from_ints(lst[n]) for n in ("member0", "member1", "member2", "member3", "one", "member0")])
    p1, _, p2, _ = X.crs(16)
    g1, g2 = g1_points_to_affine(p1, flag=True), g2_points_to_affine(p2, flag=True)  # the 104- and 200-byte Rust records
    s = np.stack([fr_from_int(0x1234567 + 0x89ABCDEF * i) for i in range(8)])
    tw = np.stack([fr_from_int(0x1F3D5B79)])
    inp = str(tmp_path / "in.bin")
    with open(inp, "wb") as fh:
        for arr in (x, good, g1, g2, s, tw):
            _wvec(fh, arr)
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True, timeout=120).stdout
    got = {}
    for ln in (ln.split() for ln in out.strip().splitlines()):
        got.setdefault(ln[0], []).append(ln[1:])
    hexes = lambda rows: np.array([[int(v, 16) for v in r] for r in rows], dtype=np.uint64)  # noqa: E731

    gm.capi.init()
    assert (hexes(got["fe"]) == gm.gt_final_exp_many(x)).all() and got["fe_empty"] == [["0"]]
    assert (hexes(got["pair"]) == gm.pairing_each(g1, g2)).all()
    b1, b2 = gm.G1Bases.register(g1), gm.G2Bases.register(g2)
    assert (hexes(got["pair_h"]) == gm.pairing_each(b1, b2, 5, off1=1, step1=2, off2=0, step2=3)).all()
    b1.free()
    b2.free()
    res = gm.gt_check(x)
    assert list(res.status) == want_status
    assert got["check"] == [[str(int(res.ok)), str(res.first_bad)] + [str(v) for v in res.status]] == [["0", "0"] + [str(v) for v in want_status]]
    assert got["check_good"] == [["1", "6"] + ["0"] * 6] and got["check_empty"] == [["1", "0"]]
    assert got["not_cyclotomic"] == [["5"]]
    assert got["hgt"] == [["1", "6"]] and got["hgt_bad"] == [["0", "4"]]
    bad = good.copy()
    bad[4] = x[0]
    Pv = GtModuleTimeProver(bad, s[:6], tw[0])
    Pv.fold(s[7])
    res = Pv.check()
    assert not res.ok and res.first_bad == 2 and got["hgt_bad_folded"] == [["0", "2"]]
    Pv.free()
    assert got["ipa"] == [["1", "6", "3"]]
