"""GPU: gm::HerringG1Space / gm::HerringG2Space of the C++ host mirror (include/gemini_hip.hpp) compiled with g++ against
libgemini_hip.so.  Every value the program prints must equal what the Python mirror returns for the same calls -- the Python mirror
itself is checked against the reference side in tests/test_gpu_herring_space.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import g2_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N1, N2, NS = 21, 14, 19
SWITCH = {"g1": 2, "g2": 0}  # messages before to_time, as tests/cpp/test_herring_space_api.cpp takes them


def _wvec(fh, arr):
    arr = np.ascontiguousarray(arr)
    fh.write(struct.pack("<Q", arr.shape[0]))
    fh.write(arr.tobytes())


def python_run(G, ch, switch_at):
    """the calls of run() in the C++ program -> its lines as (tag, limbs)"""
    lines, vm, T, k = [], None, None, 0
    while True:
        if k == switch_at:
            if vm is not None:
                G.fold(vm)
            vm = None
            T = G.to_time()
            lines.append(("time", [T.round(), T.rounds()]))
        m = G.next_message(vm)
        if T is not None:
            t = T.next_message(vm)
            assert (t is None) == (m is None)
            if t is not None:
                lines += [("ta", list(t[0])), ("tb", list(t[1]))]
        if m is None:
            break
        lines += [("a", list(m[0])), ("b", list(m[1]))]
        vm = ch[k]
        k += 1
    f0, g0 = G.final_foldings()
    lines += [("f0", list(f0)), ("g0", list(g0))]
    tf = T.final_foldings()
    lines += [("tf0", list(tf[0])), ("tg0", list(tf[1]))]
    lines.append(("path", list(G.path())))
    T.free()
    return lines


def test_cpp_herring_space(tmp_path, oracle):
    import gemini_amd as gm
    from gemini_amd.fr import FrVec
    from gemini_amd.g2msm import G2Bases, g2_points_to_affine
    from gemini_amd.herring import G1ModuleSpaceProver, G2ModuleSpaceProver

    exe = str(tmp_path / "test_herring_space_api")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_herring_space_api.cpp"),
                           "-L", os.path.join(ROOT, "gemini_amd"), "-lgemini_hip", "-Wl,-rpath," + os.path.join(ROOT, "gemini_amd"), "-o", exe])
    r1 = oracle.g1_fixed_base_mul(oracle.g1_generator(), oracle.random_fr(3200, N1))
    rust1 = np.zeros((N1, 13), dtype=np.uint64)  # the 104-byte Rust records
    rust1[:, :12] = r1
    rust2 = g2_points_to_affine(list(g2_ref.chain(N2)), flag=True)  # the 200-byte Rust records
    stream, tw, ch = (oracle.fr_to_mont(oracle.random_fr(seed, n)) for seed, n in ((3201, NS), (3202, 1), (3203, 8)))
    inp = str(tmp_path / "in.bin")
    with open(inp, "wb") as fh:
        for arr in (rust1, rust2, stream, tw, ch):
            _wvec(fh, arr)
    out = subprocess.run([exe, inp], check=True, capture_output=True, text=True, timeout=120).stdout
    got = {"g1": [], "g2": []}
    cur, key1 = None, None
    for ln in (x.split() for x in out.strip().splitlines()):
        if ln[0] in got and ln[1] == "rounds":
            cur = ln[0]
            got[cur].append(("rounds", [int(ln[2])]))
        elif ln[0] in got:
            got[ln[0]].append((ln[1], [int(x) for x in ln[2:]]))
        elif ln[0] == "key1":
            key1 = [int(x, 16) for x in ln[1:]]
        else:
            got[cur].append((ln[0], [int(x, 16) for x in ln[1:]]))

    gm.capi.init()
    vec = FrVec.from_host(stream)
    k1, k2 = gm.G1Bases.register(r1), G2Bases.register(rust2[:, :24].copy())
    provers = {"g1": G1ModuleSpaceProver(k1, vec, tw[0], offset=2, n=N1 - 2), "g2": G2ModuleSpaceProver(vec, k2, tw[0], offset=1, n=N2 - 1)}
    for tag, G in provers.items():
        want = [("rounds", [G.rounds()])] + python_run(G, ch, SWITCH[tag])
        assert [(t, [int(x) for x in v]) for t, v in want] == got[tag], tag
        G.free()
    assert key1 == [int(x) for x in r1.reshape(-1)]  # the borrowed key after both runs
    for x in (vec, k1, k2):
        x.free()
