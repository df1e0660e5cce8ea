#!/usr/bin/env python3
"""G2 MSM against the G1 MSM of the same build (profiles/g2_msm.md): gm_g2_msm_d and gm_g1_msm_d on device-resident canonical
scalars, fixed-base tables off, the plain path, alternating the two in one process.

  device time gm_prof_read: HIP events on the library's stream around digits + sort / accumulation / merge / bucket reduction,
              `--calls` calls in a pass of its own (every event pair costs a bubble); their sum is the device time of a call,
              and the ratio of the sums the G2 / G1 figure that holds no host work
  call time   host clock around the call (it ends in a stream synchronise and the host Horner: what a caller waits for,
              ctypes overhead included on both sides), `--calls` calls
  identity    n pairs of 64 cycled points with known logs: the result must be ((sum b_i s_i) mod r) G

usage: g2_msm_bench.py [--logn 16 20 22] [--calls 20] [--check-logn 20] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemini_amd as gm  # noqa: E402
from gemini_amd import g2  # noqa: E402
from gemini_amd.fr import FrVec  # noqa: E402
from gemini_amd.g2msm import g2_jac_to_point, g2_points_to_affine  # noqa: E402
from gemini_amd.kzg import g1_generator_mont  # noqa: E402
from tests import g2_ref  # noqa: E402
from tests.util import dot_ints  # noqa: E402

STAGES = ("digits", "scan", "scatter", "accumulate", "merge", "reduce")


def scalars(rng, n):
    sc = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)  # < 2^254 < r
    return sc


def prof(lib, fn, calls):
    gm.capi.check(lib.gm_prof_enable(C.c_int(1)))
    for _ in range(calls):
        fn()
    ms = np.zeros(8)
    cnt = np.zeros(8, dtype=np.uint64)
    gm.capi.check(lib.gm_prof_read(gm.capi.ptr(ms), gm.capi.ptr(cnt), C.c_int(8)))
    mhz = C.c_double()
    gm.capi.check(lib.gm_prof_read_clock(C.byref(mhz)))
    gm.capi.check(lib.gm_prof_enable(C.c_int(0)))
    return {s: round(ms[i] / calls, 4) for i, s in enumerate(STAGES) if cnt[i]}, round(mhz.value, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, nargs="*", default=[16, 20, 22])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--check-logn", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gm.capi.init(0)
    lib = gm.capi.load()
    gm.capi.check(lib.gm_set_auto_tables(C.c_int(0), C.c_size_t(0)))
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    rng = np.random.default_rng(2025)
    nmax = 1 << max(a.logn + [a.check_logn])
    pts = g2_ref.chain(64 * 3)[::3]
    logs = np.array([[(g2_ref.chain_log(3 * i) >> (64 * k)) & (2**64 - 1) for k in range(4)] for i in range(64)], dtype=np.uint64)
    rec = g2_points_to_affine(pts)
    sel = np.arange(nmax) % 64
    b2 = gm.G2Bases.register(rec[sel])
    sc = scalars(rng, nmax)
    b1 = gm.G1Bases.fixed_base(g1_generator_mont(), sc[::-1].copy())  # tables are off: a plain key
    assert b1.table_info() == (0, 0)
    vec = FrVec.from_host(sc)  # raw copy: the call reads it as canonical integers (mont = 0)
    dptr = vec.device_ptr()

    n = 1 << a.check_logn
    t0 = time.perf_counter()
    got = g2_jac_to_point(b2.msm_device(dptr, n, mont=False))
    exp = g2.mul(g2_ref.G, dot_ints(logs[sel[:n]], sc[:n]) % g2.R_ORDER)
    emit({"check": "discrete-log identity", "logn": a.check_logn, "ok": bool(got == exp), "s": round(time.perf_counter() - t0, 2)})
    assert got == exp

    for lg in a.logn:
        n = 1 << lg
        f2 = lambda: b2.msm_device(dptr, n, mont=False)  # noqa: E731
        f1 = lambda: b1.msm_device(dptr, n, mont=False)  # noqa: E731
        for _ in range(3):
            f2(), f1()
        t = {"g2": [], "g1": []}
        for _ in range(a.calls):  # alternating: both see the same machine state
            for k, f in (("g2", f2), ("g1", f1)):
                t0 = time.perf_counter()
                f()
                t[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: float(np.median(v)) for k, v in t.items()}
        st2, _ = prof(lib, f2, a.calls)
        st1, mhz = prof(lib, f1, a.calls)
        dev2, dev1 = sum(st2.values()), sum(st1.values())
        emit({"logn": lg, "calls": a.calls, "g2_ms": round(med["g2"], 3), "g2_min_ms": round(min(t["g2"]), 3), "g2_max_ms": round(max(t["g2"]), 3),
              "g1_ms": round(med["g1"], 3), "g1_min_ms": round(min(t["g1"]), 3), "g1_max_ms": round(max(t["g1"]), 3),
              "ratio": round(med["g2"] / med["g1"], 2),
              "g2_device_ms": round(dev2, 3), "g1_device_ms": round(dev1, 3), "device_ratio": round(dev2 / dev1, 2), "g2_Mpairs_s": round(n / med["g2"] / 1e3, 2), "g1_Mpairs_s": round(n / med["g1"] / 1e3, 2),
              "g2_stage_ms": st2, "g1_stage_ms": st1, "g1_acc_shader_mhz": mhz})
    vec.free(), b1.free(), b2.free()


if __name__ == "__main__":
    main()
