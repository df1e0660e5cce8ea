#!/usr/bin/env python3
"""Multi-pairing on the device (profiles/pairing.md): the identity check at 2^16 pairs, gm_pairing_multi_h at 2^10 / 2^14 / 2^16 pairs,
the host final exponentiation, and k_miller against k_g2_acc -- the kernel on the same Fq2 layer -- from one rocprofv3 pass.

  identity    2^16 pairs of 64 G1 points against 63 G2 points with known logs, cycled: the result must be E^(sum a_i b_i mod r),
              E = e(G1, G2) from oracle/pairing.py
  call time   host clock around the call (Miller kernel, reductions, copy, host product, conjugation and final exponentiation: what
              a caller waits for), `--calls` calls
  stages      HIP events on the library's stream (gm_prof_enable(1)): "accumulate" = k_miller, "reduce" = the k_gt_reduce launches
  final exp   gm_gt_final_exp on the host, `--calls` calls
  kernels     `rocprofv3 --kernel-trace --stats` around a child of this program (--child) that runs pairing calls at 2^16 pairs and
              G2 MSMs at 2^20 pairs; Fq products per second of k_miller and k_g2_acc from the operation counts of the loops as written

usage: pairing_bench.py [--logn 10 14 16] [--calls 20] [--check-logn 16] [--out FILE] [--no-trace] [--trace-dir DIR]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemini_amd as gm  # noqa: E402
from gemini_amd import pairing as gp  # noqa: E402
from gemini_amd.g2msm import _fq_limbs, g2_points_to_affine  # noqa: E402
from oracle import pairing as OP  # noqa: E402
from oracle import pyref as P  # noqa: E402
from tests import g2_ref  # noqa: E402
from tests.test_pairing_cpu import w_of_gt  # noqa: E402

STAGES = ("digits", "scan", "scatter", "accumulate", "merge", "reduce")
# Fq products per pair in k_miller, from the loop as written (pairing.hip): 63 steps of f^2 (36) + f * line (39) + doubling with its
# line (3 M + 6 S over Fq2 = 21, + 4 to scale the line), 5 steps of f * line (39) + addition (11 M + 2 S = 37, + 4); the block product
# is 63 Fq12 products (54 each) per 64 pairs
MILLER_FQ_PER_PAIR = 63 * (36 + 39 + 25) + 5 * (39 + 41) + 63 * 54 / 64
# k_g2_acc: one mixed addition (8 M + 2 S over Fq2 = 28 Fq products) per entry, 16 entries per pair at c = 16 (2^20 pairs)
G2_ACC_FQ_PER_PAIR = 16 * 28
TRACE_PAIRS_LOG, TRACE_MSM_LOG, TRACE_CALLS = 16, 20, 5


def points():
    """64 G1 and 63 G2 points with their logs, as records"""
    a = [(0x1234567 + 0x9E3779B97F4A7C15F39CC0605CEDC834 * i) % OP.R for i in range(64)]
    p1 = [P.g1_mul(P.G1_GEN, a[0])]
    step = P.g1_mul(P.G1_GEN, (a[1] - a[0]) % OP.R)
    for _ in range(63):
        p1.append(P.g1_add(p1[-1], step))
    r1 = np.array([_fq_limbs(p[0]) + _fq_limbs(p[1]) for p in p1], dtype=np.uint64)
    b = [g2_ref.chain_log(i) for i in range(63)]
    return a, r1, b, g2_points_to_affine(g2_ref.chain(63))


def register(r1, r2, n):
    return gm.G1Bases.register(r1[np.arange(n) % 64]), gm.G2Bases.register(r2[np.arange(n) % 63])


def child():
    """the traced workload: pairing calls at 2^16 pairs, G2 MSMs at 2^20 pairs"""
    from gemini_amd.fr import FrVec

    gm.capi.init(0)
    gm.capi.check(gm.capi.load().gm_set_auto_tables(C.c_int(0), C.c_size_t(0)))
    _, r1, _, r2 = points()
    n = 1 << TRACE_PAIRS_LOG
    b1, b2 = register(r1, r2, n)
    for _ in range(TRACE_CALLS):
        gp.multi_pairing_h(b1, b2, n)
    b1.free(), b2.free()
    m = 1 << TRACE_MSM_LOG
    sc = np.random.default_rng(2026).integers(0, 1 << 64, size=(m, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)
    big = gm.G2Bases.register(r2[np.arange(m) % 63])
    vec = FrVec.from_host(sc)
    for _ in range(TRACE_CALLS):
        big.msm_device(vec.device_ptr(), m, mont=False)
    vec.free(), big.free()


def trace(trace_dir):
    """-> {kernel short name: (calls, average ns, min ns, max ns)} of k_miller, k_gt_reduce and k_g2_acc"""
    os.makedirs(trace_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "-o", "pairing", "--", sys.executable, os.path.abspath(__file__), "--child"]
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    files = glob.glob(os.path.join(trace_dir, "**", "pairing_kernel_stats.csv"), recursive=True)
    assert files, f"no kernel stats under {trace_dir}"
    out = {}
    with open(files[0]) as fh:
        for row in csv.DictReader(fh):
            for k in ("k_miller", "k_gt_reduce", "k_g2_acc"):
                if f"gm::{k}(" in row["Name"]:
                    out[k] = (int(row["Calls"]), float(row["AverageNs"]), int(row["MinNs"]), int(row["MaxNs"]))
    return out, files[0]


def prof(lib, fn, calls):
    gm.capi.check(lib.gm_prof_enable(C.c_int(1)))
    for _ in range(calls):
        fn()
    ms = np.zeros(8)
    cnt = np.zeros(8, dtype=np.uint64)
    gm.capi.check(lib.gm_prof_read(gm.capi.ptr(ms), gm.capi.ptr(cnt), C.c_int(8)))
    gm.capi.check(lib.gm_prof_enable(C.c_int(0)))
    return {s: round(ms[i] / calls, 4) for i, s in enumerate(STAGES) if cnt[i]}


def shader_mhz(lib):
    """the clock the library reports for the G1 accumulation (gm_prof_read_clock), from one small G1 MSM under the profiler"""
    from tests.util import rand_bases
    from oracle import oracle as orc

    gm.capi.check(lib.gm_prof_enable(C.c_int(1)))
    gm.VariableBaseMSM.msm_bigint(rand_bases(orc, 1, 1 << 14), orc.random_fr(2, 1 << 14))
    mhz = C.c_double()
    gm.capi.check(lib.gm_prof_read_clock(C.byref(mhz)))
    gm.capi.check(lib.gm_prof_enable(C.c_int(0)))
    return round(mhz.value, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, nargs="*", default=[10, 14, 16])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--check-logn", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-dir", default="pairing_rocprof")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    gm.capi.init(0)
    lib = gm.capi.load()
    gm.capi.check(lib.gm_set_auto_tables(C.c_int(0), C.c_size_t(0)))  # the G1 side is read as plain records
    la, r1, lb, r2 = points()
    nmax = 1 << max(a.logn + [a.check_logn])
    b1, b2 = register(r1, r2, nmax)

    n = 1 << a.check_logn
    t0 = time.perf_counter()
    got = w_of_gt(gp.multi_pairing_h(b1, b2, n))
    E = OP.f12_inv(OP.pairing(g2_ref.G, P.G1_GEN))
    exp = OP.f12_pow(E, sum(la[i % 64] * lb[i % 63] for i in range(n)) % OP.R)
    emit({"check": "pairing identity", "logn": a.check_logn, "ok": bool(got == exp), "s": round(time.perf_counter() - t0, 2)})
    assert got == exp

    mhz = shader_mhz(lib)
    x = gp.multi_pairing_h(b1, b2, 3)
    fe = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        gp.gt_final_exp(x)
        fe.append((time.perf_counter() - t0) * 1e3)
    emit({"final_exp_host_ms": round(float(np.median(fe)), 3), "min_ms": round(min(fe), 3), "max_ms": round(max(fe), 3), "calls": a.calls})

    for lg in a.logn:
        n = 1 << lg
        f = lambda: gp.multi_pairing_h(b1, b2, n)  # noqa: E731
        for _ in range(3):
            f()
        t = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            f()
            t.append((time.perf_counter() - t0) * 1e3)
        st = prof(lib, f, a.calls)
        med = float(np.median(t))
        emit({"logn": lg, "calls": a.calls, "call_ms": round(med, 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "stage_ms": st,
              "device_ms": round(sum(st.values()), 3), "kpairs_s": round(n / med, 1), "g1_acc_shader_mhz": mhz})
    b1.free(), b2.free()

    if not a.no_trace:
        k, path = trace(a.trace_dir)
        mil, acc = k["k_miller"], k["k_g2_acc"]
        mil_rate = (1 << TRACE_PAIRS_LOG) * MILLER_FQ_PER_PAIR / (mil[1] * 1e-9)
        acc_rate = (1 << TRACE_MSM_LOG) * G2_ACC_FQ_PER_PAIR / (acc[1] * 1e-9)
        emit({"trace": os.path.relpath(path), "k_miller": {"pairs_log": TRACE_PAIRS_LOG, "calls": mil[0], "avg_us": round(mil[1] / 1e3, 1), "min_us": round(mil[2] / 1e3, 1),
                                                           "max_us": round(mil[3] / 1e3, 1), "fq_products_per_pair": round(MILLER_FQ_PER_PAIR, 1),
                                                           "fq_products_per_s": round(mil_rate / 1e9, 2)},
              "k_gt_reduce": {"calls": k["k_gt_reduce"][0], "avg_us": round(k["k_gt_reduce"][1] / 1e3, 1)} if "k_gt_reduce" in k else None,
              "k_g2_acc": {"pairs_log": TRACE_MSM_LOG, "calls": acc[0], "avg_us": round(acc[1] / 1e3, 1), "min_us": round(acc[2] / 1e3, 1), "max_us": round(acc[3] / 1e3, 1),
                           "fq_products_per_pair": G2_ACC_FQ_PER_PAIR, "fq_products_per_s": round(acc_rate / 1e9, 2)},
              "unit": "1e9 Fq products per second", "miller_over_g2_acc": round(mil_rate / acc_rate, 3)})


if __name__ == "__main__":
    main()
