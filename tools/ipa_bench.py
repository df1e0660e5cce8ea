#!/usr/bin/env python3
"""herring's InnerProductProof on the device (profiles/herring_ipa.md): gm_ipa_new and gm_vrs_from_crs against the per-prover
composition of tests/stepwise/ipa.py -- what the library could do before the batched kernels -- in one process on one box.

  ipa_new     host clock around gm_ipa_new (it ends in a device synchronise and returns the finished proof), `--calls` calls after a
              warm-up call at every size; median, min and max.  With it what the call spent on the host (gm_ipa_host_times): the GT
              multi-exponentiations and the final exponentiations
  vrs         the same for gm_vrs_from_crs
  stepwise    tests/stepwise/ipa.py at d = 2^`--stepwise-logd`, `--stepwise-calls` calls after a warm-up at d = 2^6.  The fold of the
              CRS on Python integers is not part of the per-prover path the comparison is about: it is timed apart and taken out
  clock       gm_prof_read_clock after the run: the shader clock the library measured
  trace       `rocprofv3 --kernel-trace --stats` around a child of this program (--child) that makes ONE proof at d = 2^`--trace-logd`
              after a warm-up proof at d = 2^6: kernels per name and calls, i.e. the launches per round

The CRS is a chain of 2048 points with known logs, repeated: the times do not depend on the points, and a proof of every size is
checked by gm_ipa_verify before it is timed.

usage: ipa_bench.py [--logd 10 14] [--calls 5] [--stepwise-logd 10] [--stepwise-calls 2] [--out FILE] [--no-trace] [--trace-dir DIR]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemini_amd as gm  # noqa: E402
from gemini_amd.fr import fr_from_int  # noqa: E402
from gemini_amd.g2msm import g2_points_to_affine  # noqa: E402
from oracle import pyref as P  # noqa: E402
from tests import ipa_exponent_ref as X  # noqa: E402
from tests.stepwise import ipa as steps  # noqa: E402

CHAIN = 2048
LABEL = b"gemini-tests"


def g1_records(points) -> np.ndarray:
    return steps._g1_records(points)


def crs_records(n: int):
    p1, _, p2, _ = X.crs(min(n, CHAIN))
    r1, r2 = g1_records(p1), g2_points_to_affine(p2)
    reps = -(-n // len(r1))
    return np.tile(r1, (reps, 1))[:n].copy(), np.tile(r2, (reps, 1))[:n].copy()


def scalars(seed: int, n: int):
    rng = P.SplitMix64(seed)
    return [rng.fr() for _ in range(n)]


def mont(v) -> np.ndarray:
    return np.stack([fr_from_int(x) for x in v])


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "calls": len(ms)}


def bench_size(logd: int, calls: int) -> dict:
    d = 1 << logd
    r1, r2 = crs_records(2 * d)
    a, b = scalars(11 + logd, d), scalars(22 + logd, d)
    am, bm = mont(a), mont(b)
    crs = gm.Crs(r1, r2)
    out = {"logd": logd, "crs": 2 * d}
    t_vrs, vrs = [], None
    for k in range(calls + 1):
        if vrs is not None:
            vrs.free()
        t0 = time.perf_counter()
        vrs = gm.Vrs(crs)
        if k:
            t_vrs.append((time.perf_counter() - t0) * 1e3)
    out["vrs_from_crs"] = dict(spread(t_vrs), levels=vrs.levels)
    t_new, host = [], []
    for k in range(calls + 1):
        tr = gm.Transcript(LABEL)
        t0 = time.perf_counter()
        proof = gm.InnerProductProof.new(tr, crs, am, bm)
        dt = (time.perf_counter() - t0) * 1e3
        if k == 0:  # the proof that is timed is a proof that verifies
            y = fr_from_int(sum(x * z for x, z in zip(a, b)) % X.R)
            assert proof.verify_transcript(vrs, crs.commit_g1(am), crs.commit_g2(bm), y), "the proof does not verify"
        else:
            t_new.append(dt)
            host.append(proof.host_times())
        proof.free()
        tr.free()
    out["ipa_new"] = dict(spread(t_new), rounds=logd, host_gt_multi_pow_ms=round(statistics.median(h["gt_multi_pow_ms"] for h in host), 3),
                          host_final_exp_ms=round(statistics.median(h["final_exp_ms"] for h in host), 3))
    vrs.free()
    crs.free()
    return out


def bench_stepwise(logd: int, calls: int) -> dict:
    out = {"logd": logd}
    for ld, n_calls in ((6, 0), (logd, calls)):  # the small one warms every kernel and code path up
        d = 1 << ld
        p1, _, p2, _ = X.crs(2 * d)
        a, b = scalars(11 + ld, d), scalars(22 + ld, d)
        total, fold = [], []
        for _ in range(max(n_calls, 1)):
            tr, timers = gm.Transcript(LABEL), {}
            t0 = time.perf_counter()
            steps.new(tr, p1, p2, a, b, timers)
            total.append((time.perf_counter() - t0) * 1e3)
            fold.append(timers.get("fold_s", 0.0) * 1e3)
            tr.free()
        if n_calls:
            net = [t - f for t, f in zip(total, fold)]
            out["stepwise"] = dict(spread(net), python_crs_fold_ms_taken_out=round(statistics.median(fold), 1), with_fold_median_ms=round(statistics.median(total), 1))
    return out


def shader_mhz() -> float:
    """the clock the library reports for the G1 accumulation (gm_prof_read_clock), from one commitment under the profiler"""
    lib = gm.capi.load()
    r1, r2 = crs_records(CHAIN)
    crs = gm.Crs(r1, r2)
    gm.capi.check(lib.gm_prof_enable(C.c_int(1)))
    crs.commit_g1(mont(scalars(3, CHAIN - 1)))
    mhz = C.c_double()
    gm.capi.check(lib.gm_prof_read_clock(C.byref(mhz)))
    gm.capi.check(lib.gm_prof_enable(C.c_int(0)))
    crs.free()
    return round(mhz.value, 1)


def child(logd: int):
    """what the trace wraps: one warm-up proof at d = 2^6, then ONE proof at d = 2^logd"""
    gm.capi.init()
    for ld in (6, logd):
        d = 1 << ld
        r1, r2 = crs_records(2 * d)
        crs = gm.Crs(r1, r2)
        tr = gm.Transcript(LABEL)
        proof = gm.InnerProductProof.new(tr, crs, mont(scalars(11 + ld, d)), mont(scalars(22 + ld, d)))
        proof.free()
        tr.free()
        crs.free()


def trace(logd: int, trace_dir: str) -> dict:
    os.makedirs(trace_dir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", trace_dir, "-o", "ipa", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child",
           "--trace-logd", str(logd)]
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as fh:
            rows += list(csv.DictReader(fh))
    kernels = {r["Name"].split("(")[0]: {"calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3)} for r in rows}
    return {"logd": logd, "warmup_logd": 6, "kernels": kernels, "kernel_ms_total": round(sum(k["total_ms"] for k in kernels.values()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logd", type=int, nargs="*", default=[10, 14])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--stepwise-logd", type=int, default=10)
    ap.add_argument("--stepwise-calls", type=int, default=2)
    ap.add_argument("--trace-logd", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "tools", "_build", "ipa_trace"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        child(args.trace_logd)
        return
    lines = []
    if not args.no_trace:  # first: the child must be the only process of this program with the device open while it is traced
        lines.append({"trace": trace(args.trace_logd, args.trace_dir)})
    gm.capi.init()
    for logd in args.logd:
        lines.append(bench_size(logd, args.calls))
    if args.stepwise_calls:
        lines.append(bench_stepwise(args.stepwise_logd, args.stepwise_calls))
    lines.append({"shader_clock_mhz": shader_mhz()})
    text = "\n".join(json.dumps(ln) for ln in lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
