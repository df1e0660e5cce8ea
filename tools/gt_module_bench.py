#!/usr/bin/env python3
"""GtModule on the device (profiles/gt_module.md): gm_gt_multi_pow against the same product composed from gm_gt_pow / gm_gt_mul on
the host -- the only way before the device kernels -- and the herring GtModule prover, in one process on one box.

Method (that of profiles/herring_ipa.md): host clock around calls that end in a device synchronise, one warm-up call, then `--calls`
timed calls; median with min - max.  Both paths run in this process.  The shader clock is gm_prof_read_clock's, from a G1 MSM
under the profiler.

  multi_pow   gm_gt_multi_pow at n = 2^6, 2^10, 2^14 (elements and exponents start on the host: the call uploads them) against the
              host loop; at more than `--host-max` terms the host loop is timed on its first `--host-max` terms and scaled, and
              the line says so
  crossover   both at n = 1, 2, 4, ..., 128: the first n at which the device call is faster
  prover      one gm_hgt_round (no challenge) and one gm_hgt_fold at nf = ng = 2^10 and 2^14, a fresh prover per call
  launch      HIP events of the library (gm_prof_enable(1)): ms per k_gt_multi_pow launch and per k_miller launch at 2^10 terms /
              pairs, and the prediction (Fq products per lane) / 6700 x k_miller

The elements are powers of e(G1, G2) from a pool of 256, tiled: no time here depends on the values.

usage: gt_module_bench.py [--calls 5] [--out profiles/gt_module.md] [--json FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemini_amd as gm  # noqa: E402
from gemini_amd import pairing as gp  # noqa: E402
from gemini_amd.fr import fr_from_int  # noqa: E402
from gemini_amd.g2msm import g2_points_to_affine  # noqa: E402
from gemini_amd.herring import GtModuleTimeProver  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import gt_module_ref as GR  # noqa: E402
from tests import ipa_exponent_ref as X  # noqa: E402
from tests.stepwise import ipa as steps  # noqa: E402
from tests.test_pairing_cpu import gt_of_w  # noqa: E402

POOL = 256
FQ_PER_LANE_MILLER = 6700
R = GR.R


def fq_per_lane_pow(window: int) -> int:
    """as gt_pow_lane is written: 256 squarings, one product per window, the table built by products"""
    return 256 * 36 + (256 // window) * 54 + ((1 << window) - 2) * 54


def source_window() -> int:
    import re

    src = open(os.path.join(ROOT, "gemini_amd", "csrc", "pairing.hip")).read()
    return int(re.search(r"constexpr\s+int\s+GT_WINDOW\s*=\s*(\d+);", src).group(1))


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "calls": len(ms)}


def timed(fn, calls):
    fn()  # warm-up
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def host_multi_pow(xs, es):
    lib, acc, tmp = gm.capi.load(), gp.gt_one(), np.empty(72, dtype=np.uint64)
    for x, e in zip(xs, es):  # straight on the C entries: no Python conversion inside the timed loop
        lib.gm_gt_pow(gm.capi.ptr(x), gm.capi.ptr(e), gm.capi.ptr(tmp))
        lib.gm_gt_mul(gm.capi.ptr(acc), gm.capi.ptr(tmp), gm.capi.ptr(acc))
    return acc


def inputs(n, pool, seed):
    rng = np.random.default_rng(seed)
    xs = np.ascontiguousarray(np.tile(pool, (-(-n // POOL), 1))[:n])
    es = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    es[:, 3] &= np.uint64((1 << 62) - 1)  # below r: what a prover's exponents are
    return xs, es


def bench_multi_pow(n, pool, calls, host_max):
    xs, es = inputs(n, pool, 100 + n)
    dev = timed(lambda: gm.gt_multi_pow(xs, es), calls)
    m = min(n, host_max)
    host = timed(lambda: host_multi_pow(xs[:m], es[:m]), 1 if m >= 1024 else calls)
    if m == n:
        assert (gm.gt_multi_pow(xs, es) == host_multi_pow(xs, es)).all(), "device and host products differ"
    line = {"n": n, "device": dev, "host_terms_timed": m, "host": host, "host_scaled_ms": round(host["median_ms"] * n / m, 1)}
    line["speedup"] = round(line["host_scaled_ms"] / dev["median_ms"], 2)
    return line


def bench_prover(n, pool, calls):
    xs, es = inputs(n, pool, 200 + n)
    g = np.stack([fr_from_int(sum(int(w) << (64 * i) for i, w in enumerate(row)) % R) for row in es[:POOL]])
    g = np.ascontiguousarray(np.tile(g, (-(-n // POOL), 1))[:n])
    tw, ch = fr_from_int(0x1234567), fr_from_int(0x89ABCDEF0123)
    rounds, folds = [], []
    for k in range(calls + 1):
        Pv = GtModuleTimeProver(xs, g, tw)
        t0 = time.perf_counter()
        Pv.next_message()
        t1 = time.perf_counter()
        Pv.fold(ch)
        t2 = time.perf_counter()
        Pv.free()
        if k:
            rounds.append((t1 - t0) * 1e3)
            folds.append((t2 - t1) * 1e3)
    return {"n": n, "round": spread(rounds), "fold": spread(folds)}


def prof(fn, calls):
    """-> (ms per accumulate launch, ms per reduce group) of `calls` calls of fn under gm_prof_enable(1)"""
    lib = gm.capi.load()
    fn()
    gm.capi.check(lib.gm_prof_enable(C.c_int(1)))
    for _ in range(calls):
        fn()
    ms, cnt = (C.c_double * 8)(), (C.c_uint64 * 8)()
    gm.capi.check(lib.gm_prof_read(ms, cnt, C.c_int(8)))
    gm.capi.check(lib.gm_prof_enable(C.c_int(0)))
    return round(ms[3] / max(cnt[3], 1), 3), round(ms[5] / max(cnt[5], 1), 3), int(cnt[3])


def shader_mhz() -> float:
    lib = gm.capi.load()
    n = 1 << 12
    bases = orc.g1_fixed_base_mul(orc.g1_generator(), orc.random_fr(1, n))
    sc = orc.random_fr(2, n)
    gm.capi.check(lib.gm_prof_enable(C.c_int(1)))
    gm.VariableBaseMSM.msm_bigint(bases, sc)
    mhz = C.c_double()
    gm.capi.check(lib.gm_prof_read_clock(C.byref(mhz)))
    gm.capi.check(lib.gm_prof_enable(C.c_int(0)))
    return round(mhz.value, 1)


def bench_launch(pool, calls, window):
    n = 1 << 10
    xs, es = inputs(n, pool, 300)
    pow_ms, pow_red, launches = prof(lambda: gm.gt_multi_pow(xs, es), calls)
    p1, _, p2, _ = X.crs(64)
    r1 = np.tile(steps._g1_records(p1), (n // 64, 1)).copy()
    r2 = np.tile(g2_points_to_affine(p2), (n // 64, 1)).copy()
    mil_ms, mil_red, _ = prof(lambda: gm.multi_pairing(r1, r2), calls)
    fq = fq_per_lane_pow(window)
    return {"n": n, "k_gt_multi_pow_ms": pow_ms, "k_gt_reduce_ms": pow_red, "launches": launches, "k_miller_ms": mil_ms, "k_miller_reduce_ms": mil_red,
            "fq_per_lane_pow": fq, "fq_per_lane_miller": FQ_PER_LANE_MILLER, "predicted_ms": round(fq / FQ_PER_LANE_MILLER * mil_ms, 3),
            "measured_over_predicted": round(pow_ms / (fq / FQ_PER_LANE_MILLER * mil_ms), 3)}


def fmt(s):
    return f"{s['median_ms']:.2f} ({s['min_ms']:.2f} – {s['max_ms']:.2f})"


def markdown(res) -> str:
    L, w = res["launch"], res["window"]
    cross = res["crossover"]
    first = next((c["n"] for c in cross if c["device"]["median_ms"] < c["host"]["median_ms"]), None)
    out = ["# GtModule on the MI355X: device GT multi-exponentiation against the host loop, the GtModule prover",
           "",
           "Everything below is one build, one box, one process: `python tools/gt_module_bench.py` wrote this file.  Host clock around calls that",
           f"end in a device synchronise, one warm-up call, then {res['calls']} timed calls: median (min – max).  The shader clock `gm_prof_read_clock`",
           f"reports for a G1 accumulation of this process: **{res['shader_clock_mhz']} MHz**.  The kernel walks a {w}-bit window: "
           f"{L['fq_per_lane_pow']} Fq products per lane.",
           "",
           "## `gm_gt_multi_pow` against the composition of `gm_gt_pow` / `gm_gt_mul`",
           "",
           "The device call takes host elements and exponents: it uploads n × 608 bytes, converts, launches `k_gt_multi_pow` and the",
           "`k_gt_reduce` levels, and multiplies the last ≤ 4 partials on the host.  The host loop is the parent commit's only way: one 256-step",
           "square-and-multiply per term on one CPU thread.",
           "",
           "| n | device call ms | host loop ms | host terms timed | host / device |",
           "|---|---|---|---|---|"]
    for m in res["multi_pow"]:
        sub = "all" if m["host_terms_timed"] == m["n"] else f"first {m['host_terms_timed']} of {m['n']}, one call, scaled by n / {m['host_terms_timed']}"
        out.append(f"| {m['n']} | {fmt(m['device'])} | {m['host_scaled_ms']:.1f} | {sub} | **{m['speedup']:.1f}** |")
    out += ["",
            "## Where the device call starts to win",
            "",
            "| n | device call ms | host loop ms |",
            "|---|---|---|"]
    for c in cross:
        out.append(f"| {c['n']} | {fmt(c['device'])} | {fmt(c['host'])} |")
    out += ["",
            (f"The device call is faster from **n = {first}** on (powers of two measured)." if first is not None else
             "The device call is not faster at any n measured here."),
            "A launch is one 256-bit power deep whatever n is; the host loop is linear in n.  `gm_ipa_new` and `gm_ipa_verify` multiply 3 to 29 terms per call",
            "(profiles/herring_ipa.md) and stay on the host in this change: the table says on which side of the crossover those counts lie.",
            "",
            "## The prover: one `gm_hgt_round` and one `gm_hgt_fold`",
            "",
            "A fresh prover per call (its creation, which uploads f, is not timed).  The round is the first one, without a challenge: a over n/2 terms",
            "and b over n terms, two launches with their reductions.  The fold is `k_gt_split_fold` over n/2 lanes plus the Fr fold.",
            "",
            "| nf = ng | round ms | fold ms |",
            "|---|---|---|"]
    for p in res["prover"]:
        out.append(f"| {p['n']} | {fmt(p['round'])} | {fmt(p['fold'])} |")
    out += ["",
            "## Time per launch against the prediction from `k_miller`",
            "",
            f"HIP events of the library (`gm_prof_enable(1)`), {L['launches']} calls each at 2^10 terms / pairs in this process: \"accumulate\" is the power",
            "kernel or `k_miller`, \"reduce\" the `k_gt_reduce` launches behind it.",
            "",
            "| kernel | Fq products per lane | ms per launch | reduce ms |",
            "|---|---|---|---|",
            f"| `k_miller` | {L['fq_per_lane_miller']} | {L['k_miller_ms']:.3f} | {L['k_miller_reduce_ms']:.3f} |",
            f"| `k_gt_multi_pow` | {L['fq_per_lane_pow']} | {L['k_gt_multi_pow_ms']:.3f} | {L['k_gt_reduce_ms']:.3f} |",
            "",
            f"Predicted from the product counts: {L['fq_per_lane_pow']} / {L['fq_per_lane_miller']} × {L['k_miller_ms']:.3f} ms = **{L['predicted_ms']:.2f} ms**; measured "
            f"**{L['k_gt_multi_pow_ms']:.2f} ms**, {L['measured_over_predicted']:.2f} of the prediction.",
            ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--host-max", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_module.md"))
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    gm.capi.init()
    e = gt_of_w(GR.E())
    rng = np.random.default_rng(7)
    pool = np.stack([gp.gt_pow(e, int.from_bytes(rng.bytes(31), "little")) for _ in range(POOL)])
    res = {"calls": args.calls, "window": source_window(), "shader_clock_mhz": shader_mhz()}
    res["multi_pow"] = [bench_multi_pow(1 << ld, pool, args.calls, args.host_max) for ld in (6, 10, 14)]
    res["crossover"] = []
    for ld in range(0, 8):
        xs, es = inputs(1 << ld, pool, 400 + ld)
        res["crossover"].append({"n": 1 << ld, "device": timed(lambda: gm.gt_multi_pow(xs, es), args.calls), "host": timed(lambda: host_multi_pow(xs, es), args.calls)})
    res["prover"] = [bench_prover(1 << ld, pool, max(args.calls // 2, 2)) for ld in (10, 14)]
    res["launch"] = bench_launch(pool, args.calls, res["window"])
    text = json.dumps(res)
    print(text)
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(text + "\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(markdown(res))


if __name__ == "__main__":
    main()
