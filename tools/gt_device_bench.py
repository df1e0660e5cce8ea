#!/usr/bin/env python3
"""GT element by element on the device (profiles/gt_device.md): gm_gt_final_exp_many, gm_pairing_each and gm_gt_check against the
host loops they replace and against their Fq product counts, and gm_vrs_from_crs against the parent commit's library.

Method (that of tools/gt_module_bench.py): host clock around calls that end in a device synchronise, one warm-up call, then `--calls`
timed calls; median with min - max.  Both sides of a comparison run in this process, except the library A/B of gm_vrs_from_crs:

  tools/gt_device_bench.py --vrs new    >> vrs.jsonl          (this build)
  GM_LIB_PATH=tools/_build/varparent/gemini_amd/libgemini_hip.so tools/gt_device_bench.py --vrs parent >> vrs.jsonl
  tools/gt_device_bench.py --vrs-jsonl vrs.jsonl              (everything else, and the report)

where varparent is the parent commit's csrc built the way tools/build_variants.sh builds a variant.  The shader clock is
gm_prof_read_clock's, from a G1 MSM under the profiler.  Kernel times are HIP events of the library (gm_prof_enable(1)).

usage: gt_device_bench.py [--calls 5] [--out profiles/gt_device.md] [--jsonl profiles/gt_device_bench.jsonl] [--vrs-jsonl FILE] | --vrs LABEL
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
from gemini_amd.g2msm import g2_points_to_affine  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from oracle import pairing as OP  # noqa: E402
from tests import gt_module_ref as GR  # noqa: E402
from tests import ipa_exponent_ref as X  # noqa: E402
from tests.stepwise import ipa as steps  # noqa: E402
from tests.test_pairing_cpu import gt_of_w  # noqa: E402

POOL = 64
Q = OP.Q
X_ABS = 0xD201000000010000
E3 = (X_ABS + 1) // 3
FQ_MILLER = 6700  # per pair, as k_miller is written (pairing.hip)
FQ12_MUL, CYC_SQR, FROB1, FROB2 = 54, 18, 15, 10


def pow_products(e: int) -> int:
    """fq12_pow_const: one cyclotomic squaring per bit below the top one, one product per set bit below it"""
    return (e.bit_length() - 1) * CYC_SQR + (bin(e).count("1") - 1) * FQ12_MUL


def fq_products():
    """Fq products per lane, counted from the kernels as written (gt.cuh, pairing.hip)"""
    fq_inv = 381 + bin(Q - 2).count("1")          # fq_inv (g1.cuh): a squaring per bit, a product per set bit
    fq2_inv = 2 + fq_inv + 2
    fq6_inv = 3 * (2 + 3) + 9 + fq2_inv + 9
    fq12_inv = 2 * 18 + fq6_inv + 2 * 18
    easy = fq12_inv + FQ12_MUL + FROB2 + FQ12_MUL
    hard = pow_products(E3) + 4 * pow_products(X_ABS) + FQ12_MUL + (FQ12_MUL + FROB1) + (2 * FQ12_MUL + FROB2) + FQ12_MUL
    return {"final_exp": easy + hard, "final_exp_easy": easy, "check": 2 * FROB2 + FQ12_MUL + pow_products(X_ABS) + FROB1, "miller": FQ_MILLER}


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "calls": len(ms)}


def timed(fn, calls, after=None):
    out = []
    for k in range(calls + 1):  # the first call is the warm-up
        t0 = time.perf_counter()
        r = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if after:
            after(r)
        if k:
            out.append(dt)
    return spread(out)


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
    return round(ms[3] / max(cnt[3], 1), 3), round(ms[5] / max(cnt[5], 1), 3)


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


def tile(a, n):
    return np.ascontiguousarray(np.tile(a, (-(-n // len(a)), 1))[:n])


def host_final_exps(xs):
    lib, out = gm.capi.load(), np.empty(72, dtype=np.uint64)
    for x in xs:
        lib.gm_gt_final_exp(gm.capi.ptr(x), gm.capi.ptr(out))


def single_pairings(r1, r2):
    lib, out = gm.capi.load(), np.empty(72, dtype=np.uint64)
    for i in range(len(r1)):
        lib.gm_pairing_multi(gm.capi.ptr(r1[i:i + 1]), C.c_size_t(96), gm.capi.ptr(r2[i:i + 1]), C.c_size_t(192), C.c_size_t(1), gm.capi.ptr(out))


def bench_vrs(label, calls):
    rng = np.random.default_rng(5)
    for logd in (10, 14):
        n = 2 << logd
        crs = gm.Crs.from_scalars(rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64), rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64))
        line = {"what": "vrs", "lib": label, "logd": logd, "crs": n, **timed(lambda: gm.Vrs(crs), calls, lambda v: v.free())}
        crs.free()
        print(json.dumps(line), flush=True)


def fmt(s):
    return f"{s['median_ms']:.2f} ({s['min_ms']:.2f} – {s['max_ms']:.2f})"


def markdown(res) -> str:
    fq, L = res["fq"], res["launch"]
    per = L["k_miller_ms"] / fq["miller"]
    cross = next((c["n"] for c in res["crossover"] if c["device"]["median_ms"] < c["host"]["median_ms"]), None)
    out = ["# GT element by element on the MI355X: final exponentiation, pairings and the membership check",
           "",
           "`python tools/gt_device_bench.py` wrote this file; the raw lines are in `gt_device_bench.jsonl`.  Host clock around calls that end in a",
           f"device synchronise, one warm-up call, then {res['calls']} timed calls: median (min – max).  One box, one process per library.  The shader",
           f"clock `gm_prof_read_clock` reports for a G1 accumulation of this process: **{res['shader_clock_mhz']} MHz**.",
           "",
           "## Fq products per lane and the time per launch",
           "",
           f"Counted from the kernels as written: `k_gt_final_exp` **{fq['final_exp']}** ({fq['final_exp_easy']} of them the easy part with its one Fermat",
           f"inversion in Fq), `k_gt_check` **{fq['check']}**, `k_miller` / `k_miller_each` {fq['miller']}.  `k_miller` at 2^10 pairs takes {L['k_miller_ms']:.3f} ms per",
           f"launch in this process (HIP events of the library), {per * 1e3:.2f} µs per Fq product and wave.  A launch of up to 2^16 lanes is one wave deep.",
           "",
           "| kernel | n | Fq products per lane | predicted ms | measured ms per launch | measured / predicted |",
           "|---|---|---|---|---|---|",
           f"| `k_gt_final_exp` | 2^10 | {fq['final_exp']} | {fq['final_exp'] * per:.2f} | {L['k_gt_final_exp_ms']:.3f} | {L['k_gt_final_exp_ms'] / (fq['final_exp'] * per):.2f} |",
           f"| `k_miller_each` | 2^10 | {fq['miller']} | {fq['miller'] * per:.2f} | {L['k_miller_each_ms']:.3f} | {L['k_miller_each_ms'] / (fq['miller'] * per):.2f} |",
           "",
           "## `gm_gt_final_exp_many` against n × `gm_gt_final_exp`",
           "",
           "The device call takes host elements: it uploads n × 576 bytes, converts, launches `k_gt_final_exp`, converts back and downloads.  The host",
           "loop is one `gm_gt_final_exp` per element on one CPU thread; above 64 elements it is timed on its first 64 and scaled.",
           "",
           "| n | device call ms | host loop ms | host / device |",
           "|---|---|---|---|"]
    for m in res["final_exp"]:
        out.append(f"| {m['n']} | {fmt(m['device'])} | {m['host_scaled_ms']:.1f} | **{m['host_scaled_ms'] / m['device']['median_ms']:.1f}** |")
    out += ["",
            "| n | device call ms | host loop ms |",
            "|---|---|---|"]
    for c in res["crossover"]:
        out.append(f"| {c['n']} | {fmt(c['device'])} | {fmt(c['host'])} |")
    out += ["",
            (f"The device call is faster from **n = {cross}** on (powers of two measured)." if cross else "The device call is not faster at any n measured here."),
            "Calls that make ONE final exponentiation stay on the host function.",
            "",
            "## `gm_pairing_each` against n single `gm_pairing_multi` calls",
            "",
            "The single calls are timed on the first 64 pairs and scaled.  Predicted: `k_miller`'s launch plus the `k_gt_final_exp` launch above.",
            "",
            "| n | device call ms | n single calls ms | single / each | predicted launches ms |",
            "|---|---|---|---|---|"]
    for m in res["pairing_each"]:
        out.append(f"| {m['n']} | {fmt(m['device'])} | {m['host_scaled_ms']:.0f} | **{m['host_scaled_ms'] / m['device']['median_ms']:.0f}** | "
                   f"{L['k_miller_ms'] + L['k_gt_final_exp_ms']:.2f} |")
    out += ["",
            "## `gm_gt_check`",
            "",
            f"Host elements in, one status byte per element out.  Predicted launch: {fq['check']} × {per * 1e3:.2f} µs = {fq['check'] * per:.2f} ms.",
            "",
            "| n | call ms |",
            "|---|---|"]
    for m in res["check"]:
        out.append(f"| {m['n']} | {fmt(m['device'])} |")
    out += ["", "## `gm_vrs_from_crs` against the parent commit's library", ""]
    if res["vrs"]:
        out += ["The parent finishes each of its 4 · levels Miller values with `pairing_finish` on the host; this build keeps them on the device and",
                "runs ONE conjugating `k_gt_final_exp` launch over them.  Same box, one process per library, alternating.",
                "",
                "| d | CRS | library | call ms |",
                "|---|---|---|---|"]
        for v in res["vrs"]:
            out.append(f"| 2^{v['logd']} | {v['crs']} | {v['lib']} | {fmt(v)} |")
        best = {}
        for v in res["vrs"]:
            best.setdefault(v["logd"], {}).setdefault(v["lib"], []).append(v["median_ms"])
        faster = all(statistics.median(b.get("new", [1e9])) < statistics.median(b.get("parent", [0])) for b in best.values())
        out += ["",
                ("**Decision: the switch stays** -- this build is faster at both sizes." if faster else
                 "**Decision: NOT faster at both sizes** -- `gm_vrs_from_crs` must keep `pairing_finish`.")]
    else:
        out += ["Not measured in this run (no `--vrs-jsonl`)."]
    out.append("")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_device.md"))
    ap.add_argument("--jsonl", default=os.path.join(ROOT, "profiles", "gt_device_bench.jsonl"))
    ap.add_argument("--vrs-jsonl", default=None)
    ap.add_argument("--vrs", default=None, metavar="LABEL")
    args = ap.parse_args()
    gm.capi.init()
    if args.vrs:
        bench_vrs(args.vrs, args.calls)
        return
    e = gt_of_w(GR.E())
    rng = np.random.default_rng(7)
    pool = np.stack([gp.gt_pow(e, int.from_bytes(rng.bytes(31), "little")) for _ in range(POOL)])
    p1, _, p2, _ = X.crs(64)
    g1, g2 = steps._g1_records(p1), g2_points_to_affine(p2)
    res = {"calls": args.calls, "shader_clock_mhz": shader_mhz(), "fq": fq_products(), "final_exp": [], "crossover": [], "pairing_each": [], "check": []}
    host64 = timed(lambda: host_final_exps(pool), args.calls)
    for n in (1, 64, 1 << 10, 1 << 14):
        xs = tile(pool, n)
        m = min(n, 64)
        host = timed(lambda: host_final_exps(xs[:m]), args.calls) if n < 64 else host64
        res["final_exp"].append({"n": n, "device": timed(lambda: gm.gt_final_exp_many(xs), args.calls), "host": host, "host_scaled_ms": round(host["median_ms"] * n / m, 2)})
    for n in (1, 2, 4, 8, 16, 32):
        xs = tile(pool, n)
        res["crossover"].append({"n": n, "device": timed(lambda: gm.gt_final_exp_many(xs), args.calls), "host": timed(lambda: host_final_exps(xs), args.calls)})
    single64 = timed(lambda: single_pairings(g1, g2), 2)
    for n in (1 << 10, 1 << 14):
        r1, r2 = tile(g1, n), tile(g2, n)
        res["pairing_each"].append({"n": n, "device": timed(lambda: gm.pairing_each(r1, r2), args.calls), "single_64": single64,
                                    "host_scaled_ms": round(single64["median_ms"] * n / 64, 1)})
    for n in (64, 1 << 10, 1 << 14):
        xs = tile(pool, n)
        res["check"].append({"n": n, "device": timed(lambda: gm.gt_check(xs), args.calls)})
    n = 1 << 10
    xs, r1, r2 = tile(pool, n), tile(g1, n), tile(g2, n)
    mil_ms, _ = prof(lambda: gm.multi_pairing(r1, r2), args.calls)
    _, fe_ms = prof(lambda: gm.gt_final_exp_many(xs), args.calls)
    each_ms, _ = prof(lambda: gm.pairing_each(r1, r2), args.calls)
    res["launch"] = {"n": n, "k_miller_ms": mil_ms, "k_gt_final_exp_ms": fe_ms, "k_miller_each_ms": each_ms}
    res["vrs"] = []
    if args.vrs_jsonl:
        with open(args.vrs_jsonl) as fh:
            res["vrs"] = [json.loads(ln) for ln in fh if ln.strip().startswith("{")]
    with open(args.jsonl, "w") as fh:
        for key in ("final_exp", "crossover", "pairing_each", "check"):
            for line in res[key]:
                fh.write(json.dumps({"what": key, **line}) + "\n")
        fh.write(json.dumps({"what": "launch", "shader_clock_mhz": res["shader_clock_mhz"], "fq": res["fq"], **res["launch"]}) + "\n")
        for line in res["vrs"]:
            fh.write(json.dumps(line) + "\n")
    with open(args.out, "w") as fh:
        fh.write(markdown(res))
    print(json.dumps(res["launch"]))


if __name__ == "__main__":
    main()
