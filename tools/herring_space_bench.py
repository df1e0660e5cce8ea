#!/usr/bin/env python3
"""herring's module space prover against the module time prover (profiles/herring_space.md), both on the same data in one process.

For G1Module and G2Module at n = 2^16 and 2^20 (nf = ng = n, a twist != 1):
  space     G*ModuleSpaceProver over a registered key: every next_message timed on its own, final_foldings, the whole sumcheck
  time      G*ModuleTimeProver over the same vectors (host records: the upload is outside the clock): the same
  to_time   the cost of to_time() after k folds, k = 1, 2, 4, 8
  peak      gm_mem_stats in_use_peak over the run, minus what was in use before the prover was made (so the key does not count)
  msm       one gm_g*_msm_d call of n pairs on the same key, and for G1 the per-MSM time of a two-call batch: the prediction is
            2 x that per message and rounds x that for the sumcheck
For G1 at 2^20 the space prover also runs with the key's fixed-base tables switched off (gm_set_msm_table_min).

Method: host clock around calls that end in a device synchronise; one warm-up run, then `--runs` timed runs, median (min - max).
The shader clock is gm_prof_read_clock's, from a G1 MSM under the library's profiler at the end.

usage: herring_space_bench.py [--logn 16 20] [--runs 3] [--out profiles/herring_space.md] [--json FILE]
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
from gemini_amd import herring  # noqa: E402
from gemini_amd.fr import FrVec, fr_from_int  # noqa: E402
from gemini_amd.g2msm import G2Bases, g2_points_to_affine  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import g2_ref  # noqa: E402

TWIST = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E3


def med(v):
    return {"ms": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def sumcheck(P, ch):
    """-> (ms per message, ms of final_foldings, ms of the whole run)"""
    per, vm, k = [], None, 0
    t0 = time.perf_counter()
    while True:
        dt, m = clock(lambda: P.next_message(vm))
        if m is None:
            break
        per.append(dt)
        vm = ch[k]
        k += 1
    dtf, _ = clock(P.final_foldings)
    return per, dtf, (time.perf_counter() - t0) * 1e3


def peak_of(make, ch):
    base = gm.capi.mem_stats()["in_use"]
    gm.capi.mem_reset_peak()
    P = make()
    sumcheck(P, ch)
    peak = gm.capi.mem_stats()["in_use_peak"] - base
    P.free()
    return int(peak)


def bench_runs(make, ch, runs):
    per, fin, whole = [], [], []
    for i in range(runs + 1):
        P = make()
        p, f, w = sumcheck(P, ch)
        P.free()
        if i:
            per.append(p)
            fin.append(f)
            whole.append(w)
    rounds = len(per[0])
    return {"rounds": rounds, "per_message_ms": [round(statistics.median(r[k] for r in per), 3) for k in range(rounds)], "final": med(fin), "whole": med(whole)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    gm.capi.init(0)
    orc.build()
    lib = gm.capi.load()
    tw = fr_from_int(TWIST)
    ch = orc.fr_to_mont(orc.random_fr(4203, 32))
    tau = orc.random_fr(4201, 1)[0]
    g2gen = g2_points_to_affine([g2_ref.G])[0]
    res = {"runs": a.runs, "cases": []}
    for logn in a.logn:
        n = 1 << logn
        sc = orc.random_fr(4202, n)  # any integers below r are Montgomery images of field elements
        vec = FrVec.from_host(sc)
        for module in ("G1", "G2"):
            if module == "G1":
                key = gm.G1Bases.srs(orc.g1_generator(), tau, n)
                rec = key.download()
                space = lambda: herring.G1ModuleSpaceProver(key, vec, tw)  # noqa: E731
                timep = lambda: herring.G1ModuleTimeProver(rec[::-1].copy(), sc[::-1].copy(), tw)  # noqa: E731
                tables = key.table_info()
            else:
                key = G2Bases.srs(g2gen, tau, n)
                rec = key.download()
                space = lambda: herring.G2ModuleSpaceProver(vec, key, tw)  # noqa: E731
                timep = lambda: herring.G2ModuleTimeProver(sc[::-1].copy(), rec[::-1].copy(), tw)  # noqa: E731
                tables = (0, 0)
            case = {"module": module, "logn": logn, "tables_c": tables[0], "tables_bytes": tables[1]}
            # one MSM of n pairs on this key, scalars on the device
            dptr = vec.device_ptr()
            one = [clock(lambda: key.msm_device(dptr, n, True))[0] for _ in range(a.runs + 1)][1:]
            case["msm_one_call"] = med(one)
            if module == "G1":
                two = [clock(lambda: key.msm_vec_batch([vec, vec], [n, n]))[0] / 2 for _ in range(a.runs + 1)][1:]
                case["msm_per_call_of_two"] = med(two)
            case["space"] = bench_runs(space, ch, a.runs)
            case["space_peak_bytes"] = peak_of(space, ch)
            if module == "G1" and tables[0] and logn >= 17:
                gm.capi.check(lib.gm_set_msm_table_min(C.c_size_t(1 << 62)))
                case["space_no_tables"] = bench_runs(space, ch, a.runs)
                one = [clock(lambda: key.msm_device(dptr, n, True))[0] for _ in range(a.runs + 1)][1:]
                case["msm_one_call_no_tables"] = med(one)
                gm.capi.check(lib.gm_set_msm_table_min(C.c_size_t(1 << 17)))
            case["time"] = bench_runs(timep, ch, a.runs)
            case["time_peak_bytes"] = peak_of(timep, ch)
            tt = {}
            for k in (1, 2, 4, 8):
                S = space()
                for j in range(k):
                    S.fold(ch[j])
                dt, T = clock(S.to_time)
                tt[k] = round(dt, 3)
                T.free()
                S.free()
            case["to_time_ms_after_k_folds"] = tt
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            key.free()
        vec.free()
    # the shader clock, from a G1 MSM under the profiler
    key = gm.G1Bases.srs(orc.g1_generator(), tau, 1 << 16)
    v = FrVec.from_host(orc.random_fr(4204, 1 << 16))
    gm.capi.check(lib.gm_prof_enable(C.c_int(1)))
    key.msm_device(v.device_ptr(), 1 << 16, True)
    mhz = C.c_double()
    gm.capi.check(lib.gm_prof_read_clock(C.byref(mhz)))
    gm.capi.check(lib.gm_prof_enable(C.c_int(0)))
    res["shader_clock_mhz"] = round(mhz.value, 1)
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)
    if a.out:
        write_md(res, a.out)


def switch_round(space, timep, tt):
    """the first measured k at which to_time after k folds plus the time prover's remaining rounds beats the space prover's"""
    for k in sorted(tt):
        if k >= len(space):
            break
        if tt[k] + sum(timep[k:]) < sum(space[k:]):
            return k
    return None


def write_md(res, path):
    L = ["# herring's module space prover against the module time prover", "",
         "`python tools/herring_space_bench.py --out profiles/herring_space.md`: both provers on the same data in one process on one MI355X;",
         f"host clock around calls that end in a device synchronise, one warm-up run, then {res['runs']} timed runs, median (min – max). Shader clock",
         f"`gm_prof_read_clock` reports for a G1 accumulation of this process: **{res['shader_clock_mhz']} MHz**. nf = ng = n, twist ≠ 1.", "",
         "The prediction: one message costs 2 × one MSM of n pairs on the key (G1: the per-call time of a two-call batch), the sumcheck rounds × that.", "",
         "| module | n | tables | one MSM, ms | message, ms (median over rounds) | predicted | ratio | sumcheck, ms | predicted | ratio | time prover sumcheck, ms | space peak, MiB | time peak, MiB |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    notes = []
    for c in res["cases"]:
        msm = c.get("msm_per_call_of_two", c["msm_one_call"])["ms"]
        sp, tp = c["space"], c["time"]
        msg = statistics.median(sp["per_message_ms"])
        pm, ps = 2 * msm, 2 * msm * sp["rounds"]
        w = sp["whole"]
        L.append(f"| {c['module']} | 2^{c['logn']} | {'c = %d' % c['tables_c'] if c['tables_c'] else 'none'} | {msm} | {round(msg, 3)} | {round(pm, 3)} | "
                 f"{round(msg / pm, 2)} | {w['ms']} ({w['min']} – {w['max']}) | {round(ps, 1)} | {round(w['ms'] / ps, 2)} | {tp['whole']['ms']} "
                 f"({tp['whole']['min']} – {tp['whole']['max']}) | {round(c['space_peak_bytes'] / 2**20, 1)} | {round(c['time_peak_bytes'] / 2**20, 1)} |")
        k = switch_round(sp["per_message_ms"], tp["per_message_ms"], {int(a): b for a, b in c["to_time_ms_after_k_folds"].items()})
        notes.append(f"- {c['module']} 2^{c['logn']}: space messages by round {sp['per_message_ms']} ms; time prover rounds (fold + message) "
                     f"{tp['per_message_ms']} ms; to_time after k folds {c['to_time_ms_after_k_folds']} ms; "
                     + (f"of k = 1, 2, 4, 8 the first at which to_time plus the time prover's remaining rounds is cheaper than the space prover's remaining rounds: **k = {k}**"
                        if k is not None else "at none of k = 1, 2, 4, 8 is to_time plus the time prover's remaining rounds cheaper than staying"))
        if "space_no_tables" in c:
            nt = c["space_no_tables"]
            notes.append(f"  - the same space prover with the key's tables switched off: message {round(statistics.median(nt['per_message_ms']), 3)} ms, sumcheck "
                         f"{nt['whole']['ms']} ms; one MSM without tables {c['msm_one_call_no_tables']['ms']} ms")
    L += ["", "Per round:", ""] + notes + [""]
    open(path, "w").write("\n".join(L))


if __name__ == "__main__":
    main()
