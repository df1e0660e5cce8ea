#!/usr/bin/env python3
"""gm_ipa_new_many against a loop of gm_ipa_new (profiles/ipa_new_many.md).

  size     d = 2^10, the reference's own test size, over a CRS of 2 d points (generated on the device from known scalars: a
           benchmark CRS, see gemini_amd.ipa.Crs.from_scalars); S proofs of distinct vectors, S = 1, 2, 4, 16.  `--log-d 14 --S 1 4`
           adds the d = 2^14 column
  compare  ONE gm_ipa_new_many call (gm_set_ipa_new_many_min(1): S = 1 is the lockstep path too) against a loop of gm_ipa_new over the
           same vectors on fresh transcripts -- the parent's code path, which the new entry does not touch
  method   one process, the two paths alternate call by call, `--warmup` calls of each per S first, a host clock around calls that each
           end in a device synchronise; median with minimum and maximum over `--calls`

  --terms       one gm_g2_lincomb_many call over S n terms, in segments of 32 as the first level of the prover's sums has them, against
                S G2 MSMs of n points over a registered key, at the term counts of the first round of d = 2^10 and 2^14 (1.5 d): the
                rows behind the choice between one lane per term and per-proof MSMs
  --trace S K   no timing: K lockstep calls of S proofs, and exit.  For `rocprofv3 --kernel-trace --stats -- python
                tools/ipa_new_many_bench.py --trace S K` in a run of its own; the launches of one call are the difference of the
                counts at two values of K (the set-up launches cancel).  `--trace-stats S A.csv B.csv` folds two such tables (K = 1 and
                K = 3) into `--json`.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gemini_amd as gm  # noqa: E402
from gemini_amd import ipa  # noqa: E402
from gemini_amd.fr import fr_from_int  # noqa: E402

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
LABEL = b"ipa-new-many-bench"


def rand_fr(rng, n):
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)]


def canon(v):
    return np.array([[(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for x in v], dtype=np.uint64)


def setup(log_d, S):
    """-> (crs, a_monts, b_monts): one CRS of 2 d points and S pairs of vectors of d = 2^log_d scalars"""
    d = 1 << log_d
    rng = np.random.default_rng(0x1FB)
    crs = gm.Crs.from_scalars(canon(rand_fr(rng, 2 * d)), canon(rand_fr(rng, 2 * d)))
    vecs = [np.stack([fr_from_int(x) for x in rand_fr(rng, d)]) for _ in range(2 * S)]
    return crs, vecs[:S], vecs[S:]


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def call_many(crs, am, bm):
    S = len(am)
    trs = [gm.Transcript(LABEL) for _ in range(S)]
    proofs = gm.InnerProductProof.new_many(trs, crs, am, bm)
    assert ipa.new_many_path()[:2] == (S, 0)
    return trs, proofs


def call_loop(crs, am, bm):
    trs = [gm.Transcript(LABEL) for _ in am]
    return trs, [gm.InnerProductProof.new(t, crs, a, b) for t, a, b in zip(trs, am, bm)]


def measure(args):
    crs, am, bm = setup(args.log_d, max(args.S))
    ipa.set_new_many_min(1)
    rows = []
    for S in args.S:
        a, b = am[:S], bm[:S]
        tm, tl = [], []
        for i in range(args.warmup + args.calls):  # alternating: drift of the box lands on both
            kept = []
            t_many = clock(lambda: kept.append(call_many(crs, a, b)))
            t_loop = clock(lambda: kept.append(call_loop(crs, a, b)))
            if i == 0:  # the two paths give the same bytes
                for p, q in zip(kept[0][1], kept[1][1]):
                    assert p.fields().messages.tobytes() == q.fields().messages.tobytes()
            for trs, proofs in kept:
                for o in trs + proofs:
                    o.free()
            if i >= args.warmup:
                tm.append(t_many)
                tl.append(t_loop)
        rows.append({"S": S, "many": spread(tm), "loop": spread(tl), "path": list(ipa.new_many_path())})
        print(json.dumps(rows[-1]), flush=True)
    return {"log_d": args.log_d, "crs": 2 << args.log_d, "calls": args.calls, "warmup": args.warmup, "rows": rows}


def terms(args):
    """one lane per term against per-proof bucket MSMs in G2, at the term counts of a first round"""
    from gemini_amd.g2msm import G2Bases, g2_lincomb_many, g2_points_to_affine
    from gemini_amd import g2

    rng = np.random.default_rng(0x1FC)
    rows = []
    for log_d in (10, 14):
        n = 3 << (log_d - 1)
        key = G2Bases.fixed_base(g2_points_to_affine([g2.generator()])[0], canon(rand_fr(rng, n)))
        rec = key.download()
        for S in (1, 4, 16):
            sc = canon(rand_fr(rng, n))
            pts, scs = np.concatenate([rec] * S), np.concatenate([sc] * S)
            off = list(range(0, S * n, 32)) + [S * n]  # chunks of 32 terms, the first level of the prover's sums
            tl, tmsm = [], []
            for i in range(args.warmup + args.calls):
                t1 = clock(lambda: g2_lincomb_many(pts, scs, off))
                t2 = clock(lambda: [key.msm_bigint(sc) for _ in range(S)])
                if i >= args.warmup:
                    tl.append(t1)
                    tmsm.append(t2)
            rows.append({"log_d": log_d, "terms_per_proof": n, "S": S, "lincomb": spread(tl), "msm_loop": spread(tmsm)})
            print(json.dumps(rows[-1]), flush=True)
        key.free()
    return {"terms": rows}


def trace(log_d, S, K):
    crs, am, bm = setup(log_d, S)
    ipa.set_new_many_min(1)
    for _ in range(K):
        call_many(crs, am, bm)


def short(name):
    return name.split("(")[0].replace("void gm::", "").replace("gm::", "")


def kernel_calls(stats_csv):
    with open(stats_csv, newline="") as fh:
        return {short(r["Name"]): int(r["Calls"]) for r in csv.DictReader(fh)}


def per_call(k1_stats, k3_stats):
    """{kernel: [launches per lockstep call, mean ms of the LAST call's launches]}: the counts from the stats tables of a run with 1
    call and of a run with 3, the durations from the trace of the run with 3 (beside its stats table)"""
    a, b = kernel_calls(k1_stats), kernel_calls(k3_stats)
    with open(k3_stats.replace("_kernel_stats.csv", "_kernel_trace.csv"), newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for name in sorted(set(a) | set(b)):
        calls = b.get(name, 0) - a.get(name, 0)
        assert calls % 2 == 0, (name, calls)
        if calls:
            last = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if short(r["Kernel_Name"]) == name][-(calls // 2):]
            out[name] = [calls // 2, round(sum(last) / len(last) / 1e6, 3)]
    return out


def render(res):
    cell = lambda v: f"{v['median']:.1f} ({v['min']:.1f}–{v['max']:.1f})"  # noqa: E731
    out = ["# `gm_ipa_new_many` against a loop of `gm_ipa_new`", "",
           "`tools/ipa_new_many_bench.py`: S proofs of distinct vectors over one CRS of 2 d points.  One process; the two paths alternate call by",
           "call on fresh transcripts; a host clock around calls that each end in a device synchronise; median (min–max), in ms.",
           "`gm_set_ipa_new_many_min(1)` throughout, so S = 1 is the lockstep path too.  The yardstick, the loop, is the code path of `gm_ipa_new`,",
           "which the new entry does not touch.", ""]
    for key in sorted(k for k in res if k.startswith("d2^")):
        r = res[key]
        out += [f"## d = 2^{r['log_d']}, a CRS of {r['crs']} points ({r['warmup']} warm-up, {r['calls']} calls)", "",
                "| S | one `gm_ipa_new_many` call | loop of `gm_ipa_new` | loop / many | launches | waits |", "|---:|---:|---:|---:|---:|---:|"]
        for row in r["rows"]:
            out.append(f"| {row['S']} | {cell(row['many'])} | {cell(row['loop'])} | {row['loop']['median'] / row['many']['median']:.2f} | {row['path'][2]} | {row['path'][3]} |")
        wins = [row["S"] for row in r["rows"] if row["many"]["max"] < row["loop"]["min"]]
        out += ["", f"Smallest measured S at which the slowest lockstep call beats the fastest loop: {wins[0] if wins else 'none'}.", ""]
    if "terms" in res:
        out += ["## One lane per term against per-proof bucket MSMs (G2)", "",
                "One `gm_g2_lincomb_many` call over S n terms, in segments of 32 terms as the first level of the prover's sums has them, against S",
                "`gm_g2_msm_h` calls of n points over a registered key; n = 1.5 d, the terms of a proof's G2Module message in the first round.  Both",
                "columns include the upload of their scalars; the combination also uploads its points, which the prover does not.", "",
                "| d | terms per proof | S | one combination launch group | S MSMs |", "|---:|---:|---:|---:|---:|"]
        for row in res["terms"]:
            out.append(f"| 2^{row['log_d']} | {row['terms_per_proof']} | {row['S']} | {cell(row['lincomb'])} | {cell(row['msm_loop'])} |")
        out.append("")
    lp = res.get("launches_per_call", {})
    if lp:
        keys = sorted(lp, key=int)
        names = sorted(set().union(*[set(v) for v in lp.values()]))
        out += ["## Launches per lockstep call, d = 2^10", "",
                "`rocprofv3 --kernel-trace --stats` in runs of their own (no counter collection): `--trace S 1` and `--trace S 3`.  The difference of the two",
                "stats tables, halved, is one call -- the launches of the set-up cancel; ms is the mean duration of the last call's launches in the trace of the",
                "second run.", "", "| kernel | " + " | ".join(f"S = {k}: launches | ms each | ms" for k in keys) + " |", "|---|" + "---:|---:|---:|" * len(keys)]
        for n in names:
            out.append(f"| `{n}` | " + " | ".join(f"{lp[k].get(n, [0, 0])[0]} | {lp[k].get(n, [0, 0])[1]:.3f} | {lp[k].get(n, [0, 0])[0] * lp[k].get(n, [0, 0])[1]:.1f}" for k in keys) + " |")
        out += ["| all | " + " | ".join(f"{sum(v[0] for v in lp[k].values())} | | {sum(v[0] * v[1] for v in lp[k].values()):.1f}" for k in keys) + " |", ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--log-d", type=int, default=10)
    ap.add_argument("--S", type=int, nargs="+", default=[1, 2, 4, 16])
    ap.add_argument("--json", default="ipa_new_many.json")
    ap.add_argument("--md", help="render --json into this file and exit")
    ap.add_argument("--terms", action="store_true")
    ap.add_argument("--trace", nargs=2, type=int, metavar=("S", "K"))
    ap.add_argument("--trace-stats", nargs=3, metavar=("S", "K1_CSV", "K3_CSV"))
    args = ap.parse_args()
    if args.md:
        open(args.md, "w").write(render(json.load(open(args.json))))
        return
    res = json.load(open(args.json)) if os.path.exists(args.json) else {}
    if args.trace_stats:
        res.setdefault("launches_per_call", {})[args.trace_stats[0]] = per_call(args.trace_stats[1], args.trace_stats[2])
        json.dump(res, open(args.json, "w"), indent=1)
        return
    gm.capi.init()
    if args.trace:
        trace(args.log_d, *args.trace)
        return
    if args.terms:
        res.update(terms(args))
    else:
        res[f"d2^{args.log_d}"] = measure(args)
    json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
