#!/usr/bin/env python3
"""gm_ipa_new_batch against a loop of gm_ipa_new and against gm_ipa_new_many; gm_ipa_verify_batch against gm_ipa_verify_many
(profiles/ipa_new_batch.md).

  size     d = 2^log_d over a CRS of 2 d points (generated on the device from known scalars: a benchmark CRS, see
           gemini_amd.ipa.Crs.from_scalars); K claims of distinct vectors.  The issue's table is `--log-d 10 --K 1 2 4 16 64` and
           `--log-d 14 --K 1 4`
  compare  ONE gm_ipa_new_batch call (one proof for K claims) against a loop of K gm_ipa_new calls against ONE gm_ipa_new_many call
           with S = K (K proofs), all over the same vectors on fresh transcripts; then gm_ipa_verify_batch on the one proof against
           gm_ipa_verify_many on the K proofs.  The three forms prove the same K statements; they are not the same bytes
  method   one process, the forms alternate call by call (drift of the box lands on all of them), `--warmup` rounds first, a host
           clock around calls that each end in a device synchronise; median with minimum and maximum over `--calls` (at least 5)
  size of a proof in 64-bit limbs, counted from the fields: messages 144 R, challenges 4 R, batch challenges 4 (3 K + 2 (R - 1)),
           final foldings 54 x 2 (R - 1), foldings (8 + 22 + 40) K -- against K times the K = 1 figure
"""
import argparse
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
LABEL = b"ipa-new-batch-bench"


def rand_fr(rng, n):
    return [int.from_bytes(rng.bytes(32), "little") % R for _ in range(n)]


def canon(v):
    return np.array([[(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for x in v], dtype=np.uint64)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def proof_limbs(rounds: int, K: int) -> int:
    return 144 * rounds + 4 * rounds + 4 * (3 * K + 2 * (rounds - 1)) + 54 * 2 * (rounds - 1) + 70 * K


def measure(args):
    d = 1 << args.log_d
    rng = np.random.default_rng(0x1FD)
    crs = gm.Crs.from_scalars(canon(rand_fr(rng, 2 * d)), canon(rand_fr(rng, 2 * d)))
    vrs = gm.Vrs(crs)
    Kmax = max(args.K)
    ints = [(rand_fr(rng, d), rand_fr(rng, d)) for _ in range(Kmax)]
    am = [np.stack([fr_from_int(x) for x in a]) for a, _ in ints]
    bm = [np.stack([fr_from_int(x) for x in b]) for _, b in ints]
    ca, cb = np.stack([crs.commit_g1(a) for a in am]), np.stack([crs.commit_g2(b) for b in bm])
    y = np.stack([fr_from_int(sum(p * q for p, q in zip(a, b)) % R) for a, b in ints])
    ipa.set_new_many_min(1)
    ipa.set_verify_many_min(1)
    rows = []
    for K in args.K:
        a, b = am[:K], bm[:K]
        t = {k: [] for k in ("batch", "loop", "many", "verify_batch", "verify_many")}
        path = None
        for i in range(args.warmup + args.calls):
            tr = gm.Transcript(LABEL)
            tb, one = clock(lambda: gm.InnerProductProof.new_batch(tr, crs, a, b))
            path = ipa.new_batch_path()
            trs = [gm.Transcript(LABEL) for _ in range(K)]
            tl, loop = clock(lambda: [gm.InnerProductProof.new(x, crs, u, v) for x, u, v in zip(trs, a, b)])
            trm = [gm.Transcript(LABEL) for _ in range(K)]
            tm, many = clock(lambda: gm.InnerProductProof.new_many(trm, crs, a, b))
            tvb, okb = clock(lambda: one.verify_batch(vrs, ca[:K], cb[:K], y[:K]))
            tvm, okm = clock(lambda: gm.InnerProductProof.verify_many(many, vrs, ca[:K], cb[:K], y[:K]))
            assert okb and all(okm)
            if i == 0:
                rounds = one.fields().rounds
                assert loop[0].fields().messages.tobytes() == many[0].fields().messages.tobytes()
            for o in [one, tr] + loop + trs + many + trm:
                o.free()
            if i >= args.warmup:
                for k, v in zip(t, (tb, tl, tm, tvb, tvm)):
                    t[k].append(v)
        rows.append({"log_d": args.log_d, "K": K, **{k: spread(v) for k, v in t.items()}, "path": list(path),
                     "limbs_batch": proof_limbs(rounds, K), "limbs_K_proofs": K * proof_limbs(rounds, 1)})
        print(json.dumps(rows[-1]), flush=True)
    return {"log_d": args.log_d, "crs": 2 * d, "calls": args.calls, "warmup": args.warmup, "rows": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--log-d", type=int, default=10)
    ap.add_argument("--K", type=int, nargs="+", default=[1, 2, 4, 16, 64])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--json", help="write the result here")
    args = ap.parse_args()
    assert args.calls >= 5, "the median and range of at least five calls"
    gm.capi.init()
    out = measure(args)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
