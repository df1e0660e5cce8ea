#!/usr/bin/env python3
"""The verifiers on the device (profiles/verifier.md), in one process on one box.

  bilinear    gm_spm_bilinear_pm x 3 (A, B, C against powers(beta); weights tensor(rho) o powers(alpha), tensor(rho), powers(alpha)) against
              the composition it replaces on the UNCHANGED kernels -- 6 gm_spm_mul and 6 gm_fr_ip over powers(beta) and powers(-beta) -- for
              dummy_r1cs and for a random sparse instance of 4 entries per row.  The two are alternated, `--calls` rounds after a warm-up
              round; host clock around calls that each end in a device synchronise; median, min, max.  The gm_fr_powers calls (one for
              the fused form, two for the composition) are timed apart.  The values are compared before anything is timed.
  snark       gm_snark_verify on a device proof of dummy_r1cs (`snark -i N`), and its parts timed on their own with the same operands:
              the O(n) vector part (powers(beta, n), tensor(rho), powers(alpha), their Hadamard product, x at +-beta), the three
              bilinear forms, the KZG check (gm_kzg_verify_multi_points on the proof's commitments: one G1 MSM, one G2 MSM, one
              two-pair multi-pairing with its final exponentiation), and of that the pairing alone (gm_pairing_multi, 2 pairs)
  psnark      gm_psnark_verify on a device proof of dummy_r1cs (`psnark -i N`)

usage: verify_bench.py [--bilinear-logn 20 24] [--snark-logn 20 24] [--psnark-logn 20] [--calls 7] [--out FILE]
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
from gemini_amd import fr as F  # noqa: E402
from gemini_amd.circuit import SparseMatrix, dummy_r1cs  # noqa: E402
from gemini_amd.fr import FrVec, fr_from_int  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from oracle import pyref as P  # noqa: E402

E = 0x1D2C3B4A59687766554433221100FFEE % P.R_MOD
TAU = 0x0123456789ABCDEF0FEDCBA987654321 % P.R_MOD


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "calls": len(ms)}


def random_sparse(n, per_row, seed):
    """three n x n matrices of `per_row` entries per row: random columns, values from a table of 2^20 random field elements (the times do
    not depend on the values)"""
    table = orc.fr_to_mont(orc.random_fr(seed, 1 << 20))
    rng = np.random.default_rng(seed)
    rowptr = np.arange(n + 1, dtype=np.uint64) * np.uint64(per_row)
    mats = []
    for k in range(3):
        cols = rng.integers(0, n, size=n * per_row, dtype=np.uint32)
        vals = table[rng.integers(0, len(table), size=n * per_row)]
        mats.append(SparseMatrix.from_csr(rowptr, cols, vals, n, n))
        mats[-1].csr = None
    return mats


def bench_bilinear(logn, kind, calls):
    n = 1 << logn
    rng = P.SplitMix64(77 + logn)
    if kind == "dummy":
        d = SparseMatrix.from_csr(np.arange(n + 1, dtype=np.uint64), np.arange(n, dtype=np.uint32), np.tile(fr_from_int(pow(E, -1, P.R_MOD)), (n, 1)), n, n)
        mats = [d, d, d]
    else:
        mats = random_sparse(n, 4, 5 + logn)
    beta, alpha = rng.fr(), rng.fr()
    rho = np.stack([fr_from_int(rng.fr()) for _ in range(logn)])
    t = F.tensor(rho)
    a = F.powers(fr_from_int(alpha), n)
    weights = [F.hadamard(t, a), t, a]
    bm, nbm = fr_from_int(beta), fr_from_int((-beta) % P.R_MOD)

    def fused(bp):
        return [m.bilinear_pm(bp, w) for m, w in zip(mats, weights)]

    def composition(bp, nbp):
        out = []
        for m, w in zip(mats, weights):
            pair = []
            for pw in (bp, nbp):
                y = m.mul(pw)
                pair.append(F.ip(y, w))
                y.free()
            out.append(tuple(pair))
        return out

    bp, nbp = F.powers(bm, n), F.powers(nbm, n)
    for (p1, n1), (p2, n2) in zip(fused(bp), composition(bp, nbp)):  # same values, and the warm-up round
        assert (p1 == p2).all() and (n1 == n2).all(), "the fused form and the composition differ"
    tf, tc, tp = [], [], []
    for _ in range(calls):
        tf.append(clock(lambda: fused(bp))[0])
        tc.append(clock(lambda: composition(bp, nbp))[0])
        ms, v = clock(lambda: F.powers(bm, n))
        v.free()
        tp.append(ms)
    for v in weights + [bp, nbp]:
        v.free()
    for m in {id(m): m for m in mats}.values():
        m.free()
    f, c, p = summary(tf), summary(tc), summary(tp)
    return {"logn": logn, "instance": kind, "entries_per_row": 1 if kind == "dummy" else 4, "fused_3_calls": f, "composition_12_calls": c, "one_gm_fr_powers": p,
            "speedup_kernels": round(c["median_ms"] / f["median_ms"], 3),
            "speedup_with_powers": round((c["median_ms"] + 2 * p["median_ms"]) / (f["median_ms"] + p["median_ms"]), 3)}


def bench_snark(logn, calls):
    from gemini_amd.kzg import CommitterKey, VerificationError, VerifierKey
    from gemini_amd.snark import Proof

    n = 1 << logn
    ck = CommitterKey.new(2 * n, 5, orc.ints_to_limbs([TAU], 4)[0])
    vk = VerifierKey.from_committer_key(ck)
    r1cs = dummy_r1cs(E, n)
    proof = Proof.new_time(r1cs, ck)
    prover_ms = proof.spans["ark_gemini::snark::time_prover"] * 1e3
    proof.verify(r1cs, vk)
    whole = [clock(lambda: proof.verify(r1cs, vk))[0] for _ in range(calls)]
    # the parts, on operands of the same shapes (the challenges do not matter for the times)
    rng = P.SplitMix64(logn)
    beta, alpha = fr_from_int(rng.fr()), fr_from_int(rng.fr())
    rho = np.stack([fr_from_int(rng.fr()) for _ in range(logn)])
    pts = np.stack([beta, fr_from_int((-F.fr_to_int(beta)) % P.R_MOD)])

    def vectors():
        bp = F.powers(beta, n)
        t = F.tensor(rho)
        a = F.powers(alpha, n)
        h = F.hadamard(t, a)
        F.evaluate_le(r1cs.x, pts)
        return bp, [h, t, a]

    bp, w = vectors()
    tv, tb = [], []
    for _ in range(calls):
        for v in [bp] + w:
            v.free()
        ms, (bp, w) = clock(vectors)
        tv.append(ms)
        tb.append(clock(lambda: [m.bilinear_pm(bp, x) for m, x in zip((r1cs.a, r1cs.b, r1cs.c), w)])[0])
    for v in [bp] + w:
        v.free()
    tc = proof.tensorcheck_proof
    comms = [proof.witness_commitment] + list(tc.folded_polynomials_commitments)
    ev = np.zeros((len(comms), 3, 4), dtype=np.uint64)
    kp = np.stack([fr_from_int(3), fr_from_int(5), fr_from_int(7)])

    def kzg():
        try:
            vk.verify_multi_points(comms, kp, ev, tc.evaluation_proof, fr_from_int(11))
        except VerificationError:
            pass  # the claimed evaluations are not the proof's: the work is the same

    kzg()
    tk = [clock(kzg)[0] for _ in range(calls)]
    from gemini_amd.kzg import g1_generator_mont, g2_records
    from gemini_amd import g2 as G2

    g1 = np.stack([g1_generator_mont(), g1_generator_mont()])
    g2 = np.ascontiguousarray(np.repeat(g2_records([G2.generator()]), 2, axis=0))
    gt = np.zeros(72, dtype=np.uint64)
    pair = lambda: gm.capi.check(gm.capi.load().gm_pairing_multi(gm.capi.ptr(g1), C.c_size_t(96), gm.capi.ptr(g2), C.c_size_t(192), C.c_size_t(2), gm.capi.ptr(gt)))  # noqa: E731
    pair()
    tpair = [clock(pair)[0] for _ in range(calls)]
    r1cs.free()
    vk.free()
    ck.powers_of_g.free()
    return {"logn": logn, "prover_ms": round(prover_ms, 3), "gm_snark_verify": summary(whole), "vector_part": summary(tv), "three_bilinear_forms": summary(tb),
            "kzg_check": summary(tk), "of_it_pairing_2_pairs": summary(tpair), "commitments": len(comms)}


def bench_psnark(logn, calls):
    from gemini_amd.kzg import CommitterKey, VerifierKey
    from gemini_amd.psnark import Proof

    n = 1 << logn
    ck = CommitterKey.new(2 * n + 1, 5, orc.ints_to_limbs([TAU], 4)[0])
    vk = VerifierKey.from_committer_key(ck)
    r1cs = dummy_r1cs(E, n)
    index = Proof.index(ck, r1cs)
    proof = Proof.new_time(ck, r1cs, index)
    proof.verify(r1cs, vk, index, n)
    ms = [clock(lambda: proof.verify(r1cs, vk, index, n))[0] for _ in range(calls)]
    out = {"logn": logn, "prover_ms": round(proof.spans["ark_gemini::psnark::time_prover"] * 1e3, 3), "gm_psnark_verify": summary(ms)}
    r1cs.free()
    vk.free()
    ck.powers_of_g.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bilinear-logn", type=int, nargs="*", default=[20, 24])
    ap.add_argument("--snark-logn", type=int, nargs="*", default=[20, 24])
    ap.add_argument("--psnark-logn", type=int, nargs="*", default=[20])
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    gm.capi.init()
    res = {"bilinear": [], "snark": [], "psnark": []}
    for logn in args.bilinear_logn:
        for kind in ("dummy", "random"):
            res["bilinear"].append(bench_bilinear(logn, kind, args.calls))
            print(json.dumps(res["bilinear"][-1]), flush=True)
    for logn in args.snark_logn:
        res["snark"].append(bench_snark(logn, args.calls))
        print(json.dumps(res["snark"][-1]), flush=True)
    for logn in args.psnark_logn:
        res["psnark"].append(bench_psnark(logn, args.calls))
        print(json.dumps(res["psnark"][-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
