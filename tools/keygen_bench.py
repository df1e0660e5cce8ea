#!/usr/bin/env python3
"""Key generation on the device (profiles/keygen.md, profiles/keygen_bench.jsonl): gm_g1_/gm_g2_fixed_base_register,
gm_g1_/gm_g2_srs_register, gm_g1_bases_from_candidates and gm_g2_bases_from_candidates at 2^16 and 2^20 produced points,
gm_g1_bases_precompute (the window tables, c = 20) on the 2^20 key, gm_crs_fold at 2^14 points.

  call time   host clock around the C call (each ends in a stream synchronise): one warm-up, then the median of `--calls` with min
              and max.  A call includes the upload of its scalars / candidates from pageable host memory and the allocation of the
              key; the handle it hands out is freed outside the timed region
  clock       gm_prof_read_clock after a small G1 MSM under the profiler: the shader clock the library measured
  yardsticks  in the same process: gm_g2_bases_check on a generated key (1674 Fq products a point, points.hip) and the accumulation
              stage of a G2 MSM (gm_prof_read; 28 Fq products per mixed addition, one per non-zero digit).  A kernel's prediction is
              its Fq-product count, read off its loops, at each of the two rates
  SRS         today's alternative for the G2 half of CommitterKey.new: gemini_amd.g2.mul on Python integers, timed over
              `--py-points` points and scaled
  candidates  uniformly random bytes (numpy), 4 n + 64 of them for n points, as Crs.new asks of its SHAKE-256 stream

usage: keygen_bench.py [--logn 16 20] [--fold-logn 14] [--calls 5] [--out-dir profiles]
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
from gemini_amd import g2 as G2  # noqa: E402
from gemini_amd.fr import FrVec, fr_from_int  # noqa: E402
from gemini_amd.g2msm import g2_points_to_affine  # noqa: E402
from gemini_amd.kzg import g1_generator_mont  # noqa: E402

TAU = 0x2F4E6D8C0B1A39587766554433221100FFEEDDCCBBAA9988776655443322110F % G2.R_ORDER
# Fq products, read off the kernels' loops (a square counts as a product; Fq2 product 3, Fq2 square 2; G2 doubling 24, mixed
# addition 28, full addition 37; G1 doubling 9, mixed addition 10)
P_CHECK_G2 = 1674                                  # k_pt_check<PtG2> (points.hip)
P_MADD_G2 = 28
P_INV = 380 + 190 + 2 + 2 + 2                      # fq2_inv: two squares, the Fermat ladder, two products
P_NORM_G2 = 6 + 3 + 6 + 6 + 6 + P_INV / 8          # k_normalise<GrpG2> (bases.hip) per point: prefix, 1 / (zz zzz), update, x, y; an inversion per 8
P_FIXED_G2 = 31 * P_MADD_G2 + P_NORM_G2            # 32 non-zero digits: the first lands in an empty accumulator
P_ROOT_G1, P_ROOT_G2 = 5 + 606, 9 + 1221           # candidate -> curve point (rules 1 and 2)
P_CLEAR_G1 = 63 * 9 + 6 * 10                       # [|x|] P + P
P_CLEAR_G2 = 2 * 63 * 24 + 6 * 28 + 5 * 37 + 135   # two ladders and the tail (points.hip: pt_g2_clear)
P_NORM_G1 = 2 + 1 + 2 + 2 + 2 + (380 + 190) / 8    # k_normalise<GrpG1> per point
P_FOLD_G1 = 255 * 9 + 127 * 10 + 10 + 575          # k_split_fold<GrpG1> per output: the ladder of an average scalar, one addition, one inversion
P_FOLD_G2 = 255 * 24 + 127 * 28 + 28 + P_INV + 15  # k_split_fold<GrpG2>


def timed(fn, calls, after=None):
    ts = []
    for k in range(calls + 1):  # the first call is the warm-up
        t0 = time.perf_counter()
        r = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if after:
            after(r)
        if k:
            ts.append(dt)
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3)}


def shader_mhz(lib):
    rng = np.random.default_rng(1)
    sc = rng.integers(0, 1 << 64, size=(1 << 14, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 62) - 1)
    key = gm.G1Bases.fixed_base(g1_generator_mont(), sc)
    gm.capi.check(lib.gm_prof_enable(C.c_int(1)))
    key.msm_bigint(sc)
    mhz = C.c_double()
    gm.capi.check(lib.gm_prof_read_clock(C.byref(mhz)))
    gm.capi.check(lib.gm_prof_enable(C.c_int(0)))
    key.free()
    return round(mhz.value, 1)


def g2_acc_rate(lib, key, sc, n, calls):
    """Fq products / s of k_g2_acc in a G2 MSM of n pairs: 28 per entry, an entry per non-zero 16-bit digit"""
    vec = FrVec.from_host(sc[:n])
    fn = lambda: key.msm_device(vec.device_ptr(), n, mont=False)  # noqa: E731
    fn()
    gm.capi.check(lib.gm_prof_enable(C.c_int(1)))
    for _ in range(calls):
        fn()
    ms, cnt = np.zeros(8), np.zeros(8, dtype=np.uint64)
    gm.capi.check(lib.gm_prof_read(gm.capi.ptr(ms), gm.capi.ptr(cnt), C.c_int(8)))
    gm.capi.check(lib.gm_prof_enable(C.c_int(0)))
    vec.free()
    acc_ms = ms[3] / calls
    windows = 16 if n > (1 << 17) else 22  # c = 16 above 2^17 pairs, c = 12 below (g2msm.hip: g2_choose_window); 255-bit scalars
    return acc_ms, n * windows * P_MADD_G2 / (acc_ms * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--fold-logn", type=int, default=14)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--py-points", type=int, default=8)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    gm.capi.init()
    lib = gm.capi.load()
    gm.capi.check(lib.gm_set_auto_tables(C.c_int(0), C.c_size_t(0)))
    rows = []

    def emit(**kw):
        rows.append(kw)
        print(json.dumps(kw), flush=True)

    emit(what="shader_clock", mhz=shader_mhz(lib))
    g2rec = g2_points_to_affine([G2.generator()])[0]
    tau = np.array([(TAU >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
    rng = np.random.default_rng(2026)
    free_g1 = lambda h: gm.capi.check(lib.gm_g1_bases_free(C.c_uint64(h)))  # noqa: E731
    free_g2 = lambda h: gm.capi.check(lib.gm_g2_bases_free(C.c_uint64(h)))  # noqa: E731

    t0 = time.perf_counter()
    for i in range(a.py_points):
        G2.mul(G2.generator(), pow(TAU, i + 1, G2.R_ORDER))
    emit(what="python_g2_mul", points=a.py_points, ms_per_point=round((time.perf_counter() - t0) * 1e3 / a.py_points, 3))

    one = rng.integers(0, 1 << 62, size=(1, 4), dtype=np.uint64)
    h1 = C.c_uint64(0)

    def fixed_one():  # the table alone: its last window is a chain of 248 doublings in one lane
        gm.capi.check(lib.gm_g2_fixed_base_register(gm.capi.ptr(g2rec), gm.capi.ptr(one), C.c_size_t(1), C.byref(h1)))
        return h1.value

    emit(what="gm_g2_fixed_base_register_one_point", **timed(fixed_one, a.calls, free_g2))
    g1rec = g1_generator_mont()

    def fixed_one_g1():
        gm.capi.check(lib.gm_g1_fixed_base_register(gm.capi.ptr(g1rec), gm.capi.ptr(one), C.c_size_t(1), C.byref(h1)))
        return h1.value

    emit(what="gm_g1_fixed_base_register_one_point", **timed(fixed_one_g1, a.calls, free_g1))

    for logn in a.logn:
        n = 1 << logn
        sc = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        sc[:, 3] &= np.uint64((1 << 62) - 1)  # < 2^254 < r: the MSM yardstick reads the same scalars
        h = C.c_uint64(0)

        def fixed():
            gm.capi.check(lib.gm_g2_fixed_base_register(gm.capi.ptr(g2rec), gm.capi.ptr(sc), C.c_size_t(n), C.byref(h)))
            return h.value

        def srs():
            gm.capi.check(lib.gm_g2_srs_register(gm.capi.ptr(g2rec), gm.capi.ptr(tau), C.c_size_t(n), C.byref(h)))
            return h.value

        emit(what="gm_g2_fixed_base_register", logn=logn, products_per_point=round(P_FIXED_G2, 1), **timed(fixed, a.calls, free_g2))
        emit(what="gm_g2_srs_register", logn=logn, products_per_point=round(P_FIXED_G2, 1), **timed(srs, a.calls, free_g2))

        def fixed_g1():  # (the automatic window tables are off, above: the call is the generation alone)
            gm.capi.check(lib.gm_g1_fixed_base_register(gm.capi.ptr(g1rec), gm.capi.ptr(sc), C.c_size_t(n), C.byref(h)))
            return h.value

        def srs_g1():
            gm.capi.check(lib.gm_g1_srs_register(gm.capi.ptr(g1rec), gm.capi.ptr(tau), C.c_size_t(n), C.byref(h)))
            return h.value

        emit(what="gm_g1_fixed_base_register", logn=logn, **timed(fixed_g1, a.calls, free_g1))
        emit(what="gm_g1_srs_register", logn=logn, **timed(srs_g1, a.calls, free_g1))
        if logn == 20:  # 12 rows of 2^20 doublings-by-20 and their normalisation (msm.hip: build_window_table)
            key1 = gm.G1Bases.fixed_base(g1rec, sc)
            emit(what="gm_g1_bases_precompute", logn=logn, c=20, **timed(lambda: key1.precompute(20), a.calls))
            key1.free()

        # the yardsticks, on a generated key
        key = gm.G2Bases.fixed_base(g2rec, sc)
        ok, fb = C.c_int(0), C.c_size_t(0)

        def check():
            gm.capi.check(lib.gm_g2_bases_check(C.c_uint64(key.handle), C.c_size_t(0), C.c_size_t(n), None, C.byref(fb), C.byref(ok)))
            assert ok.value == 1

        t = timed(check, a.calls)
        emit(what="gm_g2_bases_check", logn=logn, products_per_point=P_CHECK_G2, rate_gproducts_s=round(n * P_CHECK_G2 / t["median_ms"] / 1e6, 2), **t)
        acc_ms, rate = g2_acc_rate(lib, key, sc, n, a.calls)
        emit(what="k_g2_acc", logn=logn, acc_ms=round(acc_ms, 3), rate_gproducts_s=round(rate / 1e9, 2))
        key.free()

        for group, fn, free in ((1, lib.gm_g1_bases_from_candidates, free_g1), (2, lib.gm_g2_bases_from_candidates, free_g2)):
            m = 4 * n + 64
            cand = rng.integers(0, 256, size=m * 48 * group, dtype=np.uint8)
            used, found = C.c_size_t(0), C.c_size_t(0)

            def draw():
                gm.capi.check(fn(gm.capi.ptr(cand), C.c_size_t(m), C.c_size_t(n), C.byref(h), C.byref(used), C.byref(found)))
                assert h.value and found.value == n
                return h.value

            t = timed(draw, a.calls, free)
            # candidates read per produced point; of those the share below q reaches the root, the squares among them the clearing
            x = cand.view("<u8").reshape(m * group, 6)[: used.value * group]
            top = x[:, 5] & np.uint64((1 << 61) - 1)  # bits 320 .. 380: enough to compare with q's top word but for a 2^-61 sliver
            below = (top < np.uint64(G2.Q >> 320)).reshape(-1, group).all(axis=1).sum()
            emit(what=f"gm_g{group}_bases_from_candidates", logn=logn, candidates=m, used=used.value, read_per_point=round(used.value / n, 3),
                 roots_per_point=round(float(below) / n, 3), **t)

    nf = 1 << a.fold_logn
    crs = gm.Crs.from_scalars(rng.integers(0, 1 << 62, size=(nf, 4), dtype=np.uint64), rng.integers(0, 1 << 62, size=(nf, 4), dtype=np.uint64))
    ch = fr_from_int(int(rng.integers(1, 1 << 62)) ** 4 % G2.R_ORDER)
    emit(what="gm_crs_fold", logn=a.fold_logn, products_per_output_g1=P_FOLD_G1, products_per_output_g2=P_FOLD_G2, **timed(lambda: crs.fold(ch), a.calls, lambda c: c.free()))
    crs.free()

    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "keygen_bench.jsonl"), "w") as fh:
        fh.write("\n".join(json.dumps(r) for r in rows) + "\n")
    with open(os.path.join(a.out_dir, "keygen.md"), "w") as fh:
        fh.write(report(rows, a))


def report(rows, a) -> str:
    get = lambda what, logn=None: next(r for r in rows if r["what"] == what and (logn is None or r.get("logn") == logn))  # noqa: E731
    ms = lambda r: f"**{r['median_ms']}** ({r['min_ms']} – {r['max_ms']})"  # noqa: E731
    out = ["# Key generation on the device", "",
           "What is measured: `gm_g2_fixed_base_register`, `gm_g2_srs_register` (`gemini_amd/csrc/g2msm.hip`), `gm_g1_bases_from_candidates`, "
           "`gm_g2_bases_from_candidates` (`points.hip`) and `gm_crs_fold` (`ipa.hip`). Tool: `tools/keygen_bench.py`; raw lines: "
           "`profiles/keygen_bench.jsonl`; compiler resource report: `profiles/keygen_kernel_resources.txt`.", "",
           f"Method: host clock around the C call, which ends in a stream synchronise. One warm-up call, then the median of {a.calls} with minimum "
           "and maximum. A call includes the upload of its scalars or candidates from pageable host memory and the allocation of the new key; the "
           "handle is freed outside the timed region. One MI355X, one process, all figures from one run. Shader clock read by "
           f"`gm_prof_read_clock` in this process: **{get('shader_clock')['mhz']} MHz**. Scalars are uniform below 2^254; candidates are uniformly "
           "random bytes, 4 n + 64 of them for n points.", "", "## Times", "", "Median ms (min – max).", "",
           "| | " + " | ".join(f"2^{lg} points" for lg in a.logn) + " |", "|---|" + "---|" * len(a.logn)]
    for what in ("gm_g2_fixed_base_register", "gm_g2_srs_register", "gm_g1_bases_from_candidates", "gm_g2_bases_from_candidates", "gm_g2_bases_check"):
        out.append(f"| `{what}`" + (" (yardstick)" if what.endswith("check") else "") + " | " + " | ".join(ms(get(what, lg)) for lg in a.logn) + " |")
    f = get("gm_crs_fold")
    out += ["", f"`gm_crs_fold` at 2^{f['logn']} points of each group (2^{f['logn'] - 1} outputs): {ms(f)} ms.", "", "## Against the yardsticks", "",
            "Each kernel's Fq-product count, read off its loops (the constants at the top of the tool), at the rate `gm_g2_bases_check` "
            f"({P_CHECK_G2} products a point) and the accumulation of a G2 MSM (`k_g2_acc`, {P_MADD_G2} products an entry) reach in the same process.", "",
            "| | " + " | ".join(f"2^{lg}" for lg in a.logn) + " |", "|---|" + "---|" * len(a.logn)]
    rate = {lg: (get("gm_g2_bases_check", lg)["rate_gproducts_s"], get("k_g2_acc", lg)["rate_gproducts_s"]) for lg in a.logn}
    out.append("| rate of `gm_g2_bases_check`, 10^9 Fq products / s | " + " | ".join(str(rate[lg][0]) for lg in a.logn) + " |")
    out.append("| rate of `k_g2_acc` | " + " | ".join(str(rate[lg][1]) for lg in a.logn) + " |")

    def line(name, what, products):
        cells = []
        for lg in a.logn:
            r, n = get(what, lg), 1 << lg
            p = products(r) * n
            pred = [p / (x * 1e9) * 1e3 for x in rate[lg]]
            cells.append(f"{p / n:.0f} products a point: predicted {pred[0]:.2f} / {pred[1]:.2f} ms, measured {r['median_ms']} ms, ratio {r['median_ms'] / pred[0]:.2f} / {r['median_ms'] / pred[1]:.2f}")
        out.append(f"| {name} | " + " | ".join(cells) + " |")

    fixed_ms = get("gm_g2_fixed_base_register_one_point")["median_ms"]
    line("`gm_g2_fixed_base_register`", "gm_g2_fixed_base_register", lambda r: P_FIXED_G2)
    line("`gm_g2_srs_register`", "gm_g2_srs_register", lambda r: P_FIXED_G2)
    line("`gm_g1_bases_from_candidates`", "gm_g1_bases_from_candidates", lambda r: r["read_per_point"] * P_ROOT_G1 + P_CLEAR_G1 * _cleared(r, 1) + P_NORM_G1)
    line("`gm_g2_bases_from_candidates`", "gm_g2_bases_from_candidates", lambda r: r["read_per_point"] * P_ROOT_G2 + P_CLEAR_G2 * _cleared(r, 2) + P_NORM_G2)
    py = get("python_g2_mul")
    out += ["", f"Both fixed-base calls carry a cost that does not depend on n: the table of 32 x 256 multiples, whose last window is a chain of 248 "
            f"doublings in one lane (248 x 24 products at one wave's latency) and one inversion. A call for ONE point takes **{fixed_ms} ms**; the "
            "predictions above are for the n-dependent part only, so the ratio to read is (measured - that) / predicted: "
            + ", ".join(f"2^{lg}: {(get('gm_g2_fixed_base_register', lg)['median_ms'] - fixed_ms) / (P_FIXED_G2 * (1 << lg) / (rate[lg][0] * 1e9) * 1e3):.2f}" for lg in a.logn)
            + " at the check's rate."]
    out += ["", "(predicted at the check's rate / at the accumulation's rate; the G1 rows are set against the same two G2 rates, which is the wrong "
            "yardstick for Fq arithmetic at two waves per SIMD and is given for completeness only.)", "", "## Per produced point", "",
            "| | " + " | ".join(f"2^{lg}" for lg in a.logn) + " |", "|---|" + "---|" * len(a.logn)]
    for g in (1, 2):
        out.append(f"| G{g}: candidates read / square roots / clearings per produced point | "
                   + " | ".join(f"{get(f'gm_g{g}_bases_from_candidates', lg)['read_per_point']} / {get(f'gm_g{g}_bases_from_candidates', lg)['roots_per_point']} / "
                                f"{_cleared(get(f'gm_g{g}_bases_from_candidates', lg), g):.3f}" for lg in a.logn) + " |")
    out += ["", "A candidate with a coordinate >= q costs its lane a compare and one whose x^3 + b is no square the root -- but a wave of the root kernel runs "
            "as long as its slowest lane, and nearly every wave holds a lane that takes the root: the predictions above therefore charge one root per "
            "candidate READ, then one clearing and one normalisation per produced point (the clearing and gather launches have dense lanes). ",
            "The three figures count the candidates [0, used): the call reads its stream in pieces (points.hip: cand_piece, at most 2^20 candidates, "
            "sized so that the last one is expected to finish the key) and has also taken the roots of the candidates of its last piece that lie "
            "behind the n-th survivor -- 64 and about 2 % (G1) or 7 % (G2) of what that piece was asked for; those are not counted here. Of a "
            "piece's curve points only as many as the key still needs are cleared, so the clearings are exactly one per produced point.", "", "## The SRS against Python integers", "",
            f"`gemini_amd.g2.mul`, what `CommitterKey.new` ran per power until now: {py['ms_per_point']} ms a point over {py['points']} points, i.e. "
            + ", ".join(f"{py['ms_per_point'] * (1 << lg) / 1e3:.0f} s for 2^{lg}" for lg in a.logn) + " (scaled, not run) against "
            + ", ".join(f"{get('gm_g2_srs_register', lg)['median_ms']} ms" for lg in a.logn) + " on the device.", "", "## Not measured", "",
            "No counters were collected and no kernel was timed on its own: the ratios compare whole calls with product counts. Sizes above 2^20 "
            "points and slabs (a key above 2^22 points) were not run. `gm_crs_truncate`, `gm_crs_halve` and `gm_crs_to_bases` are device copies and "
            "were not timed.", ""]
    return "\n".join(out)


def _cleared(r, group) -> float:
    """clearings per produced point among the candidates [0, used): the n survivors, exactly"""
    return 1.0


if __name__ == "__main__":
    main()
