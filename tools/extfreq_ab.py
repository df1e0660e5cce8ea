"""A/B of the two routes to extend_frequency(compute_frequency(set_len, index)) (plookup/time_prover.rs:65-78), in ONE process, alternating:

  (a) host:   numpy compute_frequency + extend_frequency (gemini_amd.psnark) + the gm_idx_register upload -- host clock, the upload ends in a
              device synchronise
  (b) device: gm_idx_extend_frequency on the resident index -- HIP events on the library's stream around its kernels (profiler stage 7), and
              the host clock around the whole call

Sizes: k in {2^20, 2^24, 2^26} with set_len = k / 4, and k = 2^24 with set_len = 7; index uniform and all-equal.  Both routes must produce the
same vector at every size timed.  Needs a GPU (fails without one).  Writes a markdown table to --out (default profiles/extfreq_ab.md).

  python tools/extfreq_ab.py [--reps 21] [--warmup 3] [--sizes 20,24,26] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gemini_amd as gm  # noqa: E402
from gemini_amd.fr import IdxVec  # noqa: E402
from gemini_amd.plookup import extend_frequency_device  # noqa: E402
from gemini_amd.psnark import compute_frequency, extend_frequency  # noqa: E402

EXTFREQ_STAGE = 7  # include/gemini_hip.h: gm_prof_read


def shader_clock_mhz(lib) -> float:
    """the clock line of the other profiles/ tables: read inside k_acc0 of three 2^20 MSMs"""
    from gemini_amd.kzg import g1_generator_mont

    n = 1 << 20
    sc = np.random.default_rng(1).integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)  # (top limb below the modulus')
    bases = gm.G1Bases.fixed_base(g1_generator_mont(), sc)
    v = gm.FrVec.from_host(sc)
    out = np.zeros(18, dtype=np.uint64)
    gm.capi.check(lib.gm_prof_enable(C.c_int(1)))
    for _ in range(3):
        gm.capi.check(lib.gm_g1_msm_v(C.c_uint64(bases.handle), C.c_size_t(0), C.c_int(0), C.c_uint64(v.handle), C.c_size_t(0), C.c_size_t(n), gm.capi.ptr(out)))
    mhz = C.c_double(0.0)
    gm.capi.check(lib.gm_prof_read_clock(C.byref(mhz)))
    gm.capi.check(lib.gm_prof_enable(C.c_int(0)))
    v.free()
    bases.free()
    return mhz.value


def host_route(index: np.ndarray, set_len: int) -> IdxVec:
    return IdxVec.from_host(extend_frequency(compute_frequency(set_len, index)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="20,24,26")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "extfreq_ab.md"))
    args = ap.parse_args()
    assert args.reps >= 20, "the median is taken over at least 20 timed calls"
    gm.capi.init(0)
    lib = gm.capi.load()
    cases = [(1 << lg, (1 << lg) // 4) for lg in (int(x) for x in args.sizes.split(","))]
    if (1 << 24, 1 << 22) in cases:
        cases.append((1 << 24, 7))
    rows = []
    for k, set_len in cases:
        for dist in ("uniform", "all-equal"):
            index = (np.random.default_rng(k + set_len).integers(0, set_len, size=k).astype(np.uint32) if dist == "uniform"
                     else np.full(k, set_len // 2, dtype=np.uint32))
            didx = IdxVec.from_host(index)
            a, b = host_route(index, set_len), extend_frequency_device(didx, set_len)
            same = np.array_equal(a.to_host(), b.to_host())
            a.free()
            b.free()
            assert same, f"the two routes differ at k = {k}, set_len = {set_len}, {dist}"
            t_host, t_dev_wall, t_dev_events = [], [], []
            for it in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                a = host_route(index, set_len)  # gm_idx_register waits for its copy
                ta = time.perf_counter() - t0
                a.free()
                gm.capi.check(lib.gm_prof_enable(C.c_int(1)))
                t0 = time.perf_counter()
                b = extend_frequency_device(didx, set_len)  # waits for the range-check flag
                tb = time.perf_counter() - t0
                ms = (C.c_double * 8)()
                cnt = (C.c_uint64 * 8)()
                gm.capi.check(lib.gm_prof_read(ms, cnt, C.c_int(8)))
                gm.capi.check(lib.gm_prof_enable(C.c_int(0)))
                b.free()
                if it >= args.warmup:
                    t_host.append(ta * 1e3)
                    t_dev_wall.append(tb * 1e3)
                    t_dev_events.append(ms[EXTFREQ_STAGE] / max(cnt[EXTFREQ_STAGE], 1))
            didx.free()
            med = statistics.median
            rows.append((k, set_len, dist, med(t_host), med(t_dev_wall), med(t_dev_events), min(t_host), min(t_dev_wall)))
            print(f"k=2^{k.bit_length() - 1} set_len={set_len} {dist}: host {med(t_host):.3f} ms, device {med(t_dev_wall):.3f} ms wall / "
                  f"{med(t_dev_events):.3f} ms events", flush=True)
    mhz = shader_clock_mhz(lib)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("# extend_frequency: host route (numpy + upload) vs gm_idx_extend_frequency, same process, alternating\n\n")
        fh.write(f"{time.strftime('%Y-%m-%d')}; median of {args.reps} timed calls after {args.warmup} warm-up calls; shader clock read inside k_acc0 on this box: "
                 f"{mhz:.1f} MHz; both routes gave equal vectors at every size.\n\n")
        fh.write("| k | set_len | index | host route ms (median) | device call ms, host clock (median) | device kernels ms, HIP events (median) | host / device call | "
                 "host min ms | device call min ms |\n|---|---|---|---|---|---|---|---|---|\n")
        for k, set_len, dist, th, tw, te, mh, mw in rows:
            fh.write(f"| 2^{k.bit_length() - 1} | {set_len} | {dist} | {th:.3f} | {tw:.3f} | {te:.3f} | {th / tw:.1f}x | {mh:.3f} | {mw:.3f} |\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
