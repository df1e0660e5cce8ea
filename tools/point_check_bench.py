#!/usr/bin/env python3
"""Point validation on the device (profiles/point_check.md): gm_g1_bases_check, gm_g1_bases_from_bytes (compressed, validate on),
gm_g2_bases_check and gm_g1_powers_check at the sizes of a committer key, and the same G1 check on the host.

  call time   host clock around the C call (it ends in a stream synchronise and hands back ok / first_bad; the status array is not
              asked for, so only the per-block summaries cross): one warm-up, then the median of `--calls` with min and max
  clock       gm_prof_read_clock after a small G1 MSM under the profiler: the shader clock the library measured
  host        tools/point_check_host.cpp, built here with g++ -O3: the same check on gmh:: (host_field.hpp), one thread, 2^12 points
  keys        gm_g1_srs_register (tau^i g, generated on the device; tables off); their compressed bytes are made here from the
              downloaded records (arkworks framing: canonical little-endian x, the y-sign flag in bit 7 of the last byte)
  G2 points   64 points with known logs, cycled: the cost of the check does not depend on the point

usage: point_check_bench.py [--g1-logn 20 24] [--g2-logn 16 20] [--calls 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gemini_amd as gm  # noqa: E402
from gemini_amd.fr import fr_from_int  # noqa: E402
from gemini_amd.kzg import VerifierKey, g1_generator_mont, g2_records  # noqa: E402
from gemini_amd import g2 as G2  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import g2_ref  # noqa: E402
from tests import points_ref as pr  # noqa: E402

TAU = 0x2F4E6D8C0B1A39587766554433221100FFEEDDCCBBAA9988776655443322110F % pr.R
HALF_Q = (pr.Q - 1) // 2


def timed(fn, calls):
    fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3)}


def shader_mhz(lib):
    from tests.util import rand_bases

    gm.capi.check(lib.gm_prof_enable(C.c_int(1)))
    gm.VariableBaseMSM.msm_bigint(rand_bases(orc, 1, 1 << 14), orc.random_fr(2, 1 << 14))
    mhz = C.c_double()
    gm.capi.check(lib.gm_prof_read_clock(C.byref(mhz)))
    gm.capi.check(lib.gm_prof_enable(C.c_int(0)))
    return round(mhz.value, 1)


def compressed_bytes(records: np.ndarray) -> np.ndarray:
    """(n, 12) Montgomery records of non-identity points -> n x 48 bytes, arkworks framing"""
    n = len(records)
    canon = orc.fq_from_mont(np.ascontiguousarray(records.reshape(2 * n, 6))).reshape(n, 2, 6)
    half = np.array([(HALF_Q >> (64 * i)) & (2**64 - 1) for i in range(6)], dtype=np.uint64)
    y = canon[:, 1, :]
    larger = np.zeros(n, dtype=bool)
    decided = np.zeros(n, dtype=bool)
    for k in range(5, -1, -1):  # y > (q - 1) / 2, most significant limb first
        gt, lt = (y[:, k] > half[k]) & ~decided, (y[:, k] < half[k]) & ~decided
        larger |= gt
        decided |= gt | lt
    out = np.ascontiguousarray(canon[:, 0, :]).view(np.uint8).reshape(n, 48).copy()
    out[larger, 47] |= 0x80
    return out


def host_check(records: np.ndarray):
    with tempfile.TemporaryDirectory() as tmp:  # nothing is built into the tree
        exe, path = os.path.join(tmp, "point_check_host"), os.path.join(tmp, "in.bin")
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-march=native", "-I", os.path.join(ROOT, "gemini_amd", "csrc"),
                               os.path.join(ROOT, "tools", "point_check_host.cpp"), "-o", exe])
        with open(path, "wb") as fh:
            fh.write(struct.pack("<Q", len(records)))
            fh.write(struct.pack("<6Q", *pr.fq_limbs(pr.fq_mont(pr.BETA))))
            fh.write(np.ascontiguousarray(records).tobytes())
        best = None
        for _ in range(3):
            passed, ms = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.split()
            assert int(passed) == len(records)
            best = float(ms) if best is None else min(best, float(ms))
        return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g1-logn", type=int, nargs="*", default=[20, 24])
    ap.add_argument("--g2-logn", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    gm.capi.init(0)
    lib = gm.capi.load()
    gm.capi.check(lib.gm_set_auto_tables(C.c_int(0), C.c_size_t(0)))
    out = open(a.out, "w") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    emit({"what": "clock", "shader_mhz": shader_mhz(lib)})
    tau = orc.ints_to_limbs([TAU], 4)[0]
    vk = VerifierKey.from_trapdoor(tau, 1)
    raw = vk.powers_of_g2_bytes(enc=0)
    vk.free()
    g2p = g2_records([G2.deserialize_uncompressed(raw[8 + 192 * i: 8 + 192 * (i + 1)], 0) for i in range(2)])
    rho = fr_from_int(0x6A09E667F3BCC908B2FB1366EA957D3E3ADEC17512775099DA2F590B0667322A)
    fb, ok, h = C.c_size_t(0), C.c_int(0), C.c_uint64(0)

    for logn in a.g1_logn:
        n = 1 << logn
        key = gm.G1Bases.srs(g1_generator_mont(), tau, n)

        def bases_check():
            gm.capi.check(lib.gm_g1_bases_check(C.c_uint64(key.handle), C.c_size_t(0), C.c_size_t(n), None, C.byref(fb), C.byref(ok)))
            assert ok.value == 1 and fb.value == n

        t = timed(bases_check, a.calls)
        emit({"what": "gm_g1_bases_check", "logn": logn, **t, "mpoints_per_s": round(n / t["median_ms"] / 1e3, 2)})

        def powers():
            gm.capi.check(lib.gm_g1_powers_check(C.c_uint64(key.handle), C.c_size_t(0), C.c_size_t(n), gm.capi.ptr(g2p[0]), gm.capi.ptr(g2p[1]), gm.capi.ptr(rho),
                                                 C.byref(ok)))
            assert ok.value == 1

        emit({"what": "gm_g1_powers_check", "logn": logn, **timed(powers, a.calls)})
        rec = key.download()
        if logn == min(a.g1_logn):
            m = 1 << 12
            dev = timed(lambda: gm.capi.check(lib.gm_g1_check(gm.capi.ptr(rec[:m]), C.c_size_t(96), C.c_size_t(m), None, C.byref(fb), C.byref(ok))), a.calls)
            host_ms = host_check(rec[:m])
            emit({"what": "host_vs_device", "points": m, "host_one_thread_ms": round(host_ms, 2), "gm_g1_check_ms": dev["median_ms"],
                  "device_at_key_size_us_per_point": round(t["median_ms"] * 1e3 / n, 4), "host_us_per_point": round(host_ms * 1e3 / m, 2)})
        key.free()
        data = compressed_bytes(rec)
        del rec

        def from_bytes():
            gm.capi.check(lib.gm_g1_bases_from_bytes(gm.capi.ptr(data), C.c_size_t(n), C.c_int(1), C.c_int(0), C.c_int(1), C.byref(h), None, C.byref(fb), C.byref(ok)))
            assert ok.value == 1 and fb.value == n and h.value
            gm.capi.check(lib.gm_g1_bases_free(h))

        t = timed(from_bytes, a.calls)
        emit({"what": "gm_g1_bases_from_bytes compressed validate", "logn": logn, **t, "mpoints_per_s": round(n / t["median_ms"] / 1e3, 2)})
        del data

    pts = g2_records(list(g2_ref.chain(64)))
    for logn in a.g2_logn:
        n = 1 << logn
        reg = gm.G2Bases.register(pts[np.arange(n) % 64])

        def g2_check():
            gm.capi.check(lib.gm_g2_bases_check(C.c_uint64(reg.handle), C.c_size_t(0), C.c_size_t(n), None, C.byref(fb), C.byref(ok)))
            assert ok.value == 1 and fb.value == n

        t = timed(g2_check, a.calls)
        emit({"what": "gm_g2_bases_check", "logn": logn, **t, "mpoints_per_s": round(n / t["median_ms"] / 1e3, 2)})
        reg.free()


if __name__ == "__main__":
    main()
