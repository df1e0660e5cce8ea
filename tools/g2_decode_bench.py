#!/usr/bin/env python3
"""G2 keys from bytes and keys back to bytes on the device (profiles/g2_decode.md): gm_g2_bases_from_bytes compressed and uncompressed,
with and without validate; gm_g2_bases_check on the same points in the same process (the yardstick that was there before the
decoder); gm_g1_bases_to_bytes and gm_g2_bases_to_bytes.

  call time   host clock around the C call (each ends in a stream synchronise; the status array is not asked for): one warm-up,
              then the median of `--calls` with min and max.  A from_bytes call includes the host-to-device copy of its bytes and
              the registration, a to_bytes call the copy back; the handle a decode hands out is freed outside the timed region
  G2 points   64 members of G2 with known logs, cycled: the cost of decode and check does not depend on the point.  Their bytes
              come from gm_g2_bases_to_bytes (zcash framing for the compressed form, arkworks for the uncompressed one)
  G1 key      gm_g1_srs_register (tau^i g, generated on the device; tables off)

usage: g2_decode_bench.py [--logn 16 20] [--calls 5] [--out FILE]
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
from gemini_amd.kzg import g1_generator_mont  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import g2_ref  # noqa: E402
from tests import points_ref as pr  # noqa: E402

TAU = 0x2F4E6D8C0B1A39587766554433221100FFEEDDCCBBAA9988776655443322110F % pr.R


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    gm.capi.init()
    lib = gm.capi.load()
    gm.capi.check(lib.gm_set_auto_tables(C.c_int(0)))
    orc.build()
    base = np.array([pr.g2_record(p) for p in g2_ref.chain(64)], dtype=np.uint64)
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    for logn in args.logn:
        n = 1 << logn
        reg = gm.G2Bases.register(np.tile(base, (n // 64, 1)))
        ok, fb = C.c_int(0), C.c_size_t(0)

        def check():
            gm.capi.check(lib.gm_g2_bases_check(C.c_uint64(reg.handle), C.c_size_t(0), C.c_size_t(n), None, C.byref(fb), C.byref(ok)))
            assert ok.value == 1

        emit(what="gm_g2_bases_check", logn=logn, **timed(check, args.calls))
        for compressed, enc in ((True, 1), (False, 0)):
            out = np.zeros(n * (96 if compressed else 192), dtype=np.uint8)

            def encode():
                gm.capi.check(lib.gm_g2_bases_to_bytes(C.c_uint64(reg.handle), C.c_size_t(0), C.c_size_t(n), C.c_int(int(compressed)), C.c_int(enc), gm.capi.ptr(out),
                                                       C.c_size_t(len(out))))

            emit(what="gm_g2_bases_to_bytes", logn=logn, compressed=compressed, encoding=enc, **timed(encode, args.calls))
            for validate in (True, False):
                h = C.c_uint64(0)

                def decode():
                    gm.capi.check(lib.gm_g2_bases_from_bytes(gm.capi.ptr(out), C.c_size_t(n), C.c_int(int(compressed)), C.c_int(enc), C.c_int(int(validate)), C.byref(h),
                                                             None, C.byref(fb), C.byref(ok)))
                    assert ok.value == 1 and h.value
                    return h.value

                def free(handle):
                    gm.capi.check(lib.gm_g2_bases_free(C.c_uint64(handle)))

                emit(what="gm_g2_bases_from_bytes", logn=logn, compressed=compressed, encoding=enc, validate=validate, **timed(decode, args.calls, free))
        reg.free()
        key = gm.G1Bases.srs(g1_generator_mont(), orc.ints_to_limbs([TAU], 4)[0], n)
        for compressed in (True, False):
            out = np.zeros(n * (48 if compressed else 96), dtype=np.uint8)

            def encode1():
                gm.capi.check(lib.gm_g1_bases_to_bytes(C.c_uint64(key.handle), C.c_size_t(0), C.c_size_t(n), C.c_int(int(compressed)), C.c_int(0), gm.capi.ptr(out),
                                                       C.c_size_t(len(out))))

            emit(what="gm_g1_bases_to_bytes", logn=logn, compressed=compressed, encoding=0, **timed(encode1, args.calls))
        key.free()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
