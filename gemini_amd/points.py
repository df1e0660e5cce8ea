"""Host mirror of the point-validation block of include/gemini_hip.h (gemini_amd/csrc/points.hip): untrusted G1 / G2 points and a
committer key checked -- and G1 byte encodings decoded -- on the device.

What `CanonicalDeserialize::deserialize_with_mode(.., Validate::Yes)` of ark-ec does per point, for whole keys: gemini_amd/wire.py
states the same on Python integers, one point at a time, which suits the O(log n) points of a proof and not a 2^26-point key.
Every call returns a `CheckResult`; a bad point is a result, not an exception (exceptions are for misuse, as everywhere here).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import enum
import secrets

import numpy as np

from . import capi
from .fr import R_MOD, fr_from_int
from .g2msm import G2Bases
from .msm import G1Bases


class PointStatus(enum.IntEnum):
    """GM_PT_*: the FIRST check of a point that fails, in this order"""
    OK = 0
    BAD_ENCODING = 1
    NONCANONICAL = 2
    NOT_ON_CURVE = 3
    NOT_IN_SUBGROUP = 4


# wire.g1_deserialize(strict=True) raises WireError with one of these messages for a point it rejects; the device reports the status
# on the right (tests/test_points_cpu.py checks the table against wire.py's source).  "not enough bytes" is the caller's length check.
WIRE_ERROR_STATUS = {
    "G1 flags: infinity together with the y sign": PointStatus.BAD_ENCODING,
    "G1 compression flag does not match the requested mode": PointStatus.BAD_ENCODING,
    "G1 flags: unexpected sort flag": PointStatus.BAD_ENCODING,
    "G1 point at infinity with non-zero coordinates": PointStatus.BAD_ENCODING,
    "G1 y-sign flag does not match y": PointStatus.BAD_ENCODING,
    "G1 coordinate is not a canonical field element": PointStatus.NONCANONICAL,
    "G1 x coordinate is not on the curve": PointStatus.NOT_ON_CURVE,
    "G1 point is not on the curve": PointStatus.NOT_ON_CURVE,
    "G1 point is not in the prime-order subgroup": PointStatus.NOT_IN_SUBGROUP,
}


@dataclasses.dataclass
class CheckResult:
    ok: bool
    first_bad: int          # the smallest bad index; n when every point passes
    status: np.ndarray      # (n,) uint8 of PointStatus values

    def __bool__(self):
        return self.ok


def _run(fn, n: int, *args) -> CheckResult:
    status = np.zeros(n, dtype=np.uint8)
    first_bad, ok = C.c_size_t(0), C.c_int(0)
    capi.check(fn(*args, C.c_size_t(n), capi.ptr(status), C.byref(first_bad), C.byref(ok)))
    return CheckResult(bool(ok.value), first_bad.value, status)


def _records(records, limbs: int) -> np.ndarray:
    records = capi.u64(records)
    assert records.ndim == 2 and records.shape[1] in (limbs, limbs + 1), f"records of {limbs} or {limbs + 1} limbs"
    return records


def check_g1(records) -> CheckResult:
    """gm_g1_check: host records as G1Bases.register takes them, (n, 12) or (n, 13) with the infinity byte"""
    capi.ensure_init()
    r = _records(records, 12)
    return _run(capi.load().gm_g1_check, len(r), capi.ptr(r), C.c_size_t(r.shape[1] * 8))


def check_g2(records) -> CheckResult:
    """gm_g2_check: host records as G2Bases.register takes them, (n, 24) or (n, 25)"""
    capi.ensure_init()
    r = _records(records, 24)
    return _run(capi.load().gm_g2_check, len(r), capi.ptr(r), C.c_size_t(r.shape[1] * 8))


def check_g1_bases(bases: G1Bases, offset: int = 0, n: int | None = None) -> CheckResult:
    """gm_g1_bases_check over bases[offset : offset + n] (G1Bases.check)"""
    n = len(bases) - offset if n is None else n
    return _run(capi.load().gm_g1_bases_check, n, C.c_uint64(bases.handle), C.c_size_t(offset))


def check_g2_bases(bases: G2Bases, offset: int = 0, n: int | None = None) -> CheckResult:
    """gm_g2_bases_check over bases[offset : offset + n] (G2Bases.check)"""
    n = len(bases) - offset if n is None else n
    return _run(capi.load().gm_g2_bases_check, n, C.c_uint64(bases.handle), C.c_size_t(offset))


def g1_bases_from_bytes(data: bytes, n: int, compress: bool, enc: int = 0, validate: bool = True):
    """gm_g1_bases_from_bytes: n points of 48 (compress) or 96 bytes, framing `enc` (wire.G1Encoding), decoded -- and with
    `validate` checked -- on the device.  Returns (G1Bases or None, CheckResult): acceptance is that of
    wire.g1_deserialize(strict=True, validate=validate) point for point, and nothing stays registered when a point is rejected."""
    capi.ensure_init()
    size = 48 if compress else 96
    assert len(data) == n * size, f"{len(data)} bytes for {n} points of {size}"
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    status = np.zeros(n, dtype=np.uint8)
    h, first_bad, ok = C.c_uint64(0), C.c_size_t(0), C.c_int(0)
    capi.check(capi.load().gm_g1_bases_from_bytes(capi.ptr(buf), C.c_size_t(n), C.c_int(int(bool(compress))), C.c_int(int(enc)), C.c_int(int(bool(validate))),
                                                  C.byref(h), capi.ptr(status), C.byref(first_bad), C.byref(ok)))
    res = CheckResult(bool(ok.value), first_bad.value, status)
    assert (h.value != 0) == res.ok, "gm_g1_bases_from_bytes: a handle exactly when every point was accepted"
    return (G1Bases(h.value, n) if res.ok else None), res


def _g2_record(p) -> np.ndarray:
    """a 24-limb record, or an affine point of gemini_amd.g2"""
    if isinstance(p, tuple):
        from .kzg import g2_records

        return g2_records([p])[0]
    return capi.u64(p).reshape(24)


def check_powers(bases: G1Bases, g2, tau_g2, rho=None, offset: int = 0, n: int | None = None) -> bool:
    """gm_g1_powers_check: bases[offset + i + 1] = tau bases[offset + i] for the tau of (g2, tau_g2).  rho (an integer) is drawn with
    `secrets` when it is not given: it must be unpredictable to whoever made the key.  The points are taken as members of their
    groups -- run `bases.check()` first."""
    n = len(bases) - offset if n is None else n
    if rho is None:
        rho = 1 + secrets.randbelow(R_MOD - 1)
    ok = C.c_int(0)
    capi.check(capi.load().gm_g1_powers_check(C.c_uint64(bases.handle), C.c_size_t(offset), C.c_size_t(n), capi.ptr(_g2_record(g2)), capi.ptr(_g2_record(tau_g2)),
                                              capi.ptr(fr_from_int(int(rho) % R_MOD)), C.byref(ok)))
    return bool(ok.value)
