"""Host mirror of the point-validation block of include/gemini_hip.h (gemini_amd/csrc/points.hip): untrusted G1 / G2 points and a
committer key checked, G1 and G2 byte encodings decoded and resident keys encoded on the device, and the check entries of what a
verifier consumes (a CRS, a verifier key, the group elements of a proof).

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


# ---- G2 keys from bytes, keys back to bytes, and the checks of what a verifier consumes ----------------------------------------------
def g2_bases_from_bytes(data: bytes, n: int, compress: bool, enc: int = 0, validate: bool = True):
    """gm_g2_bases_from_bytes: n points of 96 (compress) or 192 bytes, decoded -- and with `validate` checked -- on the device.
    Returns (G2Bases or None, CheckResult): acceptance is that of g2.deserialize(strict=True, validate=validate) point for point."""
    capi.ensure_init()
    size = 96 if compress else 192
    assert len(data) == n * size, f"{len(data)} bytes for {n} points of {size}"
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    status = np.zeros(n, dtype=np.uint8)
    h, first_bad, ok = C.c_uint64(0), C.c_size_t(0), C.c_int(0)
    capi.check(capi.load().gm_g2_bases_from_bytes(capi.ptr(buf), C.c_size_t(n), C.c_int(int(bool(compress))), C.c_int(int(enc)), C.c_int(int(bool(validate))),
                                                  C.byref(h), capi.ptr(status), C.byref(first_bad), C.byref(ok)))
    res = CheckResult(bool(ok.value), first_bad.value, status)
    assert (h.value != 0) == res.ok, "gm_g2_bases_from_bytes: a handle exactly when every point was accepted"
    return (G2Bases(h.value, n) if res.ok else None), res


# ---- points without a known logarithm ------------------------------------------------------------------------------------------------
CANDIDATE_BYTES = {1: 48, 2: 96}
CANDIDATE_DOMAIN = b"gemini_amd candidates v1"


def bases_from_candidates(group: int, cand: bytes, n: int):
    """gm_g1_bases_from_candidates / gm_g2_bases_from_candidates: `cand` holds m candidates of 48 (G1: x and, in bit 383, the choice
    of y) or 96 bytes (G2: x.c0 | x.c1); the first n whose x is < q and on the curve and whose cofactor-cleared point is not the
    identity are registered, in candidate order.  -> (G1Bases / G2Bases, or None on a shortfall; used; found): `used` is the index
    after the n-th survivor (m on a shortfall), `found` the survivors among the candidates before it."""
    capi.ensure_init()
    size = CANDIDATE_BYTES[group]
    assert len(cand) % size == 0, f"{len(cand)} bytes are no whole number of {size}-byte candidates"
    m = len(cand) // size
    buf = np.frombuffer(bytes(cand), dtype=np.uint8)
    h, used, found = C.c_uint64(0), C.c_size_t(0), C.c_size_t(0)
    fn = capi.load().gm_g1_bases_from_candidates if group == 1 else capi.load().gm_g2_bases_from_candidates
    capi.check(fn(capi.ptr(buf) if m else None, C.c_size_t(m), C.c_size_t(n), C.byref(h), C.byref(used), C.byref(found)))
    assert (h.value != 0) == (found.value >= n), "from_candidates: a handle exactly when n candidates survived"
    return ((G1Bases if group == 1 else G2Bases)(h.value, n) if h.value else None), used.value, found.value


def candidate_stream(seed: bytes, group: int, start: int, count: int) -> bytes:
    """candidates [start, start + count) of the stream of (seed, group): SHAKE-256 over the domain string, the group byte and the
    seed, cut into 48- / 96-byte candidates.  This stream is this package's own convention: NO parity with the draws of an
    arkworks `rand` is claimed (README, "Unpinned conventions")."""
    import hashlib

    size = CANDIDATE_BYTES[group]
    return hashlib.shake_256(CANDIDATE_DOMAIN + bytes([group]) + bytes(seed)).digest((start + count) * size)[start * size:]


def bases_from_seed(group: int, seed: bytes, n: int):
    """n points of G1 / G2 whose logarithms nobody knows, from the candidate stream of `seed`: 4 n + 64 candidates first (about
    half of all x are on the curve), and the same stream continued from `used` on a shortfall"""
    if n == 0:
        return bases_from_candidates(group, b"", 0)[0]
    parts, start, count = [], 0, 4 * n + 64
    try:
        while True:
            got = sum(len(p) for p in parts)
            b, used, found = bases_from_candidates(group, candidate_stream(seed, group, start, count), n - got)
            if b is not None:
                parts.append(b)
                break
            if found:  # keep what this stretch gave: the survivors of [start, start + count), all of them
                part, _, _ = bases_from_candidates(group, candidate_stream(seed, group, start, count), found)
                parts.append(part)
            start += used
        if len(parts) == 1:
            return parts.pop()
        rec = np.concatenate([p.download() for p in parts])  # (a shortfall of 4 n + 64 candidates has probability ~2^-n: not a hot path)
        return (G1Bases if group == 1 else G2Bases).register(rec)
    finally:
        for p in parts:
            p.free()


def _to_bytes(fn, handle: int, size: int, compress: bool, offset: int, n: int, enc: int) -> bytes:
    out = np.zeros(n * size, dtype=np.uint8)
    capi.check(fn(C.c_uint64(handle), C.c_size_t(offset), C.c_size_t(n), C.c_int(int(bool(compress))), C.c_int(int(enc)), capi.ptr(out) if n else None,
                  C.c_size_t(len(out))))
    return out.tobytes()


def g1_bases_to_bytes(bases: G1Bases, compress: bool, enc: int = 0, offset: int = 0, n: int | None = None) -> bytes:
    """gm_g1_bases_to_bytes: bases[offset : offset + n] as n x 48 / 96 bytes, what wire.g1_serialize writes point by point"""
    n = len(bases) - offset if n is None else n
    return _to_bytes(capi.load().gm_g1_bases_to_bytes, bases.handle, 48 if compress else 96, compress, offset, n, enc)


def g2_bases_to_bytes(bases: G2Bases, compress: bool, enc: int = 0, offset: int = 0, n: int | None = None) -> bytes:
    """gm_g2_bases_to_bytes: n x 96 / 192 bytes, what g2.serialize_compressed / serialize_uncompressed write point by point"""
    n = len(bases) - offset if n is None else n
    return _to_bytes(capi.load().gm_g2_bases_to_bytes, bases.handle, 96 if compress else 192, compress, offset, n, enc)


@dataclasses.dataclass
class KeyCheckResult:
    ok: bool
    first_bad_g1: int       # the smallest bad index of each group; its length when every point passes
    first_bad_g2: int

    def __bool__(self):
        return self.ok


def _key_check(fn, handle: int) -> KeyCheckResult:
    b1, b2, ok = C.c_size_t(0), C.c_size_t(0), C.c_int(0)
    capi.check(fn(C.c_uint64(handle), C.byref(b1), C.byref(b2), C.byref(ok)))
    return KeyCheckResult(bool(ok.value), b1.value, b2.value)


def check_crs(crs) -> KeyCheckResult:
    """gm_crs_check: curve and subgroup over both arrays of an ipa.Crs"""
    return _key_check(capi.load().gm_crs_check, crs.handle)


def check_vk(vk) -> KeyCheckResult:
    """gm_vk_check: canonical limbs, curve and subgroup over both arrays of a kzg.VerifierKey"""
    return _key_check(capi.load().gm_vk_check, vk.handle)


@dataclasses.dataclass
class ProofCheckResult:
    ok: bool
    first_bad: int          # in the order include/gemini_hip.h lists the elements; their number when every one passes

    def __bool__(self):
        return self.ok


def check_proof(fn, proof_arg) -> ProofCheckResult:
    """gm_snark_proof_check / gm_psnark_proof_check (a byref to the packed record) / gm_ipa_check (the handle)"""
    fb, ok = C.c_size_t(0), C.c_int(0)
    capi.check(fn(proof_arg, C.byref(fb), C.byref(ok)))
    return ProofCheckResult(bool(ok.value), fb.value)


def debug_fq2_sqrt(a_mont):
    """gm_debug_fq2_sqrt: (n, 12) ark-ff Montgomery limbs (c0 | c1) -> (roots (n, 12), is_square (n,) uint8)"""
    capi.ensure_init()
    a = capi.u64(a_mont).reshape(-1, 12)
    root, sq = np.zeros_like(a), np.zeros(len(a), dtype=np.uint8)
    capi.check(capi.load().gm_debug_fq2_sqrt(capi.ptr(a), C.c_size_t(len(a)), capi.ptr(root), capi.ptr(sq)))
    return root, sq
