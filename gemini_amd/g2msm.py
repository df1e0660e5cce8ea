"""Host mirror of the G2 MSM surface herring uses: `P::G2::msm_unchecked` behind Crs::commit_g2 / CrsStream::commit_g2
(src/herring/ipa.rs:107-118,185-189) and G2Module::ip (src/herring/module.rs:114-124).  All arithmetic happens in
libgemini_hip.so (gm_g2_*); gemini_amd/g2.py stays what it was, Python integers for a handful of setup points.

Data conventions (numpy uint64): affine bases (n, 24) Montgomery x.c0 | x.c1 | y.c0 | y.c1 with the all-zero row = identity, or
(n, 25) with column 24 = ark-ec's `infinity` flag word (stride 200, the Rust layout); scalars (n, 4) as in gemini_amd.msm;
results (36,) Jacobian X, Y, Z over Fq2 (c0 before c1), Montgomery, normalised.  The integer side is the layout of
gemini_amd/g2.py: a point is ((x0, x1), (y0, y1)) or None.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .g2 import Q

_R384 = 1 << 384


def _fq_limbs(v: int) -> list:
    v = v * _R384 % Q
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]


def _fq_int(limbs) -> int:
    v = 0
    for i, w in enumerate(limbs):
        v |= int(w) << (64 * i)
    return v * pow(_R384, -1, Q) % Q


def g2_points_to_affine(points, flag: bool = False) -> np.ndarray:
    """[((x0, x1), (y0, y1)) | None] -> (n, 24) records, or (n, 25) with the infinity word when `flag`"""
    out = np.zeros((len(points), 25 if flag else 24), dtype=np.uint64)
    for i, p in enumerate(points):
        if p is None:
            if flag:
                out[i, 24] = 1
            continue
        (x0, x1), (y0, y1) = p
        out[i, :24] = _fq_limbs(x0) + _fq_limbs(x1) + _fq_limbs(y0) + _fq_limbs(y1)
    return out


def g2_affine_to_points(records) -> list:
    """(n, 24) / (n, 25) records -> [((x0, x1), (y0, y1)) | None]"""
    rec = capi.u64(records)
    rec = rec.reshape(-1, rec.shape[-1])
    out = []
    for row in rec:
        if (rec.shape[1] == 25 and row[24]) or not row[:24].any():
            out.append(None)
            continue
        v = [_fq_int(row[6 * k: 6 * k + 6]) for k in range(4)]
        out.append(((v[0], v[1]), (v[2], v[3])))
    return out


def g2_point_to_jac(p) -> np.ndarray:
    """((x0, x1), (y0, y1)) | None -> (36,) normalised Jacobian"""
    out = np.zeros(36, dtype=np.uint64)
    one = _fq_limbs(1)
    if p is None:
        out[0:6] = one
        out[12:18] = one
        return out
    out[:24] = g2_points_to_affine([p])[0]
    out[24:30] = one
    return out


def g2_jac_to_point(jac):
    """(36,) Jacobian, normalised or not -> ((x0, x1), (y0, y1)) | None, canonical integers"""
    from . import g2

    j = capi.u64(jac).reshape(6, 6)
    X, Y, Z = ((_fq_int(j[2 * k]), _fq_int(j[2 * k + 1])) for k in range(3))
    if Z == (0, 0):
        return None
    zi = g2.f2_inv(Z)
    zi2 = g2.f2_mul(zi, zi)
    return (g2.f2_mul(X, zi2), g2.f2_mul(Y, g2.f2_mul(zi2, zi)))


def g2_sum(points: np.ndarray) -> np.ndarray:
    """normalise(sum of Jacobian points) on the host (gm_g2_sum; no GPU needed)"""
    pts = capi.u64(points).reshape(-1, 36)
    out = np.empty(36, dtype=np.uint64)
    capi.check(capi.load().gm_g2_sum(capi.ptr(pts), C.c_size_t(len(pts)), capi.ptr(out)))
    return out


def _records(bases) -> np.ndarray:
    bases = capi.u64(bases)
    assert bases.ndim == 2 and bases.shape[1] in (24, 25)
    return bases


def g2_lincomb_many(points: np.ndarray, scalars_canonical: np.ndarray, offsets) -> np.ndarray:
    """gm_g2_lincomb_many, the G2 twin of msm.g1_lincomb_many: out[s] = sum of scalars[t] * points[t] over
    offsets[s] <= t < offsets[s + 1], for S = len(offsets) - 1 short segments in a fixed number of launches; (S, 36) normalised
    Jacobian limbs.  Records (n, 24) / (n, 25) and canonical scalars as for G2VariableBaseMSM.msm_bigint; an empty segment is
    the identity."""
    capi.ensure_init()
    pts = _records(points)
    sc = capi.u64(scalars_canonical).reshape(-1, 4)
    off = np.ascontiguousarray(offsets, dtype=np.uintp)
    S = len(off) - 1
    assert S >= 0 and (S == 0 or int(off[-1]) <= min(len(pts), len(sc)))
    out = np.empty((max(S, 0), 36), dtype=np.uint64)
    capi.check(capi.load().gm_g2_lincomb_many(capi.ptr(pts), C.c_size_t(pts.shape[1] * 8), capi.ptr(sc), capi.ptr(off), C.c_size_t(S), capi.ptr(out)))
    return out


class G2Bases:
    """G2 points resident in HBM (the `g2s` of herring's Crs, src/herring/ipa.rs:86-96)."""

    def __init__(self, handle: int, n: int):
        self.handle = handle
        self.n = n

    @classmethod
    def register(cls, bases: np.ndarray) -> "G2Bases":
        capi.ensure_init()
        bases = _records(bases)
        h = C.c_uint64()
        capi.check(capi.load().gm_g2_bases_register(capi.ptr(bases), C.c_size_t(bases.shape[1] * 8), C.c_size_t(len(bases)), C.byref(h)))
        return cls(h.value, len(bases))

    @classmethod
    def fixed_base(cls, base_affine: np.ndarray, scalars_canonical: np.ndarray) -> "G2Bases":
        """[s_i * base] generated on the device (gm_g2_fixed_base_register): base a 24-limb record, scalars (n, 4) canonical --
        any 256-bit value, taken as that integer; a zero scalar gives the identity record"""
        capi.ensure_init()
        sc = capi.u64(scalars_canonical).reshape(-1, 4)
        h = C.c_uint64()
        capi.check(capi.load().gm_g2_fixed_base_register(capi.ptr(capi.u64(base_affine).reshape(24)), capi.ptr(sc), C.c_size_t(len(sc)), C.byref(h)))
        return cls(h.value, len(sc))

    @classmethod
    def srs(cls, base_affine: np.ndarray, tau_canonical: np.ndarray, n: int) -> "G2Bases":
        """powers_of_g2[i] = tau^i * g2 (src/kzg/time.rs:60-67), generated on the device (gm_g2_srs_register)"""
        capi.ensure_init()
        h = C.c_uint64()
        capi.check(capi.load().gm_g2_srs_register(capi.ptr(capi.u64(base_affine).reshape(24)), capi.ptr(capi.u64(tau_canonical).reshape(4)), C.c_size_t(n),
                                                  C.byref(h)))
        return cls(h.value, n)

    @classmethod
    def from_candidates(cls, cand: bytes, n: int):
        """gm_g2_bases_from_candidates: the first n surviving candidates (96 bytes each), cofactor-cleared on the device
        -> (G2Bases or None on a shortfall, used, found)"""
        from .points import bases_from_candidates

        return bases_from_candidates(2, cand, n)

    def download(self, offset: int = 0, n: int | None = None) -> np.ndarray:
        n = self.n - offset if n is None else n
        out = np.empty((n, 24), dtype=np.uint64)
        capi.check(capi.load().gm_g2_bases_download(C.c_uint64(self.handle), C.c_size_t(offset), C.c_size_t(n), capi.ptr(out)))
        return out

    def msm_bigint(self, scalars: np.ndarray, offset: int = 0, reversed_: bool = False) -> np.ndarray:
        sc = capi.u64(scalars).reshape(-1, 4)
        out = np.empty(36, dtype=np.uint64)
        capi.check(capi.load().gm_g2_msm_h(C.c_uint64(self.handle), C.c_size_t(offset), C.c_int(int(reversed_)), capi.ptr(sc),
                                           C.c_size_t(len(sc)), capi.ptr(out)))
        return out

    def msm_device(self, d_scalars_ptr: int, n: int, mont: bool, offset: int = 0, reversed_: bool = False) -> np.ndarray:
        out = np.empty(36, dtype=np.uint64)
        capi.check(capi.load().gm_g2_msm_d(C.c_uint64(self.handle), C.c_size_t(offset), C.c_int(int(reversed_)), C.c_void_p(d_scalars_ptr),
                                           C.c_int(int(mont)), C.c_size_t(n), capi.ptr(out)))
        return out

    def msm_vec(self, vec, n: int | None = None, voffset: int = 0, offset: int = 0, reversed_: bool = False) -> np.ndarray:
        n = len(vec) - voffset if n is None else n
        out = np.empty(36, dtype=np.uint64)
        capi.check(capi.load().gm_g2_msm_v(C.c_uint64(self.handle), C.c_size_t(offset), C.c_int(int(reversed_)), C.c_uint64(vec.handle),
                                           C.c_size_t(voffset), C.c_size_t(n), capi.ptr(out)))
        return out

    def check(self, offset: int = 0, n: int | None = None):
        """curve and subgroup check of the resident points (gm_g2_bases_check); a points.CheckResult"""
        from .points import check_g2_bases

        return check_g2_bases(self, offset, n)

    @classmethod
    def from_bytes(cls, data: bytes, n: int, compress: bool, enc: int = 0, validate: bool = True):
        """gm_g2_bases_from_bytes -> (G2Bases or None, points.CheckResult); the definition is g2.deserialize(strict=True)"""
        from .points import g2_bases_from_bytes

        return g2_bases_from_bytes(data, n, compress, enc, validate)

    def to_bytes(self, compress: bool, enc: int = 0, offset: int = 0, n: int | None = None) -> bytes:
        """the canonical encodings of the resident points, n x 96 / 192 bytes (gm_g2_bases_to_bytes)"""
        from .points import g2_bases_to_bytes

        return g2_bases_to_bytes(self, compress, enc, offset, n)

    def free(self):
        if self.handle:
            capi.check(capi.load().gm_g2_bases_free(C.c_uint64(self.handle)))
            self.handle = 0

    def __len__(self):
        return self.n


class G2VariableBaseMSM:
    """ark_ec::VariableBaseMSM for G2Projective."""

    @staticmethod
    def msm_bigint(bases: np.ndarray, bigints: np.ndarray) -> np.ndarray:
        capi.ensure_init()
        bases = _records(bases)
        sc = capi.u64(bigints).reshape(-1, 4)
        n = min(len(bases), len(sc))  # zip semantics of the reference
        out = np.empty(36, dtype=np.uint64)
        capi.check(capi.load().gm_g2_msm(capi.ptr(bases), C.c_size_t(bases.shape[1] * 8), capi.ptr(sc), C.c_size_t(n), capi.ptr(out)))
        return out

    @staticmethod
    def msm_unchecked(bases: np.ndarray, scalars_mont: np.ndarray) -> np.ndarray:
        """Silently truncates to the shorter input, like the reference (src/herring/ipa.rs:117)."""
        from .fr import FrVec

        capi.ensure_init()
        bases = _records(bases)
        sc = capi.u64(scalars_mont).reshape(-1, 4)
        n = min(len(bases), len(sc))
        if n == 0:
            return g2_sum(np.empty((0, 36), dtype=np.uint64))
        reg = G2Bases.register(bases[:n])
        vec = FrVec.from_host(sc[:n])
        try:
            return reg.msm_vec(vec)  # into_bigint happens on device
        finally:
            vec.free()
            reg.free()
