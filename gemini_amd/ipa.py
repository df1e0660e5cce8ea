"""Host mirror of herring's inner-product argument (src/herring/ipa.rs): `Crs` (:172-213), `Vrs` (:215-247) and
`InnerProductProof` with `new` (:533-685) and `verify_transcript` (:250-343).  All arithmetic happens in libgemini_hip.so
(gm_crs_*, gm_vrs_*, gm_ipa_*; gemini_amd/csrc/ipa.hip): the prover keeps every vector on the device and the round loop is the
library's, with the transcript inside it.

Data conventions (numpy uint64): G1 records (n, 12) / (n, 13) as in gemini_amd.msm, G2 records (n, 24) / (n, 25) as in
gemini_amd.g2msm, scalars (n, 4) Montgomery, points (18,) / (36,) normalised Jacobian, GT elements (72,) as in gemini_amd.pairing.
The reference defines no wire format for this proof and none is claimed here.  `InnerProductProof::generic` (pub(crate), called
by one test of the reference) and `CrsStream` (its fold is a todo!() in the reference) are out of scope.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, replace

import numpy as np

from . import capi
from .g2msm import _records as _g2_records
from .pairing import _g1_records


class Crs:
    """`Crs`: G1 and G2 points resident in HBM"""

    def __init__(self, g1_records, g2_records):
        capi.ensure_init()
        g1, g2 = _g1_records(g1_records), _g2_records(g2_records)
        h = C.c_uint64()
        capi.check(capi.load().gm_crs_new(capi.ptr(g1), C.c_size_t(g1.shape[1] * 8), C.c_size_t(len(g1)), capi.ptr(g2), C.c_size_t(g2.shape[1] * 8),
                                          C.c_size_t(len(g2)), C.byref(h)))
        self.handle = h.value
        self.n1, self.n2 = len(g1), len(g2)

    @classmethod
    def from_bases(cls, g1, g2) -> "Crs":
        """gm_crs_from_bases: a CRS from two registered handles (G1Bases, G2Bases) by device-to-device copy; the handles stay the caller's"""
        h = C.c_uint64()
        capi.check(capi.load().gm_crs_from_bases(C.c_uint64(g1.handle), C.c_uint64(g2.handle), C.byref(h)))
        crs = cls.__new__(cls)
        crs.handle, crs.n1, crs.n2 = h.value, len(g1), len(g2)
        return crs

    @classmethod
    def from_bytes(cls, g1_bytes: bytes, n1: int, g2_bytes: bytes, n2: int, compress: bool, enc: int = 0, validate: bool = True):
        """A CRS that arrives as bytes, decoded (and with `validate` checked) on the device without visiting the host as points.
        -> (Crs or None, the points.CheckResult of the G1 half, that of the G2 half or None when the G1 half was rejected)"""
        from .points import g1_bases_from_bytes, g2_bases_from_bytes

        b1, r1 = g1_bases_from_bytes(g1_bytes, n1, compress, enc, validate)
        if b1 is None:
            return None, r1, None
        try:
            b2, r2 = g2_bases_from_bytes(g2_bytes, n2, compress, enc, validate)
            if b2 is None:
                return None, r1, r2
            try:
                return cls.from_bases(b1, b2), r1, r2
            finally:
                b2.free()
        finally:
            b1.free()

    @classmethod
    def from_scalars(cls, a_canonical, b_canonical, g1_affine=None, g2_affine=None) -> "Crs":
        """g1s[i] = a_i g1, g2s[i] = b_i g2, both generated on the device (gm_g1_fixed_base_register, gm_g2_fixed_base_register).
        FOR TESTS AND BENCHMARKS ONLY: whoever knows a and b knows every discrete logarithm of this CRS and can break the binding
        of the commitments, and with it the soundness of the inner-product argument.  `Crs.new` draws points nobody has the logarithms of."""
        from .g2 import generator
        from .g2msm import G2Bases, g2_points_to_affine
        from .kzg import g1_generator_mont
        from .msm import G1Bases

        g1 = g1_generator_mont() if g1_affine is None else g1_affine
        g2 = g2_points_to_affine([generator()])[0] if g2_affine is None else g2_affine
        b1 = G1Bases.fixed_base(g1, a_canonical)
        try:
            b2 = G2Bases.fixed_base(g2, b_canonical)
            try:
                return cls.from_bases(b1, b2)
            finally:
                b2.free()
        finally:
            b1.free()

    @classmethod
    def new(cls, seed: bytes, d: int) -> "Crs":
        """`Crs::new(rng, d)` (ipa.rs:173-177) with a seed in the place of the rng: d points of each group whose logarithms nobody
        knows, the survivors of the SHAKE-256 candidate stream of (seed, group) cleared of their cofactors on the device
        (points.bases_from_seed).  The stream and the map from candidates to points are this package's own: no parity with the
        draws of arkworks' `rand` is claimed."""
        from .points import bases_from_seed

        assert d >= 1
        b1 = bases_from_seed(1, seed, d)
        try:
            b2 = bases_from_seed(2, seed, d)
            try:
                return cls.from_bases(b1, b2)
            finally:
                b2.free()
        finally:
            b1.free()

    @classmethod
    def _of(cls, handle: int) -> "Crs":
        n1, n2 = C.c_size_t(), C.c_size_t()
        capi.check(capi.load().gm_crs_len(C.c_uint64(handle), C.byref(n1), C.byref(n2)))
        crs = cls.__new__(cls)
        crs.handle, crs.n1, crs.n2 = handle, n1.value, n2.value
        return crs

    def truncate(self, rounds: int) -> "Crs":
        """Crs::truncate (ipa.rs:191-196) as a NEW Crs: the first min(len, 2^rounds) points of each group; this one stays valid"""
        h = C.c_uint64()
        capi.check(capi.load().gm_crs_truncate(C.c_uint64(self.handle), C.c_size_t(rounds), C.byref(h)))
        return self._of(h.value)

    def halve(self) -> "Crs":
        """Crs::halve (ipa.rs:198-203) as a new Crs: the first ceil(len / 2) points of each group"""
        h = C.c_uint64()
        capi.check(capi.load().gm_crs_halve(C.c_uint64(self.handle), C.byref(h)))
        return self._of(h.value)

    def fold(self, challenge_mont) -> "Crs":
        """Crs::fold (ipa.rs:205-212) as a new Crs: g[i] = g[2i] + c g[2i+1] in both groups on the device, an odd tail against the
        identity.  Groups of different lengths are refused (GM_EINVAL)."""
        h = C.c_uint64()
        capi.check(capi.load().gm_crs_fold(C.c_uint64(self.handle), capi.ptr(capi.u64(challenge_mont).reshape(4)), C.byref(h)))
        return self._of(h.value)

    def bases(self):
        """gm_crs_to_bases: device copies of both arrays -> (G1Bases, G2Bases), the caller's to free; the inverse of from_bases"""
        from .g2msm import G2Bases
        from .msm import G1Bases

        h1, h2 = C.c_uint64(), C.c_uint64()
        capi.check(capi.load().gm_crs_to_bases(C.c_uint64(self.handle), C.byref(h1), C.byref(h2)))
        return G1Bases(h1.value, self.n1), G2Bases(h2.value, self.n2)

    def check(self):
        """gm_crs_check: curve and subgroup over both arrays; a points.KeyCheckResult"""
        from .points import check_crs

        return check_crs(self)

    def commit_g1(self, scalars_mont) -> np.ndarray:
        """Crs::commit_g1: the CRS must be longer than the scalars"""
        sc = capi.u64(scalars_mont).reshape(-1, 4)
        out = np.empty(18, dtype=np.uint64)
        capi.check(capi.load().gm_crs_commit_g1(C.c_uint64(self.handle), capi.ptr(sc), C.c_size_t(len(sc)), capi.ptr(out)))
        return out

    def commit_g2(self, scalars_mont) -> np.ndarray:
        sc = capi.u64(scalars_mont).reshape(-1, 4)
        out = np.empty(36, dtype=np.uint64)
        capi.check(capi.load().gm_crs_commit_g2(C.c_uint64(self.handle), capi.ptr(sc), C.c_size_t(len(sc)), capi.ptr(out)))
        return out

    def free(self):
        if self.handle:
            capi.check(capi.load().gm_crs_free(C.c_uint64(self.handle)))
            self.handle = 0


class Vrs:
    """`Vrs::from(&crs)`: per level the (even, odd) multi-pairings of each group against the other, one segmented launch for all"""

    def __init__(self, crs: Crs):
        h = C.c_uint64()
        capi.check(capi.load().gm_vrs_from_crs(C.c_uint64(crs.handle), C.byref(h)))
        self.handle = h.value

    @property
    def levels(self) -> int:
        n = C.c_size_t()
        capi.check(capi.load().gm_vrs_levels(C.c_uint64(self.handle), C.byref(n)))
        return n.value

    def level(self, l: int):
        """-> (vk1, vk2), each (2, 72): even, odd"""
        vk1, vk2 = np.empty((2, 72), dtype=np.uint64), np.empty((2, 72), dtype=np.uint64)
        capi.check(capi.load().gm_vrs_get(C.c_uint64(self.handle), C.c_size_t(l), capi.ptr(vk1), capi.ptr(vk2)))
        return vk1, vk2

    def free(self):
        if self.handle:
            capi.check(capi.load().gm_vrs_free(C.c_uint64(self.handle)))
            self.handle = 0


@dataclass
class IpaFields:
    """the fields of `InnerProductProof` (and of its `Sumcheck<PModule>`)"""

    rounds: int
    messages: np.ndarray          # (rounds, 2, 72)
    challenges: np.ndarray        # (rounds, 4)
    batch_challenges: np.ndarray  # (2 rounds + 1, 4)
    final_lhs: np.ndarray         # (2 (rounds - 1), 18)
    final_rhs: np.ndarray         # (2 (rounds - 1), 36)
    foldings_ff: np.ndarray       # (2, 4)
    foldings_fg1: tuple           # ((18,), (4,))
    foldings_fg2: tuple           # ((4,), (36,))
    # a proof for K claims (InnerProductProof.new_batch): batch_challenges (3 K + 2 (rounds - 1), 4) and K-long foldings,
    # foldings_ff (K, 2, 4), foldings_fg1 ((K, 18), (K, 4)), foldings_fg2 ((K, 4), (K, 36))
    claims: int = 1


class InnerProductProof:
    def __init__(self, handle: int):
        self.handle = handle

    @classmethod
    def new(cls, transcript, crs: Crs, a_mont, b_mont) -> "InnerProductProof":
        """InnerProductProof::new(transcript, crs, (a, b)); d = len(a) = len(b) >= 2 and the CRS holds max(d + 1, 2^rounds) points"""
        a, b = capi.u64(a_mont).reshape(-1, 4), capi.u64(b_mont).reshape(-1, 4)
        assert len(a) == len(b)
        h = C.c_uint64()
        capi.check(capi.load().gm_ipa_new(C.c_uint64(transcript.handle), C.c_uint64(crs.handle), capi.ptr(a), capi.ptr(b), C.c_size_t(len(a)), C.byref(h)))
        return cls(h.value)

    @classmethod
    def new_many(cls, transcripts, crs: Crs, a_monts, b_monts) -> list:
        """gm_ipa_new_many: [InnerProductProof.new(transcripts[s], crs, a_monts[s], b_monts[s]) for every s], byte for byte, with
        the rounds of all proofs in lockstep -- one launch group per round whatever the number of proofs.  All vectors have
        the same length d; every proof needs a transcript of its own, which is left as the single call leaves it."""
        capi.ensure_init()
        S = len(transcripts)
        assert len(a_monts) == S and len(b_monts) == S
        if S == 0:
            capi.check(capi.load().gm_ipa_new_many(None, C.c_uint64(crs.handle), None, None, C.c_size_t(0), C.c_size_t(0), None))
            return []
        a = np.ascontiguousarray(np.stack([capi.u64(x).reshape(-1, 4) for x in a_monts]))
        b = np.ascontiguousarray(np.stack([capi.u64(x).reshape(-1, 4) for x in b_monts]))
        assert a.shape == b.shape
        ts = np.array([t.handle for t in transcripts], dtype=np.uint64)
        hs = np.zeros(S, dtype=np.uint64)
        capi.check(capi.load().gm_ipa_new_many(capi.ptr(ts), C.c_uint64(crs.handle), capi.ptr(a), capi.ptr(b), C.c_size_t(a.shape[1]), C.c_size_t(S), capi.ptr(hs)))
        return [cls(int(h)) for h in hs]

    @classmethod
    def new_batch(cls, transcript, crs: Crs, a_monts, b_monts) -> "InnerProductProof":
        """gm_ipa_new_batch: ONE proof for the K claims <a_i, b_i> = y_i, <a_i, crs.g1> = comm_a_i, <b_i, crs.g2> = comm_b_i
        (InnerProductProof::generic with every twist one): one transcript, one set of round messages.  All vectors have the same
        length d.  K = 1 is `new` byte for byte."""
        capi.ensure_init()
        K = len(a_monts)
        assert len(b_monts) == K and K >= 1
        a = np.ascontiguousarray(np.stack([capi.u64(x).reshape(-1, 4) for x in a_monts]))
        b = np.ascontiguousarray(np.stack([capi.u64(x).reshape(-1, 4) for x in b_monts]))
        assert a.shape == b.shape
        h = C.c_uint64()
        capi.check(capi.load().gm_ipa_new_batch(C.c_uint64(transcript.handle), C.c_uint64(crs.handle), capi.ptr(a), capi.ptr(b), C.c_size_t(a.shape[1]), C.c_size_t(K),
                                                C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_fields_batch(cls, f: IpaFields) -> "InnerProductProof":
        """gm_ipa_from_fields_batch: a proof for f.claims claims from `batch_fields()`"""
        capi.ensure_init()
        K, k = f.claims, 2 * (f.rounds - 1)
        fg1 = np.ascontiguousarray(np.concatenate([capi.u64(f.foldings_fg1[0]).reshape(K, 18), capi.u64(f.foldings_fg1[1]).reshape(K, 4)], axis=1))
        fg2 = np.ascontiguousarray(np.concatenate([capi.u64(f.foldings_fg2[0]).reshape(K, 4), capi.u64(f.foldings_fg2[1]).reshape(K, 36)], axis=1))
        lhs, rhs = capi.u64(f.final_lhs).reshape(k, 18), capi.u64(f.final_rhs).reshape(k, 36)
        h = C.c_uint64()
        capi.check(capi.load().gm_ipa_from_fields_batch(C.c_size_t(f.rounds), C.c_size_t(K), capi.ptr(capi.u64(f.messages).reshape(f.rounds, 144)),
                                                        capi.ptr(capi.u64(f.challenges).reshape(f.rounds, 4)),
                                                        capi.ptr(capi.u64(f.batch_challenges).reshape(3 * K + k, 4)), capi.ptr(lhs) if k else None,
                                                        capi.ptr(rhs) if k else None, capi.ptr(capi.u64(f.foldings_ff).reshape(K, 8)), capi.ptr(fg1), capi.ptr(fg2),
                                                        C.byref(h)))
        return cls(h.value)

    @property
    def claims(self) -> int:
        """gm_ipa_claims: K of a `new_batch` proof, 1 for every other"""
        n = C.c_size_t()
        capi.check(capi.load().gm_ipa_claims(C.c_uint64(self.handle), C.byref(n)))
        return n.value

    def batch_fields(self) -> IpaFields:
        """the fields with K-long foldings, whatever K is (gm_ipa_foldings_batch)"""
        lib, h = capi.load(), C.c_uint64(self.handle)
        n = C.c_size_t()
        capi.check(lib.gm_ipa_rounds(h, C.byref(n)))
        r, K = n.value, self.claims
        k = 2 * (r - 1)
        msgs, ch, bch = np.empty((r, 2, 72), dtype=np.uint64), np.empty((r, 4), dtype=np.uint64), np.empty((3 * K + k, 4), dtype=np.uint64)
        lhs, rhs = np.empty((k, 18), dtype=np.uint64), np.empty((k, 36), dtype=np.uint64)
        ff, fg1, fg2 = np.empty((K, 2, 4), dtype=np.uint64), np.empty((K, 22), dtype=np.uint64), np.empty((K, 40), dtype=np.uint64)
        capi.check(lib.gm_ipa_messages(h, capi.ptr(msgs)))
        capi.check(lib.gm_ipa_challenges(h, capi.ptr(ch)))
        capi.check(lib.gm_ipa_batch_challenges(h, capi.ptr(bch)))
        capi.check(lib.gm_ipa_final_foldings(h, capi.ptr(lhs) if k else None, capi.ptr(rhs) if k else None))
        capi.check(lib.gm_ipa_foldings_batch(h, capi.ptr(ff), capi.ptr(fg1), capi.ptr(fg2)))
        return IpaFields(r, msgs, ch, bch, lhs, rhs, ff, (fg1[:, :18].copy(), fg1[:, 18:].copy()), (fg2[:, :4].copy(), fg2[:, 4:].copy()), K)

    def verify_batch(self, vrs: Vrs, comm_as, comm_bs, ys) -> bool:
        """gm_ipa_verify_batch: verify_transcript with 3 K initial claims; True for Ok(()).  K = len(ys) must be the proof's."""
        K = len(ys)
        ca, cb, y = capi.u64(comm_as).reshape(K, 18), capi.u64(comm_bs).reshape(K, 36), capi.u64(ys).reshape(K, 4)
        ok = C.c_int()
        capi.check(capi.load().gm_ipa_verify_batch(C.c_uint64(self.handle), C.c_uint64(vrs.handle), capi.ptr(ca), capi.ptr(cb), capi.ptr(y), C.c_size_t(K), C.byref(ok)))
        return bool(ok.value)

    @classmethod
    def from_fields(cls, f: IpaFields) -> "InnerProductProof":
        """a proof for one claim from `fields()`"""
        return cls.from_fields_batch(replace(f, claims=1))

    def fields(self) -> IpaFields:
        """`batch_fields()`, the foldings without the axis of the claims when there is one claim"""
        f = self.batch_fields()
        if f.claims == 1:
            f.foldings_ff, f.foldings_fg1, f.foldings_fg2 = f.foldings_ff[0], tuple(x[0] for x in f.foldings_fg1), tuple(x[0] for x in f.foldings_fg2)
        return f

    def verify_transcript(self, vrs: Vrs, comm_a, comm_b, y_mont) -> bool:
        """InnerProductProof::verify_transcript(vrs, comm_a, comm_b, y): True for Ok(())"""
        ok = C.c_int()
        capi.check(capi.load().gm_ipa_verify(C.c_uint64(self.handle), C.c_uint64(vrs.handle), capi.ptr(capi.u64(comm_a).reshape(18)),
                                             capi.ptr(capi.u64(comm_b).reshape(36)), capi.ptr(capi.u64(y_mont).reshape(4)), C.byref(ok)))
        return bool(ok.value)

    @staticmethod
    def verify_many(proofs, vrs: Vrs, comm_as, comm_bs, ys) -> list:
        """gm_ipa_verify_many: [proofs[s].verify_transcript(vrs, comm_as[s], comm_bs[s], ys[s]) for every s] from ONE launch
        group, whatever the number of proofs; they may differ in their number of rounds.  A proof with an element outside its
        group is answered by the per-proof path, so the list is the single entry's for every input."""
        capi.ensure_init()
        S = len(proofs)
        hs = np.array([p.handle for p in proofs], dtype=np.uint64)
        ca, cb, y = capi.u64(comm_as).reshape(S, 18), capi.u64(comm_bs).reshape(S, 36), capi.u64(ys).reshape(S, 4)
        ok = np.zeros(max(S, 1), dtype=np.intc)
        capi.check(capi.load().gm_ipa_verify_many(capi.ptr(hs) if S else None, C.c_uint64(vrs.handle), capi.ptr(ca) if S else None, capi.ptr(cb) if S else None,
                                                  capi.ptr(y) if S else None, C.c_size_t(S), capi.ptr(ok)))
        return [bool(v) for v in ok[:S]]

    def stated_terms(self, y_mont):
        """gm_debug_ipa_stated_terms, a test aid: the exponents of the one product in GT that verify_many states for this proof,
        as integers -- (6 rounds - 4 for the GT terms, 2 rounds + 4 for the pairing terms), in the order of tests/ipa_flat_ref.py"""
        n = C.c_size_t()
        capi.check(capi.load().gm_ipa_rounds(C.c_uint64(self.handle), C.byref(n)))
        r = n.value
        g, p = np.zeros((max(6 * r - 4, 1), 4), dtype=np.uint64), np.zeros((2 * r + 4, 4), dtype=np.uint64)
        capi.check(capi.load().gm_debug_ipa_stated_terms(C.c_uint64(self.handle), capi.ptr(capi.u64(y_mont).reshape(4)), capi.ptr(g), capi.ptr(p)))
        to_int = lambda row: sum(int(v) << (64 * k) for k, v in enumerate(row))  # noqa: E731
        return [to_int(e) for e in g[: 6 * r - 4]], [to_int(e) for e in p]

    def check_points(self):
        """gm_ipa_check: every G1 and G2 element verify_transcript reads from the proof (the G1 ones first); a points.ProofCheckResult.
        The GT elements of the messages are checked by `check_messages`."""
        from .points import check_proof

        return check_proof(capi.load().gm_ipa_check, C.c_uint64(self.handle))

    def check_messages(self):
        """gm_ipa_check_gt: GT membership of the 2 rounds message elements (a of round i is index 2 i, b is 2 i + 1); a
        points.ProofCheckResult"""
        from .points import check_proof

        return check_proof(capi.load().gm_ipa_check_gt, C.c_uint64(self.handle))

    def host_times(self) -> dict:
        """what gm_ipa_new spent on the host making this proof, ms (a measurement aid: tools/ipa_bench.py)"""
        ms = (C.c_double * 3)()
        capi.check(capi.load().gm_ipa_host_times(C.c_uint64(self.handle), ms))
        return {"gt_multi_pow_ms": ms[0], "final_exp_ms": ms[1], "call_ms": ms[2]}

    def free(self):
        if self.handle:
            capi.check(capi.load().gm_ipa_free(C.c_uint64(self.handle)))
            self.handle = 0


def set_new_many_min(proofs: int):
    """gm_set_ipa_new_many_min: fewer proofs than this make InnerProductProof.new_many run them one by one, as `new` does.  The
    bytes do not depend on it (profiles/ipa_new_many.md has the measurement behind the default)."""
    capi.ensure_init()
    capi.check(capi.load().gm_set_ipa_new_many_min(C.c_size_t(proofs)))


def new_many_path() -> tuple:
    """gm_debug_ipa_new_many_path, for the last new_many call: (proofs on the lockstep path, proofs on the per-proof path, kernel
    launches the lockstep path enqueued, stream waits it made)"""
    capi.ensure_init()
    counts = (C.c_size_t * 4)()
    capi.check(capi.load().gm_debug_ipa_new_many_path(counts))
    return tuple(int(c) for c in counts)


def new_batch_path() -> tuple:
    """gm_debug_ipa_new_batch_path, for the last new_batch call: (split-fold launches, MSM calls, Miller launches)"""
    capi.ensure_init()
    counts = (C.c_size_t * 3)()
    capi.check(capi.load().gm_debug_ipa_new_batch_path(counts))
    return tuple(int(c) for c in counts)


def set_verify_many_min(proofs: int):
    """gm_set_ipa_verify_many_min: fewer proofs than this make InnerProductProof.verify_many run them one by one, as
    verify_transcript does.  Verdicts do not depend on it (profiles/ipa_verify_many.md has the measurement behind the default)."""
    capi.ensure_init()
    capi.check(capi.load().gm_set_ipa_verify_many_min(C.c_size_t(proofs)))


def verify_many_path() -> tuple:
    """gm_debug_ipa_verify_many_path: (proofs of the last verify_many call that took the batched path, proofs that took the per-proof path)"""
    capi.ensure_init()
    counts = (C.c_size_t * 2)()
    capi.check(capi.load().gm_debug_ipa_verify_many_path(counts))
    return int(counts[0]), int(counts[1])
