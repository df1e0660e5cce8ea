"""TensorcheckProof (src/subprotocols/tensorcheck/mod.rs:39-46), foldings_polynomial (:124-133) and the prover `TensorcheckProof.new_time`
(:190-275) as one call into the library (gm_tensorcheck_new_time, gemini_amd/csrc/subprotocols.cpp).  The whole provers call the same
statement (gemini_amd/csrc/tensorcheck.hpp); its step-wise statement is tests/stepwise/tensorcheck_steps.py."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .fr import FrVec, _as_vec, fold_polynomial


class _Body(C.Structure):
    _fields_ = [("polys", C.c_void_p), ("npolys", C.c_size_t), ("challenges_mont", C.c_void_p), ("nchallenges", C.c_size_t)]


class _Proof(C.Structure):
    _fields_ = [("nfold", C.c_size_t), ("cap_folds", C.c_size_t), ("fold_commitments", C.c_void_p), ("fold_evaluations", C.c_void_p),
                ("evaluation_proof", C.c_uint64 * 18), ("nbase", C.c_size_t), ("base_evaluations", C.c_void_p)]


class _Claim(C.Structure):
    _fields_ = [("asserted_res_mont", C.c_void_p), ("nasserted", C.c_size_t), ("fold_randomness_mont", C.c_void_p), ("nrandomness", C.c_size_t),
                ("direct_base_evals_mont", C.c_uint64 * 8)]


def foldings_polynomial(polynomial: FrVec, challenges_mont) -> list:
    """:124-133  successive folds with all challenges but the last (strip_last)"""
    out = []
    cur = polynomial
    for ch in list(challenges_mont)[:-1]:
        cur = fold_polynomial(cur, ch)
        out.append(cur)
    return out


class TensorcheckProof:
    def __init__(self, folded_polynomials_commitments, folded_polynomials_evaluations, evaluation_proof, base_polynomials_evaluations):
        self.folded_polynomials_commitments = folded_polynomials_commitments
        self.folded_polynomials_evaluations = folded_polynomials_evaluations
        self.evaluation_proof = evaluation_proof
        self.base_polynomials_evaluations = base_polynomials_evaluations

    @staticmethod
    def new_time(transcript, ck, base_polynomials, body_polynomials, cap_folds: int | None = None) -> "TensorcheckProof":
        """:190-275.  base_polynomials: device vectors (FrVec) or host arrays; body_polynomials: [(polynomials, challenges)], the
        challenges Montgomery (k, 4).  cap_folds: room for the foldings (default: exactly sum (len(challenges) - 1))."""
        tmp = []

        def dev(p):
            v, t = _as_vec(p)
            if t:
                tmp.append(v)
            return v.handle

        try:
            bases = np.array([dev(p) for p in base_polynomials], dtype=np.uint64)
            keep, bodies = [], (_Body * max(len(body_polynomials), 1))()
            nfold = 0
            for b, (polys, challenges) in enumerate(body_polynomials):
                hp = np.array([dev(p) for p in polys], dtype=np.uint64)
                ch = capi.u64(np.asarray(challenges, dtype=np.uint64).reshape(-1, 4))
                keep += [hp, ch]
                bodies[b] = _Body(hp.ctypes.data, len(hp), ch.ctypes.data, len(ch))
                nfold += max(len(ch) - 1, 0)
            cap = nfold if cap_folds is None else int(cap_folds)
            fc = np.zeros((max(cap, 1), 18), dtype=np.uint64)
            fe = np.zeros((max(cap, 1), 2, 4), dtype=np.uint64)
            be = np.zeros((max(len(bases), 1), 3, 4), dtype=np.uint64)
            rec = _Proof(0, cap, fc.ctypes.data, fe.ctypes.data, (C.c_uint64 * 18)(), len(bases), be.ctypes.data)
            capi.check(capi.load().gm_tensorcheck_new_time(C.c_uint64(transcript.handle), C.c_uint64(ck.powers_of_g.handle), capi.ptr(bases),
                                                           C.c_size_t(len(bases)), bodies, C.c_size_t(len(body_polynomials)), C.byref(rec)))
        finally:
            for v in tmp:
                v.free()
        n = rec.nfold
        return TensorcheckProof([fc[i].copy() for i in range(n)], [fe[i].copy() for i in range(n)], np.array(rec.evaluation_proof, dtype=np.uint64),
                                [be[i].copy() for i in range(len(bases))])

    def _record(self):
        """the gm_tensorcheck_proof record of this proof and the arrays it points into (keep them alive)"""
        n = len(self.folded_polynomials_commitments)
        fc = capi.u64(np.asarray(self.folded_polynomials_commitments, dtype=np.uint64).reshape(n, 18))
        fe = capi.u64(np.asarray(self.folded_polynomials_evaluations, dtype=np.uint64).reshape(n, 8))
        nb = len(self.base_polynomials_evaluations)
        be = capi.u64(np.asarray(self.base_polynomials_evaluations, dtype=np.uint64).reshape(nb, 12))
        ep = (C.c_uint64 * 18)(*[int(v) for v in capi.u64(self.evaluation_proof).reshape(18)])
        return _Proof(n, n, fc.ctypes.data, fe.ctypes.data, ep, nb, be.ctypes.data), (fc, fe, be)

    def verify(self, transcript, vk, asserted_res_vec, base_polynomials_commitments, direct_base_polynomials_evaluations, fold_randomness, eval_chal,
               batch_challenge) -> None:
        """:286-385 (gm_tensorcheck_verify): one entry of asserted_res_vec / direct_base_polynomials_evaluations / fold_randomness per
        tensor-check instance, all Montgomery.  Raises VerificationError on a rejected proof."""
        from .kzg import VerificationError

        rec, keep = self._record()
        k = len(fold_randomness)
        assert len(asserted_res_vec) == k and len(direct_base_polynomials_evaluations) == k
        claims = (_Claim * max(k, 1))()
        for i in range(k):
            ar = capi.u64(np.asarray(asserted_res_vec[i], dtype=np.uint64).reshape(-1, 4))
            fr_ = capi.u64(np.asarray(fold_randomness[i], dtype=np.uint64).reshape(-1, 4))
            de = capi.u64(np.asarray(direct_base_polynomials_evaluations[i], dtype=np.uint64).reshape(8))
            keep += (ar, fr_)
            claims[i] = _Claim(ar.ctypes.data, len(ar), fr_.ctypes.data, len(fr_), (C.c_uint64 * 8)(*[int(v) for v in de]))
        bc = capi.u64(np.asarray(base_polynomials_commitments, dtype=np.uint64).reshape(-1, 18))
        ok = C.c_int()
        capi.check(capi.load().gm_tensorcheck_verify(C.c_uint64(transcript.handle), C.c_uint64(vk.handle), C.byref(rec), capi.ptr(bc), C.c_size_t(len(bc)), claims,
                                                     C.c_size_t(k), capi.ptr(capi.u64(eval_chal).reshape(4)), capi.ptr(capi.u64(batch_challenge).reshape(4)), C.byref(ok)))
        if not ok.value:
            raise VerificationError("tensorcheck: rejected")
