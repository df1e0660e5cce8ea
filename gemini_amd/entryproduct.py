"""EntryProduct (src/subprotocols/entryproduct/mod.rs:21-31) and its time provers `new_time` / `new_time_batch`
(entryproduct/time_prover.rs:61-147) as one call into the library: gm_entryproduct_new_time_batch (gemini_amd/csrc/subprotocols.cpp)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .fr import _as_vec
from .sumcheck import TimeProver


class EntryProductMsgs:
    """entryproduct/mod.rs:21-25"""

    def __init__(self, acc_v_commitments, claimed_sumchecks):
        self.acc_v_commitments = acc_v_commitments
        self.claimed_sumchecks = claimed_sumchecks


class EntryProduct:
    """entryproduct/mod.rs:27-31: the prover's messages, the challenge, and one sumcheck prover per vector -- `TimeProver`s that own their
    data (the inputs may be freed at once) for `Sumcheck.prove_batch`."""

    def __init__(self, msgs: EntryProductMsgs, chal, provers):
        self.msgs, self.chal, self.provers = msgs, chal, provers

    @staticmethod
    def new_time_batch(transcript, ck, vs, claimed_products, acc_vs=None) -> "EntryProduct":
        """:61-114.  vs: device vectors (FrVec) or host arrays; acc_vs: accumulated_product(monic(v)) of each, when the caller holds them already."""
        assert len(vs) == len(claimed_products)
        assert acc_vs is None or len(acc_vs) == len(vs)
        k = len(vs)
        dev = [_as_vec(v) for v in vs]
        acc = [_as_vec(v) for v in acc_vs] if acc_vs is not None else None
        try:
            hv = np.array([v.handle for v, _ in dev], dtype=np.uint64)
            ha = np.array([v.handle for v, _ in acc], dtype=np.uint64) if acc is not None else None
            cps = capi.u64(np.asarray(claimed_products, dtype=np.uint64).reshape(k, 4))
            cms = np.zeros((k, 18), dtype=np.uint64)
            sums = np.zeros((k, 4), dtype=np.uint64)
            chal = np.zeros(4, dtype=np.uint64)
            provers = np.zeros(k, dtype=np.uint64)
            capi.check(capi.load().gm_entryproduct_new_time_batch(
                C.c_uint64(transcript.handle), C.c_uint64(ck.powers_of_g.handle), capi.ptr(hv), None if ha is None else capi.ptr(ha), C.c_size_t(k),
                capi.ptr(cps), capi.ptr(cms), capi.ptr(sums), capi.ptr(chal), capi.ptr(provers)))
        finally:
            for v, tmp in dev + (acc or []):
                if tmp:
                    v.free()
        return EntryProduct(EntryProductMsgs([cms[i].copy() for i in range(k)], [sums[i].copy() for i in range(k)]), chal,
                            [TimeProver.from_handle(int(h)) for h in provers])

    @staticmethod
    def new_time(transcript, ck, v, claimed_product) -> "EntryProduct":
        """:117-147"""
        return EntryProduct.new_time_batch(transcript, ck, [v], [claimed_product])

    def free(self):
        for p in self.provers:
            p.free()
