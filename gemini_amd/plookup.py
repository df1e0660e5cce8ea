"""src/subprotocols/plookup/time_prover.rs: `lookup` (:5-8), `plookup` (:89-112) and the extended frequency behind `sorted` (:65-78), which the
library builds on the device (gm_idx_extend_frequency: no host pass over the index, no upload)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .fr import FrVec, IdxVec, _as_vec, lookup  # noqa: F401  (lookup: re-exported under the reference's path)


def extend_frequency_device(index: IdxVec, set_len: int) -> IdxVec:
    """extend_frequency(compute_frequency(set_len, index)) (:65-78) as a NEW device index vector: every v < set_len appears
    1 + #{j : index[j] == v} times, in order.  An entry >= set_len raises (GM_EINVAL)."""
    h, n = C.c_uint64(), C.c_size_t()
    capi.check(capi.load().gm_idx_extend_frequency(C.c_uint64(index.handle), C.c_size_t(set_len), C.byref(h), C.byref(n)))
    return IdxVec(h.value, n.value)


def plookup(subset, set_, index: IdxVec, y, z, zeta, ext_fre: IdxVec | None = None) -> list:
    """:89-112 -> [lookup_set, lookup_subset, lookup_sorted] (three new FrVec).  ext_fre: the extended frequency of `index` over
    `set_` when the caller keeps it across proofs (extend_frequency_device, or what the preprocessing builds); else it is built
    on the device inside the call and dropped."""
    sub, tmp_sub = _as_vec(subset)
    st, tmp_set = _as_vec(set_)
    out = np.zeros(3, dtype=np.uint64)
    try:
        capi.check(capi.load().gm_plookup_new_time(
            C.c_uint64(sub.handle), C.c_uint64(st.handle), C.c_uint64(index.handle), C.c_uint64(ext_fre.handle if ext_fre is not None else 0),
            capi.ptr(capi.u64(y).reshape(4)), capi.ptr(capi.u64(z).reshape(4)), capi.ptr(capi.u64(zeta).reshape(4)), capi.ptr(out)))
    finally:
        if tmp_sub:
            sub.free()
        if tmp_set:
            st.free()
    res = []
    for h in out:
        n = C.c_size_t()
        capi.check(capi.load().gm_fr_vec_len(C.c_uint64(int(h)), C.byref(n)))
        res.append(FrVec(int(h), n.value))
    return res
