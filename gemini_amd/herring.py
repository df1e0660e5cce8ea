"""Host mirror of herring's sumcheck over a bilinear module (src/herring): the TimeProver of
src/herring/time_prover.rs:42-137 for the five module instances of src/herring/module.rs:
FModule (F x F -> F), G1Module (G1 x F -> G1), G2Module (F x G2 -> G2), PModule (G1 x G2 -> GT; pairings are
gemini_amd/pairing.py) and GtModule (GT x F -> GT; the device multi-exponentiation is pairing.gt_multi_pow), and the SpaceProver of
src/herring/space_prover.rs:39-316 for G1Module and G2Module over a registered key (G1ModuleSpaceProver, G2ModuleSpaceProver).  The inner-product
argument built on them is gemini_amd/ipa.py (its PModule provers are batched inside the library, not instances of the classes here, and
its GT multi-exponentiations stay on the host); InnerProductProof::generic and CrsStream are out of scope."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .sumcheck import TimeProver as _FieldTimeProver


class FModuleTimeProver(_FieldTimeProver):
    """TimeProver<FModule>: messages a = <f_e, g_e>, b = <f_e, g_o> + <f_o, g_e>; the twist only enters fold"""

    def __init__(self, f, g, twist_mont):
        super().__init__(f, g, twist_mont)
        capi.check(capi.load().gm_sc_set_herring(C.c_uint64(self.handle), C.c_int(1)))


class _ModuleTimeProver:
    """what the module provers share; a subclass sets the prefix of its C functions (gm_<prefix>_round, ...) and the limb counts of
    a message element and of the two final foldings, and creates `self.handle`"""

    _prefix = ""
    _msg = _final_f = _final_g = 0

    def _call(self, name, *args):
        capi.check(getattr(capi.load(), f"gm_{self._prefix}_{name}")(C.c_uint64(self.handle), *args))

    def next_message(self, verifier_message=None):
        a = np.empty(self._msg, dtype=np.uint64)
        b = np.empty(self._msg, dtype=np.uint64)
        has = C.c_int()
        ch = None if verifier_message is None else capi.ptr(capi.u64(verifier_message).reshape(4))
        self._call("round", ch, capi.ptr(a), capi.ptr(b), C.byref(has))
        return (a, b) if has.value else None

    def fold(self, challenge):
        self._call("fold", capi.ptr(capi.u64(challenge).reshape(4)))

    def rounds(self) -> int:
        t = C.c_size_t()
        self._call("rounds", C.byref(t), None)
        return t.value

    def round(self) -> int:
        r = C.c_size_t()
        self._call("rounds", None, C.byref(r))
        return r.value

    def final_foldings(self):
        f0 = np.empty(self._final_f, dtype=np.uint64)
        g0 = np.empty(self._final_g, dtype=np.uint64)
        has = C.c_int()
        self._call("final", capi.ptr(f0), capi.ptr(g0), C.byref(has))
        return (f0, g0) if has.value else None

    def free(self):
        if self.handle:
            self._call("free")
            self.handle = 0


class G1ModuleTimeProver(_ModuleTimeProver):
    """TimeProver<G1Module>: f = G1 points ((n, 12) affine Montgomery, or (n, 13) Rust records), g = Fr"""

    _prefix, _msg, _final_f, _final_g = "hg1", 18, 18, 4

    def __init__(self, f_points, g, twist_mont):
        capi.ensure_init()
        fp = capi.u64(f_points)
        gm_ = capi.u64(g).reshape(-1, 4)
        h = C.c_uint64()
        capi.check(capi.load().gm_hg1_new(capi.ptr(fp), C.c_size_t(fp.shape[1] * 8), C.c_size_t(len(fp)), capi.ptr(gm_), C.c_size_t(len(gm_)),
                                          capi.ptr(capi.u64(twist_mont).reshape(4)), C.byref(h)))
        self.handle = h.value


class G2ModuleTimeProver(_ModuleTimeProver):
    """TimeProver<G2Module>: f = Fr, g = G2 points ((n, 24) affine Montgomery, or (n, 25) Rust records); messages and the final
    g are (36,) normalised Jacobian"""

    _prefix, _msg, _final_f, _final_g = "hg2", 36, 4, 36

    def __init__(self, f, g_points, twist_mont):
        capi.ensure_init()
        fm = capi.u64(f).reshape(-1, 4)
        gp = capi.u64(g_points)
        h = C.c_uint64()
        capi.check(capi.load().gm_hg2_new(capi.ptr(fm), C.c_size_t(len(fm)), capi.ptr(gp), C.c_size_t(gp.shape[1] * 8), C.c_size_t(len(gp)),
                                          capi.ptr(capi.u64(twist_mont).reshape(4)), C.byref(h)))
        self.handle = h.value


class PModuleTimeProver(_ModuleTimeProver):
    """TimeProver<PModule>: f = G1 points ((n, 12) / (n, 13) records), g = G2 points ((n, 24) / (n, 25) records); messages are
    pairs of (72,) GT elements (gemini_amd/pairing.py), b one Miller product over both halves with one final exponentiation.
    A call after the one that returned None raises GM_ESTATE."""

    _prefix, _msg, _final_f, _final_g = "hp", 72, 18, 36

    def __init__(self, f_points, g_points, twist_mont):
        capi.ensure_init()
        fp = capi.u64(f_points)
        gp = capi.u64(g_points)
        h = C.c_uint64()
        capi.check(capi.load().gm_hp_new(capi.ptr(fp), C.c_size_t(fp.shape[1] * 8), C.c_size_t(len(fp)), capi.ptr(gp), C.c_size_t(gp.shape[1] * 8),
                                         C.c_size_t(len(gp)), capi.ptr(capi.u64(twist_mont).reshape(4)), C.byref(h)))
        self.handle = h.value


class GtModuleTimeProver(_ModuleTimeProver):
    """TimeProver<GtModule>: f = GT elements ((n, 72) limbs, gemini_amd/pairing.py; any reduced coefficients are taken on trust),
    g = Fr; messages are pairs of (72,) GT elements, a = prod f[2i]^g[2i], b = prod f[2i]^g[2i+1] * prod f[2i+1]^g[2i] in one
    launch; the fold is f'[i] = f[2i] * f[2i+1]^(r twist).  Calls after the one that returned None go on as G1/G2 do."""

    _prefix, _msg, _final_f, _final_g = "hgt", 72, 72, 4

    def __init__(self, f_gt, g, twist_mont):
        capi.ensure_init()
        fg = capi.u64(f_gt).reshape(-1, 72)
        gm_ = capi.u64(g).reshape(-1, 4)
        h = C.c_uint64()
        capi.check(capi.load().gm_hgt_new(capi.ptr(fg), C.c_size_t(len(fg)), capi.ptr(gm_), C.c_size_t(len(gm_)),
                                          capi.ptr(capi.u64(twist_mont).reshape(4)), C.byref(h)))
        self.handle = h.value

    def check(self):
        """gm_hgt_check: the GT membership test (pairing.gt_check) over the CURRENT f vector, where it lies on the device; a
        points.ProofCheckResult (ok, first_bad = the smallest bad index, the length when all pass)"""
        from .points import check_proof

        return check_proof(capi.load().gm_hgt_check, C.c_uint64(self.handle))


class _ModuleSpaceProver(_ModuleTimeProver):
    """what the two module space provers share: the TimeProver's calls under the gm_hsp*_ names, to_time and path.  The key and the
    Fr vector a prover was made from stay alive and unmodified until free()"""

    _time_class = None

    def to_time(self):
        """TimeProver::from(&SpaceProver): a time prover of the same module at the same round, twist and number of rounds, its point
        vector the folded points in an allocation of its own; this prover stays valid"""
        h = C.c_uint64()
        self._call("to_time", C.byref(h))
        t = self._time_class.__new__(self._time_class)
        t.handle = h.value
        return t

    def path(self):
        """gm_debug_hsp_path: (MSM calls, launches of k_hsp_scalars, point bytes allocated, scalar bytes allocated) so far"""
        out = (C.c_size_t * 4)()
        capi.check(capi.load().gm_debug_hsp_path(C.c_uint64(self.handle), out))
        return tuple(out)


class G1ModuleSpaceProver(_ModuleSpaceProver):
    """SpaceProver<G1Module>: the Lhs is the big-endian stream bases[offset + i], i < n, of a msm.G1Bases key, read where it lies;
    the Rhs an fr.FrVec holding the big-endian Fr stream.  Messages and the final f are (18,) normalised Jacobian.  The messages
    carry the twist (space_prover.rs:188-207), a TimeProver's do not: the two agree at twist = 1"""

    _prefix, _msg, _final_f, _final_g = "hsp1", 18, 18, 4
    _time_class = G1ModuleTimeProver

    def __init__(self, bases, g_stream, twist_mont, offset: int = 0, n: int | None = None):
        capi.ensure_init()
        n = bases.n - offset if n is None else n
        h = C.c_uint64()
        capi.check(capi.load().gm_hsp1_new_borrow(C.c_uint64(bases.handle), C.c_size_t(offset), C.c_size_t(n), C.c_uint64(g_stream.handle),
                                                  capi.ptr(capi.u64(twist_mont).reshape(4)), C.byref(h)))
        self.handle = h.value
        self._keep = (bases, g_stream)

    @classmethod
    def from_host(cls, f_points, g_stream, twist_mont):
        """gm_hsp1_new: host records ((n, 12) or (n, 13)) and a host stream; the prover registers a key of its own"""
        capi.ensure_init()
        fp = capi.u64(f_points)
        gm_ = capi.u64(g_stream).reshape(-1, 4)
        h = C.c_uint64()
        capi.check(capi.load().gm_hsp1_new(capi.ptr(fp), C.c_size_t(fp.shape[1] * 8), C.c_size_t(len(fp)), capi.ptr(gm_), C.c_size_t(len(gm_)),
                                           capi.ptr(capi.u64(twist_mont).reshape(4)), C.byref(h)))
        self = cls.__new__(cls)
        self.handle = h.value
        self._keep = ()
        return self


class G2ModuleSpaceProver(_ModuleSpaceProver):
    """SpaceProver<G2Module>: the Lhs is an fr.FrVec holding the big-endian Fr stream, the Rhs the stream bases[offset + i], i < n, of
    a g2msm.G2Bases key.  Messages and the final g are (36,) normalised Jacobian"""

    _prefix, _msg, _final_f, _final_g = "hsp2", 36, 4, 36
    _time_class = G2ModuleTimeProver

    def __init__(self, f_stream, bases, twist_mont, offset: int = 0, n: int | None = None):
        capi.ensure_init()
        n = bases.n - offset if n is None else n
        h = C.c_uint64()
        capi.check(capi.load().gm_hsp2_new_borrow(C.c_uint64(f_stream.handle), C.c_uint64(bases.handle), C.c_size_t(offset), C.c_size_t(n),
                                                  capi.ptr(capi.u64(twist_mont).reshape(4)), C.byref(h)))
        self.handle = h.value
        self._keep = (f_stream, bases)

    @classmethod
    def from_host(cls, f_stream, g_points, twist_mont):
        """gm_hsp2_new: a host stream and host records ((n, 24) or (n, 25))"""
        capi.ensure_init()
        fm = capi.u64(f_stream).reshape(-1, 4)
        gp = capi.u64(g_points)
        h = C.c_uint64()
        capi.check(capi.load().gm_hsp2_new(capi.ptr(fm), C.c_size_t(len(fm)), capi.ptr(gp), C.c_size_t(gp.shape[1] * 8), C.c_size_t(len(gp)),
                                           capi.ptr(capi.u64(twist_mont).reshape(4)), C.byref(h)))
        self = cls.__new__(cls)
        self.handle = h.value
        self._keep = ()
        return self
