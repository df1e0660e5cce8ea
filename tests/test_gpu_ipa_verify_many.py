"""GPU: gm_ipa_verify_many -- many inner-product proofs verified in one launch group (gemini_amd/csrc/ipa.hip: ipa_verify_many; the
GT half is k_gt_multi_pow_seg of pairing.hip).

The contract is "ok[s] is gm_ipa_verify's answer, for every input": every list is held against the single entry called proof by
proof AND against the pattern the construction fixes (a device proof verifies, a tampered copy does not).  One call takes one Vrs,
so the proofs that are mixed in one call are made over one CRS of 128 points (d = 2, 3, 4, 5, 64: 1, 2, 2, 3 and 6 rounds, all but
the last under a Vrs deeper than their rounds); the shapes (d, n) = (2, 4), (3, 4), (4, 8), (5, 16) and the CRS with points at
infinity get calls over their own CRS.
"""
import ctypes as C
import os
import re
import threading

import numpy as np
import pytest

from gemini_amd import pairing as gp
from gemini_amd.fr import fr_from_int, fr_to_int
from tests import ipa_exponent_ref as X
from tests import ipa_flat_ref as F
from tests import points_ref as pr
from tests.test_gpu_gt_module import nonmembers
from tests.test_gpu_ipa import LABEL, mont, reference, scalars
from tests.test_gpu_pairing import g1_points_to_affine

pytestmark = pytest.mark.gpu

R = X.R
GM_EINVAL, GM_EHANDLE = -1, -3
DS = (2, 3, 4, 5, 64)


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


def default_min() -> int:
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gemini_amd", "csrc", "ctx.hpp")).read()
    m = re.search(r"size_t\s+ipa_verify_many_min\s*=\s*(\d+);", src)
    assert m, "ipa_verify_many_min not found in ctx.hpp"
    return int(m.group(1))


class Case:
    """one (proof, comm_a, comm_b, y) and what verify_transcript must say"""

    def __init__(self, name, proof, comm_a, comm_b, y, expect):
        self.name, self.proof, self.comm_a, self.comm_b, self.y, self.expect = name, proof, comm_a, comm_b, y, expect


def device_cases(gm, crs, d, zeros=()):
    """a device proof of <a, b> = y over `crs` and its tampered copies: the cases of test_verifier_rejects, a wrong y, the commitment
    of the other vector"""
    a, b = scalars(1000 + d, d, zeros), scalars(2000 + d, d, zeros[:1])
    am, bm = mont(a), mont(b)
    tr = gm.Transcript(LABEL)
    proof = gm.InnerProductProof.new(tr, crs, am, bm)
    tr.free()
    ca, cb, y = crs.commit_g1(am), crs.commit_g2(bm), fr_from_int(X.ip(a, b))
    out = [Case(f"d{d}", proof, ca, cb, y, True), Case(f"d{d} wrong y", proof, ca, cb, fr_from_int((X.ip(a, b) + 1) % R), False),
           Case(f"d{d} comm_a of b", proof, crs.commit_g1(bm), cb, y, False), Case(f"d{d} comm_b of a", proof, ca, crs.commit_g2(am), y, False)]
    f = proof.fields()
    e2 = gp.gt_from_ints(X.gt_ints(2))
    for i, h in sorted({(0, 0), (f.rounds - 1, 1), (min(1, f.rounds - 1), 0)}):
        g = proof.fields()
        g.messages[i, h] = gp.gt_mul(g.messages[i, h], e2)
        out.append(Case(f"d{d} message {i}.{h}", gm.InnerProductProof.from_fields(g), ca, cb, y, False))
    g = proof.fields()
    g.foldings_ff[0] = fr_from_int((fr_to_int(g.foldings_ff[0]) + 1) % R)
    out.append(Case(f"d{d} foldings_ff", gm.InnerProductProof.from_fields(g), ca, cb, y, False))
    if f.rounds > 1:
        g = proof.fields()
        g.final_lhs[0] = g.final_lhs[1]
        out.append(Case(f"d{d} final folding", gm.InnerProductProof.from_fields(g), ca, cb, y, False))
        g = proof.fields()
        g.challenges[0] = fr_from_int((fr_to_int(g.challenges[0]) + 1) % R)
        out.append(Case(f"d{d} challenge", gm.InnerProductProof.from_fields(g), ca, cb, y, False))
    return out


def singles(cases, vrs):
    return [c.proof.verify_transcript(vrs, c.comm_a, c.comm_b, c.y) for c in cases]


def many(gm, cases, vrs):
    return gm.InnerProductProof.verify_many([c.proof for c in cases], vrs, np.stack([c.comm_a for c in cases]), np.stack([c.comm_b for c in cases]),
                                            np.stack([c.y for c in cases]))


def free_all(cases, *others):
    for h in {c.proof.handle: c.proof for c in cases}.values():
        h.free()
    for o in others:
        o.free()


@pytest.fixture(scope="module")
def mixed(gm):
    """the CRS of 128 points, its Vrs, and the device proofs of every d with their tampered copies; the verdicts of the single entry"""
    ref = reference(64, 128)
    crs = gm.Crs(ref["r1"], ref["r2"])
    vrs = gm.Vrs(crs)
    cases = [c for d in DS for c in device_cases(gm, crs, d)]
    single = singles(cases, vrs)
    yield crs, vrs, cases, single
    free_all(cases, vrs, crs)


def test_mixed_rounds_in_one_call(gm, mixed):
    _, vrs, cases, single = mixed
    assert single == [c.expect for c in cases], [c.name for c, s in zip(cases, single) if s != c.expect]
    got = many(gm, cases, vrs)
    assert got == single, [c.name for c, g, s in zip(cases, got, single) if g != s]
    assert gm.ipa.verify_many_path() == (len(cases), 0)  # every element is a member: all on the batched path
    perm = np.random.default_rng(0x9E37).permutation(len(cases))
    assert many(gm, [cases[i] for i in perm], vrs) == [single[i] for i in perm]


def test_one_proof_and_none(gm, mixed):
    _, vrs, cases, single = mixed
    lib = gm.capi.load()
    try:
        gm.ipa.set_verify_many_min(1)  # S = 1 on the batched path too
        for k in (0, 1, len(cases) - 1):
            assert many(gm, cases[k:k + 1], vrs) == single[k:k + 1], cases[k].name
            assert gm.ipa.verify_many_path() == (1, 0)
    finally:
        gm.ipa.set_verify_many_min(default_min())
    assert gm.InnerProductProof.verify_many([], vrs, np.zeros((0, 18), np.uint64), np.zeros((0, 36), np.uint64), np.zeros((0, 4), np.uint64)) == []
    assert lib.gm_ipa_verify_many(None, C.c_uint64(vrs.handle), None, None, None, C.c_size_t(0), None) == 0
    assert gm.ipa.verify_many_path() == (0, 0)


def test_the_knob_does_not_change_verdicts(gm, mixed):
    _, vrs, cases, single = mixed
    sub = cases[::3]
    exp = single[::3]
    try:
        gm.ipa.set_verify_many_min(0)
        assert many(gm, sub, vrs) == exp and gm.ipa.verify_many_path() == (len(sub), 0)
        gm.ipa.set_verify_many_min(len(sub) + 1)
        assert many(gm, sub, vrs) == exp and gm.ipa.verify_many_path() == (0, len(sub))
    finally:
        gm.ipa.set_verify_many_min(default_min())


@pytest.mark.parametrize("d,n,special", [(2, 4, False), (3, 4, False), (4, 8, False), (5, 16, False), (8, 16, True)], ids=["d2n4", "d3n4", "d4n8", "d5n16", "special"])
def test_own_crs(gm, d, n, special):
    """the shapes over a CRS of their own length (the Vrs has exactly rounds - 1 levels, none for d = 2); special: points at infinity at
    1 and 6 of the CRS, zeros among the scalars"""
    ref = reference(d, n, special)
    crs = gm.Crs(ref["r1"], ref["r2"])
    vrs = gm.Vrs(crs)
    cases = device_cases(gm, crs, d, (0, 3) if special else ())
    single = singles(cases, vrs)
    assert single == [c.expect for c in cases], [c.name for c, s in zip(cases, single) if s != c.expect]
    assert many(gm, cases, vrs) == single
    assert gm.ipa.verify_many_path() == (len(cases), 0)
    free_all(cases, vrs, crs)


def test_the_vrs_of_another_crs(gm, mixed):
    """the same points in another order: every proof is rejected, as the single entry rejects it"""
    _, _, cases, _ = mixed
    ref = reference(64, 128)
    crs2 = gm.Crs(ref["r1"][::-1].copy(), ref["r2"][::-1].copy())
    vrs2 = gm.Vrs(crs2)
    sub = [c for c in cases if c.expect and c.proof.fields().rounds > 1]
    assert len(sub) == 4
    assert many(gm, sub, vrs2) == singles(sub, vrs2) == [False] * 4
    vrs2.free()
    crs2.free()


def fq_one_mont() -> np.ndarray:
    return np.array(gp.gt_one()[:6])


def test_elements_outside_their_groups_take_the_single_path(gm, mixed):
    """a non-member message, a final folding on the curve but outside G1, a coordinate >= q: the verdict is the single entry's and
    exactly these proofs are reported on the per-proof path"""
    _, vrs, cases, single = mixed
    base = next(c for c in cases if c.name == "d5")
    rng = np.random.default_rng(0x0BAD)
    g = base.proof.fields()
    g.messages[1, 0] = nonmembers(rng, 5)[0]
    bad_gt = Case("non-member message", gm.InnerProductProof.from_fields(g), base.comm_a, base.comm_b, base.y, None)
    g = base.proof.fields()
    outside = pr.g1_random_curve_points(1)[0]  # on the curve, not in G1
    g.final_lhs[2] = np.concatenate([g1_points_to_affine([outside])[0][:12], fq_one_mont()])
    bad_g1 = Case("final folding outside G1", gm.InnerProductProof.from_fields(g), base.comm_a, base.comm_b, base.y, None)
    g = base.proof.fields()
    q5 = pr.Q + 5
    g.final_rhs[1][:6] = [(q5 >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(6)]
    bad_q = Case("coordinate >= q", gm.InnerProductProof.from_fields(g), base.comm_a, base.comm_b, base.y, None)
    good = [next(c for c in cases if c.name == name) for name in ("d2", "d64", "d4 wrong y")]
    lot = [good[0], bad_gt, good[1], bad_g1, bad_q, good[2]]
    exp = singles(lot, vrs)
    assert exp[0] and exp[2] and not exp[5]
    assert not bad_gt.proof.check_messages().ok and not bad_g1.proof.check_points().ok and not bad_q.proof.check_points().ok
    assert many(gm, lot, vrs) == exp
    assert gm.ipa.verify_many_path() == (3, 3)
    # a commitment outside G1 is the caller's element: the same rule
    off = Case("comm_a outside G1", base.proof, np.concatenate([g1_points_to_affine([outside])[0][:12], fq_one_mont()]), base.comm_b, base.y, None)
    lot2 = [good[0], off]
    assert many(gm, lot2, vrs) == singles(lot2, vrs)
    assert gm.ipa.verify_many_path() == (1, 1)
    for c in (bad_gt, bad_g1, bad_q):
        c.proof.free()


def test_stated_terms_equal_the_python_statement(gm, mixed):
    """gm_debug_ipa_stated_terms: the exponents the host part states, against tests/ipa_flat_ref.py on the proof's own scalars"""
    _, _, cases, _ = mixed
    for c in cases:
        if not c.expect:
            continue
        f = c.proof.fields()
        logs = {"challenges": [fr_to_int(x) for x in f.challenges], "batch_challenges": [fr_to_int(x) for x in f.batch_challenges],
                "foldings_ff": (fr_to_int(f.foldings_ff[0]), fr_to_int(f.foldings_ff[1])), "foldings_fg1": (None, fr_to_int(f.foldings_fg1[1])),
                "foldings_fg2": (fr_to_int(f.foldings_fg2[0]), None)}
        gt, pair = c.proof.stated_terms(c.y)
        assert len(gt) == 6 * f.rounds - 4 and len(pair) == 2 * f.rounds + 4
        assert (gt, pair) == F.exponents(logs, fr_to_int(c.y)), c.name


def test_refusals(gm, mixed):
    crs, vrs, cases, _ = mixed
    lib, ptr = gm.capi.load(), gm.capi.ptr
    sub = [c for c in cases if c.expect][:3]
    hs = np.array([c.proof.handle for c in sub], dtype=np.uint64)
    ca, cb, y = np.stack([c.comm_a for c in sub]), np.stack([c.comm_b for c in sub]), np.stack([c.y for c in sub])
    ok = np.zeros(3, dtype=np.intc)

    def call(handles, vh, pa=ptr(ca), pok=ptr(ok)):
        return lib.gm_ipa_verify_many(ptr(handles), C.c_uint64(vh), pa, ptr(cb), ptr(y), C.c_size_t(3), pok)

    assert call(hs, vrs.handle) == 0 and list(ok) == [1, 1, 1]
    stale = hs.copy()
    stale[1] = vrs.handle  # a handle of another kind in the middle
    assert call(stale, vrs.handle) == GM_EHANDLE
    gone = gm.InnerProductProof.from_fields(sub[0].proof.fields())
    stale[1] = gone.handle
    gone.free()
    assert call(stale, vrs.handle) == GM_EHANDLE
    assert call(hs, crs.handle) == GM_EHANDLE
    assert call(hs, vrs.handle, pa=None) == GM_EINVAL and call(hs, vrs.handle, pok=None) == GM_EINVAL
    assert lib.gm_ipa_verify_many(None, C.c_uint64(vrs.handle), ptr(ca), ptr(cb), ptr(y), C.c_size_t(3), ptr(ok)) == GM_EINVAL
    # a Vrs too shallow for ONE of the proofs (d = 2 needs no level, d = 3 one)
    ref = reference(64, 128)
    tiny = gm.Crs(ref["r1"][:2], ref["r2"][:2])
    tiny_vrs = gm.Vrs(tiny)
    assert tiny_vrs.levels == 0 and sub[0].proof.fields().rounds == 1 and sub[1].proof.fields().rounds == 2
    assert call(hs, tiny_vrs.handle) == GM_EINVAL
    assert lib.gm_debug_ipa_verify_many_path(None) == GM_EINVAL
    tiny_vrs.free()
    tiny.free()


def test_two_threads(gm, mixed):
    _, vrs, cases, single = mixed
    lots = [list(range(0, len(cases), 4)), list(range(1, len(cases), 5))]
    got, errs = [None, None], []

    def run(t):
        try:
            got[t] = many(gm, [cases[i] for i in lots[t]], vrs)
        except Exception as e:  # noqa: BLE001 -- reported below with the thread index
            errs.append((t, e))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errs, errs
    for t in range(2):
        assert got[t] == [single[i] for i in lots[t]], t
