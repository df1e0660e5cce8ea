"""G2 keys from bytes on the device, resident keys back to bytes, and the check entries of what a verifier consumes: gm_debug_fq2_sqrt,
gm_g2_bases_from_bytes, gm_g1_bases_to_bytes / gm_g2_bases_to_bytes, gm_crs_from_bases, gm_crs_check, gm_vk_check,
gm_snark_proof_check, gm_psnark_proof_check, gm_ipa_check.

The definition of the encodings is gemini_amd/g2.py on Python integers (tests/test_g2_wire_cpu.py); every compare here is exact:
records, status bytes, first_bad, ok, bytes.  Valid points are members by construction (multiples of the generator), so only the
planted encodings go through the definition's subgroup ladder, once each."""
import copy
import ctypes as C
import functools
import random

import numpy as np
import pytest

from gemini_amd import capi, g2, wire
from gemini_amd.fr import R_MOD
from gemini_amd.kzg import VerifierKey, g2_records
from gemini_amd.points import (check_proof, debug_fq2_sqrt, g1_bases_from_bytes, g1_bases_to_bytes, g2_bases_from_bytes, g2_bases_to_bytes)
from oracle import oracle as orc
from tests import g2_ref
from tests import points_ref as pr
from tests.g2_cases import g2_bytes, rejection_cases
from tests.points_cases import g1_bytes

pytestmark = pytest.mark.gpu

GM_EINVAL, GM_EHANDLE = -1, -3
Q = pr.Q
RINV = pow(1 << 384, -1, Q)
FORMATS = [(c, e) for e in (0, 1) for c in (True, False)]
IDS = [f"{'compressed' if c else 'uncompressed'}-{'zcash' if e else 'arkworks'}" for c, e in FORMATS]


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


# ---- gm_debug_fq2_sqrt -------------------------------------------------------------------------------------------------------------
def f2_limbs(a) -> list:
    return pr.fq_limbs(pr.fq_mont(a[0])) + pr.fq_limbs(pr.fq_mont(a[1]))


def f2_from_limbs(row) -> tuple:
    v = [sum(int(w) << (64 * i) for i, w in enumerate(row[6 * c: 6 * c + 6])) for c in (0, 1)]
    assert v[0] < Q and v[1] < Q  # the device hands out fully reduced limbs
    return (v[0] * RINV % Q, v[1] * RINV % Q)


def delta_is_residue(a) -> bool:
    """which way the root's w^2 = +-delta branch goes for a square a with a1 != 0, whichever root of the norm the device takes"""
    s = pr.fq_sqrt((a[0] * a[0] + a[1] * a[1]) % Q)
    return pow((a[0] + s) * pow(2, -1, Q) % Q, (Q - 1) // 2, Q) == 1


@functools.lru_cache(maxsize=None)
def sqrt_inputs():
    """257 elements of Fq2 and whether each is a square"""
    rng = random.Random(0x5172)
    g = (1, 1)  # no square: its norm 2 is a non-residue of Fq (q = 3 mod 8)
    assert pr.f2_sqrt(g) is None
    res, non = 4, 5
    assert pr.fq_sqrt(res) is not None and pr.fq_sqrt(non) is None
    fixed = [(0, 0), (1, 0), (Q - 1, 0), (0, 1), (0, Q - 1),
             (res, 0), (non, 0),  # a real residue; a real non-residue, whose root is purely imaginary
             (0, res), (0, non), (0, Q - res)]  # purely imaginary, over a residue and over a non-residue: squares both (the norm is c^2)
    out = [(a, pr.f2_sqrt(a) is not None) for a in fixed]
    assert all(sq for a, sq in out)  # every element of Fq, and every multiple of u, is a square of Fq2
    while len(out) < 257:
        b = (rng.randrange(Q), rng.randrange(Q))
        sq = g2.f2_mul(b, b)
        out.append((sq, True))
        out.append((g2.f2_mul(sq, g), False))
    out = out[:257]
    for a, sq in out[:16]:
        assert (pr.f2_sqrt(a) is not None) == sq
    return tuple(out)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_fq2_sqrt(gm, n):
    cases = sqrt_inputs()[-n:] if n < 64 else sqrt_inputs()[:n]  # the short runs take random elements, the long ones start with the fixed list
    if n == 1:
        cases = sqrt_inputs()[6:7]  # the real non-residue: a purely imaginary root
    a = np.array([f2_limbs(c[0]) for c in cases], dtype=np.uint64)
    root, flag = debug_fq2_sqrt(a)
    assert [int(f) for f in flag] == [int(c[1]) for c in cases]
    for (v, sq), r in zip(cases, root):
        if sq:
            r = f2_from_limbs(r)
            assert g2.f2_mul(r, r) == v, v
    if n == 1:
        assert f2_from_limbs(root[0])[0] == 0
    if n >= 63:  # both sides of the w^2 = delta / w^2 = -delta branch occur among the squares
        sides = {delta_is_residue(v) for v, sq in cases if sq and v[1]}
        assert sides == {True, False}


def test_fq2_sqrt_of_curve_right_hand_sides(gm):
    """x = (k, 0), k = 1 .. 40: the 15 / 25 split of x^3 + 4 (1 + u)"""
    rhs = [g2.f2_add(g2.f2_mul(g2.f2_mul((k, 0), (k, 0)), (k, 0)), (4, 4)) for k in range(1, 41)]
    root, flag = debug_fq2_sqrt(np.array([f2_limbs(v) for v in rhs], dtype=np.uint64))
    assert [bool(f) for f in flag] == [pr.f2_sqrt(v) is not None for v in rhs] and int(flag.sum()) == 15


# ---- gm_g2_bases_from_bytes --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def g2_members():
    """200 members of G2: multiples of the generator with both signs of y, and the identity twice"""
    pts = list(g2_ref.chain(200))
    pts[0], pts[1] = pr.G2_GEN, pr.g2_neg(pr.G2_GEN)
    for i in range(5, 200, 3):
        pts[i] = pr.g2_neg(pts[i])
    pts[3] = pts[66] = None
    larger = [g2._f2_gt(p[1], g2.f2_neg(p[1])) for p in pts if p is not None]
    assert any(larger) and not all(larger)
    return tuple(pts)


@functools.lru_cache(maxsize=None)
def defined_status(one: bytes, compress: bool, enc: int, validate: bool) -> int:
    """what the Python definition makes of one encoding: 0 or the status of its WireError"""
    try:
        g2.deserialize(one, 0, compress, enc, validate=validate)
        return 0
    except wire.WireError as e:
        return e.status


def records_of(pts) -> np.ndarray:
    return np.array([pr.g2_record(p) for p in pts], dtype=np.uint64)


@pytest.mark.parametrize("validate", [True, False], ids=["validate", "novalidate"])
@pytest.mark.parametrize("compress,enc", FORMATS, ids=IDS)
@pytest.mark.parametrize("n", [1, 64, 65, 200])
def test_g2_from_bytes(gm, n, compress, enc, validate):
    pts = list(g2_members()[:n]) if n > 1 else [g2_members()[4]]
    good = [g2_bytes(p, compress, enc) for p in pts]
    size = g2.g2_size(compress)
    # the definition reads the same points back (validate=False: members by construction; the device validates below)
    assert [g2.deserialize(b, 0, compress, enc, validate=False)[0] for b in good[:8]] == pts[:8]
    bases, res = g2_bases_from_bytes(b"".join(good), n, compress, enc, validate)
    assert res.ok and res.first_bad == n and not res.status.any() and bases is not None and bases.handle != 0
    try:
        assert (bases.download() == records_of(pts)).all()
    finally:
        bases.free()

    # one of each rejection class: at the first, a middle and the last index, the rest spread between
    cases = rejection_cases(compress, enc)
    rot = (n + 2 * enc + int(compress)) % len(cases)
    cases = cases[rot:] + cases[:rot]
    if n == 1:  # room for one: a class that this mode rejects
        cases.sort(key=lambda c: defined_status(c[1], compress, enc, validate) == 0)
    spots = [0, n // 2, n - 1] + [1 + 3 * k for k in range(len(cases))]
    spots = [i for k, i in enumerate(spots) if 0 <= i < n and i not in spots[:k]][: len(cases)]
    data, want = list(good), np.zeros(n, dtype=np.uint8)
    for i, (name, one, status) in zip(spots, cases):
        data[i] = one
        want[i] = defined_status(one, compress, enc, validate)
        assert want[i] == (status if validate or status in (1, 2) or (status == 3 and compress) else 0), name
    assert want.any()
    before = capi.mem_stats()
    buf = np.frombuffer(b"".join(data), dtype=np.uint8)
    assert len(buf) == n * size
    st = np.full(n, 0xEE, dtype=np.uint8)
    h, fb, ok = C.c_uint64(0xFEEDFACE), C.c_size_t(n + 1), C.c_int(1)
    rc = capi.load().gm_g2_bases_from_bytes(capi.ptr(buf), C.c_size_t(n), C.c_int(int(compress)), C.c_int(enc), C.c_int(int(validate)), C.byref(h), capi.ptr(st),
                                            C.byref(fb), C.byref(ok))
    assert rc == 0 and ok.value == 0 and h.value == 0 and fb.value == int(np.flatnonzero(want)[0])
    assert (st == want).all(), [(i, int(st[i]), int(want[i])) for i in np.flatnonzero(st != want)[:8]]
    after = capi.mem_stats()
    assert after["keys"] == before["keys"] and after["in_use"] == before["in_use"], (before, after)
    if not validate and n >= 64:
        # what validate=False lets through is decoded to the point the definition reads: a curve point outside G2, and for the
        # uncompressed framings the point off the twist
        kept = [(i, one) for i, (name, one, status) in zip(spots, cases) if want[i] == 0]
        assert kept
        data2, pts2 = list(good), list(pts)
        for i, one in kept:
            data2[i] = one
            pts2[i] = g2.deserialize(one, 0, compress, enc, validate=False)[0]
        bases, res = g2_bases_from_bytes(b"".join(data2), n, compress, enc, False)
        assert res.ok and bases is not None
        try:
            assert (bases.download() == records_of(pts2)).all()
            assert not bases.check().ok and bases.check().first_bad == min(i for i, _ in kept)
        finally:
            bases.free()


@pytest.mark.parametrize("enc", [0, 1], ids=["arkworks", "zcash"])
def test_g2_from_bytes_real_x(gm, enc):
    """x = (k, 0), k = 1 .. 40 under both sign flags: 15 decode to the root the flag names, 25 are NOT_ON_CURVE"""
    data, want, pts = [], [], []
    for k in range(1, 41):
        for larger in (False, True):
            one = bytearray(g2.serialize_compressed(((k, 0), (0, 1)), enc))
            if larger:
                one[95 if enc == 0 else 0] |= 0x80 if enc == 0 else 0x20
            data.append(bytes(one))
            want.append(defined_status(bytes(one), True, enc, False))
            pts.append(g2.deserialize(bytes(one), 0, True, enc, validate=False)[0] if want[-1] == 0 else None)
    assert want.count(0) == 30 and want.count(3) == 50
    bases, res = g2_bases_from_bytes(b"".join(data), 80, True, enc, False)
    assert bases is None and [int(s) for s in res.status] == want and res.first_bad == want.index(3)
    on = [i for i, w in enumerate(want) if w == 0]
    bases, res = g2_bases_from_bytes(b"".join(data[i] for i in on), len(on), True, enc, False)
    assert res.ok
    try:
        assert (bases.download() == records_of([pts[i] for i in on])).all()
    finally:
        bases.free()
    _, res = g2_bases_from_bytes(b"".join(data[i] for i in on), len(on), True, enc, True)  # none of them is in G2
    assert not res.ok and (res.status == 4).all()


# ---- to_bytes and the round trips ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def g1_members():
    orc.build()
    rec = orc.g1_fixed_base_mul(orc.g1_generator(), orc.random_fr(0x9018, 70))
    rec[1] = pr.g1_record(pr.g1_neg(pr.G1_GEN))
    rec[7] = 0
    pts = [None if not r.any() else orc.affine_to_ints(r) for r in rec]
    return rec, pts


@pytest.mark.parametrize("compress,enc", FORMATS, ids=IDS)
def test_round_trips(gm, compress, enc):
    rec1, pts1 = g1_members()
    pts2 = list(g2_members()[:70])
    rec2 = records_of(pts2)
    k1, k2 = gm.G1Bases.register(rec1), gm.G2Bases.register(rec2)
    try:
        off, n = 3, 65  # strictly inside the handle, across a wave of the decoder
        b1, b2 = k1.to_bytes(compress, enc, off, n), k2.to_bytes(compress, enc, off, n)
        assert b1 == b"".join(g1_bytes(p, compress, enc) for p in pts1[off: off + n])
        assert b2 == b"".join(g2_bytes(p, compress, enc) for p in pts2[off: off + n])
        assert g1_bases_to_bytes(k1, compress, enc) == b"".join(g1_bytes(p, compress, enc) for p in pts1)
        assert g2_bases_to_bytes(k2, compress, enc, 69, 1) == g2_bytes(pts2[69], compress, enc)
        assert k1.to_bytes(compress, enc, 70, 0) == b"" and k2.to_bytes(compress, enc, 0, 0) == b""
        back1, r1 = g1_bases_from_bytes(b1, n, compress, enc)
        back2, r2 = gm.G2Bases.from_bytes(b2, n, compress, enc)
        assert r1.ok and r2.ok
        try:
            assert (back1.download() == rec1[off: off + n]).all() and (back2.download() == rec2[off: off + n]).all()
        finally:
            back1.free()
            back2.free()
    finally:
        k1.free()
        k2.free()


@pytest.mark.parametrize("enc", [0, 1], ids=["arkworks", "zcash"])
def test_vk_g2_bytes_decode_to_the_keys_records(gm, enc):
    tau = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100ABCD % R_MOD
    vk = VerifierKey.from_trapdoor(orc.ints_to_limbs([tau], 4)[0], 3)
    try:
        raw = vk.powers_of_g2_bytes(enc=enc)
        assert vk.check().ok
    finally:
        vk.free()
    assert int.from_bytes(raw[:8], "little") == 4
    bases, res = g2_bases_from_bytes(raw[8:], 4, False, enc, True)
    assert res.ok
    try:
        assert (bases.download() == g2_records([g2.mul(g2.generator(), pow(tau, i, R_MOD)) for i in range(4)])).all()
    finally:
        bases.free()


# ---- gm_crs_from_bases, gm_crs_check, gm_vk_check -----------------------------------------------------------------------------------
def fields_equal(a, b) -> bool:
    return a.rounds == b.rounds and all(np.array_equal(x, y) for x, y in (
        (a.messages, b.messages), (a.challenges, b.challenges), (a.batch_challenges, b.batch_challenges), (a.final_lhs, b.final_lhs), (a.final_rhs, b.final_rhs),
        (a.foldings_ff, b.foldings_ff), (a.foldings_fg1[0], b.foldings_fg1[0]), (a.foldings_fg1[1], b.foldings_fg1[1]), (a.foldings_fg2[0], b.foldings_fg2[0]),
        (a.foldings_fg2[1], b.foldings_fg2[1])))


def test_crs_from_bases(gm):
    from tests.test_gpu_ipa import LABEL, reference

    ref = reference(8, 16)
    r1, r2 = np.array(ref["r1"]), np.array(ref["r2"])
    k1, k2 = gm.G1Bases.register(r1), gm.G2Bases.register(r2)
    old = gm.Crs(r1, r2)
    new = gm.Crs.from_bases(k1, k2)
    decoded, c1, c2 = gm.Crs.from_bytes(k1.to_bytes(True, 1), 16, k2.to_bytes(True, 1), 16, True, 1)
    k1.free()  # the handles stay the caller's: the CRS holds copies
    k2.free()
    assert c1.ok and c2.ok and (new.n1, new.n2) == (decoded.n1, decoded.n2) == (16, 16)
    try:
        want = None
        for crs in (old, new, decoded):
            assert crs.check().ok
            tr = gm.Transcript(LABEL)
            proof = gm.InnerProductProof.new(tr, crs, ref["a_mont"], ref["b_mont"])
            got = (crs.commit_g1(ref["a_mont"]), crs.commit_g2(ref["b_mont"]), proof.fields())
            vrs = gm.Vrs(crs)
            assert proof.check_points().ok
            assert proof.verify_transcript(vrs, got[0], got[1], gm.fr.fr_from_int(ref["y"]))
            for o in (vrs, proof, tr):
                o.free()
            if want is None:
                want = got
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and fields_equal(got[2], want[2])
    finally:
        for crs in (old, new, decoded):
            crs.free()


@functools.lru_cache(maxsize=None)
def outsiders():
    """curve points outside the subgroups, checked once with the ladder"""
    p1, p2 = pr.g1_random_curve_points(1)[0], pr.g2_random_curve_points(1)[0]
    assert pr.g1_on_curve(p1) and not pr.g1_in_subgroup_ladder(p1) and pr.g2_on_curve(p2) and not pr.g2_in_subgroup_ladder(p2)
    return p1, p2


@pytest.mark.parametrize("kind", ["crs", "vk"])
def test_key_checks_name_the_group_and_the_index(gm, kind):
    rec1, _ = g1_members()
    rec1 = rec1[:9].copy()
    rec2 = records_of(g2_members()[:9])
    p1, p2 = outsiders()
    make = (lambda a, b: gm.Crs(a, b)) if kind == "crs" else (lambda a, b: VerifierKey.from_powers(a, b))  # noqa: E731
    key = make(rec1, rec2)
    res = key.check()
    key.free()
    assert res.ok and (res.first_bad_g1, res.first_bad_g2) == (9, 9)
    bad1 = rec1.copy()
    bad1[5] = np.array(pr.g1_record(p1), dtype=np.uint64)
    key = make(bad1, rec2)
    res = key.check()
    key.free()
    assert not res.ok and (res.first_bad_g1, res.first_bad_g2) == (5, 9)
    bad2 = rec2.copy()
    bad2[8] = np.array(pr.g2_record(p2), dtype=np.uint64)
    key = make(rec1, bad2)
    res = key.check()
    key.free()
    assert not res.ok and (res.first_bad_g1, res.first_bad_g2) == (9, 8)


# ---- the group elements of a proof ----------------------------------------------------------------------------------------------------
LAMBDA = 0xABCDEF0123456789  # a non-trivial Jacobian representative: (x l^2, y l^3, l)


def g1_jac(p, lam=LAMBDA) -> np.ndarray:
    x, y = p
    return np.array(sum((pr.fq_limbs(pr.fq_mont(v)) for v in (x * lam * lam % Q, y * pow(lam, 3, Q) % Q, lam)), []), dtype=np.uint64)


def g2_jac(p, lam=(LAMBDA, 3)) -> np.ndarray:
    l2 = g2.f2_mul(lam, lam)
    X, Y = g2.f2_mul(p[0], l2), g2.f2_mul(p[1], g2.f2_mul(l2, lam))
    return np.array(sum((pr.fq_limbs(pr.fq_mont(v)) for v in (X[0], X[1], Y[0], Y[1], lam[0], lam[1])), []), dtype=np.uint64)


def bad_g1_elements():
    p1, _ = outsiders()
    off = (p1[0], (p1[1] + 1) % Q)
    assert not pr.g1_on_curve(off)
    return [g1_jac(p1), g1_jac(off)]


def test_snark_proof_check(gm, oracle, pyref):
    from tests.test_gpu_verifier import _snark_case

    proof = _snark_case(gm, oracle, pyref, "dummy", 1 << 3)["proof"]
    nf = len(proof.tensorcheck_proof.folded_polynomials_commitments)
    assert nf >= 2
    res = proof.check_points()
    assert res.ok and res.first_bad == nf + 2
    # an honest element in another representative passes
    p = copy.deepcopy(proof)
    p.witness_commitment = g1_jac(orc.affine_to_ints(orc.g1_to_affine(np.asarray(proof.witness_commitment, dtype=np.uint64))))
    assert p.check_points().ok
    for bad in bad_g1_elements():
        for slot in range(nf + 2):
            p = copy.deepcopy(proof)
            if slot == 0:
                p.witness_commitment = bad
            elif slot == nf + 1:
                p.tensorcheck_proof.evaluation_proof = bad
            else:
                p.tensorcheck_proof.folded_polynomials_commitments[slot - 1] = bad
            res = p.check_points()
            assert not res.ok and res.first_bad == slot
    p = copy.deepcopy(proof)  # a coordinate >= q has no value: reported, not reduced
    p.tensorcheck_proof.evaluation_proof = np.full(18, 2**64 - 1, dtype=np.uint64)
    res = p.check_points()
    assert not res.ok and res.first_bad == nf + 1


def test_psnark_proof_check(gm, oracle, pyref):
    from tests.test_gpu_verifier import _psnark_case

    proof = _psnark_case(gm, oracle, pyref, "dummy", 1 << 3)["proof"]
    nf = len(proof.tensorcheck_proof.folded_polynomials_commitments)
    res = proof.check_points()
    assert res.ok and res.first_bad == 19 + nf

    def put(p, slot, v):
        if slot == 0:
            p.witness_commitment = v
        elif slot <= 3:
            p.r_star_commitments[slot - 1] = v
        elif slot == 4:
            p.z_star_commitment = v
        elif slot <= 7:
            setattr(p, ("sorted_r_commitment", "sorted_alpha_commitment", "sorted_z_commitment")[slot - 5], v)
        elif slot <= 16:
            p.ep_msgs.acc_v_commitments[slot - 8] = v
        elif slot == 17:
            p.ralpha_star_acc_mu_proof = v
        elif slot < 18 + nf:
            p.tensorcheck_proof.folded_polynomials_commitments[slot - 18] = v
        else:
            p.tensorcheck_proof.evaluation_proof = v

    for bad in bad_g1_elements():
        for slot in (0, 2, 4, 6, 16, 17, 18, 18 + nf):
            p = copy.deepcopy(proof)
            put(p, slot, bad)
            res = p.check_points()
            assert not res.ok and res.first_bad == slot, slot


def test_ipa_check(gm):
    from tests.test_gpu_ipa import prove_on_device, reference

    crs, tr, proof = prove_on_device(gm, reference(4, 8))
    f = proof.fields()
    k = 2 * (f.rounds - 1)
    assert k == 2
    res = proof.check_points()
    assert res.ok and res.first_bad == 2 * (1 + k)
    p1, p2 = outsiders()
    off1 = (p1[0], (p1[1] + 1) % Q)
    off2 = (p2[0], ((p2[1][0] + 1) % Q, p2[1][1]))
    assert not pr.g1_on_curve(off1) and not pr.g2_on_curve(off2)
    for b1, b2 in ((g1_jac(p1), g2_jac(p2)), (g1_jac(off1), g2_jac(off2))):
        for slot in range(2 * (1 + k)):
            g = proof.fields()
            if slot == 0:
                g.foldings_fg1 = (b1, g.foldings_fg1[1])
            elif slot <= k:
                g.final_lhs[slot - 1] = b1
            elif slot == 1 + k:
                g.foldings_fg2 = (g.foldings_fg2[0], b2)
            else:
                g.final_rhs[slot - 2 - k] = b2
            bad = gm.InnerProductProof.from_fields(g)
            res = bad.check_points()
            bad.free()
            assert not res.ok and res.first_bad == slot, slot
    for o in (proof, tr, crs):
        o.free()


# ---- fail closed; misuse ---------------------------------------------------------------------------------------------------------------
def test_every_new_entry_fails_closed(gm):
    """a negative return value comes with *ok = 0 (and *handle = 0, *crs = 0) whatever the caller had put there"""
    lib = capi.load()
    rec1, _ = g1_members()
    k1, k2 = gm.G1Bases.register(rec1[:4].copy()), gm.G2Bases.register(records_of(g2_members()[:4]))
    st = np.zeros(4, dtype=np.uint8)
    fb, fb2, ok, h = C.c_size_t(0), C.c_size_t(0), C.c_int(1), C.c_uint64(0xFEEDFACE)
    out = np.zeros(4 * 192, dtype=np.uint8)
    data = np.frombuffer(g2_bytes(pr.G2_GEN, True, 0), dtype=np.uint8)

    def closed(rc, want):
        assert rc == want and ok.value == 0, (rc, want, ok.value)
        ok.value = 1

    try:
        dec = lambda p, n, enc, hp, okp: lib.gm_g2_bases_from_bytes(p, C.c_size_t(n), C.c_int(1), C.c_int(enc), C.c_int(1), hp, capi.ptr(st), C.byref(fb), okp)  # noqa: E731
        for args in ((capi.ptr(data), 1, 2), (None, 1, 0), (capi.ptr(data), (1 << 64) // 192 + 1, 0)):  # unknown framing; null bytes; a size that overflows
            h.value = 0xFEEDFACE
            closed(dec(*args, C.byref(h), C.byref(ok)), GM_EINVAL)
            assert h.value == 0
        h.value = 0xFEEDFACE
        closed(dec(capi.ptr(data), 1, 0, None, C.byref(ok)), GM_EINVAL)
        assert dec(capi.ptr(data), 1, 0, C.byref(h), None) == GM_EINVAL and h.value == 0

        enc1 = lambda hh, off, n, enc, p, cap: lib.gm_g1_bases_to_bytes(C.c_uint64(hh), C.c_size_t(off), C.c_size_t(n), C.c_int(1), C.c_int(enc), p, C.c_size_t(cap))  # noqa: E731
        enc2 = lambda hh, off, n, enc, p, cap: lib.gm_g2_bases_to_bytes(C.c_uint64(hh), C.c_size_t(off), C.c_size_t(n), C.c_int(1), C.c_int(enc), p, C.c_size_t(cap))  # noqa: E731
        for fn, good, other in ((enc1, k1.handle, k2.handle), (enc2, k2.handle, k1.handle)):
            assert fn(good, 0, 4, 0, capi.ptr(out), len(out)) == 0
            assert fn(good, 3, 2, 0, capi.ptr(out), len(out)) == GM_EINVAL      # a range outside the handle
            assert fn(good, 5, 0, 0, capi.ptr(out), len(out)) == GM_EINVAL
            assert fn(good, 0, 4, 2, capi.ptr(out), len(out)) == GM_EINVAL      # unknown framing
            assert fn(good, 0, 4, 0, None, len(out)) == GM_EINVAL               # null
            assert fn(good, 0, 4, 0, capi.ptr(out), 4 * 48 - 1) == GM_EINVAL    # too small for either group
            assert fn(other, 0, 1, 0, capi.ptr(out), len(out)) == GM_EHANDLE    # a handle of the other group
            assert fn(0xDEAD0021, 0, 1, 0, capi.ptr(out), len(out)) == GM_EHANDLE

        for a, b in ((0xDEAD0022, k2.handle), (k1.handle, 0xDEAD0023), (k2.handle, k1.handle)):
            h.value = 0xFEEDFACE
            assert lib.gm_crs_from_bases(C.c_uint64(a), C.c_uint64(b), C.byref(h)) == GM_EHANDLE and h.value == 0
        assert lib.gm_crs_from_bases(C.c_uint64(k1.handle), C.c_uint64(k2.handle), None) == GM_EINVAL

        for fn in (lib.gm_crs_check, lib.gm_vk_check):
            closed(fn(C.c_uint64(0xDEAD0024), C.byref(fb), C.byref(fb2), C.byref(ok)), GM_EHANDLE)
        crs = gm.Crs.from_bases(k1, k2)
        assert lib.gm_crs_check(C.c_uint64(crs.handle), None, None, None) == GM_EINVAL
        assert lib.gm_crs_check(C.c_uint64(crs.handle), None, None, C.byref(ok)) == 0 and ok.value == 1  # the indices are optional
        closed(lib.gm_vk_check(C.c_uint64(crs.handle), C.byref(fb), C.byref(fb2), C.byref(ok)), GM_EHANDLE)  # a CRS is no verifier key
        crs.free()

        closed(lib.gm_snark_proof_check(None, C.byref(fb), C.byref(ok)), GM_EINVAL)
        closed(lib.gm_psnark_proof_check(None, C.byref(fb), C.byref(ok)), GM_EINVAL)
        closed(lib.gm_ipa_check(C.c_uint64(0xDEAD0025), C.byref(fb), C.byref(ok)), GM_EHANDLE)
        one = np.array([f2_limbs((4, 0))], dtype=np.uint64)
        assert lib.gm_debug_fq2_sqrt(None, C.c_size_t(1), capi.ptr(one), capi.ptr(st)) == GM_EINVAL
        assert lib.gm_debug_fq2_sqrt(capi.ptr(one), C.c_size_t(1), None, capi.ptr(st)) == GM_EINVAL
        assert lib.gm_debug_fq2_sqrt(None, C.c_size_t(0), None, None) == 0
    finally:
        k1.free()
        k2.free()


def test_mirrors_raise_on_misuse(gm):
    with pytest.raises(capi.GeminiHipError) as e:
        check_proof(capi.load().gm_ipa_check, C.c_uint64(0xDEAD0026))
    assert e.value.code == GM_EHANDLE
    with pytest.raises(capi.GeminiHipError) as e:
        gm.G2Bases(0xDEAD0027, 4).to_bytes(True)
    assert e.value.code == GM_EHANDLE
