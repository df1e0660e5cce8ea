"""GPU: GT element by element on the device -- k_gt_final_exp, k_miller_each, k_gt_check and the five device functions of gt.cuh
(gm_gt_final_exp_many, gm_pairing_each(_h), gm_gt_check, gm_hgt_check, gm_ipa_check_gt, gm_debug_gt_op).

Every compare is bit-exact: against the host entries gm_gt_final_exp / gm_gt_mul / gm_gt_pow / gm_pairing_multi on raw limbs, or on
canonical integers against oracle/pairing.py and the two statements of membership of tests/gt_check_ref.py.

Sizes: n in {0, 1, 2, 63, 64, 65, 130} -- the block edge, a second block, and a block with a two-lane tail (64 lanes per block):
the smallest shapes at which the lane and block indexing can go wrong.  The inputs of a size are the adversarial list of
gt_check_ref.py laid end to end, so members and non-members of every kind sit next to each other inside one block.
"""
import ctypes as C
import threading

import numpy as np
import pytest

from gemini_amd import pairing as gp
from gemini_amd.fr import fr_from_int
from oracle import pairing as OP
from tests import gt_check_ref as ref
from tests.test_gpu_pairing import e_pow, g1_points_to_affine, pts  # noqa: F401  (pts: a fixture)
from tests.test_pairing_cpu import gt_of_w, w_of_gt

pytestmark = pytest.mark.gpu

Q, R = OP.Q, OP.R
SIZES = [0, 1, 2, 63, 64, 65, 130]
GM_EINVAL, GM_EHANDLE = -1, -3
OP_FROB1, OP_FROB2, OP_INV, OP_CYC_SQR, OP_POW_X = range(5)


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


@pytest.fixture(scope="module")
def cases():
    """(names, (m, 72) limbs, expected statuses, host final exponentiations (m, 72)) of the adversarial list: computed once, never
    modified"""
    lst = ref.adversarial()
    x = np.stack([gp.gt_from_ints(c) for _, c, _ in lst])
    fe = np.stack([gp.gt_final_exp(v) for v in x])
    st = np.array([s for _, _, s in lst], dtype=np.uint8)
    for a in (x, fe, st):
        a.setflags(write=False)
    return [n for n, _, _ in lst], x, st, fe


def tiled(a, n: int, shift: int = 0):
    """n rows of `a`, cycling from row `shift`"""
    return a[(np.arange(n) + shift) % len(a)]


def limbs_of(c) -> np.ndarray:
    """12 integers < 2^384 as they are (NOT reduced): (72,) limbs in ark-ff's Montgomery form for those < q, raw limbs otherwise"""
    out = np.zeros(72, dtype=np.uint64)
    for k, v in enumerate(c):
        out[6 * k:6 * k + 6] = gp.gt_from_ints([v % Q] + [0] * 11)[:6] if v < Q else [(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(6)]
    return out


# ---- gm_debug_gt_op: the device functions one by one ---------------------------------------------------------------------------
def test_frobenius_maps(gm, cases):
    _, x, _, _ = cases
    got1, got2 = gp.debug_gt_op(OP_FROB1, x), gp.debug_gt_op(OP_FROB2, x)
    for i in (0, 3, 5, 6, 11, len(x) - 3):  # random, a Miller value, 1, 0, a member, the cyclotomic non-member
        f = w_of_gt(x[i])
        assert w_of_gt(got1[i]) == OP.f12_pow(f, Q), i
        assert w_of_gt(got2[i]) == OP.f12_pow(f, Q * Q), i
    again = gp.debug_gt_op(OP_FROB1, gp.debug_gt_op(OP_FROB1, x))
    assert (again == got2).all()  # on every element of the list


def test_inverse(gm, cases):
    names, x, _, _ = cases
    got = gp.debug_gt_op(OP_INV, tiled(x, 65))
    one = gp.gt_one()
    for i in range(65):
        j = i % len(x)
        if names[j] == "zero":
            assert not got[i].any()
        else:
            assert (gp.gt_mul(got[i], x[j]) == one).all(), names[j]
    for i in (0, 4):
        assert w_of_gt(got[i]) == OP.f12_inv(w_of_gt(x[i]))


def test_cyclotomic_squaring_and_pow_x(gm, cases):
    """on the cyclotomic elements of the list -- members, the non-member g, g^r, member * g^r, 1 -- over two blocks"""
    _, x, st, _ = cases
    cyc = x[(st == ref.OK) | (st == ref.NOT_IN_SUBGROUP)]
    assert len(cyc) >= 8
    inp = tiled(cyc, 66)
    sq, px = gp.debug_gt_op(OP_CYC_SQR, inp), gp.debug_gt_op(OP_POW_X, inp)
    want_sq = [gp.gt_mul(v, v) for v in cyc]
    want_px = [gp.gt_pow(v, ref.X_ABS) for v in cyc]
    for i in range(66):
        assert (sq[i] == want_sq[i % len(cyc)]).all(), i
        assert (px[i] == want_px[i % len(cyc)]).all(), i


def test_debug_op_refusals(gm):
    lib, x = gm.capi.load(), np.zeros((1, 72), dtype=np.uint64)
    assert lib.gm_debug_gt_op(C.c_int(5), gm.capi.ptr(x), C.c_size_t(1), gm.capi.ptr(x)) == GM_EINVAL
    assert lib.gm_debug_gt_op(C.c_int(-1), gm.capi.ptr(x), C.c_size_t(1), gm.capi.ptr(x)) == GM_EINVAL
    assert lib.gm_debug_gt_op(C.c_int(0), None, C.c_size_t(1), gm.capi.ptr(x)) == GM_EINVAL
    assert lib.gm_debug_gt_op(C.c_int(0), None, C.c_size_t(0), None) == 0


# ---- gm_gt_final_exp_many --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_final_exp_many_equals_the_host_function(gm, cases, n):
    """bit for bit gm_gt_final_exp element by element, members or not: the non-cyclotomic inputs prove the easy part, 0 gives 0"""
    _, x, _, fe = cases
    got = gm.gt_final_exp_many(tiled(x, n, shift=n))
    assert got.shape == (n, 72)
    assert (got == tiled(fe, n, shift=n)).all()


def test_final_exp_many_against_the_oracle(gm, cases):
    names, x, _, _ = cases
    pick = [names.index(s) for s in ("random0", "miller0", "one", "member0", "cyclotomic_non_member")]
    got = gm.gt_final_exp_many(x[pick])
    for g, i in zip(got, pick):
        assert w_of_gt(g) == OP.final_exponentiation(w_of_gt(x[i])), names[i]
    lib = gm.capi.load()
    assert lib.gm_gt_final_exp_many(None, C.c_size_t(1), gm.capi.ptr(got)) == GM_EINVAL
    assert lib.gm_gt_final_exp_many(gm.capi.ptr(got), C.c_size_t(1), None) == GM_EINVAL
    assert lib.gm_gt_final_exp_many(None, C.c_size_t(0), None) == 0


# ---- gm_pairing_each / gm_pairing_each_h -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def singles(gm, pts):  # noqa: F811
    """gm_pairing_multi of the single pair i, i < 130: computed once, never modified"""
    _, _, r1, _, _, r2 = pts
    out = np.stack([gm.multi_pairing(r1[i:i + 1], r2[i:i + 1]) for i in range(130)])
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_pairing_each_equals_single_pairings(gm, pts, singles, n):  # noqa: F811
    _, a, r1, _, b, r2 = pts
    got = gm.pairing_each(r1[:n], r2[:n])
    assert got.shape == (n, 72) and (got == singles[:n]).all()
    for i in sorted({0, n // 2, n - 1} & set(range(n))):  # points with known logs: e(a P, b Q) = E^(a b)
        assert w_of_gt(got[i]) == e_pow(a[i] * b[i]), i
    if n:
        res = gm.gt_check(got)
        assert res.ok and res.first_bad == n and not res.status.any()


def test_pairing_each_identity_gives_one(gm, pts, singles):  # noqa: F811
    p1, _, _, p2, _, _ = pts
    from gemini_amd.g2msm import g2_points_to_affine

    q1, q2 = list(p1[:66]), list(p2[:66])
    for i in (0, 63, 65):
        q1[i] = None
    for i in (1, 63, 64):
        q2[i] = None
    got = gm.pairing_each(g1_points_to_affine(q1, flag=True), g2_points_to_affine(q2, flag=True))
    one = gm.gt_one()
    for i in range(66):
        assert (got[i] == (one if i in (0, 1, 63, 64, 65) else singles[i])).all(), i


def test_pairing_each_handles_offsets_steps_and_refusals(gm, pts, singles):  # noqa: F811
    _, _, r1, _, _, r2 = pts
    b1, b2 = gm.G1Bases.register(r1), gm.G2Bases.register(r2)
    assert (gm.pairing_each(b1, b2, 130) == singles).all()
    got = gm.pairing_each(b1, b2, 65, off1=1, step1=2, off2=1, step2=2)  # pairs (1, 1), (3, 3), ..., (129, 129)
    assert (got == singles[1::2]).all()
    got = gm.pairing_each(b1, b2, 3, off1=5, step1=1, off2=7, step2=60)  # e(P_5, Q_7), e(P_6, Q_67), e(P_7, Q_127)
    for k in range(3):
        assert (got[k] == gm.multi_pairing(r1[5 + k:6 + k], r2[7 + 60 * k:8 + 60 * k])).all(), k
    lib, out = gm.capi.load(), np.zeros((132, 72), dtype=np.uint64)

    def call(h1, o1, s1, h2, o2, s2, n, o=out):
        return lib.gm_pairing_each_h(C.c_uint64(h1), C.c_size_t(o1), C.c_size_t(s1), C.c_uint64(h2), C.c_size_t(o2), C.c_size_t(s2), C.c_size_t(n),
                                     gm.capi.ptr(o) if o is not None else None)

    n = len(r1)
    assert call(b1.handle, 0, 1, b2.handle, 0, 1, n) == 0
    assert call(b1.handle, 0, 1, b2.handle, 0, 1, n + 1) == GM_EINVAL
    assert call(b1.handle, 1, 1, b2.handle, 0, 1, n) == GM_EINVAL
    assert call(b1.handle, 0, 1, b2.handle, 0, 2, n // 2 + 1) == GM_EINVAL
    assert call(b1.handle, n, 1, b2.handle, 0, 1, 1) == GM_EINVAL
    assert call(b1.handle, 0, 0, b2.handle, 0, 1, 2) == GM_EINVAL and call(b1.handle, 0, 1, b2.handle, 0, 0, 2) == GM_EINVAL
    assert call(b1.handle, 0, 1, b2.handle, 0, 1, 2, None) == GM_EINVAL
    assert call(b2.handle, 0, 1, b2.handle, 0, 1, 2) == GM_EHANDLE and call(b1.handle, 0, 1, b1.handle, 0, 1, 2) == GM_EHANDLE
    assert call(0xDEAD0031, 0, 1, b2.handle, 0, 1, 2) == GM_EHANDLE
    assert call(b1.handle, 0, 1, b2.handle, 0, 1, 0, None) == 0
    assert lib.gm_pairing_each(None, C.c_size_t(96), gm.capi.ptr(r2), C.c_size_t(192), C.c_size_t(2), gm.capi.ptr(out)) == GM_EINVAL
    assert lib.gm_pairing_each(gm.capi.ptr(r1), C.c_size_t(88), gm.capi.ptr(r2), C.c_size_t(192), C.c_size_t(2), gm.capi.ptr(out)) == GM_EINVAL
    assert lib.gm_pairing_each(gm.capi.ptr(r1), C.c_size_t(96), gm.capi.ptr(r2), C.c_size_t(96), C.c_size_t(2), gm.capi.ptr(out)) == GM_EINVAL
    b1.free()
    b2.free()


# ---- gm_gt_check -----------------------------------------------------------------------------------------------------------------
def test_check_list_against_both_statements(gm, cases):
    """the list once, in order: statuses as gt_check_ref.py expects them (tests/test_gt_device_cpu.py holds that table against
    status_tests), and acceptance as the literal f^r = 1 has it (one f12_pow per element, under 40 elements)"""
    names, x, st, _ = cases
    assert len(x) <= 40
    res = gm.gt_check(x)
    assert list(res.status) == list(st), list(zip(names, res.status, st))
    for name, c, _ in ref.adversarial():
        assert (ref.status_literal(c) == ref.OK) == (res.status[names.index(name)] == ref.OK), name
    assert not res.ok and res.first_bad == int(np.flatnonzero(st != ref.OK)[0])


@pytest.mark.parametrize("n", SIZES)
def test_check_sizes_and_first_bad(gm, cases, n):
    """members and non-members mixed inside every block; then members only with ONE bad element at the last index"""
    _, x, st, _ = cases
    res = gm.gt_check(tiled(x, n, shift=2 * n))
    want = tiled(st, n, shift=2 * n)
    bad = np.flatnonzero(want != ref.OK)
    assert list(res.status) == list(want)
    assert res.ok == (len(bad) == 0) and res.first_bad == (int(bad[0]) if len(bad) else n)
    members = x[st == ref.OK]
    good = tiled(members, n).copy()
    res = gm.gt_check(good)
    assert res.ok and res.first_bad == n and not res.status.any()
    if n:
        good[n - 1] = x[st == ref.NOT_IN_SUBGROUP][0]
        res = gm.gt_check(good)
        assert not res.ok and res.first_bad == n - 1 and res.status[n - 1] == ref.NOT_IN_SUBGROUP and not res.status[:n - 1].any()


def test_check_noncanonical_host_input(gm, cases):
    """a coefficient equal to q, and one of 2^384 - 1, in each of the 12 positions, between members"""
    _, x, st, _ = cases
    member = x[st == ref.OK][1]
    bad = ref.noncanonical_cases()
    inp = np.stack([limbs_of(c) if k % 2 == 0 else member for c in (c for _, c, _ in bad) for k in range(2)])
    res = gm.gt_check(inp)
    assert list(res.status) == [ref.NONCANONICAL, ref.OK] * len(bad)
    assert not res.ok and res.first_bad == 0
    assert gm.gt_check(inp[1:2]).ok


def test_check_refusals_fail_closed(gm, cases):
    _, x, _, _ = cases
    lib, ptr = gm.capi.load(), gm.capi.ptr
    st = np.zeros(4, dtype=np.uint8)
    fb, ok = C.c_size_t(9), C.c_int(1)
    assert lib.gm_gt_check(None, C.c_size_t(2), ptr(st), C.byref(fb), C.byref(ok)) == GM_EINVAL and ok.value == 0
    assert lib.gm_gt_check(ptr(x), C.c_size_t(2), ptr(st), C.byref(fb), None) == GM_EINVAL
    ok.value = 0
    assert lib.gm_gt_check(None, C.c_size_t(0), None, C.byref(fb), C.byref(ok)) == 0 and ok.value == 1 and fb.value == 0
    ok.value = 1
    assert lib.gm_gt_check(ptr(x), C.c_size_t(2), None, None, C.byref(ok)) == 0 and ok.value == 0  # status and first_bad may be null
    for fn in (lib.gm_hgt_check, lib.gm_ipa_check_gt):
        ok.value = 1
        assert fn(C.c_uint64(0xDEAD0032), C.byref(fb), C.byref(ok)) == GM_EHANDLE and ok.value == 0
        assert fn(C.c_uint64(0xDEAD0032), None, None) == GM_EHANDLE


def test_check_from_two_threads(gm, cases):
    _, x, st, _ = cases
    inp = tiled(x, 65)
    out = [None, None]

    def run(k):
        out[k] = [gm.gt_check(inp) for _ in range(2)]

    ts = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for rs in out:
        for r in rs:
            assert list(r.status) == list(tiled(st, 65))


# ---- gm_hgt_check ----------------------------------------------------------------------------------------------------------------
def test_hgt_check_before_and_after_a_fold(gm, cases):
    from gemini_amd.herring import GtModuleTimeProver

    _, x, st, _ = cases
    members, g = x[st == ref.OK], x[st == ref.NOT_IN_SUBGROUP][0]
    f = tiled(members, 6).copy()
    gs = np.stack([fr_from_int(3 + 5 * i) for i in range(6)])
    tw, ch = 0x1F3D5B79, 0x2468ACE13579BDF02468ACE13579BDF
    G = GtModuleTimeProver(f, gs, fr_from_int(tw))
    res = G.check()
    assert res.ok and res.first_bad == 6
    G.fold(fr_from_int(ch))
    res = G.check()
    assert res.ok and res.first_bad == 3  # a fold of members is a vector of members
    G.free()
    f[3] = g
    G = GtModuleTimeProver(f, gs, fr_from_int(tw))
    res = G.check()
    assert not res.ok and res.first_bad == 3
    G.fold(fr_from_int(ch))  # f'[1] = f[2] f[3]^(ch tw)
    folded = gp.gt_mul(f[2], gp.gt_pow(f[3], ch * tw % R))
    assert ref.status_tests(gp.gt_to_ints(folded)) == ref.NOT_IN_SUBGROUP
    res = G.check()
    assert not res.ok and res.first_bad == 1
    G.free()


# ---- gm_ipa_check_gt -------------------------------------------------------------------------------------------------------------
def test_ipa_check_gt(gm, cases):
    from tests.test_gpu_ipa import prove_on_device, reference

    _, x, st, _ = cases
    crs, tr, proof = prove_on_device(gm, reference(8, 16))
    f = proof.fields()
    assert f.rounds == 3
    res = proof.check_messages()
    assert res.ok and res.first_bad == 6
    f.messages[1, 1] = x[st == ref.NOT_IN_SUBGROUP][0]  # b of round 1: index 3
    bad = gm.InnerProductProof.from_fields(f)
    res = bad.check_messages()
    assert not res.ok and res.first_bad == 3
    pts_res = bad.check_points()  # gm_ipa_check is what it was: the points of this proof are fine
    assert pts_res.ok
    for o in (bad, proof, tr, crs):
        o.free()


# ---- gm_vrs_from_crs -------------------------------------------------------------------------------------------------------------
def test_vrs_levels_equal_their_four_products(gm):
    """a CRS of 16 points per group: every level equals the four gm_pairing_multi_h products that define it"""
    from tests import ipa_exponent_ref as X
    from gemini_amd.g2msm import g2_points_to_affine

    n = 16
    p1, _, p2, _ = X.crs(n)
    r1, r2 = g1_points_to_affine(p1), g2_points_to_affine(p2)
    crs, b1, b2 = gm.Crs(r1, r2), gm.G1Bases.register(r1), gm.G2Bases.register(r2)
    vrs = gm.Vrs(crs)
    assert vrs.levels == 3
    for l in range(vrs.levels):
        size = 2 << l
        got1, got2 = vrs.level(l)
        one = [gm.multi_pairing_h(b1, b2, min(size, n // 2), off1=0, step1=2), gm.multi_pairing_h(b1, b2, min(size, n // 2), off1=1, step1=2),
               gm.multi_pairing_h(b1, b2, min(size, n // 2), off2=0, step2=2), gm.multi_pairing_h(b1, b2, min(size, n // 2), off2=1, step2=2)]
        assert (got1[0] == one[0]).all() and (got1[1] == one[1]).all() and (got2[0] == one[2]).all() and (got2[1] == one[3]).all(), l
    for o in (vrs, b1, b2, crs):
        o.free()
