"""Key generation on the device: gm_g1_/gm_g2_fixed_base_register and gm_g1_/gm_g2_srs_register against the integers of
oracle/pyref.py and gemini_amd/g2.py, the register -> download round trip of both groups, gm_g1_bases_from_candidates / gm_g2_bases_from_candidates point for point against tests/keygen_ref.py, and the Crs operations
(gm_crs_truncate, gm_crs_halve, gm_crs_fold, gm_crs_to_bases) against the exponents of a Crs.from_scalars.

Shapes: the normalisation kernel takes 8 points a lane and 64 (G2) or 256 (G1) lanes a block, the multiply and the fold one lane a
scalar or an output -- n = 7, 8, 9 sit below, at and above a group, 257 above a block of the multiply of either group, 514 folds
to 257 outputs, and 2^12 + 3 spans 9 blocks of the G2 normalisation with an odd tail.
The candidate streams are read in pieces (points.hip: cand_piece); the junk prefix of test_pieces makes the call take several.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from gemini_amd import g2 as G2
from gemini_amd.fr import R_MOD, fr_from_int
from gemini_amd.g2msm import g2_affine_to_points, g2_jac_to_point, g2_points_to_affine
from oracle import pyref as P
from tests import keygen_ref as kr
from tests import points_ref as pr

pytestmark = pytest.mark.gpu

GM_EINVAL = -1
GM_EHANDLE = -3
Q, R = pr.Q, pr.R
assert R == R_MOD
LABEL = b"gemini-tests"
TAU = 0x1234567890ABCDEF0FEDCBA0987654321 % R
_RINV = pow(1 << 384, -1, Q)


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


def canon(vals) -> np.ndarray:
    """integers < 2^256 -> (n, 4) canonical limbs"""
    return np.array([[(int(v) >> (64 * i)) & (2**64 - 1) for i in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def g1_records_to_points(rec) -> list:
    out = []
    for row in np.asarray(rec, dtype=np.uint64).reshape(-1, 12):
        if not row.any():
            out.append(None)
            continue
        v = [sum(int(w) << (64 * i) for i, w in enumerate(row[6 * k: 6 * k + 6])) * _RINV % Q for k in range(2)]
        out.append((v[0], v[1]))
    return out


def g2_gen_record() -> np.ndarray:
    return g2_points_to_affine([G2.generator()])[0]


def g1_gen_record() -> np.ndarray:
    from gemini_amd.kzg import g1_generator_mont

    return g1_generator_mont()


def g2_records_sum(gm, rec):
    """the sum of affine records as an integer point (gm_g2_sum on the host)"""
    rec = np.asarray(rec, dtype=np.uint64).reshape(-1, 24)
    one = [(((1 << 384) % Q) >> (64 * i)) & (2**64 - 1) for i in range(6)]
    jac = np.zeros((len(rec), 36), dtype=np.uint64)
    jac[:, :24] = rec
    jac[rec.any(axis=1), 24:30] = one
    return g2_jac_to_point(gm.g2_sum(jac))


SPECIAL = [0, 1, R - 1, (1 << 255) + 1, (1 << 256) - 1, 0xAB << 248]  # zero, one, -1, above r, every byte 0xFF, one non-zero top byte


def fixed_base_scalars(n: int) -> list:
    rng = P.SplitMix64(7000 + n)
    v = [rng.fr() for _ in range(n)]
    for i, s in enumerate(SPECIAL):  # the specials from the front and again at the very end, as far as they fit
        if i < n:
            v[i] = s
        if n > 16 and i < 3:
            v[n - 1 - i] = SPECIAL[3 + i]
    return v


# ---- fixed base G2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 257])
def test_fixed_base_g2(gm, n):
    """gm_g2_fixed_base_register against g2.mul: every point for n <= 9; at 257 the specials, the edges of the normalisation groups
    and of the multiply's blocks, and the sum of all outputs (one multiplication)"""
    sc = fixed_base_scalars(n)
    b = gm.G2Bases.fixed_base(g2_gen_record(), canon(sc))
    assert b.handle != 0 and len(b) == n
    ln = C.c_size_t(99)
    gm.capi.check(gm.capi.load().gm_g2_bases_len(C.c_uint64(b.handle), C.byref(ln)))
    assert ln.value == n
    rec = b.download()
    pts = g2_affine_to_points(rec)
    spots = range(n) if n <= 9 else [0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 248, 254, 255, 256]
    for i in spots:
        assert pts[i] == G2.mul(G2.generator(), sc[i] % R), (i, hex(sc[i]))
    if n:
        assert not rec[0].any()  # a zero scalar: the all-zero identity record
        assert g2_records_sum(gm, rec) == G2.mul(G2.generator(), sum(sc) % R)
    b.free()


def test_fixed_base_g2_large(gm):
    """n = 2^12 + 3: the sum of the outputs, 16 spot indices, and every point in G2"""
    n = (1 << 12) + 3
    rng = np.random.default_rng(4099)
    limbs = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)  # any 256-bit value
    sc = [sum(int(w) << (64 * i) for i, w in enumerate(row)) for row in limbs]
    b = gm.G2Bases.fixed_base(g2_gen_record(), limbs)
    rec = b.download()
    assert g2_records_sum(gm, rec) == G2.mul(G2.generator(), sum(sc) % R)
    pts = g2_affine_to_points(rec)
    for i in [0, 7, 8, 511, 512, 513, 1023, 2047, 2048, 3000, 4088, 4095, 4096, 4097, 4098, 1234]:
        assert pts[i] == G2.mul(G2.generator(), sc[i] % R), i
    res = b.check()
    assert res.ok and res.first_bad == n
    b.free()


def test_fixed_base_g2_other_base_and_misuse(gm):
    """a base that is not the generator; null pointers are GM_EINVAL"""
    base = G2.mul(G2.generator(), 0xC0FFEE)
    sc = [5, R - 2, 1 << 200]
    b = gm.G2Bases.fixed_base(g2_points_to_affine([base])[0], canon(sc))
    assert g2_affine_to_points(b.download()) == [G2.mul(base, s % R) for s in sc]
    b.free()
    lib, h = gm.capi.load(), C.c_uint64(0)
    rec, one = g2_gen_record(), canon([1])
    assert lib.gm_g2_fixed_base_register(None, gm.capi.ptr(one), C.c_size_t(1), C.byref(h)) == GM_EINVAL
    assert lib.gm_g2_fixed_base_register(gm.capi.ptr(rec), None, C.c_size_t(1), C.byref(h)) == GM_EINVAL
    assert lib.gm_g2_fixed_base_register(gm.capi.ptr(rec), gm.capi.ptr(one), C.c_size_t(1), None) == GM_EINVAL
    assert lib.gm_g2_srs_register(gm.capi.ptr(rec), None, C.c_size_t(1), C.byref(h)) == GM_EINVAL


# ---- fixed base G1: the mirror of the above, against oracle/pyref.py ---------------------------------------------------------------
def g1_points_sum(pts):
    return functools.reduce(P.g1_add, pts, None)


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 257])
def test_fixed_base_g1(gm, n):
    """gm_g1_fixed_base_register against pyref.g1_mul: every point for n <= 9; at 257 the same spots as G2 and the sum of all outputs"""
    sc = fixed_base_scalars(n)
    b = gm.G1Bases.fixed_base(g1_gen_record(), canon(sc))
    assert b.handle != 0 and len(b) == n
    ln = C.c_size_t(99)
    gm.capi.check(gm.capi.load().gm_g1_bases_len(C.c_uint64(b.handle), C.byref(ln)))
    assert ln.value == n
    rec = b.download()
    pts = g1_records_to_points(rec)
    spots = range(n) if n <= 9 else [0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 248, 254, 255, 256]
    for i in spots:
        assert pts[i] == P.g1_mul(P.G1_GEN, sc[i] % R), (i, hex(sc[i]))
    if n:
        assert not rec[0].any()  # a zero scalar: the all-zero identity record
        assert g1_points_sum(pts) == P.g1_mul(P.G1_GEN, sum(sc) % R)
    b.free()


def test_srs_g1_against_integers(gm):
    b = gm.G1Bases.srs(g1_gen_record(), canon([TAU]), 9)
    assert g1_records_to_points(b.download()) == [P.g1_mul(P.G1_GEN, pow(TAU, i, R)) for i in range(9)]
    b.free()
    e = gm.G1Bases.srs(g1_gen_record(), canon([TAU]), 0)
    assert e.handle != 0 and len(e.download()) == 0
    e.free()


# ---- both groups: what a description (groups.cuh) tells apart, by number --------------------------------------------------------------
GROUPS = {
    1: dict(cls="G1Bases", words=12, gen=g1_gen_record, point=lambda k: P.g1_mul(P.G1_GEN, k), record=pr.g1_record, points=g1_records_to_points),
    2: dict(cls="G2Bases", words=24, gen=g2_gen_record, point=lambda k: G2.mul(G2.generator(), k), record=pr.g2_record, points=g2_affine_to_points),
}


@pytest.mark.parametrize("group", [1, 2])
def test_normalisation_with_identities_at_every_position(gm, group):
    """n = 17 is two full groups of the batched normalisation and one point: zero scalars -- identity records among the XYZZ results --
    at the first and the last place of a group, in a group of their own and next to ordinary points; then every scalar zero (the
    product that is inverted is the empty one)"""
    g = GROUPS[group]
    sc = [k + 2 for k in range(17)]
    for i in (0, 7, 8, 15, 16):
        sc[i] = 0
    b = getattr(gm, g["cls"]).fixed_base(g["gen"](), canon(sc))
    rec = b.download()
    assert g["points"](rec) == [g["point"](k) if k else None for k in sc]
    assert [i for i in range(17) if not rec[i].any()] == [0, 7, 8, 15, 16]
    b.free()
    z = getattr(gm, g["cls"]).fixed_base(g["gen"](), canon([0] * 17))
    assert z.download().shape == (17, g["words"]) and not z.download().any()
    z.free()


@pytest.mark.parametrize("flagged", [False, True])
@pytest.mark.parametrize("n", [1, 257])
@pytest.mark.parametrize("group", [1, 2])
def test_register_download_round_trip(gm, group, n, flagged):
    """records of the plain stride (96 / 192 bytes) and of the flagged one (104 / 200: the infinity flag behind the coordinates) come
    back limb for limb; a row whose flag is set comes back all-zero whatever its coordinates hold"""
    g = GROUPS[group]
    w = g["words"]
    plain = np.array([g["record"](g["point"](k + 1)) for k in range(n)], dtype=np.uint64)
    rec, want = plain, plain.copy()
    if flagged:
        rec = np.zeros((n, w + 1), dtype=np.uint64)
        rec[:, :w] = plain
        for i in ({0} if n == 1 else {1, n - 2}):  # two rows, each between unflagged neighbours; the single row of n = 1
            rec[i, w] = 1
            want[i] = 0
    b = getattr(gm, g["cls"]).register(rec)
    got = b.download()
    assert got.shape == (n, w) and (got == want).all()
    if n > 1:
        assert (b.download(offset=n - 2, n=2) == want[n - 2:]).all()
    b.free()


def test_bases_misuse(gm):
    """a range that overflows, a null length pointer; a handle of one group is unknown to the other group's entries, which free nothing"""
    lib = gm.capi.load()
    b1 = gm.G1Bases.fixed_base(g1_gen_record(), canon([1, 2, 3]))
    b2 = gm.G2Bases.fixed_base(g2_gen_record(), canon([1, 2, 3]))
    out = np.zeros((3, 24), dtype=np.uint64)
    ln = C.c_size_t(0)
    ops = {1: (lib.gm_g1_bases_free, lib.gm_g1_bases_len, lib.gm_g1_bases_download), 2: (lib.gm_g2_bases_free, lib.gm_g2_bases_len, lib.gm_g2_bases_download)}
    for mine, other, b in ((1, 2, b1), (2, 1, b2)):
        free, length, download = ops[mine]
        h = C.c_uint64(b.handle)
        assert download(h, C.c_size_t(2**64 - 1), C.c_size_t(2), gm.capi.ptr(out)) == GM_EINVAL
        assert download(h, C.c_size_t(2), C.c_size_t(2), gm.capi.ptr(out)) == GM_EINVAL
        assert download(h, C.c_size_t(0), C.c_size_t(1), None) == GM_EINVAL
        assert length(h, None) == GM_EINVAL
        o_free, o_length, o_download = ops[other]
        assert o_length(h, C.byref(ln)) == GM_EHANDLE
        assert o_download(h, C.c_size_t(0), C.c_size_t(1), gm.capi.ptr(out)) == GM_EHANDLE
        assert o_free(h) == GM_EHANDLE
        gm.capi.check(length(h, C.byref(ln)))  # still there
        assert ln.value == 3 and len(b.download()) == 3
    b1.free()
    b2.free()
    assert lib.gm_g1_bases_free(C.c_uint64(b1.handle)) == GM_EHANDLE and lib.gm_g2_bases_free(C.c_uint64(b2.handle)) == GM_EHANDLE


# ---- SRS ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def g2_powers(n: int) -> tuple:
    return tuple(G2.mul(G2.generator(), pow(TAU, i, R)) for i in range(n))


def test_srs_g2_against_integers(gm):
    b = gm.G2Bases.srs(g2_gen_record(), canon([TAU]), 9)
    assert g2_affine_to_points(b.download()) == list(g2_powers(9))
    b.free()
    e = gm.G2Bases.srs(g2_gen_record(), canon([TAU]), 0)
    assert e.handle != 0 and len(e.download()) == 0
    e.free()


def test_srs_g2_equals_the_verifier_key(gm):
    """the first max_eval_points + 1 powers are the G2 half of gm_vk_from_trapdoor for the same tau, byte for byte"""
    from gemini_amd.kzg import VerifierKey

    mep = 3
    vk = VerifierKey.from_trapdoor(canon([TAU]), mep)
    raw = vk.powers_of_g2_bytes(enc=0)
    b = gm.G2Bases.srs(g2_gen_record(), canon([TAU]), mep + 3)
    assert int.from_bytes(raw[:8], "little") == mep + 1 and raw[8:] == b.to_bytes(False, 0, 0, mep + 1)
    b.free()


def test_g1_srs_passes_the_powers_check_against_the_g2_srs(gm):
    """gm_g1_powers_check of a gm_g1_srs_register key against elements 0 and 1 of the G2 key; and fails against elements 0 and 2"""
    b2 = gm.G2Bases.srs(g2_gen_record(), canon([TAU]), 3)
    rec = b2.download()
    b1 = gm.G1Bases.srs(g1_gen_record(), canon([TAU]), 33)
    assert gm.check_powers(b1, rec[0], rec[1], rho=0xDEADBEEF12345)
    assert not gm.check_powers(b1, rec[0], rec[2], rho=0xDEADBEEF12345)
    b1.free()
    b2.free()


def test_committer_key_new_takes_its_g2_half_from_the_device(gm):
    from gemini_amd.kzg import CommitterKey

    ck = CommitterKey.new(16, 4, canon([TAU]))
    assert ck.powers_of_g2 == list(g2_powers(5))
    assert ck.powers_of_g2_bytes() == G2.serialize_vec_uncompressed(list(g2_powers(5)))
    ck.powers_of_g.free()
    other = G2.mul(G2.generator(), 77)
    ck = CommitterKey.new(4, 1, canon([TAU]), g2_affine=other)
    assert ck.powers_of_g2 == [other, G2.mul(other, TAU)]
    ck.powers_of_g.free()


# ---- candidates, hand-built --------------------------------------------------------------------------------------------------------
def _non_square_x(group: int):
    if group == 1:
        x = 1
        while pr.fq_sqrt((x**3 + 4) % Q) is not None:
            x += 1
        return x
    x = (1, 1)
    while pr.g2_point_from_x(x) is not None:
        x = (x[0] + 1, 1)
    return x


@functools.lru_cache(maxsize=None)
def hand_built(group: int):
    """64 candidates -> (bytes, [(status, cleared point)]): every skip rule, both choice bits, the ignored bits, then random bytes"""
    rng = np.random.default_rng(640 + group)
    rand = lambda: rng.integers(0, 256, size=48 * group, dtype=np.uint8).tobytes()  # noqa: E731
    if group == 1:
        x = [p[0] for p in pr.g1_random_curve_points(3)]
        c = [kr.g1_candidate_bytes(x[0], False), kr.g1_candidate_bytes(x[0], True), kr.g1_candidate_bytes(Q, False), kr.g1_candidate_bytes(Q + 2, True),
             kr.g1_candidate_bytes((1 << 381) - 1, False), kr.g1_candidate_bytes(_non_square_x(1), False), kr.g1_candidate_bytes(_non_square_x(1), True, 3),
             kr.g1_candidate_bytes(0, False), kr.g1_candidate_bytes(0, True), kr.g1_candidate_bytes(x[1], True, 1), kr.g1_candidate_bytes(x[1], True, 2),
             kr.g1_candidate_bytes(x[2], False, 3), kr.g1_candidate_bytes(Q - 1, True), kr.g1_candidate_bytes(1, False), kr.g1_candidate_bytes(2, True)]
    else:
        x = [p[0] for p in pr.g2_random_curve_points(2)]
        ns = _non_square_x(2)
        c = [kr.g2_candidate_bytes(x[0], False), kr.g2_candidate_bytes(x[0], True), kr.g2_candidate_bytes((Q, x[0][1]), False),
             kr.g2_candidate_bytes((x[0][0], Q + 1), True), kr.g2_candidate_bytes((Q, ns[1]), False), kr.g2_candidate_bytes(ns, False),
             kr.g2_candidate_bytes(ns, True, (1, 2)), kr.g2_candidate_bytes(x[1], True, (3, 0)), kr.g2_candidate_bytes(x[1], False, (0, 3), c0_top=True),
             kr.g2_candidate_bytes(x[1], True, (2, 1), c0_top=True), kr.g2_candidate_bytes((0, 0), False), kr.g2_candidate_bytes((Q - 1, 0), True),
             kr.g2_candidate_bytes((0, Q - 1), True), kr.g2_candidate_bytes((3, 0), False), kr.g2_candidate_bytes((0, 5), True)]
    c += [rand() for _ in range(64 - len(c))]
    one = kr.g1_from_candidate if group == 1 else kr.g2_from_candidate
    return b"".join(c), tuple(one(b) for b in c)


def device_points(group: int, bases) -> list:
    return g1_records_to_points(bases.download()) if group == 1 else g2_affine_to_points(bases.download())


def from_candidates(gm, group: int, cand: bytes, n: int):
    return (gm.G1Bases if group == 1 else gm.G2Bases).from_candidates(cand, n)


@pytest.mark.parametrize("group", [1, 2])
def test_candidates_point_for_point(gm, group):
    cand, ref = hand_built(group)
    statuses = [st for st, _ in ref]
    assert {kr.OK, kr.GE_Q, kr.NO_SQUARE} <= set(statuses) and (group == 2 or kr.IDENTITY in statuses)
    good = [i for i, st in enumerate(statuses) if st == kr.OK]
    total = len(good)
    assert total >= 12 and good[-4] < 63
    # n reached before m: used < m, found = n
    n = total - 3
    b, used, found = from_candidates(gm, group, cand, n)
    assert (used, found) == (good[n - 1] + 1, n) and used < 64
    assert device_points(group, b) == [ref[i][1] for i in good[:n]]
    assert b.check().ok
    b.free()
    assert (used, found) == kr.from_candidates(group, cand, n)[1:]
    # all of them
    b, used, found = from_candidates(gm, group, cand, total)
    assert (used, found) == (good[-1] + 1, total) and device_points(group, b) == [ref[i][1] for i in good]
    b.free()
    # a shortfall is a result
    b, used, found = from_candidates(gm, group, cand, total + 1)
    assert b is None and (used, found) == (64, total)
    # one point; no point (an empty handle, nothing read); no candidates
    b, used, found = from_candidates(gm, group, cand, 1)
    assert (used, found) == (good[0] + 1, 1) and device_points(group, b) == [ref[good[0]][1]]
    b.free()
    b, used, found = from_candidates(gm, group, cand, 0)
    assert b is not None and b.handle != 0 and (used, found) == (0, 0) and len(b.download()) == 0
    b.free()
    b, used, found = from_candidates(gm, group, b"", 2)
    assert b is None and (used, found) == (0, 0)


@pytest.mark.parametrize("group", [1, 2])
def test_candidates_in_pieces(gm, group):
    """a junk prefix longer than the first piece: the call reads on, piece after piece, and counts across them"""
    cand, ref = hand_built(group)
    good = [i for i, (st, _) in enumerate(ref) if st == kr.OK]
    junk = b"\xff" * (48 * group * 200)  # 200 candidates with x >= q
    n = 5
    b, used, found = from_candidates(gm, group, junk + cand, n)
    assert (used, found) == (200 + good[n - 1] + 1, n)
    assert device_points(group, b) == [ref[i][1] for i in good[:n]]
    b.free()
    b, used, found = from_candidates(gm, group, junk + cand, len(good) + 1)
    assert b is None and (used, found) == (264, len(good))


def test_candidates_misuse(gm):
    lib, z = gm.capi.load(), C.c_size_t
    cand = np.zeros(96, dtype=np.uint8)
    for fn in (lib.gm_g1_bases_from_candidates, lib.gm_g2_bases_from_candidates):
        h, used, found = C.c_uint64(9), z(), z()
        assert fn(None, z(1), z(1), C.byref(h), C.byref(used), C.byref(found)) == GM_EINVAL and h.value == 0
        assert fn(gm.capi.ptr(cand), z(1), z(1), None, C.byref(used), C.byref(found)) == GM_EINVAL
        h = C.c_uint64(9)
        assert fn(gm.capi.ptr(cand), z(1), z(1), C.byref(h), None, C.byref(found)) == GM_EINVAL and h.value == 0
        assert fn(gm.capi.ptr(cand), z(1), z(1), C.byref(h), C.byref(used), None) == GM_EINVAL


# ---- candidates at scale -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
def test_candidates_at_scale(gm, group):
    """n = 1000 from a fixed seed: acceptance of every candidate by the reference's square roots, found and used, the first 8 and the
    last 2 points, and all 1000 in the subgroup"""
    from gemini_amd.points import candidate_stream

    n = 1000
    cand = candidate_stream(b"test_gpu_keygen scale", group, 0, 4 * n + 64)
    acc = kr.accepted(group, cand)
    assert len(acc) >= n
    b, used, found = from_candidates(gm, group, cand, n)
    assert (used, found) == (acc[n - 1] + 1, n)
    size = 48 * group
    one = kr.g1_from_candidate if group == 1 else kr.g2_from_candidate
    pts = device_points(group, b)
    for j in list(range(8)) + [n - 2, n - 1]:
        assert (kr.OK, pts[j]) == one(cand[size * acc[j]: size * (acc[j] + 1)]), j
    assert len(set(pts)) == n and None not in pts
    res = b.check()
    assert res.ok and res.first_bad == n
    b.free()
    # the stream continues from `used`: the next points are the next survivors
    b, used2, found2 = from_candidates(gm, group, cand[size * used:], 2)
    assert (used + used2, found2) == (acc[n + 1] + 1, 2)
    assert device_points(group, b)[1] == one(cand[size * acc[n + 1]: size * (acc[n + 1] + 1)])[1]
    b.free()


def test_bases_from_seed_continues_its_stream(gm, monkeypatch):
    """points.bases_from_seed with a first request too short for n: the same points as one long request"""
    from gemini_amd import points

    n = 6
    whole, _, _ = points.bases_from_candidates(2, points.candidate_stream(b"seed", 2, 0, 4 * n + 64), n)
    want = whole.download()
    whole.free()
    real = points.candidate_stream
    monkeypatch.setattr(points, "candidate_stream", lambda seed, group, start, count: real(seed, group, start, min(count, 7)))
    got = points.bases_from_seed(2, b"seed", n)
    assert (got.download() == want).all()
    got.free()


# ---- Crs ---------------------------------------------------------------------------------------------------------------------------
def mont(v) -> np.ndarray:
    return np.stack([fr_from_int(x) for x in v]) if len(v) else np.zeros((0, 4), dtype=np.uint64)


def scalars(seed: int, n: int) -> list:
    rng = P.SplitMix64(seed)
    return [rng.fr() for _ in range(n)]


def prove_and_verify(gm, crs, d: int) -> bool:
    a, b = scalars(31, d), scalars(32, d)
    tr = gm.Transcript(LABEL)
    proof = gm.InnerProductProof.new(tr, crs, mont(a), mont(b))
    vrs = gm.Vrs(crs)
    comm_a, comm_b = crs.commit_g1(mont(a)), crs.commit_g2(mont(b))
    y = sum(x * z for x, z in zip(a, b)) % R
    ok = proof.verify_transcript(vrs, comm_a, comm_b, fr_from_int(y))
    bad = proof.verify_transcript(vrs, comm_a, comm_b, fr_from_int((y + 1) % R))
    for o in (proof, vrs, tr):
        o.free()
    return ok and not bad


def test_crs_from_scalars_proves_and_verifies(gm):
    crs = gm.Crs.from_scalars(canon(scalars(41, 16)), canon(scalars(42, 16)))
    assert (crs.n1, crs.n2) == (16, 16) and crs.check().ok
    assert prove_and_verify(gm, crs, 8)
    crs.free()


def test_crs_new_from_a_seed_proves_and_verifies(gm):
    crs = gm.Crs.new(b"test_gpu_keygen crs", 16)
    assert (crs.n1, crs.n2) == (16, 16) and crs.check().ok
    assert prove_and_verify(gm, crs, 8)
    again = gm.Crs.new(b"test_gpu_keygen crs", 16)
    other = gm.Crs.new(b"another seed", 16)
    b1, b2 = crs.bases()
    a1, a2 = again.bases()
    o1, o2 = other.bases()
    assert (b1.download() == a1.download()).all() and (b2.download() == a2.download()).all()  # a function of the seed
    assert not (b1.download() == o1.download()).any(axis=1).any() and not (b2.download() == o2.download()).any(axis=1).any()
    for o in (b1, b2, a1, a2, o1, o2, crs, again, other):
        o.free()


def crs_points(crs):
    """both arrays read back through gm_crs_to_bases"""
    b1, b2 = crs.bases()
    out = g1_records_to_points(b1.download()), g2_affine_to_points(b2.download())
    assert len(b1) == crs.n1 and len(b2) == crs.n2
    b1.free()
    b2.free()
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 514])
def test_crs_fold_against_integers(gm, n):
    """n = 514 folds to 257 outputs, past a 256-lane block of the G1 fold and into the fifth 64-lane block of the G2 fold: there the outputs
    at the block edges and the sum of all outputs are checked against the exponents, not every point"""
    a, b = scalars(50 + n, n), scalars(60 + n, n)
    if n >= 5:
        a[3], b[2] = 0, 0  # identities among the points
    c = scalars(70, 1)[0]
    crs = gm.Crs.from_scalars(canon(a), canon(b))
    w = mont(scalars(80, max(n - 1, 0)))
    before = (crs.commit_g1(w), crs.commit_g2(w))
    folded = crs.fold(fr_from_int(c))
    m = (n + 1) // 2
    assert (folded.n1, folded.n2) == (m, m) and folded.handle != crs.handle
    fold_exp = lambda v: [(v[2 * i] + (c * v[2 * i + 1] if 2 * i + 1 < n else 0)) % R for i in range(m)]  # noqa: E731
    g1s, g2s = crs_points(folded)
    spots = range(m) if n <= 8 else [0, 63, 64, 255, 256]
    assert [g1s[i] for i in spots] == [pr.g1_mul_raw(pr.G1_GEN, fold_exp(a)[i]) for i in spots]
    assert [g2s[i] for i in spots] == [G2.mul(G2.generator(), fold_exp(b)[i]) for i in spots]
    if n > 8:
        assert g1_points_sum(g1s) == P.g1_mul(P.G1_GEN, sum(fold_exp(a)) % R)
        b1, b2 = folded.bases()
        assert g2_records_sum(gm, b2.download()) == G2.mul(G2.generator(), sum(fold_exp(b)) % R)
        b1.free()
        b2.free()
    # the input is the caller's, unchanged
    assert (crs.n1, crs.n2) == (n, n)
    after = (crs.commit_g1(w), crs.commit_g2(w))
    assert (before[0] == after[0]).all() and (before[1] == after[1]).all()
    g1s, g2s = crs_points(crs)
    spots = range(n) if n <= 8 else [0, 1, 127, 128, 511, 512, 513]
    assert [g1s[i] for i in spots] == [pr.g1_mul_raw(pr.G1_GEN, a[i]) for i in spots]
    assert [g2s[i] for i in spots] == [G2.mul(G2.generator(), b[i]) for i in spots]
    folded.free()
    crs.free()


def test_crs_halve_and_truncate(gm):
    n = 5
    a, b = scalars(91, n), scalars(92, n)
    crs = gm.Crs.from_scalars(canon(a), canon(b))
    all1, all2 = crs_points(crs)
    w = mont(scalars(93, 2))
    before = crs.commit_g1(w)
    h = crs.halve()
    assert (h.n1, h.n2) == (3, 3) and crs_points(h) == (all1[:3], all2[:3])
    hh = h.halve().halve()
    assert (hh.n1, hh.n2) == (1, 1) and crs_points(hh.halve()) == (all1[:1], all2[:1])
    for rounds, k in ((0, 1), (1, 2), (2, 4), (3, 5), (10, 5), (63, 5), (64, 5), (1000, 5)):
        t = crs.truncate(rounds)
        assert (t.n1, t.n2) == (k, k) and crs_points(t) == (all1[:k], all2[:k]), rounds
        t.free()
    assert (crs.commit_g1(w) == before).all() and (crs.n1, crs.n2) == (5, 5)
    # groups of different lengths: truncate and halve act on each, fold refuses
    b1, b2 = crs.bases()
    uneven = gm.Crs(b1.download()[:4], b2.download()[:3])
    t = uneven.truncate(2)
    assert (t.n1, t.n2) == (4, 3)
    hv = uneven.halve()
    assert (hv.n1, hv.n2) == (2, 2)
    out = C.c_uint64(5)
    lib = gm.capi.load()
    assert lib.gm_crs_fold(C.c_uint64(uneven.handle), gm.capi.ptr(fr_from_int(3)), C.byref(out)) == GM_EINVAL and out.value == 0
    assert b"ipa.rs" in lib.gm_last_error()
    # misuse: unknown handles, null pointers; one half of gm_crs_to_bases alone
    assert lib.gm_crs_fold(C.c_uint64(crs.handle), None, C.byref(out)) == GM_EINVAL
    assert lib.gm_crs_halve(C.c_uint64(crs.handle), None) == GM_EINVAL
    assert lib.gm_crs_halve(C.c_uint64(2**40), C.byref(out)) == -3 and lib.gm_crs_to_bases(C.c_uint64(2**40), C.byref(out), None) == -3
    only2 = C.c_uint64(0)
    gm.capi.check(lib.gm_crs_to_bases(C.c_uint64(crs.handle), None, C.byref(only2)))
    k2 = gm.G2Bases(only2.value, 5)
    assert g2_affine_to_points(k2.download()) == all2
    for o in (k2, b1, b2, t, hv, uneven, h, hh, crs):
        o.free()
