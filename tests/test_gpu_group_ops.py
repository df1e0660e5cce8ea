"""GPU: the device's group law element by element against Python integers -- the canonical XYZZ law of g1.cuh and g2.cuh
(gm_debug_g1_op, gm_debug_g2_op) and the two asm statements of the bucket accumulator (gm_debug_acc30_op: g1_madd30_asm, g1_add30_asm).

Results are compared as POINTS: zz == 0 exactly is the identity; otherwise x = X / ZZ and y = Y / ZZZ must be the integer result of
the affine chord-and-tangent law (oracle/pyref.py for G1, tests/g2_ref.py for G2) and ZZ^3 = ZZZ^2 must hold.  For the Acc30
statements every value leaving must also be normalised and below the bound the generator states for it, and acc30_to_canonical of it
must be its residue.

Case kinds for (accumulator, operand): generic; equal points with the accumulator in a non-trivial representation (doubling);
negatives (cancellation); identity + Q; P + identity; identity + identity.  Neither curve has a point of order 2 (both group orders
are odd, tests/field_cases.py), so no y = 0 input exists and none is built.

Wave composition is the point of the Acc30 tests -- the statements handle an identity accumulator, doubling and cancellation by EXEC
masking and a wave-level branch, which only a wave with lanes of different kinds exercises.  tests/acc30_cases.py: waves() states
the compositions; each is one block of 64 lanes, and every lane must give its own integer result whatever its neighbours do.
"""
import functools
import random

import numpy as np
import pytest

from gemini_amd import debug as D
from oracle import pyref
from tests import acc30_cases as ac
from tests import field_cases as fc
from tests import g2_ref

pytestmark = pytest.mark.gpu

Q = fc.Q
SIZES = [1, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


def tiled(seq, n: int, shift: int = 0):
    return [seq[(i + shift) % len(seq)] for i in range(n)]


# ---- the canonical law: cases ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def g1_cases():
    """dicts: kind, acc (X, Y, ZZ, ZZZ canonical device residues), B (the operand as an affine point, None = identity), lam (its
    representation when the op takes XYZZ)"""
    rnd = random.Random(0x61)
    pts = fc.G1_POINTS
    out = []
    for i, B in enumerate(pts):
        P = pts[(i + 5) % len(pts)]
        assert P[0] != B[0]
        lam, lam2 = rnd.randrange(2, Q), rnd.randrange(2, Q)
        out.append(dict(kind="generic", acc=fc.g1_xyzz(P, lam), B=B, lam=lam2))
        out.append(dict(kind="generic", acc=fc.g1_xyzz(P, 1), B=B, lam=1))
        out.append(dict(kind="equal", acc=fc.g1_xyzz(B, lam), B=B, lam=lam2))
        out.append(dict(kind="negatives", acc=fc.g1_xyzz(pyref.g1_neg(B), lam), B=B, lam=lam2))
        out.append(dict(kind="identity + Q", acc=(0, 0, 0, 0), B=B, lam=lam2))
        out.append(dict(kind="identity + Q", acc=(rnd.randrange(Q), rnd.randrange(Q), 0, rnd.randrange(Q)), B=B, lam=lam2))  # only zz == 0 marks it
        out.append(dict(kind="P + identity", acc=fc.g1_xyzz(P, lam), B=None, lam=lam2))
    out.append(dict(kind="identity + identity", acc=(0, 0, 0, 0), B=None, lam=1))
    out.append(dict(kind="identity + identity", acc=(5, 7, 0, 9), B=None, lam=1))
    return tuple(out)


def g1_expected(c):
    return pyref.g1_add(fc.g1_point_of(c["acc"]), c["B"])


@functools.lru_cache(maxsize=None)
def g2_cases():
    rnd = random.Random(0x62)
    pts = fc.G2_POINTS
    f2 = lambda: (rnd.randrange(1, Q), rnd.randrange(1, Q))
    zero = ((0, 0),) * 4
    out = []
    for i, B in enumerate(pts):
        P = pts[(i + 2) % len(pts)]
        assert P[0] != B[0]
        lam, lam2 = f2(), f2()
        out.append(dict(kind="generic", acc=fc.g2_xyzz(P, lam), B=B, lam=lam2))
        out.append(dict(kind="generic", acc=fc.g2_xyzz(P, (1, 0)), B=B, lam=(1, 0)))
        out.append(dict(kind="equal", acc=fc.g2_xyzz(B, lam), B=B, lam=lam2))
        out.append(dict(kind="negatives", acc=fc.g2_xyzz(g2_ref.neg(B), lam), B=B, lam=lam2))
        out.append(dict(kind="identity + Q", acc=zero, B=B, lam=lam2))
        out.append(dict(kind="identity + Q", acc=(f2(), f2(), (0, 0), f2()), B=B, lam=lam2))
        out.append(dict(kind="P + identity", acc=fc.g2_xyzz(P, lam), B=None, lam=lam2))
    out.append(dict(kind="identity + identity", acc=zero, B=None, lam=(1, 0)))
    return tuple(out)


def g2_expected(c):
    return g2_ref.add(fc.g2_point_of(c["acc"]), c["B"])


def g1_rows(recs):
    return D.rows_words(recs, len(recs[0]))


def g2_rows(recs):
    return D.rows_words([tuple(x for c in r for x in c) for r in recs], 2 * len(recs[0]))


def g2_recs(a: np.ndarray):
    return [tuple((t[2 * k], t[2 * k + 1]) for k in range(len(t) // 2)) for t in D.ints_of_words(a)]


def check_g1(got: np.ndarray, want, cases):
    for rec, w, c in zip(D.ints_of_words(got), want, cases):
        assert all(v < Q for v in rec), (c["kind"], "a coordinate is not canonical")
        assert fc.g1_point_of(rec) == w, c["kind"]


def check_g2(got: np.ndarray, want, cases):
    for rec, w, c in zip(g2_recs(got), want, cases):
        assert all(v < Q for co in rec for v in co), (c["kind"], "a coordinate is not canonical")
        assert fc.g2_point_of(rec) == w, c["kind"]


# ---- G1, canonical ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES + [len(g1_cases())])
def test_g1_madd_and_add(gm, n):
    cases = tiled(g1_cases(), n, n)
    want = [g1_expected(c) for c in cases]
    acc = g1_rows([c["acc"] for c in cases])
    aff = g1_rows([(0, 0) if c["B"] is None else fc.g1_affine_dev(c["B"]) for c in cases])
    check_g1(D.g1_op(D.G1_MADD, acc, aff), want, cases)
    xyzz = g1_rows([fc.g1_xyzz(c["B"], c["lam"]) for c in cases])
    check_g1(D.g1_op(D.G1_ADD, acc, xyzz), want, cases)


def test_g1_add_takes_any_identity_operand(gm):
    """only zz == 0 marks the identity operand of xyzz_add"""
    cases = [c for c in g1_cases() if c["kind"] in ("generic", "identity + Q")]
    acc = g1_rows([c["acc"] for c in cases])
    oth = g1_rows([(11, 13, 0, 17)] * len(cases))
    check_g1(D.g1_op(D.G1_ADD, acc, oth), [fc.g1_point_of(c["acc"]) for c in cases], cases)


@pytest.mark.parametrize("n", [1, 65, len(g1_cases())])
def test_g1_doublings(gm, n):
    cases = tiled(g1_cases(), n, n)
    acc = g1_rows([c["acc"] for c in cases])
    P = [fc.g1_point_of(c["acc"]) for c in cases]
    check_g1(D.g1_op(D.G1_DBL, acc), [pyref.g1_add(p, p) for p in P], cases)
    # the affine doubling reads x | y from the first 24 words; the other 24 are not its input
    aff = g1_rows([((0, 0) if c["B"] is None else fc.g1_affine_dev(c["B"])) + (3, 5) for c in cases])
    check_g1(D.g1_op(D.G1_DBL_AFFINE, aff), [pyref.g1_add(c["B"], c["B"]) for c in cases], cases)


@pytest.mark.parametrize("n", [1, 65, len(g1_cases())])
def test_g1_loose_record_round_trip(gm, n):
    """g1_store_xyzz30 then g1_load_xyzz30: the canonical coordinates come back bit for bit, the identity as the all-zero record"""
    cases = tiled(g1_cases(), n, n)
    acc = g1_rows([c["acc"] for c in cases])
    want = g1_rows([(0, 0, 0, 0) if c["acc"][2] == 0 else c["acc"] for c in cases])
    assert (D.g1_op(D.G1_STORE_LOAD30, acc) == want).all()
    edge = g1_rows([(v, (v + 1) % Q or 1, v or 1, Q - 1 - v if v != Q - 1 else 1) for v in fc.FQ_VALUES])  # the field list through every coordinate
    assert (D.g1_op(D.G1_STORE_LOAD30, edge) == edge).all()


# ---- G2, canonical ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_g2_madd_and_add(gm, n):
    cases = tiled(g2_cases(), n, n)
    want = [g2_expected(c) for c in cases]
    acc = g2_rows([c["acc"] for c in cases])
    zero2 = ((0, 0), (0, 0))
    aff = g2_rows([zero2 if c["B"] is None else (fc.f2d(c["B"][0]), fc.f2d(c["B"][1])) for c in cases])
    check_g2(D.g2_op(D.G2_MADD, acc, aff), want, cases)
    xyzz = g2_rows([fc.g2_xyzz(c["B"], c["lam"]) for c in cases])
    check_g2(D.g2_op(D.G2_ADD, acc, xyzz), want, cases)


@pytest.mark.parametrize("n", [1, 65])
def test_g2_doublings_and_to_affine(gm, n):
    cases = tiled(g2_cases(), n, n)
    acc = g2_rows([c["acc"] for c in cases])
    P = [fc.g2_point_of(c["acc"]) for c in cases]
    check_g2(D.g2_op(D.G2_DBL, acc), [g2_ref.add(p, p) for p in P], cases)
    zero2 = ((0, 0), (0, 0))
    aff = g2_rows([(zero2 if c["B"] is None else (fc.f2d(c["B"][0]), fc.f2d(c["B"][1]))) + ((3, 0), (5, 0)) for c in cases])
    check_g2(D.g2_op(D.G2_DBL_AFFINE, aff), [g2_ref.add(c["B"], c["B"]) for c in cases], cases)
    # grp_to_affine<GrpG2>: the affine coordinates themselves, bit for bit; the identity is the all-zero record
    want = g2_rows([(zero2 if p is None else (fc.f2d(p[0]), fc.f2d(p[1]))) + zero2 for p in P])
    assert (D.g2_op(D.G2_TO_AFFINE, acc) == want).all()


# ---- the Acc30 statements ---------------------------------------------------------------------------------------------------------------------------
def run_acc30(which: str, lanes):
    op = D.ACC30_MADD if which == "madd" else D.ACC30_ADD
    acc = D.rows_limbs30([l["acc"] for l in lanes], 4)
    if which == "madd":
        other = D.rows_words([l["other"] for l in lanes], 2)
        neg = np.array([l["neg"] for l in lanes], dtype=np.uint32)
    else:
        other, neg = D.rows_limbs30([l["other"] for l in lanes], 4), None
    out, canon = D.acc30_op(op, acc, other, neg)
    assert (out[:, [i for i in range(52) if i % 13 != 12]] < 1 << 30).all() and (out[:, 12::13] < 1 << 26).all(), "limbs not normalised"
    return D.ints_of_limbs30(out), D.ints_of_words(canon)


def check_acc30(which: str, lanes, label):
    bnd = ac.bounds(which)
    outs, canons = run_acc30(which, lanes)
    for i, (lane, out, canon) in enumerate(zip(lanes, outs, canons)):
        try:
            ac.check_lane(which, lane, out, canon, bnd)
        except AssertionError as e:
            raise AssertionError(f"{which}: {label}: lane {i} (wave lane {i % 64}, {lane['kind']}): {e}") from e


@pytest.mark.parametrize("which", ["madd", "add"])
def test_acc30_wave_compositions(gm, which):
    """every composition of acc30_cases.waves() -- all ordinary, all doubling, all cancelling, all identity, one exceptional lane at
    lane 0 / at lane 63, the kinds interleaved, false positives of the filter beside ordinary and exceptional lanes -- each its own
    block of 64 lanes, in one call"""
    ws = ac.waves(which)
    lanes = ac.build(which, [k for _, kinds in ws for k in kinds], seed=21)
    bnd = ac.bounds(which)
    outs, canons = run_acc30(which, lanes)
    for w, (name, _) in enumerate(ws):
        for i in range(64 * w, 64 * w + 64):
            try:
                ac.check_lane(which, lanes[i], outs[i], canons[i], bnd)
            except AssertionError as e:
                raise AssertionError(f"{which}: wave '{name}', lane {i % 64} ({lanes[i]['kind']}): {e}") from e


@pytest.mark.parametrize("which", ["madd", "add"])
def test_acc30_one_live_lane_in_the_second_wave(gm, which):
    """the 65-element call: a full interleaved wave, then a wave whose only live lane is of each kind in turn"""
    inter = dict(ac.waves(which))["interleaved"]
    for k in ("ordinary", "fp") + ac.EXCEPTIONAL[which]:
        check_acc30(which, ac.build(which, inter + [k], seed=33), f"65 lanes, the last one {k}")


@pytest.mark.parametrize("which", ["madd", "add"])
@pytest.mark.parametrize("n", SIZES)
def test_acc30_block_edges(gm, which, n):
    w = dict(ac.waves(which))
    kinds = w["interleaved"] + w["false positives beside ordinary and exceptional lanes"]
    check_acc30(which, ac.build(which, tiled(kinds, n, n), seed=40 + n), f"n = {n}")


def test_acc30_madd_sign(gm):
    """neg: 0 adds the base, every non-zero value its negative -- 1 and 0x80000000 alike"""
    rnd = random.Random(77)
    lanes = []
    for k in ("ordinary", "double", "cancel", "identity") * 4:
        lane = ac.madd_lane(k, rnd)
        lanes.append(lane)
        if lane["neg"]:
            lanes.append(dict(lane, neg=1 if lane["neg"] != 1 else 0x80000000))
        else:  # the same accumulator with the sign flipped: an ordinary addition of -B, whatever the lane was built as
            P = fc.g1_point_of(lane["acc"]) if lane["acc"][2] else None
            B = pyref.g1_neg((fc.val(lane["other"][0]), fc.val(lane["other"][1])))
            lanes.append(dict(kind="ordinary" if k == "ordinary" else "sign flipped", acc=lane["acc"], other=lane["other"], neg=1, point=pyref.g1_add(P, B)))
    check_acc30("madd", lanes, "signs")
