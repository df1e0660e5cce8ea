"""GPU: gm_pairing_multi_many(_h) -- S independent pairing products in ONE segmented Miller launch and ONE launch of final
exponentiations.  Every output equals gm_pairing_multi on that product byte for byte: both raise to exactly (q^12 - 1) / r and an
element of GT has one canonical form."""
import numpy as np
import pytest

from gemini_amd import g2
from gemini_amd import pairing as gp
from gemini_amd.g2msm import G2Bases, g2_points_to_affine
from oracle import pairing as OP
from oracle import pyref as P
from tests.test_gpu_pairing import NPTS, g1_points_to_affine, pts  # noqa: F401  (pts: the module's fixture of 132 points with known logs)

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 5, 64, 65, 130)
# twelve 5-pair products fill a 64-lane block, so the 13th starts the next; 65 and 130 pairs span two and three blocks (a
# reduction level); 0 is the empty product
CASES = {1: [130], 2: [65, 0], 13: [5] * 13, 14: [5, 0, 64, 1, 65, 5, 130, 5, 5, 0, 1, 64, 5, 5]}


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


def _pairs(pts, lens):
    """the records of every product back to back (product s starts at point 7 s of the 132) and the offsets"""
    _, _, r1, _, _, r2 = pts
    idx = np.concatenate([(7 * s + np.arange(n)) % NPTS for s, n in enumerate(lens)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return np.ascontiguousarray(r1[idx]), np.ascontiguousarray(r2[idx]), off


@pytest.mark.parametrize("S", sorted(CASES))
def test_every_product_equals_the_single_call(gm, pts, S):
    lens = CASES[S]
    assert len(lens) == S and set(lens) <= set(LENGTHS)
    g1, g2r, off = _pairs(pts, lens)
    got = gp.multi_pairing_many(g1, g2r, off)
    assert got.shape == (S, 72)
    for s in range(S):
        lo, hi = int(off[s]), int(off[s + 1])
        want = gp.multi_pairing(g1[lo:hi], g2r[lo:hi]) if hi > lo else gp.gt_one()
        assert got[s].tobytes() == want.tobytes(), (S, s, hi - lo)


def test_registered_bases_and_no_products(gm, pts):
    from gemini_amd.msm import G1Bases

    lens = CASES[14]
    g1, g2r, off = _pairs(pts, lens)
    want = gp.multi_pairing_many(g1, g2r, off)
    pad1, pad2 = np.concatenate([g1[:3], g1]), np.concatenate([g2r[:2], g2r])
    b1, b2 = G1Bases.register(pad1), G2Bases.register(pad2)
    try:
        assert gp.multi_pairing_many_h(b1, b2, off, off1=3, off2=2).tobytes() == want.tobytes()
        with pytest.raises(gm.capi.GeminiHipError) as e:
            gp.multi_pairing_many_h(b1, b2, off, off1=4, off2=2)  # one pair past the end of the G1 bases
        assert e.value.code == -1
    finally:
        b1.free()
        b2.free()
    assert gp.multi_pairing_many(g1, g2r, [0]).shape == (0, 72)
    with pytest.raises(gm.capi.GeminiHipError):
        gp.multi_pairing_many(g1, g2r, np.array([0, 5, 3], dtype=np.uint64))


def test_bilinear_product_is_one(gm, pts):
    """e(a P, Q) e(-P, a Q) = 1 as ONE product, beside a product that is not 1"""
    p1, _, _, p2, _, _ = pts
    a = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA5 % OP.R
    Pt, Qt = p1[3], p2[2]
    g1 = g1_points_to_affine([P.g1_mul(Pt, a), P.g1_neg(Pt), Pt])
    g2r = g2_points_to_affine([Qt, g2.mul(Qt, a), Qt])
    got = gp.multi_pairing_many(g1, g2r, [0, 2, 3])
    one = gp.gt_one()
    assert got[0].tobytes() == one.tobytes()
    assert got[1].tobytes() != one.tobytes() and got[1].tobytes() == gp.multi_pairing(g1[2:], g2r[2:]).tobytes()
