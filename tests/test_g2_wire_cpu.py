"""The G2 encodings of gemini_amd/g2.py on Python integers: serialize_compressed / serialize_uncompressed / deserialize in both framings,
the image of wire.g1_serialize / g1_deserialize over Fq2.  This is the definition the device decoder follows
(tests/test_gpu_g2_bytes.py holds k_pt_decode<PtG2> against it); here it is held against a published vector, against its own inverse and
against the status each rejection class is assigned."""
import random

import pytest

from gemini_amd import g2, wire
from tests import points_ref as pr
from tests.g2_cases import BAD_ENCODING, NONCANONICAL, NOT_IN_SUBGROUP, NOT_ON_CURVE, g2_bytes, real_x_split, rejection_cases

# the compressed generator of G2 in the zcash framing, as published with the curve (x.c1 | x.c0 big-endian, the compression bit set)
ZCASH_G2_GENERATOR = ("93e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e"
                      "024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8")
FORMATS = [(c, e) for e in (0, 1) for c in (True, False)]
IDS = [f"{'compressed' if c else 'uncompressed'}-{'zcash' if e else 'arkworks'}" for c, e in FORMATS]


def test_known_answer():
    G = g2.generator()
    assert not g2._f2_gt(G[1], g2.f2_neg(G[1]))  # the sign bit (0x20) is clear in the vector
    assert g2.serialize_compressed(G, 1).hex() == ZCASH_G2_GENERATOR
    assert g2.deserialize(bytes.fromhex(ZCASH_G2_GENERATOR), 0, True, 1) == (G, 96)
    neg = bytearray.fromhex(ZCASH_G2_GENERATOR)
    neg[0] |= 0x20
    assert g2.deserialize(bytes(neg), 0, True, 1) == ((G[0], g2.f2_neg(G[1])), 96)


def test_f2_sqrt_norm_method():
    """the derivation the square root of k_pt_decode<PtG2> rests on, against tests/points_ref.py's and against squaring"""
    rng = random.Random(0xF2)
    sides = set()
    for _ in range(40):
        a = (rng.randrange(pr.Q), rng.randrange(pr.Q))
        sq = g2.f2_mul(a, a)
        r = g2.f2_sqrt(sq)
        assert r in (a, g2.f2_neg(a)) and pr.f2_sqrt(sq) in (a, g2.f2_neg(a))
        delta = (sq[0] + pr.fq_sqrt((sq[0] ** 2 + sq[1] ** 2) % pr.Q)) * pow(2, -1, pr.Q) % pr.Q
        sides.add(pow(delta, (pr.Q - 1) // 2, pr.Q) == 1)
        non = g2.f2_mul(sq, (1, 1))  # 1 + u is no square
        assert g2.f2_sqrt(non) is None and pr.f2_sqrt(non) is None
    assert sides == {True, False}  # delta a residue, and delta a non-residue
    for a in ((0, 0), (1, 0), (pr.Q - 1, 0), (0, 1), (0, pr.Q - 1), (4, 0), (5, 0), (0, 2)):
        r, ref = g2.f2_sqrt(a), pr.f2_sqrt(a)
        assert (r is None) == (ref is None)
        if r is not None:
            assert g2.f2_mul(r, r) == a


@pytest.mark.parametrize("compress,enc", FORMATS, ids=IDS)
def test_round_trip(compress, enc):
    G = g2.generator()
    members = [G, None] + [g2.mul(G, k) for k in (2, 3, 0xC0FFEE, g2.R_ORDER - 1)]
    signs = {g2._f2_gt(p[1], g2.f2_neg(p[1])) for p in members if p is not None}
    assert signs == {True, False}
    size = g2.g2_size(compress)
    data = b"".join(g2_bytes(p, compress, enc) for p in members)
    pos = 0
    for p in members:
        got, pos = g2.deserialize(data, pos, compress, enc)
        assert got == p
    assert pos == len(data) == size * len(members)
    for p in pr.g2_random_curve_points(2):
        one = g2_bytes(p, compress, enc)
        assert g2.deserialize(one, 0, compress, enc, validate=False) == (p, size)
        assert g2.deserialize(g2_bytes((p[0], g2.f2_neg(p[1])), compress, enc), 0, compress, enc, validate=False) == ((p[0], g2.f2_neg(p[1])), size)
    if not compress:
        assert g2.deserialize_uncompressed(g2_bytes(G, False, enc), enc) == G  # the reader that was here before agrees
    with pytest.raises(wire.WireError):
        g2.deserialize(data[: size - 1], 0, compress, enc)


@pytest.mark.parametrize("compress,enc", FORMATS, ids=IDS)
def test_rejections(compress, enc):
    cases = rejection_cases(compress, enc)
    assert {c[2] for c in cases} == {BAD_ENCODING, NONCANONICAL, NOT_ON_CURVE, NOT_IN_SUBGROUP}
    names = " | ".join(c[0] for c in cases)
    for want in ["infinity with a non-zero byte", "not in the subgroup", "coordinate 0 >= q", "coordinate 1 >= q"] + \
                (["no square"] if compress else ["off the twist", "coordinate 2 >= q", "coordinate 3 >= q"]) + \
                (["flags = 3"] if enc == 0 else ["sort flag on infinity"] + ([] if compress else ["sort flag on uncompressed"])) + \
                (["sign flag does not match y"] if enc == 0 and not compress else []):
        assert want in names, want
    for name, one, status in cases:
        with pytest.raises(wire.WireError) as e:
            g2.deserialize(one, 0, compress, enc, validate=True)
        assert e.value.status == status, name
        if status == NOT_IN_SUBGROUP:  # validate=False accepts a curve point outside the subgroup, and nothing else of the table
            assert g2.deserialize(one, 0, compress, enc, validate=False)[0] == pr.g2_random_curve_points(1)[0]
        elif status != NOT_ON_CURVE or compress:
            with pytest.raises(wire.WireError) as e:
                g2.deserialize(one, 0, compress, enc, validate=False)
            assert e.value.status == status, name


@pytest.mark.parametrize("enc", [0, 1], ids=["arkworks", "zcash"])
def test_real_x_both_branches(enc):
    """x = (k, 0), k = 1 .. 40: 15 lie on the twist and 25 do not -- "not a square" and "a square" without a search"""
    on, off = real_x_split()
    assert len(on) == 15 and len(off) == 25
    for k in range(1, 41):
        for larger in (False, True):
            one = bytearray(g2.serialize_compressed(((k, 0), (0, 1)), enc))  # y only lends its sign: (0, 1) is the smaller of +-u
            if larger:
                one[95 if enc == 0 else 0] |= 0x80 if enc == 0 else 0x20
            if k in off:
                with pytest.raises(wire.WireError) as e:
                    g2.deserialize(bytes(one), 0, True, enc, validate=False)
                assert e.value.status == NOT_ON_CURVE
            else:
                p, _ = g2.deserialize(bytes(one), 0, True, enc, validate=False)
                assert p[0] == (k, 0) and g2.on_curve(p) and g2._f2_gt(p[1], g2.f2_neg(p[1])) == larger
                with pytest.raises(wire.WireError) as e:  # none of them is in G2 (the cofactor is ~2^253)
                    g2.deserialize(bytes(one), 0, True, enc, validate=True)
                assert e.value.status == NOT_IN_SUBGROUP
