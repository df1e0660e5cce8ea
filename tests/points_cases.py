"""The planted encodings of the G1 decode tests (test infrastructure): one rejected 48- / 96-byte string per row of the status table of
gm_g1_bases_from_bytes, per (compression, framing) where the row applies.  tests/test_points_cpu.py holds them against wire.py,
tests/test_gpu_points.py against the device."""
from gemini_amd import wire
from gemini_amd.points import PointStatus
from tests import points_ref as pr

ARK, ZCASH = wire.G1Encoding.ARKWORKS, wire.G1Encoding.ZCASH


def g1_bytes(p, compress, enc) -> bytes:
    """the canonical encoding of an affine point (x, y) / None -- whether or not it is on the curve"""
    return wire.g1_serialize(wire.g1_from_affine_ints(p), compress, enc)


def _nonsquare_x() -> int:
    x = 1
    while pr.fq_sqrt((x**3 + 4) % pr.Q) is not None:
        x += 1
    return x


def rejection_cases(compress: bool, enc) -> list:
    """[(name, bytes of one point, PointStatus)]"""
    G = pr.G1_GEN
    good = bytearray(g1_bytes(G, compress, enc))
    n = len(good)
    outside = pr.g1_random_curve_points(1)[0]  # on the curve, not in G1
    cases = []

    def add(name, data, status):
        assert len(data) == n
        cases.append((name, bytes(data), status))

    if enc == ARK:
        b = bytearray(good)
        b[n - 1] |= 0xC0
        add("flags = 3", b, PointStatus.BAD_ENCODING)
    else:
        b = bytearray(good)
        b[0] ^= 0x80
        add("compression bit wrong", b, PointStatus.BAD_ENCODING)
        if not compress:
            b = bytearray(good)
            b[0] |= 0x20
            add("sort flag on uncompressed", b, PointStatus.BAD_ENCODING)
        else:
            b = bytearray(n)
            b[0] = 0x80 | 0x40 | 0x20
            add("sort flag on infinity", b, PointStatus.BAD_ENCODING)
    # x >= q: the bytes of x replaced by those of q + 5 (below 2^381, so no flag bit is touched)
    xb = (pr.Q + 5).to_bytes(48, "little" if enc == ARK else "big")
    b = bytearray(good)
    if enc == ARK:
        flags = b[47] & 0xC0 if compress else 0
        b[:48] = xb
        b[47] |= flags
    else:
        flags = b[0] & 0xE0
        b[:48] = xb
        b[0] |= flags
    add("x >= q", b, PointStatus.NONCANONICAL)
    if compress:
        b = bytearray(g1_bytes((_nonsquare_x(), 0), True, enc))
        add("x^3 + 4 is no square", b, PointStatus.NOT_ON_CURVE)
    else:
        add("off the curve", g1_bytes((G[0], (G[1] + 1) % pr.Q), False, enc), PointStatus.NOT_ON_CURVE)
    b = bytearray(g1_bytes(None, compress, enc))
    b[5] = 1
    add("infinity with non-zero bytes", b, PointStatus.BAD_ENCODING)
    if enc == ARK and not compress:
        b = bytearray(good)
        b[n - 1] ^= 0x80
        add("sign flag does not match y", b, PointStatus.BAD_ENCODING)
    add("not in the subgroup", g1_bytes(outside, compress, enc), PointStatus.NOT_IN_SUBGROUP)
    return cases
