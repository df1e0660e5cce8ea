"""The planted encodings of the G2 decode tests (test infrastructure): one rejected 96- / 192-byte string per row of the status table of
gm_g2_bases_from_bytes, per (compression, framing) where the row applies -- the image of tests/points_cases.py over Fq2.
tests/test_g2_wire_cpu.py holds them against gemini_amd/g2.py, tests/test_gpu_g2_bytes.py against the device."""
import functools

from gemini_amd import g2
from tests import points_ref as pr

BAD_ENCODING, NONCANONICAL, NOT_ON_CURVE, NOT_IN_SUBGROUP = g2.PT_BAD_ENCODING, g2.PT_NONCANONICAL, g2.PT_NOT_ON_CURVE, g2.PT_NOT_IN_SUBGROUP


def g2_bytes(p, compress, enc) -> bytes:
    """the canonical encoding of an affine point / None -- whether or not it is on the twist"""
    return g2.serialize_compressed(p, enc) if compress else g2.serialize_uncompressed(p, enc)


def coord_offset(coord: int, enc: int) -> int:
    """where coordinate `coord` (0 x.c0, 1 x.c1, 2 y.c0, 3 y.c1) starts in an encoding: the zcash framing puts c1 first"""
    return 48 * (coord ^ 1 if enc == 1 else coord)


@functools.lru_cache(maxsize=None)
def real_x_split():
    """x = (k, 0), k = 1 .. 40 -> (the k on the twist, the k whose x^3 + 4 (1 + u) is no square)"""
    on = [k for k in range(1, 41) if pr.g2_point_from_x((k, 0)) is not None]
    return on, [k for k in range(1, 41) if k not in on]


def with_coord(data: bytes, coord: int, enc: int, value: int) -> bytearray:
    """`data` with one coordinate replaced by `value` (< 2^381, so no flag bit is touched); the flag bits of the slot are kept"""
    b = bytearray(data)
    off = coord_offset(coord, enc)
    flag_at, mask = (off + 47, 0xC0) if enc == 0 else (off, 0xE0)
    flags = b[flag_at] & mask
    b[off: off + 48] = value.to_bytes(48, "little" if enc == 0 else "big")
    b[flag_at] |= flags
    return b


def rejection_cases(compress: bool, enc: int) -> list:
    """[(name, bytes of one point, status)]"""
    G = pr.G2_GEN
    good = g2_bytes(G, compress, enc)
    n = len(good)
    outside = pr.g2_random_curve_points(1)[0]  # on the twist, not in G2
    cases = []

    def add(name, data, status):
        assert len(data) == n
        cases.append((name, bytes(data), status))

    if enc == 0:
        b = bytearray(good)
        b[n - 1] |= 0xC0
        add("flags = 3", b, BAD_ENCODING)
    else:
        b = bytearray(good)
        b[0] ^= 0x80
        add("compression bit wrong", b, BAD_ENCODING)
        if not compress:
            b = bytearray(good)
            b[0] |= 0x20
            add("sort flag on uncompressed", b, BAD_ENCODING)
        b = bytearray(n)
        b[0] = (0x80 if compress else 0) | 0x40 | 0x20
        add("sort flag on infinity", b, BAD_ENCODING)
    # a coordinate >= q, under the flag of the LARGER y: the arkworks framing compares the sign flag of an uncompressed point first, and
    # a y component >= q reads as larger than its negative
    larger = G if g2._f2_gt(G[1], g2.f2_neg(G[1])) else (G[0], g2.f2_neg(G[1]))
    for coord in range(2 if compress else 4):
        add(f"coordinate {coord} >= q", with_coord(g2_bytes(larger, compress, enc), coord, enc, pr.Q + 5), NONCANONICAL)
    if compress:
        add("x^3 + 4 (1 + u) is no square", g2_bytes(((real_x_split()[1][0], 0), (0, 0)), True, enc), NOT_ON_CURVE)
    else:
        add("off the twist", g2_bytes((G[0], ((G[1][0] + 1) % pr.Q, G[1][1])), False, enc), NOT_ON_CURVE)
    for at in (5, n - 7):
        b = bytearray(g2_bytes(None, compress, enc))
        b[at] = 1
        add(f"infinity with a non-zero byte at {at}", b, BAD_ENCODING)
    if enc == 0 and not compress:
        b = bytearray(good)
        b[n - 1] ^= 0x80
        add("sign flag does not match y", b, BAD_ENCODING)
        # the sign flag is compared BEFORE the canonical test, and a component >= q reads as larger than its negative: y.c1 + q under
        # the clear flag of the smaller y is a flag mismatch, not a non-canonical coordinate
        P = G if not g2._f2_gt(G[1], g2.f2_neg(G[1])) else (G[0], g2.f2_neg(G[1]))
        add("y.c1 >= q under a clear sign flag", with_coord(g2_bytes(P, False, 0), 3, 0, P[1][1] + pr.Q), BAD_ENCODING)
        # y.c1 = 0 hands the comparison to y.c0, where the same rule holds: y.c0 + q reads as larger.  Both rejections come before the
        # curve test, so y need not belong to x; 12345 + q < 2^382 leaves the flag bits free
        b = with_coord(g2_bytes((G[0], (12345, 0)), False, 0), 2, 0, 12345 + pr.Q)
        add("y.c1 = 0 and y.c0 >= q under a clear sign flag", b, BAD_ENCODING)
        b = bytearray(b)
        b[n - 1] |= 0x80
        add("y.c1 = 0 and y.c0 >= q under a set sign flag", b, NONCANONICAL)
    add("not in the subgroup", g2_bytes(outside, compress, enc), NOT_IN_SUBGROUP)
    return cases
