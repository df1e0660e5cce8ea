"""Fr values shared by the element-by-element tests (test_gpu_fr_edges.py, test_gpu_fr_blocks.py, test_fr_block_cases_cpu.py).

The vectors' Montgomery LIMBS are drawn from the values where a 32-bit-limb multiplier and its conditional subtraction can go wrong:
0, 1, r - 1, r - 2, all-ones words below the top, single words at every position.  What the device is given is the limbs m; the
field element they stand for is m 2^-256 mod r, and the reference computes on those; the limbs the device must give for a field
element v are v 2^256 mod r.  Every comparison is bit for bit."""
import numpy as np

from oracle import pyref

R = pyref.R_MOD
RINV = pow(1 << 256, -1, R)


def edge_limbs():
    """Montgomery limb patterns, every one a valid element (< r)"""
    top = R >> 224
    out = [0, 1, R - 1, R - 2, (1 << 224) - 1, (top << 224) - 1, top << 224, (R - 1) // 2, (R + 1) // 2, (1 << 256) % R]
    out += [1 << (32 * k) for k in range(1, 8)] + [0xFFFFFFFF << (32 * k) for k in range(7)]
    assert all(0 <= v < R for v in out) and len(set(out)) == len(out)
    return tuple(out)


EDGE = edge_limbs()


def limbs(ms) -> np.ndarray:
    """Montgomery integers -> (n, 4) uint64, as they are"""
    return np.array([[(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for m in ms], dtype=np.uint64).reshape(len(ms), 4)


def canon(ms):
    """the field elements the limbs stand for"""
    return [m * RINV % R for m in ms]


def mont(vs) -> np.ndarray:
    """field elements -> the limbs the device must give"""
    return limbs([v * (1 << 256) % R for v in vs])


EDGE_LIMBS, EDGE_CANON = limbs(EDGE), canon(EDGE)


class Vec:
    """a vector drawn from EDGE by index: the limbs for the device, the field elements for the reference"""

    def __init__(self, idx):
        self.idx = np.asarray(idx, dtype=np.int64) % len(EDGE)

    @property
    def limbs(self) -> np.ndarray:
        return EDGE_LIMBS[self.idx]

    @property
    def canon(self):
        return [EDGE_CANON[i] for i in self.idx.tolist()]


def vectors(n: int, shift: int):
    """two vectors cycling through the list with different strides, so every pair of edge values meets within 24^2 elements"""
    i = np.arange(n, dtype=np.int64)
    return Vec(i + shift), Vec(i // len(EDGE) + 3 * i + 2 * shift)


R_MINUS_1 = EDGE.index(R - 1)

# the list without 0, for products: one zero element makes everything below it 0 and hides every other value
EDGE_NZ = tuple(m for m in EDGE if m != 0)


def limbs_fast(ms) -> np.ndarray:
    """limbs() through int.to_bytes and np.frombuffer: the list comprehension of limbs() takes seconds at 2^19 elements"""
    buf = b"".join([m.to_bytes(32, "little") for m in ms])
    return np.frombuffer(buf, dtype="<u8").astype(np.uint64).reshape(len(ms), 4)


def mont_fast(vs) -> np.ndarray:
    """mont() through limbs_fast"""
    return limbs_fast([(v << 256) % R for v in vs])


def ints_of(l: np.ndarray):
    """(n, 4) uint64 limbs -> the integers they spell (the inverse of limbs_fast)"""
    buf = np.ascontiguousarray(l, dtype="<u8").tobytes()
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]
