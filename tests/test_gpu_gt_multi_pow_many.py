"""GPU: gm_gt_multi_pow_many -- S independent GT multi-exponentiations in one launch (k_gt_multi_pow_seg and the k_gt_reduce_seg
levels of gemini_amd/csrc/pairing.hip).

Every compare is bit-exact.  A product is held against gm_gt_multi_pow on the same range and against the composition of the host
entries gm_gt_pow / gm_gt_mul, the pinned contract of the single entry; the long product against ONE host power of E on the logs.
"""
import ctypes as C
import threading

import numpy as np
import pytest

from gemini_amd import pairing as gp
from tests import gt_module_ref as GR
from tests.test_gpu_gt_module import DK, K0, R, host_multi_pow, nonmembers, rand_ints
from tests.test_pairing_cpu import gt_of_w

pytestmark = pytest.mark.gpu

GM_EINVAL = -1
LENGTHS = [0, 1, 2, 40, 40, 63, 64, 65, 130]  # the second 40 does not fit behind the first in a block of 64 and moves to the next
NPOOL = 48


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


@pytest.fixture(scope="module")
def pool(gm):
    """(E as limbs, logs k_i, E^k_i as an (NPOOL, 72) array through the host gm_gt_pow, five non-members): computed once, never modified"""
    e = gt_of_w(GR.E())
    k = [(K0 + i * DK) % R for i in range(NPOOL)]
    x = np.stack([gp.gt_pow(e, v) for v in k])
    bad = nonmembers(np.random.default_rng(0x6E6E), 5)
    for a in (e, x, bad):
        a.setflags(write=False)
    return e, k, x, bad


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.uintp)


def test_segment_lengths_and_edge_exponents(gm, pool):
    """lengths around the block of 64 in one call; members, non-members and the edge exponents spread over all products"""
    _, _, x, bad = pool
    rng = np.random.default_rng(0x5E61)
    off = offsets_of(LENGTHS)
    n = int(off[-1])
    xs = x[rng.integers(0, NPOOL, size=n)].copy()
    es = rand_ints(rng, n, 256)
    edge = [0, 1, R - 1, (1 << 256) - 1, 3, 1 << 255]
    for j, e in enumerate(edge):  # one of each in the product of 2, of 40, of 63 and of 130
        for s in (2, 3, 5, 8):
            es[int(off[s]) + (7 * j + s) % LENGTHS[s]] = e
    # non-members: a random one in the single-term product, a random one and the 1 + 0 w in the product of 65 (0 would swallow it)
    xs[int(off[1])] = bad[0]
    xs[int(off[7]) + 9], xs[int(off[7]) + 64] = bad[2], bad[3]
    got = gm.gt_multi_pow_many(xs, es, off)
    assert got.shape == (len(LENGTHS), 72)
    for s, m in enumerate(LENGTHS):
        lo, hi = int(off[s]), int(off[s + 1])
        assert (got[s] == gm.gt_multi_pow(xs[lo:hi], es[lo:hi])).all(), ("gm_gt_multi_pow", s, m)
        assert (got[s] == host_multi_pow(xs[lo:hi], es[lo:hi])).all(), ("gm_gt_pow / gm_gt_mul", s, m)
    assert (got[0] == gm.gt_one()).all()


def test_zero_swallows_only_its_own_product(gm, pool):
    """0^e = 0 (e != 0) and 0^0 = 1 as gm_gt_pow has them, next to products that must not notice"""
    _, _, x, bad = pool
    xs = np.stack([x[0], bad[1], x[1], x[2], bad[1], x[3], x[4]])
    es = [5, 7, 11, 13, 0, 17, 19]
    off = offsets_of([3, 1, 2, 1])
    got = gm.gt_multi_pow_many(xs, es, off)
    assert not got[0].any() and got[1:].any(axis=1).all()
    for s in range(4):
        lo, hi = int(off[s]), int(off[s + 1])
        assert (got[s] == host_multi_pow(xs[lo:hi], es[lo:hi])).all(), s


def test_two_reduction_levels_between_short_products(gm, pool):
    """4097 terms: 65 partials of the exponentiation launch, 2 of the first reduction level, 1 of the second.  On the logs the product
    is ONE host power of E."""
    e, k, x, _ = pool
    rng = np.random.default_rng(0x1001)
    lengths = [3, 4097, 2]
    off = offsets_of(lengths)
    n = int(off[-1])
    sel = rng.integers(0, NPOOL, size=n)
    es = [v % R for v in rand_ints(rng, n)]
    got = gm.gt_multi_pow_many(x[sel], es, off)
    for s in range(3):
        lo, hi = int(off[s]), int(off[s + 1])
        log = sum(k[i] * v for i, v in zip(sel[lo:hi], es[lo:hi])) % R
        assert (got[s] == gp.gt_pow(e, log)).all(), s
    assert (got[1] == gm.gt_multi_pow(x[sel[3:4100]], es[3:4100])).all()


def test_empty_calls_and_refusals(gm, pool):
    _, _, x, _ = pool
    lib, ptr = gm.capi.load(), gm.capi.ptr
    assert gm.gt_multi_pow_many(x[:0], [], [0]).shape == (0, 72)  # S = 0
    assert lib.gm_gt_multi_pow_many(None, None, None, C.c_size_t(0), None) == 0
    got = gm.gt_multi_pow_many(x[:0], [], [0, 0, 0])  # every product empty
    assert (got == gm.gt_one()).all() and got.shape == (2, 72)
    xs, sc, out = np.array(x[:4]), np.ones((4, 4), dtype=np.uint64), np.zeros((2, 72), dtype=np.uint64)

    def call(px, ps, off, S, po):
        o = np.array(off, dtype=np.uintp)
        return lib.gm_gt_multi_pow_many(px, ps, ptr(o), C.c_size_t(S), po)

    assert call(ptr(xs), ptr(sc), [0, 2, 4], 2, ptr(out)) == 0
    assert call(ptr(xs), ptr(sc), [0, 3, 2], 2, ptr(out)) == GM_EINVAL  # descending
    assert call(ptr(xs), ptr(sc), [1, 2, 4], 2, ptr(out)) == GM_EINVAL  # offsets[0] != 0
    assert call(None, ptr(sc), [0, 2, 4], 2, ptr(out)) == GM_EINVAL and call(ptr(xs), None, [0, 2, 4], 2, ptr(out)) == GM_EINVAL
    assert call(ptr(xs), ptr(sc), [0, 2, 4], 2, None) == GM_EINVAL
    assert lib.gm_gt_multi_pow_many(ptr(xs), ptr(sc), None, C.c_size_t(2), ptr(out)) == GM_EINVAL
    assert call(ptr(xs), ptr(sc), [0, 2, (1 << 20) + 1], 2, ptr(out)) == GM_EINVAL  # more than 2^20 terms: refused before anything is read


def test_two_threads(gm, pool):
    _, _, x, _ = pool
    got, errs = [None, None], []
    inputs = []
    for t in range(2):
        rng = np.random.default_rng(0x7400 + t)
        lengths = [5, 70, 1] if t == 0 else [64, 2, 33]
        n = sum(lengths)
        inputs.append((x[rng.integers(0, NPOOL, size=n)].copy(), rand_ints(rng, n, 256), offsets_of(lengths)))

    def run(t):
        try:
            got[t] = [gm.gt_multi_pow_many(*inputs[t]) for _ in range(2)]
        except Exception as e:  # noqa: BLE001 -- reported below with the thread index
            errs.append((t, e))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errs, errs
    for t in range(2):
        xs, es, off = inputs[t]
        for s in range(3):
            lo, hi = int(off[s]), int(off[s + 1])
            exp = host_multi_pow(xs[lo:hi], es[lo:hi])
            assert (got[t][0][s] == exp).all() and (got[t][1][s] == exp).all(), (t, s)
