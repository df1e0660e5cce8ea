"""GPU: the block sort of a plain one-call MSM with 4-byte pass-1 entries and one block per coarse group (msm.hip:
k_sort1_staged_c, k_sort2_group; gm_set_msm_sort_group / gm_debug_msm_sort_path).  Every result is compared, as an affine point,
with the CPU Pippenger of the oracle on the same inputs and with the same call through the 8-byte passes (mode 0); the path
read-out says which kernels ran: 0 the 8-byte passes, 1 every group loaded once, 2 at least one group chunked.

Sizes are the smallest that reach the code: 2^17 + 1 pairs is the first size on the block sort at c = 16 (more than 2^21 entries),
2^21 pairs fills the 21 index bits of an entry, 2^21 + 1 no longer fits."""
import ctypes as C

import numpy as np
import pytest

from tests.util import assert_same_point, jac_to_affine_ints

pytestmark = pytest.mark.gpu

N0 = (1 << 17) + 1
NMAX = 1 << 21
CAP_MAX = (160 * 1024 - 3 * 1024 * 4 - 64) // 4  # MSM_SORT_GROUP_CAP_MAX (ctx.hpp)


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


def _mode(gm, mode, cap=0):
    gm.capi.check(gm.capi.load().gm_set_msm_sort_group(C.c_int(mode), C.c_size_t(cap)))


def _path(gm) -> int:
    out = C.c_int(-1)
    gm.capi.check(gm.capi.load().gm_debug_msm_sort_path(C.byref(out)))
    return out.value


@pytest.fixture(scope="module")
def key(gm):
    """2^21 + 8 points k_i * G WITHOUT fixed-base tables (the plain path is the one under test), and their host copy"""
    import bench

    lib = gm.capi.load()
    gm.capi.check(lib.gm_set_auto_tables(C.c_int(0), C.c_size_t(0)))
    try:
        reg = gm.G1Bases.fixed_base(_generator(), bench.uniform_fr(np.random.default_rng(1721), NMAX + 8))
    finally:
        gm.capi.check(lib.gm_set_auto_tables(C.c_int(1), C.c_size_t(0)))  # the library default
    host = reg.download()
    yield reg, host
    _mode(gm, 1)
    reg.free()


def _generator():
    from oracle import oracle as orc

    return orc.g1_generator()


def coarse_group_sizes(sc, c=16, fb=10):
    """entries per coarse group (window, bucket >> fb) of the block sort: the signed digits of msm.hip's DigitIter"""
    sc = np.ascontiguousarray(sc, dtype=np.uint64).reshape(-1, 4)
    per, gpw = 64 // c, 1 << (c - 1 - fb)
    W = 4 * per
    sizes = np.zeros(W * gpw, dtype=np.int64)
    carry = np.zeros(len(sc), dtype=np.int64)
    for w in range(W):
        d = ((sc[:, w // per] >> np.uint64(c * (w % per))) & np.uint64((1 << c) - 1)).astype(np.int64) + carry
        if w < W - 1:
            carry = (d + (1 << (c - 1))) >> c
            d = d - (carry << c)
        mag = np.abs(d)
        sizes[w * gpw:(w + 1) * gpw] = np.bincount((mag[mag != 0] - 1) >> fb, minlength=gpw)[:gpw]
    return sizes


_inputs = {}


def scalars(oracle, pyref, kind, n=N0):
    """canonical scalars (n, 4), made once per kind"""
    if (kind, n) in _inputs:
        return _inputs[(kind, n)]
    import bench

    sc = bench.uniform_fr(np.random.default_rng(1000 + n % 977), n)
    if kind == "zero":
        sc = np.zeros_like(sc)
    elif kind == "equal":
        sc = np.tile(oracle.random_fr(17, 1)[0], (n, 1))
    elif kind == "special":
        r = pyref.R_MOD
        half = [sum(0x8000 << (16 * w) for w in ws) for ws in ([0], [0, 3, 7], [1, 2, 14], list(range(0, 15, 2)))]  # digits -2^15: bucket 32 767
        vals = [0, 1, r - 1, 1 << 254, (1 << 15) - 1, 0x8001] + half + [r - h for h in half] + [h + (0x73EC << 240) for h in half]
        special = oracle.ints_to_limbs(vals, 4)
        for rep in range(5):  # in the first and the last sort block, and at a few places between
            at = rep * (n - len(special)) // 4
            sc[at:at + len(special)] = special
    else:
        assert kind == "uniform"
    _inputs[(kind, n)] = sc
    return sc


_expected = {}


def expected(oracle, host, kind, sc, lo, hi, rev=False):
    """the oracle's result for scalars `kind` against host[lo:hi] (reversed: walked downwards), computed once"""
    k = (kind, len(sc), lo, hi, rev)
    if k not in _expected:
        b = host[lo:hi]
        _expected[k] = oracle.msm_pippenger(np.ascontiguousarray(b[::-1]) if rev else b, sc)
    return _expected[k]


PATH_OF = {"uniform": 1, "zero": 1, "equal": 2, "special": 1}


@pytest.mark.parametrize("variant", ["plain", "mont", "slice"])
@pytest.mark.parametrize("kind", ["uniform", "zero", "equal", "special"])
def test_first_size_on_the_block_sort(gm, oracle, pyref, key, kind, variant):
    """2^17 + 1 pairs: uniform scalars; all-zero scalars (no entries at all: the identity); all-equal scalars (one group of n entries
    per window, chunked under the default capacity: path 2); 0, 1, r - 1, 2^254 and digits of exactly -2^15 (bucket 32 767, the last
    slot of a group) -- as canonical integers, as Montgomery values of a device vector, and against a slice of the key walked
    downwards from base n + 6."""
    from gemini_amd.fr import FrVec

    reg, host = key
    sc = scalars(oracle, pyref, kind)
    n = len(sc)
    if variant == "slice":
        call = lambda: reg.msm_bigint(sc, offset=n + 6, reversed_=True)  # noqa: E731
        exp = expected(oracle, host, kind, sc, 7, n + 7, rev=True)
    elif variant == "mont":
        vec = FrVec.from_host(oracle.fr_to_mont(sc))
        call = lambda: reg.msm_vec(vec, n=n)  # noqa: E731
        exp = expected(oracle, host, kind, sc, 0, n)
    else:
        call = lambda: reg.msm_bigint(sc)  # noqa: E731
        exp = expected(oracle, host, kind, sc, 0, n)
    try:
        _mode(gm, 1)
        got = call()
        path = _path(gm)
        _mode(gm, 0)
        old = call()
        assert _path(gm) == 0
    finally:
        _mode(gm, 1)
        if variant == "mont":
            vec.free()
    assert path == PATH_OF[kind]
    assert_same_point(oracle, got, exp)
    assert (got == old).all()
    if kind == "zero":
        assert jac_to_affine_ints(oracle, got) is None


@pytest.mark.parametrize("cap", [4096, "largest - 1"])
def test_ordinary_input_through_the_chunked_branch(gm, oracle, pyref, key, cap):
    """uniform scalars with the capacity of a block set below group sizes: about half of the groups (cap 4096, the mean size), or only
    the largest one with a last chunk of ONE entry (cap = largest group - 1), take the counting sweep + the chunks"""
    reg, host = key
    sc = scalars(oracle, pyref, "uniform")
    sizes = coarse_group_sizes(sc)
    if cap != 4096:
        cap = int(sizes.max()) - 1
    assert 1024 <= cap and (sizes > cap).sum() >= 1
    try:
        _mode(gm, 1, cap)
        got = reg.msm_bigint(sc)
        path = _path(gm)
    finally:
        _mode(gm, 1)
    assert path == 2
    assert_same_point(oracle, got, expected(oracle, host, "uniform", sc, 0, len(sc)))
    assert (got == reg.msm_bigint(sc)).all() and _path(gm) == 1


def test_2_18_default_capacity_loads_every_group_once(gm, oracle, pyref, key):
    reg, host = key
    n = 1 << 18
    sc = scalars(oracle, pyref, "uniform", n)
    assert coarse_group_sizes(sc).max() <= CAP_MAX
    try:
        got = reg.msm_bigint(sc)
        assert _path(gm) == 1
        _mode(gm, 0)
        old = reg.msm_bigint(sc)
        assert _path(gm) == 0
    finally:
        _mode(gm, 1)
    assert_same_point(oracle, got, expected(oracle, host, "uniform", sc, 0, n))
    assert (got == old).all()


def test_2_21_fills_the_entry(gm, oracle, pyref, key):
    """2^21 pairs: the pair index needs all 21 bits, the entry is full at 32; the groups (65 Ki entries) are chunked"""
    reg, host = key
    sc = scalars(oracle, pyref, "uniform", NMAX).copy()
    sc[-1] = oracle.ints_to_limbs([pyref.R_MOD - 1], 4)[0]  # the last index, with a negative digit in window 0
    try:
        got = reg.msm_bigint(sc)
        assert _path(gm) == 2
        _mode(gm, 0)
        old = reg.msm_bigint(sc)
        assert _path(gm) == 0
    finally:
        _mode(gm, 1)
    assert_same_point(oracle, got, oracle.msm_pippenger(host[:NMAX], sc))
    assert (got == old).all()


def test_2_21_plus_1_keeps_the_8_byte_passes(gm, oracle, pyref, key):
    """one pair more and index + sign + fine key bits are 33 bits: path 0 whatever the mode; as is a 2^17-pair prefix (2^21 entries:
    the flat sort), which is checked against the oracle"""
    reg, host = key
    n = NMAX + 1
    sc = scalars(oracle, pyref, "uniform", n)
    try:
        got = reg.msm_bigint(sc)
        assert _path(gm) == 0
        pre = reg.msm_bigint(sc[: 1 << 17])
        assert _path(gm) == 0
        _mode(gm, 0)
        old = reg.msm_bigint(sc)
    finally:
        _mode(gm, 1)
    assert (got == old).all()
    assert_same_point(oracle, pre, oracle.msm_pippenger(host[: 1 << 17], sc[: 1 << 17]))


def test_scalar_beyond_2_255_still_fails(gm, oracle, pyref, key):
    reg, host = key
    sc = scalars(oracle, pyref, "uniform")
    bad = sc.copy()
    bad[len(sc) // 2, 3] |= np.uint64(1 << 63)
    with pytest.raises(gm.capi.GeminiHipError) as ei:
        reg.msm_bigint(bad)
    assert ei.value.code == -1  # GM_EINVAL
    assert _path(gm) == 1  # ... on the compact path
    assert_same_point(oracle, reg.msm_bigint(sc), expected(oracle, host, "uniform", sc, 0, len(sc)))


def test_batch_takes_the_new_path_without_harm(gm, oracle, pyref, key):
    """msm_vec_batch of {2^18, 2^17 + 1, 2^12} pairs equals the one-call results"""
    from gemini_amd.fr import FrVec

    reg, host = key
    sizes = [1 << 18, N0, 1 << 12]
    vecs = [FrVec.from_host(oracle.fr_to_mont(scalars(oracle, pyref, "uniform", m))) for m in sizes]
    try:
        single = [reg.msm_vec(v, n=m) for v, m in zip(vecs, sizes)]
        got = reg.msm_vec_batch(vecs, sizes)
    finally:
        for v in vecs:
            v.free()
    assert all((got[j] == single[j]).all() for j in range(len(sizes)))
    assert_same_point(oracle, got[1], expected(oracle, host, "uniform", scalars(oracle, pyref, "uniform"), 0, N0))
    assert_same_point(oracle, got[2], oracle.msm_pippenger(host[: 1 << 12], scalars(oracle, pyref, "uniform", 1 << 12)))


def test_setter_rejects_what_does_not_fit(gm):
    lib = gm.capi.load()
    for mode, cap in [(2, 0), (-1, 0), (1, CAP_MAX + 1), (1, 1023), (0, 1 << 40)]:
        assert lib.gm_set_msm_sort_group(C.c_int(mode), C.c_size_t(cap)) == -1, (mode, cap)
    for mode, cap in [(1, CAP_MAX), (1, 1024), (1, 0)]:
        assert lib.gm_set_msm_sort_group(C.c_int(mode), C.c_size_t(cap)) == 0, (mode, cap)
