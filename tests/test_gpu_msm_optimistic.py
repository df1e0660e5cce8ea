"""GPU: the optimistic path of an unsplit one-call MSM (msm.hip: msm_run_one, k_sort1_staged_c / k_sort2_group with fixed bins,
k_boundary; gm_set_msm_optimistic / gm_debug_msm_optimistic).  Every result is compared, as an affine point, with the CPU Pippenger
of the oracle on the same inputs and with the same call under gm_set_msm_optimistic(0, 0).  The key has no fixed-base tables.

The read-out is (fixed bins gave the result, the boundary pass gave the result, parts whose check failed: 1 bins | 2 boundary,
calls run again so far, chunk length L of the accumulation).

The boundary pass is only tried where uniform scalars make a bucket of L + 2 entries unlikely (msm_enqueue: buckets x the Chernoff
bound of the Poisson tail <= 1): `boundary_tried` restates that rule.  Small calls run with L = 4 and well-filled buckets (n = 1000
has c = 6: 31 entries per bucket), so they keep the merge levels -- and are not run twice."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.util import assert_same_point

pytestmark = pytest.mark.gpu

N0 = (1 << 17) + 1  # the first size on the block sort at c = 16 (more than 2^21 entries)
BINS, BOUNDARY = 1, 2


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


def _opt(gm, bins, boundary):
    """sets the two parts; also resets the back-off"""
    gm.capi.check(gm.capi.load().gm_set_msm_optimistic(C.c_int(bins), C.c_int(boundary)))


def _readout(gm):
    out = (C.c_int * 5)()
    gm.capi.check(gm.capi.load().gm_debug_msm_optimistic(out))
    return list(out)


def _path(gm) -> int:
    out = C.c_int(-1)
    gm.capi.check(gm.capi.load().gm_debug_msm_sort_path(C.byref(out)))
    return out.value


@pytest.fixture(scope="module")
def key(gm, oracle):
    """2^17 + 9 points k_i * G without fixed-base tables, and their host copy"""
    import bench

    lib = gm.capi.load()
    gm.capi.check(lib.gm_set_auto_tables(C.c_int(0), C.c_size_t(0)))
    try:
        reg = gm.G1Bases.fixed_base(oracle.g1_generator(), bench.uniform_fr(np.random.default_rng(1723), N0 + 8))
    finally:
        gm.capi.check(lib.gm_set_auto_tables(C.c_int(1), C.c_size_t(0)))  # the library default
    host = reg.download()
    yield reg, host
    _opt(gm, 1, 1)
    gm.capi.check(lib.gm_set_msm_window(C.c_int(0)))
    reg.free()


def window_of(n: int) -> int:
    """choose_window of msm.hip for n <= 2^22 pairs"""
    lg = max(0, (n - 1).bit_length())
    return 16 if lg >= 14 else 8 if lg >= 11 else lg - 4 if lg >= 8 else lg + 1 if lg >= 5 else 4


def boundary_tried(n: int, c: int, L: int) -> bool:
    """msm_enqueue's rule for trying the boundary pass on a plain call of n pairs with window c and chunk length L"""
    W = (256 + c - 1) // c
    buckets = W << (c - 1)
    mean, k = n * W / buckets, L + 2.0
    return mean < k and buckets * math.exp(k - mean + k * math.log(mean / k)) <= 1.0


_cache = {}


def uniform(n):
    import bench

    if ("u", n) not in _cache:
        _cache[("u", n)] = bench.uniform_fr(np.random.default_rng(2000 + n % 977), n)
    return _cache[("u", n)]


def expected(oracle, host, name, sc):
    """the oracle's result for the named scalar set against the first len(sc) points, computed once"""
    if ("e", name) not in _cache:
        _cache[("e", name)] = oracle.msm_pippenger(host[: len(sc)], sc)
    return _cache[("e", name)]


def general(gm, reg, name, sc):
    """the same call with both parts off, computed once per scalar set"""
    if ("g", name) not in _cache:
        _opt(gm, 0, 0)
        try:
            _cache[("g", name)] = reg.msm_bigint(sc)
            assert _readout(gm)[:3] == [0, 0, 0]
        finally:
            _opt(gm, 1, 1)
    return _cache[("g", name)]


def test_uniform_first_size_on_the_block_sort(gm, oracle, key):
    """uniform scalars, 2^17 + 1 pairs: fixed bins, boundary pass, no repeat, every group loaded once; then each part alone"""
    reg, host = key
    sc = uniform(N0)
    exp, old = expected(oracle, host, "u0", sc), general(gm, reg, "u0", sc)
    try:
        _opt(gm, 1, 1)
        before = _readout(gm)[3]
        got = reg.msm_bigint(sc)
        ro = _readout(gm)
        assert ro[:3] == [1, 1, 0] and ro[3] == before and ro[4] == 18  # 2^21 + 16 entries over 131072 lanes, made even
        assert _path(gm) == 1
        assert_same_point(oracle, got, exp)
        assert (got == old).all()
        for bins, boundary in [(1, 0), (0, 1)]:
            _opt(gm, bins, boundary)
            part = reg.msm_bigint(sc)
            assert _readout(gm)[:3] == [bins, boundary, 0] and _path(gm) == 1
            assert (part == old).all()
    finally:
        _opt(gm, 1, 1)


@pytest.mark.parametrize("n", [1, 2, 63, 1000, 1 << 14])
def test_uniform_small_calls(gm, oracle, key, n):
    """below the block sort's 4-byte entries only the boundary pass can apply; no call is run twice"""
    reg, host = key
    sc = uniform(n)
    try:
        _opt(gm, 1, 1)
        before = _readout(gm)[3]
        got = reg.msm_bigint(sc)
        ro = _readout(gm)
        print(f"n = {n}: read-out {ro}")
        assert ro[0] == 0 and ro[2] == 0 and ro[3] == before
        assert ro[1] == int(boundary_tried(n, window_of(n), ro[4]))
        if n <= 2:
            assert ro[1] == 1
    finally:
        _opt(gm, 1, 1)
    assert_same_point(oracle, got, oracle.msm_pippenger(host[:n], sc))
    assert (got == general(gm, reg, f"u{n}", sc)).all()


def test_all_equal_scalars_fail_both_checks_once(gm, oracle, key):
    """all scalars equal, 2^17 + 1 pairs: every window is ONE coarse group (bin overflow) and ONE bucket (a run over every lane).
    The first call is run again -- both flags --, the second goes straight to the general path; uniform calls bring the fast
    path back"""
    reg, host = key
    sc = np.tile(oracle.random_fr(17, 1)[0], (N0, 1))
    exp, old = expected(oracle, host, "eq", sc), general(gm, reg, "eq", sc)
    u = uniform(N0)
    try:
        _opt(gm, 1, 1)
        before = _readout(gm)[3]
        got1 = reg.msm_bigint(sc)
        ro1, path1 = _readout(gm), _path(gm)
        got2 = reg.msm_bigint(sc)
        ro2, path2 = _readout(gm), _path(gm)
        assert ro1[:3] == [0, 0, BINS | BOUNDARY] and ro1[3] == before + 1
        assert ro2[:3] == [0, 0, 0] and ro2[3] == before + 1
        assert path1 == 2 and path2 == 2
        back = None
        for k in range(4):
            ug = reg.msm_bigint(u)
            if _readout(gm)[:3] == [1, 1, 0]:
                back = k
                break
        assert back is not None
        assert (ug == general(gm, reg, "u0", u)).all()
    finally:
        _opt(gm, 1, 1)
    assert_same_point(oracle, got1, exp)
    assert (got1 == old).all() and (got2 == old).all()


def test_long_run_without_a_sort_overflow(gm, oracle, key):
    """uniform scalars with 300 of them set to one value: the groups stay in their bins, a bucket of >= 300 entries spans 16 lanes
    of L = 18: the long-run flag rises, the call is run again once -- with the bins -- and is right"""
    reg, host = key
    sc = uniform(N0).copy()
    sc[np.random.default_rng(5).choice(N0, 300, replace=False)] = oracle.random_fr(23, 1)[0]
    try:
        _opt(gm, 1, 1)
        before = _readout(gm)[3]
        got = reg.msm_bigint(sc)
        ro = _readout(gm)
        assert ro[:3] == [1, 0, BOUNDARY] and ro[3] == before + 1
        assert _path(gm) == 1
    finally:
        _opt(gm, 1, 1)
    assert_same_point(oracle, got, oracle.msm_pippenger(host[:N0], sc))
    assert (got == general(gm, reg, "long", sc)).all()


def boundary_shapes(n, L, three):
    """n scalars below 2^15 whose sorted values 1, 2, 3, ... have these multiplicities: at c = 16 each makes one entry in window 0,
    so lane t of the accumulation holds sorted values [t L, (t + 1) L).  Lane 0 | 1: a bucket of two partials (tail + head).
    Lane 3: one bucket of exactly L entries between different neighbours.  three: a bucket of L + 2 entries from the last slot of
    lane 5 to the first slot of lane 7.  The last lane is a single run."""
    mult = [1] * (L - 1) + [2] + [1] * (2 * L - 1) + [L] + [1] * L
    if three:
        mult += [1] * (L - 1) + [L + 2] + [1] * (L - 1)
    last = n % L or L
    fill = n - last - sum(mult)
    assert fill % L == 0 and fill > 0
    mult += [1] * fill + [last]
    vals = np.repeat(np.arange(1, len(mult) + 1, dtype=np.uint64), mult)
    assert len(vals) == n and vals.max() < (1 << 15)
    sc = np.zeros((n, 4), dtype=np.uint64)
    sc[:, 0] = np.random.default_rng(11).permutation(vals)
    return sc


@pytest.mark.parametrize("three", [False, True])
def test_boundary_shapes(gm, oracle, key, three):
    reg, host = key
    n = 4096
    lib = gm.capi.load()
    gm.capi.check(lib.gm_set_msm_window(C.c_int(16)))
    try:
        _opt(gm, 1, 1)
        reg.msm_bigint(uniform(n))
        L = _readout(gm)[4]
        assert L == 4
        _opt(gm, 1, 1)  # whatever that call did, the next one is tried
        sc = boundary_shapes(n, L, three)
        before = _readout(gm)[3]
        got = reg.msm_bigint(sc)
        ro = _readout(gm)
        if three:
            assert ro[:3] == [0, 0, BOUNDARY] and ro[3] == before + 1
        else:
            assert ro[:3] == [0, 1, 0] and ro[3] == before
        _opt(gm, 0, 0)
        old = reg.msm_bigint(sc)
    finally:
        gm.capi.check(lib.gm_set_msm_window(C.c_int(0)))
        _opt(gm, 1, 1)
    assert_same_point(oracle, got, oracle.msm_pippenger(host[:n], sc))
    assert (got == old).all()


def test_scalar_of_2_255_fails_on_the_fixed_bins(gm, oracle, key):
    reg, host = key
    sc = uniform(N0)
    bad = sc.copy()
    bad[N0 // 3] = np.array([0, 0, 0, 1 << 63], dtype=np.uint64)
    _opt(gm, 1, 1)
    with pytest.raises(gm.capi.GeminiHipError) as ei:
        reg.msm_bigint(bad)
    assert ei.value.code == -1  # GM_EINVAL
    assert "a scalar passed as a canonical integer is >= 2^255" in str(ei.value)
    assert _path(gm) == 1  # ... on the 4-byte path
    got = reg.msm_bigint(sc)
    assert _readout(gm)[:3] == [1, 1, 0]
    assert (got == general(gm, reg, "u0", sc)).all()


def test_setter_rejects_other_values(gm):
    lib = gm.capi.load()
    for a, b in [(2, 0), (0, 2), (-1, 1), (1, -1)]:
        assert lib.gm_set_msm_optimistic(C.c_int(a), C.c_int(b)) == -1, (a, b)
    for a, b in [(0, 0), (1, 0), (0, 1), (1, 1)]:
        assert lib.gm_set_msm_optimistic(C.c_int(a), C.c_int(b)) == 0, (a, b)
    assert lib.gm_debug_msm_optimistic(None) == -1
