"""GPU: gm_spm_bilinear_pm -- weights^T M powers at powers(beta) and powers(-beta) in one pass over the CSR matrix -- against two
independent statements: (a) the composition it replaces in the snark verifier, gm_fr_powers -> gm_spm_mul -> gm_fr_ip with +beta and
with -beta, on the unchanged kernels; (b) Python integers at the small sizes.  Field elements: equality is bit-exact.

The kernel walks a row per lane over a grid of at most 512 blocks of 256 lanes, so 2^17 + 3 rows is the first size at which a lane
takes a second row; the even / odd split of the column sums is what all-even and all-odd column sets pin (a swapped sign passes any
test whose columns mix parities evenly)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRID_LANES = 512 * 256


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


def _csr(rows):
    rowptr = np.zeros(len(rows) + 1, dtype=np.uint64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    cols = np.array([c for r in rows for _, c in r], dtype=np.uint32)
    return rowptr, cols, [v for r in rows for v, _ in r]


def _check(gm, pyref, rows, ncols, npowers=None, nweights=None, seed=1, ints=True):
    """rows: [[(value int, column)]]; powers has npowers entries (default ncols), weights nweights (default len(rows))"""
    from gemini_amd.circuit import SparseMatrix
    from gemini_amd.fr import FrVec, fr_from_int, fr_to_int, ip, powers

    R = pyref.R_MOD
    rng = pyref.SplitMix64(seed)
    nrows = len(rows)
    npowers = ncols if npowers is None else npowers
    nweights = nrows if nweights is None else nweights
    beta = rng.fr()
    w_int = [rng.fr() for _ in range(nweights)]
    rowptr, cols, vals = _csr(rows)
    vals_m = np.stack([fr_from_int(v) for v in vals]) if vals else np.empty((0, 4), dtype=np.uint64)
    M = SparseMatrix.from_csr(rowptr, cols, vals_m, nrows, ncols)
    w = FrVec.from_host(np.stack([fr_from_int(v) for v in w_int]) if w_int else np.empty((0, 4), dtype=np.uint64))
    bp = powers(fr_from_int(beta), npowers)
    pos, neg = M.bilinear_pm(bp, w)
    # (a) the composition on the existing kernels, once with beta and once with -beta
    w_cut = FrVec.from_host(w.to_host()[:nrows]) if nweights != nrows else w
    for got, point in ((pos, beta), (neg, (-beta) % R)):
        pw = powers(fr_from_int(point), npowers)
        y = M.mul(pw)
        assert (ip(y, w_cut) == got).all()
        pw.free()
        y.free()
    # (b) Python integers
    if ints:
        for got, point in ((pos, beta), (neg, (-beta) % R)):
            p = pyref.powers(point, npowers)
            want = sum(w_int[r] * sum(v * (p[c] if c < npowers else 0) for v, c in row) for r, row in enumerate(rows)) % R
            assert fr_to_int(got) == want
    if w_cut is not w:
        w_cut.free()
    for x in (M, w, bp):
        x.free()
    return pos, neg


def _random_rows(pyref, nrows, ncols, seed, max_entries=3, empty=()):
    rng = pyref.SplitMix64(seed)
    return [[] if r in empty else [(rng.fr(), int(rng.next() % ncols)) for _ in range(1 + int(rng.next() % max_entries))] for r in range(nrows)]


@pytest.mark.parametrize("nrows", [1, 63, 64, 65, 255, 257, 1025])
def test_sizes_around_the_wave_and_the_block(gm, pyref, nrows):
    """ncols = nrows, weights of length nrows and of the next power of two (tensor(rho) is that long)"""
    rows = _random_rows(pyref, nrows, nrows, 100 + nrows)
    _check(gm, pyref, rows, nrows, seed=nrows)
    _check(gm, pyref, rows, nrows, nweights=1 << max(nrows - 1, 1).bit_length(), seed=nrows + 1)


def test_more_rows_than_one_grid_sweep(gm, oracle, pyref):
    """2^17 + 3 rows of <= 2 entries: the last three rows are the second row of lanes 0..2.  Values and weights come from the C
    oracle's generator (Montgomery limbs as they are); the composition is the reference, and the tail rows -- alone in a second
    matrix -- are checked in integers as well."""
    from gemini_amd.circuit import SparseMatrix
    from gemini_amd.fr import FrVec, fr_from_int, fr_to_int, ip, powers

    R = pyref.R_MOD
    n = GRID_LANES + 3
    r = np.arange(n, dtype=np.uint64)
    second = (r % 3 == 0)
    counts = 1 + second.astype(np.uint64)
    rowptr = np.zeros(n + 1, dtype=np.uint64)
    rowptr[1:] = np.cumsum(counts)
    cols = np.zeros(int(rowptr[-1]), dtype=np.uint32)
    cols[rowptr[:-1].astype(np.int64)] = (r * 7919) % n
    cols[rowptr[:-1].astype(np.int64)[second] + 1] = ((r[second] * 104729) + 1) % n
    vals = oracle.fr_to_mont(oracle.random_fr(71, len(cols)))
    w_host = oracle.fr_to_mont(oracle.random_fr(72, n))
    beta = pyref.SplitMix64(73).fr()
    M = SparseMatrix.from_csr(rowptr, cols, vals, n, n)
    w = FrVec.from_host(w_host)
    bp = powers(fr_from_int(beta), n)
    pos, neg = M.bilinear_pm(bp, w)
    for got, point in ((pos, beta), (neg, (-beta) % R)):
        pw = powers(fr_from_int(point), n)
        y = M.mul(pw)
        assert (ip(y, w) == got).all()
        pw.free()
        y.free()
    # only the three rows past the first sweep: rows 0 .. n - 4 empty
    lo = int(rowptr[n - 3])
    tail_ptr = np.concatenate([np.zeros(n - 3, dtype=np.uint64), rowptr[n - 3:] - np.uint64(lo)])
    T = SparseMatrix.from_csr(tail_ptr, cols[lo:], vals[lo:], n, n)
    pos, neg = T.bilinear_pm(bp, w)
    for got, point in ((pos, beta), (neg, (-beta) % R)):
        want = 0
        for i in range(n - 3, n):
            row = sum(fr_to_int(vals[k]) * pow(point, int(cols[k]), R) for k in range(int(rowptr[i]), int(rowptr[i + 1])))
            want = (want + fr_to_int(w_host[i]) * row) % R
        assert fr_to_int(got) == want and want != 0
    for x in (M, T, w, bp):
        x.free()


def test_empty_rows_first_last_and_in_runs(gm, pyref):
    n = 200
    empty = {0, 1, 2, n - 1, n - 2} | set(range(60, 130)) | {140, 150}
    _check(gm, pyref, _random_rows(pyref, n, n, 21, empty=empty), n, seed=22)


def test_a_row_longer_than_a_wave_beside_one_entry_rows(gm, pyref):
    n = 70
    rng = pyref.SplitMix64(31)
    rows = [[(rng.fr(), int(rng.next() % 400))] for _ in range(n)]
    rows[33] = [(rng.fr(), c) for c in range(300)]
    _check(gm, pyref, rows, 400, seed=32)


def test_a_matrix_with_no_entries_and_one_with_no_rows(gm, pyref):
    pos, neg = _check(gm, pyref, [[] for _ in range(65)], 65, seed=41)
    assert not pos.any() and not neg.any()
    pos, neg = _check(gm, pyref, [], 5, seed=42)
    assert not pos.any() and not neg.any()


@pytest.mark.parametrize("parity", [0, 1])
def test_all_even_and_all_odd_columns(gm, pyref, parity):
    """with every column of one parity, neg = +pos (even) or -pos (odd): a swapped sign cannot pass"""
    from gemini_amd.fr import fr_to_int

    n = 129
    rng = pyref.SplitMix64(50 + parity)
    rows = [[(rng.fr(), 2 * int(rng.next() % 64) + parity) for _ in range(1 + int(rng.next() % 3))] for _ in range(n)]
    pos, neg = _check(gm, pyref, rows, n, seed=52 + parity)
    assert fr_to_int(pos) != 0
    assert fr_to_int(neg) == (fr_to_int(pos) if parity == 0 else (-fr_to_int(pos)) % pyref.R_MOD)


def test_fewer_columns_than_rows_and_columns_beyond_the_powers(gm, pyref):
    # ncols < nrows
    _check(gm, pyref, _random_rows(pyref, 300, 17, 61), 17, seed=62)
    # column indices >= len(powers) contribute zero, as in gm_spm_mul
    rows = _random_rows(pyref, 100, 100, 63)
    rows[5].append((12345, 99))
    rows[99].append((777, 64))
    _check(gm, pyref, rows, 100, npowers=64, seed=64)


def test_weights_too_short_and_unknown_handles(gm, pyref):
    from gemini_amd import capi
    from gemini_amd.circuit import SparseMatrix
    from gemini_amd.fr import FrVec, fr_from_int, powers

    n = 10
    rowptr, cols, vals = _csr([[(3, r)] for r in range(n)])
    M = SparseMatrix.from_csr(rowptr, cols, np.stack([fr_from_int(v) for v in vals]), n, n)
    bp = powers(fr_from_int(5), n)
    short = FrVec.alloc(n - 1)
    short.fill(fr_from_int(1))
    out = np.zeros(8, dtype=np.uint64)
    lib = capi.load()
    call = lambda m, p, w: lib.gm_spm_bilinear_pm(C.c_uint64(m), C.c_uint64(p), C.c_uint64(w), capi.ptr(out[:4]), capi.ptr(out[4:]))  # noqa: E731
    assert call(M.handle, bp.handle, short.handle) == -1  # GM_EINVAL: the reference's ip would panic
    assert call(M.handle + 1000, bp.handle, bp.handle) == -3  # GM_EHANDLE
    assert call(M.handle, bp.handle, M.handle) == -3  # a matrix handle is no vector
    assert call(M.handle, bp.handle, bp.handle) == 0
    for x in (M, bp, short):
        x.free()
