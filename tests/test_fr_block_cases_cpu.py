"""No GPU: the block references of tests/fr_block_cases.py against the whole-vector references (oracle/psnark_ref.py, oracle/pyref.py)
on every size and tiling test_gpu_fr_blocks.py uses, and the teeth of those shapes and values -- a model of each way a block builder
can be wrong must differ from the whole reference on every tiling of more than one block."""
import time

import numpy as np
import pytest

from oracle import psnark_ref as pr
from oracle import pyref
from tests import fr_block_cases as bc
from tests import fr_cases as fc

R = fc.R
Y, Z, ZETA, X = fc.canon([fc.EDGE[5], bc.RANDOM_M, R - 1, bc.RANDOM_M])


def rhos_for(k: int, pattern: str = "scalars"):
    """k field elements: the scalars of the GPU tests in turn, or k distinct ones"""
    if pattern == "scalars":
        return fc.canon([bc.SCALARS_M[(j + 2) % len(bc.SCALARS_M)] for j in range(k)])
    return [pow(bc.RANDOM_M, j + 2, R) for j in range(k)]


def test_sizes_cross_the_thresholds():
    assert bc.SIZES == sorted(set(bc.SIZES)) and bc.SIZES[0] == 1
    assert bc.ACC_K + 1 in bc.SIZES and bc.SEGN + 1 in bc.SIZES and 2 * bc.SEGN + 1 in bc.SIZES  # second chunk, second and third segment
    assert bc.LARGE == bc.GRID_CAP * bc.LANES + 1 and bc.POWERS_COUNTS[-1] == bc.POWERS_CAP * bc.LANES + 1
    assert (bc.FOLD_LENGTHS[-1] + 1) // 2 == bc.LARGE
    for n in bc.SIZES + [bc.LARGE]:
        t = bc.tilings(n)
        assert t["one"] == [0, n + 1]
        assert any(b[-1] == (n, 0, 1) for b in (bc.blocks(c, n) for c in t.values()))  # a block with no input and one output
        assert all(sum(b[2] for b in bc.blocks(c, n)) == n + 1 and sum(b[1] for b in bc.blocks(c, n)) == n for c in t.values())
    t = bc.tilings(2 * bc.SEGN + 1)
    assert t["acc"][1:-1] == bc.ACC_CUTS and [b - a for a, b in zip(t["ones"], t["ones"][1:])][:3] == [1, 1, 1]
    assert [b - a for a, b in zip(t["ones"], t["ones"][1:])][-3:] == [1, 1, 1]
    assert bc.tilings(bc.SEGN)["multiple4"] == [0, bc.SEGN // 4, bc.SEGN // 2, 3 * bc.SEGN // 4, bc.SEGN, bc.SEGN + 1]
    assert bc.tilings(bc.SEGN)["world2"] == [0, bc.SEGN, bc.SEGN + 1]


def test_fast_conversions():
    ms = list(fc.EDGE) + fc.ints_of(bc.random_limbs(3, 50))
    assert (fc.limbs_fast(ms) == fc.limbs(ms)).all() and fc.limbs_fast(ms).dtype == np.uint64
    vs = fc.canon(ms)
    assert (fc.mont_fast(vs) == fc.mont(vs)).all() and (fc.mont_fast(vs) == fc.limbs(ms)).all()
    assert fc.ints_of(fc.limbs(ms)) == ms
    assert 0 not in fc.EDGE_NZ and len(fc.EDGE_NZ) == len(fc.EDGE) - 1
    for kind in bc.KINDS:
        l, c = bc.values(kind, 100)
        assert fc.ints_of(l) == [v * (1 << 256) % R for v in c] and all(0 <= v < R for v in c)
    assert 0 in bc.values("edge", 100)[1] and 0 not in bc.values("edge", 100, nonzero=True)[1] and bc.values("edge", 1)[1][0] != 0


@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("n", bc.SIZES)
def test_blocks_concatenate_to_the_whole(n, kind):
    _, v = bc.values(kind, n)
    _, w = bc.values(kind, n, nonzero=True)
    want_set, want_rot = pr.plookup_set(v, Y, Z), pr.right_rotation(pr.monic(v))
    want_acc, want_acc0, want_hash = pr.accumulated_product(pr.monic(w)), pr.accumulated_product(pr.monic(v)), pr.alg_hash(v, range(n), ZETA)
    want_pow = pyref.powers(X, n + 1)
    for name, cuts in bc.tilings(n).items():
        assert bc.tiled_plookup_set(v, cuts, Y, Z) == want_set, name
        assert bc.tiled_shift(v, cuts) == want_rot, name
        assert bc.tiled_acc_product(w, cuts) == want_acc, name
        assert bc.tiled_acc_product(v, cuts) == want_acc0, name  # with the zeros of the edge list
        bl = bc.blocks(cuts, n)
        assert sum((bc.alg_hash_from(v[lo:lo + nin], lo, ZETA) for lo, nin, _ in bl), []) == want_hash, name
        assert sum((bc.powers_range(X, lo, nout) for lo, _, nout in bl), []) == want_pow, name
    assert bc.product(w) == pr.product(w) == want_acc[0] and bc.product([]) == 1


@pytest.mark.parametrize("k", [k for k in bc.TENSOR_KS if k <= 10] + [13])
def test_tensor_ranges_concatenate_to_the_whole(k):
    for pattern in ("scalars", "distinct"):
        rhos = rhos_for(k, pattern)
        want = pyref.tensor(rhos)
        assert [bc.tensor_at(rhos, i) for i in range(1 << k)] == want
        for name, cuts in bc.tilings((1 << k) - 1).items():  # 2^k outputs
            assert sum((bc.tensor_range(rhos, a, b - a) for a, b in zip(cuts, cuts[1:])), []) == want, name
        for start, count in bc.tensor_ranges(k):
            assert bc.tensor_range(rhos, start, count) == want[start:start + count]


def test_the_ranges_and_gathers_of_the_gpu_tests():
    rhos = rhos_for(20, "distinct")
    want = pyref.tensor(rhos)
    for start, count in bc.tensor_ranges(20):
        assert bc.tensor_range(rhos, start, count) == want[start:start + count]
    assert (0, bc.LARGE) in bc.tensor_ranges(20) and ((1 << 10) - 1, 257) in bc.tensor_ranges(20)
    assert ((1 << 32) - 257, 257) in bc.tensor_ranges(32) and max(c for _, c in bc.tensor_ranges(32)) == 257
    rhos = rhos_for(32, "distinct")
    for start, count in bc.tensor_ranges(32):
        got = bc.tensor_range(rhos, start, count)
        assert got[0] == bc.tensor_at(rhos, start) and got[-1] == bc.tensor_at(rhos, start + count - 1)
    for start in bc.POWERS_STARTS:
        got = bc.powers_range(X, start, 257)
        assert got[0] == pow(X, start, R) and got[100] == pow(X, start + 100, R)
    assert bc.powers_range(0, 0, 3) == [1, 0, 0] and bc.powers_gather(0, [0, 1, 0]) == [1, 0, 1]
    for k in bc.TENSOR_KS:
        rhos = rhos_for(k, "distinct")
        for name, idx in bc.gather_indices(k, 300).items():
            idx = idx.tolist()
            assert all(0 <= i < (1 << k) for i in idx), name
            assert bc.tensor_gather_bytes(rhos, idx) == bc.tensor_gather(rhos, idx) == [bc.tensor_at(rhos, i) for i in idx], (k, name)
            assert bc.powers_gather_bytes(X, idx) == bc.powers_gather(X, idx) == [pow(X, i, R) for i in idx], (k, name)
        ix = bc.gather_indices(k, 300)
        assert (ix["sorted"][1:] >= ix["sorted"][:-1]).all() and (ix["top"] == (1 << k) - 1).all()
        if k >= 2:
            assert {(1 << bc.klo_of(k)) - 1, 1 << bc.klo_of(k)} <= set(ix["alternating"].tolist())


def test_fold_scale_add_references():
    f = bc.values("edge", 9)[1]
    levels = bc.fold_chain(f, [Y, Z, 0, 1, X, X])
    cur = f
    for lv, r in zip(levels, [Y, Z, 0, 1, X, X]):
        cur = pyref.fold_polynomial(cur, r)
        assert lv == cur
    assert [len(lv) for lv in levels] == [5, 3, 2, 1, 1, 1] and levels[-1] == levels[-2]
    assert bc.scale_into_many([7, 7, 7, 7, 7], [[1, 2], [], [3]], [5, 9, R - 1], [1, 3, 4]) == [7, 5, 10, 7, R - 3]
    assert bc.add_at([R - 1, 5, R - 1], [2, 0], [R - 1, 1]) == [0, 5, R - 2]


def test_reference_cost_at_the_large_size():
    """the references alone at 2^19 + 1 elements, every tiling: a few seconds"""
    n = bc.LARGE
    t0 = time.perf_counter()
    l, v = bc.values("edge", n)
    want_set, want_rot, want_hash = pr.plookup_set(v, Y, Z), pr.right_rotation(pr.monic(v)), pr.alg_hash(v, range(n), ZETA)
    for name, cuts in bc.tilings(n).items():
        assert bc.tiled_plookup_set(v, cuts, Y, Z) == want_set, name
        assert bc.tiled_shift(v, cuts) == want_rot, name
        assert sum((bc.alg_hash_from(v[lo:lo + nin], lo, ZETA) for lo, nin, _ in bc.blocks(cuts, n)), []) == want_hash, name
    assert (fc.mont_fast(v) == l).all()
    dt = time.perf_counter() - t0
    print("references at n = %d over %d tilings: %.2f s" % (n, len(bc.tilings(n)), dt))
    assert dt < 20.0


# ---- teeth: models of the ways a block builder can be wrong ---------------------------------------------------------------------------
def wrong_plookup_set(v, cuts, y, z, how):
    out = []
    for lo, nin, nout in bc.blocks(cuts, len(v)):
        prev = None if lo == 0 or how == "dropped" else (v[lo] if nin else 0)  # "own": the block's own first element
        out += bc.plookup_set_block(v[lo:lo + nin], prev, nout, y, z)
    return out


def wrong_shift(v, cuts, how):
    out = []
    for lo, nin, nout in bc.blocks(cuts, len(v)):
        first = 1 if lo == 0 or how == "dropped" else (v[lo] if nin else 0)
        out += bc.shift_block(v[lo:lo + nin], first, nout)
    return out


def wrong_acc_product(v, cuts, how):
    bl = bc.blocks(cuts, len(v))
    prods = [bc.product(v[lo:lo + nin]) for lo, nin, _ in bl]
    cs = bc.carries(prods)
    if how == "below":  # the product of the blocks below instead of above
        cs = list(reversed(bc.carries(list(reversed(prods)))))
    out = []
    for j, ((lo, nin, nout), c) in enumerate(zip(bl, cs)):
        monic = (j == 0) if how == "monic_first" else (nout == nin + 1)
        out += bc.acc_product_block(v[lo:lo + nin], c, monic)
    return out


def tensor_split(rhos, idx, split):
    """the device's two half tables (low: rhos[:klo], high: rhos[klo:]) addressed with an index cut at bit `split`: tensor(rhos)[idx]
    for split = klo.  A bit that addresses past a table counts as absent."""
    k, klo = len(rhos), bc.klo_of(len(rhos))
    a, b = idx & ((1 << split) - 1), idx >> split
    return bc.tensor_at(rhos[:klo], a & ((1 << klo) - 1)) * bc.tensor_at(rhos[klo:], b & ((1 << (k - klo)) - 1)) % R


MULTI = [(n, name, cuts) for n in bc.SIZES for name, cuts in bc.tilings(n).items() if len(cuts) > 2]


@pytest.mark.parametrize("kind", bc.KINDS)
def test_teeth_of_the_halos(kind):
    """A dropped halo shows on every tiling with every pattern.  The halo taken from the block's own first element cannot show in the
    all-(r - 1) vector, where every element equals its neighbour: the cycling edge list and the random vector carry that one."""
    for n, name, cuts in MULTI:
        _, v = bc.values(kind, n)
        for how in ("dropped", "own"):
            if how == "own" and kind == "rm1":
                continue
            assert wrong_plookup_set(v, cuts, Y, Z, how) != pr.plookup_set(v, Y, Z), (n, name, how)
            assert wrong_shift(v, cuts, how) != pr.right_rotation(pr.monic(v)), (n, name, how)


@pytest.mark.parametrize("kind", bc.KINDS)
def test_teeth_of_the_carries(kind):
    """The monic entry written by the first block shows with every pattern, wherever a block above the first holds an input (where
    none does, the first block's carry is the monic entry: the same vector, and the GPU test tells the two by the blocks' lengths).  The carry taken from the blocks below shows with the
    cycling edge list (without 0) and the random vector; in the all-(r - 1) vector every product is 1 or r - 1 by the parity of its
    length alone, so a tiling whose blocks below and above have the same parity hides it: that pattern is left to the other two."""
    for n, name, cuts in MULTI:
        _, v = bc.values(kind, n, nonzero=True)
        want = pr.accumulated_product(pr.monic(v))
        if bc.blocks(cuts, n)[0][1] < n:
            assert wrong_acc_product(v, cuts, "monic_first") != want, (n, name)
        if kind != "rm1":
            assert wrong_acc_product(v, cuts, "below") != want, (n, name)
        assert wrong_acc_product(v, cuts, "right") == want


def test_teeth_of_start_and_klo():
    """start off by one, on every block but the lowest (tensor: one below; powers and hash: one above), and the index cut one bit
    beside klo.  rhos: distinct elements and the scalars of the GPU tests in turn (0, 1 and r - 1 among them).  One rho that is 0 leaves
    half the tensor 0 -- a block that lies in that half cannot see its start move, so the start is held against the distinct elements --
    and a tensor of 1 and r - 1 alone depends on the parity of the index only: the GPU tests use both patterns."""
    for k in (2, 3, 9, 10):
        for pattern in ("distinct", "scalars"):
            rhos = rhos_for(k, pattern)
            want = pyref.tensor(rhos)
            for name, cuts in bc.tilings((1 << k) - 1).items():
                if len(cuts) > 2 and pattern == "distinct":
                    assert sum((bc.tensor_range(rhos, a - (1 if a else 0), b - a) for a, b in zip(cuts, cuts[1:])), []) != want, (k, name)
            assert [tensor_split(rhos, i, bc.klo_of(k)) for i in range(1 << k)] == want
            if k >= 3:
                for d in (-1, 1):
                    assert [tensor_split(rhos, i, bc.klo_of(k) + d) for i in range(1 << k)] != want, (k, pattern, d)
    for k in (20, 32):  # the range that straddles 2^klo sees a cut beside klo
        rhos, klo = rhos_for(k, "distinct"), bc.klo_of(k)
        start, count = (1 << klo) - 1, 257
        assert (start, count) in bc.tensor_ranges(k)
        want = bc.tensor_range(rhos, start, count)
        assert [tensor_split(rhos, i, klo) for i in range(start, start + count)] == want
        for d in (-1, 1):
            assert [tensor_split(rhos, i, klo + d) for i in range(start, start + count)] != want
    for n, name, cuts in MULTI:
        _, v = bc.values("rm1", n)
        bl = bc.blocks(cuts, n)
        for x in fc.canon([R - 1, bc.RANDOM_M]):
            assert sum((bc.powers_range(x, lo + (1 if lo else 0), nout) for lo, _, nout in bl), []) != pyref.powers(x, n + 1), (n, name)
        if any(lo and nin for lo, nin, _ in bl):
            assert sum((bc.alg_hash_from(v[lo:lo + nin], lo + (1 if lo else 0), ZETA) for lo, nin, _ in bl), []) != pr.alg_hash(v, range(n), ZETA)


def test_teeth_of_the_hash_index():
    """the high limb of the index dropped: it shows from the first index past 2^32 on, with every zeta but 0"""
    _, v = bc.values("edge", 5)
    for first in bc.HASH_FIRSTS:
        for zeta in fc.canon(bc.SCALARS_M):
            want = bc.alg_hash_from(v, first, zeta)
            assert want == pr.alg_hash(v, range(first, first + 5), zeta)
            low = [(e + ((first + i) & 0xFFFFFFFF) * zeta) % R for i, e in enumerate(v)]
            assert (low != want) == (first + 4 >= (1 << 32) and zeta != 0), (first, zeta)
    assert bc.HASH_FIRSTS[2] < (1 << 32) <= bc.HASH_FIRSTS[2] + 4
