"""GPU: the block builders of the sharded prover (gm_fr_tensor_range .. gm_fr_add_at in include/gemini_hip.h), entry by entry, in one
process, against Python integers bit for bit -- at the sizes where their kernels change path and with the values of tests/fr_cases.py.

Inside whole sharded proofs (test_gpu_dist_native.py) these entries see power-of-two blocks of 128 to 512 uniformly random elements.
Here (tests/fr_block_cases.py reads the constants from fr.hip):
  chunk        ACC_K - 1 | ACC_K | ACC_K + 1 elements: one chunk of the suffix scan, and the first element of the second
  segment      ACC_K SEG - 1 | ACC_K SEG | ACC_K SEG + 1 and 2 ACC_K SEG + 1: the carry between segments (k_accp_phase2a / 3), two of them
  grid stride  GRID_CAP 256 + 1 elements: lane 0 of an element-wise kernel takes a second element; for k_powers POWERS_CAP 256 + 1,
               where cur = cur * step is first used
  2^32         the first index of gm_fr_alg_hash_from (two 32-bit limbs), exponents of gm_fr_powers_range up to 2^39, k = 32 of the tensor
  2^klo        ranges and indices that straddle the step from one entry of the high half table to the next

A vector is cut into blocks by every tiling of fr_block_cases.tilings and each block gets exactly what the sharded prover feeds it
(psnark_sharded.cpp): the halo, the product of the blocks above, write_monic where position n falls into the block.  The concatenation
must equal the block reference, and what the whole-vector builder of gemini_amd.fr returns.

The convention is test_gpu_fr_edges.py's: the device gets the limbs m, the reference computes on m 2^-256 mod r, the expected limbs
are v 2^256 mod r."""
import numpy as np
import pytest

from gemini_amd import fr as F
from oracle import psnark_ref as pr
from oracle import pyref
from tests import fr_block_cases as bc
from tests import fr_cases as fc

pytestmark = pytest.mark.gpu

R = fc.R
GM_EINVAL = -1
SC_M = bc.SCALARS_M                     # limbs given to the device
SC = fc.canon(SC_M)                     # the elements they stand for
ONE_L = fc.limbs([bc.ONE_M])[0]


@pytest.fixture(scope="module")
def gm():
    import gemini_amd

    gemini_amd.capi.init()
    return gemini_amd


def L(m) -> np.ndarray:
    return fc.limbs([m])[0]


def same(a, b) -> bool:
    return a.shape == b.shape and bool((a == b).all())


def free_all(vs):
    for v in vs:
        if v is not None:
            v.free()


class Expect:
    """field elements -> limbs, converted once while the elements stay the same (every tiling has the same whole vector)"""

    def __init__(self):
        self.ints, self.l = None, None

    def __call__(self, ints):
        if ints != self.ints:
            self.ints, self.l = ints, fc.mont_fast(ints).reshape(len(ints), 4)
        return self.l


def run_block(limbs_in, nout, call):
    """upload one block, run call(block, out) into a vector of nout elements, return the output's limbs"""
    vs = []
    try:
        vs.append(F.FrVec.from_host(limbs_in))
        vs.append(F.FrVec.alloc(nout))
        assert call(vs[0], vs[1]) == 0
        assert len(vs[1]) == nout
        return vs[1].to_host()
    finally:
        free_all(vs)


def cat(parts):
    return np.concatenate(parts) if parts else np.empty((0, 4), dtype=np.uint64)


def host_and_free(v):
    try:
        return v.to_host()
    finally:
        v.free()


def scalar_pairs(n):
    """(y, z) as indices into the scalars: every scalar in both places at the small sizes, one pair at the large one"""
    if n >= bc.LARGE:
        return [(3, 4)]
    return [(i, (i + 1) % len(SC)) for i in range(len(SC))] + [(0, 0), (2, 2)]


# ---- plookup_set and the rotation: element-wise, halos ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("n", bc.SIZES + [bc.LARGE])
def test_plookup_set_blocks(gm, n, kind):
    l, v = bc.values(kind, n)
    whole = F.FrVec.from_host(l)
    try:
        for yi, zi in scalar_pairs(n):
            y, z, want = L(SC_M[yi]), L(SC_M[zi]), Expect()
            got_whole = host_and_free(F.plookup_set(whole, y, z))
            assert same(got_whole, want(pr.plookup_set(v, SC[yi], SC[zi]))), (yi, zi)
            for name, cuts in bc.tilings(n).items():
                ref = want(bc.tiled_plookup_set(v, cuts, SC[yi], SC[zi]))
                for form in ("set", "sorted"):
                    parts = []
                    for lo, nin, nout in bc.blocks(cuts, n):
                        halo = 1 if lo else 0
                        if form == "set":  # the block with its halo in front: v_offset = 1, prev = its first element
                            parts.append(run_block(l[lo - halo:lo + nin], nout, lambda b, o: bc.gm_fr_plookup_set_block(
                                b, halo, nin, l[lo - 1] if halo else None, nout, y, z, o)))
                        else:              # the block alone, the halo from the block below
                            parts.append(run_block(l[lo:lo + nin], nout, lambda b, o: bc.gm_fr_plookup_set_block(
                                b, 0, nin, l[lo - 1] if halo else None, nout, y, z, o)))
                    got = cat(parts)
                    assert same(got, ref), (name, form, yi, zi)
                    assert same(got, got_whole), (name, form, yi, zi)
    finally:
        whole.free()


@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("n", bc.SIZES + [bc.LARGE])
def test_shift_blocks(gm, n, kind):
    l, v = bc.values(kind, n)
    want = Expect()
    got_whole = host_and_free(F.shift_monic(l))
    assert same(got_whole, want(pr.right_rotation(pr.monic(v))))
    for name, cuts in bc.tilings(n).items():
        ref = want(bc.tiled_shift(v, cuts))
        got = cat([run_block(l[lo:lo + nin], nout, lambda b, o: bc.gm_fr_shift_block(b, l[lo - 1] if lo else ONE_L, nout, o))
                   for lo, nin, nout in bc.blocks(cuts, n)])
        assert same(got, ref) and same(got, got_whole), name
    # `first` is the caller's: any scalar
    for m in SC_M:
        got = run_block(l[:min(n, 3)], min(n, 3) + 1, lambda b, o: bc.gm_fr_shift_block(b, L(m), min(n, 3) + 1, o))
        assert same(got, fc.mont(bc.shift_block(v[:min(n, 3)], fc.canon([m])[0], min(n, 3) + 1)))


# ---- the product and the accumulated product: chunks, segments, carries --------------------------------------------------------------
def device_products(l, cuts, n):
    """gm_fr_product of every block, as limbs"""
    out = []
    for lo, nin, _ in bc.blocks(cuts, n):
        b = F.FrVec.from_host(l[lo:lo + nin])
        try:
            rc, total = bc.gm_fr_product(b)
            assert rc == 0
            out.append(total)
        finally:
            b.free()
    return out


def tiled_acc_on_device(l, cuts, n, null_top=False):
    """the blocks' accumulated products with the carries made from the blocks' gm_fr_product, as the prover makes them on the host"""
    prods = device_products(l, cuts, n)
    cs = fc.mont(bc.carries(fc.canon(fc.ints_of(np.array(prods)))))
    parts = []
    for (lo, nin, nout), c in zip(bc.blocks(cuts, n), cs):
        carry = None if null_top and lo + nout == n + 1 else c
        parts.append(run_block(l[lo:lo + nin], nout, lambda b, o: bc.gm_fr_acc_product_block(b, carry, nout == nin + 1, o)))
    return prods, cat(parts)


@pytest.mark.parametrize("kind", bc.KINDS + ("edge with 0",))
@pytest.mark.parametrize("n", bc.SIZES)
def test_acc_product_blocks(gm, n, kind):
    l, v = bc.values(kind.split()[0], n, nonzero=(kind != "edge with 0"))
    want = Expect()
    got_whole = host_and_free(F.accumulated_product_monic(l))
    assert same(got_whole, want(pr.accumulated_product(pr.monic(v))))
    for name, cuts in bc.tilings(n).items():
        ref = want(bc.tiled_acc_product(v, cuts))
        for null_top in (False, True):
            prods, got = tiled_acc_on_device(l, cuts, n, null_top)
            assert same(np.array(prods), fc.mont([bc.product(v[lo:lo + nin]) for lo, nin, _ in bc.blocks(cuts, n)])), name
            assert same(got, ref) and same(got, got_whole), (name, null_top)


@pytest.mark.parametrize("n", [0, 1, bc.ACC_K + 1, bc.SEGN + 1])
def test_product_and_carry_scalars(gm, n):
    """gm_fr_product on its own (the empty vector: one), and a block under every carry, with and without the monic entry"""
    for kind in bc.KINDS:
        l, v = bc.values(kind, n, nonzero=True)
        b = F.FrVec.from_host(l)
        try:
            rc, total = bc.gm_fr_product(b)
            assert rc == 0 and same(total, fc.mont([bc.product(v)])[0]), kind
        finally:
            b.free()
        for m, c in zip(SC_M, SC):
            for monic in (0, 1):
                got = run_block(l, n + monic, lambda b, o: bc.gm_fr_acc_product_block(b, L(m), monic, o))
                assert same(got, fc.mont_fast(bc.acc_product_block(v, c, monic)).reshape(n + monic, 4)), (kind, hex(m), monic)


def test_acc_product_single_zero(gm):
    """one 0 at a chunk edge, a segment edge, just below and just above a block cut: everything at or below it is 0, everything above unchanged"""
    n = 2 * bc.SEGN + 1
    cut = bc.SEGN + 10 * bc.ACC_K + 5
    l, v = bc.values("edge", n, nonzero=True)
    base = host_and_free(F.accumulated_product_monic(l))
    assert same(base, fc.mont_fast(pr.accumulated_product(pr.monic(v))))
    for p in (bc.ACC_K - 1, bc.ACC_K, bc.SEGN - 1, bc.SEGN, cut - 1, cut):
        lz = l.copy()
        lz[p] = 0
        want = base.copy()
        want[:p + 1] = 0
        assert same(host_and_free(F.accumulated_product_monic(lz)), want), p
        for cuts in ([0, n + 1], [0, cut, n + 1], bc.tilings(n)["acc"]):
            prods, got = tiled_acc_on_device(lz, cuts, n)
            assert same(got, want), (p, cuts)
            assert [not t.any() for t in prods] == [lo <= p < lo + nin for lo, nin, _ in bc.blocks(cuts, n)], (p, cuts)


# ---- ranges of the tensor and of the powers -----------------------------------------------------------------------------------------
def rhos_m(k: int, pattern: str):
    """k elements as limbs: the scalars in turn (0, 1 and r - 1 among them), or distinct seeded ones"""
    if pattern == "scalars":
        return [SC_M[(j + 2) % len(SC_M)] for j in range(k)]
    return fc.ints_of(bc.random_limbs(40 + k, k))


@pytest.mark.parametrize("k", bc.TENSOR_KS)
def test_tensor_range(gm, k):
    for pattern in ("distinct", "scalars"):
        rm = rhos_m(k, pattern)
        rl, rc_ = fc.limbs(rm), fc.canon(rm)
        for start, count in bc.tensor_ranges(k):
            if count >= bc.LARGE and pattern != "distinct":
                continue
            got = run_block(np.empty((0, 4), dtype=np.uint64), count, lambda b, o: bc.gm_fr_tensor_range(rl, k, start, count, o))
            assert same(got, fc.mont_fast(bc.tensor_range(rc_, start, count)).reshape(count, 4)), (pattern, start, count)
        if k <= 20:  # tiled ranges against the whole tensor of gemini_amd.fr
            whole = host_and_free(F.tensor(rl))
            if k <= 10:
                assert same(whole, fc.mont_fast(pyref.tensor(rc_)))
            for name, cuts in bc.tilings((1 << k) - 1).items():
                got = cat([run_block(np.empty((0, 4), dtype=np.uint64), b - a, lambda _, o: bc.gm_fr_tensor_range(rl, k, a, b - a, o))
                           for a, b in zip(cuts, cuts[1:])])
                assert same(got, whole), (pattern, name)


@pytest.mark.parametrize("count", bc.POWERS_COUNTS)
def test_powers_range(gm, count):
    xs = SC_M if count < bc.POWERS_TRIP else (bc.RANDOM_M, fc.EDGE[5])
    for m in xs:
        x = fc.canon([m])[0]
        for start in bc.POWERS_STARTS:
            got = run_block(np.empty((0, 4), dtype=np.uint64), count, lambda b, o: bc.gm_fr_powers_range(L(m), start, count, o))
            assert same(got, fc.mont_fast(bc.powers_range(x, start, count)).reshape(count, 4)), (hex(m), start)
        whole = host_and_free(F.powers(L(m), count))
        assert same(whole, fc.mont_fast(pyref.powers(x, count)).reshape(count, 4)), hex(m)
        for name, cuts in bc.tilings(count - 1).items():
            got = cat([run_block(np.empty((0, 4), dtype=np.uint64), b - a, lambda _, o: bc.gm_fr_powers_range(L(m), a, b - a, o))
                       for a, b in zip(cuts, cuts[1:])])
            assert same(got, whole), (hex(m), name)


# ---- gathers of the tensor and of the powers ----------------------------------------------------------------------------------------
def expect_gather(per_index, table_of_bytes, idx):
    """limbs of f(index[i]) computed per DISTINCT index (Python's pow / the product over the index's bits; from byte tables where half a
    million indices are distinct)"""
    uniq, inv = np.unique(idx, return_inverse=True)
    vals = (table_of_bytes if len(uniq) > 4096 else per_index)(uniq.tolist())
    return fc.mont_fast(vals).reshape(len(uniq), 4)[inv]


@pytest.mark.parametrize("which", ["tensor", "powers"])
@pytest.mark.parametrize("k", bc.TENSOR_KS)
def test_gathers(gm, k, which):
    for n in bc.GATHER_LENGTHS:
        if which == "tensor":
            params = [rhos_m(k, p) for p in (("distinct",) if n >= bc.LARGE else ("distinct", "scalars"))]
        else:
            params = [bc.RANDOM_M] if n >= bc.LARGE else list(SC_M)  # x = 0 among them: 0^0 = 1
        for name, idx in bc.gather_indices(k, n).items():
            ix = F.IdxVec.from_host(idx)
            try:
                for prm in params:
                    if which == "tensor":
                        rl, rc_ = fc.limbs(prm), fc.canon(prm)
                        got = run_block(np.empty((0, 4), dtype=np.uint64), n, lambda b, o: bc.gm_fr_tensor_gather(rl, k, ix, o))
                        want = expect_gather(lambda u: bc.tensor_gather(rc_, u), lambda u: bc.tensor_gather_bytes(rc_, u), idx)
                    else:
                        x = fc.canon([prm])[0]
                        got = run_block(np.empty((0, 4), dtype=np.uint64), n, lambda b, o: bc.gm_fr_powers_gather(L(prm), k, ix, o))
                        want = expect_gather(lambda u: bc.powers_gather(x, u), lambda u: bc.powers_gather_bytes(x, u), idx)
                    assert same(got, want), (n, name)
            finally:
                ix.free()


# ---- the algebraic hash of a range -----------------------------------------------------------------------------------------------------
def test_alg_hash_from_across_2_32(gm):
    l, v = bc.values("edge", 5)
    for first in bc.HASH_FIRSTS:
        for m, zeta in zip(SC_M, SC):
            got = run_block(l, 5, lambda b, o: bc.gm_fr_alg_hash_from(b, first, L(m), o))
            assert same(got, fc.mont(bc.alg_hash_from(v, first, zeta))), (first, hex(m))


@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("n", bc.SIZES + [bc.LARGE])
def test_alg_hash_blocks(gm, n, kind):
    l, v = bc.values(kind, n)
    for m, zeta in list(zip(SC_M, SC))[4:5] if n >= bc.LARGE else list(zip(SC_M, SC)):
        want = Expect()
        got_whole = host_and_free(F.alg_hash(l, None, L(m)))
        assert same(got_whole, want(pr.alg_hash(v, range(n), zeta))), hex(m)
        for name, cuts in bc.tilings(n).items():
            bl = [b for b in bc.blocks(cuts, n) if b[1]]
            got = cat([run_block(l[lo:lo + nin], nin, lambda b, o: bc.gm_fr_alg_hash_from(b, lo, L(m), o)) for lo, nin, _ in bl])
            assert same(got, want(sum((bc.alg_hash_from(v[lo:lo + nin], lo, zeta) for lo, nin, _ in bl), []))) and same(got, got_whole), (name, hex(m))
        # the whole vector as a range that crosses 2^32 in its second half
        first = (1 << 32) - (n + 1) // 2 - 1
        got = run_block(l, n, lambda b, o: bc.gm_fr_alg_hash_from(b, first, L(m), o))
        assert same(got, fc.mont_fast(bc.alg_hash_from(v, first, zeta)).reshape(n, 4)), hex(m)


# ---- the folding tree in one call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", bc.FOLD_LENGTHS)
def test_fold_chain(gm, n):
    """k = 0 .. two levels past the one that reaches length 1; every level against pyref.fold_polynomial applied again and again and
    against gemini_amd.fr.fold_polynomial level by level.  The references are made once for the longest chain."""
    kmax = pyref.ceil_log2(n) + 2
    ch_m = [SC_M[(j + 1) % len(SC_M)] for j in range(kmax)]
    ch_l, ch = fc.limbs(ch_m), fc.canon(ch_m)
    for kind in (("edge",) if n >= bc.LARGE else bc.KINDS):
        l, v = bc.values(kind, n)
        levels, cur = [], v
        for r in ch:
            cur = pyref.fold_polynomial(cur, r)
            levels.append(cur)
        assert levels == bc.fold_chain(v, ch) and [len(x) for x in ([v] + levels)[-3:]] == [1, 1, 1] and (n == 1 or len(([v] + levels)[-4]) == 2)
        want = [fc.mont_fast(lv).reshape(len(lv), 4) for lv in levels]
        vs = [F.FrVec.from_host(l)]
        try:
            dev = vs[0]
            for j in range(kmax):  # level by level through gm_fr_fold
                dev = F.fold_polynomial(dev, ch_l[j])
                vs.append(dev)
                assert same(dev.to_host(), want[j]), (kind, j)
            for k in range(kmax + 1):
                outs = []
                try:
                    for j in range(k):
                        outs.append(F.FrVec.alloc(len(levels[j])))  # exactly ceil(len / 2^(j + 1))
                    assert bc.gm_fr_fold_chain(vs[0], ch_l[:k], k, outs) == 0
                    for j in range(k):
                        assert len(outs[j]) == len(levels[j]) and same(outs[j].to_host(), want[j]), (kind, k, j)
                finally:
                    free_all(outs)
            assert same(vs[0].to_host(), l)  # the input is as it was
        finally:
            free_all(vs)


# ---- scaled vectors laid out side by side, sparse updates ------------------------------------------------------------------------------
def test_scale_into(gm):
    total = bc.LARGE + 2000
    base_l, base = bc.values("edge", total)
    ins = [bc.values(kind, n) for kind, n in (("edge", 257), ("rm1", 1), ("random", 0), ("edge", bc.LARGE), ("random", 300))]
    coeff = [1, 2, 3, 4, 0]  # indices into the scalars
    layouts = {"adjacent, to the end": [total - bc.LARGE - 558, total - bc.LARGE - 301, total - bc.LARGE - 300, total - bc.LARGE, total - bc.LARGE - 300],
               "gaps": [5, 300, 300, 1000, bc.LARGE + 1500]}
    vs = []
    try:
        vs = [F.FrVec.from_host(l) for l, _ in ins]
        for name, offs in layouts.items():
            want = fc.mont_fast(bc.scale_into_many(base, [v for _, v in ins], [SC[i] for i in coeff], offs))
            for many in (True, False):
                out = F.FrVec.from_host(base_l)
                try:
                    if many:
                        assert bc.gm_fr_scale_into_many(vs, fc.limbs([SC_M[i] for i in coeff]), out, offs) == 0
                    else:
                        for v, i, off in zip(vs, coeff, offs):
                            assert bc.gm_fr_scale_into(v, L(SC_M[i]), out, off) == 0
                    assert len(out) == total and same(out.to_host(), want), (name, many)
                finally:
                    out.free()
        out = F.FrVec.from_host(base_l[:3])
        try:  # no vector at all, and an empty one at the very end
            assert bc.gm_fr_scale_into_many([], np.empty((0, 4), dtype=np.uint64), out, []) == 0
            assert bc.gm_fr_scale_into(vs[2], L(SC_M[2]), out, 3) == 0
            assert same(out.to_host(), base_l[:3])
        finally:
            out.free()
    finally:
        free_all(vs)


@pytest.mark.parametrize("k", [1, 64, 65, 4096])
def test_add_at(gm, k):
    """distinct positions, 0 and len - 1 among them; (r - 1) + (r - 1) and (r - 1) + 1 in limbs: with and without the subtraction of r"""
    n = 2 * k + 1
    pos = [n - 1, 0][:k] + (np.random.default_rng(k).permutation(np.arange(1, n - 1))[:max(k - 2, 0)]).tolist()
    assert len(pos) == k == len(set(pos))
    vals = [(R - 1, 1)[j % 2] for j in range(k)]
    v = F.FrVec.from_host(np.tile(L(R - 1), (n, 1)))
    try:
        assert bc.gm_fr_add_at(v, pos, fc.limbs(vals)) == 0
        # limbs add like the elements they stand for
        assert same(v.to_host(), fc.limbs(bc.add_at([R - 1] * n, pos, vals)))
        assert same(v.to_host(), fc.mont(bc.add_at(fc.canon([R - 1] * n), pos, fc.canon(vals))))
    finally:
        v.free()


# ---- the whole-vector builders at the edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["edge", "rm1"])
@pytest.mark.parametrize("n", bc.SIZES + [bc.LARGE])
def test_whole_builders_on_edge_values(gm, n, kind):
    """alg_hash (over the range and over an index vector), plookup_subset and lookup here; plookup_set, shift_monic and
    accumulated_product_monic on the same vectors in test_plookup_set_blocks, test_shift_blocks and test_acc_product_blocks (the scan
    up to 2 ACC_K SEG + 1 elements, the element-wise ones up to GRID_CAP 256 + 1)"""
    l, v = bc.values(kind, n)
    words = np.array([0, 1, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0xFFFF0000, 0x0000FFFF, 2], dtype=np.uint32)
    hidx = words[(np.arange(n) * 3 + n) % len(words)]                     # 32-bit edge words for the hash
    gidx = np.array([0, n - 1, n // 2, n - 1, 0], dtype=np.uint32)[np.arange(n + 3) % 5]  # positions in v for the lookup, longer than v
    vs = []
    try:
        whole, hi, gi = F.FrVec.from_host(l), F.IdxVec.from_host(hidx), F.IdxVec.from_host(gidx)
        vs += [whole, hi, gi]
        for j in ((4,) if n >= bc.LARGE else range(len(SC))):
            m, c = L(SC_M[j]), SC[j]
            assert same(host_and_free(F.alg_hash(whole, hi, m)), fc.mont_fast(pr.alg_hash(v, hidx.tolist(), c)).reshape(n, 4)), j
            assert same(host_and_free(F.plookup_subset(whole, m)), fc.mont_fast(pr.plookup_subset(v, c)).reshape(n, 4)), j
        assert same(host_and_free(F.lookup(whole, gi)), l[gidx.astype(np.int64)])
        assert same(host_and_free(F.lookup(whole, gi)), fc.mont_fast(pr.lookup(v, gidx.tolist())))
    finally:
        free_all(vs)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(gm):
    """every refused call returns GM_EINVAL and is followed by a good call on the same context whose result is checked"""
    l, v = bc.values("edge", 8)
    rm = rhos_m(33, "distinct")
    rl, rc_ = fc.limbs(rm), fc.canon(rm)
    x_m = bc.RANDOM_M
    x = fc.canon([x_m])[0]
    vs = []
    try:
        src, out, big = F.FrVec.from_host(l), F.FrVec.alloc(16), F.FrVec.alloc(16)
        vs += [src, out, big]

        def good():
            assert bc.gm_fr_tensor_range(rl, 3, 2, 5, out) == 0 and same(out.to_host(), fc.mont(bc.tensor_range(rc_[:3], 2, 5)))
            assert bc.gm_fr_shift_block(src, ONE_L, 9, out) == 0 and same(out.to_host(), fc.mont(bc.shift_block(v, 1, 9)))
            assert same(src.to_host(), l)

        # tensor_range: k = 0, k = 33, start + count > 2^k
        for k, start, count in ((0, 0, 1), (33, 0, 1), (3, 4, 5), (3, 9, 0)):
            assert bc.gm_fr_tensor_range(rl, k, start, count, out) == GM_EINVAL, (k, start, count)
            good()
        # powers_range: start = 2^39
        assert bc.gm_fr_powers_range(L(x_m), 1 << 39, 1, out) == GM_EINVAL
        assert bc.gm_fr_powers_range(L(x_m), (1 << 39) - 1, 2, out) == 0 and same(out.to_host(), fc.mont(bc.powers_range(x, (1 << 39) - 1, 2)))
        # a gather with an index equal to 2^k
        ix = F.IdxVec.from_host(np.array([0, 8, 7], dtype=np.uint32))
        vs.append(ix)
        assert bc.gm_fr_tensor_gather(rl, 3, ix, out) == GM_EINVAL and bc.gm_fr_powers_gather(L(x_m), 3, ix, out) == GM_EINVAL
        assert bc.gm_fr_tensor_gather(rl, 4, ix, out) == 0 and same(out.to_host(), fc.mont(bc.tensor_gather(rc_[:4], [0, 8, 7])))
        assert bc.gm_fr_powers_gather(L(x_m), 4, ix, out) == 0 and same(out.to_host(), fc.mont(bc.powers_gather(x, [0, 8, 7])))
        # plookup_set_block: nout = nv + 2, v_offset + v_count > len, out = v
        y, z = L(SC_M[3]), L(SC_M[4])
        for off, nv, nout, o in ((0, 8, 10, out), (1, 8, 8, out), (9, 0, 0, out), (0, 8, 8, src)):
            assert bc.gm_fr_plookup_set_block(src, off, nv, None, nout, y, z, o) == GM_EINVAL, (off, nv, nout)
            good()
        assert bc.gm_fr_plookup_set_block(src, 1, 7, l[0], 8, y, z, out) == 0
        assert same(out.to_host(), fc.mont(bc.plookup_set_block(v[1:], v[0], 8, SC[3], SC[4])))
        # shift_block: nout = len + 2
        assert bc.gm_fr_shift_block(src, ONE_L, 10, out) == GM_EINVAL
        good()
        # acc_product_block: out = v (with and without room for the monic entry)
        for monic in (0, 1):
            assert bc.gm_fr_acc_product_block(src, None, monic, src) == GM_EINVAL
        assert bc.gm_fr_acc_product_block(src, None, 1, out) == 0 and same(out.to_host(), fc.mont(bc.acc_product_block(v, None, True)))
        assert same(src.to_host(), l)
        # add_at: k = 4097, a repeated position, a position equal to len
        far = F.FrVec.from_host(np.tile(L(R - 1), (5000, 1)))
        vs.append(far)
        assert bc.gm_fr_add_at(far, list(range(4097)), np.tile(L(1), (4097, 1))) == GM_EINVAL
        assert bc.gm_fr_add_at(far, [3, 7, 3], np.tile(L(1), (3, 1))) == GM_EINVAL
        assert bc.gm_fr_add_at(far, [3, 5000], np.tile(L(1), (2, 1))) == GM_EINVAL
        assert same(far.to_host(), np.tile(L(R - 1), (5000, 1)))  # nothing was added
        assert bc.gm_fr_add_at(far, [4999], L(1).reshape(1, 4)) == 0
        assert same(far.to_host(), fc.limbs([R - 1] * 4999 + [0]))
        # scale_into: past the end, out as its own input
        assert bc.gm_fr_scale_into(src, y, big, 9) == GM_EINVAL
        assert bc.gm_fr_scale_into(src, y, src, 0) == GM_EINVAL
        assert bc.gm_fr_scale_into_many([src, big], np.array([y, y]), big, [0, 0]) == GM_EINVAL
        big.fill(L(0))
        assert bc.gm_fr_scale_into(src, y, big, 8) == 0
        assert same(big.to_host(), fc.mont([0] * 8 + [SC[3] * e % R for e in v]))
        assert same(src.to_host(), l)
        # fold_chain: a repeated output, an output equal to f, a capacity one too small (at the first and at the last level)
        a, b, c, small = F.FrVec.alloc(4), F.FrVec.alloc(2), F.FrVec.alloc(1), F.FrVec.alloc(3)
        vs += [a, b, c, small]
        ch = fc.limbs([SC_M[3], SC_M[4], SC_M[2]])
        assert bc.gm_fr_fold_chain(src, ch, 3, [a, b, a]) == GM_EINVAL
        assert bc.gm_fr_fold_chain(src, ch, 3, [a, src, c]) == GM_EINVAL
        assert bc.gm_fr_fold_chain(src, ch, 1, [src]) == GM_EINVAL
        assert bc.gm_fr_fold_chain(src, ch, 3, [small, b, c]) == GM_EINVAL
        assert bc.gm_fr_fold_chain(src, ch, 3, [a, c, b]) == GM_EINVAL   # level 1 needs 2 elements, c holds 1
        assert same(src.to_host(), l)
        assert bc.gm_fr_fold_chain(src, ch, 3, [a, b, c]) == 0
        for o, lv in zip((a, b, c), bc.fold_chain(v, fc.canon([SC_M[3], SC_M[4], SC_M[2]]))):
            assert same(o.to_host(), fc.mont(lv))
    finally:
        free_all(vs)
