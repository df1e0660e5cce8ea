"""The block builders of the sharded prover (include/gemini_hip.h: gm_fr_tensor_range .. gm_fr_add_at): the sizes at which their
kernels change path, the ways a vector is cut into blocks, references in plain Python integers and thin ctypes callers.

Sizes come from gemini_amd/csrc/fr.hip, read with regular expressions, so a retune moves them:
  ACC_K        elements per chunk of the three-phase suffix scan (k_accp_phase1 / 3)
  SEG          chunks per segment (fr_acc_product_ex: `seg`); the carry between segments starts at ACC_K * SEG + 1 elements
  GRID_CAP     blocks a launch is capped at (grid_for); a lane of an element-wise kernel takes a second element from GRID_CAP * LANES on
  POWERS_CAP   the cap k_powers is launched with; `cur = cur * step` is first used from element POWERS_CAP * LANES on

A tiling of the positions 0 .. n (n inputs, n + 1 outputs: the builders of the entry product and plookup append one entry) is a list
of cut points 0 = c_0 < c_1 < ... = n + 1; block j holds the outputs [c_j, c_j+1) and the inputs of those that exist, [c_j, min(c_j+1, n)).

Every block reference is written from the statement in the header comment, not by slicing the whole-vector result: that the two agree
on every tiling is what test_fr_block_cases_cpu.py checks.  The whole-vector references stay oracle/psnark_ref.py and oracle/pyref.py."""
import ctypes as C
import os
import re

import numpy as np

from tests import fr_cases as fc

R = fc.R
LANES = 256


def source_constants() -> dict:
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gemini_amd", "csrc", "fr.hip")).read()
    out = {}
    m = re.search(r"constexpr\s+int\s+ACC_K\s*=\s*(\d+)\s*;", src)
    assert m, "ACC_K not found in fr.hip"
    out["ACC_K"] = int(m.group(1))
    body = src[src.index("int fr_acc_product_ex("):]
    body = body[:body.index("\n}\n")]
    m = re.search(r"\bseg\s*=\s*(\d+)\s*[,;]", body)
    assert m, "seg of fr_acc_product_ex not found in fr.hip"
    out["SEG"] = int(m.group(1))
    m = re.search(r"static\s+unsigned\s+grid_for\(size_t n, unsigned max_blocks = (\d+)\)", src)
    assert m, "the block cap of grid_for not found in fr.hip"
    out["GRID_CAP"] = int(m.group(1))
    for fn in ("fr_powers", "fr_powers_at"):
        body = src[src.index("int %s(" % fn):]
        m = re.search(r"k_powers, dim3\(grid_for\(n, (\d+)\)\), dim3\((\d+)\)", body[:body.index("\n}\n")])
        assert m and int(m.group(2)) == LANES, "the launch of k_powers in %s not found in fr.hip" % fn
        assert out.setdefault("POWERS_CAP", int(m.group(1))) == int(m.group(1))
    # the element-wise block kernels run LANES lanes a block
    for k in ("k_plookup_set_block, dim3(grid_for(nout))", "k_shift_block, dim3(grid_for(nout))", "k_tensor, dim3(grid_for(count))",
              "k_gather_prod2, dim3(grid_for(index->n))", "k_alg_hash, dim3(grid_for(n))"):
        assert k + ", dim3(%d)" % LANES in src, k
    return out


_K = source_constants()
ACC_K, SEG, GRID_CAP, POWERS_CAP = _K["ACC_K"], _K["SEG"], _K["GRID_CAP"], _K["POWERS_CAP"]
SEGN = ACC_K * SEG                      # elements of one segment
SIZES = [1, 2, ACC_K - 1, ACC_K, ACC_K + 1, SEGN - 1, SEGN, SEGN + 1, 2 * SEGN + 1]
LARGE = GRID_CAP * LANES + 1            # lane 0 takes a second element: the element-wise builders only
POWERS_TRIP = POWERS_CAP * LANES        # k_powers: the first element a lane reaches by cur * step
ACC_CUTS = [ACC_K - 1, ACC_K, ACC_K + 1, SEGN - 1, SEGN, SEGN + 1]

TENSOR_KS = (1, 2, 3, 9, 10, 20, 32)
POWERS_STARTS = (0, 1, POWERS_TRIP - 1, (1 << 32) - 2, (1 << 39) - 300)
POWERS_COUNTS = (1, 257, POWERS_TRIP + 1)
HASH_FIRSTS = (0, 1, (1 << 32) - 2, 1 << 40)    # a five-element vector crosses 2^32 from the third
FOLD_LENGTHS = (1, 2, 3, 5, 257, SEGN + 1, 2 * GRID_CAP * LANES + 1)  # the last: GRID_CAP * LANES + 1 outputs at the first level
GATHER_LENGTHS = (1, 255, 256, 257, LARGE)


def klo_of(k: int) -> int:
    """the bits of an index that address the low half table (fr_tensor_range): ceil(k / 2), and k itself for k = 1"""
    return (k + 1) // 2 if k >= 2 else k


def tensor_ranges(k: int):
    """(start, count): starts 0, 1, 2^klo - 1, 2^klo, 2^k - count; counts 1, 257 and, for k >= 20, LARGE -- what fits into 2^k entries.
    At k = 32 short ranges only, the last of them ending at 2^32."""
    out = []
    for count in (1, 257) + ((LARGE,) if 20 <= k < 32 else ()):
        if count > (1 << k):
            continue
        for start in (0, 1, (1 << klo_of(k)) - 1, 1 << klo_of(k), (1 << k) - count):
            if 0 <= start and start + count <= (1 << k) and (start, count) not in out:
                out.append((start, count))
    return out


def gather_indices(k: int, n: int, seed: int = 7) -> dict:
    """name -> n indices below 2^k: all 0, all 2^k - 1, sorted, random, alternating around 2^klo"""
    top, mid = (1 << k) - 1, 1 << klo_of(k)
    rnd = np.random.default_rng(seed + 100 * k + n).integers(0, top + 1, size=n, dtype=np.uint64)
    alt = np.array([mid - 1, mid, mid + 1, mid, mid - 1, 0, mid], dtype=np.uint64)
    alt = np.minimum(alt, np.uint64(top))
    return {"zeros": np.zeros(n, dtype=np.uint32), "top": np.full(n, top, dtype=np.uint32), "sorted": np.sort(rnd).astype(np.uint32),
            "random": rnd.astype(np.uint32), "alternating": alt[np.arange(n) % len(alt)].astype(np.uint32)}


# ---- tilings --------------------------------------------------------------------------------------------------------------------
def tilings(n: int) -> dict:
    """name -> cut points over the n + 1 outputs of n inputs; tilings that coincide are listed once"""
    N = n + 1
    cand = [("one", [0, N])]
    for w in (2, 4):
        # sumcheck_blocks.hpp, Sh: rank r holds [r B, (r + 1) B) of what exists, B a power of two with w B >= the family's length
        B = 1
        while w * B < N:
            B *= 2
        cand.append(("world%d" % w, sorted({min(r * B, N) for r in range(w + 1)})))
    for w in (1, 2, 4):
        if n and n % w == 0:  # w B = n: the block above the last full one holds position n only -- no input, one output
            cand.append(("multiple%d" % w, [r * (n // w) for r in range(w + 1)] + [N]))
    cand.append(("acc", [0] + [c for c in ACC_CUTS if 0 < c < N] + [N]))
    cand.append(("ones", sorted({c for c in (0, 1, 2, 3, n - 2, n - 1, n, N) if 0 <= c <= N})))
    out = {}
    for name, cuts in cand:
        assert cuts[0] == 0 and cuts[-1] == N and all(a < b for a, b in zip(cuts, cuts[1:])), (name, cuts)
        if cuts not in out.values():
            out[name] = cuts
    return out


def blocks(cuts, n):
    """(lo, number of inputs, number of outputs) of every block"""
    return [(a, max(min(b, n) - a, 0), b - a) for a, b in zip(cuts, cuts[1:])]


# ---- block references, from the statements of include/gemini_hip.h ---------------------------------------------------------------
def plookup_set_block(v_block, prev, nout, y, z):
    """out[t] = (1 + z) y + (t >= 1 ? v[t - 1] : prev, nothing at lo = 0) + (t < |v| ? z v[t] : 0), t < nout <= |v| + 1"""
    nv = len(v_block)
    assert nout <= nv + 1
    y1z = (1 + z) * y % R
    out = []
    if nout:
        out.append((y1z + (prev if prev is not None else 0) + (z * v_block[0] if nv else 0)) % R)
    m = min(nout, nv)
    out += [(y1z + a + z * b) % R for a, b in zip(v_block[:m - 1], v_block[1:m])]
    if nout == nv + 1 and nv:
        out.append((y1z + v_block[nv - 1]) % R)
    return out


def shift_block(v_block, first, nout):
    """out[0] = first (1 on the lowest block, else the last element of the block below), out[t] = v[t - 1]"""
    assert nout <= len(v_block) + 1
    return ([first] + list(v_block[:nout - 1])) if nout else []


def product(v):
    acc = 1
    for e in v:
        acc = acc * e % R
    return acc


def acc_product_block(v_block, carry, write_monic):
    """the suffix scan started from `carry` (the product of the blocks above; None: one); write_monic: the entry at |v| -- the carry"""
    state = 1 if carry is None else carry
    out = [state] if write_monic else []
    for e in reversed(v_block):
        state = state * e % R
        out.append(state)
    out.reverse()
    return out


def alg_hash_from(v_block, first_index, zeta):
    """out[i] = v[i] + (first_index + i) zeta"""
    return [(e + (first_index + i) * zeta) % R for i, e in enumerate(v_block)]


def tensor_at(rhos, idx):
    """tensor(rhos)[sum b_j 2^j] = prod rho_j^(b_j)"""
    assert 0 <= idx < (1 << len(rhos))
    acc, j = 1, 0
    while idx:
        if idx & 1:
            acc = acc * rhos[j] % R
        idx >>= 1
        j += 1
    return acc


def tensor_range(rhos, start, count):
    """out[i] = tensor(rhos)[start + i]: the entry with the lowest set bit cleared times that bit's rho -- one product an entry once
    the range has passed the entry it builds on, the bits of the index (tensor_at) before"""
    assert start + count <= (1 << len(rhos))
    out = []
    for idx in range(start, start + count):
        below = idx & (idx - 1)
        if idx and below >= start:
            out.append(out[below - start] * rhos[(idx & -idx).bit_length() - 1] % R)
        else:
            out.append(tensor_at(rhos, idx))
    return out


def powers_range(x, start, count):
    """out[i] = x^(start + i): pow for the first, one product for each of the others, pow again for the last"""
    out = []
    cur = pow(x, start, R)
    for _ in range(count):
        out.append(cur)
        cur = cur * x % R
    assert not count or out[-1] == pow(x, start + count - 1, R)
    return out


def tensor_gather(rhos, index):
    """out[i] = tensor(rhos)[index[i]], computed per index"""
    memo = {}
    return [memo[i] if i in memo else memo.setdefault(i, tensor_at(rhos, i)) for i in index]


def powers_gather(x, index):
    """out[i] = x^index[i], computed per index (0^0 = 1)"""
    memo = {}
    return [memo[i] if i in memo else memo.setdefault(i, pow(x, i, R)) for i in index]


def tensor_gather_bytes(rhos, index):
    """tensor_gather for half a million distinct indices: one table of 256 entries for every byte of the index (its own eight rhos),
    one product a byte.  Not the device's split into two half tables at klo; test_fr_block_cases_cpu.py holds it against tensor_at."""
    tabs = []
    for b in range(0, len(rhos), 8):
        part = rhos[b:b + 8]
        tabs.append([tensor_at(part, v) if v < (1 << len(part)) else None for v in range(256)])
    out = []
    for i in index:
        acc = tabs[0][i & 255]
        for t in tabs[1:]:
            i >>= 8
            if i & 255:
                acc = acc * t[i & 255] % R
        out.append(acc)
    return out


def powers_gather_bytes(x, index, nbytes=4):
    """powers_gather with one table of 256 powers for every byte of the exponent"""
    tabs = [[pow(x, v << (8 * b), R) for v in range(256)] for b in range(nbytes)]
    out = []
    for i in index:
        assert i < (1 << (8 * nbytes))
        acc = tabs[0][i & 255]
        for t in tabs[1:]:
            i >>= 8
            if i & 255:
                acc = acc * t[i & 255] % R
        out.append(acc)
    return out


def fold(f, r):
    """out[i] = f[2i] + r f[2i + 1], the odd tail padded with 0"""
    return [(a + r * b) % R for a, b in zip(f[0::2], list(f[1::2]) + [0] * (len(f) % 2))]


def fold_chain(f, challenges):
    """outs[j] = fold(outs[j - 1], challenge j), outs[-1] = f"""
    outs = []
    for r in challenges:
        f = fold(f, r)
        outs.append(f)
    return outs


def scale_into_many(out, ins, coeffs, offsets):
    """out[offsets[j] + i] = c_j in_j[i], every other element as it was"""
    out = list(out)
    for v, c, off in zip(ins, coeffs, offsets):
        assert off + len(v) <= len(out)
        out[off:off + len(v)] = [c * e % R for e in v]
    return out


def add_at(v, positions, values):
    """v[positions[j]] += values[j], the positions distinct"""
    assert len(set(positions)) == len(positions)
    v = list(v)
    for p, e in zip(positions, values):
        v[p] = (v[p] + e) % R
    return v


# ---- whole vectors from blocks: what the sharded prover hands from block to block ------------------------------------------------
def tiled_plookup_set(v, cuts, y, z):
    n, out = len(v), []
    for lo, nin, nout in blocks(cuts, n):
        out += plookup_set_block(v[lo:lo + nin], v[lo - 1] if lo else None, nout, y, z)
    return out


def tiled_shift(v, cuts):
    n, out = len(v), []
    for lo, nin, nout in blocks(cuts, n):
        out += shift_block(v[lo:lo + nin], v[lo - 1] if lo else 1, nout)
    return out


def carries(prods):
    """carry of block j = the product of the blocks above it"""
    out, acc = [], 1
    for p in reversed(prods):
        out.append(acc)
        acc = acc * p % R
    out.reverse()
    return out


def tiled_acc_product(v, cuts):
    n, out = len(v), []
    bl = blocks(cuts, n)
    cs = carries([product(v[lo:lo + nin]) for lo, nin, _ in bl])
    for (lo, nin, nout), c in zip(bl, cs):
        out += acc_product_block(v[lo:lo + nin], c, nout == nin + 1)
    return out


# ---- values ----------------------------------------------------------------------------------------------------------------------
def random_limbs(seed: int, n: int) -> np.ndarray:
    """seeded elements below 2^254 < r"""
    l = np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    l[:, 3] &= np.uint64((1 << 62) - 1)
    return l


RANDOM_M = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
ONE_M = (1 << 256) % R
# the scalars (y, z, zeta, x, rhos, carries), as limbs: 0, 1, r - 1, EDGE[5], one random element -- and the field's one
SCALARS_M = (0, 1, R - 1, fc.EDGE[5], RANDOM_M, ONE_M)


def _edge_shift() -> int:
    """where the cycle through the edge list starts: element 0 is not 0, and on every tiling of every size some block's halo -- the
    element below its first -- is neither 0 nor one, the two values a dropped halo of plookup_set / the rotation cannot be told from"""
    blind = (fc.EDGE.index(0), fc.EDGE.index(ONE_M))
    for s in range(1, len(fc.EDGE)):
        if all(any((c - 1 + s) % len(fc.EDGE) not in blind for c in cuts[1:-1]) for n in SIZES + [LARGE] for cuts in tilings(n).values() if len(cuts) > 2):
            return s
    raise AssertionError("no start of the edge cycle shows a dropped halo on every tiling")


EDGE_SHIFT = _edge_shift()


def values(kind: str, n: int, nonzero: bool = False):
    """(limbs for the device, field elements for the reference) of one vector: `edge` cycles through the edge list from entry
    EDGE_SHIFT, `rm1` is r - 1 in every slot, `random` is seeded"""
    if kind == "edge":
        src = fc.EDGE_NZ if nonzero else fc.EDGE
        tab_l, tab_c = fc.limbs(src), fc.canon(src)
        idx = (np.arange(n, dtype=np.int64) + EDGE_SHIFT) % len(src)
        return tab_l[idx], [tab_c[i] for i in idx.tolist()]
    if kind == "rm1":
        return np.tile(fc.limbs([R - 1]), (n, 1)), fc.canon([R - 1]) * n
    assert kind == "random"
    l = random_limbs(1000 + n, n)
    return l, fc.canon(fc.ints_of(l))


KINDS = ("edge", "rm1", "random")


# ---- ctypes callers: the raw return code ------------------------------------------------------------------------------------------
def _p(a):
    from gemini_amd import capi

    return capi.ptr(a)


def _u64(a, shape):
    from gemini_amd import capi

    return capi.u64(a).reshape(shape)


def _lib():
    from gemini_amd import capi

    return capi.load()


def _opt4(x):
    return None if x is None else _u64(x, 4)


def gm_fr_tensor_range(rhos_m, k, start, count, out) -> int:
    e = _u64(rhos_m, (-1, 4))
    return _lib().gm_fr_tensor_range(_p(e), C.c_size_t(k), C.c_size_t(start), C.c_size_t(count), C.c_uint64(out.handle))


def gm_fr_powers_range(x_m, start, count, out) -> int:
    x = _u64(x_m, 4)
    return _lib().gm_fr_powers_range(_p(x), C.c_size_t(start), C.c_size_t(count), C.c_uint64(out.handle))


def gm_fr_tensor_gather(rhos_m, k, index, out) -> int:
    e = _u64(rhos_m, (-1, 4))
    return _lib().gm_fr_tensor_gather(_p(e), C.c_size_t(k), C.c_uint64(index.handle), C.c_uint64(out.handle))


def gm_fr_powers_gather(x_m, log_len, index, out) -> int:
    x = _u64(x_m, 4)
    return _lib().gm_fr_powers_gather(_p(x), C.c_size_t(log_len), C.c_uint64(index.handle), C.c_uint64(out.handle))


def gm_fr_alg_hash_from(v, first_index, zeta_m, out) -> int:
    z = _u64(zeta_m, 4)
    return _lib().gm_fr_alg_hash_from(C.c_uint64(v.handle), C.c_size_t(first_index), _p(z), C.c_uint64(out.handle))


def gm_fr_plookup_set_block(v, v_offset, v_count, prev_m, out_count, y_m, z_m, out) -> int:
    prev, y, z = _opt4(prev_m), _u64(y_m, 4), _u64(z_m, 4)
    return _lib().gm_fr_plookup_set_block(C.c_uint64(v.handle), C.c_size_t(v_offset), C.c_size_t(v_count), None if prev is None else _p(prev),
                                          C.c_size_t(out_count), _p(y), _p(z), C.c_uint64(out.handle))


def gm_fr_shift_block(v, first_m, out_count, out) -> int:
    first = _u64(first_m, 4)
    return _lib().gm_fr_shift_block(C.c_uint64(v.handle), _p(first), C.c_size_t(out_count), C.c_uint64(out.handle))


def gm_fr_product(v):
    """(return code, the product's limbs)"""
    total = np.zeros(4, dtype=np.uint64)
    rc = _lib().gm_fr_product(C.c_uint64(v.handle), _p(total))
    return rc, total


def gm_fr_acc_product_block(v, carry_m, write_monic, out) -> int:
    carry = _opt4(carry_m)
    return _lib().gm_fr_acc_product_block(C.c_uint64(v.handle), None if carry is None else _p(carry), C.c_int(int(write_monic)), C.c_uint64(out.handle))


def gm_fr_fold_chain(f, challenges_m, k, outs) -> int:
    ch = _u64(challenges_m, (-1, 4))
    h = np.array([o.handle for o in outs], dtype=np.uint64)
    return _lib().gm_fr_fold_chain(C.c_uint64(f.handle), _p(ch) if len(ch) else None, C.c_size_t(k), _p(h) if len(h) else None)


def gm_fr_scale_into(vin, c_m, out, out_offset) -> int:
    c = _u64(c_m, 4)
    return _lib().gm_fr_scale_into(C.c_uint64(vin.handle), _p(c), C.c_uint64(out.handle), C.c_size_t(out_offset))


def gm_fr_scale_into_many(ins, coeffs_m, out, out_offsets) -> int:
    h = np.array([v.handle for v in ins], dtype=np.uint64)
    c = _u64(coeffs_m, (-1, 4))
    off = np.array(out_offsets, dtype=np.uint64)  # size_t
    assert len(h) == len(c) == len(off)
    return _lib().gm_fr_scale_into_many(_p(h) if len(h) else None, _p(c) if len(h) else None, C.c_size_t(len(h)), C.c_uint64(out.handle),
                                        _p(off) if len(h) else None)


def gm_fr_add_at(v, positions, values_m) -> int:
    pos = np.array(positions, dtype=np.uint64)  # size_t
    val = _u64(values_m, (-1, 4))
    assert len(pos) == len(val)
    return _lib().gm_fr_add_at(C.c_uint64(v.handle), _p(pos) if len(pos) else None, _p(val) if len(pos) else None, C.c_size_t(len(pos)))
