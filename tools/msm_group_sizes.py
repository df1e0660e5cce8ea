"""CPU check behind k_sort2_group (gemini_amd/csrc/msm.hip): how many entries does each coarse group of the block sort hold for
the scalars bench.py times?  One block stages a whole group in LDS only if the group has at most MSM_SORT_GROUP_CAP_MAX = 37 872
entries (ctx.hpp); a larger group takes the chunked branch.

A plain call of n pairs at window c = 16 has W = 16 windows of 2^15 buckets; the sort's coarse bin of an entry is
(window, bucket >> 10): G = 512 groups of 1024 buckets.  The digits are the signed ones of DigitIter (msm.hip): d in [-2^15, 2^15),
the carry of the last window folded back in.

    python tools/msm_group_sizes.py [--logn 20]          # no GPU needed

prints, for each of the two seeded scalar sets of bench.py, the largest group, the largest group outside the top window, the
number of non-empty groups of the top window and how many groups exceed the capacity (profiles/msm_group_sort.md quotes it), and
the largest BUCKET against L + 2, L the chunk length of k_acc0: a bucket of at least L + 2 entries can span three lanes, which
the boundary pass of the optimistic one-call path (k_boundary) hands back to the merge levels (profiles/msm_optimistic_tail.md)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C_WINDOW, FB, CAP_MAX = 16, 10, (160 * 1024 - 3 * 1024 * 4 - 64) // 4


def coarse_group_sizes(scalars: np.ndarray, c: int = C_WINDOW, fb: int = FB) -> np.ndarray:
    """entries per coarse group of the block sort, scalars (n, 4) little-endian u64 canonical; c must divide 64"""
    assert 64 % c == 0 and fb <= c - 1
    sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    per = 64 // c
    W = 4 * per
    gpw = 1 << (c - 1 - fb)  # groups per window
    sizes = np.zeros(W * gpw, dtype=np.int64)
    carry = np.zeros(len(sc), dtype=np.int64)
    for w in range(W):
        raw = ((sc[:, w // per] >> np.uint64(c * (w % per))) & np.uint64((1 << c) - 1)).astype(np.int64)
        d = raw + carry
        if w < W - 1:
            carry = (d + (1 << (c - 1))) >> c
            d = d - (carry << c)
        mag = np.abs(d)
        live = mag != 0
        sizes[w * gpw:(w + 1) * gpw] = np.bincount((mag[live] - 1) >> fb, minlength=gpw)[:gpw]
    return sizes


def chunk_length(n: int, W: int = 16) -> int:
    """msm_enqueue's chunk length L of k_acc0 for a plain call of n pairs"""
    N = n * W
    lanes = 262144 if N >= 1 << 24 else 131072
    return (min(256, max(4, -(-N // lanes))) + 1) & ~1


def main():
    import bench

    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=20)
    args = ap.parse_args()
    n = 1 << args.logn
    rng = np.random.default_rng(0x47454D494E49)  # rank 0 of bench.py
    bench.uniform_fr(rng, n)  # the base scalars come first
    gpw = 1 << (C_WINDOW - 1 - FB)
    print(f"n = 2^{args.logn}, c = {C_WINDOW}, FB = {FB}: {16 * gpw} coarse groups, capacity of one block {CAP_MAX} entries")
    print("| scalar set | entries | largest group | largest outside the top window | non-empty groups of the top window | groups over the capacity |")
    print("|---|---:|---:|---:|---:|---:|")
    largest = []
    for k in range(2):
        sc = bench.uniform_fr(rng, n)
        s = coarse_group_sizes(sc)
        top = s[-gpw:]
        print(f"| {k} | {s.sum()} | {s.max()} | {s[:-gpw].max()} | {(top > 0).sum()} | {(s > CAP_MAX).sum()} |")
        largest.append(int(coarse_group_sizes(sc, fb=0).max()))  # FB = 0: one group per bucket
    L = chunk_length(n)
    for k, b in enumerate(largest):
        print(f"scalar set {k}: largest bucket {b} entries against L + 2 = {L + 2} (L = {L}): "
              + ("no bucket spans three lanes" if b < L + 2 else "a bucket may span three lanes"))


if __name__ == "__main__":
    main()
