// The shape of one step of herring's module space prover (herring.hip: hsp_*), as plain host arithmetic: what the folded streams
// look like after k folds, how the two sides are aligned, how the tensor of the challenges splits into its half tables, and what
// the prover allocates.  No device code and no state, so it is also compiled on its own (tests/cpp/herring_space_plan_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace gm {

// ark_std::log2: the ceiling, log2(0) = log2(1) = 0
inline uint32_t hsp_ceil_log2(size_t n) {
  uint32_t k = 0;
  while (k < 8 * sizeof(size_t) - 1 && ((size_t)1 << k) < n) k++;
  return k;
}
// FoldedPolynomialStream::len (streams.rs:204-206): ceil(n / 2^k)
inline size_t hsp_folded_len(size_t n, uint32_t k) {
  if (k >= 8 * sizeof(size_t) - 1) return n ? 1 : 0;
  const size_t span = (size_t)1 << k;
  return n / span + (n % span ? 1 : 0);
}

struct HspPlan {
  uint32_t k = 0, klo = 0, khi = 0;  // folds so far; the half tables hold 2^klo and 2^khi weights, klo + khi = k
  size_t lp = 0, ls = 0;             // folded lengths of the point side and of the scalar side
  // space_prover.rs:150-184 reads both folded streams from their high ends, skips what the longer one has beyond the shorter and
  // starts either side on a zero "odd" element when its length is odd: pair j is (block 2j, block 2j + 1) of both sides, the
  // missing block of an odd length is zero, and there are as many pairs as the shorter side has
  size_t npairs = 0;
  // final_foldings (:270-276) is the FIRST item of each folded stream, the block of the highest index: its points are the first
  // `top_points` of the big-endian stream (fewer than 2^k when the length is no multiple of 2^k: init_stack's zero padding)
  size_t top_points = 0;
};
inline HspPlan hsp_plan(size_t np, size_t ns, uint32_t k) {
  HspPlan P;
  P.k = k;
  P.klo = (k + 1) / 2;
  P.khi = k - P.klo;
  P.lp = hsp_folded_len(np, k);
  P.ls = hsp_folded_len(ns, k);
  const size_t pp = (P.lp + 1) / 2, ps = (P.ls + 1) / 2;
  P.npairs = pp < ps ? pp : ps;
  P.top_points = P.lp ? np - ((P.lp - 1) << k) : 0;
  return P;
}

// Bytes of the prover's work block: two vectors of np canonical scalars, the two half tables of the deepest round, the challenges
inline size_t hsp_work_bytes(size_t np, uint32_t tot_rounds) {
  const uint32_t klo = (tot_rounds + 1) / 2;
  return 2 * np * 32 + 2 * ((size_t)32 << klo) + ((size_t)tot_rounds + 1) * 32;
}
// the byte offsets of its parts
struct HspWork {
  size_t a, b, lo, hi, ch;
};
inline HspWork hsp_work_layout(size_t np, uint32_t tot_rounds) {
  const uint32_t klo = (tot_rounds + 1) / 2;
  HspWork W;
  W.a = 0;
  W.b = np * 32;
  W.lo = 2 * np * 32;
  W.hi = W.lo + ((size_t)32 << klo);
  W.ch = W.hi + ((size_t)32 << klo);
  return W;
}

// TimeProver::from(&SpaceProver): the point side is folded level by level out of place into two buffers that become the time
// prover's ping and pong.  first holds ceil(np / 2) records (np with no fold to make), second half of that, rounded up; the
// folded vector ends in `first` after an odd number of levels and after none
struct HspTimeBuffers {
  size_t first = 0, second = 0;  // records
  int result_in = 0;             // 0: first, 1: second
};
inline HspTimeBuffers hsp_time_buffers(size_t np, uint32_t k) {
  HspTimeBuffers B;
  B.first = k == 0 ? np : (np + 1) / 2;
  B.second = (B.first + 1) / 2;
  B.result_in = (k == 0 || (k & 1)) ? 0 : 1;
  return B;
}

}  // namespace gm
