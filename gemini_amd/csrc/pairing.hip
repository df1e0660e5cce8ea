// The BLS12-381 pairing on the device: multi-Miller loop and GT product reduction (gfx950); the herring PModule prover of herring.hip calls them.
//
// Replaces `P::multi_pairing` as PModule::ip calls it (src/herring/module.rs:60-79: G1 x G2 -> GT), i.e. the messages of
// TimeProver<PModule> (src/herring/time_prover.rs:91-123, two such provers per round of InnerProductProof::new,
// src/herring/ipa.rs:533-685) and the 4 log d multi-pairings of Vrs::from (ipa.rs:215-247).  The value is the reduced ate pairing
// as ark-ec 0.4.2 states it for BLS12 (models/bls12/mod.rs): Miller loop over |x| = 0xd201000000010000, conjugation (x < 0),
// f^((q^12 - 1) / r); a pair with a point at infinity contributes 1.
//
//   1. k_miller      one lane per pair, each with its own accumulator f.  T walks the twist in homogeneous projective
//                    coordinates (no inversion in the loop; the formulas of Costello-Lange-Naehrig as ark-ec's g2.rs writes them,
//                    scaled by 4 to drop its constant 1/2), the line is (l0, l1 x_P, l4 y_P) at 1, v, v w and enters f through
//                    the sparse product of gt.cuh.  Lines differ from the affine chord-and-tangent lines by factors in Fq2,
//                    which the final exponentiation removes.  The wave multiplies its 64 accumulators in LDS and writes ONE
//                    partial product (576 bytes) per block.
//   2. k_gt_reduce   64 partials -> 1 per block, repeated while more than GT_HOST_MAX remain
//   3. host          the last <= GT_HOST_MAX partials, the conjugation, the final exponentiation (host_field.hpp)
//
// The SEGMENTED form (k_miller_seg, k_gt_reduce_seg; miller_products) computes S independent products in one launch per level: the
// rounds of InnerProductProof::new ask 2 j + 2 PModule provers for a message each, all over vectors of the same short length
// (ipa.hip), and Vrs::from asks for 4 (log2 len - 1) products.  Lanes map to (segment, pair) through a table of segment starts,
// the per-lane loop is k_miller's, the block product multiplies only neighbours of the same segment and every segment that
// touches a block writes one partial.  Partials of a segment are consecutive, so the next level is the same reduction over a
// table of its own; the launch count depends on the longest segment only, never on S.
//
// Registers and LDS: f is 144 VGPRs, T 72, a line 36, and an Fq6 product keeps ~10 Fq2 alive: too much for the 512 registers of
// a lane at one wave per SIMD if f stayed resident.  f therefore lives in LDS ([coefficient limb][lane], 576 B per lane, 36 KiB per
// wave: four waves per CU, one per SIMD) and is in registers only from the load in front of f^2 to the store behind f * line;
// the point arithmetic runs while it is parked.  What the compiler still spills is in profiles/pairing_kernel_resources.txt.
// The squaring of f is NOT shared between the pairs of a product (the classic multi-Miller saving of about a third): lanes stay
// independent, and a product of n pairs is one wave-latency deep up to 2^16 pairs.
//
// Launches go on the library's stream under the MSM lock: the prover's folds stage their scalars in the MSM workspace
// (C->msm.misc) and the partial buffers (C->pairing) are single-flight like it.
#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "gt.cuh"
#include "host_field.hpp"

namespace gm {

constexpr int PAIR_BLOCK = 64;          // pairs per block of k_miller = partials per block of k_gt_reduce: one wave
constexpr size_t GT_HOST_MAX = 4;       // partials the host multiplies itself
constexpr int G1_AFF_BYTES = 96;
constexpr int GT_WORDS = 12 * Fq::N;
constexpr uint64_t ATE_LOOP = 0xd201000000010000ull;

// ---- f in LDS: limb j of lane l at sh[j * PAIR_BLOCK + l] (conflict-free: a wave reads 64 consecutive words) ----------------
GM_DEV void gt_lds_store(uint32_t* sh, int lane, const Fq12& a) {
  const FqE* e = reinterpret_cast<const FqE*>(&a);  // 12 FqE back to back, tower order
#pragma unroll
  for (int k = 0; k < 12; k++) {
#pragma unroll
    for (int i = 0; i < Fq::N; i++) sh[(k * Fq::N + i) * PAIR_BLOCK + lane] = e[k].l[i];
  }
}
GM_DEV Fq12 gt_lds_load(const uint32_t* sh, int lane) {
  Fq12 a;
  FqE* e = reinterpret_cast<FqE*>(&a);
#pragma unroll
  for (int k = 0; k < 12; k++) {
#pragma unroll
    for (int i = 0; i < Fq::N; i++) e[k].l[i] = sh[(k * Fq::N + i) * PAIR_BLOCK + lane];
  }
  return a;
}
// the product of the block's 64 accumulators ends in lane 0's column: 6 levels, one Fq12 product deep each
GM_DEV void gt_block_product(uint32_t* sh, int lane) {
  for (int s = PAIR_BLOCK / 2; s >= 1; s >>= 1) {
    __syncthreads();
    if (lane < s) gt_lds_store(sh, lane, fq12_mul(gt_lds_load(sh, lane), gt_lds_load(sh, lane + s)));
  }
  __syncthreads();
}

// ---- the point of the twist, homogeneous projective (x = X / Z, y = Y / Z) -----------------------------------------------
struct G2Proj {
  Fq2 x, y, z;
};
struct Line {
  Fq2 l0, l1, l4;
};
// T <- 2 T and the tangent at T evaluated at P: (3 b' Z^2 - Y^2, 3 X^2 x_P, -2 Y Z y_P), b' = 4 xi.  3 M + 6 S + 4 Fq products.
GM_DEV Line miller_dbl_step(G2Proj& T, const G1Affine& P) {
  const Fq2 a = fq2_mul(T.x, T.y);                                     // X Y
  const Fq2 b = fq2_sqr(T.y);
  const Fq2 c = fq2_sqr(T.z);
  const Fq2 e = fq2_mul12(fq2_mul_xi(c));                              // 3 b' Z^2 = 12 xi Z^2
  const Fq2 f = fq2_add(fq2_dbl(e), e);                                // 9 b' Z^2
  const Fq2 g = fq2_add(b, f);                                         // Y^2 + 9 b' Z^2
  const Fq2 h = fq2_sub(fq2_sub(fq2_sqr(fq2_add(T.y, T.z)), b), c);    // 2 Y Z
  const Fq2 j = fq2_sqr(T.x);
  Line l;
  l.l0 = fq2_sub(e, b);
  l.l1 = fq2_mul_fq(fq2_add(fq2_dbl(j), j), P.x);
  l.l4 = fq2_mul_fq(fq2_neg(h), P.y);
  T.x = fq2_dbl(fq2_mul(a, fq2_sub(b, f)));                            // 2 X Y (Y^2 - 9 b' Z^2)
  T.y = fq2_sub(fq2_sqr(g), fq2_mul12(fq2_sqr(e)));                    // (Y^2 + 9 b' Z^2)^2 - 12 (3 b' Z^2)^2
  T.z = fq2_dbl(fq2_dbl(fq2_mul(b, h)));                               // 4 Y^2 (2 Y Z)
  return l;
}
// T <- T + Q (Q affine, T != +-Q: T is a multiple k Q with 1 < k < r) and the chord evaluated at P:
// (theta x_Q - lambda y_Q, -theta x_P, lambda y_P).  11 M + 2 S + 4 Fq products.
GM_DEV Line miller_add_step(G2Proj& T, const G2Affine& Q, const G1Affine& P) {
  const Fq2 theta = fq2_sub(T.y, fq2_mul(Q.y, T.z));
  const Fq2 lambda = fq2_sub(T.x, fq2_mul(Q.x, T.z));
  const Fq2 c = fq2_sqr(theta);
  const Fq2 d = fq2_sqr(lambda);
  const Fq2 e = fq2_mul(lambda, d);
  const Fq2 f = fq2_mul(T.z, c);
  const Fq2 g = fq2_mul(T.x, d);
  const Fq2 h = fq2_sub(fq2_add(e, f), fq2_dbl(g));
  Line l;
  l.l0 = fq2_sub(fq2_mul(theta, Q.x), fq2_mul(lambda, Q.y));
  l.l1 = fq2_mul_fq(fq2_neg(theta), P.x);
  l.l4 = fq2_mul_fq(lambda, P.y);
  T.y = fq2_sub(fq2_mul(theta, fq2_sub(g, h)), fq2_mul(e, T.y));
  T.x = fq2_mul(lambda, h);
  T.z = fq2_mul(T.z, e);
  return l;
}

// The loop of one lane: f_{|x|, Q}(P) into the lane's column of sh (1 when the pair is not live).  Shared by k_miller and k_miller_seg.
GM_DEV void miller_lane(uint32_t* sh, int lane, bool live, const G1Affine& P, const G2Affine& Q) {
  gt_lds_store(sh, lane, fq12_one());
  if (live) {
    G2Proj T;
    T.x = Q.x;
    T.y = Q.y;
    T.z = fq2_one();
    // the loop bits are those of a constant: the branch below is the same for every lane of every wave (a scalar branch),
    // and the body is stated once -- unrolling 63 steps of ~100 out-of-line Fq products each buys nothing
#pragma unroll 1
    for (int bit = 62; bit >= 0; bit--) {
      Line l = miller_dbl_step(T, P);
      Fq12 f = fq12_mul_014(fq12_sqr(gt_lds_load(sh, lane)), l.l0, l.l1, l.l4);
      if ((ATE_LOOP >> bit) & 1ull) {
        gt_lds_store(sh, lane, f);
        l = miller_add_step(T, Q, P);
        f = fq12_mul_014(gt_lds_load(sh, lane), l.l0, l.l1, l.l4);
      }
      gt_lds_store(sh, lane, f);
    }
  }
}

// Two ranges of pairs per launch (the second may be empty): pair i < n0 is (g1[first1 + step1 i], g2[first2 + step2 i]) of
// range 0, the others of range 1 -- the b message of the PModule prover is ONE product over (f_e, g_o) and (f_o, g_e).
struct PairRange {
  const uint8_t* g1;
  const uint8_t* g2;
  long long first1, step1, first2, step2;
  unsigned long long n;
};

// Fq products of the loop as written: 63 x (36 square + 39 line + 25 doubling) + 5 x (39 line + 41 addition) = 6700 per pair,
// + 6 x 54 for the block product (profiles/pairing.md).
__global__ __launch_bounds__(PAIR_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_miller(PairRange r0, PairRange r1, uint8_t* __restrict__ partials) {
  __shared__ uint32_t sh[GT_WORDS * PAIR_BLOCK];
  const int lane = threadIdx.x;
  const unsigned long long i = (unsigned long long)blockIdx.x * PAIR_BLOCK + lane;
  G1Affine P;
  G2Affine Q;
  bool live = false;
  if (i < r0.n + r1.n) {
    const bool second = i >= r0.n;
    const long long k = (long long)(second ? i - r0.n : i);
    const long long i1 = second ? r1.first1 + r1.step1 * k : r0.first1 + r0.step1 * k;
    const long long i2 = second ? r1.first2 + r1.step2 * k : r0.first2 + r0.step2 * k;
    P = g1_load_affine((second ? r1.g1 : r0.g1) + (size_t)i1 * G1_AFF_BYTES);
    Q = g2_load_affine((second ? r1.g2 : r0.g2) + (size_t)i2 * G2_AFF_BYTES);
    live = !(P.is_identity() || Q.is_identity());  // a point at infinity never enters the product
  }
  miller_lane(sh, lane, live, P, Q);
  gt_block_product(sh, lane);
  if (lane == 0) fq12_store(partials + (size_t)blockIdx.x * GT_BYTES, gt_lds_load(sh, 0));
}

// out[b] = prod of in[64 b .. 64 b + 63] (as far as m reaches)
__global__ __launch_bounds__(PAIR_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_gt_reduce(const uint8_t* __restrict__ in, size_t m, uint8_t* __restrict__ out) {
  __shared__ uint32_t sh[GT_WORDS * PAIR_BLOCK];
  const int lane = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * PAIR_BLOCK + lane;
  gt_lds_store(sh, lane, i < m ? fq12_load(in + i * GT_BYTES) : fq12_one());
  gt_block_product(sh, lane);
  if (lane == 0) fq12_store(out + (size_t)blockIdx.x * GT_BYTES, gt_lds_load(sh, 0));
}

// ---- the segmented form: S independent products per launch ------------------------------------------------------------------
// Segment s owns the lanes [start, start + count) of a level and writes its partials from index `out` on, one per block it touches.
// The host (seg_levels) lays the segments out so that one of at most PAIR_BLOCK lanes never crosses a block; lanes between two
// segments belong to none.
struct SegMap {
  unsigned long long start, count, out;
};
struct PairSeg {
  PairRange r0, r1;
};
constexpr uint32_t NO_SEG = 0xffffffffu;

// the segment of lane i, NO_SEG between segments: the last entry that starts at or below i (starts ascend)
GM_DEV uint32_t seg_find(const SegMap* __restrict__ map, unsigned nseg, unsigned long long i) {
  if (i < map[0].start) return NO_SEG;
  unsigned lo = 0, hi = nseg;  // map[lo].start <= i < map[hi].start (map[nseg]: past the end)
  while (hi - lo > 1) {
    const unsigned mid = (lo + hi) >> 1;
    if (map[mid].start <= i) lo = mid;
    else hi = mid;
  }
  return i - map[lo].start < map[lo].count ? lo : NO_SEG;
}

// The block's accumulators multiplied segment by segment: after the step of stride s a lane holds the product of the lanes
// [lane, lane + 2 s) of its segment, so the first lane of every segment ends with all of it -- at most 6 levels, fewer when the
// segments are short (the loop ends with the first stride no lane can use).  That lane writes the segment's partial of this block.
GM_DEV void gt_block_product_seg(uint32_t* sh, uint32_t* seg, int lane, uint32_t sid, const SegMap* __restrict__ map, uint8_t* __restrict__ out) {
  seg[lane] = sid;
  __syncthreads();
  for (int s = 1; s < PAIR_BLOCK; s <<= 1) {
    const bool take = sid != NO_SEG && lane + s < PAIR_BLOCK && seg[lane + s] == sid;
    if (!__syncthreads_or(take)) break;
    Fq12 p;
    if (take) p = fq12_mul(gt_lds_load(sh, lane), gt_lds_load(sh, lane + s));
    __syncthreads();
    if (take) gt_lds_store(sh, lane, p);
  }
  __syncthreads();
  if (sid != NO_SEG && (lane == 0 || seg[lane - 1] != sid))
    fq12_store(out + (size_t)(map[sid].out + (blockIdx.x - map[sid].start / PAIR_BLOCK)) * GT_BYTES, gt_lds_load(sh, lane));
}

// k_miller over a table of products: lane -> (segment, pair), the loop of miller_lane, one partial per (block, segment)
__global__ __launch_bounds__(PAIR_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_miller_seg(const PairSeg* __restrict__ spans, const SegMap* __restrict__ map, unsigned nseg,
                                                                                                         uint8_t* __restrict__ partials) {
  __shared__ uint32_t sh[GT_WORDS * PAIR_BLOCK];
  __shared__ uint32_t seg[PAIR_BLOCK];
  const int lane = threadIdx.x;
  const unsigned long long i = (unsigned long long)blockIdx.x * PAIR_BLOCK + lane;
  const uint32_t sid = seg_find(map, nseg, i);
  G1Affine P;
  G2Affine Q;
  bool live = false;
  if (sid != NO_SEG) {
    const unsigned long long k0 = i - map[sid].start;
    const bool second = k0 >= spans[sid].r0.n;
    const PairRange r = second ? spans[sid].r1 : spans[sid].r0;
    const long long k = (long long)(second ? k0 - spans[sid].r0.n : k0);
    P = g1_load_affine(r.g1 + (size_t)(r.first1 + r.step1 * k) * G1_AFF_BYTES);
    Q = g2_load_affine(r.g2 + (size_t)(r.first2 + r.step2 * k) * G2_AFF_BYTES);
    live = !(P.is_identity() || Q.is_identity());
  }
  miller_lane(sh, lane, live, P, Q);
  gt_block_product_seg(sh, seg, lane, sid, map, partials);
}

// one level of the reduction behind it: lane i holds partial i of the level below
__global__ __launch_bounds__(PAIR_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_gt_reduce_seg(const uint8_t* __restrict__ in, const SegMap* __restrict__ map, unsigned nseg,
                                                                                                            uint8_t* __restrict__ out) {
  __shared__ uint32_t sh[GT_WORDS * PAIR_BLOCK];
  __shared__ uint32_t seg[PAIR_BLOCK];
  const int lane = threadIdx.x;
  const unsigned long long i = (unsigned long long)blockIdx.x * PAIR_BLOCK + lane;
  const uint32_t sid = seg_find(map, nseg, i);
  gt_lds_store(sh, lane, sid != NO_SEG ? fq12_load(in + (size_t)i * GT_BYTES) : fq12_one());
  gt_block_product_seg(sh, seg, lane, sid, map, out);
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
void pairing_workspace_release(PairingWorkspace& w) {
  for (DevBuf& b : w.part) b.release();
  if (w.host_out) (void)hipHostFree(w.host_out);
  w.host_out = nullptr;
  w.seg_tab.release();
  if (w.host_seg) (void)hipHostFree(w.host_seg);
  w.host_seg = nullptr;
  w.host_seg_cap = 0;
}

// The Miller product of both spans (PairSpan: ctx.hpp), NOT conjugated, not exponentiated.  Caller holds the MSM lock.
int miller_product(Context* C, const PairSpan& s0, const PairSpan& s1, gmh::Fq12* out) {
  const size_t n = s0.n + s1.n;
  *out = gmh::Fq12::one();
  if (n == 0) return GM_OK;
  GM_CHECK(n <= ((size_t)1 << 36), GM_EINVAL, "pairing: %zu pairs in one call (at most 2^36)", n);
  hipStream_t st = C->stream;
  PairingWorkspace& ws = C->pairing;
  Profiler& pf = C->prof;
  size_t m = (n + PAIR_BLOCK - 1) / PAIR_BLOCK;
  int rc;
  if ((rc = ws.part[0].ensure(m * GT_BYTES))) return rc;
  if ((rc = ws.part[1].ensure(((m + PAIR_BLOCK - 1) / PAIR_BLOCK) * GT_BYTES))) return rc;
  if (!ws.host_out) GM_HIP(hipHostMalloc((void**)&ws.host_out, GT_HOST_MAX * GT_BYTES, hipHostMallocDefault));
  const PairRange r0{s0.g1, s0.g2, (long long)s0.first1, (long long)s0.step1, (long long)s0.first2, (long long)s0.step2, (unsigned long long)s0.n};
  const PairRange r1{s1.g1, s1.g2, (long long)s1.first1, (long long)s1.step1, (long long)s1.first2, (long long)s1.step2, (unsigned long long)s1.n};
  pf.begin(PROF_ACC0, st);
  hipLaunchKernelGGL(k_miller, dim3((unsigned)m), dim3(PAIR_BLOCK), 0, st, r0, r1, ws.part[0].as<uint8_t>());
  pf.end(PROF_ACC0, st);
  GM_HIP(hipGetLastError());
  int cur = 0;
  pf.begin(PROF_REDUCE, st);
  while (m > GT_HOST_MAX) {
    const size_t mp = (m + PAIR_BLOCK - 1) / PAIR_BLOCK;
    hipLaunchKernelGGL(k_gt_reduce, dim3((unsigned)mp), dim3(PAIR_BLOCK), 0, st, ws.part[cur].as<uint8_t>(), m, ws.part[cur ^ 1].as<uint8_t>());
    cur ^= 1;
    m = mp;
  }
  pf.end(PROF_REDUCE, st);
  GM_HIP(hipGetLastError());
  GM_HIP(hipMemcpyAsync(ws.host_out, ws.part[cur].p, m * GT_BYTES, hipMemcpyDeviceToHost, st));
  GM_HIP(hipStreamSynchronize(st));
  pf.collect();
  gmh::Fq12 f = gmh::Fq12::from_device(ws.host_out);
  for (size_t k = 1; k < m; k++) f = f * gmh::Fq12::from_device(ws.host_out + k * (GT_BYTES / 8));
  *out = f;
  return GM_OK;
}

// One level of the segmented layout: segment s has counts[s] >= 1 lanes.  Fills start / count / out and returns the number of
// lanes of the level; counts becomes the partials per segment (the next level's lanes), *partials their total.  A segment of at
// most PAIR_BLOCK lanes is moved to the next block rather than split, so it yields ONE partial and the levels end: a longer one
// yields at most count / 64 + 2 < count.
static unsigned long long seg_level(std::vector<unsigned long long>& counts, const std::vector<unsigned long long>& starts_or_empty, SegMap* map,
                                    unsigned long long* partials) {
  unsigned long long lane = 0, out = 0;
  for (size_t s = 0; s < counts.size(); s++) {
    const unsigned long long n = counts[s];
    if (!starts_or_empty.empty()) lane = starts_or_empty[s];  // a reduction level reads where the level below wrote
    else if (n <= PAIR_BLOCK && lane % PAIR_BLOCK + n > PAIR_BLOCK) lane = (lane / PAIR_BLOCK + 1) * PAIR_BLOCK;
    const unsigned long long nb = (lane + n - 1) / PAIR_BLOCK - lane / PAIR_BLOCK + 1;
    if (nb <= PAIR_BLOCK && out % PAIR_BLOCK + nb > PAIR_BLOCK) out = (out / PAIR_BLOCK + 1) * PAIR_BLOCK;
    map[s] = SegMap{lane, n, out};
    lane += n;
    out += nb;
    counts[s] = nb;
  }
  *partials = out;
  return lane;
}

// S independent Miller products in one launch per level (NOT conjugated, not exponentiated): out[s] is the product over both spans
// of prods[s], 1 for an empty one.  Caller holds the MSM lock.
int miller_products(Context* C, const PairProduct* prods, size_t S, gmh::Fq12* out) {
  std::vector<size_t> idx;
  std::vector<unsigned long long> counts;
  std::vector<PairSeg> spans;
  for (size_t s = 0; s < S; s++) {
    out[s] = gmh::Fq12::one();
    const PairSpan &a = prods[s].s0, &b = prods[s].s1;
    if (a.n + b.n == 0) continue;
    GM_CHECK(a.n + b.n <= ((size_t)1 << 36), GM_EINVAL, "pairing: %zu pairs in one product (at most 2^36)", a.n + b.n);
    idx.push_back(s);
    counts.push_back(a.n + b.n);
    spans.push_back(PairSeg{PairRange{a.g1, a.g2, (long long)a.first1, (long long)a.step1, (long long)a.first2, (long long)a.step2, (unsigned long long)a.n},
                            PairRange{b.g1, b.g2, (long long)b.first1, (long long)b.step1, (long long)b.first2, (long long)b.step2, (unsigned long long)b.n}});
  }
  const size_t nseg = idx.size();
  if (nseg == 0) return GM_OK;
  GM_CHECK(nseg < ((size_t)1 << 24), GM_EINVAL, "pairing: %zu products in one call (at most 2^24)", nseg);
  // every level's table, then ONE copy: level 0 maps pairs, the others the partials of the level below
  struct Level {
    unsigned long long lanes, partials;
  };
  std::vector<Level> levels;
  std::vector<SegMap> maps;
  std::vector<unsigned long long> starts;
  for (;;) {
    maps.resize(maps.size() + nseg);
    SegMap* m = maps.data() + maps.size() - nseg;
    Level l;
    l.lanes = seg_level(counts, starts, m, &l.partials);
    levels.push_back(l);
    GM_CHECK(l.lanes <= ((unsigned long long)1 << 37), GM_EINVAL, "pairing: %llu lanes in one segmented launch (at most 2^37)", l.lanes);
    if (l.partials == nseg) break;  // one partial per segment, back to back
    starts.resize(nseg);
    for (size_t s = 0; s < nseg; s++) starts[s] = m[s].out;
  }
  hipStream_t st = C->stream;
  PairingWorkspace& ws = C->pairing;
  Profiler& pf = C->prof;
  int rc;
  const size_t span_bytes = nseg * sizeof(PairSeg), map_bytes = maps.size() * sizeof(SegMap);
  if ((rc = ws.seg_tab.ensure(span_bytes + map_bytes))) return rc;
  for (size_t l = 0; l < levels.size(); l++)  // level l writes its partials into part[l & 1]
    if ((rc = ws.part[l & 1].ensure(levels[l].partials * GT_BYTES))) return rc;
  if (ws.host_seg_cap < nseg) {
    if (ws.host_seg) (void)hipHostFree(ws.host_seg);
    ws.host_seg = nullptr;
    ws.host_seg_cap = 0;
    const size_t cap = std::max<size_t>(2 * nseg, 64);
    GM_HIP(hipHostMalloc((void**)&ws.host_seg, cap * GT_BYTES, hipHostMallocDefault));
    ws.host_seg_cap = cap;
  }
  uint8_t* d_tab = ws.seg_tab.as<uint8_t>();
  GM_HIP(hipMemcpyAsync(d_tab, spans.data(), span_bytes, hipMemcpyHostToDevice, st));
  GM_HIP(hipMemcpyAsync(d_tab + span_bytes, maps.data(), map_bytes, hipMemcpyHostToDevice, st));
  const SegMap* d_map = reinterpret_cast<const SegMap*>(d_tab + span_bytes);
  pf.begin(PROF_ACC0, st);
  hipLaunchKernelGGL(k_miller_seg, dim3((unsigned)((levels[0].lanes + PAIR_BLOCK - 1) / PAIR_BLOCK)), dim3(PAIR_BLOCK), 0, st, reinterpret_cast<const PairSeg*>(d_tab), d_map,
                     (unsigned)nseg, ws.part[0].as<uint8_t>());
  pf.end(PROF_ACC0, st);
  GM_HIP(hipGetLastError());
  int cur = 0;
  pf.begin(PROF_REDUCE, st);
  for (size_t l = 1; l < levels.size(); l++) {
    hipLaunchKernelGGL(k_gt_reduce_seg, dim3((unsigned)((levels[l].lanes + PAIR_BLOCK - 1) / PAIR_BLOCK)), dim3(PAIR_BLOCK), 0, st, ws.part[cur].as<uint8_t>(), d_map + l * nseg,
                       (unsigned)nseg, ws.part[cur ^ 1].as<uint8_t>());
    cur ^= 1;
  }
  pf.end(PROF_REDUCE, st);
  GM_HIP(hipGetLastError());
  GM_HIP(hipMemcpyAsync(ws.host_seg, ws.part[cur].p, nseg * GT_BYTES, hipMemcpyDeviceToHost, st));
  GM_HIP(hipStreamSynchronize(st));  // the tables above are read by their copies until here
  pf.collect();
  for (size_t s = 0; s < nseg; s++) out[idx[s]] = gmh::Fq12::from_device(ws.host_seg + s * (GT_BYTES / 8));
  return GM_OK;
}

// Miller product -> GT: conjugation (the loop parameter is negative), then the one final exponentiation
void pairing_finish(const gmh::Fq12& miller, uint64_t out_gt[72]) { gmh::gt_final_exponentiation(miller.conj()).to_limbs(out_gt); }

// prod_i e(g1[first1 + step1 i], g2[first2 + step2 i]) over packed device records
int pairing_run(Context* C, const uint8_t* d_g1, int64_t first1, int64_t step1, const uint8_t* d_g2, int64_t first2, int64_t step2, size_t n, uint64_t out_gt[72]) {
  GM_MSM_LOCK(C);
  PairSpan s;
  s.g1 = d_g1;
  s.g2 = d_g2;
  s.first1 = first1;
  s.step1 = step1;
  s.first2 = first2;
  s.step2 = step2;
  s.n = n;
  gmh::Fq12 f;
  int rc = miller_product(C, s, PairSpan(), &f);
  if (rc) return rc;
  pairing_finish(f, out_gt);
  return GM_OK;
}

// host records on both sides (gm_pairing_multi)
int pairing_run_host(Context* C, const void* g1, size_t stride1, const void* g2, size_t stride2, size_t n, uint64_t out_gt[72]) {
  std::unique_ptr<Bases> b1;
  std::unique_ptr<G2Bases> b2;
  int rc = bases_from_host(C, g1, stride1, n, b1);
  if (!rc) rc = g2_bases_from_host(C, g2, stride2, n, b2);
  if (!rc) rc = pairing_run(C, b1->d, 0, 1, b2->d, 0, 1, n, out_gt);
  if (b1 && b1->d) (void)gm::raw_free(b1->d);
  if (b2 && b2->d) (void)gm::raw_free(b2->d);
  return rc;
}

}  // namespace gm
