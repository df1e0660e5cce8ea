// The BLS12-381 pairing on the device: multi-Miller loop and GT product reduction (gfx950); the herring PModule prover of herring.hip calls them.
// Also here, on the same LDS parking and block product: GtModule's kernels (k_gt_multi_pow, k_gt_split_fold; "GtModule" below).
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
// table of its own; the launch count depends on the longest segment only, never on S.  k_gt_multi_pow_seg is GtModule's power in
// the same form: S independent multi-exponentiations in one launch (gm_gt_multi_pow_many; the GT half of ipa.hip's batched verifier).
//
// ELEMENT BY ELEMENT (k_miller_each, k_gt_final_exp, k_gt_check; "GT element by element" below): one lane per element and no block
// product -- out[i] = e(P_i, Q_i) as one launch of Miller loops and one of final exponentiations by an exact x-chain over the
// cyclotomic squarings of gt.cuh, and the GT membership test.  Vrs::from finishes its Miller values through the same launch.
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

// ---- GtModule: powers of GT elements (GT x Fr -> GT, src/herring/module.rs; ip = prod x_i^e_i) --------------------------------
// One lane per element, acc <- x^e for the 256-bit integer e as given (not reduced mod r), plain fq12_sqr / fq12_mul on any 12
// reduced coefficients: the value of gmh::Fq12::pow.  The exponent is walked in fixed windows of GT_WINDOW bits from the top:
// GT_WINDOW squarings, then ONE product by table[digit] with table[0] = 1 selected in registers, so the 64 lanes of a wave run
// the same instructions whatever their exponents are.  The accumulator is parked in LDS as k_miller parks f; the table x, x^2,
// x^3 of a lane is a [limb][lane] slice of a device workspace (PairingWorkspace::gt_tab), read coalesced.
// GT_WINDOW = 2: 256 squarings x 36 + 128 products x 54 + 108 for the table = 16 236 Fq products per lane.  A window of 4 would
// take 256 x 36 + 64 x 54 + 756 = 13 428 (-17 %) for a table of 15 entries, 8640 B per lane instead of 1728 -- at 2^14 elements
// 141 MB instead of 28 MB of workspace that the table build writes and the loop reads back with per-lane entry indices -- and the
// loop body is the same two operands of 144 registers either way (profiles/gt_module_kernel_resources.txt: the body spills as
// k_gt_reduce's product does).  Measured, the kernel runs at k_miller's time per Fq product (profiles/gt_module.md: 26.6 ms per
// launch), so the wider window would buy its 17 % and nothing else, ~4.5 ms per launch; the narrow one is kept for its footprint.
constexpr int GT_WINDOW = 2;
constexpr int GT_TABLE = (1 << GT_WINDOW) - 1;                      // entries per lane: x^1 .. x^(2^w - 1)
constexpr size_t GT_TAB_BLOCK = (size_t)GT_TABLE * GT_WORDS * PAIR_BLOCK;  // words of table per block
static_assert(256 % GT_WINDOW == 0 && GT_WINDOW < 32, "the window walks 8 x 32-bit words");

// table[d] of the lane, 1 for d = 0 (tab: the block's slice, entry t = x^(t+1) at tab + t * GT_WORDS * PAIR_BLOCK)
GM_DEV Fq12 gt_tab_load(const uint32_t* tab, int lane, uint32_t d) {
  const Fq12 one = fq12_one();
  const FqE* o = reinterpret_cast<const FqE*>(&one);
  const uint32_t* p = tab + (size_t)(d ? d - 1 : 0) * GT_WORDS * PAIR_BLOCK;
  Fq12 a;
  FqE* e = reinterpret_cast<FqE*>(&a);
#pragma unroll
  for (int k = 0; k < 12; k++) {
#pragma unroll
    for (int i = 0; i < Fq::N; i++) {
      const uint32_t v = p[(k * Fq::N + i) * PAIR_BLOCK + lane];
      e[k].l[i] = d ? v : o[k].l[i];
    }
  }
  return a;
}

// x^e into the lane's column of sh (1 when the lane is not live); e: 8 words, least significant first, consumed
GM_DEV void gt_pow_lane(uint32_t* sh, uint32_t* tab, int lane, bool live, const Fq12& x, uint32_t e[8]) {
  gt_lds_store(sh, lane, fq12_one());
  if (live) {
    Fq12 p = x;
    gt_lds_store(tab, lane, p);
#pragma unroll 1
    for (int t = 1; t < GT_TABLE; t++) {  // x^(t+1) = x^t x (x^2 as a product: one code path, 18 Fq products of 16 236)
      p = fq12_mul(p, gt_lds_load(tab, lane));
      gt_lds_store(tab + (size_t)t * GT_WORDS * PAIR_BLOCK, lane, p);
    }
#pragma unroll 1
    for (int w = 0; w < 256 / GT_WINDOW; w++) {
      const uint32_t d = e[7] >> (32 - GT_WINDOW);  // the top digit, then the exponent moves up by one window
#pragma unroll
      for (int i = 7; i > 0; i--) e[i] = (e[i] << GT_WINDOW) | (e[i - 1] >> (32 - GT_WINDOW));
      e[0] <<= GT_WINDOW;
      Fq12 f = gt_lds_load(sh, lane);
#pragma unroll 1
      for (int k = 0; k < GT_WINDOW; k++) f = fq12_sqr(f);
      gt_lds_store(sh, lane, fq12_mul(f, gt_tab_load(tab, lane, d)));
    }
  }
}

// Up to three ranges of (element, exponent) per launch: term i of a range is x[first_x + step_x i] (576-byte device records)
// to the power e[first_e + step_e i] (32-byte records: Fr in Montgomery form when `mont`, else 8 canonical words as they are)
struct GtRange {
  const uint8_t* x;
  const uint8_t* e;
  long long first_x, step_x, first_e, step_e;
  unsigned long long n;
};

__global__ __launch_bounds__(PAIR_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_gt_multi_pow(GtRange r0, GtRange r1, GtRange r2, int mont, uint32_t* __restrict__ tab,
                                                                                                           uint8_t* __restrict__ partials) {
  __shared__ uint32_t sh[GT_WORDS * PAIR_BLOCK];
  const int lane = threadIdx.x;
  const unsigned long long i = (unsigned long long)blockIdx.x * PAIR_BLOCK + lane;
  const bool live = i < r0.n + r1.n + r2.n;
  Fq12 x = fq12_one();
  uint32_t e[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live) {
    const GtRange r = i < r0.n ? r0 : i < r0.n + r1.n ? r1 : r2;
    const long long k = (long long)(i < r0.n ? i : i < r0.n + r1.n ? i - r0.n : i - r0.n - r1.n);
    x = fq12_load(r.x + (size_t)(r.first_x + r.step_x * k) * GT_BYTES);
    Fr s = fp_load<FrParams>(r.e + (size_t)(r.first_e + r.step_e * k) * 32);
    if (mont) s = fp_from_mont<FrParams>(s);
#pragma unroll
    for (int j = 0; j < 8; j++) e[j] = s.l[j];
  }
  gt_pow_lane(sh, tab + (size_t)blockIdx.x * GT_TAB_BLOCK, lane, live, x, e);
  gt_block_product(sh, lane);
  if (lane == 0) fq12_store(partials + (size_t)blockIdx.x * GT_BYTES, gt_lds_load(sh, 0));
}

// herring split_fold over GT (src/herring/time_prover.rs:72-76, multiplicative): out[i] = f[2i] f[2i+1]^s, an odd tail is
// out[i] = f[2i].  s8: the canonical scalar, 8 x u32 -- the same in every lane.  One lane per output.
__global__ __launch_bounds__(PAIR_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_gt_split_fold(const uint8_t* __restrict__ in, size_t n, const uint32_t* __restrict__ s8,
                                                                                                            uint32_t* __restrict__ tab, uint8_t* __restrict__ out) {
  __shared__ uint32_t sh[GT_WORDS * PAIR_BLOCK];
  const int lane = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * PAIR_BLOCK + lane, m = (n + 1) / 2;
  const bool live = 2 * i + 1 < n;
  uint32_t e[8];
#pragma unroll
  for (int j = 0; j < 8; j++) e[j] = s8[j];
  gt_pow_lane(sh, tab + (size_t)blockIdx.x * GT_TAB_BLOCK, lane, live, live ? fq12_load(in + (2 * i + 1) * GT_BYTES) : fq12_one(), e);
  if (i < m) {
    const Fq12 lo = fq12_load(in + (2 * i) * GT_BYTES);
    fq12_store(out + i * GT_BYTES, live ? fq12_mul(lo, gt_lds_load(sh, lane)) : lo);
  }
}

// host records (12 Fq in ark-ff's Montgomery form, 2^384) -> device records (2^390), in place: one thread per coefficient
__global__ __launch_bounds__(256) void k_gt_import(uint8_t* __restrict__ d, size_t ncoef) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ncoef) fqe_store(d + i * 48, fqe_import(fqe_load(d + i * 48)));
}

// device records -> host records (ark-ff's Montgomery form), in place
__global__ __launch_bounds__(256) void k_gt_export(uint8_t* __restrict__ d, size_t ncoef) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ncoef) fqe_store(d + i * 48, fqe_export(fqe_load(d + i * 48)));
}

// ---- GT element by element: final exponentiation, pairings, membership (one lane per element, no block product) ----------------
// The lane's running value is parked in its LDS column, as k_miller parks f.  LDS holds ONE Fq12 per lane (36 KiB per block, four
// blocks per CU); every other value that has to survive a power -- the base of fq12_pow_x, the saved m and c of the chain -- lies
// in a [limb][lane] column of the block's slice of PairingWorkspace::gt_tab (GT_SLOTS columns per lane, the table of
// k_gt_multi_pow reused), read coalesced.
constexpr int GT_SLOTS = 3;
static_assert(GT_SLOTS <= GT_TABLE, "the slots are the table entries of k_gt_multi_pow's workspace");
GM_DEV uint32_t* gt_slot(uint32_t* tab, int t, int lane) { return tab + (size_t)t * GT_WORDS * PAIR_BLOCK + lane; }

// f^((q^12 - 1) / r) for the lane: f in registers, the result in registers.  With x = -|x| and h = (q^4 - q^2 + 1) / r,
//   (q^12 - 1) / r = (q^6 - 1)(q^2 + 1) h,   h = ((x - 1)^2 / 3)(x + q)(x^2 + q^2 - 1) + 1   (exact; (x - 1)^2 / 3 = ((|x| + 1) / 3)(|x| + 1))
// so the value is gmh::gt_final_exponentiation's on ANY 12 reduced coefficients (the easy part lands in the cyclotomic subgroup
// whatever f is, 0 stays 0).  Fq products as written: easy part 837, 614 of them the one Fermat inversion in Fq; powers 62 x 18 +
// 27 x 54 and 4 x (63 x 18 + 5 x 54); 6 products, 3 Frobenius maps: 9322 in all (tools/gt_device_bench.py counts them the same way).
GM_DEV Fq12 gt_final_exp_lane(uint32_t* sh, uint32_t* tab, int lane, const Fq12& f) {
  uint32_t* acc = sh + lane;
  uint32_t *s0 = gt_slot(tab, 0, lane), *s1 = gt_slot(tab, 1, lane), *s2 = gt_slot(tab, 2, lane);
  {
    const Fq12 a = fq12_mul(fq12_conj(f), fq12_inv(f));  // f^(q^6 - 1)
    const Fq12 m = fq12_mul(fq12_frobenius2(a), a);      // ^(q^2 + 1): cyclotomic from here on, the inverse is the conjugate
    fq12_col_store(s0, PAIR_BLOCK, m);
    fq12_col_store(s1, PAIR_BLOCK, m);
  }
  fq12_pow_const(acc, s0, PAIR_BLOCK, BLS_X_ABS_P1_DIV3);  // a = m^((|x| + 1) / 3)
  fq12_col_store(s0, PAIR_BLOCK, fq12_col_load(acc, PAIR_BLOCK));
  fq12_pow_x(acc, s0, PAIR_BLOCK);
  fq12_col_store(s0, PAIR_BLOCK, fq12_mul(fq12_col_load(acc, PAIR_BLOCK), fq12_col_load(s0, PAIR_BLOCK)));  // b = a^(|x| + 1) = m^((x - 1)^2 / 3)
  fq12_pow_x(acc, s0, PAIR_BLOCK);
  {
    const Fq12 c = fq12_mul(fq12_conj(fq12_col_load(acc, PAIR_BLOCK)), fq12_frobenius1(fq12_col_load(s0, PAIR_BLOCK)));  // b^(x + q)
    fq12_col_store(s0, PAIR_BLOCK, c);
    fq12_col_store(s2, PAIR_BLOCK, c);
  }
  fq12_pow_x(acc, s0, PAIR_BLOCK);
  fq12_col_store(s0, PAIR_BLOCK, fq12_col_load(acc, PAIR_BLOCK));
  fq12_pow_x(acc, s0, PAIR_BLOCK);  // c^(x^2): the two signs cancel
  Fq12 d = fq12_mul(fq12_col_load(acc, PAIR_BLOCK), fq12_frobenius2(fq12_col_load(s2, PAIR_BLOCK)));
  d = fq12_mul(d, fq12_conj(fq12_col_load(s2, PAIR_BLOCK)));  // c^(x^2 + q^2 - 1)
  return fq12_mul(d, fq12_col_load(s1, PAIR_BLOCK));          // ... + 1
}

// out[i] = in[i]^((q^12 - 1) / r) over device records, conjugated first when `conj` (Miller values: x < 0); in == out is fine
__global__ __launch_bounds__(PAIR_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_gt_final_exp(const uint8_t* in, size_t n, int conj, uint32_t* __restrict__ tab, uint8_t* out) {
  __shared__ uint32_t sh[GT_WORDS * PAIR_BLOCK];
  const int lane = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * PAIR_BLOCK + lane;
  Fq12 f = i < n ? fq12_load(in + i * GT_BYTES) : fq12_one();
  if (conj) f = fq12_conj(f);
  f = gt_final_exp_lane(sh, tab + (size_t)blockIdx.x * GT_TAB_BLOCK, lane, f);
  if (i < n) fq12_store(out + i * GT_BYTES, f);
}

// out[i] = f_{|x|, Q_i}(P_i), the lane's own Miller value (1 when either point is the identity): the loop of k_miller, no product
__global__ __launch_bounds__(PAIR_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_miller_each(PairRange r, uint8_t* __restrict__ out) {
  __shared__ uint32_t sh[GT_WORDS * PAIR_BLOCK];
  const int lane = threadIdx.x;
  const unsigned long long i = (unsigned long long)blockIdx.x * PAIR_BLOCK + lane;
  G1Affine P;
  G2Affine Q;
  bool live = false;
  if (i < r.n) {
    P = g1_load_affine(r.g1 + (size_t)(r.first1 + r.step1 * (long long)i) * G1_AFF_BYTES);
    Q = g2_load_affine(r.g2 + (size_t)(r.first2 + r.step2 * (long long)i) * G2_AFF_BYTES);
    live = !(P.is_identity() || Q.is_identity());
  }
  miller_lane(sh, lane, live, P, Q);
  if (i < r.n) fq12_store(out + (size_t)i * GT_BYTES, gt_lds_load(sh, lane));
}

// GT membership, one status byte per element: the first test that fails of
//   1. a coefficient >= q                    GM_PT_NONCANONICAL    (host_form only: resident records are reduced by construction)
//   2. f = 0 or f^(q^4) f != f^(q^2)         GM_PT_NOT_CYCLOTOMIC  (two Frobenius maps and a product: valid for any f)
//   3. f^q != conj(f^|x|), i.e. f^q != f^x   GM_PT_NOT_IN_SUBGROUP (cyclotomic squarings, licensed by 2.)
// 2. and 3. give f^(x^4 - x^2 + 1) = f^r = 1: q^4 - q^2 + 1 = 0 on f by 2., q = x on f by 3., r = x^4 - x^2 + 1 for BLS12.
// Every lane runs every test and selects its status at the end; summary[block] is the block's first bad lane (GT_NO_BAD: none).
// Fq products as written: 2 x 10 + 54 + 1404 + 15 = ~1500.
constexpr uint32_t GT_NO_BAD = 0xffffffffu;
__global__ __launch_bounds__(PAIR_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_gt_check(const uint8_t* __restrict__ src, int host_form, size_t n, uint32_t* __restrict__ tab,
                                                                                                       uint8_t* __restrict__ status, uint32_t* __restrict__ summary) {
  __shared__ uint32_t sh[GT_WORDS * PAIR_BLOCK];
  const int lane = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * PAIR_BLOCK + lane;
  Fq12 f = fq12_one();
  bool canonical = true;
  if (i < n) {
    f = fq12_load(src + i * GT_BYTES);
    if (host_form) {
      FqE* e = reinterpret_cast<FqE*>(&f);
#pragma unroll
      for (int k = 0; k < 12; k++) canonical = canonical && !pt_raw_ge_q(e[k]);
      if (!canonical) f = fq12_one();  // no value to go on with; the lane still runs the tests
#pragma unroll
      for (int k = 0; k < 12; k++) e[k] = canonical ? fqe_import(e[k]) : e[k];
    }
  }
  uint32_t* s0 = gt_slot(tab + (size_t)blockIdx.x * GT_TAB_BLOCK, 0, lane);
  fq12_col_store(s0, PAIR_BLOCK, f);
  bool cyclotomic;
  {
    const Fq12 f2 = fq12_frobenius2(f);
    cyclotomic = !fq12_is_zero(f) && fq12_eq(fq12_mul(fq12_frobenius2(f2), f), f2);
  }
  fq12_pow_x(sh + lane, s0, PAIR_BLOCK);
  const bool member = fq12_eq(fq12_frobenius1(fq12_col_load(s0, PAIR_BLOCK)), fq12_conj(fq12_col_load(sh + lane, PAIR_BLOCK)));
  const uint8_t st = !canonical ? GM_PT_NONCANONICAL : !cyclotomic ? GM_PT_NOT_CYCLOTOMIC : !member ? GM_PT_NOT_IN_SUBGROUP : GM_PT_OK;
  const bool bad = i < n && st != GM_PT_OK;
  if (i < n) status[i] = st;
  const unsigned long long m = __ballot(bad);  // one wave per block
  if (lane == 0) summary[blockIdx.x] = m ? (uint32_t)__ffsll((long long)m) - 1u : GT_NO_BAD;
}

// gm_debug_gt_op: ONE of the device functions of gt.cuh per lane, over device records
enum { GT_OP_FROBENIUS1 = 0, GT_OP_FROBENIUS2 = 1, GT_OP_INVERSE = 2, GT_OP_CYCLOTOMIC_SQR = 3, GT_OP_POW_X = 4 };
__global__ __launch_bounds__(PAIR_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_gt_debug_op(int op, const uint8_t* in, size_t n, uint32_t* __restrict__ tab, uint8_t* out) {
  __shared__ uint32_t sh[GT_WORDS * PAIR_BLOCK];
  const int lane = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * PAIR_BLOCK + lane;
  const Fq12 f = i < n ? fq12_load(in + i * GT_BYTES) : fq12_one();
  Fq12 r;
  if (op == GT_OP_FROBENIUS1) {
    r = fq12_frobenius1(f);
  } else if (op == GT_OP_FROBENIUS2) {
    r = fq12_frobenius2(f);
  } else if (op == GT_OP_INVERSE) {
    r = fq12_inv(f);
  } else if (op == GT_OP_CYCLOTOMIC_SQR) {
    r = fq12_cyclotomic_sqr(f);
  } else {
    uint32_t* s0 = gt_slot(tab + (size_t)blockIdx.x * GT_TAB_BLOCK, 0, lane);
    fq12_col_store(s0, PAIR_BLOCK, f);
    fq12_pow_x(sh + lane, s0, PAIR_BLOCK);
    r = fq12_col_load(sh + lane, PAIR_BLOCK);
  }
  if (i < n) fq12_store(out + i * GT_BYTES, r);
}

// gm_debug_gt_op2: ONE of the Miller-loop functions of gt.cuh per lane, over device records a and b (b is read by the ops that
// take a second operand only).  The Fq6 ops run on both halves (c0 with c0, c1 with c1), the Fq2 ops on each of the six Fq2 slots;
// a line (l0, l1, l4) is the first three Fq2 slots of b, an Fq scalar the c0 of b's slot.
enum {
  GT_OP2_MUL = 0, GT_OP2_SQR = 1, GT_OP2_CONJ = 2, GT_OP2_MUL_014 = 3, GT_OP2_FQ6_MUL = 4, GT_OP2_FQ6_MUL_V = 5, GT_OP2_FQ6_MUL_01 = 6,
  GT_OP2_FQ6_MUL_1 = 7, GT_OP2_FQ2_MUL_XI = 8, GT_OP2_FQ2_MUL12 = 9, GT_OP2_FQ2_MUL_FQ = 10, GT_OP2_FQ2_CONJ = 11, GT_OP2_END = 12
};
static bool gt_op2_is_binary(int op) {
  return op == GT_OP2_MUL || op == GT_OP2_MUL_014 || op == GT_OP2_FQ6_MUL || op == GT_OP2_FQ6_MUL_01 || op == GT_OP2_FQ6_MUL_1 || op == GT_OP2_FQ2_MUL_FQ;
}
__global__ __launch_bounds__(PAIR_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_gt_debug_op2(int op, const uint8_t* a_in, const uint8_t* b_in, size_t n, uint8_t* out) {
  const size_t i = (size_t)blockIdx.x * PAIR_BLOCK + threadIdx.x;
  if (i >= n) return;
  const Fq12 a = fq12_load(a_in + i * GT_BYTES);
  const Fq12 b = b_in ? fq12_load(b_in + i * GT_BYTES) : fq12_one();
  const Fq2* as = reinterpret_cast<const Fq2*>(&a);  // 6 Fq2 back to back, tower order
  const Fq2* bs = reinterpret_cast<const Fq2*>(&b);
  Fq12 r;
  Fq2* rs = reinterpret_cast<Fq2*>(&r);
  if (op == GT_OP2_MUL) {
    r = fq12_mul(a, b);
  } else if (op == GT_OP2_SQR) {
    r = fq12_sqr(a);
  } else if (op == GT_OP2_CONJ) {
    r = fq12_conj(a);
  } else if (op == GT_OP2_MUL_014) {
    r = fq12_mul_014(a, bs[0], bs[1], bs[2]);
  } else if (op == GT_OP2_FQ6_MUL) {
    r.c0 = fq6_mul(a.c0, b.c0);
    r.c1 = fq6_mul(a.c1, b.c1);
  } else if (op == GT_OP2_FQ6_MUL_V) {
    r.c0 = fq6_mul_v(a.c0);
    r.c1 = fq6_mul_v(a.c1);
  } else if (op == GT_OP2_FQ6_MUL_01) {
    r.c0 = fq6_mul_01(a.c0, bs[0], bs[1]);
    r.c1 = fq6_mul_01(a.c1, bs[0], bs[1]);
  } else if (op == GT_OP2_FQ6_MUL_1) {
    r.c0 = fq6_mul_1(a.c0, bs[0]);
    r.c1 = fq6_mul_1(a.c1, bs[0]);
  } else {
#pragma unroll
    for (int k = 0; k < 6; k++)
      rs[k] = op == GT_OP2_FQ2_MUL_XI ? fq2_mul_xi(as[k]) : op == GT_OP2_FQ2_MUL12 ? fq2_mul12(as[k]) : op == GT_OP2_FQ2_MUL_FQ ? fq2_mul_fq(as[k], bs[k].c0) : fq2_conj(as[k]);
  }
  fq12_store(out + i * GT_BYTES, r);
}

// gm_debug_miller_step: ONE step of the Miller loop per lane.  A record of 576 bytes in: T (X | Y | Z, any Z), Q (x | y), P (x | y, two
// field elements as they are: the steps only multiply by them); out: the new T (X | Y | Z) and the line (l0 | l1 | l4).
enum { MILLER_OP_DBL = 0, MILLER_OP_ADD = 1 };
static_assert(3 * 96 + G2_AFF_BYTES + G1_AFF_BYTES == GT_BYTES, "T | Q | P is one GT record");
__global__ __launch_bounds__(PAIR_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_miller_debug_step(int op, const uint8_t* in, size_t n, uint8_t* out) {
  const size_t i = (size_t)blockIdx.x * PAIR_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint8_t* p = in + i * GT_BYTES;
  G2Proj T;
  T.x = fq2_load(p);
  T.y = fq2_load(p + 96);
  T.z = fq2_load(p + 192);
  const G2Affine Q = g2_load_affine(p + 288);
  const G1Affine P = g1_load_affine(p + 288 + G2_AFF_BYTES);
  const Line l = op == MILLER_OP_DBL ? miller_dbl_step(T, P) : miller_add_step(T, Q, P);
  uint8_t* o = out + i * GT_BYTES;
  fq2_store(o, T.x);
  fq2_store(o + 96, T.y);
  fq2_store(o + 192, T.z);
  fq2_store(o + 288, l.l0);
  fq2_store(o + 384, l.l1);
  fq2_store(o + 480, l.l4);
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

// k_gt_multi_pow over a table of products: lane -> (segment, term), the power of gt_pow_lane, one partial per (block, segment).
// Term t names a row of x (576-byte device records) and a row of e (32 bytes: 8 canonical words as they are), so many terms may
// raise the same element; first[s] is the first term of segment s.  Both indices come from the host, which has checked them; the
// only address a lane forms from the VALUE of an exponent is the 2-bit digit that picks one of the three table entries of its own
// slice (gt_tab_load), and none from the value of an element.  (GtTerm: ctx.hpp)
__global__ __launch_bounds__(PAIR_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_gt_multi_pow_seg(const uint8_t* __restrict__ x, const uint8_t* __restrict__ e,
                                                                                                               const GtTerm* __restrict__ terms,
                                                                                                               const unsigned long long* __restrict__ first,
                                                                                                               const SegMap* __restrict__ map, unsigned nseg, uint32_t* __restrict__ tab,
                                                                                                               uint8_t* __restrict__ partials) {
  __shared__ uint32_t sh[GT_WORDS * PAIR_BLOCK];
  __shared__ uint32_t seg[PAIR_BLOCK];
  const int lane = threadIdx.x;
  const unsigned long long i = (unsigned long long)blockIdx.x * PAIR_BLOCK + lane;
  const uint32_t sid = seg_find(map, nseg, i);
  const bool live = sid != NO_SEG;
  Fq12 f = fq12_one();
  uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live) {
    const GtTerm t = terms[first[sid] + (i - map[sid].start)];
    f = fq12_load(x + (size_t)t.x * GT_BYTES);
    const Fr s = fp_load<FrParams>(e + (size_t)t.e * 32);
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = s.l[j];
  }
  gt_pow_lane(sh, tab + (size_t)blockIdx.x * GT_TAB_BLOCK, lane, live, f, w);
  gt_block_product_seg(sh, seg, lane, sid, map, partials);
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
void pairing_workspace_release(PairingWorkspace& w) {
  for (DevBuf& b : w.part) b.release();
  if (w.host_out) (void)hipHostFree(w.host_out);
  w.host_out = nullptr;
  w.seg_tab.release();
  w.gt_tab.release();
  if (w.host_seg) (void)hipHostFree(w.host_seg);
  w.host_seg = nullptr;
  w.host_seg_cap = 0;
}

// room for the m partials of a launch (part[0]), the level behind them and the pinned copy of the last few
static int gt_partials_ensure(PairingWorkspace& ws, size_t m) {
  int rc;
  if ((rc = ws.part[0].ensure(m * GT_BYTES))) return rc;
  if ((rc = ws.part[1].ensure(((m + PAIR_BLOCK - 1) / PAIR_BLOCK) * GT_BYTES))) return rc;
  if (!ws.host_out) GM_HIP(hipHostMalloc((void**)&ws.host_out, GT_HOST_MAX * GT_BYTES, hipHostMallocDefault));
  return GM_OK;
}
static int gt_reduce_partials(Context* C, size_t m, gmh::Fq12* out);
static int gt_to_host(Context* C, uint8_t* d, size_t n, uint64_t* out);

// The Miller product of both spans (PairSpan: ctx.hpp), NOT conjugated, not exponentiated.  Caller holds the MSM lock.
int miller_product(Context* C, const PairSpan& s0, const PairSpan& s1, gmh::Fq12* out) {
  const size_t n = s0.n + s1.n;
  *out = gmh::Fq12::one();
  if (n == 0) return GM_OK;
  GM_CHECK(n <= ((size_t)1 << 36), GM_EINVAL, "pairing: %zu pairs in one call (at most 2^36)", n);
  hipStream_t st = C->stream;
  PairingWorkspace& ws = C->pairing;
  Profiler& pf = C->prof;
  const size_t m = (n + PAIR_BLOCK - 1) / PAIR_BLOCK;
  int rc;
  if ((rc = gt_partials_ensure(ws, m))) return rc;
  const PairRange r0{s0.g1, s0.g2, (long long)s0.first1, (long long)s0.step1, (long long)s0.first2, (long long)s0.step2, (unsigned long long)s0.n};
  const PairRange r1{s1.g1, s1.g2, (long long)s1.first1, (long long)s1.step1, (long long)s1.first2, (long long)s1.step2, (unsigned long long)s1.n};
  pf.begin(PROF_ACC0, st);
  hipLaunchKernelGGL(k_miller, dim3((unsigned)m), dim3(PAIR_BLOCK), 0, st, r0, r1, ws.part[0].as<uint8_t>());
  pf.end(PROF_ACC0, st);
  GM_HIP(hipGetLastError());
  return gt_reduce_partials(C, m, out);
}

// The product of the m partials that a launch left in part[0] (both levels and the pinned copy are there): k_gt_reduce levels,
// the copy of the last few, their product on the host.  Behind k_miller and k_gt_multi_pow alike.
static int gt_reduce_partials(Context* C, size_t m, gmh::Fq12* out) {
  hipStream_t st = C->stream;
  PairingWorkspace& ws = C->pairing;
  Profiler& pf = C->prof;
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

// ---- GtModule on the host side: prod x_i^e_i over up to three spans (GtSpan: ctx.hpp).  Caller holds the MSM lock. ------------------
int gt_multi_pow(Context* C, const GtSpan spans[3], int mont, gmh::Fq12* out) {
  const size_t n = spans[0].n + spans[1].n + spans[2].n;
  *out = gmh::Fq12::one();
  if (n == 0) return GM_OK;
  GM_CHECK(spans[0].n <= ((size_t)1 << 36) && spans[1].n <= ((size_t)1 << 36) && spans[2].n <= ((size_t)1 << 36), GM_EINVAL,
           "gt_multi_pow: %zu terms in one call (at most 2^36 per span)", n);
  hipStream_t st = C->stream;
  PairingWorkspace& ws = C->pairing;
  Profiler& pf = C->prof;
  const size_t m = (n + PAIR_BLOCK - 1) / PAIR_BLOCK;
  int rc;
  if ((rc = gt_partials_ensure(ws, m))) return rc;
  if ((rc = ws.gt_tab.ensure(m * GT_TAB_BLOCK * sizeof(uint32_t)))) return rc;
  GtRange r[3];
  for (int j = 0; j < 3; j++)
    r[j] = GtRange{spans[j].x, spans[j].e, (long long)spans[j].first_x, (long long)spans[j].step_x, (long long)spans[j].first_e, (long long)spans[j].step_e,
                   (unsigned long long)spans[j].n};
  pf.begin(PROF_ACC0, st);
  hipLaunchKernelGGL(k_gt_multi_pow, dim3((unsigned)m), dim3(PAIR_BLOCK), 0, st, r[0], r[1], r[2], mont, ws.gt_tab.as<uint32_t>(), ws.part[0].as<uint8_t>());
  pf.end(PROF_ACC0, st);
  GM_HIP(hipGetLastError());
  return gt_reduce_partials(C, m, out);
}

// out[i] = in[2i] in[2i+1]^s over device records, s at d_s8 (canonical, 8 x u32), on C->stream without a wait.  Caller holds the
// MSM lock (the table workspace) and collects the profiler after its wait.
int gt_split_fold_launch(Context* C, const uint8_t* in, size_t n, const uint32_t* d_s8, uint8_t* out) {
  const size_t blocks = ((n + 1) / 2 + PAIR_BLOCK - 1) / PAIR_BLOCK;
  if (blocks == 0) return GM_OK;
  int rc = C->pairing.gt_tab.ensure(blocks * GT_TAB_BLOCK * sizeof(uint32_t));
  if (rc) return rc;
  C->prof.begin(PROF_ACC0, C->stream);
  hipLaunchKernelGGL(k_gt_split_fold, dim3((unsigned)blocks), dim3(PAIR_BLOCK), 0, C->stream, in, n, d_s8, C->pairing.gt_tab.as<uint32_t>(), out);
  C->prof.end(PROF_ACC0, C->stream);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

// n host records of 72 x u64 (ark-ff's Montgomery form) as a device vector of 576-byte records: a dev_malloc block the caller frees
int gt_from_host(Context* C, const uint64_t* x, size_t n, uint8_t** d) {
  *d = nullptr;
  uint8_t* p = nullptr;
  GM_HIP(dev_malloc((void**)&p, n * GT_BYTES));
  const size_t ncoef = n * 12;
  hipError_t e = hipMemcpyAsync(p, x, n * GT_BYTES, hipMemcpyHostToDevice, C->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_gt_import, dim3((unsigned)((ncoef + 255) / 256)), dim3(256), 0, C->stream, p, ncoef);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(C->stream);  // `x` is read by the copy until here
  if (e != hipSuccess) {
    (void)gm::raw_free(p);
    GM_HIP(e);
  }
  *d = p;
  return GM_OK;
}

// gm_gt_multi_pow: host elements and canonical 256-bit exponents (n x 4 u64, as they are)
static int gt_multi_pow_staged(Context* C, const uint8_t* dx, uint8_t* de, const uint64_t* scalars_canonical, size_t n, uint64_t out_gt[72]) {
  GM_HIP(hipMemcpyAsync(de, scalars_canonical, n * 32, hipMemcpyHostToDevice, C->stream));
  GtSpan s[3];
  s[0].x = dx;
  s[0].e = de;
  s[0].n = n;
  gmh::Fq12 f;
  int rc = gt_multi_pow(C, s, 0, &f);  // ends in a wait: the scalars have been copied
  if (rc) return rc;
  f.to_limbs(out_gt);
  return GM_OK;
}
int gt_multi_pow_host(Context* C, const uint64_t* x, const uint64_t* scalars_canonical, size_t n, uint64_t out_gt[72]) {
  GM_MSM_LOCK(C);
  uint8_t *dx = nullptr, *de = nullptr;
  int rc = gt_from_host(C, x, n, &dx);
  if (rc) return rc;
  const hipError_t e = dev_malloc((void**)&de, n * 32);
  if (e == hipSuccess) {
    rc = gt_multi_pow_staged(C, dx, de, scalars_canonical, n, out_gt);
    if (rc) (void)hipStreamSynchronize(C->stream);  // nothing in flight reads the two vectors once they go
    (void)gm::raw_free(de);
  }
  (void)gm::raw_free(dx);
  GM_HIP(e);
  return rc;
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

// Every level of the layout for segments of counts[s] >= 1 lanes: `maps` gets one table of counts.size() entries per level (level
// 0 maps the terms, the others the partials of the level below), the last level leaves one partial per segment, back to back.
struct SegLevel {
  unsigned long long lanes, partials;
};
static int seg_levels(std::vector<unsigned long long>& counts, std::vector<SegMap>& maps, std::vector<SegLevel>& levels) {
  const size_t nseg = counts.size();
  std::vector<unsigned long long> starts;
  for (;;) {
    maps.resize(maps.size() + nseg);
    SegMap* m = maps.data() + maps.size() - nseg;
    SegLevel l;
    l.lanes = seg_level(counts, starts, m, &l.partials);
    levels.push_back(l);
    GM_CHECK(l.lanes <= ((unsigned long long)1 << 37), GM_EINVAL, "pairing: %llu lanes in one segmented launch (at most 2^37)", l.lanes);
    if (l.partials == nseg) break;  // one partial per segment, back to back
    starts.resize(nseg);
    for (size_t s = 0; s < nseg; s++) starts[s] = m[s].out;
  }
  return GM_OK;
}

// The launches of S independent Miller products, one per level (NOT conjugated, not exponentiated), on C->stream without a wait:
// the products of the non-empty prods[idx[k]], k < idx.size(), end as consecutive device records at *d_out (a level buffer of the
// workspace).  Caller holds the MSM lock and keeps `t` until it has waited for the stream: the copies of the tables read it.
struct SegTables {
  std::vector<size_t> idx;
  std::vector<PairSeg> spans;
  std::vector<SegMap> maps;
};
static int miller_products_launch(Context* C, const PairProduct* prods, size_t S, SegTables& t, uint8_t** d_out) {
  std::vector<unsigned long long> counts;
  std::vector<size_t>& idx = t.idx;
  std::vector<PairSeg>& spans = t.spans;
  std::vector<SegMap>& maps = t.maps;
  *d_out = nullptr;
  for (size_t s = 0; s < S; s++) {
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
  std::vector<SegLevel> levels;
  int rc = seg_levels(counts, maps, levels);
  if (rc) return rc;
  hipStream_t st = C->stream;
  PairingWorkspace& ws = C->pairing;
  Profiler& pf = C->prof;
  const size_t span_bytes = nseg * sizeof(PairSeg), map_bytes = maps.size() * sizeof(SegMap);
  if ((rc = ws.seg_tab.ensure(span_bytes + map_bytes))) return rc;
  for (size_t l = 0; l < levels.size(); l++)  // level l writes its partials into part[l & 1]
    if ((rc = ws.part[l & 1].ensure(levels[l].partials * GT_BYTES))) return rc;
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
  *d_out = ws.part[cur].as<uint8_t>();
  return GM_OK;
}

// S independent Miller products (NOT conjugated, not exponentiated): out[s] is the product over both spans of prods[s], 1 for an
// empty one.  Caller holds the MSM lock.
int miller_products(Context* C, const PairProduct* prods, size_t S, gmh::Fq12* out) {
  for (size_t s = 0; s < S; s++) out[s] = gmh::Fq12::one();
  SegTables t;
  uint8_t* d = nullptr;
  int rc = miller_products_launch(C, prods, S, t, &d);
  const size_t nseg = t.idx.size();
  if (rc || nseg == 0) {
    if (rc) (void)hipStreamSynchronize(C->stream);
    return rc;
  }
  PairingWorkspace& ws = C->pairing;
  if (ws.host_seg_cap < nseg) {
    if (ws.host_seg) (void)hipHostFree(ws.host_seg);
    ws.host_seg = nullptr;
    ws.host_seg_cap = 0;
    const size_t cap = std::max<size_t>(2 * nseg, 64);
    GM_HIP(hipHostMalloc((void**)&ws.host_seg, cap * GT_BYTES, hipHostMallocDefault));
    ws.host_seg_cap = cap;
  }
  GM_HIP(hipMemcpyAsync(ws.host_seg, d, nseg * GT_BYTES, hipMemcpyDeviceToHost, C->stream));
  GM_HIP(hipStreamSynchronize(C->stream));  // the tables of `t` are read by their copies until here
  C->prof.collect();
  for (size_t s = 0; s < nseg; s++) out[t.idx[s]] = gmh::Fq12::from_device(ws.host_seg + s * (GT_BYTES / 8));
  return GM_OK;
}

// The same products as GT elements: conjugated and raised to (q^12 - 1) / r by ONE k_gt_final_exp launch over the S Miller values
// where the reduction left them (Vrs::from: 4 (log2 len - 1) of them); out_gt: S x 72 limbs.  Caller holds the MSM lock.
int pairing_products(Context* C, const PairProduct* prods, size_t S, uint64_t* out_gt) {
  SegTables t;
  uint8_t* d = nullptr;
  int rc = miller_products_launch(C, prods, S, t, &d);
  const size_t nseg = t.idx.size();
  std::vector<uint64_t> got(nseg * 72);
  if (!rc && nseg) rc = gt_final_exp_launch(C, d, nseg, 1, d);
  if (!rc && nseg) rc = gt_to_host(C, d, nseg, got.data());  // ends in a wait
  if (rc) {
    (void)hipStreamSynchronize(C->stream);
    return rc;
  }
  for (size_t s = 0; s < S; s++) gmh::Fq12::one().to_limbs(out_gt + 72 * s);
  for (size_t s = 0; s < nseg; s++) memcpy(out_gt + 72 * t.idx[s], got.data() + 72 * s, GT_BYTES);
  return GM_OK;
}

// gm_pairing_multi_many: host records on both sides, product s over the pairs [offsets[s], offsets[s + 1])
int pairing_products_host(Context* C, const void* g1, size_t stride1, const void* g2, size_t stride2, const size_t* offsets, size_t S, uint64_t* out_gt) {
  GM_CHECK(offsets[0] == 0, GM_EINVAL, "pairing_multi_many: offsets[0] = %zu, the first product starts at 0", offsets[0]);
  for (size_t s = 0; s < S; s++)
    GM_CHECK(offsets[s] <= offsets[s + 1], GM_EINVAL, "pairing_multi_many: offsets[%zu] = %zu is above offsets[%zu] = %zu", s, offsets[s], s + 1, offsets[s + 1]);
  const size_t n = offsets[S];
  std::unique_ptr<Bases> b1;
  std::unique_ptr<G2Bases> b2;
  int rc = bases_from_host(C, g1, stride1, n, b1);
  if (!rc) rc = g2_bases_from_host(C, g2, stride2, n, b2);
  if (!rc) {
    std::vector<PairProduct> prods(S);
    for (size_t s = 0; s < S; s++) {
      PairSpan& p = prods[s].s0;
      p.g1 = b1->d;
      p.g2 = b2->d;
      p.first1 = p.first2 = (int64_t)offsets[s];
      p.n = offsets[s + 1] - offsets[s];
    }
    GM_MSM_LOCK(C);
    rc = pairing_products(C, prods.data(), S, out_gt);
  }
  if (b1 && b1->d) (void)gm::raw_free(b1->d);
  if (b2 && b2->d) (void)gm::raw_free(b2->d);
  return rc;
}

// The batched KZG checks (ctx.hpp).  Everything is enqueued on C->stream behind the copies of the caller's arrays; the one wait is
// pairing_products'.
int kzg_checks_run(Context* C, const uint8_t* d_g2, const void* points, size_t stride, const uint64_t* scalars_canonical, const size_t* seg_offsets,
                   size_t nseg, const size_t* check_seg, size_t S, int* ok) {
  if (S == 0) return GM_OK;
  GM_MSM_LOCK(C);
  uint8_t* d_aff = nullptr;
  int rc = g1_lincomb_many_launch(C, points, stride, scalars_canonical, seg_offsets, nseg, &d_aff);
  if (rc) {
    (void)hipStreamSynchronize(C->stream);
    return rc;
  }
  std::vector<PairProduct> prods(S);
  for (size_t s = 0; s < S; s++) {
    const size_t first = check_seg[s], n = check_seg[s + 1] - first;
    if (n == 0) continue;
    PairSpan &a = prods[s].s0, &b = prods[s].s1;
    a.g1 = b.g1 = d_aff;
    a.g2 = b.g2 = d_g2;
    a.first1 = (int64_t)first;  // L against g2
    a.n = 1;
    b.first1 = (int64_t)first + 1;  // the multiples of the proof element against the powers of tau
    b.n = n - 1;
  }
  std::vector<uint64_t> gt(72 * S), one(72);
  rc = pairing_products(C, prods.data(), S, gt.data());
  if (rc) return rc;
  gmh::Fq12::one().to_limbs(one.data());
  for (size_t s = 0; s < S; s++) ok[s] = memcmp(gt.data() + 72 * s, one.data(), GT_BYTES) == 0 ? 1 : 0;
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

// ---- GT element by element: the host side of k_gt_final_exp, k_miller_each, k_gt_check.  Callers hold the MSM lock: the slots
// are the table workspace of the GtModule kernels. ---------------------------------------------------------------------------
constexpr size_t GT_EACH_MAX = (size_t)1 << 20;  // elements per call: 1728 B of slots and 576 B of record each

namespace {
struct GtTmp {  // a device block of one call: nothing in flight reads it once it goes
  Context* C;
  uint8_t* p = nullptr;
  explicit GtTmp(Context* c) : C(c) {}
  ~GtTmp() {
    if (!p) return;
    (void)hipStreamSynchronize(C->stream);
    (void)gm::raw_free(p);
  }
};
}  // namespace

static int gt_slots_ensure(Context* C, size_t n, size_t* blocks) {
  GM_CHECK(n <= GT_EACH_MAX, GM_EINVAL, "gt: %zu elements in one call (at most 2^20)", n);
  *blocks = (n + PAIR_BLOCK - 1) / PAIR_BLOCK;
  return C->pairing.gt_tab.ensure(*blocks * GT_TAB_BLOCK * sizeof(uint32_t));
}

// out[i] = in[i]^((q^12 - 1) / r) over device records (in == out is fine), on C->stream without a wait
int gt_final_exp_launch(Context* C, const uint8_t* in, size_t n, int conj, uint8_t* out) {
  size_t blocks;
  int rc = gt_slots_ensure(C, n, &blocks);
  if (rc || n == 0) return rc;
  C->prof.begin(PROF_REDUCE, C->stream);
  hipLaunchKernelGGL(k_gt_final_exp, dim3((unsigned)blocks), dim3(PAIR_BLOCK), 0, C->stream, in, n, conj, C->pairing.gt_tab.as<uint32_t>(), out);
  C->prof.end(PROF_REDUCE, C->stream);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

// n device records -> n x 72 host limbs (the records are converted in place); ends in a wait
static int gt_to_host(Context* C, uint8_t* d, size_t n, uint64_t* out) {
  const size_t ncoef = n * 12;
  hipLaunchKernelGGL(k_gt_export, dim3((unsigned)((ncoef + 255) / 256)), dim3(256), 0, C->stream, d, ncoef);
  GM_HIP(hipGetLastError());
  GM_HIP(hipMemcpyAsync(out, d, n * GT_BYTES, hipMemcpyDeviceToHost, C->stream));
  GM_HIP(hipStreamSynchronize(C->stream));
  C->prof.collect();
  return GM_OK;
}

// gm_gt_final_exp_many: host elements, no conjugation
int gt_final_exp_many(Context* C, const uint64_t* in, size_t n, uint64_t* out) {
  GM_CHECK(n <= GT_EACH_MAX, GM_EINVAL, "gt_final_exp_many: %zu elements in one call (at most 2^20)", n);
  GM_MSM_LOCK(C);
  GtTmp d(C);
  int rc = gt_from_host(C, in, n, &d.p);
  if (!rc) rc = gt_final_exp_launch(C, d.p, n, 0, d.p);
  if (!rc) rc = gt_to_host(C, d.p, n, out);
  return rc;
}

// out[i] = e(g1[first1 + step1 i], g2[first2 + step2 i]) over packed device records: one k_miller_each, one k_gt_final_exp
int pairing_each_run(Context* C, const uint8_t* d_g1, int64_t first1, int64_t step1, const uint8_t* d_g2, int64_t first2, int64_t step2, size_t n, uint64_t* out_gt) {
  GM_CHECK(n <= GT_EACH_MAX, GM_EINVAL, "pairing_each: %zu pairs in one call (at most 2^20)", n);
  GM_MSM_LOCK(C);
  GtTmp d(C);
  GM_HIP(dev_malloc((void**)&d.p, n * GT_BYTES));
  const PairRange r{d_g1, d_g2, (long long)first1, (long long)step1, (long long)first2, (long long)step2, (unsigned long long)n};
  C->prof.begin(PROF_ACC0, C->stream);
  hipLaunchKernelGGL(k_miller_each, dim3((unsigned)((n + PAIR_BLOCK - 1) / PAIR_BLOCK)), dim3(PAIR_BLOCK), 0, C->stream, r, d.p);
  C->prof.end(PROF_ACC0, C->stream);
  GM_HIP(hipGetLastError());
  int rc = gt_final_exp_launch(C, d.p, n, 1, d.p);
  if (!rc) rc = gt_to_host(C, d.p, n, out_gt);
  return rc;
}
int pairing_each_host(Context* C, const void* g1, size_t stride1, const void* g2, size_t stride2, size_t n, uint64_t* out_gt) {
  std::unique_ptr<Bases> b1;
  std::unique_ptr<G2Bases> b2;
  int rc = bases_from_host(C, g1, stride1, n, b1);
  if (!rc) rc = g2_bases_from_host(C, g2, stride2, n, b2);
  if (!rc) rc = pairing_each_run(C, b1->d, 0, 1, b2->d, 0, 1, n, out_gt);
  if (b1 && b1->d) (void)gm::raw_free(b1->d);
  if (b2 && b2->d) (void)gm::raw_free(b2->d);
  return rc;
}

// k_gt_check over n records on the device (host_form: 72 x u64 of ark-ff's form as copied, else device records); *ok was cleared
// by the entry.  n = 0 passes.
int gt_check_run(Context* C, const uint8_t* d_src, int host_form, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok) {
  if (n == 0) {
    if (first_bad) *first_bad = 0;
    *ok = 1;
    return GM_OK;
  }
  size_t blocks;
  int rc = gt_slots_ensure(C, n, &blocks);
  if (rc) return rc;
  const size_t st_bytes = (n + 15) & ~(size_t)15;  // status bytes, then one u32 per block
  GtTmp rep(C);
  GM_HIP(dev_malloc((void**)&rep.p, st_bytes + blocks * 4));
  uint32_t* d_sum = reinterpret_cast<uint32_t*>(rep.p + st_bytes);
  hipLaunchKernelGGL(k_gt_check, dim3((unsigned)blocks), dim3(PAIR_BLOCK), 0, C->stream, d_src, host_form, n, C->pairing.gt_tab.as<uint32_t>(), rep.p, d_sum);
  GM_HIP(hipGetLastError());
  std::vector<uint32_t> s(blocks);
  GM_HIP(hipMemcpyAsync(s.data(), d_sum, blocks * 4, hipMemcpyDeviceToHost, C->stream));
  if (status_or_null) GM_HIP(hipMemcpyAsync(status_or_null, rep.p, n, hipMemcpyDeviceToHost, C->stream));
  GM_HIP(hipStreamSynchronize(C->stream));
  size_t fb = n;
  for (size_t b = 0; b < blocks; b++)
    if (s[b] != GT_NO_BAD) {
      fb = b * PAIR_BLOCK + s[b];
      break;
    }
  if (first_bad) *first_bad = fb;
  *ok = fb == n ? 1 : 0;
  return GM_OK;
}
int gt_check_host(Context* C, const uint64_t* x, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok) {
  GM_CHECK(n <= GT_EACH_MAX, GM_EINVAL, "gt_check: %zu elements in one call (at most 2^20)", n);
  GM_MSM_LOCK(C);
  GtTmp stage(C);
  if (n) {
    GM_HIP(dev_malloc((void**)&stage.p, n * GT_BYTES));
    GM_HIP(hipMemcpyAsync(stage.p, x, n * GT_BYTES, hipMemcpyHostToDevice, C->stream));
  }
  return gt_check_run(C, stage.p, 1, n, status_or_null, first_bad, ok);
}

// ---- S independent GT multi-exponentiations (k_gt_multi_pow_seg and the levels of k_gt_reduce_seg) ---------------------------------
// The launches on C->stream without a wait: the products of the non-empty term ranges [offsets[s], offsets[s + 1]) end as
// consecutive device records at *d_out (a level buffer of the workspace), in the order of t.idx.  The caller has checked the
// offsets and every term's rows against the two tables, holds the MSM lock and keeps `t` and `terms` until it has waited.
struct GtSegTables {
  std::vector<size_t> idx;
  std::vector<unsigned long long> first;
  std::vector<SegMap> maps;
};
static int gt_multi_pow_seg_launch(Context* C, const uint8_t* d_x, const uint8_t* d_e, const GtTerm* terms, const size_t* offsets, size_t S, GtSegTables& t, uint8_t** d_out) {
  *d_out = nullptr;
  std::vector<unsigned long long> counts;
  for (size_t s = 0; s < S; s++) {
    if (offsets[s + 1] == offsets[s]) continue;
    t.idx.push_back(s);
    t.first.push_back(offsets[s]);
    counts.push_back(offsets[s + 1] - offsets[s]);
  }
  const size_t nseg = t.idx.size(), T = offsets[S];
  if (nseg == 0) return GM_OK;
  std::vector<SegLevel> levels;
  int rc = seg_levels(counts, t.maps, levels);
  if (rc) return rc;
  hipStream_t st = C->stream;
  PairingWorkspace& ws = C->pairing;
  Profiler& pf = C->prof;
  const size_t blocks = (size_t)((levels[0].lanes + PAIR_BLOCK - 1) / PAIR_BLOCK);
  if ((rc = ws.gt_tab.ensure(blocks * GT_TAB_BLOCK * sizeof(uint32_t)))) return rc;
  const size_t first_bytes = nseg * sizeof(unsigned long long), map_bytes = t.maps.size() * sizeof(SegMap), term_bytes = T * sizeof(GtTerm);
  if ((rc = ws.seg_tab.ensure(first_bytes + map_bytes + term_bytes))) return rc;
  for (size_t l = 0; l < levels.size(); l++)  // level l writes its partials into part[l & 1]
    if ((rc = ws.part[l & 1].ensure(levels[l].partials * GT_BYTES))) return rc;
  uint8_t* d_tab = ws.seg_tab.as<uint8_t>();
  GM_HIP(hipMemcpyAsync(d_tab, t.first.data(), first_bytes, hipMemcpyHostToDevice, st));
  GM_HIP(hipMemcpyAsync(d_tab + first_bytes, t.maps.data(), map_bytes, hipMemcpyHostToDevice, st));
  GM_HIP(hipMemcpyAsync(d_tab + first_bytes + map_bytes, terms, term_bytes, hipMemcpyHostToDevice, st));
  const SegMap* d_map = reinterpret_cast<const SegMap*>(d_tab + first_bytes);
  pf.begin(PROF_ACC0, st);
  hipLaunchKernelGGL(k_gt_multi_pow_seg, dim3((unsigned)blocks), dim3(PAIR_BLOCK), 0, st, d_x, d_e, reinterpret_cast<const GtTerm*>(d_tab + first_bytes + map_bytes),
                     reinterpret_cast<const unsigned long long*>(d_tab), d_map, (unsigned)nseg, ws.gt_tab.as<uint32_t>(), ws.part[0].as<uint8_t>());
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
  *d_out = ws.part[cur].as<uint8_t>();
  return GM_OK;
}

// gm_gt_multi_pow_many: host elements and canonical 256-bit exponents, term i raises x[i] to scalars[i]
int gt_multi_pow_many_host(Context* C, const uint64_t* x, const uint64_t* scalars_canonical, const size_t* offsets, size_t S, uint64_t* out_gt) {
  GM_CHECK(offsets[0] == 0, GM_EINVAL, "gt_multi_pow_many: offsets[0] = %zu, the first product starts at 0", offsets[0]);
  for (size_t s = 0; s < S; s++)
    GM_CHECK(offsets[s] <= offsets[s + 1], GM_EINVAL, "gt_multi_pow_many: offsets[%zu] = %zu is above offsets[%zu] = %zu", s, offsets[s], s + 1, offsets[s + 1]);
  const size_t n = offsets[S];
  GM_CHECK(n <= GT_EACH_MAX, GM_EINVAL, "gt_multi_pow_many: %zu terms in one call (at most 2^20)", n);
  GM_CHECK(n == 0 || (x != nullptr && scalars_canonical != nullptr), GM_EINVAL, "gt_multi_pow_many: null pointer");
  for (size_t s = 0; s < S; s++) gmh::Fq12::one().to_limbs(out_gt + 72 * s);
  if (n == 0) return GM_OK;
  GM_MSM_LOCK(C);
  GtTmp d(C);  // the elements, then the exponents
  GM_HIP(dev_malloc((void**)&d.p, n * (GT_BYTES + 32)));
  GM_HIP(hipMemcpyAsync(d.p, x, n * GT_BYTES, hipMemcpyHostToDevice, C->stream));
  GM_HIP(hipMemcpyAsync(d.p + n * GT_BYTES, scalars_canonical, n * 32, hipMemcpyHostToDevice, C->stream));
  hipLaunchKernelGGL(k_gt_import, dim3((unsigned)((n * 12 + 255) / 256)), dim3(256), 0, C->stream, d.p, n * 12);
  GM_HIP(hipGetLastError());
  std::vector<GtTerm> terms(n);
  for (size_t i = 0; i < n; i++) terms[i] = GtTerm{(uint32_t)i, (uint32_t)i};
  GtSegTables t;
  uint8_t* d_out = nullptr;
  int rc = gt_multi_pow_seg_launch(C, d.p, d.p + n * GT_BYTES, terms.data(), offsets, S, t, &d_out);
  const size_t nseg = t.idx.size();
  std::vector<uint64_t> got(nseg * 72);
  if (!rc) rc = gt_to_host(C, d_out, nseg, got.data());  // the one wait
  if (rc) {
    (void)hipStreamSynchronize(C->stream);  // the host arrays are read by their copies until here
    return rc;
  }
  for (size_t s = 0; s < nseg; s++) memcpy(out_gt + 72 * t.idx[s], got.data() + 72 * s, GT_BYTES);
  return GM_OK;
}

int miller_gt_products(Context* C, const PairProduct* prods, size_t P, const uint64_t* exps_canonical, size_t ne, const GtTerm* terms, const size_t* offsets, size_t S,
                       uint64_t* out_gt, size_t* launches) {
  if (S == 0) return GM_OK;
  GM_CHECK(offsets[0] == 0, GM_EINVAL, "miller_gt_products: offsets[0] = %zu", offsets[0]);
  for (size_t p = 0; p < P; p++) GM_CHECK(prods[p].s0.n + prods[p].s1.n > 0, GM_EINVAL, "miller_gt_products: product %zu is empty", p);
  for (size_t s = 0; s < S; s++) {
    GM_CHECK(offsets[s] < offsets[s + 1], GM_EINVAL, "miller_gt_products: segment %zu is empty", s);
    for (size_t i = offsets[s]; i < offsets[s + 1]; i++)
      GM_CHECK(terms[i].x < P && terms[i].e < ne, GM_EINVAL, "miller_gt_products: term %zu names product %u of %zu, exponent %u of %zu", i, terms[i].x, P, terms[i].e, ne);
  }
  GM_CHECK(offsets[S] <= GT_EACH_MAX && P <= GT_EACH_MAX && S <= GT_EACH_MAX, GM_EINVAL, "miller_gt_products: %zu terms over %zu products in %zu segments (at most 2^20 of each)",
           offsets[S], P, S);
  GtTmp res(C);  // the P Miller values, the ne exponents, then the S results: the launch groups share the level buffers of the workspace
  const size_t o_e = P * GT_BYTES, o_out = o_e + ((ne * 32 + 63) & ~(size_t)63);
  GM_HIP(dev_malloc((void**)&res.p, o_out + S * GT_BYTES));
  SegTables pt;
  GtSegTables gt;
  uint8_t* d = nullptr;
  auto enqueue = [&]() -> int {
    GM_HIP(hipMemcpyAsync(res.p + o_e, exps_canonical, ne * 32, hipMemcpyHostToDevice, C->stream));
    int r = miller_products_launch(C, prods, P, pt, &d);
    if (r) return r;
    GM_HIP(hipMemcpyAsync(res.p, d, P * GT_BYTES, hipMemcpyDeviceToDevice, C->stream));
    if ((r = gt_multi_pow_seg_launch(C, res.p, res.p + o_e, terms, offsets, S, gt, &d))) return r;
    if ((r = gt_final_exp_launch(C, d, S, 1, res.p + o_out))) return r;
    return gt_to_host(C, res.p + o_out, S, out_gt);  // the one wait: the tables of `pt` and `gt` are read by their copies until here
  };
  const int rc = enqueue();
  if (rc) (void)hipStreamSynchronize(C->stream);
  else if (launches) *launches += pt.maps.size() / P + gt.maps.size() / S + 2;  // a launch per level of either group, k_gt_final_exp, k_gt_export
  return rc;
}

int gt_checks_run(Context* C, const PairProduct* prods, const uint8_t* d_x, size_t nx, const uint8_t* d_e, size_t ne, const GtTerm* terms, const size_t* offsets, size_t S,
                  uint64_t* out_gt) {
  if (S == 0) return GM_OK;
  GM_CHECK(offsets[0] == 0, GM_EINVAL, "gt_checks: offsets[0] = %zu", offsets[0]);
  for (size_t s = 0; s < S; s++) {
    GM_CHECK(offsets[s] < offsets[s + 1] && prods[s].s0.n + prods[s].s1.n > 0, GM_EINVAL, "gt_checks: check %zu has an empty product", s);
    for (size_t i = offsets[s]; i < offsets[s + 1]; i++)
      GM_CHECK(terms[i].x < nx && terms[i].e < ne, GM_EINVAL, "gt_checks: term %zu names element %u of %zu, exponent %u of %zu", i, terms[i].x, nx, terms[i].e, ne);
  }
  GM_CHECK(offsets[S] <= GT_EACH_MAX && S <= GT_EACH_MAX / 2, GM_EINVAL, "gt_checks: %zu terms in %zu checks (at most 2^20 terms)", offsets[S], S);
  GtTmp res(C);  // the S pairing values, then the S powers: the two launch groups share the level buffers of the workspace
  GM_HIP(dev_malloc((void**)&res.p, 2 * S * GT_BYTES));
  SegTables pt;
  GtSegTables gt;
  uint8_t* d = nullptr;
  int rc = miller_products_launch(C, prods, S, pt, &d);
  if (!rc) rc = gt_final_exp_launch(C, d, S, 1, res.p);
  if (!rc) rc = gt_multi_pow_seg_launch(C, d_x, d_e, terms, offsets, S, gt, &d);
  if (!rc) {
    const hipError_t e = hipMemcpyAsync(res.p + S * GT_BYTES, d, S * GT_BYTES, hipMemcpyDeviceToDevice, C->stream);
    if (e != hipSuccess) rc = gm::hip_fail(e, "hipMemcpyAsync", __FILE__, __LINE__);
  }
  if (!rc) rc = gt_to_host(C, res.p, 2 * S, out_gt);  // the one wait: the tables of `pt` and `gt` are read by their copies until here
  if (rc) (void)hipStreamSynchronize(C->stream);
  return rc;
}

// gm_debug_gt_op
int gt_debug_op(Context* C, int op, const uint64_t* in, size_t n, uint64_t* out) {
  GM_CHECK(op >= GT_OP_FROBENIUS1 && op <= GT_OP_POW_X, GM_EINVAL, "debug_gt_op: unknown op %d", op);
  GM_MSM_LOCK(C);
  size_t blocks;
  int rc = gt_slots_ensure(C, n, &blocks);
  if (rc) return rc;
  GtTmp d(C);
  if ((rc = gt_from_host(C, in, n, &d.p))) return rc;
  hipLaunchKernelGGL(k_gt_debug_op, dim3((unsigned)blocks), dim3(PAIR_BLOCK), 0, C->stream, op, d.p, n, C->pairing.gt_tab.as<uint32_t>(), d.p);
  GM_HIP(hipGetLastError());
  return gt_to_host(C, d.p, n, out);
}

// gm_debug_gt_op2: b_or_null is read by the ops that take a second operand
int gt_debug_op2(Context* C, int op, const uint64_t* a, const uint64_t* b_or_null, size_t n, uint64_t* out) {
  GM_CHECK(op >= 0 && op < GT_OP2_END, GM_EINVAL, "debug_gt_op2: unknown op %d", op);
  GM_CHECK(n <= GT_EACH_MAX, GM_EINVAL, "debug_gt_op2: %zu elements in one call (at most 2^20)", n);
  const bool binary = gt_op2_is_binary(op);
  GM_CHECK(!binary || b_or_null != nullptr, GM_EINVAL, "debug_gt_op2: op %d takes a second operand", op);
  GM_MSM_LOCK(C);
  GtTmp da(C), db(C);
  int rc = gt_from_host(C, a, n, &da.p);
  if (!rc && binary) rc = gt_from_host(C, b_or_null, n, &db.p);
  if (rc) return rc;
  hipLaunchKernelGGL(k_gt_debug_op2, dim3((unsigned)((n + PAIR_BLOCK - 1) / PAIR_BLOCK)), dim3(PAIR_BLOCK), 0, C->stream, op, da.p, db.p, n, da.p);
  GM_HIP(hipGetLastError());
  return gt_to_host(C, da.p, n, out);
}

// gm_debug_miller_step: n records T | Q | P in, n records T' | line out
int miller_debug_step(Context* C, int op, const uint64_t* in, size_t n, uint64_t* out) {
  GM_CHECK(op == MILLER_OP_DBL || op == MILLER_OP_ADD, GM_EINVAL, "debug_miller_step: unknown op %d", op);
  GM_CHECK(n <= GT_EACH_MAX, GM_EINVAL, "debug_miller_step: %zu records in one call (at most 2^20)", n);
  GM_MSM_LOCK(C);
  GtTmp d(C);
  int rc = gt_from_host(C, in, n, &d.p);
  if (rc) return rc;
  hipLaunchKernelGGL(k_miller_debug_step, dim3((unsigned)((n + PAIR_BLOCK - 1) / PAIR_BLOCK)), dim3(PAIR_BLOCK), 0, C->stream, op, d.p, n, d.p);
  GM_HIP(hipGetLastError());
  return gt_to_host(C, d.p, n, out);
}

// gm_debug_miller_each: out[i] = f_{|x|, Q_i}(P_i) as k_miller_each stores it -- no conjugation, no product, no final exponentiation
static int miller_debug_each_run(Context* C, const uint8_t* d_g1, const uint8_t* d_g2, size_t n, uint64_t* out) {
  GM_MSM_LOCK(C);
  GtTmp d(C);
  GM_HIP(dev_malloc((void**)&d.p, n * GT_BYTES));
  const PairRange r{d_g1, d_g2, 0, 1, 0, 1, (unsigned long long)n};
  hipLaunchKernelGGL(k_miller_each, dim3((unsigned)((n + PAIR_BLOCK - 1) / PAIR_BLOCK)), dim3(PAIR_BLOCK), 0, C->stream, r, d.p);
  GM_HIP(hipGetLastError());
  return gt_to_host(C, d.p, n, out);
}
int miller_debug_each(Context* C, const void* g1, size_t stride1, const void* g2, size_t stride2, size_t n, uint64_t* out) {
  GM_CHECK(n <= GT_EACH_MAX, GM_EINVAL, "debug_miller_each: %zu pairs in one call (at most 2^20)", n);
  std::unique_ptr<Bases> b1;
  std::unique_ptr<G2Bases> b2;
  int rc = bases_from_host(C, g1, stride1, n, b1);
  if (!rc) rc = g2_bases_from_host(C, g2, stride2, n, b2);
  if (!rc) rc = miller_debug_each_run(C, b1->d, b2->d, n, out);
  if (b1 && b1->d) (void)gm::raw_free(b1->d);
  if (b2 && b2->d) (void)gm::raw_free(b2->d);
  return rc;
}

}  // namespace gm
