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

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
void pairing_workspace_release(PairingWorkspace& w) {
  for (DevBuf& b : w.part) b.release();
  if (w.host_out) (void)hipHostFree(w.host_out);
  w.host_out = nullptr;
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
