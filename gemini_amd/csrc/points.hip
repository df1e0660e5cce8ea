// Validation and decoding of UNTRUSTED G1 / G2 points on the device (gfx950): canonical coordinates, the curve equation, membership
// of the prime-order subgroup, the two byte framings of gemini_amd/wire.py (G1) and gemini_amd/g2.py (G2) in both directions, the
// powers-of-tau structure of a committer key, and the check entries of what a verifier consumes (a CRS, a verifier key, a proof).
//
// Replaces, for whole keys, what `CanonicalDeserialize::deserialize_with_mode(.., Validate::Yes)` of ark-ec 0.4.2 does per point
// (is_on_curve, then is_in_correct_subgroup_assuming_on_curve); gemini_amd/wire.py states the same on Python integers with [r] P
// as a 255-step ladder, which suits the O(log n) points of a proof and not the 2^26 points of a key.
//
// One lane per point, on the FqE layer and the XYZZ law of g1.cuh / g2.cuh.  The subgroup tests are the endomorphism tests
// ark-bls12-381 uses (Bowe, "Faster subgroup checks for BLS12-381"; Scott, "A note on group membership tests for G1, G2 and GT on
// BLS pairing-friendly curves"), DESIGN.md section "Point validation":
//
//   G1   sigma(P) = (beta x, y) == -[x^2] P     two double-and-adds by |x| = 0xd201000000010000 (Hamming weight 6): 126 doublings,
//                                               5 mixed + 5 full additions, compared projectively (no inversion)
//   G2   psi(Q) = (conj(x) c_x, conj(y) c_y) == [x] Q = -[|x|] Q     one double-and-add by |x| over Fq2
//
// Fq products per point as written (a square counts as a product): G1 check 5 (import + curve) + 126 x 9 + 5 x 10 + 5 x 14 + 3
// = 1262; G2 check 11 (import + curve) + 63 x 24 + 5 x 28 + 11 = 1674; a compressed G1 decode adds the square root, 378 squares + 228 products, a compressed G2 decode
// the one in Fq2, 1221 products (pt_fq2_sqrt).
//
// Reporting: ONE status byte per point (the first check that fails, gemini_hip.h: GM_PT_*), written with ordinary stores, and one
// u32 per block holding the block's first bad lane.  The host reads the block summaries (and the status bytes when the caller asks
// for them); no coordinate crosses back.  Launches go on the library's stream under the MSM lock, as the pairing entries do.
#include <algorithm>
#include <cstring>
#include <vector>

#include "groups.cuh"
#include "host_field.hpp"

namespace gm {

constexpr int PT_BLOCK = 256;      // G1 kernels: amdgpu_waves_per_eu(2, 2) -- 96 / 160 bytes of scratch buy the second wave, 1.27 x against one wave (profiles/point_check.md)
constexpr int PT_G2_BLOCK = 64;    // G2: one wave per SIMD, the whole register file (as k_g2_acc)
constexpr uint32_t PT_NO_BAD = 0xffffffffu;
constexpr uint64_t BLS_X_ABS = 0xd201000000010000ull;  // the curve parameter is x = -BLS_X_ABS

// ---- constants, all in the device form a * 2^390 mod q.  tests/points_ref.py derives the values on Python integers ----------
// beta = 0x5f19672fdf76ce51ba69c6076a0f77eaddb3a93be6f89688de17d813620a00022e01fffffffefffe: of the two non-trivial cube roots of
// unity in Fq the one with (beta x_G, y_G) = -[x^2] G for the generator G (the other root belongs to the eigenvalue x^2 - 1)
__device__ constexpr uint32_t PT_BETA[12] = {0x629d39fcu, 0x845986deu, 0x63a68a8fu, 0x7e276aefu, 0xf512744bu, 0xd3e8af25u,
                                             0xd503c5ccu, 0xe4f473e1u, 0xf47b0197u, 0x0861fd0cu, 0x54d988d2u, 0x0edc53ceu};
// c_x = (1 + u)^-((q - 1) / 3) = (0, PSI_CX1): its real part is zero
__device__ constexpr uint32_t PT_PSI_CX1[12] = {0x9d6270afu, 0x35a57921u, 0x4dad7570u, 0xa084950fu, 0x019e81d8u, 0x9348237bu,
                                                0x1e814cf2u, 0x7f82d7a3u, 0x4ed0ab3fu, 0x42b9aaa9u, 0xe4a65dc8u, 0x0b24be1bu};
// c_y = (1 + u)^-((q - 1) / 2)
__device__ constexpr uint32_t PT_PSI_CY0[12] = {0x57305ee1u, 0x79f31769u, 0x99dc60d7u, 0x2b8c4f87u, 0xe681ea79u, 0x598955e6u,
                                                0xadfc665fu, 0x49c73136u, 0x7fa999feu, 0xdc319445u, 0xdd1a928cu, 0x0345b796u};
__device__ constexpr uint32_t PT_PSI_CY1[12] = {0xa8cf4bcau, 0x400be896u, 0x17779f28u, 0xf31fb077u, 0x102f0baau, 0x0da77cbau,
                                                0x4588ac60u, 0x1ab01a4eu, 0xc3a212d9u, 0x6eea1370u, 0x5c65540du, 0x16bb5a53u};
// 1 / 2 = 2^389 mod q
__device__ constexpr uint32_t PT_HALF[12] = {0x0068ff97u, 0x233b0000u, 0xcda40056u, 0x425c019bu, 0x7441218eu, 0x06ecd3f0u,
                                             0x5b41ee7cu, 0x61361368u, 0x31e252f7u, 0x94f8a2bbu, 0x3f9f4025u, 0x00aef4cbu};
// 2^780 mod q: the product of a canonical INTEGER with it is that integer in the device form
__device__ constexpr uint32_t PT_R2[12] = {0x4510070fu, 0xaec641c3u, 0xa0132243u, 0x6ea66ec3u, 0x1df507afu, 0x5efee07bu,
                                           0xeed21b14u, 0x41442921u, 0x2d32f70au, 0x97900177u, 0x4acd918cu, 0x0f696ee0u};

GM_DEV FqE pt_const(const uint32_t (&c)[12]) {
  FqE r;
#pragma unroll
  for (int i = 0; i < 12; i++) r.l[i] = c[i];
  return r;
}
GM_DEV FqE pt_four() { return fq_dbl(fq_dbl(fqe_one())); }
// a > b as integers
GM_DEV bool pt_raw_gt(const Fq& a, const Fq& b) {
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    uint32_t c;
    (void)__builtin_subc(b.l[i], a.l[i], borrow, &c);
    borrow = c;
  }
  return borrow != 0;
}
// canonical integer < q  <->  device form
GM_DEV FqE pt_from_int(const Fq& v) { return fq_mul(v, pt_const(PT_R2)); }
GM_DEV Fq pt_to_int(const FqE& a) {
  Fq one = Fq::zero();
  one.l[0] = 1u;
  return fq_mul(a, one);
}
// ark-ec's `y > -y` on a fully reduced integer
GM_DEV bool pt_y_is_larger(const Fq& y_int) { return pt_raw_gt(y_int, fp_neg<FqParams>(y_int)); }

// ---- G1 ---------------------------------------------------------------------------------------------------------------------
// [|x|] of an affine / an XYZZ point (neither the identity).  The bits are those of a constant: a scalar branch, the body stated once.
GM_DEV G1Xyzz pt_g1_mul_x(const G1Affine& P) {
  G1Xyzz acc = G1Xyzz::from_affine(P);
#pragma unroll 1
  for (int bit = 62; bit >= 0; bit--) {
    acc = xyzz_dbl(acc);
    if ((BLS_X_ABS >> bit) & 1ull) xyzz_madd(acc, P);
  }
  return acc;
}
GM_DEV G1Xyzz pt_g1_mul_x(const G1Xyzz& T) {
  G1Xyzz acc = T;
#pragma unroll 1
  for (int bit = 62; bit >= 0; bit--) {
    acc = xyzz_dbl(acc);
    if ((BLS_X_ABS >> bit) & 1ull) xyzz_add(acc, T);
  }
  return acc;
}
// P (device form, not the identity record) -> GM_PT_OK / NOT_ON_CURVE / NOT_IN_SUBGROUP
GM_DEV uint8_t pt_g1_status(const G1Affine& P, bool check_curve) {
  if (check_curve) {
    const FqE rhs = fq_add(fq_mul(fq_sqr(P.x), P.x), pt_four());
    if (!(fq_sqr(P.y) == rhs)) return GM_PT_NOT_ON_CURVE;
  }
  const G1Xyzz T = pt_g1_mul_x(P);
  if (T.is_identity()) return GM_PT_NOT_IN_SUBGROUP;  // [x^2] P = O != sigma(P)
  const G1Xyzz U = pt_g1_mul_x(T);
  if (U.is_identity()) return GM_PT_NOT_IN_SUBGROUP;
  // sigma(P) == -U:  beta x ZZ == X  and  y ZZZ == -Y
  const bool same_x = fq_mul(fq_mul(pt_const(PT_BETA), P.x), U.zz) == U.x;
  const bool neg_y = fq_is_zero(fq_add(fq_mul(P.y, U.zzz), U.y));
  return same_x && neg_y ? GM_PT_OK : GM_PT_NOT_IN_SUBGROUP;
}

// ---- G2 ---------------------------------------------------------------------------------------------------------------------
GM_DEV uint8_t pt_g2_status(const G2Affine& Q, bool check_curve) {
  if (check_curve) {
    Fq2 four_xi;  // 4 (1 + u)
    four_xi.c0 = pt_four();
    four_xi.c1 = four_xi.c0;
    if (!fq2_is_zero(fq2_sub(fq2_sqr(Q.y), fq2_add(fq2_mul(fq2_sqr(Q.x), Q.x), four_xi)))) return GM_PT_NOT_ON_CURVE;
  }
  G2Xyzz T = G2Xyzz::from_affine(Q);
#pragma unroll 1
  for (int bit = 62; bit >= 0; bit--) {
    T = g2_dbl(T);
    if ((BLS_X_ABS >> bit) & 1ull) g2_madd(T, Q);
  }
  if (T.is_identity()) return GM_PT_NOT_IN_SUBGROUP;
  // psi(Q) = (conj(x) c_x, conj(y) c_y); conj(x) (0 + c u) = x1 c + x0 c u
  const FqE cx1 = pt_const(PT_PSI_CX1);
  Fq2 px, py, yc, cy;
  px.c0 = fq_mul(Q.x.c1, cx1);
  px.c1 = fq_mul(Q.x.c0, cx1);
  yc.c0 = Q.y.c0;
  yc.c1 = fq_neg_canonical(Q.y.c1);
  cy.c0 = pt_const(PT_PSI_CY0);
  cy.c1 = pt_const(PT_PSI_CY1);
  py = fq2_mul(yc, cy);
  // psi(Q) == -T:  psi_x ZZ == X  and  psi_y ZZZ == -Y
  const bool same_x = fq2_is_zero(fq2_sub(fq2_mul(px, T.zz), T.x));
  const bool neg_y = fq2_is_zero(fq2_add(fq2_mul(py, T.zzz), T.y));
  return same_x && neg_y ? GM_PT_OK : GM_PT_NOT_IN_SUBGROUP;
}

// a^((q + 1) / 4): the square root of a square (q = 3 mod 4).  Bit i of the exponent is bit i + 2 of q + 1, which differs from q in
// bit 2 alone (q = ...1010 1011).  Plain square-and-multiply: 378 squares + 228 products; a 4-bit window would save ~120 of them
// for a table of 16 x 12 VGPRs.
GM_DEV FqE pt_sqrt_candidate(const FqE& a) {
  FqE acc = a;  // the top bit, 380
#pragma unroll 1
  for (int i = 379; i >= 2; i--) {
    acc = fq_sqr(acc);
    if (i == 2 || ((FqParams::MOD[i >> 5] >> (i & 31)) & 1u)) acc = fq_mul(acc, a);
  }
  return acc;
}

GM_DEV uint32_t pt_bswap(uint32_t v) { return __builtin_bswap32(v); }

// ---- G2 from bytes: a square root in Fq2 ---------------------------------------------------------------------------------------
// a^((q - 3) / 4): bit i of the exponent is bit i + 2 of q - 3, which is q with its two low bits cleared -- pt_sqrt_candidate's loop
// without the bit it sets at i = 2.  t = a^((q - 3) / 4) gives both a root candidate t a and its inverse +-t.
GM_DEV FqE pt_pow_q3_4(const FqE& a) {
  FqE acc = a;  // the top bit, 380
#pragma unroll 1
  for (int i = 379; i >= 2; i--) {
    acc = fq_sqr(acc);
    if ((FqParams::MOD[i >> 5] >> (i & 31)) & 1u) acc = fq_mul(acc, a);
  }
  return acc;
}

// A root of a = a0 + a1 u when a is a square of Fq2 = Fq[u] / (u^2 + 1); *is_square says whether it is.  The norm method
// (gemini_amd/g2.py: f2_sqrt states it on integers): n = a0^2 + a1^2 is a square of Fq exactly when a is one of Fq2; with s^2 = n and
// delta = (a0 + s) / 2, exactly one of delta and (a0 - s) / 2 is a square, their product being -(a1 / 2)^2.  t = delta^((q - 3) / 4),
// w = t delta: w^2 = +-delta and 1 / w = +-t with the same sign, so the root is (w, a1 t / 2) or (-a1 t / 2, w).  a1 = 0 takes
// delta = a0 and is always a square.  Two Fq exponentiations and no data-dependent third: 2 + (378 + 228) + 1 + 1 + (378 + 227) + 4 + 2
// = 1221 Fq products (the last two are the square that decides the flag), against ~2 700 for two Fq2 exponentiations.
GM_DEV Fq2 pt_fq2_sqrt(const Fq2& a, bool* is_square) {
  const FqE half = pt_const(PT_HALF);
  FqE delta = a.c0;
  bool norm_ok = true;
  if (!fq_is_zero(a.c1)) {
    const FqE n = fq_add(fq_sqr(a.c0), fq_sqr(a.c1));
    const FqE s = pt_sqrt_candidate(n);
    norm_ok = fq_sqr(s) == n;
    delta = fq_mul(fq_add(a.c0, s), half);
  }
  const FqE t = pt_pow_q3_4(delta);
  const FqE w = fq_mul(t, delta);
  const FqE h = fq_mul(fq_mul(a.c1, t), half);
  Fq2 r;
  if (fq_sqr(w) == delta) {
    r.c0 = w;
    r.c1 = h;
  } else {
    r.c0 = fq_neg_canonical(h);
    r.c1 = w;
  }
  const Fq2 rr = fq2_sqr(r);
  *is_square = norm_ok && rr.c0 == a.c0 && rr.c1 == a.c1;
  return r;
}

// one 48-byte coordinate of either framing -> the integer it spells (flag bits still in place)
GM_DEV Fq pt_load_coord(const uint8_t* p, int zcash) {
  Fq v = fp_load<FqParams>(p);
  if (zcash) {  // big-endian: limb k is word 11 - k, byte-swapped
    const Fq t = v;
#pragma unroll
    for (int k = 0; k < 12; k++) v.l[k] = pt_bswap(t.l[11 - k]);
  }
  return v;
}
GM_DEV void pt_store_coord(uint8_t* p, const Fq& v, int zcash) {
  Fq o = v;
  if (zcash) {
#pragma unroll
    for (int k = 0; k < 12; k++) o.l[k] = pt_bswap(v.l[11 - k]);
  }
  fp_store<FqParams>(p, o);
}

// gm_debug_fq2_sqrt: pt_fq2_sqrt on ark-ff Montgomery elements, one lane each
__global__ __launch_bounds__(PT_G2_BLOCK) void k_fq2_sqrt(const uint8_t* __restrict__ src, size_t n, uint8_t* __restrict__ root, uint8_t* __restrict__ is_square) {
  const size_t i = (size_t)blockIdx.x * PT_G2_BLOCK + threadIdx.x;
  if (i >= n) return;
  Fq2 a = fq2_load(src + i * 96);
  a.c0 = fqe_import(a.c0);
  a.c1 = fqe_import(a.c1);
  bool square;
  Fq2 r = pt_fq2_sqrt(a, &square);
  r.c0 = fqe_export(r.c0);
  r.c1 = fqe_export(r.c1);
  fq2_store(root + i * 96, r);
  is_square[i] = square ? 1 : 0;
}

// psi on XYZZ coordinates: conjugation is a field automorphism, so (X, Y, ZZ, ZZZ) -> (conj(X) c_x, conj(Y) c_y, conj(ZZ), conj(ZZZ))
// is psi of the point they stand for.  The constants are those of pt_g2_status; the identity maps to itself.
GM_DEV Fq2 pt_fq2_conj(const Fq2& a) {
  Fq2 r;
  r.c0 = a.c0;
  r.c1 = fq_neg_canonical(a.c1);
  return r;
}
GM_DEV G2Xyzz pt_g2_psi(const G2Xyzz& T) {
  const FqE cx1 = pt_const(PT_PSI_CX1);
  Fq2 cy;
  cy.c0 = pt_const(PT_PSI_CY0);
  cy.c1 = pt_const(PT_PSI_CY1);
  G2Xyzz r;
  r.x.c0 = fq_mul(T.x.c1, cx1);  // conj(x) (0 + c u) = x1 c + x0 c u
  r.x.c1 = fq_mul(T.x.c0, cx1);
  r.y = fq2_mul(pt_fq2_conj(T.y), cy);
  r.zz = pt_fq2_conj(T.zz);
  r.zzz = pt_fq2_conj(T.zzz);
  return r;
}
// [x^2 - x - 1] P + [x - 1] psi(P) + psi^2([2] P) (Budroni, Pintore: "Efficient hash maps to G2 on BLS curves"), x = -|x|: with
// U = [|x| + 1] P it is [|x|] U - P - psi(U) + psi^2([2] P) -- two |x| ladders.  U waits in the lane's slot between the five
// additions of the second ladder.  k_pt_cand_clear<PtG2> still spills: 560 bytes of scratch a lane at one wave per SIMD -- the accumulator,
// P and a full XYZZ + XYZZ addition over Fq2 are more than 512 registers, as in k_g2_reduce (profiles/keygen_kernel_resources.txt).
GM_DEV G2Xyzz pt_g2_clear(const G2Affine& P, uint8_t* slot) {
  G2Xyzz acc = G2Xyzz::from_affine(P);
#pragma unroll 1
  for (int bit = 62; bit >= 0; bit--) {
    acc = g2_dbl(acc);
    if ((BLS_X_ABS >> bit) & 1ull) g2_madd(acc, P);
  }
  g2_madd(acc, P);
  g2_store_xyzz(slot, acc);  // U
#pragma unroll 1
  for (int bit = 62; bit >= 0; bit--) {
    acc = g2_dbl(acc);
    if ((BLS_X_ABS >> bit) & 1ull) g2_add(acc, g2_load_xyzz(slot));
  }
  g2_madd(acc, g2_neg_affine(P));
  G2Xyzz pu = pt_g2_psi(g2_load_xyzz(slot));
  pu.y = fq2_neg_canonical(pu.y);
  g2_add(acc, pu);
  g2_add(acc, pt_g2_psi(pt_g2_psi(g2_dbl_affine(P))));
  return acc;
}

// ---- the two groups ------------------------------------------------------------------------------------------------------------
// What the kernels and the entries below need to know of a group beyond groups.cuh, by name: the launch shape of the point
// kernels and the functions above that differ between the groups; the only arithmetic stated here is the curve's right-hand
// side.  The host members are the two figures candidates_run needs.
struct PtG1 : GrpG1 {
  static constexpr int BLOCK = PT_BLOCK, WAVES = 2;
  static GM_DEV El curve_rhs(const El& x) { return fq_add(fq_mul(fq_sqr(x), x), pt_four()); }  // x^3 + 4
  static GM_DEV El sqrt(const El& a, bool* is_square) {
    const El r = pt_sqrt_candidate(a);
    *is_square = fq_sqr(r) == a;
    return r;
  }
  static GM_DEV uint8_t status(const Affine& P, bool check_curve) { return pt_g1_status(P, check_curve); }
  static GM_DEV Xyzz clear(const Affine& P, uint8_t*) {  // [1 - x] P = [|x|] P + P
    Xyzz T = pt_g1_mul_x(P);
    xyzz_madd(T, P);
    return T;
  }
  static size_t cand_piece(size_t want) { return want / 2 * 5 + 64; }  // candidates to read for `want` points: a little over 1 / p
};
struct PtG2 : GrpG2 {
  static constexpr int BLOCK = PT_G2_BLOCK, WAVES = 1;
  static GM_DEV El curve_rhs(const El& x) {  // x^3 + 4 (1 + u)
    El r = fq2_mul(fq2_sqr(x), x);
    r.c0 = fq_add(r.c0, pt_four());
    r.c1 = fq_add(r.c1, pt_four());
    return r;
  }
  static GM_DEV El sqrt(const El& a, bool* is_square) { return pt_fq2_sqrt(a, is_square); }
  static GM_DEV uint8_t status(const Affine& P, bool check_curve) { return pt_g2_status(P, check_curve); }
  static GM_DEV Xyzz clear(const Affine& P, uint8_t* slot) { return pt_g2_clear(P, slot); }
  static size_t cand_piece(size_t want) { return want / 4 * 13 + 64; }
};

// NC canonical integers < q  <->  an element in the device form
template <class G>
GM_DEV typename G::El pt_el_from_int(const Fq* v) {
  FqE c[G::NC];
#pragma unroll
  for (int e = 0; e < G::NC; e++) c[e] = pt_from_int(v[e]);
  return G::el(c);
}
template <class G>
GM_DEV void pt_el_to_int(const typename G::El& a, Fq* v) {
  G::parts(a, v);
#pragma unroll
  for (int e = 0; e < G::NC; e++) v[e] = pt_to_int(v[e]);
}
// y > -y in ark-ff's order of an extension, on the NC integers of y: the top non-zero component decides, c0 when all above it are
// zero (c = -c only for c = 0).  ge_q[e] (nullptr: all fully reduced) says that component e is >= q, which reads as larger than its negative.
template <int NC>
GM_DEV bool pt_is_larger(const Fq* y, const bool* ge_q = nullptr) {
  bool r = (ge_q && ge_q[0]) || pt_y_is_larger(y[0]);
#pragma unroll
  for (int e = 1; e < NC; e++) r = (ge_q && ge_q[e]) || (y[e].is_zero() ? r : pt_y_is_larger(y[e]));
  return r;
}

// ---- reporting: the status byte of the lane, and the block's first bad lane (every lane of the block arrives here) -------------
template <int BLOCK>
GM_DEV void pt_report(size_t i, size_t n, uint8_t st, uint8_t* __restrict__ status, uint32_t* __restrict__ summary) {
  __shared__ uint32_t first[BLOCK / 64];
  const bool bad = i < n && st != GM_PT_OK;
  if (i < n) status[i] = st;
  const unsigned long long m = __ballot(bad);
  if ((threadIdx.x & 63u) == 0) first[threadIdx.x >> 6] = m ? (threadIdx.x + (uint32_t)__ffsll((long long)m) - 1u) : PT_NO_BAD;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t f = PT_NO_BAD;
    for (unsigned w = 0; w < blockDim.x / 64; w++) f = first[w] < f ? first[w] : f;
    summary[blockIdx.x] = f;
  }
}

// The five kernels below are stated once for both groups.  They work on the 2 NC components of a point, c[] = x.c0 .. , y.c0 .. ;
// G1 runs them at two waves per SIMD and blocks of 256, G2 at one wave and blocks of 64.
//
// k_pt_check.  host_form != 0: records as gm_g1_bases_register / gm_g2_bases_register take them (ark-ff Montgomery limbs, stride >= AFF_BYTES, the
// infinity byte behind the coordinates when the stride has room); 0: packed device records, canonical by construction
template <class G>
__global__ __launch_bounds__(G::BLOCK) __attribute__((amdgpu_waves_per_eu(G::WAVES, G::WAVES))) void k_pt_check(const uint8_t* __restrict__ src, size_t stride, int host_form, size_t n, uint8_t* __restrict__ status, uint32_t* __restrict__ summary) {
  constexpr int NC = G::NC;
  const size_t i = (size_t)blockIdx.x * G::BLOCK + threadIdx.x;
  uint8_t st = GM_PT_OK;
  if (i < n) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src + i * stride);
    FqE c[2 * NC];
    uint32_t any = 0;
    bool canonical = true;
#pragma unroll
    for (int e = 0; e < 2 * NC; e++) {
#pragma unroll
      for (int k = 0; k < 12; k++) {
        c[e].l[k] = s[12 * e + k];
        any |= c[e].l[k];
      }
      canonical = canonical && !pt_raw_ge_q(c[e]);
    }
    const bool inf = (host_form && stride > G::AFF_BYTES && src[i * stride + G::AFF_BYTES] != 0) || any == 0;  // what k_pack_bases reads as the identity
    if (!inf) {
      if (host_form && !canonical) {
        st = GM_PT_NONCANONICAL;
      } else {
        if (host_form) {
#pragma unroll
          for (int e = 0; e < 2 * NC; e++) c[e] = fqe_import(c[e]);
        }
        typename G::Affine P;
        P.x = G::el(c);
        P.y = G::el(c + NC);
        st = G::status(P, true);
      }
    }
  }
  pt_report<G::BLOCK>(i, n, st, status, summary);
}

// 48 NC- / 96 NC-byte encodings -> packed device records (the layout k_pack_bases produces; the identity and every rejected point
// are the all-zero record).  Acceptance and the order of the checks are those of wire.g1_deserialize(.., strict = True, validate)
// and of gemini_amd/g2.py: deserialize(.., strict = True, validate).  Component e sits in wire slot e (arkworks: c0 | c1,
// little-endian) or e ^ (NC - 1) (zcash: c1 | c0, big-endian).
template <class G>
__global__ __launch_bounds__(G::BLOCK) __attribute__((amdgpu_waves_per_eu(G::WAVES, G::WAVES))) void k_pt_decode(const uint8_t* __restrict__ bytes, size_t n, int compressed, int zcash, int validate, uint8_t* __restrict__ dst, uint8_t* __restrict__ status,
                         uint32_t* __restrict__ summary) {
  constexpr int NC = G::NC;
  const size_t i = (size_t)blockIdx.x * G::BLOCK + threadIdx.x;
  uint8_t st = GM_PT_OK;
  if (i < n) {
    const int k = compressed ? NC : 2 * NC;
    const uint8_t* src = bytes + i * (size_t)(48 * k);
    Fq c[2 * NC];
#pragma unroll
    for (int e = 0; e < 2 * NC; e++) c[e] = e < k ? pt_load_coord(src + 48 * (zcash ? e ^ (NC - 1) : e), zcash) : Fq::zero();
    uint32_t &x_top = c[NC - 1].l[11], &y_top = c[2 * NC - 1].l[11];
    bool inf, larger;
    if (zcash) {  // flags in the three top bits of the first byte = the top bits of x's last component
      const uint32_t f = x_top >> 29;
      x_top &= 0x1fffffffu;
      inf = (f >> 1) & 1u;
      larger = f & 1u;
      if ((int)(f >> 2) != (compressed ? 1 : 0) || (larger && (!compressed || inf))) st = GM_PT_BAD_ENCODING;
    } else {  // flags in the two top bits of the last byte = the top bits of the last coordinate's last component
      const uint32_t f = (compressed ? x_top : y_top) >> 30;
      if (compressed) x_top &= 0x3fffffffu;
      else y_top &= 0x3fffffffu;
      inf = f == 1;
      larger = f == 2;
      if (f == 3) st = GM_PT_BAD_ENCODING;
    }
    typename G::Affine P;
    P.x = G::zero();
    P.y = G::zero();
    if (st == GM_PT_OK) {
      bool x_ge = false;
#pragma unroll
      for (int e = 0; e < NC; e++) x_ge = x_ge || pt_raw_ge_q(c[e]);
      if (inf) {
        bool zero = true;
#pragma unroll
        for (int e = 0; e < 2 * NC; e++) zero = zero && c[e].is_zero();
        if (!zero) st = GM_PT_BAD_ENCODING;  // infinity with non-zero coordinates
      } else if (compressed) {
        if (x_ge) {
          st = GM_PT_NONCANONICAL;
        } else {
          P.x = pt_el_from_int<G>(c);
          bool square;
          P.y = G::sqrt(G::curve_rhs(P.x), &square);
          if (!square) {
            st = GM_PT_NOT_ON_CURVE;  // x^3 + b is no square
          } else {
            Fq y[NC];
            pt_el_to_int<G>(P.y, y);
            if (pt_is_larger<NC>(y) != larger) P.y = G::neg(P.y);
            if (validate) st = G::status(P, false);  // on the curve by construction
          }
        }
      } else {
        bool ge[NC], y_ge = false;
#pragma unroll
        for (int e = 0; e < NC; e++) {
          ge[e] = pt_raw_ge_q(c[NC + e]);
          y_ge = y_ge || ge[e];
        }
        // wire.py and g2.py compare the sign flag BEFORE the canonical check, against (-y) mod q
        if (!zcash && pt_is_larger<NC>(c + NC, ge) != larger) {
          st = GM_PT_BAD_ENCODING;
        } else if (x_ge || y_ge) {
          st = GM_PT_NONCANONICAL;
        } else {
          P.x = pt_el_from_int<G>(c);
          P.y = pt_el_from_int<G>(c + NC);
          if (validate) st = G::status(P, true);
        }
      }
    }
    if (st != GM_PT_OK) {
      P.x = G::zero();
      P.y = G::zero();
    }
    G::store_affine(dst + i * G::AFF_BYTES, P);
  }
  pt_report<G::BLOCK>(i, n, st, status, summary);
}

// ---- resident records -> bytes: one Montgomery exit per coordinate and the y > -y compare, no inversion (the bases are affine) ------
constexpr int PT_ENC_BLOCK = 256;
template <class G>
__global__ __launch_bounds__(PT_ENC_BLOCK) void k_pt_encode(const uint8_t* __restrict__ src, size_t n, int compressed, int zcash, uint8_t* __restrict__ out) {
  constexpr int NC = G::NC;
  const size_t i = (size_t)blockIdx.x * PT_ENC_BLOCK + threadIdx.x;
  if (i >= n) return;
  const typename G::Affine P = G::load_affine(src + i * G::AFF_BYTES);
  const bool inf = P.is_identity();
  Fq c[2 * NC];  // 0 for the identity
  pt_el_to_int<G>(P.x, c);
  pt_el_to_int<G>(P.y, c + NC);
  const bool larger = !inf && pt_is_larger<NC>(c + NC);
  uint32_t &x_top = c[NC - 1].l[11], &y_top = c[2 * NC - 1].l[11];
  if (zcash) {  // the first byte is the top of x's last component
    x_top |= (compressed ? 0x80000000u : 0u) | (inf ? 0x40000000u : 0u) | (compressed && larger ? 0x20000000u : 0u);
  } else {  // the last byte is the top of the last coordinate's last component
    const uint32_t f = (inf ? 0x40000000u : 0u) | (larger ? 0x80000000u : 0u);
    if (compressed) x_top |= f;
    else y_top |= f;
  }
  const int k = compressed ? NC : 2 * NC;
  uint8_t* o = out + i * (size_t)(48 * k);
#pragma unroll
  for (int e = 0; e < 2 * NC; e++)
    if (e < k) pt_store_coord(o + 48 * (zcash ? e ^ (NC - 1) : e), c[e], zcash);
}

// ---- points without a known logarithm: candidates -> cofactor-cleared points (gm_g1_bases_from_candidates, gm_g2_...) -----------
// A candidate is an x (and one bit that chooses between y and -y); it survives when its coordinates are < q, x^3 + b is a square and
// the cleared point is not the identity (include/gemini_hip.h has the format; tests/keygen_ref.py states all of it on integers).
// Three launches, dense lanes in each, the host compacting in between from status bytes (a wave runs as long as its slowest lane:
// one kernel from bytes to cleared point took 2.4 x as long, every wave paying root AND clearing for its few survivors):
//   root    one lane per candidate: rules 1 and 2, the curve point (affine) into slot i, one status byte
//   clear   one lane per candidate ON THE CURVE, in order and only as many as the key still needs: the cleared point (XYZZ) over the
//           slot, one status byte (rule 3)
//   gather  the survivors normalised into the key, eight to an inversion
// Fq products: root G1 5 + 606, G2 9 + 1 221; clearing G1 63 x 9 + 6 x 10 = 627, G2 2 x 63 x 24 + 6 x 28 (mixed) + 5 x 37 (full) +
// 135 (the tail: one mixed and two full additions, psi three times, [2] P) = 3 512.
constexpr uint8_t PT_CAND_OK = 0, PT_CAND_GE_Q = 1, PT_CAND_NO_SQUARE = 2, PT_CAND_IDENTITY = 3;
constexpr uint32_t PT_CAND_X_MASK = 0x1fffffffu;  // bits 381 and 382 are ignored, bit 383 (of the last component) is the choice of y

template <class G>
__global__ __launch_bounds__(G::BLOCK) __attribute__((amdgpu_waves_per_eu(G::WAVES, G::WAVES))) void k_pt_cand_root(const uint8_t* __restrict__ cand, size_t m, uint8_t* __restrict__ slots, uint8_t* __restrict__ status) {
  constexpr int NC = G::NC;
  const size_t i = (size_t)blockIdx.x * G::BLOCK + threadIdx.x;
  if (i >= m) return;
  Fq c[NC];
#pragma unroll
  for (int e = 0; e < NC; e++) c[e] = fp_load<FqParams>(cand + (i * NC + e) * 48);
  const bool larger = (c[NC - 1].l[11] >> 31) != 0;
  bool ge = false;
#pragma unroll
  for (int e = 0; e < NC; e++) {
    c[e].l[11] &= PT_CAND_X_MASK;
    ge = ge || pt_raw_ge_q(c[e]);
  }
  uint8_t st = PT_CAND_OK;
  if (ge) {
    st = PT_CAND_GE_Q;
  } else {
    typename G::Affine P;
    P.x = pt_el_from_int<G>(c);
    bool square;
    P.y = G::sqrt(G::curve_rhs(P.x), &square);
    if (!square) {
      st = PT_CAND_NO_SQUARE;
    } else {
      Fq y[NC];
      pt_el_to_int<G>(P.y, y);
      if (pt_is_larger<NC>(y) != larger) P.y = G::neg(P.y);
      G::store_affine(slots + i * G::XYZZ_BYTES, P);
    }
  }
  status[i] = st;
}
// lane j clears the curve point in slot idx[j] (the affine record at its start); G2's clearing uses the slot on the way, and the
// slot takes the result
template <class G>
__global__ __launch_bounds__(G::BLOCK) __attribute__((amdgpu_waves_per_eu(G::WAVES, G::WAVES))) void k_pt_cand_clear(uint8_t* slots, const uint32_t* __restrict__ idx, size_t n, uint8_t* __restrict__ status) {
  const size_t j = (size_t)blockIdx.x * G::BLOCK + threadIdx.x;
  if (j >= n) return;
  uint8_t* slot = slots + (size_t)idx[j] * G::XYZZ_BYTES;
  const typename G::Affine P = G::load_affine(slot);
  const typename G::Xyzz R = G::clear(P, slot);
  G::store_xyzz(slot, R);
  status[j] = R.is_identity() ? PT_CAND_IDENTITY : PT_CAND_OK;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
namespace {

// status bytes (n, padded to 16) followed by one u32 per block
struct Report {
  DevTmp buf;
  size_t n = 0, blocks = 0;
  unsigned block = 0;
  uint8_t* status() const { return static_cast<uint8_t*>(buf.p); }
  uint32_t* summary() const { return reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(buf.p) + ((n + 15) & ~(size_t)15)); }
  int alloc(size_t n_, unsigned block_) {
    n = n_;
    block = block_;
    blocks = (n + block - 1) / block;
    GM_CHECK(blocks <= 0x7fffffffu, GM_EINVAL, "point check: %zu points in one call", n);
    GM_HIP(dev_malloc(&buf.p, ((n + 15) & ~(size_t)15) + blocks * 4));
    return GM_OK;
  }
  // after the kernel: the block summaries (and the status bytes on request) -> first_bad / ok
  int read(Context* C, uint8_t* status_or_null, size_t* first_bad, int* ok) {
    std::vector<uint32_t> s(blocks);
    GM_HIP(hipGetLastError());
    GM_HIP(hipMemcpyAsync(s.data(), summary(), blocks * 4, hipMemcpyDeviceToHost, C->stream));
    if (status_or_null) GM_HIP(hipMemcpyAsync(status_or_null, status(), n, hipMemcpyDeviceToHost, C->stream));
    GM_HIP(hipStreamSynchronize(C->stream));
    size_t fb = n;
    for (size_t b = 0; b < blocks; b++)
      if (s[b] != PT_NO_BAD) {
        fb = b * block + s[b];
        break;
      }
    if (first_bad) *first_bad = fb;
    *ok = fb == n ? 1 : 0;
    return GM_OK;
  }
};

// G: PtG1 / PtG2.  d_src: device memory, `stride` bytes per record.  Caller holds the MSM lock.
template <class G>
int check_run(Context* C, const uint8_t* d_src, size_t stride, int host_form, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok) {
  if (n == 0) {
    if (first_bad) *first_bad = 0;
    *ok = 1;
    return GM_OK;
  }
  Report rep;
  int rc = rep.alloc(n, G::BLOCK);
  if (rc) return rc;
  hipLaunchKernelGGL(k_pt_check<G>, dim3((unsigned)rep.blocks), dim3(G::BLOCK), 0, C->stream, d_src, stride, host_form, n, rep.status(), rep.summary());
  return rep.read(C, status_or_null, first_bad, ok);
}

template <class G>
int check_host(const void* points, size_t stride, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok) {
  if (ok) *ok = 0;  // every check entry fails closed: whatever the return value, *ok is 1 only after a pass that accepted every point
  GM_CTX();
  GM_CHECK(ok != nullptr && (points != nullptr || n == 0), GM_EINVAL, "%s_check: null pointer", G::NAME);
  GM_CHECK(stride >= G::AFF_BYTES && stride % 8 == 0, GM_EINVAL, "%s_check: stride %zu must be >= %zu and a multiple of 8", G::NAME, stride, G::AFF_BYTES);
  GM_CHECK(n <= SIZE_MAX / stride, GM_EINVAL, "%s_check: %zu records of %zu bytes do not fit a size_t", G::NAME, n, stride);
  GM_MSM_LOCK(C);
  DevTmp stage;
  if (n) {
    GM_HIP(dev_malloc(&stage.p, n * stride));
    GM_HIP(hipMemcpyAsync(stage.p, points, n * stride, hipMemcpyHostToDevice, C->stream));
  }
  return check_run<G>(C, static_cast<const uint8_t*>(stage.p), stride, 1, n, status_or_null, first_bad, ok);
}

// ---- the group elements of a proof: Jacobian, any representative -> host records for ONE check launch per group ----------------
bool limbs_lt_q(const uint64_t* p) {
  uint64_t t[6];
  return gmh::sub_n<6>(t, p, gmh::FqP::MOD) != 0;
}
// a coordinate >= q has no value to normalise: its record gets all-ones limbs, which k_pt_check reports as NONCANONICAL
void proof_g1_record(const uint64_t jac[18], uint64_t out[12]) {
  for (int c = 0; c < 3; c++)
    if (!limbs_lt_q(jac + 6 * c)) {
      memset(out, 0xff, 96);
      return;
    }
  memset(out, 0, 96);
  const gmh::G1 a = gmh::G1::from_limbs(jac).normalized();
  if (a.is_identity()) return;
  a.x.to_limbs(out);
  a.y.to_limbs(out + 6);
}
void proof_g2_record(const uint64_t jac[36], uint64_t out[24]) {
  for (int c = 0; c < 6; c++)
    if (!limbs_lt_q(jac + 6 * c)) {
      memset(out, 0xff, 192);
      return;
    }
  memset(out, 0, 192);
  const gmh::G2 a = gmh::G2::from_limbs(jac).normalized();
  if (a.is_identity()) return;
  a.x.to_limbs(out);
  a.y.to_limbs(out + 12);
}
// host records of both groups (either may be empty) -> the first bad index of each; one launch per non-empty group.  Caller holds the lock
int check_records(Context* C, const std::vector<uint64_t>& r1, const std::vector<uint64_t>& r2, size_t* bad1, size_t* bad2, int* ok) {
  const size_t n1 = r1.size() / 12, n2 = r2.size() / 24;
  DevTmp stage;
  if (n1 + n2) {
    GM_HIP(dev_malloc(&stage.p, n1 * 96 + n2 * 192));
    if (n1) GM_HIP(hipMemcpyAsync(stage.p, r1.data(), n1 * 96, hipMemcpyHostToDevice, C->stream));
    if (n2) GM_HIP(hipMemcpyAsync(static_cast<uint8_t*>(stage.p) + n1 * 96, r2.data(), n2 * 192, hipMemcpyHostToDevice, C->stream));
  }
  int ok1 = 0, ok2 = 0;
  int rc = check_run<PtG1>(C, static_cast<const uint8_t*>(stage.p), 96, 1, n1, nullptr, bad1, &ok1);
  if (!rc) rc = check_run<PtG2>(C, static_cast<const uint8_t*>(stage.p) + n1 * 96, 192, 1, n2, nullptr, bad2, &ok2);
  if (rc) return rc;
  *ok = ok1 && ok2;
  return GM_OK;
}
// the G1 elements of a proof, in the order the header lists them
int proof_check(const std::vector<const uint64_t*>& g1, size_t* first_bad, int* ok) {
  GM_CTX();
  std::vector<uint64_t> r1(g1.size() * 12), none;
  for (size_t i = 0; i < g1.size(); i++) proof_g1_record(g1[i], r1.data() + 12 * i);
  GM_MSM_LOCK(C);
  size_t b1 = 0, b2 = 0;
  int rc = check_records(C, r1, none, &b1, &b2, ok);
  if (rc) return rc;
  if (first_bad) *first_bad = b1;
  return GM_OK;
}

// bases[offset .. offset + n) of either group -> bytes on the host
template <class G>
int encode_run(Context* C, const uint8_t* d_src, size_t n, int compressed, int encoding, uint8_t* out) {
  if (n == 0) return GM_OK;
  const size_t sz = G::AFF_BYTES / (compressed ? 2 : 1);
  const size_t blocks = (n + PT_ENC_BLOCK - 1) / PT_ENC_BLOCK;
  GM_CHECK(blocks <= 0x7fffffffu && n <= SIZE_MAX / sz, GM_EINVAL, "%s_bases_to_bytes: %zu points in one call", G::NAME, n);
  DevTmp tmp;
  GM_HIP(dev_malloc(&tmp.p, n * sz));
  hipLaunchKernelGGL(k_pt_encode<G>, dim3((unsigned)blocks), dim3(PT_ENC_BLOCK), 0, C->stream, d_src, n, compressed ? 1 : 0, encoding, static_cast<uint8_t*>(tmp.p));
  GM_HIP(hipGetLastError());
  GM_HIP(hipMemcpyAsync(out, tmp.p, n * sz, hipMemcpyDeviceToHost, C->stream));
  GM_HIP(hipStreamSynchronize(C->stream));
  return GM_OK;
}

// The first n survivors of m candidates, normalised, into a new array of n records (*d_out; nullptr on a shortfall).  A candidate
// is on the curve with probability p = (q / 2^381)^k / 2 -- k = 1, 2 coordinates below q = 0.8125 x 2^381, half of all x give a
// square -- = 0.406 for G1 and 0.330 for G2.  The stream is read in pieces of (n - have) x 5 / 2 (G1), x 13 / 4 (G2) + 64 candidates,
// a little over 1 / p each, so that one piece is expected to finish the key and few roots are taken for nothing; and of at most 2^20
// (the slots of a piece: 192 / 384 MB).  Of a piece's curve points only as many as the key still needs are cleared, in order; one
// that clears to the identity (rule 3) makes the loop take the next ones.  *found counts the survivors among the candidates [0, *used).
constexpr size_t PT_CAND_PIECE = (size_t)1 << 20;
template <class G>
int candidates_run(Context* C, const uint8_t* cand, size_t m, size_t n, uint8_t** d_out, size_t* used, size_t* found) {
  const size_t csz = 48 * G::NC, xsz = G::XYZZ_BYTES, asz = G::AFF_BYTES;
  const unsigned block = G::BLOCK;
  *d_out = nullptr;
  *used = m;
  *found = 0;
  GM_MSM_LOCK(C);
  const size_t cap = std::min({m, PT_CAND_PIECE, G::cand_piece(n)});
  DevTmp out, stage, slots_, st_, idx_;
  GM_HIP(dev_malloc(&out.p, n * asz));
  GM_HIP(dev_malloc(&stage.p, cap * csz));
  GM_HIP(dev_malloc(&slots_.p, cap * xsz));
  GM_HIP(dev_malloc(&st_.p, cap));
  GM_HIP(dev_malloc(&idx_.p, cap * 4));
  uint8_t *slots = static_cast<uint8_t*>(slots_.p), *st = static_cast<uint8_t*>(st_.p);
  uint32_t* idx = static_cast<uint32_t*>(idx_.p);
  std::vector<uint8_t> h_st(cap);
  std::vector<uint32_t> on_curve, good;
  size_t pos = 0, have = 0;
  while (have < n && pos < m) {
    const size_t k = std::min({m - pos, cap, G::cand_piece(n - have)});
    GM_HIP(hipMemcpyAsync(stage.p, cand + pos * csz, k * csz, hipMemcpyHostToDevice, C->stream));
    hipLaunchKernelGGL(k_pt_cand_root<G>, dim3((unsigned)((k + block - 1) / block)), dim3(block), 0, C->stream, static_cast<const uint8_t*>(stage.p), k, slots, st);
    GM_HIP(hipGetLastError());
    GM_HIP(hipMemcpyAsync(h_st.data(), st, k, hipMemcpyDeviceToHost, C->stream));
    GM_HIP(hipStreamSynchronize(C->stream));
    on_curve.clear();
    for (size_t j = 0; j < k; j++)
      if (h_st[j] == PT_CAND_OK) on_curve.push_back((uint32_t)j);
    size_t end = k;  // candidates of this piece that count as read
    for (size_t at = 0; at < on_curve.size() && have < n;) {
      const size_t c = std::min(on_curve.size() - at, n - have);
      GM_HIP(hipMemcpyAsync(idx, on_curve.data() + at, c * 4, hipMemcpyHostToDevice, C->stream));
      hipLaunchKernelGGL(k_pt_cand_clear<G>, dim3((unsigned)((c + block - 1) / block)), dim3(block), 0, C->stream, slots, idx, c, st);
      GM_HIP(hipGetLastError());
      GM_HIP(hipMemcpyAsync(h_st.data(), st, c, hipMemcpyDeviceToHost, C->stream));
      GM_HIP(hipStreamSynchronize(C->stream));
      good.clear();
      for (size_t j = 0; j < c; j++)
        if (h_st[j] == PT_CAND_OK) good.push_back(on_curve[at + j]);
      if (!good.empty()) {
        uint8_t* dst = static_cast<uint8_t*>(out.p) + have * asz;
        if (good.size() != c) GM_HIP(hipMemcpyAsync(idx, good.data(), good.size() * 4, hipMemcpyHostToDevice, C->stream));  // else idx holds them already
        int rc = normalise_launch<typename G::Grp>(C->stream, slots, idx, good.size(), dst);  // the slots into the key: apart
        if (rc) return rc;
        GM_HIP(hipStreamSynchronize(C->stream));  // idx, the slots and the host lists are rewritten from here on
        have += good.size();
        if (have == n) end = (size_t)good.back() + 1;
      }
      at += c;
    }
    pos += end;
  }
  *found = have;
  if (have == n) {
    *used = pos;
    *d_out = static_cast<uint8_t*>(out.p);
    out.p = nullptr;
  }
  return GM_OK;
}

// ---- the gm_g1_bases_* / gm_g2_bases_* entries of this file, once for both groups --------------------------------------------------
template <class G>
int bases_check(uint64_t handle, size_t offset, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok) {
  if (ok) *ok = 0;
  GM_CTX();
  typename G::Held* b = G::find(C, handle);
  GM_CHECK(b != nullptr, GM_EHANDLE, "%s_bases_check: unknown handle %llu", G::NAME, (unsigned long long)handle);
  GM_CHECK(ok != nullptr, GM_EINVAL, "%s_bases_check: null pointer", G::NAME);
  GM_CHECK(offset <= b->n && n <= b->n - offset, GM_EINVAL, "%s_bases_check: range [%zu, %zu) outside %zu bases", G::NAME, offset, offset + n, b->n);
  GM_MSM_LOCK(C);
  return check_run<G>(C, b->d + offset * G::AFF_BYTES, G::AFF_BYTES, 0, n, status_or_null, first_bad, ok);
}

template <class G>
int bases_from_bytes(const uint8_t* bytes, size_t n, int compressed, int encoding, int validate, uint64_t* handle, uint8_t* status_or_null, size_t* first_bad, int* ok) {
  if (ok) *ok = 0;  // before anything can return: a negative code never comes with a stale 1 or a stale handle
  if (handle) *handle = 0;
  GM_CTX();
  GM_CHECK(handle != nullptr && ok != nullptr && (bytes != nullptr || n == 0), GM_EINVAL, "%s_bases_from_bytes: null pointer", G::NAME);
  GM_CHECK(encoding == 0 || encoding == 1, GM_EINVAL, "%s_bases_from_bytes: encoding %d (0 arkworks, 1 zcash)", G::NAME, encoding);
  GM_CHECK(n <= SIZE_MAX / G::AFF_BYTES, GM_EINVAL, "%s_bases_from_bytes: %zu points do not fit a size_t", G::NAME, n);
  auto b = std::make_unique<typename G::Held>();
  b->n = n;
  int rc = GM_OK;
  if (first_bad) *first_bad = 0;
  if (n) {
    GM_MSM_LOCK(C);
    const size_t sz = G::AFF_BYTES / (compressed ? 2 : 1);
    DevTmp stage, out;
    Report rep;
    if ((rc = rep.alloc(n, G::BLOCK))) return rc;
    GM_HIP(dev_malloc(&stage.p, n * sz));
    GM_HIP(dev_malloc(&out.p, n * G::AFF_BYTES));
    GM_HIP(hipMemcpyAsync(stage.p, bytes, n * sz, hipMemcpyHostToDevice, C->stream));
    hipLaunchKernelGGL(k_pt_decode<G>, dim3((unsigned)rep.blocks), dim3(G::BLOCK), 0, C->stream, static_cast<const uint8_t*>(stage.p), n, compressed ? 1 : 0, encoding,
                       validate ? 1 : 0, static_cast<uint8_t*>(out.p), rep.status(), rep.summary());
    if ((rc = rep.read(C, status_or_null, first_bad, ok))) return rc;
    if (!*ok) return GM_OK;  // a bad point is a result: nothing stays registered
    b->d = static_cast<uint8_t*>(out.p);
    out.p = nullptr;
  }
  if ((rc = G::before_put(C, b.get()))) {
    if (b->d) (void)raw_free(b->d);
    *ok = 0;
    return rc;
  }
  *handle = G::put(C, std::move(b));
  *ok = 1;
  return GM_OK;
}

// A cyclic share (gm_g1_bases_set_cyclic) is encoded as it is held: the n points of the share, not the key they were cut from.
template <class G>
int bases_to_bytes(uint64_t handle, size_t offset, size_t n, int compressed, int encoding, uint8_t* out, size_t cap) {
  GM_CTX();
  typename G::Held* b = G::find(C, handle);
  GM_CHECK(b != nullptr, GM_EHANDLE, "%s_bases_to_bytes: unknown handle %llu", G::NAME, (unsigned long long)handle);
  GM_CHECK(out != nullptr || n == 0, GM_EINVAL, "%s_bases_to_bytes: null pointer", G::NAME);
  GM_CHECK(encoding == 0 || encoding == 1, GM_EINVAL, "%s_bases_to_bytes: encoding %d (0 arkworks, 1 zcash)", G::NAME, encoding);
  GM_CHECK(offset <= b->n && n <= b->n - offset, GM_EINVAL, "%s_bases_to_bytes: range [%zu, %zu) outside %zu bases", G::NAME, offset, offset + n, b->n);
  GM_CHECK(cap / (G::AFF_BYTES / (compressed ? 2 : 1)) >= n, GM_EINVAL, "%s_bases_to_bytes: %zu bytes do not hold %zu points", G::NAME, cap, n);
  GM_MSM_LOCK(C);
  return encode_run<G>(C, b->d + offset * G::AFF_BYTES, n, compressed, encoding, out);
}

template <class G>
int bases_from_candidates(const uint8_t* cand, size_t m, size_t n, uint64_t* handle, size_t* used, size_t* found) {
  if (handle) *handle = 0;
  GM_CTX();
  GM_CHECK(handle && used && found && (cand || m == 0), GM_EINVAL, "%s_bases_from_candidates: null pointer", G::NAME);
  GM_CHECK(m <= SIZE_MAX / (48 * G::NC) && n <= SIZE_MAX / G::XYZZ_BYTES, GM_EINVAL, "%s_bases_from_candidates: %zu candidates for %zu points do not fit a size_t", G::NAME, m,
           n);
  auto b = std::make_unique<typename G::Held>();
  b->n = n;
  *used = n == 0 ? 0 : m;
  *found = 0;
  int rc;
  if (n && m) {
    if ((rc = candidates_run<G>(C, cand, m, n, &b->d, used, found))) return rc;
  }
  if (*found < n) return GM_OK;  // a shortfall is a result: nothing stays registered
  if ((rc = G::before_put(C, b.get()))) {
    if (b->d) (void)raw_free(b->d);
    return rc;
  }
  *handle = G::put(C, std::move(b));
  return GM_OK;
}

// ---- test aids: ONE device function of field.cuh / field30.cuh / g1.cuh / g2.cuh per lane (gm_debug_fq_op and its kin) -------------
// Records in, records out, no conversion at the boundary: the caller chooses the exact limbs the function sees and reads the exact
// limbs it leaves.  64 lanes per block; a lane beyond n runs the function on the device one (2 where two operands must differ), so
// the asm statements behind fq_mul see a full wave in a partial block.
constexpr int DBG_BLOCK = 64;
enum { FQ_OP_MUL = 0, FQ_OP_SQR, FQ_OP_ADD, FQ_OP_SUB, FQ_OP_DBL, FQ_OP_NEG, FQ_OP_IMPORT, FQ_OP_EXPORT, FQ_OP_INV, FQ_OP_RAW_GE_Q, FQ_OP_PACK_UNPACK, FQ_OP_END };
enum { FQ30_OP_MUL_ASM = 0, FQ30_OP_SQR_ASM, FQ30_OP_MUL_C, FQ30_OP_LOOSE_TO_CANONICAL, FQ30_OP_CANONICAL_TAIL, FQ30_OP_END };
enum { FQ2_OP_MUL = 0, FQ2_OP_SQR, FQ2_OP_ADD, FQ2_OP_SUB, FQ2_OP_NEG, FQ2_OP_INV, FQ2_OP_END };
enum { G1_OP_MADD = 0, G1_OP_ADD, G1_OP_DBL, G1_OP_DBL_AFFINE, G1_OP_STORE_LOAD30, G1_OP_END };
enum { G2_OP_MADD = 0, G2_OP_ADD, G2_OP_DBL, G2_OP_DBL_AFFINE, G2_OP_TO_AFFINE, G2_OP_END };

GM_DEV Fq dbg_load_fq(const uint32_t* p) {
  Fq r;
#pragma unroll
  for (int i = 0; i < 12; i++) r.l[i] = p[i];
  return r;
}
GM_DEV void dbg_store_fq(uint32_t* p, const Fq& a) {
#pragma unroll
  for (int i = 0; i < 12; i++) p[i] = a.l[i];
}
GM_DEV Fq2 dbg_load_fq2(const uint32_t* p) {
  Fq2 r;
  r.c0 = dbg_load_fq(p);
  r.c1 = dbg_load_fq(p + 12);
  return r;
}
GM_DEV void dbg_store_fq2(uint32_t* p, const Fq2& a) {
  dbg_store_fq(p, a.c0);
  dbg_store_fq(p + 12, a.c1);
}

__global__ __launch_bounds__(DBG_BLOCK) void k_debug_fq(int op, const uint32_t* __restrict__ a_in, const uint32_t* __restrict__ b_in, size_t n, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * DBG_BLOCK + threadIdx.x;
  const bool live = i < n;
  const bool binary = op == FQ_OP_MUL || op == FQ_OP_ADD || op == FQ_OP_SUB;
  const Fq a = live ? dbg_load_fq(a_in + i * 12) : fqe_one();
  const Fq b = live && binary ? dbg_load_fq(b_in + i * 12) : fq_dbl(fqe_one());
  Fq r = Fq::zero();
  if (op == FQ_OP_MUL) r = fq_mul(a, b);
  else if (op == FQ_OP_SQR) r = fq_sqr(a);
  else if (op == FQ_OP_ADD) r = fq_add(a, b);
  else if (op == FQ_OP_SUB) r = fq_sub(a, b);
  else if (op == FQ_OP_DBL) r = fq_dbl(a);
  else if (op == FQ_OP_NEG) r = fq_neg_canonical(a);
  else if (op == FQ_OP_IMPORT) r = fqe_import(a);
  else if (op == FQ_OP_EXPORT) r = fqe_export(a);
  else if (op == FQ_OP_INV) r = fq_inv(a);
  else if (op == FQ_OP_RAW_GE_Q) r.l[0] = pt_raw_ge_q(a) ? 1u : 0u;
  else r = fq30_pack(fq30_unpack(a));
  if (live) dbg_store_fq(out + i * 12, r);
}

__global__ __launch_bounds__(DBG_BLOCK) void k_debug_fq30(int op, const uint32_t* __restrict__ a_in, const uint32_t* __restrict__ b_in, size_t n, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * DBG_BLOCK + threadIdx.x;
  const bool live = i < n;
  const bool binary = op == FQ30_OP_MUL_ASM || op == FQ30_OP_MUL_C;
  Fq30 a = fq30_const(Fq30Consts::ONE), b = fq30_const(Fq30Consts::ONE);
  if (live) {
#pragma unroll
    for (int k = 0; k < 13; k++) a.l[k] = a_in[i * 13 + k];
    if (binary) {
#pragma unroll
      for (int k = 0; k < 13; k++) b.l[k] = b_in[i * 13 + k];
    }
  }
  Fq30 r = Fq30::zero();
  if (op == FQ30_OP_MUL_ASM) {
    r = fq30_mul_asm(a.l[0], a.l[1], a.l[2], a.l[3], a.l[4], a.l[5], a.l[6], a.l[7], a.l[8], a.l[9], a.l[10], a.l[11], a.l[12],
                     b.l[0], b.l[1], b.l[2], b.l[3], b.l[4], b.l[5], b.l[6], b.l[7], b.l[8], b.l[9], b.l[10], b.l[11], b.l[12]);
  } else if (op == FQ30_OP_SQR_ASM) {
    r = fq30_sqr_asm(a.l[0], a.l[1], a.l[2], a.l[3], a.l[4], a.l[5], a.l[6], a.l[7], a.l[8], a.l[9], a.l[10], a.l[11], a.l[12]);
  } else if (op == FQ30_OP_MUL_C) {
    r = fq30_mul(a, b);
  } else if (op == FQ30_OP_LOOSE_TO_CANONICAL) {
    const Fq c = fq30_loose_to_canonical(a);
#pragma unroll
    for (int k = 0; k < 12; k++) r.l[k] = c.l[k];  // 12 words and a zero
  } else {
    r = fq30_canonical_tail(a);
  }
  if (live) {
#pragma unroll
    for (int k = 0; k < 13; k++) out[i * 13 + k] = r.l[k];
  }
}

__global__ __launch_bounds__(DBG_BLOCK) void k_debug_fq2(int op, const uint32_t* __restrict__ a_in, const uint32_t* __restrict__ b_in, size_t n, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * DBG_BLOCK + threadIdx.x;
  const bool live = i < n;
  const bool binary = op == FQ2_OP_MUL || op == FQ2_OP_ADD || op == FQ2_OP_SUB;
  const Fq2 a = live ? dbg_load_fq2(a_in + i * 24) : fq2_one();
  const Fq2 b = live && binary ? dbg_load_fq2(b_in + i * 24) : fq2_dbl(fq2_one());
  Fq2 r;
  if (op == FQ2_OP_MUL) r = fq2_mul(a, b);
  else if (op == FQ2_OP_SQR) r = fq2_sqr(a);
  else if (op == FQ2_OP_ADD) r = fq2_add(a, b);
  else if (op == FQ2_OP_SUB) r = fq2_sub(a, b);
  else if (op == FQ2_OP_NEG) r = fq2_neg_canonical(a);
  else r = fq2_inv(a);
  if (live) dbg_store_fq2(out + i * 24, r);
}

// p: XYZZ records (4 x 12 words; G1_OP_DBL_AFFINE reads the affine point from the first 24 and ignores the rest); q: 24 words (affine)
// for G1_OP_MADD, 48 for G1_OP_ADD, not read otherwise.  out: x | y | zz | zzz as the function returns them.
__global__ __launch_bounds__(DBG_BLOCK) void k_debug_g1(int op, const uint32_t* __restrict__ p_in, const uint32_t* __restrict__ q_in, size_t n, uint32_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t rec[DBG_BLOCK * XYZZ30_BYTES];
  const size_t i = (size_t)blockIdx.x * DBG_BLOCK + threadIdx.x;
  const bool live = i < n;
  const FqE one = fqe_one();
  G1Xyzz P, Q;
  P.x = P.y = P.zz = P.zzz = one;
  Q = P;
  Q.x = fq_dbl(one);
  if (live) {
    const uint32_t* s = p_in + i * 48;
    P.x = dbg_load_fq(s); P.y = dbg_load_fq(s + 12); P.zz = dbg_load_fq(s + 24); P.zzz = dbg_load_fq(s + 36);
    if (op == G1_OP_MADD) {
      Q.x = dbg_load_fq(q_in + i * 24); Q.y = dbg_load_fq(q_in + i * 24 + 12);
    } else if (op == G1_OP_ADD) {
      const uint32_t* t = q_in + i * 48;
      Q.x = dbg_load_fq(t); Q.y = dbg_load_fq(t + 12); Q.zz = dbg_load_fq(t + 24); Q.zzz = dbg_load_fq(t + 36);
    }
  }
  G1Affine qa, pa;
  qa.x = Q.x; qa.y = Q.y;
  pa.x = P.x; pa.y = P.y;
  G1Xyzz r = P;
  if (op == G1_OP_MADD) {
    xyzz_madd(r, qa);
  } else if (op == G1_OP_ADD) {
    xyzz_add(r, Q);
  } else if (op == G1_OP_DBL) {
    r = xyzz_dbl(P);
  } else if (op == G1_OP_DBL_AFFINE) {
    r = xyzz_dbl_affine(pa);
  } else {
    g1_store_xyzz30(rec + threadIdx.x * XYZZ30_BYTES, P);
    r = g1_load_xyzz30(rec + threadIdx.x * XYZZ30_BYTES);
  }
  if (live) {
    uint32_t* o = out + i * 48;
    dbg_store_fq(o, r.x); dbg_store_fq(o + 12, r.y); dbg_store_fq(o + 24, r.zz); dbg_store_fq(o + 36, r.zzz);
  }
}

// The same over Fq2: p 4 x 24 words (G2_OP_DBL_AFFINE reads the first 48); q 48 words for G2_OP_MADD, 96 for G2_OP_ADD.  out: 96 words;
// G2_OP_TO_AFFINE writes x | y into the first 48 and zeroes behind them.
__global__ __launch_bounds__(DBG_BLOCK) void k_debug_g2(int op, const uint32_t* __restrict__ p_in, const uint32_t* __restrict__ q_in, size_t n, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * DBG_BLOCK + threadIdx.x;
  const bool live = i < n;
  G2Xyzz P, Q;
  P.x = P.y = P.zz = P.zzz = fq2_one();
  Q = P;
  Q.x = fq2_dbl(fq2_one());
  if (live) {
    const uint32_t* s = p_in + i * 96;
    P.x = dbg_load_fq2(s); P.y = dbg_load_fq2(s + 24); P.zz = dbg_load_fq2(s + 48); P.zzz = dbg_load_fq2(s + 72);
    if (op == G2_OP_MADD) {
      Q.x = dbg_load_fq2(q_in + i * 48); Q.y = dbg_load_fq2(q_in + i * 48 + 24);
    } else if (op == G2_OP_ADD) {
      const uint32_t* t = q_in + i * 96;
      Q.x = dbg_load_fq2(t); Q.y = dbg_load_fq2(t + 24); Q.zz = dbg_load_fq2(t + 48); Q.zzz = dbg_load_fq2(t + 72);
    }
  }
  G2Affine qa, pa;
  qa.x = Q.x; qa.y = Q.y;
  pa.x = P.x; pa.y = P.y;
  G2Xyzz r = P;
  if (op == G2_OP_MADD) {
    g2_madd(r, qa);
  } else if (op == G2_OP_ADD) {
    g2_add(r, Q);
  } else if (op == G2_OP_DBL) {
    r = g2_dbl(P);
  } else if (op == G2_OP_DBL_AFFINE) {
    r = g2_dbl_affine(pa);
  } else {
    const G2Affine a = grp_to_affine<GrpG2>(P);
    r.x = a.x; r.y = a.y; r.zz = fq2_zero(); r.zzz = fq2_zero();
  }
  if (live) {
    uint32_t* o = out + i * 96;
    dbg_store_fq2(o, r.x); dbg_store_fq2(o + 24, r.y); dbg_store_fq2(o + 48, r.zz); dbg_store_fq2(o + 72, r.zzz);
  }
}

// host side of the five entries above: a (aw words per element), b (bw words, 0: not read) -> out (ow words)
template <class K>
int debug_op_run(Context* C, K kernel, int op, const uint32_t* a, size_t aw, const uint32_t* b, size_t bw, size_t n, uint32_t* out, size_t ow) {
  GM_MSM_LOCK(C);
  DevTmp d;
  GM_HIP(dev_malloc(&d.p, n * (aw + bw + ow) * 4));
  uint32_t *d_a = static_cast<uint32_t*>(d.p), *d_b = d_a + n * aw, *d_out = d_b + n * bw;
  GM_HIP(hipMemcpyAsync(d_a, a, n * aw * 4, hipMemcpyHostToDevice, C->stream));
  if (bw) GM_HIP(hipMemcpyAsync(d_b, b, n * bw * 4, hipMemcpyHostToDevice, C->stream));
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + DBG_BLOCK - 1) / DBG_BLOCK)), dim3(DBG_BLOCK), 0, C->stream, op, (const uint32_t*)d_a, (const uint32_t*)d_b, n, d_out);
  GM_HIP(hipGetLastError());
  GM_HIP(hipMemcpyAsync(out, d_out, n * ow * 4, hipMemcpyDeviceToHost, C->stream));
  GM_HIP(hipStreamSynchronize(C->stream));
  return GM_OK;
}

}  // namespace

// The group elements of many proofs at once (ipa.hip: ipa_verify_many): Jacobian points of both groups, any representative ->
// the host records the proof checks build (r1: 12 limbs, r2: 24 limbs per point) and one GM_PT_* status byte per point, from ONE
// k_pt_check launch per non-empty group.  Caller holds the MSM lock.
int jac_points_status(Context* C, const std::vector<const uint64_t*>& g1, const std::vector<const uint64_t*>& g2, std::vector<uint64_t>& r1, std::vector<uint64_t>& r2,
                      std::vector<uint8_t>& st1, std::vector<uint8_t>& st2) {
  const size_t n1 = g1.size(), n2 = g2.size();
  r1.assign(n1 * 12, 0);
  r2.assign(n2 * 24, 0);
  st1.assign(n1, 0);
  st2.assign(n2, 0);
  for (size_t i = 0; i < n1; i++) proof_g1_record(g1[i], r1.data() + 12 * i);
  for (size_t i = 0; i < n2; i++) proof_g2_record(g2[i], r2.data() + 24 * i);
  DevTmp stage;
  if (n1 + n2) {
    GM_HIP(dev_malloc(&stage.p, n1 * 96 + n2 * 192));
    if (n1) GM_HIP(hipMemcpyAsync(stage.p, r1.data(), n1 * 96, hipMemcpyHostToDevice, C->stream));
    if (n2) GM_HIP(hipMemcpyAsync(stage.u8() + n1 * 96, r2.data(), n2 * 192, hipMemcpyHostToDevice, C->stream));
  }
  int ok1 = 0, ok2 = 0;
  int rc = check_run<PtG1>(C, stage.u8(), 96, 1, n1, st1.data(), nullptr, &ok1);
  if (!rc) rc = check_run<PtG2>(C, stage.u8() + n1 * 96, 192, 1, n2, st2.data(), nullptr, &ok2);
  if (rc) (void)hipStreamSynchronize(C->stream);  // nothing in flight reads the stage once it goes
  return rc;
}
}  // namespace gm

using namespace gm;

extern "C" {

int gm_g1_check(const void* points, size_t stride, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok) {
  return check_host<PtG1>(points, stride, n, status_or_null, first_bad, ok);
}
int gm_g2_check(const void* points, size_t stride, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok) {
  return check_host<PtG2>(points, stride, n, status_or_null, first_bad, ok);
}

int gm_g1_bases_check(uint64_t handle, size_t offset, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok) {
  return bases_check<PtG1>(handle, offset, n, status_or_null, first_bad, ok);
}
int gm_g2_bases_check(uint64_t handle, size_t offset, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok) {
  return bases_check<PtG2>(handle, offset, n, status_or_null, first_bad, ok);
}

int gm_g1_bases_from_bytes(const uint8_t* bytes, size_t n, int compressed, int encoding, int validate, uint64_t* handle, uint8_t* status_or_null, size_t* first_bad,
                           int* ok) {
  return bases_from_bytes<PtG1>(bytes, n, compressed, encoding, validate, handle, status_or_null, first_bad, ok);
}
int gm_g2_bases_from_bytes(const uint8_t* bytes, size_t n, int compressed, int encoding, int validate, uint64_t* handle, uint8_t* status_or_null, size_t* first_bad,
                           int* ok) {
  return bases_from_bytes<PtG2>(bytes, n, compressed, encoding, validate, handle, status_or_null, first_bad, ok);
}

int gm_g1_bases_to_bytes(uint64_t handle, size_t offset, size_t n, int compressed, int encoding, uint8_t* out, size_t cap) {
  return bases_to_bytes<PtG1>(handle, offset, n, compressed, encoding, out, cap);
}
int gm_g2_bases_to_bytes(uint64_t handle, size_t offset, size_t n, int compressed, int encoding, uint8_t* out, size_t cap) {
  return bases_to_bytes<PtG2>(handle, offset, n, compressed, encoding, out, cap);
}

int gm_g1_bases_from_candidates(const uint8_t* cand, size_t m, size_t n, uint64_t* handle, size_t* used, size_t* found) {
  return bases_from_candidates<PtG1>(cand, m, n, handle, used, found);
}
int gm_g2_bases_from_candidates(const uint8_t* cand, size_t m, size_t n, uint64_t* handle, size_t* used, size_t* found) {
  return bases_from_candidates<PtG2>(cand, m, n, handle, used, found);
}

int gm_crs_from_bases(uint64_t g1_handle, uint64_t g2_handle, uint64_t* crs) {
  if (crs) *crs = 0;
  GM_CTX();
  Bases* b1 = find_bases(g1_handle);
  GM_CHECK(b1 != nullptr, GM_EHANDLE, "crs_from_bases: unknown handle %llu", (unsigned long long)g1_handle);
  G2Bases* b2 = find_in(C, C->g2_bases, g2_handle);
  GM_CHECK(b2 != nullptr, GM_EHANDLE, "crs_from_bases: unknown G2 bases handle %llu", (unsigned long long)g2_handle);
  GM_CHECK(crs != nullptr, GM_EINVAL, "crs_from_bases: null pointer");
  GM_CHECK(b1->n >= 1 && b2->n >= 1, GM_EINVAL, "crs_from_bases: empty CRS");
  GM_MSM_LOCK(C);
  DevTmp d1, d2;
  GM_HIP(dev_malloc(&d1.p, b1->n * 96));
  GM_HIP(dev_malloc(&d2.p, b2->n * G2_AFF_BYTES));
  GM_HIP(hipMemcpyAsync(d1.p, b1->d, b1->n * 96, hipMemcpyDeviceToDevice, C->stream));
  GM_HIP(hipMemcpyAsync(d2.p, b2->d, b2->n * G2_AFF_BYTES, hipMemcpyDeviceToDevice, C->stream));
  GM_HIP(hipStreamSynchronize(C->stream));
  auto c = std::make_unique<Crs>();
  c->g1 = static_cast<uint8_t*>(d1.p);
  c->n1 = b1->n;
  c->g2 = static_cast<uint8_t*>(d2.p);
  c->n2 = b2->n;
  d1.p = d2.p = nullptr;
  *crs = put_in(C, C->crs, std::move(c));
  return GM_OK;
}

int gm_crs_check(uint64_t crs, size_t* first_bad_g1, size_t* first_bad_g2, int* ok) {
  if (ok) *ok = 0;
  GM_CTX();
  Crs* c = find_in(C, C->crs, crs);
  GM_CHECK(c != nullptr, GM_EHANDLE, "crs_check: unknown CRS handle %llu", (unsigned long long)crs);
  GM_CHECK(ok != nullptr, GM_EINVAL, "crs_check: null pointer");
  GM_MSM_LOCK(C);
  int ok1 = 0, ok2 = 0;
  int rc = check_run<PtG1>(C, c->g1, 96, 0, c->n1, nullptr, first_bad_g1, &ok1);
  if (!rc) rc = check_run<PtG2>(C, c->g2, G2_AFF_BYTES, 0, c->n2, nullptr, first_bad_g2, &ok2);
  if (rc) return rc;
  *ok = ok1 && ok2;
  return GM_OK;
}

int gm_vk_check(uint64_t vk, size_t* first_bad_g1, size_t* first_bad_g2, int* ok) {
  if (ok) *ok = 0;
  GM_CTX();
  VerifierKey* K = find_in(C, C->vks, vk);
  GM_CHECK(K != nullptr, GM_EHANDLE, "vk_check: unknown verifier key handle %llu", (unsigned long long)vk);
  GM_CHECK(ok != nullptr, GM_EINVAL, "vk_check: null pointer");
  GM_MSM_LOCK(C);
  size_t b1 = 0, b2 = 0;
  int rc = check_records(C, K->g1, K->g2, &b1, &b2, ok);
  if (rc) return rc;
  if (first_bad_g1) *first_bad_g1 = b1;
  if (first_bad_g2) *first_bad_g2 = b2;
  return GM_OK;
}

int gm_snark_proof_check(const gm_snark_proof* proof, size_t* first_bad, int* ok) {
  if (ok) *ok = 0;
  GM_CHECK(proof != nullptr && ok != nullptr && (proof->fold_commitments != nullptr || proof->nfold == 0), GM_EINVAL, "snark_proof_check: null pointer");
  std::vector<const uint64_t*> g1{proof->witness_commitment};
  for (size_t i = 0; i < proof->nfold; i++) g1.push_back(proof->fold_commitments + 18 * i);
  g1.push_back(proof->evaluation_proof);
  return proof_check(g1, first_bad, ok);
}

int gm_psnark_proof_check(const gm_psnark_proof* proof, size_t* first_bad, int* ok) {
  if (ok) *ok = 0;
  GM_CHECK(proof != nullptr && ok != nullptr && (proof->fold_commitments != nullptr || proof->nfold == 0), GM_EINVAL, "psnark_proof_check: null pointer");
  std::vector<const uint64_t*> g1{proof->witness_commitment};
  for (int i = 0; i < 3; i++) g1.push_back(proof->r_star_commitments[i]);
  g1.push_back(proof->z_star_commitment);
  for (int i = 0; i < 3; i++) g1.push_back(proof->sorted_commitments[i]);
  for (int i = 0; i < 9; i++) g1.push_back(proof->acc_v_commitments[i]);
  g1.push_back(proof->ralpha_star_acc_mu_proof);
  for (size_t i = 0; i < proof->nfold; i++) g1.push_back(proof->fold_commitments + 18 * i);
  g1.push_back(proof->evaluation_proof);
  return proof_check(g1, first_bad, ok);
}

int gm_ipa_check(uint64_t proof, size_t* first_bad, int* ok) {
  if (ok) *ok = 0;
  GM_CTX();
  IpaProof* p = find_in(C, C->ipa, proof);
  GM_CHECK(p != nullptr, GM_EHANDLE, "ipa_check: unknown proof handle %llu", (unsigned long long)proof);
  GM_CHECK(ok != nullptr, GM_EINVAL, "ipa_check: null pointer");
  const size_t k = p->final_g1.size() / 18;
  GM_CHECK(p->final_g2.size() == k * 36, GM_EINVAL, "ipa_check: %zu Lhs final foldings and %zu Rhs ones", k, p->final_g2.size() / 36);
  // the fg1 / fg2 points of claims 0 .. K - 1, then the final foldings
  const size_t K = p->K;
  GM_CHECK(K >= 1 && p->foldings_fg1.size() == K * 22 && p->foldings_fg2.size() == K * 40, GM_EINVAL, "ipa_check: the foldings of %zu claims are missing", K);
  std::vector<uint64_t> r1((K + k) * 12), r2((K + k) * 24);
  for (size_t c = 0; c < K; c++) {
    proof_g1_record(p->foldings_fg1.data() + 22 * c, r1.data() + 12 * c);
    proof_g2_record(p->foldings_fg2.data() + 40 * c + 4, r2.data() + 24 * c);
  }
  for (size_t i = 0; i < k; i++) {
    proof_g1_record(p->final_g1.data() + 18 * i, r1.data() + 12 * (K + i));
    proof_g2_record(p->final_g2.data() + 36 * i, r2.data() + 24 * (K + i));
  }
  GM_MSM_LOCK(C);
  size_t b1 = 0, b2 = 0;
  int rc = check_records(C, r1, r2, &b1, &b2, ok);
  if (rc) return rc;
  if (first_bad) *first_bad = b1 < K + k ? b1 : K + k + b2;  // the G1 elements come first
  return GM_OK;
}

int gm_debug_fq2_sqrt(const uint64_t* a_mont, size_t n, uint64_t* root_mont, uint8_t* is_square) {
  GM_CTX();
  GM_CHECK((a_mont && root_mont && is_square) || n == 0, GM_EINVAL, "debug_fq2_sqrt: null pointer");
  GM_CHECK(n <= (size_t)1 << 30, GM_EINVAL, "debug_fq2_sqrt: %zu elements in one call", n);
  if (n == 0) return GM_OK;
  GM_MSM_LOCK(C);
  DevTmp in, out;
  GM_HIP(dev_malloc(&in.p, n * 96));
  GM_HIP(dev_malloc(&out.p, n * 96 + n));
  GM_HIP(hipMemcpyAsync(in.p, a_mont, n * 96, hipMemcpyHostToDevice, C->stream));
  uint8_t* d_out = static_cast<uint8_t*>(out.p);
  hipLaunchKernelGGL(k_fq2_sqrt, dim3((unsigned)((n + PT_G2_BLOCK - 1) / PT_G2_BLOCK)), dim3(PT_G2_BLOCK), 0, C->stream, static_cast<const uint8_t*>(in.p), n, d_out,
                     d_out + n * 96);
  GM_HIP(hipGetLastError());
  GM_HIP(hipMemcpyAsync(root_mont, d_out, n * 96, hipMemcpyDeviceToHost, C->stream));
  GM_HIP(hipMemcpyAsync(is_square, d_out + n * 96, n, hipMemcpyDeviceToHost, C->stream));
  GM_HIP(hipStreamSynchronize(C->stream));
  return GM_OK;
}

// the element-wise test aids: `bw` is the second operand's width for this op, 0 when the op does not read it
#define GM_DEBUG_OP(who, kernel, end, aw, bw, ow)                                                                 \
  GM_CTX();                                                                                                       \
  GM_CHECK((a && out && (b || (bw) == 0)) || n == 0, GM_EINVAL, who ": null pointer");                            \
  if (n == 0) return GM_OK;                                                                                       \
  GM_CHECK(op >= 0 && op < (end), GM_EINVAL, who ": unknown op %d", op);                                          \
  GM_CHECK(n <= (size_t)1 << 20, GM_EINVAL, who ": %zu elements in one call (at most 2^20)", n);                  \
  return debug_op_run(C, kernel, op, a, aw, b, bw, n, out, ow)

int gm_debug_fq_op(int op, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out) {
  const size_t bw = (op == FQ_OP_MUL || op == FQ_OP_ADD || op == FQ_OP_SUB) ? 12 : 0;
  GM_DEBUG_OP("debug_fq_op", k_debug_fq, FQ_OP_END, 12, bw, 12);
}
int gm_debug_fq30_op(int op, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out) {
  const size_t bw = (op == FQ30_OP_MUL_ASM || op == FQ30_OP_MUL_C) ? 13 : 0;
  GM_DEBUG_OP("debug_fq30_op", k_debug_fq30, FQ30_OP_END, 13, bw, 13);
}
int gm_debug_fq2_op(int op, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out) {
  const size_t bw = (op == FQ2_OP_MUL || op == FQ2_OP_ADD || op == FQ2_OP_SUB) ? 24 : 0;
  GM_DEBUG_OP("debug_fq2_op", k_debug_fq2, FQ2_OP_END, 24, bw, 24);
}
int gm_debug_g1_op(int op, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out) {
  const size_t bw = op == G1_OP_MADD ? 24 : op == G1_OP_ADD ? 48 : 0;
  GM_DEBUG_OP("debug_g1_op", k_debug_g1, G1_OP_END, 48, bw, 48);
}
int gm_debug_g2_op(int op, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out) {
  const size_t bw = op == G2_OP_MADD ? 48 : op == G2_OP_ADD ? 96 : 0;
  GM_DEBUG_OP("debug_g2_op", k_debug_g2, G2_OP_END, 96, bw, 96);
}
#undef GM_DEBUG_OP

int gm_g1_powers_check(uint64_t handle, size_t offset, size_t n, const uint64_t g2_affine[24], const uint64_t tau_g2_affine[24], const uint64_t rho_mont[4], int* ok) {
  if (ok) *ok = 0;
  GM_CTX();
  Bases* b = find_bases(handle);
  GM_CHECK(b != nullptr, GM_EHANDLE, "g1_powers_check: unknown handle %llu", (unsigned long long)handle);
  GM_CHECK(g2_affine && tau_g2_affine && rho_mont && ok, GM_EINVAL, "g1_powers_check: null pointer");
  GM_CHECK(offset <= b->n && n <= b->n - offset, GM_EINVAL, "g1_powers_check: range [%zu, %zu) outside %zu bases", offset, offset + n, b->n);
  GM_CHECK((rho_mont[0] | rho_mont[1] | rho_mont[2] | rho_mont[3]) != 0, GM_EINVAL, "g1_powers_check: rho = 0 tests the first pair only");
  // a cyclic share (gm_g1_bases_set_cyclic) holds every world-th power: consecutive powers of tau^world, not of tau.  Sharded checks
  // are out of scope, and answering "bad key" would be wrong
  GM_CHECK(b->cyclic_n == 0, GM_EINVAL, "g1_powers_check: handle %llu is a cyclic share of a %zu-power key (rank %d of %d); check the whole key", (unsigned long long)handle,
           b->cyclic_n, b->cyc_rank, b->cyc_world);
  if (n <= 1) {
    *ok = 1;
    return GM_OK;
  }
  GM_MSM_LOCK(C);  // one flight for the two MSMs and the pairing (the entries below take it again: recursive)
  // A = sum rho^i P_i, B = sum rho^i P_{i+1}, i < n - 1;  e(A, tau g2) e(-B, g2) == 1
  uint64_t v = 0;
  int rc = gm_fr_vec_alloc(n - 1, &v);
  if (rc) return rc;
  uint64_t A[18], B[18];
  rc = gm_fr_powers(rho_mont, n - 1, v);
  if (!rc) rc = gm_g1_msm_v(handle, offset, 0, v, 0, n - 1, A);
  if (!rc) rc = gm_g1_msm_v(handle, offset + 1, 0, v, 0, n - 1, B);
  (void)gm_fr_vec_free(v);
  if (rc) return rc;
  uint64_t p1[24], p2[48], gt[72], one[72];
  const gmh::G1 a = gmh::G1::from_limbs(A).normalized(), nb = gmh::G1::from_limbs(B).normalized();
  memset(p1, 0, sizeof p1);  // the identity is the all-zero record
  if (!a.is_identity()) {
    a.x.to_limbs(p1);
    a.y.to_limbs(p1 + 6);
  }
  if (!nb.is_identity()) {
    nb.x.to_limbs(p1 + 12);
    nb.y.neg().to_limbs(p1 + 18);
  }
  memcpy(p2, tau_g2_affine, 192);
  memcpy(p2 + 24, g2_affine, 192);
  if ((rc = gm_pairing_multi(p1, 96, p2, 192, 2, gt))) return rc;
  if ((rc = gm_gt_one(one))) return rc;
  *ok = memcmp(gt, one, sizeof gt) == 0 ? 1 : 0;
  return GM_OK;
}

}  // extern "C"
