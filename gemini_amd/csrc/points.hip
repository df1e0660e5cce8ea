// Validation and decoding of UNTRUSTED G1 / G2 points on the device (gfx950): canonical coordinates, the curve equation, membership
// of the prime-order subgroup, the two G1 byte framings of gemini_amd/wire.py, and the powers-of-tau structure of a committer key.
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
// = 1262; G2 check 11 (import + curve) + 63 x 24 + 5 x 28 + 11 = 1674; a compressed decode adds the square root, 378 squares + 228 products.
//
// Reporting: ONE status byte per point (the first check that fails, gemini_hip.h: GM_PT_*), written with ordinary stores, and one
// u32 per block holding the block's first bad lane.  The host reads the block summaries (and the status bytes when the caller asks
// for them); no coordinate crosses back.  Launches go on the library's stream under the MSM lock, as the pairing entries do.
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "g2.cuh"
#include "host_field.hpp"

namespace gm {

int bases_build_phi(Context* C, Bases* b);  // msm.hip

constexpr int PT_BLOCK = 256;      // G1 kernels: amdgpu_waves_per_eu(2, 2) -- 96 / 112 bytes of scratch buy the second wave, 1.27 x against one wave (profiles/point_check.md)
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
// the limbs as an integer: >= q?
GM_DEV bool pt_raw_ge_q(const Fq& a) {
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    uint32_t b;
    (void)__builtin_subc(a.l[i], FqParams::MOD[i], borrow, &b);
    borrow = b;
  }
  return borrow == 0;
}
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
GM_DEV uint8_t pt_g2_status(const G2Affine& Q) {
  Fq2 four_xi;  // 4 (1 + u)
  four_xi.c0 = pt_four();
  four_xi.c1 = four_xi.c0;
  if (!fq2_is_zero(fq2_sub(fq2_sqr(Q.y), fq2_add(fq2_mul(fq2_sqr(Q.x), Q.x), four_xi)))) return GM_PT_NOT_ON_CURVE;
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

// ---- reporting: the status byte of the lane, and the block's first bad lane (every lane of the block arrives here) -------------
GM_DEV void pt_report(size_t i, size_t n, uint8_t st, uint8_t* __restrict__ status, uint32_t* __restrict__ summary) {
  __shared__ uint32_t first[PT_BLOCK / 64];
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

// host_form != 0: records as gm_g1_bases_register takes them (ark-ff Montgomery limbs, stride >= 96, the infinity byte at 96 when the
// stride has room); 0: packed device records (stride 96), canonical by construction
__global__ __launch_bounds__(PT_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_g1_check(const uint8_t* __restrict__ src, size_t stride, int host_form, size_t n, uint8_t* __restrict__ status,
                                                       uint32_t* __restrict__ summary) {
  const size_t i = (size_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  uint8_t st = GM_PT_OK;
  if (i < n) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src + i * stride);
    G1Affine P;
#pragma unroll
    for (int k = 0; k < 12; k++) {
      P.x.l[k] = s[k];
      P.y.l[k] = s[12 + k];
    }
    const bool inf = (host_form && stride >= 97 && src[i * stride + 96] != 0) || P.is_identity();  // what k_pack_bases reads as the identity
    if (!inf) {
      if (host_form && (pt_raw_ge_q(P.x) || pt_raw_ge_q(P.y))) {
        st = GM_PT_NONCANONICAL;
      } else {
        if (host_form) {
          P.x = fqe_import(P.x);
          P.y = fqe_import(P.y);
        }
        st = pt_g1_status(P, true);
      }
    }
  }
  pt_report(i, n, st, status, summary);
}

__global__ __launch_bounds__(PT_G2_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_g2_check(const uint8_t* __restrict__ src, size_t stride, int host_form, size_t n,
                                                                                                      uint8_t* __restrict__ status, uint32_t* __restrict__ summary) {
  const size_t i = (size_t)blockIdx.x * PT_G2_BLOCK + threadIdx.x;
  uint8_t st = GM_PT_OK;
  if (i < n) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src + i * stride);
    FqE c[4];
    uint32_t any = 0;
    bool canonical = true;
#pragma unroll
    for (int e = 0; e < 4; e++) {
#pragma unroll
      for (int k = 0; k < 12; k++) {
        c[e].l[k] = s[12 * e + k];
        any |= c[e].l[k];
      }
      canonical = canonical && !pt_raw_ge_q(c[e]);
    }
    const bool inf = (host_form && stride >= 193 && src[i * stride + 192] != 0) || any == 0;
    if (!inf) {
      if (host_form && !canonical) {
        st = GM_PT_NONCANONICAL;
      } else {
        if (host_form) {
#pragma unroll
          for (int e = 0; e < 4; e++) c[e] = fqe_import(c[e]);
        }
        G2Affine Q;
        Q.x.c0 = c[0];
        Q.x.c1 = c[1];
        Q.y.c0 = c[2];
        Q.y.c1 = c[3];
        st = pt_g2_status(Q);
      }
    }
  }
  pt_report(i, n, st, status, summary);
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

// 48- / 96-byte encodings -> packed device records (the layout k_pack_bases produces; the identity and every rejected point are the
// all-zero record).  Acceptance and the order of the checks are those of wire.g1_deserialize(.., strict = True, validate).
__global__ __launch_bounds__(PT_BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_g1_decode(const uint8_t* __restrict__ bytes, size_t n, int compressed, int zcash, int validate, uint8_t* __restrict__ dst,
                                                        uint8_t* __restrict__ status, uint32_t* __restrict__ summary) {
  const size_t i = (size_t)blockIdx.x * PT_BLOCK + threadIdx.x;
  uint8_t st = GM_PT_OK;
  if (i < n) {
    const size_t sz = compressed ? 48 : 96;
    Fq x = fp_load<FqParams>(bytes + i * sz), y = Fq::zero();
    if (!compressed) y = fp_load<FqParams>(bytes + i * sz + 48);
    if (zcash) {  // big-endian: limb k is word 11 - k, byte-swapped
      Fq t = x, u = y;
#pragma unroll
      for (int k = 0; k < 12; k++) {
        x.l[k] = pt_bswap(t.l[11 - k]);
        y.l[k] = pt_bswap(u.l[11 - k]);
      }
    }
    bool inf, larger;
    if (zcash) {  // flags in the three top bits of the first byte = the top bits of x
      const uint32_t f = x.l[11] >> 29;
      x.l[11] &= 0x1fffffffu;
      inf = (f >> 1) & 1u;
      larger = f & 1u;
      if ((int)(f >> 2) != (compressed ? 1 : 0) || (larger && (!compressed || inf))) st = GM_PT_BAD_ENCODING;
    } else {  // flags in the two top bits of the last byte = the top bits of the last coordinate
      const uint32_t f = (compressed ? x.l[11] : y.l[11]) >> 30;
      if (compressed) x.l[11] &= 0x3fffffffu;
      else y.l[11] &= 0x3fffffffu;
      inf = f == 1;
      larger = f == 2;
      if (f == 3) st = GM_PT_BAD_ENCODING;
    }
    G1Affine P;
    P.x = fqe_zero();
    P.y = fqe_zero();
    if (st == GM_PT_OK) {
      if (inf) {
        if (!x.is_zero() || !y.is_zero()) st = GM_PT_BAD_ENCODING;  // infinity with non-zero coordinates
      } else if (compressed) {
        if (pt_raw_ge_q(x)) {
          st = GM_PT_NONCANONICAL;
        } else {
          P.x = pt_from_int(x);
          const FqE rhs = fq_add(fq_mul(fq_sqr(P.x), P.x), pt_four());
          P.y = pt_sqrt_candidate(rhs);
          if (!(fq_sqr(P.y) == rhs)) {
            st = GM_PT_NOT_ON_CURVE;  // x^3 + 4 is no square
          } else {
            if (pt_y_is_larger(pt_to_int(P.y)) != larger) P.y = fq_neg_canonical(P.y);
            if (validate) st = pt_g1_status(P, false);  // on the curve by construction
          }
        }
      } else {
        const bool y_ge = pt_raw_ge_q(y);
        // wire.py compares the sign flag BEFORE the canonical check; for y >= q its `y > (q - y) mod q` is always true
        if (!zcash && (y_ge || pt_y_is_larger(y)) != larger) {
          st = GM_PT_BAD_ENCODING;
        } else if (y_ge || pt_raw_ge_q(x)) {
          st = GM_PT_NONCANONICAL;
        } else {
          P.x = pt_from_int(x);
          P.y = pt_from_int(y);
          if (validate) st = pt_g1_status(P, true);
        }
      }
    }
    if (st != GM_PT_OK) {
      P.x = fqe_zero();
      P.y = fqe_zero();
    }
    g1_store_affine(dst + i * 96, P);
  }
  pt_report(i, n, st, status, summary);
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
namespace {

struct DevTmp {  // freed on every path out
  void* p = nullptr;
  ~DevTmp() {
    if (p) (void)raw_free(p);
  }
};

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

// group: 1 / 2.  d_src: device memory, `stride` bytes per record.  Caller holds the MSM lock.
int check_run(Context* C, int group, const uint8_t* d_src, size_t stride, int host_form, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok) {
  if (n == 0) {
    if (first_bad) *first_bad = 0;
    *ok = 1;
    return GM_OK;
  }
  Report rep;
  int rc = rep.alloc(n, group == 1 ? PT_BLOCK : PT_G2_BLOCK);
  if (rc) return rc;
  if (group == 1)
    hipLaunchKernelGGL(k_g1_check, dim3((unsigned)rep.blocks), dim3(PT_BLOCK), 0, C->stream, d_src, stride, host_form, n, rep.status(), rep.summary());
  else
    hipLaunchKernelGGL(k_g2_check, dim3((unsigned)rep.blocks), dim3(PT_G2_BLOCK), 0, C->stream, d_src, stride, host_form, n, rep.status(), rep.summary());
  return rep.read(C, status_or_null, first_bad, ok);
}

int check_host(int group, const void* points, size_t stride, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok) {
  GM_CTX();
  const size_t rec = group == 1 ? 96 : 192;
  GM_CHECK(ok != nullptr && (points != nullptr || n == 0), GM_EINVAL, "g%d_check: null pointer", group);
  GM_CHECK(stride >= rec && stride % 8 == 0, GM_EINVAL, "g%d_check: stride %zu must be >= %zu and a multiple of 8", group, stride, rec);
  GM_CHECK(n <= SIZE_MAX / stride, GM_EINVAL, "g%d_check: %zu records of %zu bytes do not fit a size_t", group, n, stride);
  GM_MSM_LOCK(C);
  DevTmp stage;
  if (n) {
    GM_HIP(dev_malloc(&stage.p, n * stride));
    GM_HIP(hipMemcpyAsync(stage.p, points, n * stride, hipMemcpyHostToDevice, C->stream));
  }
  return check_run(C, group, static_cast<const uint8_t*>(stage.p), stride, 1, n, status_or_null, first_bad, ok);
}

}  // namespace
}  // namespace gm

using namespace gm;

extern "C" {

int gm_g1_check(const void* points, size_t stride, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok) {
  if (ok) *ok = 0;  // every entry of this block fails closed: whatever the return value, *ok is 1 only after a pass that accepted every point
  return check_host(1, points, stride, n, status_or_null, first_bad, ok);
}
int gm_g2_check(const void* points, size_t stride, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok) {
  if (ok) *ok = 0;
  return check_host(2, points, stride, n, status_or_null, first_bad, ok);
}

int gm_g1_bases_check(uint64_t handle, size_t offset, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok) {
  if (ok) *ok = 0;
  GM_CTX();
  Bases* b = find_bases(handle);
  GM_CHECK(b != nullptr, GM_EHANDLE, "g1_bases_check: unknown handle %llu", (unsigned long long)handle);
  GM_CHECK(ok != nullptr, GM_EINVAL, "g1_bases_check: null pointer");
  GM_CHECK(offset <= b->n && n <= b->n - offset, GM_EINVAL, "g1_bases_check: range [%zu, %zu) outside %zu bases", offset, offset + n, b->n);
  GM_MSM_LOCK(C);
  return check_run(C, 1, b->d + offset * 96, 96, 0, n, status_or_null, first_bad, ok);
}
int gm_g2_bases_check(uint64_t handle, size_t offset, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok) {
  if (ok) *ok = 0;
  GM_CTX();
  G2Bases* b = find_in(C, C->g2_bases, handle);
  GM_CHECK(b != nullptr, GM_EHANDLE, "g2_bases_check: unknown G2 bases handle %llu", (unsigned long long)handle);
  GM_CHECK(ok != nullptr, GM_EINVAL, "g2_bases_check: null pointer");
  GM_CHECK(offset <= b->n && n <= b->n - offset, GM_EINVAL, "g2_bases_check: range [%zu, %zu) outside %zu bases", offset, offset + n, b->n);
  GM_MSM_LOCK(C);
  return check_run(C, 2, b->d + offset * G2_AFF_BYTES, G2_AFF_BYTES, 0, n, status_or_null, first_bad, ok);
}

int gm_g1_bases_from_bytes(const uint8_t* bytes, size_t n, int compressed, int encoding, int validate, uint64_t* handle, uint8_t* status_or_null, size_t* first_bad,
                           int* ok) {
  if (ok) *ok = 0;  // before anything can return: a negative code never comes with a stale 1 or a stale handle
  if (handle) *handle = 0;
  GM_CTX();
  GM_CHECK(handle != nullptr && ok != nullptr && (bytes != nullptr || n == 0), GM_EINVAL, "g1_bases_from_bytes: null pointer");
  GM_CHECK(encoding == 0 || encoding == 1, GM_EINVAL, "g1_bases_from_bytes: encoding %d (0 arkworks, 1 zcash)", encoding);
  GM_CHECK(n <= SIZE_MAX / 96, GM_EINVAL, "g1_bases_from_bytes: %zu points do not fit a size_t", n);
  auto b = std::make_unique<Bases>();
  b->n = n;
  int rc = GM_OK;
  if (first_bad) *first_bad = 0;
  if (n) {
    GM_MSM_LOCK(C);
    const size_t sz = compressed ? 48 : 96;
    DevTmp stage, out;
    Report rep;
    if ((rc = rep.alloc(n, PT_BLOCK))) return rc;
    GM_HIP(dev_malloc(&stage.p, n * sz));
    GM_HIP(dev_malloc(&out.p, n * 96));
    GM_HIP(hipMemcpyAsync(stage.p, bytes, n * sz, hipMemcpyHostToDevice, C->stream));
    hipLaunchKernelGGL(k_g1_decode, dim3((unsigned)rep.blocks), dim3(PT_BLOCK), 0, C->stream, static_cast<const uint8_t*>(stage.p), n, compressed ? 1 : 0, encoding,
                       validate ? 1 : 0, static_cast<uint8_t*>(out.p), rep.status(), rep.summary());
    if ((rc = rep.read(C, status_or_null, first_bad, ok))) return rc;
    if (!*ok) return GM_OK;  // a bad point is a result: nothing stays registered
    b->d = static_cast<uint8_t*>(out.p);
    out.p = nullptr;
  }
  if ((rc = bases_build_phi(C, b.get()))) {
    if (b->d) (void)raw_free(b->d);
    *ok = 0;
    return rc;
  }
  *handle = put_bases(std::move(b));  // as gm_g1_bases_register: no tables here, gm_g1_bases_precompute(handle, -1) builds them
  *ok = 1;
  return GM_OK;
}

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
