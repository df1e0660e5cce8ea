// G2 multi-scalar multiplication and the G2 fold kernel of the herring provers (herring.hip) for gfx950.
//
// Replaces `P::G2::msm_unchecked` (Crs::commit_g2 / CrsStream::commit_g2, src/herring/ipa.rs:107-118,185-189; G2Module::ip,
// src/herring/module.rs:114-124) and the split_fold of TimeProver<G2Module> (src/herring/time_prover.rs:72-76).  Signed-digit bucket method with
// the semantics of VariableBaseMSM::msm_bigint, as the G1 engine of msm.hip:
//
//   1. msm_sort_plain   (msm.hip) scalars -> signed c-bit digits -> entries (bucket, sign, pair index) grouped by bucket: the digit
//                       kernels, the counting sorts and the scans are group-agnostic and shared with G1 (of the block sort the
//                       direct scatter kernels, not the LDS-staged ones G1 takes by default)
//   2. k_g2_acc         lane t sums the 192-byte bases of entries [t L, (t + 1) L) into an XYZZ accumulator over Fq2, run by run.
//                       Work per lane is L mixed additions whatever the digit distribution.  Runs interior to a chunk are complete
//                       buckets; the first and the last run of a chunk are written as chunk partials (head / tail)
//   3. k_g2_merge       one lane per bucket that crosses a chunk boundary adds the partials of the chunks it spans; empty buckets
//                       are written as the identity, so no buffer is cleared.  A bucket that spans many chunks -- every scalar
//                       equal, or the few buckets of a top window that holds two bits -- goes to a whole wave (k_g2_merge_long)
//   4. k_g2_reduce      per-window running sum, sum_b (b + 1) B_b, in levels of 8: a lane runs the classic running sum over 8
//                       neighbours and hands (segment total, weighted segment sum) to the next level, which weighs the totals by
//                       8 x as much.  ceil((c - 1) / 3) launches instead of 2^(c-1) sequential additions per window
//   5. host             window sums -> Jacobian, Horner over the windows (variable_base.rs:168-175), normalisation (host_field.hpp)
//
// Also here: the generation of a G2 key from scalars (gm_g2_fixed_base_register, gm_g2_srs_register; the `powers_of_g2` loop of
// CommitterKey::new, src/kzg/time.rs:60-67) -- a fixed-base table of 32 x 256 multiples, one lane per scalar, batched normalisation.
//
// Out of scope here: fixed-base tables for the MSM, GLV, streams, batches, sharding.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "ctx.hpp"
#include "g2.cuh"
#include "host_field.hpp"

namespace gm {

// ------------------------------------------------------------------------------------------
// bases import / export
// ------------------------------------------------------------------------------------------
// staging (stride >= 192, optional infinity flag at byte 192, ark-ff Montgomery form) -> packed 192-byte records in the
// device form (g1.cuh: a * 2^390)
__global__ void k_g2_pack_bases(const uint8_t* __restrict__ src, size_t stride, size_t n, uint8_t* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src + i * stride);
  const bool inf = stride >= 193 && src[i * stride + 192] != 0;
  for (int e = 0; e < 4; e++) {
    Fq v;
#pragma unroll
    for (int k = 0; k < 12; k++) v.l[k] = inf ? 0u : s[12 * e + k];
    fqe_store(dst + i * G2_AFF_BYTES + 48 * e, fqe_import(v));
  }
}
// device form -> ark-ff Montgomery form, 192-byte records (gm_g2_bases_download)
__global__ void k_g2_export_bases(const uint8_t* __restrict__ src, size_t n, uint8_t* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int e = 0; e < 4; e++) fp_store<FqParams>(dst + i * G2_AFF_BYTES + 48 * e, fqe_export(fqe_load(src + i * G2_AFF_BYTES + 48 * e)));
}

// ------------------------------------------------------------------------------------------
// k_g2_acc: chunk-per-lane accumulation of sorted entries
//
// Registers: an XYZZ accumulator over Fq2 is 8 x 12 = 96 VGPRs, the gathered base 48 more, and a mixed addition keeps up to six
// Fq2 temporaries alive across the out-of-line Fq product.  One wave per SIMD owns the whole 512-entry VGPR + AGPR file, which
// holds all of it without scratch (profiles/g2_kernel_resources.txt).
// ------------------------------------------------------------------------------------------
constexpr int G2_ACC_BLOCK = 64;
__global__ __launch_bounds__(G2_ACC_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_g2_acc(
    const uint64_t* __restrict__ entries, const uint32_t* __restrict__ total_ptr, uint32_t L, const uint8_t* __restrict__ bases, long long first,
    long long step, uint8_t* __restrict__ buckets, uint8_t* __restrict__ part) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t total = *total_ptr;
  const uint64_t lo = (uint64_t)t * L;
  if (lo >= total) return;
  const uint64_t hi = lo + L < total ? lo + L : total;
  G2Xyzz acc = G2Xyzz::identity();
  uint32_t cur = (uint32_t)(entries[lo] >> 32);
  bool first_run = true;
  for (uint64_t e = lo; e < hi; e++) {
    const uint64_t en = entries[e];
    const uint32_t key = (uint32_t)(en >> 32);
    if (key != cur) {  // the run of bucket `cur` ends inside this chunk: the chunk's head, or a complete bucket
      g2_store_xyzz(first_run ? part + (size_t)(2 * (uint64_t)t) * G2_XYZZ_BYTES : buckets + (size_t)cur * G2_XYZZ_BYTES, acc);
      first_run = false;
      acc = G2Xyzz::identity();
      cur = key;
    }
    const long long idx = first + step * (long long)((uint32_t)en & 0x7fffffffu);
    G2Affine p = g2_load_affine(bases + (size_t)idx * G2_AFF_BYTES);
    if ((uint32_t)en >> 31) p = g2_neg_affine(p);
    g2_madd(acc, p);
  }
  g2_store_xyzz(part + (size_t)(2 * (uint64_t)t + (first_run ? 0 : 1)) * G2_XYZZ_BYTES, acc);  // a chunk of one run has a head only
}

// Bucket b holds entries [s, e) = [offsets[b], offsets[b + 1]) and so spans chunks t0 = s / L .. t1 = (e - 1) / L.  Its run in
// chunk t is that chunk's FIRST run iff s <= t L (head), else its LAST run iff it reaches the end of the chunk (tail), else it lies
// strictly inside one chunk and k_g2_acc has written the bucket itself.
// A bucket that spans more than G2_MERGE_LONG chunks is put on `long_list` ([0]: how many, then the bucket indices) instead.
constexpr uint32_t G2_MERGE_LONG = 16;
__global__ __launch_bounds__(64) void k_g2_merge(const uint32_t* __restrict__ offsets, uint32_t nbuckets, uint32_t L, const uint8_t* __restrict__ part,
                                                 uint8_t* __restrict__ buckets, uint32_t* __restrict__ long_list) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nbuckets) return;
  const uint64_t s = offsets[b], e = offsets[b + 1], total = offsets[nbuckets];
  uint8_t* out = buckets + (size_t)b * G2_XYZZ_BYTES;
  if (s == e) {
    g2_store_xyzz(out, G2Xyzz::identity());
    return;
  }
  const uint64_t t0 = s / L, t1 = (e - 1) / L;
  const uint64_t c_end = (t0 + 1) * L < total ? (t0 + 1) * L : total;
  if (t0 == t1 && s > t0 * L && e < c_end) return;
  if (t1 - t0 >= G2_MERGE_LONG) {
    long_list[1 + atomicAdd(long_list, 1u)] = b;
    return;
  }
  G2Xyzz acc = G2Xyzz::identity();
  for (uint64_t t = t0; t <= t1; t++) {
    const G2Xyzz p = g2_load_xyzz(part + (size_t)(2 * t + (s <= t * L ? 0 : 1)) * G2_XYZZ_BYTES);
    g2_add(acc, p);
  }
  g2_store_xyzz(out, acc);
}

GM_DEV Fq2 fq2_shfl_xor(const Fq2& a, int m) {
  Fq2 r;
#pragma unroll
  for (int i = 0; i < Fq::N; i++) {
    r.c0.l[i] = __shfl_xor(a.c0.l[i], m);
    r.c1.l[i] = __shfl_xor(a.c1.l[i], m);
  }
  return r;
}
// one wave per listed bucket: lane l adds the partials of chunks t0 + l, t0 + l + 64, ..., then a butterfly over the lanes
__global__ __launch_bounds__(64) void k_g2_merge_long(const uint32_t* __restrict__ offsets, uint32_t L, const uint8_t* __restrict__ part,
                                                      const uint32_t* __restrict__ long_list, uint8_t* __restrict__ buckets) {
  if (blockIdx.x >= long_list[0]) return;
  const uint32_t b = long_list[1 + blockIdx.x];
  const uint64_t s = offsets[b], e = offsets[b + 1];
  const uint64_t t0 = s / L, t1 = (e - 1) / L;
  G2Xyzz acc = G2Xyzz::identity();
  for (uint64_t t = t0 + threadIdx.x; t <= t1; t += 64) {
    const G2Xyzz p = g2_load_xyzz(part + (size_t)(2 * t + (s <= t * L ? 0 : 1)) * G2_XYZZ_BYTES);
    g2_add(acc, p);
  }
  for (int m = 32; m >= 1; m >>= 1) {
    G2Xyzz o;
    o.x = fq2_shfl_xor(acc.x, m);
    o.y = fq2_shfl_xor(acc.y, m);
    o.zz = fq2_shfl_xor(acc.zz, m);
    o.zzz = fq2_shfl_xor(acc.zzz, m);
    g2_add(acc, o);
  }
  if (threadIdx.x == 0) g2_store_xyzz(buckets + (size_t)b * G2_XYZZ_BYTES, acc);
}

// One level of the per-window bucket reduction.  Invariant over the levels, for every window:
//   sum_b (b + 1) B_b = sum_j T_j + sum_j U_j + scale * sum_j j T_j          (level 0: T = the buckets, no U, scale = 1)
// A lane takes segment s = [8 s, 8 s + 8) of T: with u = sum_i i T_{8 s + i} (running sum), sum_j j T_j = sum_s u_s +
// 8 sum_s s T'_s for T'_s = the segment total -- so T' = segment totals, U'_s = scale u_s + the segment's U, scale' = 8 scale.
// (Every lane is a chain of dependent additions at one wave per SIMD, ~25 at 8 per segment against ~50 at 16: shorter levels
// win although there are more of them.)
// One segment left: the window sum is T'_0 + U'_0 (added by the host).
constexpr int G2_RED_LOG = 3;
constexpr uint32_t G2_RED_M = 1u << G2_RED_LOG;
__global__ __launch_bounds__(64) void k_g2_reduce(const uint8_t* __restrict__ Tin, const uint8_t* __restrict__ Uin, uint32_t K, uint32_t W, int log2scale,
                                                  uint8_t* __restrict__ Tout, uint8_t* __restrict__ Uout) {
  const uint32_t Kp = (K + G2_RED_M - 1) / G2_RED_M;
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= W * Kp) return;
  const uint32_t w = gid / Kp, s = gid - w * Kp;
  const uint32_t base = s * G2_RED_M, cnt = K - base < G2_RED_M ? K - base : G2_RED_M;
  const uint8_t* T = Tin + ((size_t)w * K + base) * G2_XYZZ_BYTES;
  G2Xyzz run = G2Xyzz::identity(), acc = G2Xyzz::identity();
  for (uint32_t i = cnt - 1; i >= 1; i--) {
    g2_add(run, g2_load_xyzz(T + (size_t)i * G2_XYZZ_BYTES));
    g2_add(acc, run);
  }
  for (int k = 0; k < log2scale; k++) acc = g2_dbl(acc);
  g2_add(run, g2_load_xyzz(T));
  if (Uin != nullptr) {
    const uint8_t* U = Uin + ((size_t)w * K + base) * G2_XYZZ_BYTES;
    for (uint32_t i = 0; i < cnt; i++) g2_add(acc, g2_load_xyzz(U + (size_t)i * G2_XYZZ_BYTES));
  }
  g2_store_xyzz(Tout + ((size_t)w * Kp + s) * G2_XYZZ_BYTES, run);
  g2_store_xyzz(Uout + ((size_t)w * Kp + s) * G2_XYZZ_BYTES, acc);
}

// herring split_fold over G2 (src/herring/time_prover.rs:72-76): out[i] = P[2i] + s * P[2i+1] (an odd tail: P[2i] alone), affine
// out.  s: canonical scalar, 8 x u32.  One lane per output: 255-bit double-and-add, one addition, one inversion.
__global__ __launch_bounds__(64) void k_g2_split_fold(const uint8_t* __restrict__ in, size_t n, const uint32_t* __restrict__ s8, uint8_t* __restrict__ out) {
  const size_t m = (n + 1) / 2;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  G2Xyzz acc = G2Xyzz::identity();
  if (2 * i + 1 < n) {
    const G2Affine hi = g2_load_affine(in + (2 * i + 1) * G2_AFF_BYTES);
    for (int bit = 254; bit >= 0; bit--) {
      acc = g2_dbl(acc);
      if ((s8[bit >> 5] >> (bit & 31)) & 1u) g2_madd(acc, hi);
    }
  }
  g2_madd(acc, g2_load_affine(in + (2 * i) * G2_AFF_BYTES));
  g2_store_affine(out + i * G2_AFF_BYTES, g2_to_affine(acc));
}

// ------------------------------------------------------------------------------------------
// fixed-base generation: out[i] = k_i * base (gm_g2_fixed_base_register, gm_g2_srs_register) -- the twins of k_fixed_base_table,
// k_fixed_base_mul and k_xyzz_to_affine_batch of msm.hip over Fq2.  Registers: profiles/keygen_kernel_resources.txt.
// ------------------------------------------------------------------------------------------
constexpr int G2_FB_BLOCK = 64;
// table[w][d] = d * 2^(8 w) * base, one lane per (w, d): the bits of d from the top, then 8 w doublings
__global__ __launch_bounds__(G2_FB_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_g2_fixed_base_table(const uint8_t* __restrict__ base, uint8_t* __restrict__ table) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 32 * 256) return;
  const uint32_t w = t >> 8, dgt = t & 255u;
  const G2Affine b = g2_load_affine(base);
  G2Xyzz acc = G2Xyzz::identity();
  for (int bit = 7; bit >= 0; bit--) {
    acc = g2_dbl(acc);
    if ((dgt >> bit) & 1u) g2_madd(acc, b);
  }
  for (uint32_t k = 0; k < 8 * w; k++) acc = g2_dbl(acc);
  g2_store_xyzz(table + (size_t)t * G2_XYZZ_BYTES, acc);
}

// one lane per scalar: at most 32 mixed additions against the affine table.  scalars canonical (mont = 0: any 256-bit value, taken as
// that integer) or Montgomery
__global__ __launch_bounds__(G2_FB_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_g2_fixed_base_mul(const uint32_t* __restrict__ scalars, int mont, size_t n,
                                                                                                              const uint8_t* __restrict__ table_aff, uint8_t* __restrict__ out_xyzz) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr s = fp_load<FrParams>(scalars + 8 * i);
  if (mont) s = fp_from_mont<FrParams>(s);
  G2Xyzz acc = G2Xyzz::identity();
  for (int w = 0; w < 32; w++) {
    const uint32_t dgt = (s.l[w >> 2] >> (8 * (w & 3))) & 255u;
    if (dgt) g2_madd(acc, g2_load_affine(table_aff + ((size_t)w * 256 + dgt) * G2_AFF_BYTES));
  }
  g2_store_xyzz(out_xyzz + i * G2_XYZZ_BYTES, acc);  // normalised in groups by k_g2_xyzz_to_affine_batch
}

// Batched normalisation, Montgomery's trick inside a lane over Fq2: prefix products of t_k = zz_k zzz_k, ONE inversion -- in Fq, of the
// norm (fq2_inv) -- and the back-substitution, per group of G2_NORM_K points.  Point k of the group is in[idx ? idx[i0 + k] : i0 + k];
// identity records (zz = 0) stay out of the products and give the all-zero affine record.
// The prefix products wait in the first 96 bytes of the group's own OUTPUT records -- record k is read back before record k + 1 is
// written over --, not in a register array: eight Fq2 prefixes are 192 VGPRs a lane would hold across the inversion.
constexpr int G2_NORM_K = 8;
__global__ __launch_bounds__(G2_FB_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_g2_xyzz_to_affine_batch(const uint8_t* __restrict__ in, const uint32_t* __restrict__ idx, size_t n,
                                                                                                                    uint8_t* out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i0 = t * G2_NORM_K;
  if (i0 >= n) return;
  const int m = (int)min((size_t)G2_NORM_K, n - i0);
  Fq2 run = fq2_one();
  for (int k = 0; k < m; k++) {
    const uint8_t* rec = in + (size_t)(idx ? idx[i0 + k] : i0 + k) * G2_XYZZ_BYTES;
    const Fq2 zz = fq2_load(rec + 192);
    if (!fq2_is_zero(zz)) run = fq2_mul(run, fq2_mul(zz, fq2_load(rec + 288)));
    fq2_store(out + (i0 + k) * G2_AFF_BYTES, run);
  }
  Fq2 inv = fq2_inv(run);
  for (int k = m - 1; k >= 0; k--) {
    const uint8_t* rec = in + (size_t)(idx ? idx[i0 + k] : i0 + k) * G2_XYZZ_BYTES;
    const Fq2 zz = fq2_load(rec + 192);
    G2Affine a;
    a.x = fq2_zero();
    a.y = fq2_zero();
    if (!fq2_is_zero(zz)) {
      const Fq2 zzz = fq2_load(rec + 288);
      const Fq2 ti = k ? fq2_mul(inv, fq2_load(out + (i0 + k - 1) * G2_AFF_BYTES)) : inv;  // 1 / (zz zzz)
      inv = fq2_mul(inv, fq2_mul(zz, zzz));
      a.x = fq2_mul(fq2_load(rec), fq2_mul(ti, zzz));
      a.y = fq2_mul(fq2_load(rec + 96), fq2_mul(ti, zz));
    }
    g2_store_affine(out + (i0 + k) * G2_AFF_BYTES, a);
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// window width: n W mixed additions against W 2^(c-1) buckets to merge and reduce.  Not tuned beyond these three steps
// (profiles/g2_msm.md); tests/test_gpu_g2.py reads the thresholds from here.
constexpr size_t G2_C8_MIN_N = 65;                       // below: c = 4
constexpr size_t G2_C12_MIN_N = 4097;                    // below: c = 8
constexpr size_t G2_C16_MIN_N = ((size_t)1 << 17) + 1;   // below: c = 12
static int g2_choose_window(size_t n) { return n >= G2_C16_MIN_N ? 16 : n >= G2_C12_MIN_N ? 12 : n >= G2_C8_MIN_N ? 8 : 4; }
constexpr uint64_t G2_ACC_LANES = 65536;  // one 64-lane wave on each of 4 x 256 SIMDs
constexpr uint64_t G2_ACC_L_MIN = 4, G2_ACC_L_MAX = 1024;
// Longer calls are cut into pieces of this many pairs whose results are added on the host (n W < 2^32 entries, 26-bit pair
// indices) -- the composition msm_run uses for G1.  GM_G2_CALL_MAX_N (read at every call) lowers the cut: that is how the suite
// runs both sides of it at a few hundred pairs (tests/test_gpu_g2.py::test_call_cut).
constexpr size_t G2_CALL_MAX_N = (size_t)1 << 25;
static size_t g2_call_max_n() {
  const char* e = getenv("GM_G2_CALL_MAX_N");
  const size_t v = e ? (size_t)strtoull(e, nullptr, 10) : 0;
  return v >= 1 && v < G2_CALL_MAX_N ? v : G2_CALL_MAX_N;
}

void g2_workspace_release(G2Workspace& w) {
  for (DevBuf* b : {&w.buckets, &w.part, &w.red[0], &w.red[1], &w.longs}) b->release();
  if (w.host_out) (void)hipHostFree(w.host_out);
  w.host_out = nullptr;
  w.host_out_cap = 0;
}

static int g2_msm_run_one(Context* C, const G2Bases* bases, int64_t first, int64_t step, const void* d_scalars, int mont, size_t n, gmh::G2* result) {
  hipStream_t st = C->stream;
  G2Workspace& ws = C->g2;
  const int64_t last = first + step * (int64_t)(n - 1);
  GM_CHECK(first >= 0 && last >= 0 && (size_t)first < bases->n && (size_t)last < bases->n, GM_EINVAL,
           "g2 msm: base range [%lld .. %lld] outside registered bases (len %zu)", (long long)first, (long long)last, bases->n);
  const int c = g2_choose_window(n);
  Profiler& pf = C->prof;
  MsmSorted S;
  pf.begin(PROF_DIGITS, st);
  int rc = msm_sort_plain(C, C->msm, st, d_scalars, mont, n, c, &S);
  pf.end(PROF_DIGITS, st);
  if (rc) return rc;
  const uint32_t W = (uint32_t)S.W, B = S.B;
  const uint64_t N = (uint64_t)n * W;  // upper bound of the entry count (zero digits have no entry)
  const uint32_t L = (uint32_t)std::min<uint64_t>(G2_ACC_L_MAX, std::max<uint64_t>(G2_ACC_L_MIN, (N + G2_ACC_LANES - 1) / G2_ACC_LANES));
  const uint64_t T = (N + L - 1) / L;
  const uint32_t K1 = (B + G2_RED_M - 1) / G2_RED_M;
  if ((rc = ws.buckets.ensure(S.nbuckets * G2_XYZZ_BYTES))) return rc;
  if ((rc = ws.part.ensure(2 * T * G2_XYZZ_BYTES))) return rc;
  // a listed bucket owns the >= G2_MERGE_LONG - 1 chunks strictly inside its span: at most T / (G2_MERGE_LONG - 1) of them
  const uint32_t max_long = (uint32_t)(T / (G2_MERGE_LONG - 1) + 1);
  if ((rc = ws.longs.ensure(((size_t)max_long + 1) * 4))) return rc;
  GM_HIP(hipMemsetAsync(ws.longs.p, 0, 4, st));
  for (DevBuf& r : ws.red)
    if ((rc = r.ensure((size_t)2 * W * K1 * G2_XYZZ_BYTES))) return rc;
  const size_t out_words = (size_t)2 * 64 * (G2_XYZZ_BYTES / 8) + 1;  // c >= 4: at most 64 windows; + the scalar-range flag
  if (!ws.host_out) {
    GM_HIP(hipHostMalloc((void**)&ws.host_out, out_words * 8, hipHostMallocDefault));
    ws.host_out_cap = out_words;
  }
  pf.begin(PROF_ACC0, st);
  hipLaunchKernelGGL(k_g2_acc, dim3((uint32_t)((T + G2_ACC_BLOCK - 1) / G2_ACC_BLOCK)), dim3(G2_ACC_BLOCK), 0, st, S.entries, S.offsets + S.nbuckets, L, bases->d,
                     (long long)first, (long long)step, ws.buckets.as<uint8_t>(), ws.part.as<uint8_t>());
  pf.end(PROF_ACC0, st);
  pf.begin(PROF_MERGE, st);
  hipLaunchKernelGGL(k_g2_merge, dim3((uint32_t)((S.nbuckets + 63) / 64)), dim3(64), 0, st, S.offsets, (uint32_t)S.nbuckets, L, ws.part.as<uint8_t>(),
                     ws.buckets.as<uint8_t>(), ws.longs.as<uint32_t>());
  hipLaunchKernelGGL(k_g2_merge_long, dim3(max_long), dim3(64), 0, st, S.offsets, L, ws.part.as<uint8_t>(), ws.longs.as<uint32_t>(), ws.buckets.as<uint8_t>());
  pf.end(PROF_MERGE, st);
  pf.begin(PROF_REDUCE, st);
  const uint8_t *Tin = ws.buckets.as<uint8_t>(), *Uin = nullptr;
  uint32_t K = B;
  int level = 0;
  for (;; level++) {
    const uint32_t Kp = (K + G2_RED_M - 1) / G2_RED_M;
    uint8_t* Tout = ws.red[level & 1].as<uint8_t>();
    uint8_t* Uout = Tout + (size_t)W * Kp * G2_XYZZ_BYTES;
    hipLaunchKernelGGL(k_g2_reduce, dim3((W * Kp + 63) / 64), dim3(64), 0, st, Tin, Uin, K, W, G2_RED_LOG * level, Tout, Uout);
    Tin = Tout;
    Uin = Uout;
    K = Kp;
    if (K == 1) break;
  }
  pf.end(PROF_REDUCE, st);
  GM_HIP(hipGetLastError());
  // T'_0 and U'_0 of every window lie back to back: one copy, and the scalar-range flag behind it
  GM_HIP(hipMemcpyAsync(ws.host_out, Tin, (size_t)2 * W * G2_XYZZ_BYTES, hipMemcpyDeviceToHost, st));
  GM_HIP(hipMemcpyAsync(ws.host_out + (size_t)2 * W * (G2_XYZZ_BYTES / 8), S.err, 4, hipMemcpyDeviceToHost, st));
  GM_HIP(hipStreamSynchronize(st));
  pf.collect();
  const uint32_t bad = *reinterpret_cast<const uint32_t*>(ws.host_out + (size_t)2 * W * (G2_XYZZ_BYTES / 8));
  GM_CHECK(bad == 0, GM_EINVAL, "g2 msm: a scalar passed as a canonical integer is >= 2^255 (not the BigInt image of an Fr element)");
  gmh::G2 acc = gmh::G2::identity();
  for (int w = (int)W - 1; w >= 0; w--) {
    for (int k = 0; k < c; k++) acc = acc.dbl();
    acc = acc.add(gmh::g2_xyzz_to_jac_dev(ws.host_out + (size_t)w * (G2_XYZZ_BYTES / 8)));
    acc = acc.add(gmh::g2_xyzz_to_jac_dev(ws.host_out + (size_t)(W + w) * (G2_XYZZ_BYTES / 8)));
  }
  *result = acc;
  return GM_OK;
}

// sum_i scalars[i] * bases[first + step i], normalised
int g2_msm_run(Context* C, const G2Bases* bases, int64_t first, int64_t step, const void* d_scalars, int mont, size_t n, uint64_t out_jac[36]) {
  GM_MSM_LOCK(C);  // the sort buffers are the G1 workspace's, the G2 buffers single-flight like them
  gmh::G2 acc = gmh::G2::identity();
  const size_t cut = g2_call_max_n();
  for (size_t off = 0; off < n; off += cut) {
    const size_t m = std::min(n - off, cut);
    gmh::G2 part;
    int rc = g2_msm_run_one(C, bases, first + step * (int64_t)off, step, reinterpret_cast<const uint8_t*>(d_scalars) + off * 32, mont, m, &part);
    if (rc) return rc;
    acc = acc.add(part);
  }
  acc.normalized().to_limbs(out_jac);
  return GM_OK;
}

// ---- bases management -----------------------------------------------------------------------
int g2_bases_from_host(Context* C, const void* bases, size_t stride, size_t n, std::unique_ptr<G2Bases>& out) {
  GM_CHECK(stride >= (size_t)G2_AFF_BYTES && (stride % 8) == 0, GM_EINVAL, "g2 bases: stride %zu must be >= 192 and a multiple of 8", stride);
  auto b = std::make_unique<G2Bases>();
  b->n = n;
  if (n) {
    uint8_t* stage = nullptr;
    GM_HIP(dev_malloc((void**)&b->d, n * G2_AFF_BYTES));
    hipError_t e = dev_malloc((void**)&stage, n * stride);
    if (e == hipSuccess) e = hipMemcpyAsync(stage, bases, n * stride, hipMemcpyHostToDevice, C->stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_g2_pack_bases, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, C->stream, stage, stride, n, b->d);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(C->stream);
    if (stage) (void)gm::raw_free(stage);
    if (e != hipSuccess) {
      (void)gm::raw_free(b->d);
      return hip_fail(e, "g2 bases upload", __FILE__, __LINE__);
    }
  }
  out = std::move(b);
  return GM_OK;
}

int g2_bases_export(Context* C, const G2Bases* b, size_t offset, size_t n, void* out192) {
  if (n == 0) return GM_OK;
  uint8_t* tmp = nullptr;
  GM_HIP(dev_malloc((void**)&tmp, n * G2_AFF_BYTES));
  hipLaunchKernelGGL(k_g2_export_bases, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, C->stream, b->d + offset * G2_AFF_BYTES, n, tmp);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out192, tmp, n * G2_AFF_BYTES, hipMemcpyDeviceToHost, C->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(C->stream);
  (void)gm::raw_free(tmp);
  return e == hipSuccess ? GM_OK : hip_fail(e, "g2 bases download", __FILE__, __LINE__);
}

// n XYZZ records (d_idx != nullptr: the records d_idx[0 .. n) of `in`) -> packed affine records, on C->stream without a wait
int g2_normalise_launch(Context* C, const uint8_t* in, const uint32_t* d_idx, size_t n, uint8_t* out) {
  if (n == 0) return GM_OK;
  const size_t groups = (n + G2_NORM_K - 1) / G2_NORM_K;
  hipLaunchKernelGGL(k_g2_xyzz_to_affine_batch, dim3((unsigned)((groups + G2_FB_BLOCK - 1) / G2_FB_BLOCK)), dim3(G2_FB_BLOCK), 0, C->stream, in, d_idx, n, out);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

namespace {
struct G2Tmp {  // device memory of one call, freed on every path out
  uint8_t* p = nullptr;
  ~G2Tmp() {
    if (p) (void)gm::raw_free(p);
  }
};
}  // namespace

// out[i] = scalars[i] * base, i < n: the affine table (32 x 256 records, 1.5 MB), then slabs of at most 2^22 points -- a multiply
// launch into an XYZZ slab and its normalisation into the key.  d_scalars: n x 32 bytes on the device, ordered on C->stream.
int g2_fixed_base_generate(Context* C, const uint64_t base_affine[24], const void* d_scalars, int mont, size_t n, std::unique_ptr<G2Bases>& out) {
  GM_CHECK(n <= SIZE_MAX / G2_XYZZ_BYTES, GM_EINVAL, "g2 fixed base: %zu points do not fit a size_t", n);
  auto b = std::make_unique<G2Bases>();
  b->n = n;
  if (n) {
    GM_MSM_LOCK(C);
    G2Tmp base, stage, t_xyzz, table, xy, key;
    const size_t T = (size_t)32 * 256;
    GM_HIP(dev_malloc((void**)&base.p, G2_AFF_BYTES));
    GM_HIP(dev_malloc((void**)&stage.p, G2_AFF_BYTES));
    GM_HIP(dev_malloc((void**)&t_xyzz.p, T * G2_XYZZ_BYTES));
    GM_HIP(dev_malloc((void**)&table.p, T * G2_AFF_BYTES));
    GM_HIP(hipMemcpyAsync(stage.p, base_affine, G2_AFF_BYTES, hipMemcpyHostToDevice, C->stream));
    hipLaunchKernelGGL(k_g2_pack_bases, dim3(1), dim3(64), 0, C->stream, stage.p, (size_t)G2_AFF_BYTES, (size_t)1, base.p);
    hipLaunchKernelGGL(k_g2_fixed_base_table, dim3((unsigned)(T / G2_FB_BLOCK)), dim3(G2_FB_BLOCK), 0, C->stream, base.p, t_xyzz.p);
    int rc = g2_normalise_launch(C, t_xyzz.p, nullptr, T, table.p);
    if (rc) return rc;
    const size_t slab = std::min<size_t>(n, (size_t)1 << 22);
    GM_HIP(dev_malloc((void**)&key.p, n * G2_AFF_BYTES));
    GM_HIP(dev_malloc((void**)&xy.p, slab * G2_XYZZ_BYTES));
    for (size_t off = 0; off < n; off += slab) {
      const size_t m = std::min(slab, n - off);
      hipLaunchKernelGGL(k_g2_fixed_base_mul, dim3((unsigned)((m + G2_FB_BLOCK - 1) / G2_FB_BLOCK)), dim3(G2_FB_BLOCK), 0, C->stream,
                         reinterpret_cast<const uint32_t*>(d_scalars) + 8 * off, mont, m, table.p, xy.p);
      if ((rc = g2_normalise_launch(C, xy.p, nullptr, m, key.p + off * G2_AFF_BYTES))) return rc;
    }
    GM_HIP(hipGetLastError());
    GM_HIP(hipStreamSynchronize(C->stream));
    b->d = key.p;
    key.p = nullptr;
  }
  out = std::move(b);
  return GM_OK;
}

// the G2 fold of the herring provers (herring.hip): out[i] = in[2i] + s in[2i+1], s at d_s8 (canonical, 8 x u32), on C->stream
int g2_split_fold_launch(Context* C, const uint8_t* in, size_t n, const uint32_t* d_s8, uint8_t* out) {
  const size_t m = (n + 1) / 2;
  hipLaunchKernelGGL(k_g2_split_fold, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, C->stream, in, n, d_s8, out);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // namespace gm
