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
// Not here: import, export and generation of a G2 key, the G2 fold of the herring provers and the batched normalisation -- bases.hip
// states them once for G1 and G2.  Deliberately not merged with msm.hip: k_g2_acc, k_g2_merge*, k_g2_reduce and the host composition
// below (the G1 engine accumulates in the 30-bit loose form, with tables, GLV and batches).
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

}  // namespace gm
