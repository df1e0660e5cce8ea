// Keys of either group on the device (gfx950), stated once over the group descriptions of groups.cuh and instantiated for G1 and
// G2: import and export of registered bases, the generation of a key from scalars (gm_g1_/gm_g2_fixed_base_register,
// gm_g1_/gm_g2_srs_register; the `powers_of_g` / `powers_of_g2` loops of CommitterKey::new, src/kzg/time.rs:49-72), the split_fold
// of the herring provers (src/herring/time_prover.rs:72-76) and the batched normalisation every one of them ends in.
//
// G1 runs these kernels in blocks of 256, G2 in blocks of 64 at one wave per SIMD (an XYZZ accumulator over Fq2 is 96 VGPRs, the
// gathered base 48 more); registers: profiles/bases_refactor_kernel_resources.txt.
//
// Not here: the MSM engines (msm.hip, g2msm.hip), the window tables of a G1 key and the GLV images (msm.hip: k_table_next,
// k_phi_bases), the short linear combinations (msm.hip: k_g1_term_mul, k_g1_seg_sum).
#include <algorithm>

#include "groups.cuh"
#include "host_field.hpp"

namespace gm {

// staging (stride >= AFF_BYTES, optional infinity flag behind the coordinates, ark-ff Montgomery form) -> packed records in the
// device form (g1.cuh: a * 2^390)
template <class G>
__global__ void k_pack_bases(const uint8_t* __restrict__ src, size_t stride, size_t n, uint8_t* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src + i * stride);
  const bool inf = stride > G::AFF_BYTES && src[i * stride + G::AFF_BYTES] != 0;
  for (int e = 0; e < 2 * G::NC; e++) {
    Fq v;
#pragma unroll
    for (int k = 0; k < 12; k++) v.l[k] = inf ? 0u : s[12 * e + k];
    fqe_store(dst + i * G::AFF_BYTES + 48 * e, fqe_import(v));
  }
}
// device form -> ark-ff Montgomery form, packed records (gm_g1_bases_download, gm_g2_bases_download)
template <class G>
__global__ void k_export_bases(const uint8_t* __restrict__ src, size_t n, uint8_t* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int e = 0; e < 2 * G::NC; e++) fp_store<FqParams>(dst + i * G::AFF_BYTES + 48 * e, fqe_export(fqe_load(src + i * G::AFF_BYTES + 48 * e)));
}

// ---- fixed-base generation: out[i] = k_i * base via 32 windows of 8 bits against a (32 x 256)-entry affine table ----------------
// table[w][d] = d * 2^(8 w) * base, one lane per (w, d): the bits of d from the top, then 8 w doublings
template <class G>
__global__ __launch_bounds__(G::KEY_BLOCK) __attribute__((amdgpu_waves_per_eu(G::KEY_WAVES, G::KEY_WAVES))) void k_fixed_base_table(const uint8_t* __restrict__ base, uint8_t* __restrict__ table) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 32 * 256) return;
  const uint32_t w = t >> 8, dgt = t & 255u;
  const typename G::Affine b = G::load_affine(base);
  typename G::Xyzz acc = G::identity();
  for (int bit = 7; bit >= 0; bit--) {
    acc = G::dbl(acc);
    if ((dgt >> bit) & 1u) G::madd(acc, b);
  }
  for (uint32_t k = 0; k < 8 * w; k++) acc = G::dbl(acc);
  G::store_xyzz(table + (size_t)t * G::XYZZ_BYTES, acc);
}

// one lane per scalar: at most 32 mixed additions against the affine table.  scalars canonical (mont = 0: any 256-bit value, taken as
// that integer) or Montgomery
template <class G>
__global__ __launch_bounds__(G::KEY_BLOCK) __attribute__((amdgpu_waves_per_eu(G::KEY_WAVES, G::KEY_WAVES))) void k_fixed_base_mul(const uint32_t* __restrict__ scalars, int mont, size_t n,
                                                                                                                        const uint8_t* __restrict__ table_aff, uint8_t* __restrict__ out_xyzz) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr s = fp_load<FrParams>(scalars + 8 * i);
  if (mont) s = fp_from_mont<FrParams>(s);
  typename G::Xyzz acc = G::identity();
  for (int w = 0; w < 32; w++) {
    const uint32_t dgt = (s.l[w >> 2] >> (8 * (w & 3))) & 255u;
    if (dgt) G::madd(acc, G::load_affine(table_aff + ((size_t)w * 256 + dgt) * G::AFF_BYTES));
  }
  G::store_xyzz(out_xyzz + i * G::XYZZ_BYTES, acc);  // normalised in groups by k_normalise
}

// herring split_fold: out[i] = P[2i] + s * P[2i+1] (an odd tail: P[2i] alone), affine out.  s: canonical scalar, 8 x u32.  One lane
// per output: 255-bit double-and-add, one addition, one inversion.
template <class G, bool REV = false>
__global__ __launch_bounds__(G::KEY_BLOCK) void k_split_fold(const uint8_t* __restrict__ in, size_t n, const uint32_t* __restrict__ s8, uint8_t* __restrict__ out) {
  const size_t m = (n + 1) / 2;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  // REV: record j of the vector is in[n - 1 - j] (a big-endian stream read as the little-endian vector it stands for)
  const auto at = [&](size_t j) { return in + (REV ? n - 1 - j : j) * G::AFF_BYTES; };
  typename G::Xyzz acc = G::identity();
  if (2 * i + 1 < n) {
    const typename G::Affine hi = G::load_affine(at(2 * i + 1));
    for (int bit = 254; bit >= 0; bit--) {
      acc = G::dbl(acc);
      if ((s8[bit >> 5] >> (bit & 31)) & 1u) G::madd(acc, hi);
    }
  }
  G::madd(acc, G::load_affine(at(2 * i)));
  G::store_affine(out + i * G::AFF_BYTES, grp_to_affine<G>(acc));
}

// out[i] = in[n - 1 - i] over records of 16 q bytes, one lane per 16 bytes
__global__ __launch_bounds__(256) void k_records_reverse(const uint4* __restrict__ in, size_t n, uint32_t q, uint4* __restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * q) return;
  const size_t i = t / q, c = t % q;
  out[t] = in[(n - 1 - i) * q + c];
}

// The segmented form: lane i folds pair i % m of span i / m, m = (n + 1) / 2 -- the spans of many proofs in one launch, each under
// the scalar its table entry names (row `ch` of s8).  Lanes of one wave may belong to spans with different scalars, so the scalar
// is the lane's own (eight registers) and the bit test is per lane: the doublings run in step, an addition runs under the mask of
// the lanes whose bit is set.  (FoldSpan: ctx.hpp.)
template <class G>
__global__ __launch_bounds__(G::KEY_BLOCK) void k_split_fold_seg(const FoldSpan* __restrict__ spans, size_t nspans, size_t n, const uint32_t* __restrict__ s8) {
  const size_t m = (n + 1) / 2;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nspans * m) return;
  const FoldSpan sp = spans[i / m];
  const size_t k = i % m;
  typename G::Xyzz acc = G::identity();
  if (2 * k + 1 < n) {
    uint32_t s[8];
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] = s8[(size_t)sp.ch * 8 + j];
    const typename G::Affine hi = G::load_affine(sp.in + (2 * k + 1) * G::AFF_BYTES);
#pragma unroll 1
    for (int w = 7; w >= 0; w--) {
      uint32_t bits = s[7];  // the top word, then the scalar moves up by one word: no register is indexed by the loop counter
#pragma unroll
      for (int j = 7; j > 0; j--) s[j] = s[j - 1];
#pragma unroll 1
      for (int b = 0; b < 32; b++) {
        acc = G::dbl(acc);
        if (bits >> 31) G::madd(acc, hi);
        bits <<= 1;
      }
    }
  }
  G::madd(acc, G::load_affine(sp.in + (2 * k) * G::AFF_BYTES));
  G::store_affine(sp.out + k * G::AFF_BYTES, grp_to_affine<G>(acc));
}

// ---- short linear combinations over either group (gm_g2_lincomb_many; the module messages of ipa.hip's lockstep prover) -------
// One lane per TERM makes the multiple by the loop of k_split_fold (one XYZZ accumulator and one affine point in the lane), one
// lane per SEGMENT adds its terms up with the complete addition, k_normalise normalises the sums.  A term names its point and its
// scalar through optional index tables, so the terms of many proofs can read vectors where they lie.  (G1's own pair for host
// records, k_g1_term_mul / k_g1_seg_sum of msm.hip, stays as it is.)
template <class G>
__global__ __launch_bounds__(G::KEY_BLOCK) void k_term_mul(const uint8_t* __restrict__ points, const uint32_t* __restrict__ pidx, const uint8_t* __restrict__ scalars,
                                                            const uint32_t* __restrict__ sidx, int mont, size_t nterms, uint8_t* __restrict__ out_xyzz) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nterms) return;
  Fr sc = fp_load<FrParams>(reinterpret_cast<const uint32_t*>(scalars + (size_t)(sidx ? sidx[t] : t) * 32));
  if (mont) sc = fp_from_mont<FrParams>(sc);
  uint32_t s[8];
#pragma unroll
  for (int j = 0; j < 8; j++) s[j] = sc.l[j];
  const typename G::Affine p = G::load_affine(points + (size_t)(pidx ? pidx[t] : t) * G::AFF_BYTES);
  typename G::Xyzz acc = G::identity();
#pragma unroll 1
  for (int w = 7; w >= 0; w--) {
    uint32_t bits = s[7];
#pragma unroll
    for (int j = 7; j > 0; j--) s[j] = s[j - 1];
#pragma unroll 1
    for (int b = 0; b < 32; b++) {
      acc = G::dbl(acc);
      if (bits >> 31) G::madd(acc, p);
      bits <<= 1;
    }
  }
  G::store_xyzz(out_xyzz + t * G::XYZZ_BYTES, acc);
}
// out[s] = the sum of the records [offsets[s], offsets[s + 1]); an empty segment is the identity.  G::add is complete: two equal
// terms double, opposite ones cancel.
template <class G>
__global__ __launch_bounds__(G::KEY_BLOCK) void k_seg_sum(const uint8_t* __restrict__ terms_xyzz, const unsigned long long* __restrict__ offsets, size_t nseg,
                                                           uint8_t* __restrict__ out_xyzz) {
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nseg) return;
  typename G::Xyzz acc = G::identity();
#pragma unroll 1
  for (unsigned long long t = offsets[s]; t < offsets[s + 1]; t++) G::add(acc, G::load_xyzz(terms_xyzz + (size_t)t * G::XYZZ_BYTES));
  G::store_xyzz(out_xyzz + s * G::XYZZ_BYTES, acc);
}

// Batched normalisation, Montgomery's trick inside a lane: prefix products of t_k = zz_k zzz_k, ONE inversion (over Fq2: in Fq, of
// the norm) and the back-substitution, per group of `group` <= NORM_K points -- a Fermat inversion is ~570 products.  Point k of the group is
// in[INDEXED ? idx[i0 + k] : i0 + k]; identity records (zz = 0) stay out of the products and give the all-zero affine record.
// Where the prefix products wait is the description's PREFIX_IN_REGS.  G2: in the first element of the group's own OUTPUT records
// -- record k is read back before record k + 1 is written over --, since eight Fq2 prefixes are 192 VGPRs a lane would hold across
// the inversion.  G1: in an array of the lane, as k_xyzz_to_affine_batch kept them -- parked in the output, the twelve table rows
// of gm_g1_bases_precompute at 2^20 points took 0.4 % and 0.9 % longer in two A/B jobs, above the margin in both
// (profiles/bases_refactor_ab.md) --, but for the indexed instance, which has no registers to spare for the array at its three
// waves and parks them as the candidates gather always did.  Either way `out` must not overlap `in`: the callers normalise a
// scratch slab or table into the key (fixed_base_generate, msm.hip: build_window_table), the region o_sums of C->lincomb into its region o_aff (msm.hip: g1_lincomb_many_launch), the candidate
// slots into the key (points.hip: candidates_run).
template <class G, bool INDEXED>
__global__ __launch_bounds__(G::KEY_BLOCK) __attribute__((amdgpu_waves_per_eu(G::KEY_WAVES, G::KEY_WAVES))) void k_normalise(const uint8_t* __restrict__ in, const uint32_t* __restrict__ idx, size_t n, int group, uint8_t* out) {
  using El = typename G::El;
  constexpr size_t E = G::EL_BYTES;
  constexpr bool IN_REGS = G::PREFIX_IN_REGS && !INDEXED;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i0 = t * group;
  if (i0 >= n) return;
  const int m = (int)min((size_t)group, n - i0);
  El pre[IN_REGS ? NORM_K : 1];
  El run = G::one();
  for (int k = 0; k < m; k++) {
    const uint8_t* rec = in + (size_t)(INDEXED ? idx[i0 + k] : i0 + k) * G::XYZZ_BYTES;
    const El zz = G::el_load(rec + 2 * E);
    if (!G::is_zero(zz)) run = G::mul(run, G::mul(zz, G::el_load(rec + 3 * E)));
    if constexpr (IN_REGS) pre[k] = run;
    else G::el_store(out + (i0 + k) * G::AFF_BYTES, run);
  }
  El inv = G::inv(run);
  for (int k = m - 1; k >= 0; k--) {
    const uint8_t* rec = in + (size_t)(INDEXED ? idx[i0 + k] : i0 + k) * G::XYZZ_BYTES;
    const El zz = G::el_load(rec + 2 * E);
    typename G::Affine a;
    if (G::is_zero(zz)) {
      a.x = G::zero();
      a.y = G::zero();
    } else {
      const El zzz = G::el_load(rec + 3 * E);
      El ti = inv;  // 1 / (zz zzz): the inverse of the product up to here, by the prefix of the points before this one
      if (k) {
        if constexpr (IN_REGS) ti = G::mul(inv, pre[k - 1]);
        else ti = G::mul(inv, G::el_load(out + (i0 + k - 1) * G::AFF_BYTES));
      }
      inv = G::mul(inv, G::mul(zz, zzz));
      a.x = G::mul(G::el_load(rec), G::mul(ti, zzz));
      a.y = G::mul(G::el_load(rec + E), G::mul(ti, zz));
    }
    G::store_affine(out + (i0 + k) * G::AFF_BYTES, a);
  }
}

// ---- host side: launches on the given stream without a wait ------------------------------------------------------------------
template <class G>
int pack_launch(hipStream_t st, const uint8_t* src, size_t stride, size_t n, uint8_t* dst) {
  hipLaunchKernelGGL(k_pack_bases<G>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, stride, n, dst);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
// out[i] = in[2i] + s in[2i+1] over packed affine records, s at d_s8 (canonical, 8 x u32)
template <class G>
int split_fold_launch(hipStream_t st, const uint8_t* in, size_t n, const uint32_t* d_s8, uint8_t* out) {
  const size_t m = (n + 1) / 2;
  hipLaunchKernelGGL(k_split_fold<G>, dim3((unsigned)((m + G::KEY_BLOCK - 1) / G::KEY_BLOCK)), dim3(G::KEY_BLOCK), 0, st, in, n, d_s8, out);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
// the same with the records read backwards (k_split_fold<G, true>)
template <class G>
static int split_fold_rev_launch(hipStream_t st, const uint8_t* in, size_t n, const uint32_t* d_s8, uint8_t* out) {
  const size_t m = (n + 1) / 2;
  hipLaunchKernelGGL((k_split_fold<G, true>), dim3((unsigned)((m + G::KEY_BLOCK - 1) / G::KEY_BLOCK)), dim3(G::KEY_BLOCK), 0, st, in, n, d_s8, out);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
// n XYZZ records (d_idx != nullptr: the records d_idx[0 .. n) of `in`) -> packed affine records, `group` (1 .. NORM_K) to a lane and an
// inversion; `out` apart from `in` (k_normalise)
template <class G>
int normalise_launch(hipStream_t st, const uint8_t* in, const uint32_t* d_idx, size_t n, uint8_t* out, int group) {
  if (n == 0) return GM_OK;
  const size_t groups = (n + group - 1) / group;
  const dim3 grid((unsigned)((groups + G::KEY_BLOCK - 1) / G::KEY_BLOCK)), block(G::KEY_BLOCK);
  if (d_idx) hipLaunchKernelGGL((k_normalise<G, true>), grid, block, 0, st, in, d_idx, n, group, out);
  else hipLaunchKernelGGL((k_normalise<G, false>), grid, block, 0, st, in, d_idx, n, group, out);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

template <class G>
int split_fold_seg_launch(hipStream_t st, const FoldSpan* d_spans, size_t nspans, size_t n, const uint32_t* d_s8) {
  const size_t lanes = nspans * ((n + 1) / 2);
  if (lanes == 0) return GM_OK;
  hipLaunchKernelGGL(k_split_fold_seg<G>, dim3((unsigned)((lanes + G::KEY_BLOCK - 1) / G::KEY_BLOCK)), dim3(G::KEY_BLOCK), 0, st, d_spans, nspans, n, d_s8);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
template <class G>
int term_mul_launch(hipStream_t st, const uint8_t* d_points, const uint32_t* d_pidx, const uint8_t* d_scalars, const uint32_t* d_sidx, int mont, size_t T, uint8_t* d_out) {
  if (T == 0) return GM_OK;
  hipLaunchKernelGGL(k_term_mul<G>, dim3((unsigned)((T + G::KEY_BLOCK - 1) / G::KEY_BLOCK)), dim3(G::KEY_BLOCK), 0, st, d_points, d_pidx, d_scalars, d_sidx, mont, T, d_out);
  GM_HIP(hipGetLastError());
  return GM_OK;
}
template <class G>
int seg_sum_launch(hipStream_t st, const uint8_t* d_in, const unsigned long long* d_off, size_t S, uint8_t* d_out) {
  if (S == 0) return GM_OK;
  hipLaunchKernelGGL(k_seg_sum<G>, dim3((unsigned)((S + G::KEY_BLOCK - 1) / G::KEY_BLOCK)), dim3(G::KEY_BLOCK), 0, st, d_in, d_off, S, d_out);
  GM_HIP(hipGetLastError());
  return GM_OK;
}

// gm_g2_lincomb_many: host records and canonical scalars staged in C->lincomb, three launches, one wait
int g2_lincomb_many_host(Context* C, const void* points, size_t stride, const uint64_t* scalars_canonical, const size_t* offsets, size_t S, uint64_t* out_jac) {
  using G = GrpG2;
  if (S == 0) return GM_OK;
  GM_CHECK(stride >= G::AFF_BYTES && (stride % 8) == 0, GM_EINVAL, "g2_lincomb_many: stride %zu must be >= %zu and a multiple of 8", stride, G::AFF_BYTES);
  GM_CHECK(offsets[0] == 0, GM_EINVAL, "g2_lincomb_many: offsets[0] = %zu, the first segment starts at 0", offsets[0]);
  for (size_t s = 0; s < S; s++)
    GM_CHECK(offsets[s] <= offsets[s + 1], GM_EINVAL, "g2_lincomb_many: offsets[%zu] = %zu is above offsets[%zu] = %zu", s, offsets[s], s + 1, offsets[s + 1]);
  const size_t T = offsets[S];
  GM_CHECK(T <= ((size_t)1 << 28) && S <= ((size_t)1 << 28), GM_EINVAL, "g2_lincomb_many: %zu terms in %zu segments (at most 2^28 of either)", T, S);
  static_assert(sizeof(size_t) == sizeof(unsigned long long), "the offsets are copied as they are");
  auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t o_raw = 0, o_pts = o_raw + up(T * stride), o_sc = o_pts + up(T * G::AFF_BYTES), o_off = o_sc + up(T * 32), o_terms = o_off + up((S + 1) * 8),
               o_sums = o_terms + T * G::XYZZ_BYTES, o_aff = o_sums + S * G::XYZZ_BYTES, total = o_aff + S * G::AFF_BYTES;
  GM_MSM_LOCK(C);
  int rc = C->lincomb.ensure(total);
  if (rc) return rc;
  uint8_t* w = C->lincomb.as<uint8_t>();
  hipStream_t st = C->stream;
  std::vector<uint64_t> aff(24 * S);
  auto enqueue = [&]() -> int {
    GM_HIP(hipMemcpyAsync(w + o_off, offsets, (S + 1) * 8, hipMemcpyHostToDevice, st));
    if (T) {
      GM_HIP(hipMemcpyAsync(w + o_raw, points, T * stride, hipMemcpyHostToDevice, st));
      GM_HIP(hipMemcpyAsync(w + o_sc, scalars_canonical, T * 32, hipMemcpyHostToDevice, st));
      int r = pack_launch<G>(st, w + o_raw, stride, T, w + o_pts);
      if (!r) r = term_mul_launch<G>(st, w + o_pts, nullptr, w + o_sc, nullptr, 0, T, w + o_terms);
      if (r) return r;
    }
    int r = seg_sum_launch<G>(st, w + o_terms, reinterpret_cast<const unsigned long long*>(w + o_off), S, w + o_sums);
    if (!r) r = normalise_launch<G>(st, w + o_sums, nullptr, S, w + o_aff);  // o_aff lies behind o_sums: apart, as the kernel needs
    if (r) return r;
    GM_HIP(hipMemcpyAsync(aff.data(), w + o_aff, S * G::AFF_BYTES, hipMemcpyDeviceToHost, st));
    return GM_OK;
  };
  rc = enqueue();
  const hipError_t e = hipStreamSynchronize(st);  // the host arrays are read by their copies until here
  if (rc) return rc;
  GM_HIP(e);
  for (size_t s = 0; s < S; s++) gmh::g2_affine_to_jac_dev(aff.data() + 24 * s).to_limbs(out_jac + 36 * s);
  return GM_OK;
}

template <class G>
int bases_from_host(Context* C, const void* bases, size_t stride, size_t n, std::unique_ptr<typename G::Held>& out) {
  GM_CHECK(stride >= G::AFF_BYTES && (stride % 8) == 0, GM_EINVAL, "%sbases: stride %zu must be >= %zu and a multiple of 8", G::WHO, stride, G::AFF_BYTES);
  auto b = std::make_unique<typename G::Held>();
  b->n = n;
  if (n) {
    DevTmp key, stage;
    GM_HIP(dev_malloc(&key.p, n * G::AFF_BYTES));
    GM_HIP(dev_malloc(&stage.p, n * stride));
    GM_HIP(hipMemcpyAsync(stage.p, bases, n * stride, hipMemcpyHostToDevice, C->stream));
    const int rc = pack_launch<G>(C->stream, stage.u8(), stride, n, key.u8());
    if (rc) return rc;
    GM_HIP(hipStreamSynchronize(C->stream));
    b->d = key.u8();
    key.p = nullptr;
  }
  out = std::move(b);
  return GM_OK;
}

template <class G>
int bases_export(Context* C, const typename G::Held* b, size_t offset, size_t n, void* out) {
  if (n == 0) return GM_OK;
  DevTmp tmp;
  GM_HIP(dev_malloc(&tmp.p, n * G::AFF_BYTES));
  hipLaunchKernelGGL(k_export_bases<G>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, C->stream, b->d + offset * G::AFF_BYTES, n, tmp.u8());
  GM_HIP(hipGetLastError());
  GM_HIP(hipMemcpyAsync(out, tmp.p, n * G::AFF_BYTES, hipMemcpyDeviceToHost, C->stream));
  GM_HIP(hipStreamSynchronize(C->stream));
  return GM_OK;
}

// out[i] = scalars[i] * base, i < n: the affine table (32 x 256 records), then slabs of at most 2^22 points -- a multiply launch into
// an XYZZ slab and its normalisation into the key.  d_scalars: n x 32 bytes on the device, ordered on C->stream.
template <class G>
int fixed_base_generate(Context* C, const uint64_t* base_affine, const void* d_scalars, int mont, size_t n, std::unique_ptr<typename G::Held>& out) {
  GM_CHECK(n <= SIZE_MAX / G::XYZZ_BYTES, GM_EINVAL, "%s fixed base: %zu points do not fit a size_t", G::NAME, n);
  auto b = std::make_unique<typename G::Held>();
  b->n = n;
  if (n) {
    GM_MSM_LOCK(C);
    DevTmp base, stage, t_xyzz, table, xy, key;
    const size_t T = (size_t)32 * 256;
    GM_HIP(dev_malloc(&base.p, G::AFF_BYTES));
    GM_HIP(dev_malloc(&stage.p, G::AFF_BYTES));
    GM_HIP(dev_malloc(&t_xyzz.p, T * G::XYZZ_BYTES));
    GM_HIP(dev_malloc(&table.p, T * G::AFF_BYTES));
    GM_HIP(hipMemcpyAsync(stage.p, base_affine, G::AFF_BYTES, hipMemcpyHostToDevice, C->stream));
    hipLaunchKernelGGL(k_pack_bases<G>, dim3(1), dim3(64), 0, C->stream, stage.u8(), (size_t)G::AFF_BYTES, (size_t)1, base.u8());
    hipLaunchKernelGGL(k_fixed_base_table<G>, dim3((unsigned)(T / G::KEY_BLOCK)), dim3(G::KEY_BLOCK), 0, C->stream, base.u8(), t_xyzz.u8());
    int rc = normalise_launch<G>(C->stream, t_xyzz.u8(), nullptr, T, table.u8(), G::TABLE_NORM_K);
    if (rc) return rc;
    const size_t slab = std::min<size_t>(n, (size_t)1 << 22);
    GM_HIP(dev_malloc(&key.p, n * G::AFF_BYTES));
    GM_HIP(dev_malloc(&xy.p, slab * G::XYZZ_BYTES));
    for (size_t off = 0; off < n; off += slab) {
      const size_t m = std::min(slab, n - off);
      hipLaunchKernelGGL(k_fixed_base_mul<G>, dim3((unsigned)((m + G::KEY_BLOCK - 1) / G::KEY_BLOCK)), dim3(G::KEY_BLOCK), 0, C->stream,
                         reinterpret_cast<const uint32_t*>(d_scalars) + 8 * off, mont, m, table.u8(), xy.u8());
      if ((rc = normalise_launch<G>(C->stream, xy.u8(), nullptr, m, key.u8() + off * G::AFF_BYTES))) return rc;
    }
    GM_HIP(hipGetLastError());
    GM_HIP(hipStreamSynchronize(C->stream));
    b->d = key.u8();
    key.p = nullptr;
  }
  out = std::move(b);
  return GM_OK;
}

// ---- the instances ---------------------------------------------------------------------------------------------------------------
template int bases_from_host<GrpG1>(Context*, const void*, size_t, size_t, std::unique_ptr<Bases>&);
template int bases_from_host<GrpG2>(Context*, const void*, size_t, size_t, std::unique_ptr<G2Bases>&);
template int bases_export<GrpG1>(Context*, const Bases*, size_t, size_t, void*);
template int bases_export<GrpG2>(Context*, const G2Bases*, size_t, size_t, void*);
template int fixed_base_generate<GrpG1>(Context*, const uint64_t*, const void*, int, size_t, std::unique_ptr<Bases>&);
template int fixed_base_generate<GrpG2>(Context*, const uint64_t*, const void*, int, size_t, std::unique_ptr<G2Bases>&);
template int normalise_launch<GrpG1>(hipStream_t, const uint8_t*, const uint32_t*, size_t, uint8_t*, int);
template int normalise_launch<GrpG2>(hipStream_t, const uint8_t*, const uint32_t*, size_t, uint8_t*, int);

// under the names of ctx.hpp
int bases_from_host(Context* C, const void* bases, size_t stride, size_t n, std::unique_ptr<Bases>& out) { return bases_from_host<GrpG1>(C, bases, stride, n, out); }
int g2_bases_from_host(Context* C, const void* bases, size_t stride, size_t n, std::unique_ptr<G2Bases>& out) { return bases_from_host<GrpG2>(C, bases, stride, n, out); }
int g1_pack_launch(hipStream_t st, const uint8_t* src, size_t stride, size_t n, uint8_t* dst) { return pack_launch<GrpG1>(st, src, stride, n, dst); }
int g1_normalise_launch(hipStream_t st, const uint8_t* in, size_t n, uint8_t* out) { return normalise_launch<GrpG1>(st, in, nullptr, n, out); }
int g1_split_fold_launch(Context* C, const uint8_t* in, size_t n, const uint32_t* d_s8, uint8_t* out) { return split_fold_launch<GrpG1>(C->stream, in, n, d_s8, out); }
int g2_split_fold_launch(Context* C, const uint8_t* in, size_t n, const uint32_t* d_s8, uint8_t* out) { return split_fold_launch<GrpG2>(C->stream, in, n, d_s8, out); }
int g1_split_fold_rev_launch(Context* C, const uint8_t* in, size_t n, const uint32_t* d_s8, uint8_t* out) { return split_fold_rev_launch<GrpG1>(C->stream, in, n, d_s8, out); }
int g2_split_fold_rev_launch(Context* C, const uint8_t* in, size_t n, const uint32_t* d_s8, uint8_t* out) { return split_fold_rev_launch<GrpG2>(C->stream, in, n, d_s8, out); }
int records_reverse_launch(Context* C, const uint8_t* in, size_t n, size_t rec_bytes, uint8_t* out) {
  const size_t lanes = n * (rec_bytes / 16);
  if (lanes == 0) return GM_OK;
  hipLaunchKernelGGL(k_records_reverse, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, C->stream, reinterpret_cast<const uint4*>(in), n,
                     (uint32_t)(rec_bytes / 16), reinterpret_cast<uint4*>(out));
  GM_HIP(hipGetLastError());
  return GM_OK;
}
int g1_split_fold_seg_launch(Context* C, const FoldSpan* d_spans, size_t nspans, size_t n, const uint32_t* d_s8) { return split_fold_seg_launch<GrpG1>(C->stream, d_spans, nspans, n, d_s8); }
int g2_split_fold_seg_launch(Context* C, const FoldSpan* d_spans, size_t nspans, size_t n, const uint32_t* d_s8) { return split_fold_seg_launch<GrpG2>(C->stream, d_spans, nspans, n, d_s8); }
int g1_term_mul_launch(Context* C, const uint8_t* d_points, const uint32_t* d_pidx, const uint8_t* d_scalars, const uint32_t* d_sidx, int mont, size_t T, uint8_t* d_out_xyzz) {
  return term_mul_launch<GrpG1>(C->stream, d_points, d_pidx, d_scalars, d_sidx, mont, T, d_out_xyzz);
}
int g2_term_mul_launch(Context* C, const uint8_t* d_points, const uint32_t* d_pidx, const uint8_t* d_scalars, const uint32_t* d_sidx, int mont, size_t T, uint8_t* d_out_xyzz) {
  return term_mul_launch<GrpG2>(C->stream, d_points, d_pidx, d_scalars, d_sidx, mont, T, d_out_xyzz);
}
int g1_seg_sum_launch(Context* C, const uint8_t* d_in_xyzz, const unsigned long long* d_off, size_t S, uint8_t* d_out_xyzz) { return seg_sum_launch<GrpG1>(C->stream, d_in_xyzz, d_off, S, d_out_xyzz); }
int g2_seg_sum_launch(Context* C, const uint8_t* d_in_xyzz, const unsigned long long* d_off, size_t S, uint8_t* d_out_xyzz) { return seg_sum_launch<GrpG2>(C->stream, d_in_xyzz, d_off, S, d_out_xyzz); }
int g2_normalise_launch(hipStream_t st, const uint8_t* in, size_t n, uint8_t* out) { return normalise_launch<GrpG2>(st, in, nullptr, n, out); }

}  // namespace gm
