// herring's TimeProver over a bilinear module (src/herring/time_prover.rs:42-137), stated once for G1Module, G2Module, PModule and
// GtModule (src/herring/module.rs:49-125).  FModule rides the field sumcheck kernel (fr.hip: sc_set_herring).
//
// The prover keeps the Lhs vector f and the Rhs vector g on the device, each in two ping-pong buffers:
//   fold(r)          f'[i] = f[2i] + (r twist) f[2i+1], g'[i] = g[2i] + r g[2i+1] (an odd tail folds against zero), twist <- twist^2
//   next_message(c)  an optional fold, then a = ip(f_even, g_even), b = ip(f_even, g_odd) + ip(f_odd, g_even); ip zips, so the
//                    shorter side ends a product.  After log2(min(len)) messages the answer is "no message"
//   final_foldings   (f[0], g[0]) once the last round is behind
// A SIDE says how a vector of its element type is held, folded and read out -- Fr, affine G1, affine G2, GT -- and a MODULE is two
// sides and its inner product `ip`: the only per-module code.  The engines (msm.hip, g2msm.hip, pairing.hip) and the fold kernels
// stay where they are.
//
// Locks: the prover's own mutex outermost; the MSM lock in fold (the canonical scalars of the point folds are staged in
// C->msm.misc) and wherever the engines take it.
#include <algorithm>
#include <cstring>

#include "ctx.hpp"
#include "herring_space_plan.hpp"
#include "host_field.hpp"

namespace gm {

// ---- sides --------------------------------------------------------------------------------------------------------------
struct HerringSide {
  size_t elem;  // bytes per element
  // the host vector on the device (point records are packed from `stride` bytes); *cap != 0: a block of the vector pool
  int (*upload)(Context* C, const void* host, size_t stride, size_t n, uint8_t** d, size_t* cap);
  int (*alloc)(Context* C, size_t n, uint8_t** d, size_t* cap);
  void (*release)(Context* C, uint8_t* d, size_t cap);
  // out[i] = in[2i] + s in[2i+1] on C->stream, no wait: Fr takes s in Montgomery form, the points the canonical copy on the device
  int (*split_fold)(Context* C, const uint8_t* in, size_t n, const uint64_t s_mont[4], const uint32_t* d_s_canon, uint8_t* out);
  void (*read0)(const uint64_t* elem, uint64_t* out);  // element 0 as final_foldings returns it: Fr as it is, points as Jacobian
};

static int fr_alloc(Context* C, size_t n, uint8_t** d, size_t* cap) { return C->pool.alloc(n * 32, (void**)d, cap); }
static int fr_upload(Context* C, const void* host, size_t, size_t n, uint8_t** d, size_t* cap) {
  int rc = fr_alloc(C, n, d, cap);
  if (rc) return rc;
  GM_HIP(hipMemcpyAsync(*d, host, n * 32, hipMemcpyHostToDevice, C->stream));
  GM_HIP(hipStreamSynchronize(C->stream));
  return GM_OK;
}
static void fr_release(Context* C, uint8_t* d, size_t cap) { C->pool.free(d, cap); }
static int fr_split_fold(Context* C, const uint8_t* in, size_t n, const uint64_t s_mont[4], const uint32_t*, uint8_t* out) {
  return fr_fold_raw(C, in, n, s_mont, out);
}
static void fr_read0(const uint64_t* elem, uint64_t* out) { memcpy(out, elem, 32); }

template <size_t ELEM>
static int point_alloc(Context*, size_t n, uint8_t** d, size_t* cap) {
  *cap = 0;
  GM_HIP(dev_malloc((void**)d, n * ELEM));
  return GM_OK;
}
static void point_release(Context*, uint8_t* d, size_t) {
  if (d) (void)gm::raw_free(d);
}
static int g1_upload(Context* C, const void* host, size_t stride, size_t n, uint8_t** d, size_t* cap) {
  std::unique_ptr<Bases> b;
  int rc = bases_from_host(C, host, stride, n, b);
  if (rc) return rc;
  *d = b->d;  // take ownership of the packed copy
  *cap = 0;
  return GM_OK;
}
static int g2_upload(Context* C, const void* host, size_t stride, size_t n, uint8_t** d, size_t* cap) {
  std::unique_ptr<G2Bases> b;
  int rc = g2_bases_from_host(C, host, stride, n, b);
  if (rc) return rc;
  *d = b->d;
  *cap = 0;
  return GM_OK;
}
static int g1_split_fold(Context* C, const uint8_t* in, size_t n, const uint64_t*, const uint32_t* d_s_canon, uint8_t* out) {
  return g1_split_fold_launch(C, in, n, d_s_canon, out);
}
static int g2_split_fold(Context* C, const uint8_t* in, size_t n, const uint64_t*, const uint32_t* d_s_canon, uint8_t* out) {
  return g2_split_fold_launch(C, in, n, d_s_canon, out);
}
static void g1_read0(const uint64_t* elem, uint64_t* out) { gmh::g1_affine_to_jac_dev(elem).to_limbs(out); }
static void g2_read0(const uint64_t* elem, uint64_t* out) { gmh::g2_affine_to_jac_dev(elem).to_limbs(out); }

// GT elements: host records of 72 x u64, 576-byte device records (gt.cuh); "+" is the product, the fold out[i] = f[2i] f[2i+1]^s
static int gt_upload(Context* C, const void* host, size_t, size_t n, uint8_t** d, size_t* cap) {
  *cap = 0;
  return gt_from_host(C, static_cast<const uint64_t*>(host), n, d);
}
static int gt_split_fold(Context* C, const uint8_t* in, size_t n, const uint64_t*, const uint32_t* d_s_canon, uint8_t* out) {
  return gt_split_fold_launch(C, in, n, d_s_canon, out);
}
static void gt_read0(const uint64_t* elem, uint64_t* out) { gmh::Fq12::from_device(elem).to_limbs(out); }

static const HerringSide FR_SIDE = {32, fr_upload, fr_alloc, fr_release, fr_split_fold, fr_read0};
static const HerringSide G1_SIDE = {96, g1_upload, point_alloc<96>, point_release, g1_split_fold, g1_read0};
static const HerringSide G2_SIDE = {192, g2_upload, point_alloc<192>, point_release, g2_split_fold, g2_read0};
static const HerringSide GT_SIDE = {576, gt_upload, point_alloc<576>, point_release, gt_split_fold, gt_read0};

// a vector where the prover keeps it: a host vector goes through the side's upload, a packed device vector (the CRS of ipa.hip) is copied
static int side_put(Context* C, const HerringSide* S, const void* src, size_t stride, size_t n, bool on_device, uint8_t** d, size_t* cap) {
  if (!on_device) return S->upload(C, src, stride, n, d, cap);
  int rc = S->alloc(C, n, d, cap);
  if (rc) return rc;
  GM_HIP(hipMemcpyAsync(*d, src, n * S->elem, hipMemcpyDeviceToDevice, C->stream));
  GM_HIP(hipStreamSynchronize(C->stream));
  return GM_OK;
}

// ---- modules ------------------------------------------------------------------------------------------------------------
struct HerringZip {  // lengths of the even / odd halves, and of the three products a message is made of
  size_t fe, fo, ge, go;
  size_t ee, eo, oe;
};

// G1Module::ip is an MSM (module.rs:91-101): three strided MSMs over the same point array, issued as ONE batch (these are small
// calls -- 2^10 points in the reference's tests -- and run side by side on the small lanes)
static int g1_message(Context* C, HerringProver* H, const HerringZip& z, uint64_t* a_jac, uint64_t* b_jac) {
  Bases fb;
  fb.d = H->f[H->cur];
  fb.n = H->nf;
  const uint8_t* g = H->g[H->cur];
  const size_t slot = (z.ge + 1) * 32;  // bytes per compacted scalar vector inside H->tmp
  const int64_t firsts[3] = {0, 0, 1};
  const size_t g_first[3] = {0, 1, 0};
  const size_t cnts[3] = {z.ee, z.eo, z.oe};
  const void* sc[3];
  int rc;
  for (int j = 0; j < 3; j++) {
    uint8_t* dst = H->tmp + (size_t)j * slot;
    if ((rc = fr_stride_raw(C, g, g_first[j], 2, cnts[j], dst))) return rc;
    sc[j] = dst;
  }
  uint64_t res[3 * 18];
  if ((rc = msm_run_batch_at(C, &fb, 0, 2, nullptr, sc, 1, cnts, 3, true, res, firsts))) return rc;
  memcpy(a_jac, res, 18 * sizeof(uint64_t));
  gmh::G1::from_limbs(res + 18).add(gmh::G1::from_limbs(res + 36)).normalized().to_limbs(b_jac);
  return GM_OK;
}

// G2Module::ip(f, g) = msm(g, f) (module.rs:114-124)
static int g2_message(Context* C, HerringProver* H, const HerringZip& z, uint64_t* a_jac, uint64_t* b_jac) {
  G2Bases gb;
  gb.d = H->g[H->cur];
  gb.n = H->ng;
  uint8_t* f_even = H->tmp;
  uint8_t* f_odd = H->tmp + (z.fe + 1) * 32;
  int rc;
  if ((rc = fr_stride_raw(C, H->f[H->cur], 0, 2, z.fe, f_even))) return rc;
  if (z.fo && (rc = fr_stride_raw(C, H->f[H->cur], 1, 2, z.fo, f_odd))) return rc;
  uint64_t b1[36], b2[36];
  if ((rc = g2_msm_run(C, &gb, 0, 2, f_even, 1, z.ee, a_jac))) return rc;
  if ((rc = g2_msm_run(C, &gb, 1, 2, f_even, 1, z.eo, b1))) return rc;
  if ((rc = g2_msm_run(C, &gb, 0, 2, f_odd, 1, z.oe, b2))) return rc;
  gmh::G2::from_limbs(b1).add(gmh::G2::from_limbs(b2)).normalized().to_limbs(b_jac);
  return GM_OK;
}

// PModule::ip is a multi-pairing (module.rs:70-78) and GT is written multiplicatively: b is ONE Miller product over both halves
// and ONE final exponentiation
static int p_message(Context* C, HerringProver* H, const HerringZip& z, uint64_t* a_gt, uint64_t* b_gt) {
  GM_MSM_LOCK(C);
  PairSpan ee, eo, oe;
  ee.g1 = eo.g1 = oe.g1 = H->f[H->cur];
  ee.g2 = eo.g2 = oe.g2 = H->g[H->cur];
  ee.step1 = ee.step2 = eo.step1 = eo.step2 = oe.step1 = oe.step2 = 2;
  ee.n = z.ee;
  eo.first2 = 1;
  eo.n = z.eo;
  oe.first1 = 1;
  oe.n = z.oe;
  gmh::Fq12 fa, fb;
  int rc;
  if ((rc = miller_product(C, ee, PairSpan(), &fa))) return rc;
  if ((rc = miller_product(C, eo, oe, &fb))) return rc;
  pairing_finish(fa, a_gt);
  pairing_finish(fb, b_gt);
  return GM_OK;
}

// GtModule::ip is a multi-exponentiation (module.rs:49-58, the default ip; GT is written multiplicatively): the exponents are the
// canonical integers of the Fr side, read strided and taken out of Montgomery form by the kernel itself -- no compacted copy --
// and b is ONE launch over both halves
static int gt_message(Context* C, HerringProver* H, const HerringZip& z, uint64_t* a_gt, uint64_t* b_gt) {
  GM_MSM_LOCK(C);
  GtSpan ee, eo, oe;
  ee.x = eo.x = oe.x = H->f[H->cur];
  ee.e = eo.e = oe.e = H->g[H->cur];
  ee.step_x = ee.step_e = eo.step_x = eo.step_e = oe.step_x = oe.step_e = 2;
  ee.n = z.ee;
  eo.first_e = 1;
  eo.n = z.eo;
  oe.first_x = 1;
  oe.n = z.oe;
  const GtSpan sa[3] = {ee, GtSpan(), GtSpan()}, sb[3] = {eo, oe, GtSpan()};
  gmh::Fq12 fa, fb;
  int rc;
  if ((rc = gt_multi_pow(C, sa, 1, &fa))) return rc;
  if ((rc = gt_multi_pow(C, sb, 1, &fb))) return rc;
  fa.to_limbs(a_gt);
  fb.to_limbs(b_gt);
  return GM_OK;
}

struct HerringModuleDesc {
  const char* name;
  const HerringSide *lhs, *rhs;
  int (*message)(Context* C, HerringProver* H, const HerringZip& z, uint64_t* a, uint64_t* b);
  // Two differences between the modules are kept as they were found; making them uniform would change behaviour.
  size_t tmp_slots;   // compacted copies of halves of the Fr side that `message` builds in H->tmp: three for G1, two for G2, none for P and Gt
  bool ends_for_good;  // P only: after the call that answered "no message", round and fold are sequence errors (GM_ESTATE)
};
static const HerringModuleDesc MODULES[] = {  // indexed by HerringModule
    {"G1", &G1_SIDE, &FR_SIDE, g1_message, 3, false},
    {"G2", &FR_SIDE, &G2_SIDE, g2_message, 2, false},
    {"P", &G1_SIDE, &G2_SIDE, p_message, 0, true},
    {"Gt", &GT_SIDE, &FR_SIDE, gt_message, 0, false},
};

// ---- the prover ---------------------------------------------------------------------------------------------------------
void herring_destroy(Context* C, HerringProver* H) {
  const HerringModuleDesc& M = MODULES[H->module];
  for (int i = 0; i < 2; i++) {
    M.lhs->release(C, H->f[i], H->fcap[i]);
    M.rhs->release(C, H->g[i], H->gcap[i]);
    H->f[i] = H->g[i] = nullptr;
  }
  C->pool.free(H->tmp, H->tmpcap);
  H->tmp = nullptr;
}

int herring_create(Context* C, HerringModule module, const void* f, size_t f_stride, size_t nf, const void* g, size_t g_stride, size_t ng,
                   const uint64_t twist[4], uint64_t* handle, int on_device) {
  const HerringModuleDesc& M = MODULES[module];
  GM_CHECK(nf >= 1 && ng >= 1, GM_EINVAL, "herring %s prover: empty vectors", M.name);
  auto H = std::make_unique<HerringProver>();
  H->module = module;
  H->nf = nf;
  H->ng = ng;
  const size_t fr_len = M.lhs == &FR_SIDE ? nf : ng;  // of the side `message` compacts (no slot: no side)
  int rc;
  if ((rc = side_put(C, M.lhs, f, f_stride, nf, on_device & 1, &H->f[0], &H->fcap[0])) || (rc = side_put(C, M.rhs, g, g_stride, ng, on_device & 2, &H->g[0], &H->gcap[0])) ||
      (rc = M.lhs->alloc(C, (nf + 1) / 2, &H->f[1], &H->fcap[1])) || (rc = M.rhs->alloc(C, (ng + 1) / 2, &H->g[1], &H->gcap[1])) ||
      (rc = C->pool.alloc(M.tmp_slots * (((fr_len + 1) / 2 + 1) * 32), (void**)&H->tmp, &H->tmpcap))) {
    herring_destroy(C, H.get());  // what has been allocated so far goes back
    return rc;
  }
  memcpy(H->twist, twist, 32);
  H->tot_rounds = (size_t)msm_ceil_log2(std::min(nf, ng));  // Witness::required_rounds: log2(min(len)) (time_prover.rs:36-39)
  std::lock_guard<std::mutex> lk(C->mu);
  *handle = C->next_handle++;
  C->herring[*handle] = std::move(H);
  return GM_OK;
}

// time_prover.rs:82-88: the Lhs folds by r twist, the Rhs by r
static int fold_locked(Context* C, HerringProver* H, const uint64_t r[4]) {
  const HerringModuleDesc& M = MODULES[H->module];
  GM_MSM_LOCK(C);  // the canonical scalars are staged in the MSM workspace (C->msm.misc)
  const gmh::Fr rr = gmh::Fr::from_limbs(r), tw = gmh::Fr::from_limbs(H->twist), rt = rr * tw;
  uint64_t mont[2][4], canon[2][4];  // {Lhs, Rhs}; scalar multiplication wants the integers
  rt.to_limbs(mont[0]);
  rr.to_limbs(mont[1]);
  rt.to_canonical(canon[0]);
  rr.to_canonical(canon[1]);
  int rc = C->msm.misc.ensure(64);
  if (rc) return rc;
  GM_HIP(hipMemcpyAsync(C->msm.misc.p, canon, 64, hipMemcpyHostToDevice, C->stream));
  if ((rc = M.lhs->split_fold(C, H->f[H->cur], H->nf, mont[0], C->msm.misc.as<uint32_t>(), H->f[H->cur ^ 1]))) return rc;
  if ((rc = M.rhs->split_fold(C, H->g[H->cur], H->ng, mont[1], C->msm.misc.as<uint32_t>() + 8, H->g[H->cur ^ 1]))) return rc;
  GM_HIP(hipStreamSynchronize(C->stream));  // `mont` and `canon` are read by the copies until here
  C->prof.collect();                        // the GT fold books its launch (gt_split_fold_launch)
  H->cur ^= 1;
  H->nf = (H->nf + 1) / 2;
  H->ng = (H->ng + 1) / 2;
  tw.sqr().to_limbs(H->twist);
  return GM_OK;
}

int herring_fold(Context* C, HerringProver* H, const uint64_t r[4]) {
  std::lock_guard<std::mutex> lk(H->mu);
  GM_CHECK(!H->finished, GM_ESTATE, "herring %s prover: fold after the last round", MODULES[H->module].name);
  return fold_locked(C, H, r);
}

// time_prover.rs:91-123
int herring_round(Context* C, HerringProver* H, const uint64_t* challenge, uint64_t* a, uint64_t* b, int* has_msg) {
  const HerringModuleDesc& M = MODULES[H->module];
  std::lock_guard<std::mutex> lk(H->mu);
  GM_CHECK(!H->finished && H->round <= H->tot_rounds, GM_ESTATE, "More rounds than needed.");
  int rc;
  if (challenge && (rc = fold_locked(C, H, challenge))) return rc;
  if (H->round == H->tot_rounds) {
    H->finished = M.ends_for_good;
    *has_msg = 0;
    return GM_OK;
  }
  const size_t fe = (H->nf + 1) / 2, fo = H->nf / 2, ge = (H->ng + 1) / 2, go = H->ng / 2;
  const HerringZip z = {fe, fo, ge, go, std::min(fe, ge), std::min(fe, go), std::min(fo, ge)};  // zip: the shorter side ends the product
  if ((rc = M.message(C, H, z, a, b))) return rc;
  H->round += 1;
  *has_msg = 1;
  return GM_OK;
}

// gm_hgt_check: the membership test over the current f vector of a GtModule prover, where it lies (*ok was cleared by the entry)
int herring_gt_check(Context* C, HerringProver* H, size_t* first_bad, int* ok) {
  std::lock_guard<std::mutex> lk(H->mu);
  GM_MSM_LOCK(C);
  return gt_check_run(C, H->f[H->cur], 0, H->nf, nullptr, first_bad, ok);
}

// time_prover.rs:135-137
int herring_final(Context* C, HerringProver* H, uint64_t* f0, uint64_t* g0, int* has) {
  const HerringModuleDesc& M = MODULES[H->module];
  std::lock_guard<std::mutex> lk(H->mu);
  if (H->round != H->tot_rounds) {
    *has = 0;
    return GM_OK;
  }
  uint64_t ef[72], eg[72];  // the largest element: GT, 576 bytes
  GM_HIP(hipMemcpyAsync(ef, H->f[H->cur], M.lhs->elem, hipMemcpyDeviceToHost, C->stream));
  GM_HIP(hipMemcpyAsync(eg, H->g[H->cur], M.rhs->elem, hipMemcpyDeviceToHost, C->stream));
  GM_HIP(hipStreamSynchronize(C->stream));
  M.lhs->read0(ef, f0);
  M.rhs->read0(eg, g0);
  *has = 1;
  return GM_OK;
}

// ---- the space prover of G1Module and G2Module ---------------------------------------------------------------------------
// src/herring/space_prover.rs:39-316 for the two modules whose p(point, scalar) = scalar * point is linear in the point.  The
// prover owns no point: the key is read where it lies as the big-endian stream key[offset + i].  After k folds the folded vectors
// are F[m] = sum_u w_u x_le[m 2^k + u] (streams.rs:209-249; x_le[i] = stream[n - 1 - i], zero past the end as init_stack pads), so
// every sum of a message is an MSM over the original points whose scalars one launch of k_hsp_scalars (fr.hip) expands.
//   fold(r)          the challenge is stored, r twist on the Lhs and r on the Rhs, the twist is squared (:255-259); the scalar side,
//                    32 bytes an element, is kept folded: S <- fold(S, its challenge)
//   next_message(c)  an optional fold; pair j is (block 2j, block 2j + 1) of both sides, as many pairs as the shorter side has, and
//                    a = sum_j twist^(2j) p(F[2j], G[2j]), b = sum_j twist^(2j) (p(F[2j], G[2j+1]) + twist p(F[2j+1], G[2j])):
//                    what :150-207 computes with twist_runner = twist^(2 pairs) stepping down by twist^-2 -- on the first pair it
//                    multiplies p, in the loop the Rhs, which is the same value
//   final_foldings   the FIRST item of each folded stream (:270-276): the block of the highest index, not element 0.  The two are
//                    one when the streams have equal lengths
//   to_time          TimeProver::from(&SpaceProver) (:279-316): the point side folded k times out of place by split_fold
// The reference's alignment (:152-164) adds the parity of the shorter length to the skip where it has to be subtracted: when the
// folded lengths differ and the shorter one is odd its assertion f_pairs == g_pairs fails.  Everywhere else its pairs are the
// ones above, which are also the TimeProver's (the zip of the even and odd halves).
struct HspModuleDesc {
  const char* name;
  HerringModule module;
  const HerringSide* point;  // G1_SIDE / G2_SIDE
  bool rhs_points;           // G2Module: the points are the Rhs (folded by r, and the twist factor of b sits on the even block)
  int (*split_fold_rev)(Context* C, const uint8_t* in, size_t n, const uint32_t* d_s8, uint8_t* out);
};
static const HspModuleDesc HSP_G1 = {"G1", HERRING_G1, &G1_SIDE, false, g1_split_fold_rev_launch};
static const HspModuleDesc HSP_G2 = {"G2", HERRING_G2, &G2_SIDE, true, g2_split_fold_rev_launch};
static const HspModuleDesc& hsp_desc(const HerringSpace* H) { return H->module == HERRING_G1 ? HSP_G1 : HSP_G2; }
static const uint8_t* hsp_key(const HerringSpace* H) {  // the first point of the stream
  return H->module == HERRING_G1 ? H->g1->d + H->offset * 96 : H->g2->d + H->offset * 192;
}

void hsp_destroy(Context* C, HerringSpace* H) {
  for (int i = 0; i < 2; i++) {
    C->pool.free(H->s[i], H->scap[i]);
    H->s[i] = nullptr;
  }
  C->pool.free(H->work, H->work_cap);
  H->work = nullptr;
  if (H->own_g1 && H->own_g1->d) (void)gm::raw_free(H->own_g1->d);
  if (H->own_g2 && H->own_g2->d) (void)gm::raw_free(H->own_g2->d);
  H->own_g1.reset();
  H->own_g2.reset();
}

// the work block holds the tables of `k` challenges (it is made for tot_rounds; folds past the last round make it grow)
static int hsp_ensure_work(Context* C, HerringSpace* H, uint32_t k) {
  const size_t need = hsp_work_bytes(H->np, k);
  if (H->work_cap >= need) return GM_OK;
  C->pool.free(H->work, H->work_cap);
  H->work = nullptr;
  H->work_cap = 0;
  int rc = C->pool.alloc(need, (void**)&H->work, &H->work_cap);
  if (!rc) H->path[3] += need;
  return rc;
}

int hsp_create(Context* C, HerringModule module, const void* key, size_t offset, const void* host_points, size_t stride, size_t np,
               const void* scalars, size_t ns, bool on_device, const uint64_t twist[4], uint64_t* handle) {
  const HspModuleDesc& M = module == HERRING_G1 ? HSP_G1 : HSP_G2;
  GM_CHECK(np >= 1 && ns >= 1, GM_EINVAL, "herring %s space prover: empty streams", M.name);
  auto H = std::make_unique<HerringSpace>();
  H->module = module;
  H->np = np;
  H->ns = H->ls = ns;
  H->offset = offset;
  int rc;
  if (key) {
    const size_t have = module == HERRING_G1 ? static_cast<const Bases*>(key)->n : static_cast<const G2Bases*>(key)->n;
    GM_CHECK(offset <= have && np <= have - offset, GM_EINVAL, "herring %s space prover: points [%zu, %zu) outside a key of %zu", M.name, offset,
             offset + np, have);
    if (module == HERRING_G1) H->g1 = static_cast<const Bases*>(key);
    else H->g2 = static_cast<const G2Bases*>(key);
  } else {  // host records: a key of the prover's own
    H->offset = 0;
    if (module == HERRING_G1) {
      if ((rc = bases_from_host(C, host_points, stride, np, H->own_g1))) return rc;
      H->g1 = H->own_g1.get();
    } else {
      if ((rc = g2_bases_from_host(C, host_points, stride, np, H->own_g2))) return rc;
      H->g2 = H->own_g2.get();
    }
    H->path[2] += np * M.point->elem;
  }
  memcpy(H->twist, twist, 32);
  H->tot_rounds = hsp_ceil_log2(std::min(np, ns));  // WitnessStream::required_rounds (:77-80)
  std::vector<uint64_t> rev;
  if ((rc = C->pool.alloc(ns * 32, (void**)&H->s[0], &H->scap[0])) || (rc = C->pool.alloc(((ns + 1) / 2) * 32, (void**)&H->s[1], &H->scap[1])) ||
      (rc = hsp_ensure_work(C, H.get(), (uint32_t)H->tot_rounds))) {
    hsp_destroy(C, H.get());
    return rc;
  }
  H->path[3] += ns * 32 + ((ns + 1) / 2) * 32;
  // S = the scalar stream as the little-endian vector it stands for
  if (on_device) {
    rc = fr_reverse_raw(C, static_cast<const uint8_t*>(scalars), ns, H->s[0]);
  } else {
    rev.resize(ns * 4);
    for (size_t i = 0; i < ns; i++) memcpy(&rev[4 * i], static_cast<const uint64_t*>(scalars) + 4 * (ns - 1 - i), 32);
    rc = hipMemcpyAsync(H->s[0], rev.data(), ns * 32, hipMemcpyHostToDevice, C->stream) == hipSuccess ? GM_OK : GM_EHIP;
  }
  if (!rc && hipStreamSynchronize(C->stream) != hipSuccess) rc = GM_EHIP;
  if (rc) {
    hsp_destroy(C, H.get());
    if (rc == GM_EHIP) set_error("herring %s space prover: the copy of the scalar stream failed", M.name);
    return rc;
  }
  std::lock_guard<std::mutex> lk(C->mu);
  *handle = C->next_handle++;
  C->herring_space[*handle] = std::move(H);
  return GM_OK;
}

// Prover::fold (:255-259)
static int hsp_push(Context* C, HerringSpace* H, const uint64_t r[4]) {
  const HspModuleDesc& M = hsp_desc(H);
  const gmh::Fr rr = gmh::Fr::from_limbs(r), tw = gmh::Fr::from_limbs(H->twist), rt = rr * tw;
  const gmh::Fr& pc = M.rhs_points ? rr : rt;  // the point side's challenge: the Lhs folds by r twist, the Rhs by r
  const gmh::Fr& sc = M.rhs_points ? rt : rr;
  uint64_t limbs[4], s_mont[4];
  sc.to_limbs(s_mont);
  int rc = fr_fold_raw(C, H->s[H->cur], H->ls, s_mont, H->s[H->cur ^ 1]);
  if (rc) return rc;
  GM_HIP(hipStreamSynchronize(C->stream));  // s_mont is read by a copy until here
  H->cur ^= 1;
  H->ls = (H->ls + 1) / 2;
  pc.to_limbs(limbs);
  H->pt_ch.insert(H->pt_ch.end(), limbs, limbs + 4);
  pc.to_canonical(limbs);
  H->pt_ch_canon.insert(H->pt_ch_canon.end(), limbs, limbs + 4);
  tw.sqr().to_limbs(H->twist);
  return GM_OK;
}

int hsp_fold(Context* C, HerringSpace* H, const uint64_t r[4]) {
  std::lock_guard<std::mutex> lk(H->mu);
  return hsp_push(C, H, r);
}

// the tensor tables of the point side's challenges and one launch of k_hsp_scalars, on C->stream without a wait
static int hsp_expand(Context* C, HerringSpace* H, const HspPlan& P, bool final_only, const HspWork& W) {
  int rc;
  if (P.k) {
    GM_HIP(hipMemcpyAsync(H->work + W.ch, H->pt_ch.data(), (size_t)P.k * 32, hipMemcpyHostToDevice, C->stream));
    if ((rc = fr_tensor_tables_raw(C, H->work + W.ch, P.k, P.klo, H->work + W.lo, H->work + W.hi))) return rc;
  }
  HspArgs A;
  A.S = H->s[H->cur];
  A.ls = H->ls;
  A.lo = H->work + W.lo;
  A.hi = H->work + W.hi;
  A.k = P.k;
  A.klo = P.klo;
  A.np = H->np;
  A.lanes = final_only ? P.top_points : H->np;
  A.npairs = P.npairs;
  memcpy(A.twist, H->twist, 32);
  A.rhs_points = hsp_desc(H).rhs_points ? 1 : 0;
  A.final_only = final_only ? 1 : 0;
  A.out_a = H->work + W.a;
  A.out_b = H->work + W.b;
  if ((rc = hsp_scalars_raw(C, A))) return rc;
  H->path[1] += 1;
  return GM_OK;
}

// k MSMs of n points each from the start of the stream, scalars at sc[j] (canonical), results normalised Jacobian, `limbs` apart
static int hsp_msm(Context* C, HerringSpace* H, const void* const* sc, size_t n, size_t k, uint64_t* out, size_t limbs) {
  int rc;
  H->path[0] += k;
  if (H->module == HERRING_G1) {  // G1 calls of one message go as one batch
    const size_t ns[2] = {n, n};
    return msm_run_batch(C, H->g1, (int64_t)H->offset, 1, sc, 0, ns, k, true, out);
  }
  for (size_t j = 0; j < k; j++)
    if ((rc = g2_msm_run(C, H->g2, (int64_t)H->offset, 1, sc[j], 0, n, out + j * limbs))) return rc;
  return GM_OK;
}

// SpaceProver::next_message (:118-250)
int hsp_round(Context* C, HerringSpace* H, const uint64_t* challenge, uint64_t* a, uint64_t* b, int* has_msg) {
  const HspModuleDesc& M = hsp_desc(H);
  std::lock_guard<std::mutex> lk(H->mu);
  GM_CHECK(H->round <= H->tot_rounds, GM_ESTATE, "More rounds than needed.");
  int rc;
  if (challenge && (rc = hsp_push(C, H, challenge))) return rc;
  if (H->round == H->tot_rounds) {
    *has_msg = 0;
    return GM_OK;
  }
  const size_t k = H->pt_ch.size() / 4;
  GM_CHECK(k == H->round, GM_ESTATE, "herring %s space prover: %zu challenges at round %zu (at the i-th round, randomness.len() = i)", M.name, k, H->round);
  GM_MSM_LOCK(C);
  const HspPlan P = hsp_plan(H->np, H->ns, (uint32_t)k);
  const HspWork W = hsp_work_layout(H->np, (uint32_t)H->tot_rounds);
  if ((rc = hsp_expand(C, H, P, false, W))) return rc;
  const size_t limbs = M.point->elem / 96 * 18;  // 18 for G1, 36 for G2
  uint64_t res[2 * 36];
  const void* sc[2] = {H->work + W.a, H->work + W.b};
  if ((rc = hsp_msm(C, H, sc, H->np, 2, res, limbs))) return rc;
  memcpy(a, res, limbs * 8);
  memcpy(b, res + limbs, limbs * 8);
  H->round += 1;
  *has_msg = 1;
  return GM_OK;
}

// final_foldings (:270-276): the first item of each folded stream
int hsp_final(Context* C, HerringSpace* H, uint64_t* point0, uint64_t* scalar0, int* has) {
  const HspModuleDesc& M = hsp_desc(H);
  std::lock_guard<std::mutex> lk(H->mu);
  if (H->round != H->tot_rounds) {
    *has = 0;
    return GM_OK;
  }
  GM_MSM_LOCK(C);
  const uint32_t k = (uint32_t)(H->pt_ch.size() / 4);
  int rc = hsp_ensure_work(C, H, std::max<uint32_t>(k, (uint32_t)H->tot_rounds));
  if (rc) return rc;
  const HspPlan P = hsp_plan(H->np, H->ns, k);
  const HspWork W = hsp_work_layout(H->np, std::max<uint32_t>(k, (uint32_t)H->tot_rounds));
  if ((rc = hsp_expand(C, H, P, true, W))) return rc;
  const void* sc[1] = {H->work + W.a};
  if ((rc = hsp_msm(C, H, sc, P.top_points, 1, point0, M.point->elem / 96 * 18))) return rc;
  GM_HIP(hipMemcpyAsync(scalar0, H->s[H->cur] + (H->ls - 1) * 32, 32, hipMemcpyDeviceToHost, C->stream));
  GM_HIP(hipStreamSynchronize(C->stream));
  *has = 1;
  return GM_OK;
}

// TimeProver::from(&SpaceProver) (:279-316): a herring_* prover of the same module at the same round, twist and tot_rounds, whose
// vectors are the folded streams in allocations of its own
int hsp_to_time(Context* C, HerringSpace* H, uint64_t* time_handle) {
  const HspModuleDesc& M = hsp_desc(H);
  const HerringModuleDesc& T = MODULES[H->module];
  std::lock_guard<std::mutex> lk(H->mu);
  const uint32_t k = (uint32_t)(H->pt_ch.size() / 4);
  const HspPlan P = hsp_plan(H->np, H->ns, k);
  const HspTimeBuffers B = hsp_time_buffers(H->np, k);
  auto TP = std::make_unique<HerringProver>();
  TP->module = H->module;
  uint8_t** pt = M.rhs_points ? TP->g : TP->f;  // the point side and the scalar side of the time prover
  size_t* ptcap = M.rhs_points ? TP->gcap : TP->fcap;
  uint8_t** sv = M.rhs_points ? TP->f : TP->g;
  size_t* svcap = M.rhs_points ? TP->fcap : TP->gcap;
  const int cur = B.result_in;
  int rc;
  if ((rc = M.point->alloc(C, B.first, &pt[0], &ptcap[0])) || (rc = M.point->alloc(C, B.second, &pt[1], &ptcap[1])) ||
      (rc = FR_SIDE.alloc(C, P.ls, &sv[cur], &svcap[cur])) || (rc = FR_SIDE.alloc(C, (P.ls + 1) / 2, &sv[cur ^ 1], &svcap[cur ^ 1])) ||
      (rc = C->pool.alloc(T.tmp_slots * (((P.ls + 1) / 2 + 1) * 32), (void**)&TP->tmp, &TP->tmpcap))) {
    herring_destroy(C, TP.get());
    return rc;
  }
  H->path[2] += (B.first + B.second) * M.point->elem;
  H->path[3] += (P.ls + (P.ls + 1) / 2) * 32;
  {
    GM_MSM_LOCK(C);  // the canonical challenges are staged in the MSM workspace (C->msm.misc), as fold_locked stages its two
    rc = C->msm.misc.ensure((size_t)k * 32 + 32);
    if (!rc && k) rc = hipMemcpyAsync(C->msm.misc.p, H->pt_ch_canon.data(), (size_t)k * 32, hipMemcpyHostToDevice, C->stream) == hipSuccess ? GM_OK : GM_EHIP;
    if (!rc && k == 0) rc = records_reverse_launch(C, hsp_key(H), H->np, M.point->elem, pt[0]);
    size_t n = H->np;
    for (uint32_t l = 0; l < k && !rc; l++) {  // level l reads the key (backwards: it is a big-endian stream), then the last level's output
      const uint32_t* s8 = C->msm.misc.as<uint32_t>() + 8 * (size_t)l;
      rc = l == 0 ? M.split_fold_rev(C, hsp_key(H), n, s8, pt[0]) : M.point->split_fold(C, pt[(l - 1) & 1], n, nullptr, s8, pt[l & 1]);
      n = (n + 1) / 2;
    }
    if (!rc) rc = hipMemcpyAsync(sv[cur], H->s[H->cur], P.ls * 32, hipMemcpyDeviceToDevice, C->stream) == hipSuccess ? GM_OK : GM_EHIP;
    if (hipStreamSynchronize(C->stream) != hipSuccess && !rc) rc = GM_EHIP;
  }
  if (rc) {
    herring_destroy(C, TP.get());
    if (rc == GM_EHIP) set_error("herring %s space prover: to_time failed on the device", M.name);
    return rc;
  }
  TP->cur = cur;
  (M.rhs_points ? TP->ng : TP->nf) = P.lp;
  (M.rhs_points ? TP->nf : TP->ng) = P.ls;
  memcpy(TP->twist, H->twist, 32);
  TP->round = H->round;
  TP->tot_rounds = H->tot_rounds;
  std::lock_guard<std::mutex> lkc(C->mu);
  *time_handle = C->next_handle++;
  C->herring[*time_handle] = std::move(TP);
  return GM_OK;
}

}  // namespace gm
