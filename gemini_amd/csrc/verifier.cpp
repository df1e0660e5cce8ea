// The verifiers of the reference as entry points of the library: kzg::VerifierKey::{verify, verify_multi_points}
// (src/kzg/mod.rs:155-244), Subclaim::{new, new_batch} (sumcheck/subclaim.rs:23-97), TensorcheckProof::verify
// (tensorcheck/mod.rs:286-385), snark::Proof::verify (src/snark/verifier.rs:19-119) and psnark::Proof::verify
// (src/psnark/verifier.rs:88-565).
//
// Host orchestration over the library's own C ABI, like snark.cpp: the O(n) part of the snark verifier is gm_fr_powers /
// gm_fr_tensor / gm_fr_hadamard, three gm_spm_bilinear_pm and one gm_fr_eval_le; every group operation is a gm_g1_msm / gm_g2_msm,
// and each KZG check is ONE gm_pairing_multi of two pairs (one final exponentiation) compared with 1.  The field arithmetic
// in between is verifier_host.hpp.  There is one KZG check, one `reduce` and one tensor-check tail for both SNARKs.
// A rejected proof is *ok = 0 with GM_OK; negative codes are for misuse only.  Proof elements are taken as members of their groups,
// as the reference takes them (no subgroup or on-curve checks).
#include "ctx.hpp"
#include "prover_common.hpp"
#include "verifier_host.hpp"

namespace {

using namespace gmprover;
using namespace gmverify;
using gm::VerifierKey;
using gmh::Fq;
using gmh::G1;
using gmh::G2;

#define REJECT()  \
  do {            \
    *ok = 0;      \
    return GM_OK; \
  } while (0)

// ---- points between their forms ---------------------------------------------------------------------------------------
// normalised Jacobian (any representative is accepted) -> the 96-byte affine record of gm_g1_bases_register; identity = zeros
void g1_record(const uint64_t jac[18], uint64_t rec[12], bool negate = false) {
  const G1 p = G1::from_limbs(jac).normalized();
  if (p.is_identity()) {
    memset(rec, 0, 96);
    return;
  }
  p.x.to_limbs(rec);
  (negate ? p.y.neg() : p.y).to_limbs(rec + 6);
}
void g2_record(const uint64_t jac[36], uint64_t rec[24]) {
  const G2 p = G2::from_limbs(jac).normalized();
  if (p.is_identity()) {
    memset(rec, 0, 192);
    return;
  }
  p.x.to_limbs(rec);
  p.y.to_limbs(rec + 12);
}
bool record_is_zero(const uint64_t* rec, size_t limbs) {
  for (size_t i = 0; i < limbs; i++)
    if (rec[i]) return false;
  return true;
}
// host records of `stride` bytes (the infinity flag behind the coordinates when the stride has room) -> packed records
int pack_records(const void* src, size_t stride, size_t n, size_t bytes, std::vector<uint64_t>& out) {
  SC_CHECK(stride >= bytes && stride % 8 == 0, GM_EINVAL, "vk_new: stride %zu for records of %zu bytes", stride, bytes);
  out.assign(n * bytes / 8, 0);
  const uint8_t* s = static_cast<const uint8_t*>(src);
  for (size_t i = 0; i < n; i++) {
    const bool infinity = stride > bytes && s[i * stride + bytes] != 0;
    if (!infinity) memcpy(out.data() + i * bytes / 8, s + i * stride, bytes);
  }
  return GM_OK;
}

// ---- the ONE KZG check ---------------------------------------------------------------------------------------------------
// e(sum_i scalars[i] C_i - [I(tau)] g, g2) * e(-proof, [Z(tau)] g2) == 1 with Z the vanishing polynomial of `points` and I the
// polynomial the claimed evaluations interpolate to (src/kzg/mod.rs:155-175 is the case of one commitment and one point)
// A check as it is STATED: what kzg_check takes.  The *_many entries collect the checks of all their proofs (kzg_check with a
// list answers *ok = 1 for the time being) and run_stated runs them together.
struct StatedCheck {
  std::vector<uint64_t> commitments_jac;  // 18 limbs per commitment
  std::vector<Fr> scalars, i_poly, points;
  uint64_t proof_jac[18];
};
using CheckList = std::vector<StatedCheck>;

int kzg_check(const VerifierKey& vk, const uint64_t* commitments_jac, const std::vector<Fr>& scalars, const std::vector<Fr>& i_poly,
              const std::vector<Fr>& points, const uint64_t proof_jac[18], int* ok, CheckList* defer = nullptr) {
  SC_CHECK(points.size() + 1 <= vk.n2 && i_poly.size() <= vk.n1, GM_EINVAL, "kzg verify: %zu evaluation points, the key holds %zu G1 and %zu G2 powers",
           points.size(), vk.n1, vk.n2);
  if (defer) {
    defer->emplace_back();
    StatedCheck& c = defer->back();
    c.commitments_jac.assign(commitments_jac, commitments_jac + 18 * scalars.size());
    c.scalars = scalars;
    c.i_poly = i_poly;
    c.points = points;
    memcpy(c.proof_jac, proof_jac, sizeof c.proof_jac);
    *ok = 1;
    return GM_OK;
  }
  const std::vector<Fr> zeros = vanishing(points);
  std::vector<uint64_t> zc(4 * zeros.size());
  for (size_t d = 0; d < zeros.size(); d++) zeros[d].to_canonical(zc.data() + 4 * d);
  uint64_t zeros_g2[36];
  RC(gm_g2_msm(vk.g2.data(), 192, zc.data(), zeros.size(), zeros_g2));

  const size_t k = scalars.size(), m = i_poly.size();
  std::vector<uint64_t> bases(12 * (k + m)), sc(4 * (k + m));
  for (size_t i = 0; i < k; i++) {
    g1_record(commitments_jac + 18 * i, bases.data() + 12 * i);
    scalars[i].to_canonical(sc.data() + 4 * i);
  }
  for (size_t d = 0; d < m; d++) {
    memcpy(bases.data() + 12 * (k + d), vk.g1.data() + 12 * d, 96);
    i_poly[d].neg().to_canonical(sc.data() + 4 * (k + d));
  }
  uint64_t lhs[18];
  RC(gm_g1_msm(bases.data(), 96, sc.data(), k + m, lhs));

  uint64_t p1[24], p2[48], gt[72], one[72];
  g1_record(lhs, p1);
  g1_record(proof_jac, p1 + 12, true);
  memcpy(p2, vk.g2.data(), 192);
  g2_record(zeros_g2, p2 + 24);
  RC(gm_pairing_multi(p1, 96, p2, 192, 2, gt));
  RC(gm_gt_one(one));
  *ok = memcmp(gt, one, sizeof gt) == 0 ? 1 : 0;
  return GM_OK;
}

// The stated checks together, ok[i] for check i.  With Z(X) = sum_d z_d X^d the vanishing polynomial of the check's m points (monic),
//   e(L, g2) e(-proof, [Z(tau)] g2) = e(L, g2) prod_{d <= m} e((r - z_d) proof, [tau^d] g2):
// m + 2 pairs against the key's G2 powers as they stand, no G2 arithmetic.  Every G1 point of every check -- L and the m + 1
// multiples of the proof element -- is one segment of ONE gm_g1_lincomb_many launch group; then one segmented Miller launch, one
// final-exponentiation launch and one wait for the whole list (pairing.hip: kzg_checks_run).  A zero z_d, an identity proof element
// or L = identity is an identity record, which k_miller_seg skips.  Fewer checks than gm_set_verify_many_min take kzg_check one by one:
// the verdicts are the same (both sides compute the same element of GT), only the time differs.
int run_stated(const VerifierKey& vk, const CheckList& checks, int* ok) {
  GM_CTX();
  if (checks.size() < C->verify_many_min || vk.d_g2 == nullptr) {
    for (size_t i = 0; i < checks.size(); i++) {
      const StatedCheck& c = checks[i];
      RC(kzg_check(vk, c.commitments_jac.data(), c.scalars, c.i_poly, c.points, c.proof_jac, &ok[i]));
    }
    return GM_OK;
  }
  size_t nterms = 0, nsegs = 0;
  for (const StatedCheck& c : checks) {
    nterms += c.scalars.size() + c.i_poly.size() + c.points.size() + 1;
    nsegs += c.points.size() + 2;
  }
  std::vector<uint64_t> bases(12 * nterms), sc(4 * nterms);
  std::vector<size_t> seg_offsets, check_seg;
  seg_offsets.reserve(nsegs + 1);
  check_seg.reserve(checks.size() + 1);
  size_t t = 0;
  seg_offsets.push_back(0);
  check_seg.push_back(0);
  for (const StatedCheck& c : checks) {
    for (size_t i = 0; i < c.scalars.size(); i++, t++) {
      g1_record(c.commitments_jac.data() + 18 * i, bases.data() + 12 * t);
      c.scalars[i].to_canonical(sc.data() + 4 * t);
    }
    for (size_t d = 0; d < c.i_poly.size(); d++, t++) {
      memcpy(bases.data() + 12 * t, vk.g1.data() + 12 * d, 96);
      c.i_poly[d].neg().to_canonical(sc.data() + 4 * t);
    }
    seg_offsets.push_back(t);  // L
    const std::vector<Fr> zeros = vanishing(c.points);
    uint64_t proof[12];
    g1_record(c.proof_jac, proof);
    for (size_t d = 0; d < zeros.size(); d++, t++) {
      memcpy(bases.data() + 12 * t, proof, 96);
      zeros[d].neg().to_canonical(sc.data() + 4 * t);
      seg_offsets.push_back(t + 1);
    }
    check_seg.push_back(seg_offsets.size() - 1);
  }
  return gm::kzg_checks_run(C, vk.d_g2, bases.data(), 96, sc.data(), seg_offsets.data(), seg_offsets.size() - 1, check_seg.data(), checks.size(), ok);
}

int find_vk(uint64_t h, const VerifierKey** vk) {
  GM_CTX();
  *vk = gm::find_in(C, C->vks, h);
  SC_CHECK(*vk != nullptr, GM_EHANDLE, "unknown verifier key handle %llu", (unsigned long long)h);
  return GM_OK;
}

int verify_multi_points(const VerifierKey& vk, const uint64_t* commitments_jac, size_t ncommitments, const std::vector<Fr>& points,
                        const std::vector<Fr>& evaluations, size_t nrows, const uint64_t proof_jac[18], const Fr& open_chal, int* ok,
                        CheckList* defer = nullptr) {
  SC_CHECK(points.size() + 1 <= vk.n2 && points.size() <= vk.n1, GM_EINVAL, "verify_multi_points: %zu evaluation points, the key holds %zu G1 and %zu G2 powers",
           points.size(), vk.n1, vk.n2);
  if (ncommitments != nrows) REJECT();  // G::msm(..).unwrap() fails on a length mismatch (:236)
  std::vector<Fr> etas(nrows);
  Fr eta = Fr::one();
  for (size_t i = 0; i < nrows; i++) {
    etas[i] = eta;
    eta = eta * open_chal;
  }
  return kzg_check(vk, commitments_jac, etas, interpolate_combination(points, evaluations.data(), nrows, open_chal), points, proof_jac, ok, defer);
}

std::vector<Fr> fr_vector(const uint64_t* mont, size_t n) {
  std::vector<Fr> v(n);
  for (size_t i = 0; i < n; i++) v[i] = Fr::from_limbs(mont + 4 * i);
  return v;
}
int challenge(uint64_t transcript, const char* label, Fr* out) {
  uint64_t c[4];
  RC(gm_transcript_challenge_fr(transcript, L(label), strlen(label), c));
  *out = Fr::from_limbs(c);
  return GM_OK;
}
int absorb_fr(uint64_t transcript, const char* label, const uint64_t* mont) { return gm_transcript_append_fr(transcript, L(label), strlen(label), mont, 1); }
int absorb_g1(uint64_t transcript, const char* label, const uint64_t* jac) { return gm_transcript_append_g1(transcript, L(label), strlen(label), jac, 1, 0); }

// ---- Subclaim (sumcheck/subclaim.rs) ---------------------------------------------------------------------------------------
// the round loop of new (:29-36) and new_batch (:58-63): absorb the message, draw the challenge, reduce the claim
int subclaim_rounds(uint64_t transcript, const uint64_t* messages, size_t rounds, Fr* claim, std::vector<Fr>& challenges) {
  challenges.resize(rounds);
  for (size_t r = 0; r < rounds; r++) {
    RC(gm_transcript_append_fr(transcript, L("evaluations"), 11, messages + 8 * r, 2));
    RC(challenge(transcript, "challenge", &challenges[r]));
    *claim = reduce(*claim, Fr::from_limbs(messages + 8 * r), Fr::from_limbs(messages + 8 * r + 4), challenges[r]);
  }
  return GM_OK;
}
int subclaim_new(uint64_t transcript, const uint64_t* messages, size_t rounds, const uint64_t final_foldings[8], Fr claim, std::vector<Fr>& challenges,
                 int* ok) {
  RC(subclaim_rounds(transcript, messages, rounds, &claim, challenges));
  RC(absorb_fr(transcript, "final-folding", final_foldings));
  RC(absorb_fr(transcript, "final-folding", final_foldings + 4));
  *ok = Fr::from_limbs(final_foldings) * Fr::from_limbs(final_foldings + 4) == claim ? 1 : 0;
  return GM_OK;
}
int subclaim_new_batch(uint64_t transcript, const uint64_t* messages, size_t rounds, const uint64_t* final_foldings, const std::vector<Fr>& asserted_sums,
                       std::vector<Fr>& challenges, int* ok) {
  const size_t k = asserted_sums.size();
  std::vector<Fr> coeff(k);
  Fr claim = Fr::zero();
  for (size_t j = 0; j < k; j++) {
    RC(challenge(transcript, "batch-sumcheck", &coeff[j]));
    claim = claim + coeff[j] * asserted_sums[j];
  }
  RC(subclaim_rounds(transcript, messages, rounds, &claim, challenges));
  Fr expected = Fr::zero();
  for (size_t j = 0; j < k; j++) {
    RC(absorb_fr(transcript, "final-folding-lhs", final_foldings + 8 * j));
    RC(absorb_fr(transcript, "final-folding-rhs", final_foldings + 8 * j + 4));
    expected = expected + Fr::from_limbs(final_foldings + 8 * j) * Fr::from_limbs(final_foldings + 8 * j + 4) * coeff[j];
  }
  *ok = expected == claim ? 1 : 0;
  return GM_OK;
}

// ---- TensorcheckProof::verify (tensorcheck/mod.rs:286-385) -----------------------------------------------------------------
struct TensorInstance {
  std::vector<Fr> asserted_res, fold_randomness;
  Fr direct_base_evals[2];
};
int tensorcheck_verify(uint64_t transcript, const VerifierKey& vk, const gm_tensorcheck_proof* P, const uint64_t* base_commitments_jac, size_t ncommitments,
                       const std::vector<TensorInstance>& instances, const Fr& eval_chal, const Fr& batch_challenge, int* ok, CheckList* defer = nullptr) {
  const Fr two_inv = fr_u64(2).inv(), two_beta_inv = eval_chal.dbl().inv();
  std::vector<Fr> evaluations = fr_vector(P->base_evaluations, 3 * P->nbase);
  size_t offset = 0;
  for (const TensorInstance& I : instances) {
    SC_CHECK(I.fold_randomness.size() >= 2, GM_EINVAL, "tensorcheck_verify: an instance needs two folding challenges or more");
    const size_t rounds = I.fold_randomness.size() - 1;
    if (offset + rounds > P->nfold) REJECT();  // folded evaluations missing
    Fr pos = I.direct_base_evals[0], neg = I.direct_base_evals[1];
    for (size_t i = 0; i < rounds; i++) {
      const uint64_t* fe = P->fold_evaluations + 8 * (offset + i);
      evaluations.push_back(evaluate_sq_fp(pos, neg, I.fold_randomness[i], two_inv, two_beta_inv));
      pos = Fr::from_limbs(fe);
      neg = Fr::from_limbs(fe + 4);
      evaluations.push_back(pos);
      evaluations.push_back(neg);
    }
    offset += rounds;
    Fr lc = Fr::zero(), bc = Fr::one();
    for (const Fr& a : I.asserted_res) {
      lc = lc + a * bc;
      bc = bc * batch_challenge;
    }
    if (!(evaluate_sq_fp(pos, neg, I.fold_randomness[rounds], two_inv, two_beta_inv) == lc)) REJECT();
  }
  for (size_t k = 0; k < 3 * P->nbase; k++) RC(absorb_fr(transcript, "eval", P->base_evaluations + 4 * k));
  for (size_t k = 0; k < 2 * P->nfold; k++) RC(absorb_fr(transcript, "eval", P->fold_evaluations + 4 * k));
  Fr open_chal;
  RC(challenge(transcript, "open-chal", &open_chal));
  std::vector<uint64_t> all(18 * (ncommitments + P->nfold));
  if (ncommitments) memcpy(all.data(), base_commitments_jac, 144 * ncommitments);
  if (P->nfold) memcpy(all.data() + 18 * ncommitments, P->fold_commitments, 144 * P->nfold);
  return verify_multi_points(vk, all.data(), ncommitments + P->nfold, {eval_chal.sqr(), eval_chal, eval_chal.neg()}, evaluations, evaluations.size() / 3,
                             P->evaluation_proof, open_chal, ok, defer);
}

// x(beta) + beta^|x| w(beta) and the same at -beta: z = x || w                                  src/snark/verifier.rs:91-104
int z_evaluations(uint64_t x_vec, const Fr& beta, const Fr& w_pos, const Fr& w_neg, Fr* z_pos, Fr* z_neg) {
  size_t nx = 0;
  if (x_vec) RC(gm_fr_vec_len(x_vec, &nx));
  uint64_t pts[8], xe[8] = {0};
  beta.to_limbs(pts);
  beta.neg().to_limbs(pts + 4);
  if (nx) RC(gm_fr_eval_le(x_vec, pts, 2, xe));
  const Fr beta_power = fr_pow_u64(beta, nx);
  *z_pos = Fr::from_limbs(xe) + beta_power * w_pos;
  *z_neg = Fr::from_limbs(xe + 4) + ((nx & 1) ? beta_power.neg() : beta_power) * w_neg;
  return GM_OK;
}

struct TranscriptNew : TranscriptGuard {
  int open(int g1_encoding) {
    static const char protocol[] = "GEMINI-v0";  // PROTOCOL_NAME, src/lib.rs:74
    RC(gm_transcript_new(L(protocol), sizeof protocol - 1, &h));
    if (g1_encoding) RC(gm_transcript_set_g1_encoding(h, g1_encoding));
    return GM_OK;
  }
};

int ceil_log2(size_t n) {
  int k = 0;
  while (((size_t)1 << k) < n) k++;
  return k;
}

}  // namespace

// ==== the C ABI ================================================================================================================
extern "C" int gm_vk_new(const void* g1, size_t g1_stride, size_t n1, const void* g2, size_t g2_stride, size_t n2, uint64_t* vk) {
  GM_CTX();
  SC_CHECK(g1 && g2 && vk && n1 >= 1 && n2 >= 1, GM_EINVAL, "vk_new: null pointer or an empty key");
  auto K = std::make_unique<VerifierKey>();
  RC(pack_records(g1, g1_stride, n1, 96, K->g1));
  RC(pack_records(g2, g2_stride, n2, 192, K->g2));
  K->n1 = n1;
  K->n2 = n2;
  {  // the G2 powers stay on the device with the key: the batched checks pair against them as they stand
    std::unique_ptr<gm::G2Bases> d;
    RC(gm::g2_bases_from_host(C, K->g2.data(), 192, n2, d));
    K->d_g2 = d->d;
  }
  *vk = gm::put_in(C, C->vks, std::move(K));
  return GM_OK;
}

extern "C" int gm_vk_from_trapdoor(const uint64_t g1_affine[12], const uint64_t g2_affine[24], const uint64_t tau[4], size_t max_eval_points, uint64_t* vk) {
  GM_CTX();
  SC_CHECK(g1_affine && g2_affine && tau && vk && max_eval_points >= 1, GM_EINVAL, "vk_from_trapdoor: null pointer or no evaluation point");
  const size_t n1 = max_eval_points, n2 = max_eval_points + 1;
  // both halves are fixed-base products by the canonical powers of tau: an MSM of one pair each, a handful of them
  std::vector<uint64_t> g1(12 * n1), g2(24 * n2);
  Fr t = Fr::one();
  const Fr tau_m = Fr::from_canonical(tau);
  for (size_t i = 0; i < n2; i++) {
    uint64_t s[4], j1[18], j2[36];
    t.to_canonical(s);
    if (i < n1) {
      RC(gm_g1_msm(g1_affine, 96, s, 1, j1));
      g1_record(j1, g1.data() + 12 * i);
    }
    RC(gm_g2_msm(g2_affine, 192, s, 1, j2));
    g2_record(j2, g2.data() + 24 * i);
    t = t * tau_m;
  }
  return gm_vk_new(g1.data(), 96, n1, g2.data(), 192, n2, vk);
}

extern "C" int gm_vk_free(uint64_t vk) {
  GM_CTX();
  std::unique_ptr<VerifierKey> K = gm::take_from(C, C->vks, vk);
  SC_CHECK(K != nullptr, GM_EHANDLE, "vk_free: unknown verifier key handle %llu", (unsigned long long)vk);
  if (K->d_g2) (void)gm::raw_free(K->d_g2);
  return GM_OK;
}

extern "C" int gm_vk_len(uint64_t vk, size_t* n1, size_t* n2) {
  const VerifierKey* K;
  RC(find_vk(vk, &K));
  if (n1) *n1 = K->n1;
  if (n2) *n2 = K->n2;
  return GM_OK;
}

// serialize_uncompressed(&powers_of_g2): u64 length, then 192 bytes per point in the framing `encoding` names
// (gm_transcript_set_g1_encoding): what psnark absorbs as b"ck".  out = NULL asks for the size only.
extern "C" int gm_vk_g2_bytes(uint64_t vk, int encoding, uint8_t* out, size_t cap, size_t* len) {
  const VerifierKey* K;
  RC(find_vk(vk, &K));
  SC_CHECK(len != nullptr && (encoding == 0 || encoding == 1), GM_EINVAL, "vk_g2_bytes: null pointer or unknown encoding %d", encoding);
  *len = 8 + 192 * K->n2;
  if (!out) return GM_OK;
  SC_CHECK(cap >= *len, GM_EINVAL, "vk_g2_bytes: %zu bytes do not hold %zu", cap, *len);
  memset(out, 0, *len);
  const uint64_t n = K->n2;
  memcpy(out, &n, 8);
  for (size_t i = 0; i < K->n2; i++) {
    const uint64_t* rec = K->g2.data() + 24 * i;
    uint8_t* o = out + 8 + 192 * i;
    if (record_is_zero(rec, 24)) {
      o[encoding ? 0 : 191] |= 0x40;
      continue;
    }
    uint64_t c[4][6];  // x.c0, x.c1, y.c0, y.c1
    for (int j = 0; j < 4; j++) Fq::from_limbs(rec + 6 * j).to_canonical(c[j]);
    if (encoding == 1) {  // zcash: x.c1 | x.c0 | y.c1 | y.c0, big-endian
      static const int order[4] = {1, 0, 3, 2};
      for (int j = 0; j < 4; j++)
        for (int b = 0; b < 48; b++) o[48 * j + b] = (uint8_t)(c[order[j]][(47 - b) / 8] >> (8 * ((47 - b) % 8)));
      continue;
    }
    for (int j = 0; j < 4; j++) memcpy(o + 48 * j, c[j], 48);
    // the sign flag: y > -y in ark-ff's order of Fq2 (c1 first, then c0)
    uint64_t nc[2][6];
    Fq::from_limbs(rec + 12).neg().to_canonical(nc[0]);
    Fq::from_limbs(rec + 18).neg().to_canonical(nc[1]);
    int cmp = 0;
    for (int part = 1; part >= 0 && !cmp; part--)
      for (int l = 5; l >= 0 && !cmp; l--)
        if (c[2 + part][l] != nc[part][l]) cmp = c[2 + part][l] > nc[part][l] ? 1 : -1;
    if (cmp > 0) o[191] |= 0x80;
  }
  return GM_OK;
}

extern "C" int gm_kzg_verify(uint64_t vk, const uint64_t commitment_jac[18], const uint64_t alpha_mont[4], const uint64_t evaluation_mont[4],
                             const uint64_t proof_jac[18], int* ok) {
  const VerifierKey* K;
  RC(find_vk(vk, &K));
  SC_CHECK(commitment_jac && alpha_mont && evaluation_mont && proof_jac && ok, GM_EINVAL, "kzg_verify: null pointer");
  return kzg_check(*K, commitment_jac, {Fr::one()}, {Fr::from_limbs(evaluation_mont)}, {Fr::from_limbs(alpha_mont)}, proof_jac, ok);
}

extern "C" int gm_kzg_verify_multi_points(uint64_t vk, const uint64_t* commitments_jac, size_t ncommitments, const uint64_t* eval_points_mont, size_t npoints,
                                          const uint64_t* evaluations_mont, size_t nrows, const uint64_t proof_jac[18], const uint64_t open_chal_mont[4], int* ok) {
  const VerifierKey* K;
  RC(find_vk(vk, &K));
  SC_CHECK((commitments_jac || !ncommitments) && eval_points_mont && (evaluations_mont || !nrows) && proof_jac && open_chal_mont && ok && npoints >= 1, GM_EINVAL,
           "kzg_verify_multi_points: null pointer or no evaluation point");
  return verify_multi_points(*K, commitments_jac, ncommitments, fr_vector(eval_points_mont, npoints), fr_vector(evaluations_mont, nrows * npoints), nrows, proof_jac,
                             Fr::from_limbs(open_chal_mont), ok);
}

extern "C" int gm_sumcheck_subclaim(uint64_t transcript, const uint64_t* messages, size_t rounds, const uint64_t final_foldings[8], const uint64_t asserted_sum_mont[4],
                                    uint64_t* challenges_mont, int* ok) {
  GM_CTX();
  (void)C;
  SC_CHECK((messages || !rounds) && final_foldings && asserted_sum_mont && (challenges_mont || !rounds) && ok, GM_EINVAL, "sumcheck_subclaim: null pointer");
  std::vector<Fr> ch;
  RC(subclaim_new(transcript, messages, rounds, final_foldings, Fr::from_limbs(asserted_sum_mont), ch, ok));
  for (size_t r = 0; r < rounds; r++) ch[r].to_limbs(challenges_mont + 4 * r);
  return GM_OK;
}

extern "C" int gm_sumcheck_subclaim_batch(uint64_t transcript, const uint64_t* messages, size_t rounds, const uint64_t* final_foldings, const uint64_t* asserted_sums_mont,
                                          size_t k, uint64_t* challenges_mont, int* ok) {
  GM_CTX();
  (void)C;
  SC_CHECK((messages || !rounds) && (final_foldings || !k) && (asserted_sums_mont || !k) && (challenges_mont || !rounds) && ok, GM_EINVAL,
           "sumcheck_subclaim_batch: null pointer");
  std::vector<Fr> ch;
  RC(subclaim_new_batch(transcript, messages, rounds, final_foldings, fr_vector(asserted_sums_mont, k), ch, ok));
  for (size_t r = 0; r < rounds; r++) ch[r].to_limbs(challenges_mont + 4 * r);
  return GM_OK;
}

extern "C" int gm_tensorcheck_verify(uint64_t transcript, uint64_t vk, const gm_tensorcheck_proof* proof, const uint64_t* base_commitments_jac, size_t ncommitments,
                                     const gm_tensorcheck_claim* claims, size_t nclaims, const uint64_t eval_chal_mont[4], const uint64_t batch_challenge_mont[4],
                                     int* ok) {
  const VerifierKey* K;
  RC(find_vk(vk, &K));
  SC_CHECK(proof && (base_commitments_jac || !ncommitments) && claims && nclaims && eval_chal_mont && batch_challenge_mont && ok, GM_EINVAL,
           "tensorcheck_verify: null pointer or no claim");
  SC_CHECK((proof->fold_commitments && proof->fold_evaluations) || !proof->nfold, GM_EINVAL, "tensorcheck_verify: null folding arrays");
  SC_CHECK(proof->base_evaluations || !proof->nbase, GM_EINVAL, "tensorcheck_verify: null base evaluations");
  std::vector<TensorInstance> inst(nclaims);
  for (size_t i = 0; i < nclaims; i++) {
    SC_CHECK(claims[i].asserted_res_mont && claims[i].fold_randomness_mont, GM_EINVAL, "tensorcheck_verify: null pointer in claim %zu", i);
    inst[i].asserted_res = fr_vector(claims[i].asserted_res_mont, claims[i].nasserted);
    inst[i].fold_randomness = fr_vector(claims[i].fold_randomness_mont, claims[i].nrandomness);
    inst[i].direct_base_evals[0] = Fr::from_limbs(claims[i].direct_base_evals_mont);
    inst[i].direct_base_evals[1] = Fr::from_limbs(claims[i].direct_base_evals_mont + 4);
  }
  return tensorcheck_verify(transcript, *K, proof, base_commitments_jac, ncommitments, inst, Fr::from_limbs(eval_chal_mont), Fr::from_limbs(batch_challenge_mont), ok);
}

// snark::Proof::verify (src/snark/verifier.rs:19-119); with `defer` the KZG check at the end is stated, not run
static int snark_verify_one(const uint64_t matrices[3], uint64_t x_vec, const VerifierKey* K, int g1_encoding, const gm_snark_proof* P, int* ok, CheckList* defer) {
  SC_CHECK(matrices && P && ok && (P->messages[0] || !P->rounds[0]) && (P->messages[1] || !P->rounds[1]), GM_EINVAL, "snark_verify: null pointer");
  SC_CHECK((P->fold_commitments && P->fold_evaluations) || !P->nfold, GM_EINVAL, "snark_verify: null folding arrays");
  size_t n = 0;
  for (int k = 0; k < 3; k++) {
    size_t rows = 0;
    RC(gm_spm_shape(matrices[k], &rows, nullptr, nullptr));
    SC_CHECK(k == 0 || rows == n, GM_EINVAL, "snark_verify: the matrices differ in their number of rows");
    n = rows;
  }
  TranscriptNew T;
  RC(T.open(g1_encoding));
  RC(absorb_g1(T.h, "witness", P->witness_commitment));
  Fr alpha, eta, gamma, beta;
  RC(challenge(T.h, "alpha", &alpha));
  RC(absorb_fr(T.h, "zc(alpha)", P->zc_alpha));
  const Fr zc_alpha = Fr::from_limbs(P->zc_alpha);
  std::vector<Fr> ch1, ch2;
  int good = 0;
  RC(subclaim_new(T.h, P->messages[0], P->rounds[0], P->final_foldings[0], zc_alpha, ch1, &good));
  if (!good) REJECT();
  RC(challenge(T.h, "eta", &eta));
  const Fr ff1[2] = {Fr::from_limbs(P->final_foldings[0]), Fr::from_limbs(P->final_foldings[0] + 4)};
  RC(subclaim_new(T.h, P->messages[1], P->rounds[1], P->final_foldings[1], ff1[0] + eta * ff1[1] + eta.sqr() * zc_alpha, ch2, &good));
  if (!good) REJECT();
  RC(challenge(T.h, "batch_challenge", &gamma));
  for (size_t k = 0; k < P->nfold; k++) RC(absorb_g1(T.h, "commitment", P->fold_commitments + 18 * k));
  RC(challenge(T.h, "evaluation-chal", &beta));

  // the matrices at the powers of +-beta against tensor(rho) o powers(alpha), tensor(rho), powers(alpha)          :63-88
  // a first sumcheck of other than ceil(log2 n) rounds cannot come from the prover (the reference's ip would panic on the lengths)
  if (n == 0 || P->rounds[0] == 0 || P->rounds[0] != (size_t)ceil_log2(n > 2 ? n : 2)) REJECT();
  if (P->rounds[1] < 2) REJECT();
  const size_t nt = (size_t)1 << P->rounds[0];
  Vecs V;
  uint64_t beta_powers, weights[3], lim[4];
  std::vector<uint64_t> rho(4 * ch1.size());
  for (size_t i = 0; i < ch1.size(); i++) ch1[i].to_limbs(rho.data() + 4 * i);
  RC(V.alloc(n, &beta_powers));
  beta.to_limbs(lim);
  RC(gm_fr_powers(lim, n, beta_powers));
  for (int k = 0; k < 3; k++) RC(V.alloc(nt, &weights[k]));
  RC(gm_fr_tensor(rho.data(), ch1.size(), weights[1]));
  alpha.to_limbs(lim);
  RC(gm_fr_powers(lim, nt, weights[2]));
  RC(gm_fr_hadamard(weights[1], weights[2], weights[0]));
  Fr m_pos = Fr::zero(), m_neg = Fr::zero(), e = Fr::one();
  for (int k = 0; k < 3; k++) {
    uint64_t pos[4], neg[4];
    RC(gm_spm_bilinear_pm(matrices[k], beta_powers, weights[k], pos, neg));
    m_pos = m_pos + e * Fr::from_limbs(pos);
    m_neg = m_neg + e * Fr::from_limbs(neg);
    e = e * eta;
  }
  Fr z_pos, z_neg;
  RC(z_evaluations(x_vec, beta, Fr::from_limbs(P->base_evaluations + 4), Fr::from_limbs(P->base_evaluations + 8), &z_pos, &z_neg));

  gm_tensorcheck_proof tc;
  memset(&tc, 0, sizeof tc);
  tc.nfold = tc.cap_folds = P->nfold;
  tc.fold_commitments = P->fold_commitments;
  tc.fold_evaluations = P->fold_evaluations;
  memcpy(tc.evaluation_proof, P->evaluation_proof, sizeof tc.evaluation_proof);
  tc.nbase = 1;
  tc.base_evaluations = const_cast<uint64_t*>(P->base_evaluations);
  std::vector<TensorInstance> inst(1);
  inst[0].asserted_res = {Fr::from_limbs(P->final_foldings[1]), Fr::from_limbs(P->final_foldings[1] + 4)};
  inst[0].fold_randomness = ch2;
  inst[0].direct_base_evals[0] = m_pos + gamma * z_pos;
  inst[0].direct_base_evals[1] = m_neg + gamma * z_neg;
  return tensorcheck_verify(T.h, *K, &tc, P->witness_commitment, 1, inst, beta, gamma, ok, defer);
}
extern "C" int gm_snark_verify(const uint64_t matrices[3], uint64_t x_vec, uint64_t vk, int g1_encoding, const gm_snark_proof* P, int* ok) {
  const VerifierKey* K;
  RC(find_vk(vk, &K));
  return snark_verify_one(matrices, x_vec, K, g1_encoding, P, ok, nullptr);
}

// psnark::Proof::verify (src/psnark/verifier.rs:88-565): O(log n) field arithmetic around two KZG checks.  With `defer` both are
// stated: the replay behind the first does not depend on its verdict (the prover's data is absorbed either way).
static int psnark_verify_one(uint64_t x_vec, size_t num_variables, size_t nnz, const uint64_t* index_commitments, uint64_t vk, const VerifierKey* K, int g1_encoding,
                             const gm_psnark_proof* P, int* ok, CheckList* defer) {
  SC_CHECK(index_commitments && P && ok && num_variables >= 1 && nnz >= 1, GM_EINVAL, "psnark_verify: null pointer or an empty instance");
  for (int k = 0; k < 3; k++) SC_CHECK(P->messages[k] || !P->rounds[k], GM_EINVAL, "psnark_verify: null messages");
  SC_CHECK((P->fold_commitments && P->fold_evaluations) || !P->nfold, GM_EINVAL, "psnark_verify: null folding arrays");
  TranscriptNew T;
  RC(T.open(g1_encoding));
  RC(absorb_g1(T.h, "witness", P->witness_commitment));
  {
    size_t len = 0;
    RC(gm_vk_g2_bytes(vk, g1_encoding, nullptr, 0, &len));
    std::vector<uint8_t> ck(len);
    RC(gm_vk_g2_bytes(vk, g1_encoding, ck.data(), len, &len));
    RC(gm_transcript_append_message(T.h, L("ck"), 2, ck.data(), len));
  }
  RC(gm_transcript_append_g1(T.h, L("instance"), 8, index_commitments, 5, 1));
  Fr alpha, eta, zeta, y, z, mu, open_chal, bc, beta;
  RC(challenge(T.h, "alpha", &alpha));
  const Fr zc_alpha = Fr::from_limbs(P->zc_alpha);
  RC(absorb_fr(T.h, "zc(alpha)", P->zc_alpha));
  std::vector<Fr> ch1, ch2, ch3;
  int good = 0;
  RC(subclaim_new(T.h, P->messages[0], P->rounds[0], P->final_foldings[0], zc_alpha, ch1, &good));
  if (!good) REJECT();
  RC(absorb_g1(T.h, "ra*", P->r_star_commitments[0]));
  RC(absorb_g1(T.h, "rb*", P->r_star_commitments[1]));
  RC(absorb_g1(T.h, "rc*", P->r_star_commitments[2]));
  RC(absorb_g1(T.h, "z*", P->z_star_commitment));
  RC(challenge(T.h, "chal", &eta));
  const Fr ff1[2] = {Fr::from_limbs(P->final_foldings[0]), Fr::from_limbs(P->final_foldings[0] + 4)};
  RC(subclaim_new(T.h, P->messages[1], P->rounds[1], P->final_foldings[1], ff1[0] + ff1[1] * eta + zc_alpha * eta.sqr(), ch2, &good));
  if (!good) REJECT();
  const Fr ff2[2] = {Fr::from_limbs(P->final_foldings[1]), Fr::from_limbs(P->final_foldings[1] + 4)};
  RC(challenge(T.h, "zeta", &zeta));
  RC(absorb_g1(T.h, "sorted_alpha_commitment", P->sorted_commitments[1]));
  RC(absorb_g1(T.h, "sorted_r_commitment", P->sorted_commitments[0]));
  RC(absorb_g1(T.h, "sorted_z_commitment", P->sorted_commitments[2]));
  RC(challenge(T.h, "gamma", &y));
  RC(challenge(T.h, "chi", &z));
  // (the labels repeat set_r_ep / subset_r_ep for the alpha products: :169-176); products = r, alpha, z x (set, subset, sorted)
  RC(absorb_fr(T.h, "set_r_ep", P->products[3]));
  RC(absorb_fr(T.h, "subset_r_ep", P->products[4]));
  RC(absorb_fr(T.h, "set_r_ep", P->products[0]));
  RC(absorb_fr(T.h, "subset_r_ep", P->products[1]));
  RC(absorb_fr(T.h, "set_z_ep", P->products[6]));
  RC(absorb_fr(T.h, "subset_z_ep", P->products[7]));
  for (int k = 0; k < 9; k++) RC(absorb_g1(T.h, "acc_v", P->acc_v_commitments[k]));
  RC(challenge(T.h, "ep-chal", &mu));
  RC(challenge(T.h, "open-chal", &open_chal));
  {
    uint64_t commitments[10 * 18];
    memcpy(commitments, P->r_star_commitments[0], 144);
    memcpy(commitments + 18, P->acc_v_commitments, 9 * 144);
    RC(verify_multi_points(*K, commitments, 10, {mu}, fr_vector(&P->ralpha_star_acc_mu_evals[0][0], 10), 10, P->ralpha_star_acc_mu_proof, open_chal, &good, defer));
    if (!good) REJECT();
  }
  for (int k = 0; k < 10; k++) RC(absorb_fr(T.h, "ralpha_star_acc_mu", P->ralpha_star_acc_mu_evals[k]));
  RC(absorb_g1(T.h, "ralpha_star_mu_proof", P->ralpha_star_acc_mu_proof));
  const Fr rstars[2] = {Fr::from_limbs(P->rstars_vals[0]), Fr::from_limbs(P->rstars_vals[1])};
  std::vector<Fr> asserted3 = fr_vector(&P->claimed_sumchecks[0][0], 9);
  asserted3.push_back(rstars[0]);
  asserted3.push_back(rstars[1]);
  asserted3.push_back((ff2[1] - rstars[0] - rstars[1] * eta) * eta.sqr().inv());
  asserted3.push_back(Fr::from_limbs(P->ralpha_star_acc_mu_evals[0]));
  RC(subclaim_new_batch(T.h, P->messages[2], P->rounds[2], &P->third_final_foldings[0][0], asserted3, ch3, &good));
  if (!good) REJECT();
  RC(challenge(T.h, "batch_challenge", &bc));
  for (size_t k = 0; k < P->nfold; k++) RC(absorb_g1(T.h, "commitment", P->fold_commitments + 18 * k));
  RC(challenge(T.h, "evaluation-chal", &beta));
  if (ch1.size() >= 40 || ch3.size() < ch2.size()) REJECT();  // no prover sends these round counts (the reference's hadamard would panic)

  auto lhs3 = [&](int i) { return Fr::from_limbs(P->third_final_foldings[i]); };
  auto rhs3 = [&](int i) { return Fr::from_limbs(P->third_final_foldings[i] + 4); };
  auto be = [&](int i, int col) { return Fr::from_limbs(P->base_evaluations[i] + 4 * col); };
  std::vector<TensorInstance> inst(4);
  for (int i = 0; i < 9; i++) inst[0].asserted_res.push_back(lhs3(i));
  inst[0].asserted_res.push_back(lhs3(12));
  for (int i = 0; i < 13; i++) inst[1].asserted_res.push_back(rhs3(i));
  inst[2].asserted_res = {ff2[0]};
  inst[3].asserted_res = {lhs3(9), lhs3(10), lhs3(11)};
  // first body: the nine accumulated products, then r*
  {
    Fr tmp = Fr::one(), d[2] = {Fr::zero(), Fr::zero()};
    for (int t = 0; t < 10; t++) {
      const int i = t < 9 ? 13 + t : 2;
      d[0] = d[0] + tmp * be(i, 1);
      d[1] = d[1] + tmp * be(i, 2);
      tmp = tmp * bc;
    }
    inst[0].direct_base_evals[0] = d[0];
    inst[0].direct_base_evals[1] = d[1];
  }
  // second body: the nine shifted monic lookup vectors, then val_a, val_b, val_c, alpha*
  const uint64_t set_len = (uint64_t)1 << ch1.size();
  Fr z_ev[2];
  RC(z_evaluations(x_vec, beta, be(0, 1), be(0, 2), &z_ev[0], &z_ev[1]));
  for (int s = 0; s < 2; s++) {
    const Fr pt = s ? beta.neg() : beta;
    const int col = 1 + s;
    const Fr terms[13] = {
        // lookup r*
        plookup_set_eval(evaluate_tensor_poly(ch1.data(), ch1.size(), pt) + zeta * evaluate_index_poly(pt, set_len), pt, y, z, set_len),
        plookup_subset_eval(be(2, col), be(5, col), pt, y, zeta, nnz),
        plookup_set_eval(be(10, col), pt, y, z, set_len + nnz),
        // lookup alpha*
        plookup_set_eval(evaluate_geometric_poly(alpha * pt, set_len) + zeta * evaluate_index_poly(pt, set_len), pt, y, z, set_len),
        plookup_subset_eval(be(3, col), be(5, col), pt, y, zeta, nnz),
        plookup_set_eval(be(11, col), pt, y, z, set_len + nnz),
        // lookup z*
        plookup_set_eval(z_ev[s] + zeta * evaluate_index_poly(pt, num_variables), pt, y, z, num_variables),
        plookup_subset_eval(be(4, col), be(6, col), pt, y, zeta, nnz),
        plookup_set_eval(be(12, col), pt, y, z, num_variables + nnz),
        // val_a, val_b, val_c, alpha*
        be(7, col), be(8, col), be(9, col), be(3, col)};
    Fr acc = Fr::zero(), tmp = Fr::one();
    for (const Fr& t : terms) {
      acc = acc + t * tmp;
      tmp = tmp * bc;
    }
    inst[1].direct_base_evals[s] = acc;
    inst[2].direct_base_evals[s] = be(4, col);
    inst[3].direct_base_evals[s] = be(1, col) + be(2, col) * bc + be(3, col) * bc.sqr();
  }
  inst[0].fold_randomness = ch3;
  {
    Fr m2 = mu;  // powers2(mu): mu, mu^2, mu^4, ...
    for (Fr& c : inst[0].fold_randomness) {
      c = c * m2;
      m2 = m2.sqr();
    }
  }
  inst[1].fold_randomness = ch3;
  inst[2].fold_randomness = ch2;
  inst[3].fold_randomness = ch2;
  for (size_t i = 0; i < ch2.size(); i++) inst[3].fold_randomness[i] = ch2[i] * ch3[i];
  for (const TensorInstance& I : inst)
    if (I.fold_randomness.size() < 2) REJECT();

  // witness, ra*, rb*, rc*, z*, the five index commitments, sorted r / alpha / z, the nine accumulated products
  uint64_t base_commitments[22 * 18];
  memcpy(base_commitments, P->witness_commitment, 144);
  memcpy(base_commitments + 18, P->r_star_commitments, 3 * 144);
  memcpy(base_commitments + 4 * 18, P->z_star_commitment, 144);
  memcpy(base_commitments + 5 * 18, index_commitments, 5 * 144);
  memcpy(base_commitments + 10 * 18, P->sorted_commitments, 3 * 144);
  memcpy(base_commitments + 13 * 18, P->acc_v_commitments, 9 * 144);
  gm_tensorcheck_proof tc;
  memset(&tc, 0, sizeof tc);
  tc.nfold = tc.cap_folds = P->nfold;
  tc.fold_commitments = P->fold_commitments;
  tc.fold_evaluations = P->fold_evaluations;
  memcpy(tc.evaluation_proof, P->evaluation_proof, sizeof tc.evaluation_proof);
  tc.nbase = 22;
  tc.base_evaluations = const_cast<uint64_t*>(&P->base_evaluations[0][0]);
  return tensorcheck_verify(T.h, *K, &tc, base_commitments, 22, inst, beta, bc, ok, defer);
}
extern "C" int gm_psnark_verify(uint64_t x_vec, size_t num_variables, size_t nnz, const uint64_t* index_commitments, uint64_t vk, int g1_encoding,
                                const gm_psnark_proof* P, int* ok) {
  const VerifierKey* K;
  RC(find_vk(vk, &K));
  return psnark_verify_one(x_vec, num_variables, nnz, index_commitments, vk, K, g1_encoding, P, ok, nullptr);
}

// ==== many proofs in one call ==================================================================================================
// One proof of a batch: its host part ran to `rc` / `ok` and stated the checks [first, first + count).  What the single entry would
// have answered follows from the verdicts of those checks IN ORDER: it stops at the first one that fails (ok = 0, GM_OK, whatever
// came behind it -- an error code included, which the single entry never reaches), and behind checks that all pass it answers what
// the host part answered.
namespace {
struct ProofRun {
  int rc = GM_OK, ok = 0;
  size_t first = 0, count = 0;
};
int settle(const VerifierKey& K, const CheckList& checks, const std::vector<ProofRun>& runs, int* ok) {
  std::vector<int> verdict(checks.size(), 0);
  RC(run_stated(K, checks, verdict.data()));
  for (size_t s = 0; s < runs.size(); s++) {
    const ProofRun& r = runs[s];
    bool pass = true;
    for (size_t i = 0; i < r.count && pass; i++) pass = verdict[r.first + i] != 0;
    if (!pass) {
      ok[s] = 0;
      continue;
    }
    if (r.rc != GM_OK) return r.rc;  // the code is that proof's; gm_last_error may hold the text of a later proof's failure
    ok[s] = r.ok;
  }
  return GM_OK;
}
}  // namespace

extern "C" int gm_kzg_verify_multi_points_many(uint64_t vk, size_t S, const uint64_t* commitments_jac, const size_t* commitment_offsets, const uint64_t* eval_points_mont,
                                               const size_t* point_offsets, const uint64_t* evaluations_mont, const size_t* row_offsets, const uint64_t* proofs_jac,
                                               const uint64_t* open_chals_mont, int* ok) {
  const VerifierKey* K;
  RC(find_vk(vk, &K));
  if (S == 0) return GM_OK;
  SC_CHECK(commitment_offsets && point_offsets && row_offsets && eval_points_mont && proofs_jac && open_chals_mont && ok, GM_EINVAL,
           "kzg_verify_multi_points_many: null pointer");
  SC_CHECK(commitment_offsets[0] == 0 && point_offsets[0] == 0 && row_offsets[0] == 0, GM_EINVAL, "kzg_verify_multi_points_many: the offset arrays start at 0");
  size_t eval_at = 0;
  std::vector<size_t> eval_offsets(S);
  for (size_t s = 0; s < S; s++) {
    SC_CHECK(commitment_offsets[s] <= commitment_offsets[s + 1] && point_offsets[s] < point_offsets[s + 1] && row_offsets[s] <= row_offsets[s + 1], GM_EINVAL,
             "kzg_verify_multi_points_many: offsets of check %zu descend, or it has no evaluation point", s);
    eval_offsets[s] = eval_at;
    eval_at += (row_offsets[s + 1] - row_offsets[s]) * (point_offsets[s + 1] - point_offsets[s]);
  }
  SC_CHECK((commitments_jac || !commitment_offsets[S]) && (evaluations_mont || !eval_at), GM_EINVAL, "kzg_verify_multi_points_many: null pointer");
  CheckList checks;
  std::vector<ProofRun> runs(S);
  for (size_t s = 0; s < S; s++) {
    const size_t nc = commitment_offsets[s + 1] - commitment_offsets[s], np = point_offsets[s + 1] - point_offsets[s], nr = row_offsets[s + 1] - row_offsets[s];
    ProofRun& r = runs[s];
    r.first = checks.size();
    r.rc = verify_multi_points(*K, commitments_jac + 18 * commitment_offsets[s], nc, fr_vector(eval_points_mont + 4 * point_offsets[s], np),
                               fr_vector(evaluations_mont + 4 * eval_offsets[s], nr * np), nr, proofs_jac + 18 * s, Fr::from_limbs(open_chals_mont + 4 * s), &r.ok,
                               &checks);
    r.count = checks.size() - r.first;
    if (r.rc != GM_OK) return r.rc;  // the one check of an entry: nothing in front of it could have rejected
  }
  return settle(*K, checks, runs, ok);
}

extern "C" int gm_snark_verify_many(const uint64_t matrices[3], const uint64_t* x_vecs, uint64_t vk, int g1_encoding, const gm_snark_proof* proofs, size_t S, int* ok) {
  const VerifierKey* K;
  RC(find_vk(vk, &K));
  if (S == 0) return GM_OK;
  SC_CHECK(matrices && x_vecs && proofs && ok, GM_EINVAL, "snark_verify_many: null pointer");
  CheckList checks;
  std::vector<ProofRun> runs(S);
  for (size_t s = 0; s < S; s++) {
    ProofRun& r = runs[s];
    r.first = checks.size();
    r.rc = snark_verify_one(matrices, x_vecs[s], K, g1_encoding, &proofs[s], &r.ok, &checks);
    r.count = checks.size() - r.first;
    if (r.rc != GM_OK && r.count == 0) return r.rc;
  }
  return settle(*K, checks, runs, ok);
}

extern "C" int gm_psnark_verify_many(const uint64_t* x_vecs, size_t num_variables, size_t nnz, const uint64_t* index_commitments, uint64_t vk, int g1_encoding,
                                     const gm_psnark_proof* proofs, size_t S, int* ok) {
  const VerifierKey* K;
  RC(find_vk(vk, &K));
  if (S == 0) return GM_OK;
  SC_CHECK(x_vecs && proofs && ok, GM_EINVAL, "psnark_verify_many: null pointer");
  CheckList checks;
  std::vector<ProofRun> runs(S);
  for (size_t s = 0; s < S; s++) {
    ProofRun& r = runs[s];
    r.first = checks.size();
    r.rc = psnark_verify_one(x_vecs[s], num_variables, nnz, index_commitments, vk, K, g1_encoding, &proofs[s], &r.ok, &checks);
    r.count = checks.size() - r.first;
    if (r.rc != GM_OK && r.count == 0) return r.rc;  // before any check was stated the single entry fails in the same way
  }
  return settle(*K, checks, runs, ok);
}
