// herring's inner-product argument on the device: Crs, Vrs, InnerProductProof::new and its verifier (src/herring/ipa.rs:172-343,
// 533-685), the consumer of g2msm.hip, pairing.hip and the module provers of herring.hip.
//
// InnerProductProof::new proves <a, b> = y, <a, crs.g1> = comm_a and <b, crs.g2> = comm_b in one batched sumcheck over GT.  The three
// claims run on the existing FModule, G1Module and G2Module provers.  Every round j adds two PModule provers (the folded CRS against
// its chopped half, ipa.rs:602-608) and asks all 2 j + 2 live ones for a message; in round j all of them hold vectors of the same
// length m_j = 2^(rounds - 1 - j).  Composed from per-prover calls that is ~rounds^2 latency-bound Miller products and as many host
// final exponentiations.  Here the PModule provers of a proof are ONE arena per group:
//
//   fold      the arena of G1 (G2) vectors is one contiguous array of even-length spans, so folding ALL provers by the round's
//             challenge is one launch of the split-fold kernel the module provers use (msm.hip / g2msm.hip) -- and the fold of the
//             chopped CRS by the same challenge (ipa.rs:596) rides in that launch as one more span.  The twist is 1 throughout.
//   messages  the a and b of every live prover, the four pairings that carry the G1 / G2 messages into GT (po_from_g1 / po_from_g2)
//             and e(G1, G2) for po_from_scalarfield are the segments of ONE segmented Miller launch (pairing.hip: miller_products)
//   batching  SumcheckMsg::ip over GT is prod_k x_k^{c_k}.  FE(prod m_k^{c_k}) = prod FE(m_k)^{c_k}, so the multi-exponentiation runs
//             on the Miller values and each half of a round message costs ONE final exponentiation.  It runs on the HOST (gt_multi_pow:
//             at most 2 rounds + 1 terms of 255 bits, shared squarings, 4-bit windows); profiles/herring_ipa.md has the measurement
//             behind that choice.
//
// Launches per round: 2 folds, 1 segmented Miller kernel and its reduction levels (none while m_j / 2 <= 64, then one per factor
// 64), whatever the number of live provers.
//
// Locks: the MSM lock around every stretch that stages in C->msm.misc or uses the pairing workspace; the module provers take their own.
#include <algorithm>
#include <array>
#include <chrono>
#include <cstring>

#include "ctx.hpp"
#include "host_field.hpp"

namespace gm {

namespace {

typedef std::array<uint64_t, 4> Scalar;  // canonical

const uint64_t G1_GEN_X[6] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL, 0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL, 0x17f1d3a73197d794ULL};
const uint64_t G1_GEN_Y[6] = {0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL, 0xfcf5e095d5d00af6ULL, 0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
const uint64_t G2_GEN_X0[6] = {0xd48056c8c121bdb8ULL, 0x0bac0326a805bbefULL, 0xb4510b647ae3d177ULL, 0xc6e47ad4fa403b02ULL, 0x260805272dc51051ULL, 0x024aa2b2f08f0a91ULL};
const uint64_t G2_GEN_X1[6] = {0xe5ac7d055d042b7eULL, 0x334cf11213945d57ULL, 0xb5da61bbdc7f5049ULL, 0x596bd0d09920b61aULL, 0x7dacd3a088274f65ULL, 0x13e02b6052719f60ULL};
const uint64_t G2_GEN_Y0[6] = {0xe193548608b82801ULL, 0x923ac9cc3baca289ULL, 0x6d429a695160d12cULL, 0xadfd9baa8cbdd3a7ULL, 0x8cc9cdc6da2e351aULL, 0x0ce5d527727d6e11ULL};
const uint64_t G2_GEN_Y1[6] = {0xaaa9075ff05f79beULL, 0x3f370d275cec1da1ULL, 0x267492ab572e99abULL, 0xcb3e287e85a763afULL, 0x32acd2b02bc28b99ULL, 0x0606c4a02ea734ccULL};

gmh::G1 g1_generator() { return gmh::G1{gmh::Fq::from_canonical(G1_GEN_X), gmh::Fq::from_canonical(G1_GEN_Y), gmh::Fq::one()}; }
gmh::G2 g2_generator() {
  return gmh::G2{gmh::Fq2{gmh::Fq::from_canonical(G2_GEN_X0), gmh::Fq::from_canonical(G2_GEN_X1)},
                 gmh::Fq2{gmh::Fq::from_canonical(G2_GEN_Y0), gmh::Fq::from_canonical(G2_GEN_Y1)}, gmh::Fq2::one()};
}

// Jacobian (ark-ff form) -> the packed affine record of the device (the all-zero record is the identity)
void g1_to_record(const gmh::G1& p, uint64_t out[12]) {
  memset(out, 0, 96);
  if (p.is_identity()) return;
  const gmh::G1 a = p.normalized();
  gmh::fq_to_device(a.x, out);
  gmh::fq_to_device(a.y, out + 6);
}
void g2_to_record(const gmh::G2& p, uint64_t out[24]) {
  memset(out, 0, 192);
  if (p.is_identity()) return;
  const gmh::G2 a = p.normalized();
  gmh::fq_to_device(a.x.c0, out);
  gmh::fq_to_device(a.x.c1, out + 6);
  gmh::fq_to_device(a.y.c0, out + 12);
  gmh::fq_to_device(a.y.c1, out + 18);
}

Scalar canonical(const gmh::Fr& x) {
  Scalar s;
  x.to_canonical(s.data());
  return s;
}

// prod_k x[k]^e[k] over Fq12 (GtModule::ip / SumcheckMsg::ip on Miller values): 4-bit windows, the squarings shared by all terms
gmh::Fq12 gt_multi_pow(const std::vector<gmh::Fq12>& x, const std::vector<Scalar>& e) {
  const size_t K = x.size();
  std::vector<gmh::Fq12> tab(K * 15, gmh::Fq12::one());  // tab[15 k + d - 1] = x[k]^d
  for (size_t k = 0; k < K; k++) {
    tab[15 * k] = x[k];
    for (int d = 2; d <= 15; d++) tab[15 * k + d - 1] = tab[15 * k + d - 2] * x[k];
  }
  gmh::Fq12 acc = gmh::Fq12::one();
  bool started = false;
  for (int w = 63; w >= 0; w--) {
    if (started)
      for (int i = 0; i < 4; i++) acc = acc.sqr();
    for (size_t k = 0; k < K; k++) {
      const unsigned d = (unsigned)(e[k][w / 16] >> (4 * (w % 16))) & 15u;
      if (d) {
        acc = started ? acc * tab[15 * k + d - 1] : tab[15 * k + d - 1];
        started = true;
      }
    }
  }
  return acc;
}

// Miller value -> GT as pairing_finish does it, kept as an element
gmh::Fq12 gt_finish(const gmh::Fq12& miller) { return gmh::gt_final_exponentiation(miller.conj()); }

gmh::Fq12 gt_pow(const gmh::Fq12& x, const gmh::Fr& s) {
  const Scalar c = canonical(s);
  return x.pow(c.data(), 4);
}

PairSpan span(const uint8_t* g1, size_t first1, size_t step1, const uint8_t* g2, size_t first2, size_t step2, size_t n) {
  PairSpan s;
  s.g1 = g1;
  s.g2 = g2;
  s.first1 = (int64_t)first1;
  s.step1 = (int64_t)step1;
  s.first2 = (int64_t)first2;
  s.step2 = (int64_t)step2;
  s.n = n;
  return s;
}

// device memory of one call, given back when it ends
struct Scratch {
  std::vector<void*> p;
  ~Scratch() {
    for (void* q : p) (void)raw_free(q);
  }
  int get(size_t bytes, uint8_t** out) {
    void* q = nullptr;
    GM_HIP(dev_malloc(&q, bytes));
    p.push_back(q);
    *out = (uint8_t*)q;
    return GM_OK;
  }
};

}  // namespace

void crs_destroy(Crs* c) {
  if (c->g1) (void)raw_free(c->g1);
  if (c->g2) (void)raw_free(c->g2);
  c->g1 = c->g2 = nullptr;
}

int crs_create(Context* C, const void* g1, size_t stride1, size_t n1, const void* g2, size_t stride2, size_t n2, uint64_t* handle) {
  std::unique_ptr<Bases> b1;
  std::unique_ptr<G2Bases> b2;
  int rc = bases_from_host(C, g1, stride1, n1, b1);
  if (!rc) rc = g2_bases_from_host(C, g2, stride2, n2, b2);
  if (rc) {
    if (b1 && b1->d) (void)raw_free(b1->d);
    if (b2 && b2->d) (void)raw_free(b2->d);
    return rc;
  }
  auto c = std::make_unique<Crs>();
  c->g1 = b1->d;
  c->n1 = n1;
  c->g2 = b2->d;
  c->n2 = n2;
  std::lock_guard<std::mutex> lk(C->mu);
  *handle = C->next_handle++;
  C->crs[*handle] = std::move(c);
  return GM_OK;
}

// Crs::commit_g1 / commit_g2 (ipa.rs:179-189): the MSM over the first n points; the reference asserts len > n
int crs_commit(Context* C, const Crs* crs, int group, const uint64_t* scalars_mont, size_t n, uint64_t* out_jac) {
  GM_CHECK((group == 1 ? crs->n1 : crs->n2) > n, GM_EINVAL, "crs_commit_g%d: %zu scalars need a CRS of more than %zu points (ipa.rs:180,186), it has %zu", group, n, n,
           group == 1 ? crs->n1 : crs->n2);
  GM_MSM_LOCK(C);  // across the upload and the MSM, as the other host-scalar entry points
  int rc;
  if ((rc = C->msm.scalars.ensure(n * 32 + 32))) return rc;
  if (n) GM_HIP(hipMemcpyAsync(C->msm.scalars.p, scalars_mont, n * 32, hipMemcpyHostToDevice, C->stream));
  if (group == 1) {
    Bases b;
    b.d = crs->g1;
    b.n = crs->n1;
    return msm_run(C, &b, 0, 1, C->msm.scalars.p, 1, n, true, out_jac);
  }
  G2Bases b;
  b.d = crs->g2;
  b.n = crs->n2;
  return g2_msm_run(C, &b, 0, 1, C->msm.scalars.p, 1, n, out_jac);
}

// Crs::fold (ipa.rs:205-212): g[i] = g[2i] + c g[2i+1] in both groups, one launch of the module provers' split-fold kernel each (an
// odd tail folds against the identity); the caller has checked n1 == n2.  `out` owns two new arrays of ceil(n / 2) points.
int crs_fold(Context* C, const Crs* in, const uint64_t challenge_mont[4], Crs* out) {
  const size_t m1 = (in->n1 + 1) / 2, m2 = (in->n2 + 1) / 2;
  const Scalar c = canonical(gmh::Fr::from_limbs(challenge_mont));
  GM_MSM_LOCK(C);
  int rc;
  if ((rc = C->msm.misc.ensure(64))) return rc;
  Scratch tmp;
  uint8_t *d1 = nullptr, *d2 = nullptr;
  if ((rc = tmp.get(m1 * 96, &d1)) || (rc = tmp.get(m2 * 192, &d2))) return rc;
  GM_HIP(hipMemcpyAsync(C->msm.misc.p, c.data(), 32, hipMemcpyHostToDevice, C->stream));
  if ((rc = g1_split_fold_launch(C, in->g1, in->n1, C->msm.misc.as<uint32_t>(), d1))) return rc;
  if ((rc = g2_split_fold_launch(C, in->g2, in->n2, C->msm.misc.as<uint32_t>(), d2))) return rc;
  GM_HIP(hipStreamSynchronize(C->stream));  // `c` is read by its copy until here
  tmp.p.clear();  // the arrays are the result's from here
  out->g1 = d1;
  out->n1 = m1;
  out->g2 = d2;
  out->n2 = m2;
  return GM_OK;
}

// Vrs::from (ipa.rs:215-247): for size = 2, 4, ... below the CRS length the four products of the even / odd points of one group
// against the first `size` of the other -- all 4 levels products in ONE segmented launch, then one final exponentiation each
int vrs_from_crs(Context* C, const Crs* crs, Vrs* out) {
  const size_t top = (size_t)msm_ceil_log2(crs->n1);  // ark_std::log2 rounds up
  out->levels = top >= 1 ? top - 1 : 0;
  std::vector<PairProduct> prods;
  for (size_t j = 1; j < top; j++) {
    const size_t size = (size_t)1 << j;
    const size_t e1 = (crs->n1 + 1) / 2, o1 = crs->n1 / 2, e2 = (crs->n2 + 1) / 2, o2 = crs->n2 / 2;  // step_by(2) and skip(1).step_by(2)
    PairProduct p[4];
    p[0].s0 = span(crs->g1, 0, 2, crs->g2, 0, 1, std::min({size, e1, crs->n2}));
    p[1].s0 = span(crs->g1, 1, 2, crs->g2, 0, 1, std::min({size, o1, crs->n2}));
    p[2].s0 = span(crs->g1, 0, 1, crs->g2, 0, 2, std::min({size, crs->n1, e2}));
    p[3].s0 = span(crs->g1, 0, 1, crs->g2, 1, 2, std::min({size, crs->n1, o2}));
    prods.insert(prods.end(), p, p + 4);
  }
  // the 4 levels Miller values stay on the device and go through ONE k_gt_final_exp launch (profiles/gt_device.md)
  std::vector<uint64_t> gt(prods.size() * 72);
  {
    GM_MSM_LOCK(C);
    int rc = pairing_products(C, prods.data(), prods.size(), gt.data());
    if (rc) return rc;
  }
  out->vk1.resize(out->levels * 144);
  out->vk2.resize(out->levels * 144);
  for (size_t l = 0; l < out->levels; l++) {
    memcpy(out->vk1.data() + 144 * l, gt.data() + 72 * (4 * l), 144 * sizeof(uint64_t));      // even || odd
    memcpy(out->vk2.data() + 144 * l, gt.data() + 72 * (4 * l + 2), 144 * sizeof(uint64_t));
  }
  return GM_OK;
}

namespace {

// The three initial provers of InnerProductProof::new, freed with the call
struct InitialProvers {
  Context* C;
  uint64_t ff = 0, fg1 = 0, fg2 = 0;
  HerringProver *h1 = nullptr, *h2 = nullptr;
  ~InitialProvers() {
    if (ff) (void)gm_sc_free(ff);
    if (fg1) (void)gm_hg1_free(fg1);
    if (fg2) (void)gm_hg2_free(fg2);
  }
};

// The PModule provers of one proof.  Prover p (in the order ipa.rs pushes them: g1fold and g2fold of round 0, of round 1, ...) keeps
// its Lhs vector in slot p of the G1 arena and its Rhs vector in slot p ^ 1 of the G2 arena: the fold of the chopped CRS lands in
// slot `live` of BOTH arenas, and it is the Lhs of the g1fold prover but the Rhs of the g2fold prover.
struct Arena {
  uint8_t *g1[2] = {nullptr, nullptr}, *g2[2] = {nullptr, nullptr};
  int cur = 0;
  size_t live = 0;  // provers
  size_t m = 0;     // length of every live vector
};

// Step 2b of a round and the fold of every live prover by `challenge` in one launch per group: the arenas hold `live` vectors of
// 2 m points, the first 2 m points of the CRS are appended, everything folds to length m, and the unfolded first m points of the
// CRS become the other side of the two new provers.  with_crs = false: the last fold (no new provers).
int arena_round(Context* C, const Crs* crs, Arena& A, const gmh::Fr& challenge, bool with_crs) {
  const size_t m = A.m / 2, spans = A.live + (with_crs ? 1 : 0);
  const int in = A.cur, outb = A.cur ^ 1;
  const Scalar c = canonical(challenge);
  int rc;
  if ((rc = C->msm.misc.ensure(64))) return rc;
  GM_HIP(hipMemcpyAsync(C->msm.misc.p, c.data(), 32, hipMemcpyHostToDevice, C->stream));
  if (with_crs) {
    GM_HIP(hipMemcpyAsync(A.g1[in] + A.live * A.m * 96, crs->g1, A.m * 96, hipMemcpyDeviceToDevice, C->stream));
    GM_HIP(hipMemcpyAsync(A.g2[in] + A.live * A.m * 192, crs->g2, A.m * 192, hipMemcpyDeviceToDevice, C->stream));
  }
  if ((rc = g1_split_fold_launch(C, A.g1[in], spans * A.m, C->msm.misc.as<uint32_t>(), A.g1[outb]))) return rc;
  if ((rc = g2_split_fold_launch(C, A.g2[in], spans * A.m, C->msm.misc.as<uint32_t>(), A.g2[outb]))) return rc;
  if (with_crs) {
    GM_HIP(hipMemcpyAsync(A.g1[outb] + (A.live + 1) * m * 96, crs->g1, m * 96, hipMemcpyDeviceToDevice, C->stream));
    GM_HIP(hipMemcpyAsync(A.g2[outb] + (A.live + 1) * m * 192, crs->g2, m * 192, hipMemcpyDeviceToDevice, C->stream));
    A.live += 2;
  }
  GM_HIP(hipStreamSynchronize(C->stream));  // `c` is read by its copy until here
  A.cur = outb;
  A.m = m;
  return GM_OK;
}

}  // namespace

// InnerProductProof::new (ipa.rs:533-685)
int ipa_prove(Context* C, uint64_t transcript, const Crs* crs, const uint64_t* a_mont, const uint64_t* b_mont, size_t d, IpaProof* proof) {
  GM_CHECK(d >= 2, GM_EINVAL, "ipa_new: d = %zu; the argument needs at least two scalars (the reference's round loop underflows at rounds - 1, ipa.rs:584)", d);
  const size_t rounds = (size_t)msm_ceil_log2(d), full = (size_t)1 << rounds;
  const size_t need = std::max(d + 1, full);
  GM_CHECK(crs->n1 >= need && crs->n2 >= need, GM_EINVAL, "ipa_new: d = %zu needs a CRS of max(d + 1, 2^rounds) = %zu points, it has %zu / %zu", d, need, crs->n1, crs->n2);
  uint64_t one[4];
  gmh::Fr::one().to_limbs(one);
  typedef std::chrono::steady_clock Clock;
  auto ms_since = [](Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); };
  const Clock::time_point t_start = Clock::now();
  proof->host_ms[0] = proof->host_ms[1] = proof->host_ms[2] = 0;

  // the three claims.  The G1 / G2 provers get the first 2^rounds points: their messages zip against d scalars and their final
  // folding is a combination of exactly those points, so the rest of a longer CRS never enters (and need not be folded)
  InitialProvers P{C};
  int rc;
  if ((rc = gm_sc_new(a_mont, d, b_mont, d, one, &P.ff)) || (rc = gm_sc_set_herring(P.ff, 1))) return rc;
  if ((rc = herring_create(C, HERRING_G1, crs->g1, 96, full, a_mont, 32, d, one, &P.fg1, 1))) return rc;
  if ((rc = herring_create(C, HERRING_G2, b_mont, 32, d, crs->g2, 192, full, one, &P.fg2, 2))) return rc;
  {
    std::lock_guard<std::mutex> lk(C->mu);
    P.h1 = C->herring[P.fg1].get();
    P.h2 = C->herring[P.fg2].get();
  }

  Scratch mem;
  Arena A;
  uint8_t *aux1 = nullptr, *aux2 = nullptr;  // G1: message a, message b, generator; G2: generator, message a, message b
  if ((rc = mem.get(3 * 96, &aux1)) || (rc = mem.get(3 * 192, &aux2))) return rc;
  if (rounds > 1) {
    for (int i = 0; i < 2; i++)
      if ((rc = mem.get(2 * full * 96, &A.g1[i])) || (rc = mem.get(2 * full * 192, &A.g2[i]))) return rc;
  }
  A.m = full;
  uint64_t rec1[36], rec2[72];
  g1_to_record(g1_generator(), rec1 + 24);
  g2_to_record(g2_generator(), rec2);

  proof->rounds = rounds;
  proof->messages.assign(rounds * 144, 0);
  proof->challenges.assign(rounds * 4, 0);
  proof->batch_challenges.clear();
  std::vector<gmh::Fr> bch;  // batch_challenges
  auto push_bch = [&](const gmh::Fr& x) {
    bch.push_back(x);
    uint64_t l[4];
    x.to_limbs(l);
    proof->batch_challenges.insert(proof->batch_challenges.end(), l, l + 4);
  };

  // One message of the batched sumcheck: the three initial provers step (folding by `vm` first when there is one), then every
  // PModule prover's products and the carriers of the first three in one segmented launch, then the two GT multi-exponentiations
  auto round_message = [&](const uint64_t* vm, uint64_t* out144) -> int {
    uint64_t fa[4], fb[4], g1a[18], g1b[18], g2a[36], g2b[36];
    int has = 0, r;
    if ((r = gm_sc_round(P.ff, vm, fa, fb, &has))) return r;
    GM_CHECK(has, GM_ESTATE, "ipa_new: the FModule prover has no message");
    if ((r = herring_round(C, P.h1, vm, g1a, g1b, &has))) return r;
    GM_CHECK(has, GM_ESTATE, "ipa_new: the G1Module prover has no message");
    if ((r = herring_round(C, P.h2, vm, g2a, g2b, &has))) return r;
    GM_CHECK(has, GM_ESTATE, "ipa_new: the G2Module prover has no message");
    g1_to_record(gmh::G1::from_limbs(g1a), rec1);
    g1_to_record(gmh::G1::from_limbs(g1b), rec1 + 12);
    g2_to_record(gmh::G2::from_limbs(g2a), rec2 + 24);
    g2_to_record(gmh::G2::from_limbs(g2b), rec2 + 48);
    // segments: e(G1, G2); (fg1.a, G2), (fg1.b, G2), (G1, fg2.a), (G1, fg2.b); then a_p, b_p of every PModule prover
    std::vector<PairProduct> prods(5 + 2 * A.live);
    prods[0].s0 = span(aux1, 2, 1, aux2, 0, 1, 1);
    prods[1].s0 = span(aux1, 0, 1, aux2, 0, 1, 1);
    prods[2].s0 = span(aux1, 1, 1, aux2, 0, 1, 1);
    prods[3].s0 = span(aux1, 2, 1, aux2, 1, 1, 1);
    prods[4].s0 = span(aux1, 2, 1, aux2, 2, 1, 1);
    const size_t h = A.m / 2;
    for (size_t p = 0; p < A.live; p++) {
      const uint8_t *f = A.g1[A.cur], *g = A.g2[A.cur];
      const size_t f0 = p * A.m, g0 = (p ^ 1) * A.m;
      prods[5 + 2 * p].s0 = span(f, f0, 2, g, g0, 2, h);          // a = ip(f_even, g_even)
      prods[5 + 2 * p + 1].s0 = span(f, f0, 2, g, g0 + 1, 2, h);  // b = ip(f_even, g_odd) + ip(f_odd, g_even)
      prods[5 + 2 * p + 1].s1 = span(f, f0 + 1, 2, g, g0, 2, h);
    }
    std::vector<gmh::Fq12> m(prods.size());
    {
      GM_MSM_LOCK(C);
      GM_HIP(hipMemcpyAsync(aux1, rec1, sizeof rec1, hipMemcpyHostToDevice, C->stream));
      GM_HIP(hipMemcpyAsync(aux2, rec2, sizeof rec2, hipMemcpyHostToDevice, C->stream));
      if ((r = miller_products(C, prods.data(), prods.size(), m.data()))) return r;
    }
    // SumcheckMsg::ip(messages, batch_challenges) (ipa.rs:636-644): E^(ff bch_0), the G1 and G2 messages by bch_1, bch_2, prover p by bch_{3 + p}
    for (int half = 0; half < 2; half++) {
      std::vector<gmh::Fq12> x;
      std::vector<Scalar> e;
      x.push_back(m[0]);
      e.push_back(canonical(gmh::Fr::from_limbs(half ? fb : fa) * bch[0]));
      x.push_back(m[1 + half]);
      e.push_back(canonical(bch[1]));
      x.push_back(m[3 + half]);
      e.push_back(canonical(bch[2]));
      for (size_t p = 0; p < A.live; p++) {
        x.push_back(m[5 + 2 * p + half]);
        e.push_back(canonical(bch[3 + p]));
      }
      Clock::time_point t0 = Clock::now();
      const gmh::Fq12 prod = gt_multi_pow(x, e);
      proof->host_ms[0] += ms_since(t0);
      t0 = Clock::now();
      gt_finish(prod).to_limbs(out144 + 72 * half);
      proof->host_ms[1] += ms_since(t0);
    }
    return GM_OK;
  };

  uint64_t ch[4];
  if ((rc = gm_transcript_challenge_fr(transcript, (const uint8_t*)"batch-chal", 10, ch))) return rc;
  const gmh::Fr bc = gmh::Fr::from_limbs(ch);
  push_bch(gmh::Fr::one());
  push_bch(bc);
  push_bch(bc.sqr());
  if ((rc = round_message(nullptr, proof->messages.data()))) return rc;
  if ((rc = gm_transcript_append_gt(transcript, (const uint8_t*)"prover_message", 14, proof->messages.data(), 2))) return rc;

  for (size_t j = 0; j + 1 < rounds; j++) {
    uint64_t* c = proof->challenges.data() + 4 * j;
    if ((rc = gm_transcript_challenge_fr(transcript, (const uint8_t*)"sumcheck-chal", 13, c))) return rc;
    if ((rc = gm_transcript_challenge_fr(transcript, (const uint8_t*)"batch-chal", 10, ch))) return rc;
    const gmh::Fr b = gmh::Fr::from_limbs(ch);
    push_bch(b);
    push_bch(b.sqr());
    {
      GM_MSM_LOCK(C);
      if ((rc = arena_round(C, crs, A, gmh::Fr::from_limbs(c), true))) return rc;
    }
    uint64_t* msg = proof->messages.data() + 144 * (j + 1);
    if ((rc = round_message(c, msg))) return rc;
    if ((rc = gm_transcript_append_gt(transcript, (const uint8_t*)"sumcheck-round", 14, msg, 2))) return rc;
  }

  uint64_t* last = proof->challenges.data() + 4 * (rounds - 1);
  if ((rc = gm_transcript_challenge_fr(transcript, (const uint8_t*)"sumcheck-chal", 13, last))) return rc;
  // final foldings: every PModule prover folds once more to length 1 (ipa.rs:655-661)
  const size_t k = A.live;
  proof->final_g1.assign(k * 18, 0);
  proof->final_g2.assign(k * 36, 0);
  if (k) {
    std::vector<uint64_t> f(k * 12), g(k * 24);
    {
      GM_MSM_LOCK(C);
      if ((rc = arena_round(C, crs, A, gmh::Fr::from_limbs(last), false))) return rc;
      GM_HIP(hipMemcpyAsync(f.data(), A.g1[A.cur], k * 96, hipMemcpyDeviceToHost, C->stream));
      GM_HIP(hipMemcpyAsync(g.data(), A.g2[A.cur], k * 192, hipMemcpyDeviceToHost, C->stream));
      GM_HIP(hipStreamSynchronize(C->stream));
    }
    for (size_t p = 0; p < k; p++) {
      gmh::g1_affine_to_jac_dev(f.data() + 12 * p).to_limbs(proof->final_g1.data() + 18 * p);
      gmh::g2_affine_to_jac_dev(g.data() + 24 * (p ^ 1)).to_limbs(proof->final_g2.data() + 36 * p);
    }
  }
  int has = 0;
  if ((rc = gm_sc_fold(P.ff, last)) || (rc = herring_fold(C, P.h1, last)) || (rc = herring_fold(C, P.h2, last))) return rc;
  if ((rc = gm_sc_final(P.ff, proof->foldings_ff, proof->foldings_ff + 4, &has))) return rc;
  GM_CHECK(has, GM_ESTATE, "ipa_new: the FModule prover has no final foldings");
  if ((rc = herring_final(C, P.h1, proof->foldings_fg1, proof->foldings_fg1 + 18, &has))) return rc;
  GM_CHECK(has, GM_ESTATE, "ipa_new: the G1Module prover has no final foldings");
  if ((rc = herring_final(C, P.h2, proof->foldings_fg2, proof->foldings_fg2 + 4, &has))) return rc;
  GM_CHECK(has, GM_ESTATE, "ipa_new: the G2Module prover has no final foldings");
  proof->host_ms[2] = ms_since(t_start);
  return GM_OK;
}

// InnerProductProof::verify_transcript (ipa.rs:250-343), GT written multiplicatively.  Its pairings -- the two commitments, the
// foldings of the three claims and every PModule final folding -- are the 1-pair segments of ONE segmented launch; the claim and the
// expected value take one final exponentiation each.
int ipa_verify(Context* C, const IpaProof* pr, const Vrs* vrs, const uint64_t comm_a[18], const uint64_t comm_b[36], const uint64_t y_mont[4], int* ok) {
  const size_t R = pr->rounds, k = R >= 1 ? 2 * (R - 1) : 0;
  GM_CHECK(R >= 1 && pr->messages.size() == R * 144 && pr->challenges.size() == R * 4 && pr->batch_challenges.size() == (3 + k) * 4 && pr->final_g1.size() == k * 18 &&
               pr->final_g2.size() == k * 36,
           GM_EINVAL, "ipa_verify: the proof's fields do not have the lengths of %zu rounds", R);
  GM_CHECK(vrs->levels + 1 >= R, GM_EINVAL, "ipa_verify: a proof of %zu rounds needs %zu levels of the Vrs, it has %zu", R, R - 1, vrs->levels);
  auto fr = [](const uint64_t* p) { return gmh::Fr::from_limbs(p); };
  std::vector<gmh::Fr> bch(3 + k), ch(R);
  for (size_t i = 0; i < 3 + k; i++) bch[i] = fr(pr->batch_challenges.data() + 4 * i);
  for (size_t i = 0; i < R; i++) ch[i] = fr(pr->challenges.data() + 4 * i);

  // records: G1 = generator, comm_a, fg1's f0, the Lhs final foldings; G2 = generator, comm_b, fg2's g0, the Rhs final foldings
  std::vector<uint64_t> r1((3 + k) * 12), r2((3 + k) * 24);
  g1_to_record(g1_generator(), r1.data());
  g1_to_record(gmh::G1::from_limbs(comm_a), r1.data() + 12);
  g1_to_record(gmh::G1::from_limbs(pr->foldings_fg1), r1.data() + 24);
  g2_to_record(g2_generator(), r2.data());
  g2_to_record(gmh::G2::from_limbs(comm_b), r2.data() + 24);
  g2_to_record(gmh::G2::from_limbs(pr->foldings_fg2 + 4), r2.data() + 48);
  for (size_t p = 0; p < k; p++) {
    g1_to_record(gmh::G1::from_limbs(pr->final_g1.data() + 18 * p), r1.data() + 12 * (3 + p));
    g2_to_record(gmh::G2::from_limbs(pr->final_g2.data() + 36 * p), r2.data() + 24 * (3 + p));
  }
  Scratch mem;
  uint8_t *d1 = nullptr, *d2 = nullptr;
  int rc;
  if ((rc = mem.get(r1.size() * 8, &d1)) || (rc = mem.get(r2.size() * 8, &d2))) return rc;
  // e(G1, G2); e(comm_a, G2), e(G1, comm_b); e(fg1.f0, G2), e(G1, fg2.g0); e(lhs_p, rhs_p)
  std::vector<PairProduct> prods(5 + k);
  prods[0].s0 = span(d1, 0, 1, d2, 0, 1, 1);
  prods[1].s0 = span(d1, 1, 1, d2, 0, 1, 1);
  prods[2].s0 = span(d1, 0, 1, d2, 1, 1, 1);
  prods[3].s0 = span(d1, 2, 1, d2, 0, 1, 1);
  prods[4].s0 = span(d1, 0, 1, d2, 2, 1, 1);
  for (size_t p = 0; p < k; p++) prods[5 + p].s0 = span(d1, 3 + p, 1, d2, 3 + p, 1, 1);
  std::vector<gmh::Fq12> m(prods.size());
  {
    GM_MSM_LOCK(C);
    GM_HIP(hipMemcpyAsync(d1, r1.data(), r1.size() * 8, hipMemcpyHostToDevice, C->stream));
    GM_HIP(hipMemcpyAsync(d2, r2.data(), r2.size() * 8, hipMemcpyHostToDevice, C->stream));
    if ((rc = miller_products(C, prods.data(), prods.size(), m.data()))) return rc;
  }
  // reduced_claim = ip([E^y, e(comm_a, G2), e(G1, comm_b)], batch_challenges[..3])   (:284-290)
  gmh::Fq12 claim = gt_finish(gt_multi_pow({m[0], m[1], m[2]}, {canonical(fr(y_mont) * bch[0]), canonical(bch[1]), canonical(bch[2])}));
  auto step = [&](size_t i) {  // a + b challenge + (claim - a) challenge^2   (:302-303, :311-312)
    const gmh::Fq12 a = gmh::Fq12::from_limbs(pr->messages.data() + 144 * i), b = gmh::Fq12::from_limbs(pr->messages.data() + 144 * i + 72);
    const gmh::Fq12 c = claim * a.inv();
    return a * gt_pow(b, ch[i]) * gt_pow(c, ch[i].sqr());
  };
  for (size_t i = 0; i + 1 < R; i++) {
    // the folded verifier key of round i: level R - 2 - i with challenge i (:257-282: the challenges reversed without the last
    // one against the levels, then both lists reversed)
    const uint64_t* l1 = vrs->vk1.data() + 144 * (R - 2 - i);
    const uint64_t* l2 = vrs->vk2.data() + 144 * (R - 2 - i);
    const gmh::Fq12 g1c = gmh::Fq12::from_limbs(l1) * gt_pow(gmh::Fq12::from_limbs(l1 + 72), ch[i]);
    const gmh::Fq12 g2c = gmh::Fq12::from_limbs(l2) * gt_pow(gmh::Fq12::from_limbs(l2 + 72), ch[i]);
    claim = step(i) * gt_pow(g1c, bch[3 + 2 * i]) * gt_pow(g2c, bch[3 + 2 * i + 1]);
  }
  claim = step(R - 1);
  // expected = ip(final_foldings, batch_challenges)   (:314-336); p(f0, g0) of the three claims moves g0 / f0 into the exponent
  std::vector<gmh::Fq12> x = {m[0], m[3], m[4]};
  std::vector<Scalar> e = {canonical(fr(pr->foldings_ff) * fr(pr->foldings_ff + 4) * bch[0]), canonical(fr(pr->foldings_fg1 + 18) * bch[1]),
                           canonical(fr(pr->foldings_fg2) * bch[2])};
  for (size_t p = 0; p < k; p++) {
    x.push_back(m[5 + p]);
    e.push_back(canonical(bch[3 + p]));
  }
  *ok = claim == gt_finish(gt_multi_pow(x, e)) ? 1 : 0;
  return GM_OK;
}

// ---- many proofs in one call ----------------------------------------------------------------------------------------------------
// verify_transcript is linear in the claim: every round maps claim -> a^(1 - ch^2) b^ch claim^(ch^2) times the folded verifier key.
// Unrolled over the R rounds, with w[i] = prod_{j > i} ch[j]^2 and W = w[0] ch[0]^2, "claim == expected" is ONE product in GT,
//
//   prod_j x_j^(e_j) * FE(conj(prod_t Miller(P_t, Q_t))) == 1
//
// over GT elements the verifier is handed (the proof's messages, the Vrs entries) with exponents the host computes from the
// challenges, and pairs whose exponent has moved onto the G1 side.  The terms, in the order ipa_state lists them (R rounds):
//
//   GT, 6 R - 4      a_i^((1 - ch_i^2) w_i), b_i^(ch_i w_i) for every round i; then for every round i < R - 1, level l = R - 2 - i:
//                    vk1_even[l]^(bch[3+2i] w_i), vk1_odd[l]^(bch[3+2i] w_i ch_i), vk2_even[l]^(bch[4+2i] w_i), vk2_odd[l]^(bch[4+2i] w_i ch_i)
//   pairs, 2 R + 4   e(G1, G2)^(y bch0 W), e(comm_a, G2)^(bch1 W), e(G1, comm_b)^(bch2 W); then the expected side, negated:
//                    e(G1, G2)^(-ff.lhs ff.rhs bch0), e(fg1.f0, G2)^(-fg1.g0 bch1), e(G1, fg2.g0)^(-fg2.f0 bch2), e(lhs_p, rhs_p)^(-bch[3+p])
//
// tests/ipa_flat_ref.py states the same on Python integers.  The unrolling holds for MEMBERS only (exponents are taken mod r, and
// e(s P, Q) = e(P, Q)^s needs P in G1 and Q in G2), so ipa_verify_many first runs the membership tests over every element a proof or the
// caller supplies and gives every proof that fails one to ipa_verify above: its answer is ipa_verify's for every input.
namespace {

void ipa_state(const IpaProof* pr, const uint64_t y_mont[4], std::vector<gmh::Fr>& gt, std::vector<gmh::Fr>& pair) {
  const size_t R = pr->rounds, k = 2 * (R - 1);
  auto fr = [](const uint64_t* p) { return gmh::Fr::from_limbs(p); };
  std::vector<gmh::Fr> bch(3 + k), ch(R), w(R);
  for (size_t i = 0; i < 3 + k; i++) bch[i] = fr(pr->batch_challenges.data() + 4 * i);
  for (size_t i = 0; i < R; i++) ch[i] = fr(pr->challenges.data() + 4 * i);
  w[R - 1] = gmh::Fr::one();
  for (size_t i = R - 1; i > 0; i--) w[i - 1] = w[i] * ch[i].sqr();
  const gmh::Fr W = w[0] * ch[0].sqr();
  gt.clear();
  pair.clear();
  for (size_t i = 0; i < R; i++) {
    gt.push_back((gmh::Fr::one() - ch[i].sqr()) * w[i]);
    gt.push_back(ch[i] * w[i]);
  }
  for (size_t i = 0; i + 1 < R; i++)
    for (size_t v = 0; v < 2; v++) {
      const gmh::Fr e = bch[3 + 2 * i + v] * w[i];
      gt.push_back(e);
      gt.push_back(e * ch[i]);
    }
  pair.push_back(fr(y_mont) * bch[0] * W);
  pair.push_back(bch[1] * W);
  pair.push_back(bch[2] * W);
  pair.push_back((fr(pr->foldings_ff) * fr(pr->foldings_ff + 4) * bch[0]).neg());
  pair.push_back((fr(pr->foldings_fg1 + 18) * bch[1]).neg());
  pair.push_back((fr(pr->foldings_fg2) * bch[2]).neg());
  for (size_t p = 0; p < k; p++) pair.push_back(bch[3 + p].neg());
}

// the lengths ipa_verify asks of a proof and of the Vrs, with its codes
int ipa_shape(const IpaProof* pr, const Vrs* vrs, const char* who) {
  const size_t R = pr->rounds, k = R >= 1 ? 2 * (R - 1) : 0;
  GM_CHECK(R >= 1 && pr->messages.size() == R * 144 && pr->challenges.size() == R * 4 && pr->batch_challenges.size() == (3 + k) * 4 && pr->final_g1.size() == k * 18 &&
               pr->final_g2.size() == k * 36,
           GM_EINVAL, "%s: the proof's fields do not have the lengths of %zu rounds", who, R);
  GM_CHECK(!vrs || vrs->levels + 1 >= R, GM_EINVAL, "%s: a proof of %zu rounds needs %zu levels of the Vrs, it has %zu", who, R, R - 1, vrs ? vrs->levels : 0);
  return GM_OK;
}

bool fr_reduced(const uint64_t* p) {
  uint64_t t[4];
  return gmh::sub_n<4>(t, p, gmh::FrP::MOD) != 0;
}
// every scalar the stated form multiplies is a reduced residue (the per-proof path takes limbs as they are)
bool ipa_scalars_reduced(const IpaProof* pr, const uint64_t y_mont[4]) {
  bool ok = fr_reduced(y_mont) && fr_reduced(pr->foldings_ff) && fr_reduced(pr->foldings_ff + 4) && fr_reduced(pr->foldings_fg1 + 18) && fr_reduced(pr->foldings_fg2);
  for (size_t i = 0; i < pr->challenges.size(); i += 4) ok = ok && fr_reduced(pr->challenges.data() + i);
  for (size_t i = 0; i < pr->batch_challenges.size(); i += 4) ok = ok && fr_reduced(pr->batch_challenges.data() + i);
  return ok;
}

// an affine host record (ark-ff's Montgomery form, the identity all zero) -> the packed record of the device
void g2_record_to_device(const uint64_t in[24], uint64_t out[24]) {
  for (int c = 0; c < 4; c++) gmh::fq_to_device(gmh::Fq::from_limbs(in + 6 * c), out + 6 * c);
}

}  // namespace

int ipa_stated_terms(const IpaProof* pr, const uint64_t y_mont[4], uint64_t* gt_exp, uint64_t* pair_exp) {
  int rc = ipa_shape(pr, nullptr, "ipa_stated_terms");
  if (rc) return rc;
  std::vector<gmh::Fr> gt, pair;
  ipa_state(pr, y_mont, gt, pair);
  for (size_t i = 0; i < gt.size(); i++) gt[i].to_canonical(gt_exp + 4 * i);
  for (size_t i = 0; i < pair.size(); i++) pair[i].to_canonical(pair_exp + 4 * i);
  return GM_OK;
}

// Launches and waits of the batched path, whatever S is: one k_pt_check per group and one k_gt_check over every element the proofs
// and the caller supply (a wait each: their verdicts decide which proofs go on), the upload of the GT table (a wait), then ONE
// launch group -- k_g1_term_mul, k_g1_seg_sum, k_normalise for every G1 point of every proof, k_miller_seg with one segment per
// proof, k_gt_final_exp over the S Miller values, k_gt_multi_pow_seg over all GT terms, the reduction levels of the longest proof --
// and its wait.  The batched kernels see members only: no element that failed a test reaches them, and none of them addresses memory
// by the value of an element (pairing.hip: k_gt_multi_pow_seg).
int ipa_verify_many(Context* C, const IpaProof* const* proofs, const Vrs* vrs, const uint64_t* comm_a, const uint64_t* comm_b, const uint64_t* y_mont, size_t S, int* ok) {
  int rc;
  for (size_t s = 0; s < S; s++)
    if ((rc = ipa_shape(proofs[s], vrs, "ipa_verify_many"))) return rc;
  for (size_t s = 0; s < S; s++) ok[s] = 0;
  GM_MSM_LOCK(C);
  C->ipa_verify_many_last[0] = C->ipa_verify_many_last[1] = 0;
  std::vector<char> clean(S, 0);
  size_t nclean = 0;
  if (S >= C->ipa_verify_many_min && S > 0) {
    // membership: G1 = comm_a, fg1.f0, the Lhs final foldings; G2 = comm_b, fg2.g0, the Rhs final foldings; GT = the messages
    std::vector<const uint64_t*> j1, j2;
    std::vector<size_t> pbase(S + 1, 0), mbase(S + 1, 0);  // first point / first message of proof s
    for (size_t s = 0; s < S; s++) {
      const IpaProof* pr = proofs[s];
      const size_t k = 2 * (pr->rounds - 1);
      j1.push_back(comm_a + 18 * s);
      j1.push_back(pr->foldings_fg1);
      j2.push_back(comm_b + 36 * s);
      j2.push_back(pr->foldings_fg2 + 4);
      for (size_t p = 0; p < k; p++) {
        j1.push_back(pr->final_g1.data() + 18 * p);
        j2.push_back(pr->final_g2.data() + 36 * p);
      }
      pbase[s + 1] = pbase[s] + 2 + k;
      mbase[s + 1] = mbase[s] + 2 * pr->rounds;
    }
    std::vector<uint64_t> r1, r2, msgs(mbase[S] * 72);
    std::vector<uint8_t> st1, st2, stg(mbase[S]);
    for (size_t s = 0; s < S; s++) memcpy(msgs.data() + 72 * mbase[s], proofs[s]->messages.data(), proofs[s]->messages.size() * 8);
    int all = 0;
    if ((rc = jac_points_status(C, j1, j2, r1, r2, st1, st2))) return rc;
    if ((rc = gt_check_host(C, msgs.data(), mbase[S], stg.data(), nullptr, &all))) return rc;
    for (size_t s = 0; s < S; s++) {
      bool good = ipa_scalars_reduced(proofs[s], y_mont + 4 * s);
      for (size_t i = pbase[s]; i < pbase[s + 1]; i++) good = good && st1[i] == GM_PT_OK && st2[i] == GM_PT_OK;
      for (size_t i = mbase[s]; i < mbase[s + 1]; i++) good = good && stg[i] == GM_PT_OK;
      clean[s] = good;
      nclean += good;
    }
    if (nclean) {
      // the tables of the clean proofs.  G1 terms (host records) and their segments: per proof [G1 y.., comm_a, G1 -ff.., fg1.f0]
      // against G2, [G1] against comm_b, [G1] against fg2.g0, [lhs_p] against rhs_p; the G2 side lists one record per segment
      uint64_t gen1[12], gen2[24];
      g1_generator().x.to_limbs(gen1);
      g1_generator().y.to_limbs(gen1 + 6);
      g2_to_record(g2_generator(), gen2);
      const size_t nv = 4 * vrs->levels;
      std::vector<uint64_t> pts, sc, q2, gtx(nv * 72), gte;
      std::vector<size_t> seg_off(1, 0), term_off(1, 0);
      std::vector<GtTerm> terms;
      std::vector<PairProduct> prods;
      std::vector<size_t> who;
      for (size_t l = 0; l < vrs->levels; l++) {  // rows 4 l ..: vk1 even, vk1 odd, vk2 even, vk2 odd
        memcpy(gtx.data() + 72 * (4 * l), vrs->vk1.data() + 144 * l, 144 * 8);
        memcpy(gtx.data() + 72 * (4 * l + 2), vrs->vk2.data() + 144 * l, 144 * 8);
      }
      std::vector<gmh::Fr> eg, ep;
      auto term1 = [&](const uint64_t* rec, const gmh::Fr& e) {
        pts.insert(pts.end(), rec, rec + 12);
        const Scalar c = canonical(e);
        sc.insert(sc.end(), c.begin(), c.end());
      };
      auto seg_end = [&](const uint64_t* rec2_dev) {
        seg_off.push_back(pts.size() / 12);
        q2.insert(q2.end(), rec2_dev, rec2_dev + 24);
      };
      for (size_t s = 0; s < S; s++) {
        if (!clean[s]) continue;
        const IpaProof* pr = proofs[s];
        const size_t R = pr->rounds, k = 2 * (R - 1);
        ipa_state(pr, y_mont + 4 * s, eg, ep);
        const uint64_t *a1 = r1.data() + 12 * pbase[s], *a2 = r2.data() + 24 * pbase[s];
        uint64_t rec2[24];
        const size_t seg0 = seg_off.size() - 1;
        term1(gen1, ep[0]);
        term1(a1, ep[1]);
        term1(gen1, ep[3]);
        term1(a1 + 12, ep[4]);
        seg_end(gen2);
        term1(gen1, ep[2]);
        g2_record_to_device(a2, rec2);
        seg_end(rec2);
        term1(gen1, ep[5]);
        g2_record_to_device(a2 + 24, rec2);
        seg_end(rec2);
        for (size_t p = 0; p < k; p++) {
          term1(a1 + 12 * (2 + p), ep[6 + p]);
          g2_record_to_device(a2 + 24 * (2 + p), rec2);
          seg_end(rec2);
        }
        PairProduct pp;
        pp.s0 = span(nullptr, seg0, 1, nullptr, seg0, 1, 3 + k);  // the two arrays are known once they are on the device
        prods.push_back(pp);
        // GT terms: the messages of this proof follow the Vrs rows
        const size_t m0 = gtx.size() / 72, e0 = gte.size() / 4;
        gtx.insert(gtx.end(), pr->messages.begin(), pr->messages.end());
        for (size_t i = 0; i < eg.size(); i++) {
          const Scalar c = canonical(eg[i]);
          gte.insert(gte.end(), c.begin(), c.end());
          uint32_t row;
          if (i < 2 * R) {
            row = (uint32_t)(m0 + i);
          } else {
            const size_t j = i - 2 * R, round = j / 4;
            row = (uint32_t)(4 * (R - 2 - round) + j % 4);
          }
          terms.push_back(GtTerm{row, (uint32_t)(e0 + i)});
        }
        term_off.push_back(terms.size());
        who.push_back(s);
      }
      const size_t nx = gtx.size() / 72, ne = gte.size() / 4, nseg = seg_off.size() - 1;
      Scratch mem;
      uint8_t *d_x = nullptr, *d_e = nullptr, *d_q2 = nullptr, *d_aff = nullptr;
      if ((rc = gt_from_host(C, gtx.data(), nx, &d_x))) return rc;  // ends in a wait
      mem.p.push_back(d_x);
      if ((rc = mem.get(ne * 32, &d_e)) || (rc = mem.get(nseg * 192, &d_q2))) return rc;
      std::vector<uint64_t> out(2 * nclean * 72);
      rc = GM_OK;
      hipError_t e = hipMemcpyAsync(d_e, gte.data(), ne * 32, hipMemcpyHostToDevice, C->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(d_q2, q2.data(), nseg * 192, hipMemcpyHostToDevice, C->stream);
      if (e != hipSuccess) rc = gm::hip_fail(e, "hipMemcpyAsync", __FILE__, __LINE__);
      if (!rc) rc = g1_lincomb_many_launch(C, pts.data(), 96, sc.data(), seg_off.data(), nseg, &d_aff);
      if (!rc) {
        for (PairProduct& pp : prods) {
          pp.s0.g1 = d_aff;
          pp.s0.g2 = d_q2;
        }
        rc = gt_checks_run(C, prods.data(), d_x, nx, d_e, ne, terms.data(), term_off.data(), nclean, out.data());  // ends in the wait
      }
      (void)hipStreamSynchronize(C->stream);  // the host tables are read by their copies until here, the device ones by the kernels
      if (rc) return rc;
      const gmh::Fq12 one = gmh::Fq12::one();
      for (size_t c = 0; c < nclean; c++)
        ok[who[c]] = gmh::Fq12::from_limbs(out.data() + 72 * c) * gmh::Fq12::from_limbs(out.data() + 72 * (nclean + c)) == one ? 1 : 0;
    }
  }
  for (size_t s = 0; s < S; s++)
    if (!clean[s] && (rc = ipa_verify(C, proofs[s], vrs, comm_a + 18 * s, comm_b + 36 * s, y_mont + 4 * s, ok + s))) return rc;
  C->ipa_verify_many_last[0] = nclean;
  C->ipa_verify_many_last[1] = S - nclean;
  return GM_OK;
}

}  // namespace gm
