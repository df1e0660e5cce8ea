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
// One claim (ipa_prove, InnerProductProof::new) and K claims in one proof (ipa_prove_batch, ::generic) are ONE round loop,
// ipa_prove_rounds, over an InitialClaims the entry fills.  The entries differ in four places only: the K FModule provers that
// step; the scalars the G1Module / G2Module provers run over -- a and b from the host, limbs as they are, or the weighted sums
// ca / cb formed on the device, for every K including 1; the exponent the module messages enter with -- bch[1] and bch[2], or
// one; and where the PModule batch challenges start, 3 or 3 K.  Which of the two a call takes is the entry's, never K == 1's.
// A proof object holds K rows of foldings whichever entry made it.  ipa_prove_lockstep (many proofs in one call) is another
// algorithm and shares only the argument checks (ipa_prover_sizes).
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
// Jacobian limbs -> the affine host record (ark-ff's Montgomery form) the short linear combinations take; `out` arrives all zero,
// which is the identity
void g1_to_host_record(const uint64_t jac[18], uint64_t out[12]) {
  const gmh::G1 p = gmh::G1::from_limbs(jac);
  if (p.is_identity()) return;
  const gmh::G1 a = p.normalized();
  a.x.to_limbs(out);
  a.y.to_limbs(out + 6);
}
void g2_to_host_record(const uint64_t jac[36], uint64_t out[24]) {
  const gmh::G2 p = gmh::G2::from_limbs(jac);
  if (p.is_identity()) return;
  const gmh::G2 a = p.normalized();
  a.x.to_limbs(out);
  a.y.to_limbs(out + 12);
}

bool fr_reduced(const uint64_t* p) {
  uint64_t t[4];
  return gmh::sub_n<4>(t, p, gmh::FrP::MOD) != 0;
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

// What the initial claims bring to the batched sumcheck (ipa_prove_rounds), as InitialTerms does for the verifier: the provers an
// entry has made, freed with the call, and how their messages enter a round message.
struct InitialClaims {
  const char* who;
  std::vector<uint64_t> ff;  // the FModule prover of every claim; its message enters as E^(weights[i] a)
  uint64_t fg1 = 0, fg2 = 0;  // the G1Module and the G2Module prover
  HerringProver *h1 = nullptr, *h2 = nullptr;
  // the batch challenge the G1 / G2 module messages enter with, as an index into `weights`, or -1 for exponent one: the module
  // provers run over sums the entry has weighted already, and their final scalars are no claim's
  int e_g1 = -1, e_g2 = -1;
  std::vector<gmh::Fr> weights;  // the batch challenges of the initial claims; the PModule provers' start at first = weights.size()
  ~InitialClaims() {
    for (uint64_t h : ff) (void)gm_sc_free(h);
    if (fg1) (void)gm_hg1_free(fg1);
    if (fg2) (void)gm_hg2_free(fg2);
  }
  int add_ff(const uint64_t* a_mont, const uint64_t* b_mont, size_t d, const uint64_t one[4]) {
    uint64_t h = 0;
    int rc = gm_sc_new(a_mont, d, b_mont, d, one, &h);
    if (rc) return rc;
    ff.push_back(h);
    return gm_sc_set_herring(h, 1);
  }
  // the G1 / G2 provers get the first 2^rounds points: their messages zip against d scalars and their final folding is a
  // combination of exactly those points, so the rest of a longer CRS never enters (and need not be folded).  The points are on the
  // device and are copied; so are the scalars when `on_device` says they are there
  int add_modules(Context* C, const Crs* crs, size_t full, const void* a, const void* b, size_t d, const uint64_t one[4], bool on_device) {
    int rc;
    if ((rc = herring_create(C, HERRING_G1, crs->g1, 96, full, a, 32, d, one, &fg1, on_device ? 3 : 1))) return rc;
    if ((rc = herring_create(C, HERRING_G2, b, 32, d, crs->g2, 192, full, one, &fg2, on_device ? 3 : 2))) return rc;
    std::lock_guard<std::mutex> lk(C->mu);
    h1 = C->herring[fg1].get();
    h2 = C->herring[fg2].get();
    return GM_OK;
  }
};

// what every prover entry asks of d and the CRS; `line` is the round loop of the reference the entry restates
int ipa_prover_sizes(size_t d, const Crs* crs, const char* who, int line, size_t* rounds, size_t* full) {
  GM_CHECK(d >= 2, GM_EINVAL, "%s: d = %zu; the argument needs at least two scalars (the reference's round loop underflows at rounds - 1, ipa.rs:%d)", who, d, line);
  *rounds = (size_t)msm_ceil_log2(d);
  *full = (size_t)1 << *rounds;
  const size_t need = std::max(d + 1, *full);
  GM_CHECK(crs->n1 >= need && crs->n2 >= need, GM_EINVAL, "%s: d = %zu needs a CRS of max(d + 1, 2^rounds) = %zu points, it has %zu / %zu", who, d, need, crs->n1, crs->n2);
  return GM_OK;
}

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

// The Miller products of one round message.  aux1 holds (G1 message a, G1 message b, G1 generator), aux2 (G2 generator, G2 message
// a, G2 message b).  Segments: e(G1, G2); (fg1.a, G2), (fg1.b, G2), (G1, fg2.a), (G1, fg2.b); then a_p, b_p of every PModule prover
std::vector<PairProduct> round_products(const uint8_t* aux1, const uint8_t* aux2, const Arena& A) {
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
  return prods;
}

// The final foldings of the PModule provers (ipa.rs:655-661): every live prover folds once more, to length 1
int arena_finals(Context* C, const Crs* crs, Arena& A, const uint64_t last[4], IpaProof* proof) {
  const size_t k = A.live;
  proof->final_g1.assign(k * 18, 0);
  proof->final_g2.assign(k * 36, 0);
  if (!k) return GM_OK;
  std::vector<uint64_t> f(k * 12), g(k * 24);
  {
    GM_MSM_LOCK(C);
    int rc = arena_round(C, crs, A, gmh::Fr::from_limbs(last), false);
    if (rc) return rc;
    GM_HIP(hipMemcpyAsync(f.data(), A.g1[A.cur], k * 96, hipMemcpyDeviceToHost, C->stream));
    GM_HIP(hipMemcpyAsync(g.data(), A.g2[A.cur], k * 192, hipMemcpyDeviceToHost, C->stream));
    GM_HIP(hipStreamSynchronize(C->stream));
  }
  for (size_t p = 0; p < k; p++) {
    gmh::g1_affine_to_jac_dev(f.data() + 12 * p).to_limbs(proof->final_g1.data() + 18 * p);
    gmh::g2_affine_to_jac_dev(g.data() + 24 * (p ^ 1)).to_limbs(proof->final_g2.data() + 36 * p);
  }
  return GM_OK;
}

typedef std::chrono::steady_clock Clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// The batched sumcheck of InnerProductProof::new and ::generic (ipa.rs:584-685, 420-531) from the first message on: the entry has
// made the initial provers and drawn the first batch challenge (T.weights).  counts: split-fold launches, MSM calls, Miller
// launches, where they are issued (gm_debug_ipa_new_batch_path).
int ipa_prove_rounds(Context* C, uint64_t transcript, const Crs* crs, size_t rounds, const InitialClaims& T, IpaProof* proof, size_t counts[3]) {
  const size_t K = T.ff.size(), first = T.weights.size(), full = (size_t)1 << rounds;
  int rc;
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
  proof->K = K;
  proof->messages.assign(rounds * 144, 0);
  proof->challenges.assign(rounds * 4, 0);
  proof->batch_challenges.clear();
  proof->host_ms[0] = proof->host_ms[1] = proof->host_ms[2] = 0;
  std::vector<gmh::Fr> bch;  // batch_challenges
  auto push_bch = [&](const gmh::Fr& x) {
    bch.push_back(x);
    uint64_t l[4];
    x.to_limbs(l);
    proof->batch_challenges.insert(proof->batch_challenges.end(), l, l + 4);
  };
  for (const gmh::Fr& w : T.weights) push_bch(w);

  // One message of the batched sumcheck: the K FModule provers step in one launch group (folding by `vm` first when there is
  // one), then the two module provers, then every PModule prover's products and the carriers of the initial messages in ONE
  // segmented Miller launch, then the two GT multi-exponentiations E^(sum_i weights[i] fa_i) m_g1^e_g1 m_g2^e_g2 prod_p m_p^bch[first + p]
  std::vector<int> has_many(K);
  const Scalar unit = canonical(gmh::Fr::one());
  auto round_message = [&](const uint64_t* vm, uint64_t* out144) -> int {
    uint64_t fa[4], fb[4], g1a[18], g1b[18], g2a[36], g2b[36];
    int has = 0, r;
    if ((r = gm_sc_round_begin_many(T.ff.data(), K, vm, has_many.data()))) return r;
    gmh::Fr sa = gmh::Fr::zero(), sb = gmh::Fr::zero();
    int all = 1;
    for (size_t i = 0; i < K; i++) {
      if (!has_many[i]) {
        all = 0;
        continue;
      }
      if ((r = gm_sc_round_end(T.ff[i], fa, fb))) return r;
      sa = sa + gmh::Fr::from_limbs(fa) * bch[i];
      sb = sb + gmh::Fr::from_limbs(fb) * bch[i];
    }
    GM_CHECK(all, GM_ESTATE, "%s: an FModule prover has no message", T.who);
    if ((r = herring_round(C, T.h1, vm, g1a, g1b, &has))) return r;
    GM_CHECK(has, GM_ESTATE, "%s: the G1Module prover has no message", T.who);
    if ((r = herring_round(C, T.h2, vm, g2a, g2b, &has))) return r;
    GM_CHECK(has, GM_ESTATE, "%s: the G2Module prover has no message", T.who);
    counts[0] += vm ? 2 : 0;  // the point side of either module prover folds in one launch
    counts[1] += 1 + 3;       // g1_message: one batch of three strided MSMs; g2_message: three MSMs
    g1_to_record(gmh::G1::from_limbs(g1a), rec1);
    g1_to_record(gmh::G1::from_limbs(g1b), rec1 + 12);
    g2_to_record(gmh::G2::from_limbs(g2a), rec2 + 24);
    g2_to_record(gmh::G2::from_limbs(g2b), rec2 + 48);
    const std::vector<PairProduct> prods = round_products(aux1, aux2, A);
    std::vector<gmh::Fq12> m(prods.size());
    {
      GM_MSM_LOCK(C);
      GM_HIP(hipMemcpyAsync(aux1, rec1, sizeof rec1, hipMemcpyHostToDevice, C->stream));
      GM_HIP(hipMemcpyAsync(aux2, rec2, sizeof rec2, hipMemcpyHostToDevice, C->stream));
      if ((r = miller_products(C, prods.data(), prods.size(), m.data()))) return r;
      counts[2] += 1;
    }
    // SumcheckMsg::ip(messages, batch_challenges) (ipa.rs:636-644)
    for (int half = 0; half < 2; half++) {
      std::vector<gmh::Fq12> x = {m[0], m[1 + half], m[3 + half]};
      std::vector<Scalar> e = {canonical(half ? sb : sa), T.e_g1 < 0 ? unit : canonical(bch[T.e_g1]), T.e_g2 < 0 ? unit : canonical(bch[T.e_g2])};
      for (size_t p = 0; p < A.live; p++) {
        x.push_back(m[5 + 2 * p + half]);
        e.push_back(canonical(bch[first + p]));
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

  if ((rc = round_message(nullptr, proof->messages.data()))) return rc;
  if ((rc = gm_transcript_append_gt(transcript, (const uint8_t*)"prover_message", 14, proof->messages.data(), 2))) return rc;

  for (size_t j = 0; j + 1 < rounds; j++) {
    uint64_t *c = proof->challenges.data() + 4 * j, ch[4];
    if ((rc = gm_transcript_challenge_fr(transcript, (const uint8_t*)"sumcheck-chal", 13, c))) return rc;
    if ((rc = gm_transcript_challenge_fr(transcript, (const uint8_t*)"batch-chal", 10, ch))) return rc;
    const gmh::Fr b = gmh::Fr::from_limbs(ch);
    push_bch(b);
    push_bch(b.sqr());
    {
      GM_MSM_LOCK(C);
      if ((rc = arena_round(C, crs, A, gmh::Fr::from_limbs(c), true))) return rc;
      counts[0] += 2;
    }
    uint64_t* msg = proof->messages.data() + 144 * (j + 1);
    if ((rc = round_message(c, msg))) return rc;
    if ((rc = gm_transcript_append_gt(transcript, (const uint8_t*)"sumcheck-round", 14, msg, 2))) return rc;
  }

  uint64_t* last = proof->challenges.data() + 4 * (rounds - 1);
  if ((rc = gm_transcript_challenge_fr(transcript, (const uint8_t*)"sumcheck-chal", 13, last))) return rc;
  counts[0] += A.live ? 2 : 0;
  if ((rc = arena_finals(C, crs, A, last, proof))) return rc;

  // final foldings, a row per claim: ff_i from prover i; fg1_i = (the folded CRS point, a scalar), fg2_i = (a scalar, the folded CRS
  // point).  The scalars are the module provers' own where those ran over the claim's a and b (limbs as they came), and else
  // ff_i.lhs and ff_i.rhs: the same vector under the same challenges with twist 1
  int has = 0;
  uint64_t p1[18 + 4], p2[4 + 36];
  if ((rc = herring_fold(C, T.h1, last)) || (rc = herring_fold(C, T.h2, last))) return rc;
  counts[0] += 2;
  if ((rc = herring_final(C, T.h1, p1, p1 + 18, &has))) return rc;
  GM_CHECK(has, GM_ESTATE, "%s: the G1Module prover has no final foldings", T.who);
  if ((rc = herring_final(C, T.h2, p2, p2 + 4, &has))) return rc;
  GM_CHECK(has, GM_ESTATE, "%s: the G2Module prover has no final foldings", T.who);
  proof->foldings_ff.assign(K * 8, 0);
  proof->foldings_fg1.assign(K * 22, 0);
  proof->foldings_fg2.assign(K * 40, 0);
  for (size_t i = 0; i < K; i++) {
    uint64_t *ff = proof->foldings_ff.data() + 8 * i, *fg1 = proof->foldings_fg1.data() + 22 * i, *fg2 = proof->foldings_fg2.data() + 40 * i;
    if ((rc = gm_sc_fold(T.ff[i], last)) || (rc = gm_sc_final(T.ff[i], ff, ff + 4, &has))) return rc;
    GM_CHECK(has, GM_ESTATE, "%s: FModule prover %zu has no final foldings", T.who, i);
    memcpy(fg1, p1, 18 * 8);
    memcpy(fg1 + 18, T.e_g1 < 0 ? ff : p1 + 18, 4 * 8);
    memcpy(fg2, T.e_g2 < 0 ? ff + 4 : p2, 4 * 8);
    memcpy(fg2 + 4, p2 + 4, 36 * 8);
  }
  return GM_OK;
}

}  // namespace

// InnerProductProof::new (ipa.rs:533-685): the module provers run over a and b as the host hands them, limbs as they are, and
// their messages enter with the batch challenges bc and bc^2
int ipa_prove(Context* C, uint64_t transcript, const Crs* crs, const uint64_t* a_mont, const uint64_t* b_mont, size_t d, IpaProof* proof) {
  size_t rounds, full;
  int rc = ipa_prover_sizes(d, crs, "ipa_new", 584, &rounds, &full);
  if (rc) return rc;
  uint64_t one[4], ch[4];
  gmh::Fr::one().to_limbs(one);
  const Clock::time_point t_start = Clock::now();

  InitialClaims T{"ipa_new"};
  if ((rc = T.add_ff(a_mont, b_mont, d, one)) || (rc = T.add_modules(C, crs, full, a_mont, b_mont, d, one, false))) return rc;
  if ((rc = gm_transcript_challenge_fr(transcript, (const uint8_t*)"batch-chal", 10, ch))) return rc;
  const gmh::Fr bc = gmh::Fr::from_limbs(ch);
  T.weights = {gmh::Fr::one(), bc, bc.sqr()};
  T.e_g1 = 1;
  T.e_g2 = 2;
  size_t counts[3] = {0, 0, 0};
  if ((rc = ipa_prove_rounds(C, transcript, crs, rounds, T, proof, counts))) return rc;
  proof->host_ms[2] = ms_since(t_start);
  return GM_OK;
}

// ---- many proofs in one call: the prover ----------------------------------------------------------------------------------------
// The S proofs of gm_ipa_new_many run the rounds of ipa_prove above in lockstep.  Every proof keeps its own transcript, challenges
// and batch challenges; what is shared is the launch group of a round.  All S proofs have the same d, so in every round every
// point vector of every proof -- the live PModule vectors, the chopped CRS, the vectors of the G1Module and G2Module provers --
// has the same length M, and the state of a proof is a list of references to spans of M records: into the CRS itself (the
// module vectors before the first fold, the unfolded halves of the newest two provers) or into the current one of two
// ping-pong buffers per group.  No span is copied: a fold reads spans where they lie and writes the halves into the other buffer.
//
//   fold      k_split_fold_seg (bases.hip), one launch per group over S (live + 2) spans, a challenge per proof
//   Fr side   the vectors a and b of a proof are the FModule prover's and, with twist 1 and one challenge for all three claims,
//             also the Rhs of the G1Module and the Lhs of the G2Module prover.  Fold and messages are 5 n products per proof and
//             round and run on the host (sc_round_begin_many folds all its provers by ONE challenge; here every proof has its own)
//   messages  the G1Module / G2Module messages are the same (scalar, point) index pairs in both groups: a = sum a[2i] F[2i],
//             b = sum a[2i+1] F[2i] + a[2i] F[2i+1].  One lane per term (k_term_mul), the sums in two levels of k_seg_sum (chunks of
//             LC_CHUNK terms, then the chunks of a segment), k_normalise: 4 launches per group whatever S is.  There is no switch
//             to per-proof bucket MSMs at large term counts: the crossing lies near 48 000 terms a proof (profiles/ipa_new_many.md)
//   GT        miller_gt_products (pairing.hip): the Miller values stay on the device, the products of the 2 S message halves are
//             ONE k_gt_multi_pow_seg launch and ONE k_gt_final_exp launch; one download and the round's one wait
//
// Device memory of a call, per proof with F = 2^rounds: ping-pong buffers 2 F (96 + 192), the multiples of at most 1.5 F terms
// in XYZZ 1.5 F (192 + 384), their chunk sums, 64 d of scalars and 12 F of index tables: about 1480 F + 64 d bytes.
namespace {

constexpr size_t LC_CHUNK = 32;  // terms to a lane of the first level of sums

struct SpanRef {  // a span of the current length: records from `off` of the CRS or of the current ping-pong buffer
  bool crs = true;
  size_t off = 0;
};
struct LockstepProof {
  std::vector<gmh::Fr> a, b;  // the folded scalar vectors
  std::vector<gmh::Fr> bch;
  std::vector<SpanRef> lhs, rhs;  // PModule prover p: Lhs in G1, Rhs in G2
  SpanRef mod;                    // the G1Module's points and the G2Module's points: the same offsets in both groups
  gmh::Fr fa, fb;                 // the FModule message of the round
};

void fr_fold(std::vector<gmh::Fr>& v, const gmh::Fr& c) {
  const size_t n = v.size(), m = (n + 1) / 2;
  for (size_t i = 0; i < m; i++) v[i] = 2 * i + 1 < n ? v[2 * i] + c * v[2 * i + 1] : v[2 * i];
  v.resize(m);
}

size_t lockstep_bytes(size_t d, size_t rounds, size_t S) {
  const size_t F = (size_t)1 << rounds, T = d + (d + 1) / 2, nch = T / LC_CHUNK + 4;
  return S * (2 * F * (96 + 192) + T * (192 + 384) + nch * (192 + 384) + 2 * d * 32 + 2 * T * 4 + (nch + 3) * 8 + 2 * (2 * rounds + 1) * sizeof(FoldSpan) + 32 + 4 * (192 + 384) +
              2 * (96 + 192)) +
         4096;
}

int ipa_prove_lockstep(Context* C, const uint64_t* transcripts, const Crs* crs, const uint64_t* a_mont, const uint64_t* b_mont, size_t d, size_t S, IpaProof* const* proofs,
                       size_t* launches, size_t* waits) {
  typedef std::chrono::steady_clock Clock;
  const Clock::time_point t_start = Clock::now();
  const size_t rounds = (size_t)msm_ceil_log2(d), F = (size_t)1 << rounds;
  const size_t Tmax = S * (d + (d + 1) / 2), NCmax = Tmax / LC_CHUNK + 4 * S;
  int rc;
  // the arena, before any transcript is touched
  {
    size_t free_b = 0, total_b = 0;
    GM_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t need = lockstep_bytes(d, rounds, S);
    GM_CHECK(need <= free_b, GM_ENOMEM, "ipa_new_many: %zu proofs of d = %zu need an arena of %zu bytes, the device has %zu free", S, d, need, free_b);
  }
  Scratch mem;
  uint8_t *P1[2], *P2[2], *T1, *T2, *CS1, *CS2, *SUM1, *SUM2, *A1, *A2, *d_sc, *d_pidx, *d_sidx, *d_off1, *d_off2, *d_ch, *d_sp1, *d_sp2;
  const size_t max_spans = S * (2 * rounds + 1);
  for (int i = 0; i < 2; i++)
    if ((rc = mem.get(S * F * 96, &P1[i])) || (rc = mem.get(S * F * 192, &P2[i]))) return rc;
  if ((rc = mem.get(Tmax * 192, &T1)) || (rc = mem.get(Tmax * 384, &T2)) || (rc = mem.get(NCmax * 192, &CS1)) || (rc = mem.get(NCmax * 384, &CS2)) ||
      (rc = mem.get(2 * S * 192, &SUM1)) || (rc = mem.get(2 * S * 384, &SUM2)) || (rc = mem.get((1 + 2 * S) * 96, &A1)) || (rc = mem.get((1 + 2 * S) * 192, &A2)) ||
      (rc = mem.get(S * 2 * d * 32, &d_sc)) || (rc = mem.get(Tmax * 4, &d_pidx)) || (rc = mem.get(Tmax * 4, &d_sidx)) || (rc = mem.get((NCmax + 1) * 8, &d_off1)) ||
      (rc = mem.get((2 * S + 1) * 8, &d_off2)) || (rc = mem.get(S * 32, &d_ch)) || (rc = mem.get(max_spans * sizeof(FoldSpan), &d_sp1)) ||
      (rc = mem.get(max_spans * sizeof(FoldSpan), &d_sp2)))
    return rc;

  std::vector<LockstepProof> L(S);
  for (size_t s = 0; s < S; s++) {
    L[s].a.resize(d);
    L[s].b.resize(d);
    for (size_t i = 0; i < d; i++) {
      L[s].a[i] = gmh::Fr::from_limbs(a_mont + 4 * (s * d + i));
      L[s].b[i] = gmh::Fr::from_limbs(b_mont + 4 * (s * d + i));
    }
    IpaProof* pr = proofs[s];
    pr->rounds = rounds;
    pr->messages.assign(rounds * 144, 0);
    pr->challenges.assign(rounds * 4, 0);
    pr->batch_challenges.clear();
    pr->host_ms[0] = pr->host_ms[1] = pr->host_ms[2] = 0;
  }
  auto push_bch = [&](size_t s, const gmh::Fr& x) {
    L[s].bch.push_back(x);
    uint64_t l[4];
    x.to_limbs(l);
    proofs[s]->batch_challenges.insert(proofs[s]->batch_challenges.end(), l, l + 4);
  };
  int cur = 0;
  size_t M = F, live = 0;
  auto ptr1 = [&](const SpanRef& r) -> uint8_t* { return (r.crs ? crs->g1 : P1[cur]) + r.off * 96; };
  auto ptr2 = [&](const SpanRef& r) -> uint8_t* { return (r.crs ? crs->g2 : P2[cur]) + r.off * 192; };
  uint64_t gen1[12], gen2[24];
  g1_to_record(g1_generator(), gen1);
  g2_to_record(g2_generator(), gen2);
  bool gens_up = false;

  // host tables of the round in flight: read by their copies until the round's wait
  std::vector<uint64_t> h_ch, h_sc, h_exp;
  std::vector<FoldSpan> h_sp1, h_sp2;
  std::vector<uint32_t> h_pidx, h_sidx;
  std::vector<unsigned long long> h_off1, h_off2;

  // every span of every proof folds by the proof's challenge ch[s]: one launch per group.  with_crs: the first M points of the CRS
  // fold as one more span and become, with their unfolded first half, the vectors of two new provers.  Enqueues only.
  auto fold_all = [&](const std::vector<gmh::Fr>& ch, bool with_crs) -> int {
    const size_t m = M / 2;
    h_ch.resize(4 * S);
    h_sp1.clear();
    h_sp2.clear();
    for (size_t s = 0; s < S; s++) {
      ch[s].to_canonical(h_ch.data() + 4 * s);
      LockstepProof& p = L[s];
      size_t at = s * F;  // the proof's region of the other buffer, in records
      auto put = [&](const uint8_t* in1, const uint8_t* in2) {
        h_sp1.push_back(FoldSpan{in1, P1[cur ^ 1] + at * 96, (uint32_t)s, 0});
        h_sp2.push_back(FoldSpan{in2, P2[cur ^ 1] + at * 192, (uint32_t)s, 0});
        const size_t was = at;
        at += m;
        return was;
      };
      for (size_t k = 0; k < live; k++) {
        const size_t o = put(ptr1(p.lhs[k]), ptr2(p.rhs[k]));
        p.lhs[k] = p.rhs[k] = SpanRef{false, o};
      }
      if (with_crs) {
        const size_t o = put(crs->g1, crs->g2);
        p.lhs.push_back(SpanRef{false, o});  // g1fold: the folded G1 half against the unfolded G2 half
        p.rhs.push_back(SpanRef{true, 0});
        p.lhs.push_back(SpanRef{true, 0});   // g2fold
        p.rhs.push_back(SpanRef{false, o});
      }
      const size_t o = put(ptr1(p.mod), ptr2(p.mod));
      p.mod = SpanRef{false, o};
    }
    const size_t nsp = h_sp1.size();
    GM_HIP(hipMemcpyAsync(d_ch, h_ch.data(), S * 32, hipMemcpyHostToDevice, C->stream));
    GM_HIP(hipMemcpyAsync(d_sp1, h_sp1.data(), nsp * sizeof(FoldSpan), hipMemcpyHostToDevice, C->stream));
    GM_HIP(hipMemcpyAsync(d_sp2, h_sp2.data(), nsp * sizeof(FoldSpan), hipMemcpyHostToDevice, C->stream));
    int r;
    if ((r = g1_split_fold_seg_launch(C, reinterpret_cast<const FoldSpan*>(d_sp1), nsp, M, reinterpret_cast<const uint32_t*>(d_ch)))) return r;
    if ((r = g2_split_fold_seg_launch(C, reinterpret_cast<const FoldSpan*>(d_sp2), nsp, M, reinterpret_cast<const uint32_t*>(d_ch)))) return r;
    *launches += 2;
    cur ^= 1;
    M = m;
    if (with_crs) live += 2;
    return GM_OK;
  };

  // the message of every proof for the current vectors, into proofs[s]->messages at round j.  Enqueues, then the round's wait.
  auto messages_all = [&](size_t j) -> int {
    const size_t n = L[0].a.size(), ce = (n + 1) / 2, fl = n / 2;
    int r;
    if (!gens_up) {
      GM_HIP(hipMemcpyAsync(A1, gen1, 96, hipMemcpyHostToDevice, C->stream));
      GM_HIP(hipMemcpyAsync(A2, gen2, 192, hipMemcpyHostToDevice, C->stream));
      gens_up = true;
    }
    // scalars: a_s at rows 2 s n, b_s at rows (2 s + 1) n; the terms of both groups are the same (scalar, point) index pairs
    h_sc.resize(S * 2 * n * 4);
    h_pidx.clear();
    h_sidx.clear();
    h_off1.clear();
    h_off2.clear();
    const bool in_crs = L[0].mod.crs;  // before the first fold every module vector is the CRS itself
    auto seg_end = [&](size_t t0) {    // the segment [t0, now) in chunks
      h_off2.push_back(h_off1.size());
      for (size_t t = t0; t < h_pidx.size(); t += LC_CHUNK) h_off1.push_back(t);
    };
    for (size_t s = 0; s < S; s++) {
      const LockstepProof& p = L[s];
      for (size_t i = 0; i < n; i++) {
        p.a[i].to_limbs(h_sc.data() + 4 * (2 * s * n + i));
        p.b[i].to_limbs(h_sc.data() + 4 * ((2 * s + 1) * n + i));
      }
      const uint32_t sb = (uint32_t)(2 * s * n), pb = (uint32_t)p.mod.off;
      size_t t0 = h_pidx.size();
      for (size_t i = 0; i < ce; i++) {
        h_sidx.push_back(sb + 2 * i);
        h_pidx.push_back(pb + 2 * i);
      }
      seg_end(t0);
      t0 = h_pidx.size();
      for (size_t i = 0; i < fl; i++) {
        h_sidx.push_back(sb + 2 * i + 1);
        h_pidx.push_back(pb + 2 * i);
      }
      for (size_t i = 0; i < ce; i++) {
        h_sidx.push_back(sb + 2 * i);
        h_pidx.push_back(pb + 2 * i + 1);
      }
      seg_end(t0);
    }
    const size_t T = h_pidx.size(), nch = h_off1.size();
    h_off1.push_back(T);
    h_off2.push_back(nch);
    GM_CHECK(T <= Tmax && nch <= NCmax, GM_ESTATE, "ipa_new_many: %zu terms in %zu chunks do not fit the arena (%zu, %zu)", T, nch, Tmax, NCmax);
    GM_HIP(hipMemcpyAsync(d_sc, h_sc.data(), S * 2 * n * 32, hipMemcpyHostToDevice, C->stream));
    GM_HIP(hipMemcpyAsync(d_pidx, h_pidx.data(), T * 4, hipMemcpyHostToDevice, C->stream));
    GM_HIP(hipMemcpyAsync(d_sidx, h_sidx.data(), T * 4, hipMemcpyHostToDevice, C->stream));
    GM_HIP(hipMemcpyAsync(d_off1, h_off1.data(), (nch + 1) * 8, hipMemcpyHostToDevice, C->stream));
    GM_HIP(hipMemcpyAsync(d_off2, h_off2.data(), (2 * S + 1) * 8, hipMemcpyHostToDevice, C->stream));
    const uint32_t *pi = reinterpret_cast<const uint32_t*>(d_pidx), *si = reinterpret_cast<const uint32_t*>(d_sidx);
    const unsigned long long *o1 = reinterpret_cast<const unsigned long long*>(d_off1), *o2 = reinterpret_cast<const unsigned long long*>(d_off2);
    if ((r = g1_term_mul_launch(C, in_crs ? crs->g1 : P1[cur], pi, d_sc, si, 1, T, T1)) || (r = g1_seg_sum_launch(C, T1, o1, nch, CS1)) ||
        (r = g1_seg_sum_launch(C, CS1, o2, 2 * S, SUM1)) || (r = g1_normalise_launch(C->stream, SUM1, 2 * S, A1 + 96)))
      return r;
    if ((r = g2_term_mul_launch(C, in_crs ? crs->g2 : P2[cur], pi, d_sc + n * 32, si, 1, T, T2)) || (r = g2_seg_sum_launch(C, T2, o1, nch, CS2)) ||
        (r = g2_seg_sum_launch(C, CS2, o2, 2 * S, SUM2)) || (r = g2_normalise_launch(C->stream, SUM2, 2 * S, A2 + 192)))
      return r;
    *launches += 8;
    // Miller segments of proof s: e(G1, G2); (fg1.a, G2), (fg1.b, G2), (G1, fg2.a), (G1, fg2.b); then a_p, b_p of every PModule prover
    const size_t per = 5 + 2 * live, eper = 4 + live, h = M / 2;
    std::vector<PairProduct> prods(S * per);
    std::vector<GtTerm> terms;
    std::vector<size_t> toff(1, 0);
    h_exp.resize(S * eper * 4);
    for (size_t s = 0; s < S; s++) {
      const LockstepProof& p = L[s];
      PairProduct* q = prods.data() + s * per;
      q[0].s0 = span(A1, 0, 1, A2, 0, 1, 1);
      q[1].s0 = span(A1, 1 + 2 * s, 1, A2, 0, 1, 1);
      q[2].s0 = span(A1, 2 + 2 * s, 1, A2, 0, 1, 1);
      q[3].s0 = span(A1, 0, 1, A2, 1 + 2 * s, 1, 1);
      q[4].s0 = span(A1, 0, 1, A2, 2 + 2 * s, 1, 1);
      for (size_t k = 0; k < live; k++) {
        const uint8_t *f = ptr1(p.lhs[k]), *g = ptr2(p.rhs[k]);
        q[5 + 2 * k].s0 = span(f, 0, 2, g, 0, 2, h);      // a = ip(f_even, g_even)
        q[5 + 2 * k + 1].s0 = span(f, 0, 2, g, 1, 2, h);  // b = ip(f_even, g_odd) + ip(f_odd, g_even)
        q[5 + 2 * k + 1].s1 = span(f, 1, 2, g, 0, 2, h);
      }
      // SumcheckMsg::ip(messages, batch_challenges): exponents [fa bch0, fb bch0, bch1, bch2, bch3 ..] of the proof
      uint64_t* e = h_exp.data() + 4 * s * eper;
      (p.fa * p.bch[0]).to_canonical(e);
      (p.fb * p.bch[0]).to_canonical(e + 4);
      for (size_t k = 1; k < 3 + live; k++) p.bch[k].to_canonical(e + 4 * (k + 1));
      const uint32_t x0 = (uint32_t)(s * per), e0 = (uint32_t)(s * eper);
      for (uint32_t half = 0; half < 2; half++) {
        terms.push_back(GtTerm{x0, e0 + half});
        terms.push_back(GtTerm{x0 + 1 + half, e0 + 2});
        terms.push_back(GtTerm{x0 + 3 + half, e0 + 3});
        for (size_t k = 0; k < live; k++) terms.push_back(GtTerm{(uint32_t)(x0 + 5 + 2 * k + half), (uint32_t)(e0 + 4 + k)});
        toff.push_back(terms.size());
      }
    }
    std::vector<uint64_t> out(2 * S * 72);
    r = miller_gt_products(C, prods.data(), prods.size(), h_exp.data(), S * eper, terms.data(), toff.data(), 2 * S, out.data(), launches);
    *waits += 1;
    if (r) return r;
    for (size_t s = 0; s < S; s++) memcpy(proofs[s]->messages.data() + 144 * j, out.data() + 144 * s, 144 * 8);
    return GM_OK;
  };
  // the FModule message of every proof, on the host
  auto fr_messages = [&]() {
    for (size_t s = 0; s < S; s++) {
      LockstepProof& p = L[s];
      const size_t n = p.a.size();
      gmh::Fr a = gmh::Fr::zero(), b = gmh::Fr::zero();
      for (size_t i = 0; 2 * i < n; i++) {
        a = a + p.a[2 * i] * p.b[2 * i];
        if (2 * i + 1 < n) b = b + p.a[2 * i] * p.b[2 * i + 1] + p.b[2 * i] * p.a[2 * i + 1];
      }
      p.fa = a;
      p.fb = b;
    }
  };
  // a failure between the launches and the wait: nothing of this call may still be read when its tables and its arena go
  auto fail = [&](int r) {
    (void)hipStreamSynchronize(C->stream);
    return r;
  };

  uint64_t ch[4];
  for (size_t s = 0; s < S; s++) {
    if ((rc = gm_transcript_challenge_fr(transcripts[s], (const uint8_t*)"batch-chal", 10, ch))) return rc;
    const gmh::Fr bc = gmh::Fr::from_limbs(ch);
    push_bch(s, gmh::Fr::one());
    push_bch(s, bc);
    push_bch(s, bc.sqr());
  }
  fr_messages();
  {
    GM_MSM_LOCK(C);
    if ((rc = messages_all(0))) return fail(rc);
  }
  for (size_t s = 0; s < S; s++)
    if ((rc = gm_transcript_append_gt(transcripts[s], (const uint8_t*)"prover_message", 14, proofs[s]->messages.data(), 2))) return rc;

  std::vector<gmh::Fr> cs(S);
  for (size_t j = 0; j + 1 < rounds; j++) {
    for (size_t s = 0; s < S; s++) {
      uint64_t* c = proofs[s]->challenges.data() + 4 * j;
      if ((rc = gm_transcript_challenge_fr(transcripts[s], (const uint8_t*)"sumcheck-chal", 13, c))) return rc;
      if ((rc = gm_transcript_challenge_fr(transcripts[s], (const uint8_t*)"batch-chal", 10, ch))) return rc;
      const gmh::Fr b = gmh::Fr::from_limbs(ch);
      push_bch(s, b);
      push_bch(s, b.sqr());
      cs[s] = gmh::Fr::from_limbs(c);
      fr_fold(L[s].a, cs[s]);
      fr_fold(L[s].b, cs[s]);
    }
    fr_messages();
    {
      GM_MSM_LOCK(C);
      if ((rc = fold_all(cs, true)) || (rc = messages_all(j + 1))) return fail(rc);
    }
    for (size_t s = 0; s < S; s++)
      if ((rc = gm_transcript_append_gt(transcripts[s], (const uint8_t*)"sumcheck-round", 14, proofs[s]->messages.data() + 144 * (j + 1), 2))) return rc;
  }

  for (size_t s = 0; s < S; s++) {
    uint64_t* last = proofs[s]->challenges.data() + 4 * (rounds - 1);
    if ((rc = gm_transcript_challenge_fr(transcripts[s], (const uint8_t*)"sumcheck-chal", 13, last))) return rc;
    cs[s] = gmh::Fr::from_limbs(last);
    fr_fold(L[s].a, cs[s]);
    fr_fold(L[s].b, cs[s]);
  }
  // final foldings: every PModule prover and the two module vectors fold once more, to length 1 -- one more segmented fold per
  // group and ONE download: proof s has its live + 1 records back to back from record s F of the buffers
  const size_t k = live, per = k + 1;
  std::vector<uint64_t> f(S * per * 12), g(S * per * 24);
  {
    GM_MSM_LOCK(C);
    if ((rc = fold_all(cs, false))) return fail(rc);
    hipError_t e = hipMemcpy2DAsync(f.data(), per * 96, P1[cur], F * 96, per * 96, S, hipMemcpyDeviceToHost, C->stream);
    if (e == hipSuccess) e = hipMemcpy2DAsync(g.data(), per * 192, P2[cur], F * 192, per * 192, S, hipMemcpyDeviceToHost, C->stream);
    const hipError_t e2 = hipStreamSynchronize(C->stream);
    *waits += 1;
    GM_HIP(e);
    GM_HIP(e2);
  }
  const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t_start).count();
  for (size_t s = 0; s < S; s++) {
    IpaProof* pr = proofs[s];
    const LockstepProof& p = L[s];
    pr->final_g1.assign(k * 18, 0);
    pr->final_g2.assign(k * 36, 0);
    const uint64_t *fs = f.data() + s * per * 12, *gs = g.data() + s * per * 24;
    for (size_t q = 0; q < k; q++) {  // the spans were written in the order of the provers, the module vector last
      gmh::g1_affine_to_jac_dev(fs + 12 * q).to_limbs(pr->final_g1.data() + 18 * q);
      gmh::g2_affine_to_jac_dev(gs + 24 * q).to_limbs(pr->final_g2.data() + 36 * q);
    }
    pr->foldings_ff.assign(8, 0);
    pr->foldings_fg1.assign(22, 0);
    pr->foldings_fg2.assign(40, 0);
    p.a[0].to_limbs(pr->foldings_ff.data());
    p.b[0].to_limbs(pr->foldings_ff.data() + 4);
    gmh::g1_affine_to_jac_dev(fs + 12 * k).to_limbs(pr->foldings_fg1.data());
    p.a[0].to_limbs(pr->foldings_fg1.data() + 18);
    p.b[0].to_limbs(pr->foldings_fg2.data());
    gmh::g2_affine_to_jac_dev(gs + 24 * k).to_limbs(pr->foldings_fg2.data() + 4);
    pr->host_ms[2] = ms;  // of the whole call: the proofs were made together
  }
  return GM_OK;
}

}  // namespace

int ipa_prove_many(Context* C, const uint64_t* transcripts, const Crs* crs, const uint64_t* a_mont, const uint64_t* b_mont, size_t d, size_t S, IpaProof* const* proofs) {
  size_t rounds, full;
  int rc = ipa_prover_sizes(d, crs, "ipa_new_many", 584, &rounds, &full);
  if (rc) return rc;
  GM_CHECK(S <=((size_t)1 << 16) && d <= ((size_t)1 << 24) && S * d <= ((size_t)1 << 28), GM_EINVAL, "ipa_new_many: %zu proofs of d = %zu (at most 2^28 scalars a side)", S, d);
  // the lockstep path computes with reduced residues; the per-proof path takes limbs as they are
  bool lockstep = S >= C->ipa_new_many_min && S > 0;
  for (size_t i = 0; lockstep && i < S * d; i++) lockstep = fr_reduced(a_mont + 4 * i) && fr_reduced(b_mont + 4 * i);
  size_t counts[4] = {0, 0, 0, 0};
  if (lockstep) {
    counts[0] = S;
    rc = ipa_prove_lockstep(C, transcripts, crs, a_mont, b_mont, d, S, proofs, &counts[2], &counts[3]);
  } else {
    counts[1] = S;
    for (size_t s = 0; s < S && !rc; s++) rc = ipa_prove(C, transcripts[s], crs, a_mont + 4 * s * d, b_mont + 4 * s * d, d, proofs[s]);
  }
  {
    GM_MSM_LOCK(C);
    memcpy(C->ipa_new_many_last, counts, sizeof counts);
  }
  return rc;
}

// InnerProductProof::verify_transcript (ipa.rs:250-343), GT written multiplicatively.  Its pairings -- the two commitments, the
// foldings of the initial claims and every PModule final folding -- are the 1-pair segments of ONE segmented launch; the claim and the
// expected value take one final exponentiation each.
namespace {

// What the initial claims put into the check: the points paired with a generator and the exponents of the six terms.  One claim
// (ipa_verify): the commitments and the fg1 / fg2 points of the proof, y bch0, bch1, bch2 and ff.lhs ff.rhs bch0, fg1.rhs bch1,
// fg2.lhs bch2.  K claims (ipa_verify_batch): the four weighted sums over the claims, with exponent one.
struct InitialTerms {
  gmh::G1 comm_a, fg1;
  gmh::G2 comm_b, fg2;
  Scalar e_y, e_comm_a, e_comm_b;  // claim_0 = E^e_y e(comm_a, G2)^e_comm_a e(G1, comm_b)^e_comm_b   (:284-290)
  Scalar e_ff, e_fg1, e_fg2;       // expected = E^e_ff e(fg1, G2)^e_fg1 e(G1, fg2)^e_fg2 prod_p e(lhs_p, rhs_p)^bch[first + p]
  size_t first;                    // of the PModule provers' batch challenges: 3 K
};

// what a verifier of K claims asks of a proof and of the Vrs (none: the lengths alone)
int ipa_shape(const IpaProof* pr, const Vrs* vrs, size_t K, const char* who) {
  const size_t R = pr->rounds, k = R >= 1 ? 2 * (R - 1) : 0;
  GM_CHECK(K >= 1 && K == pr->K, GM_EINVAL, "%s: %zu claims for a proof of %zu (gm_ipa_verify_batch takes a proof for several)", who, K, pr->K);
  GM_CHECK(R >= 1 && pr->messages.size() == R * 144 && pr->challenges.size() == R * 4 && pr->batch_challenges.size() == (3 * K + k) * 4 && pr->final_g1.size() == k * 18 &&
               pr->final_g2.size() == k * 36 && pr->foldings_ff.size() == K * 8 && pr->foldings_fg1.size() == K * 22 && pr->foldings_fg2.size() == K * 40,
           GM_EINVAL, "%s: the proof's fields do not have the lengths of %zu rounds and %zu claims", who, R, K);
  GM_CHECK(!vrs || vrs->levels + 1 >= R, GM_EINVAL, "%s: a proof of %zu rounds needs %zu levels of the Vrs, it has %zu", who, R, R - 1, vrs ? vrs->levels : 0);
  return GM_OK;
}

int ipa_verify_terms(Context* C, const IpaProof* pr, const Vrs* vrs, const InitialTerms& T, int* ok) {
  const size_t R = pr->rounds, k = 2 * (R - 1), n0 = T.first;
  auto fr = [](const uint64_t* p) { return gmh::Fr::from_limbs(p); };
  std::vector<gmh::Fr> bch(n0 + k), ch(R);
  for (size_t i = 0; i < n0 + k; i++) bch[i] = fr(pr->batch_challenges.data() + 4 * i);
  for (size_t i = 0; i < R; i++) ch[i] = fr(pr->challenges.data() + 4 * i);

  // records: G1 = generator, comm_a, fg1's f0, the Lhs final foldings; G2 = generator, comm_b, fg2's g0, the Rhs final foldings
  std::vector<uint64_t> r1((3 + k) * 12), r2((3 + k) * 24);
  g1_to_record(g1_generator(), r1.data());
  g1_to_record(T.comm_a, r1.data() + 12);
  g1_to_record(T.fg1, r1.data() + 24);
  g2_to_record(g2_generator(), r2.data());
  g2_to_record(T.comm_b, r2.data() + 24);
  g2_to_record(T.fg2, r2.data() + 48);
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
  gmh::Fq12 claim = gt_finish(gt_multi_pow({m[0], m[1], m[2]}, {T.e_y, T.e_comm_a, T.e_comm_b}));
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
    claim = step(i) * gt_pow(g1c, bch[n0 + 2 * i]) * gt_pow(g2c, bch[n0 + 2 * i + 1]);
  }
  claim = step(R - 1);
  // expected = ip(final_foldings, batch_challenges)   (:314-336); p(f0, g0) of the initial claims moves g0 / f0 into the exponent
  std::vector<gmh::Fq12> x = {m[0], m[3], m[4]};
  std::vector<Scalar> e = {T.e_ff, T.e_fg1, T.e_fg2};
  for (size_t p = 0; p < k; p++) {
    x.push_back(m[5 + p]);
    e.push_back(canonical(bch[n0 + p]));
  }
  *ok = claim == gt_finish(gt_multi_pow(x, e)) ? 1 : 0;
  return GM_OK;
}

}  // namespace

int ipa_verify(Context* C, const IpaProof* pr, const Vrs* vrs, const uint64_t comm_a[18], const uint64_t comm_b[36], const uint64_t y_mont[4], int* ok) {
  int rc = ipa_shape(pr, vrs, 1, "ipa_verify");
  if (rc) return rc;
  auto fr = [](const uint64_t* p) { return gmh::Fr::from_limbs(p); };
  const gmh::Fr b0 = fr(pr->batch_challenges.data()), b1 = fr(pr->batch_challenges.data() + 4), b2 = fr(pr->batch_challenges.data() + 8);
  const uint64_t *ff = pr->foldings_ff.data(), *fg1 = pr->foldings_fg1.data(), *fg2 = pr->foldings_fg2.data();
  InitialTerms T;
  T.comm_a = gmh::G1::from_limbs(comm_a);
  T.comm_b = gmh::G2::from_limbs(comm_b);
  T.fg1 = gmh::G1::from_limbs(fg1);
  T.fg2 = gmh::G2::from_limbs(fg2 + 4);
  T.e_y = canonical(fr(y_mont) * b0);
  T.e_comm_a = canonical(b1);
  T.e_comm_b = canonical(b2);
  T.e_ff = canonical(fr(ff) * fr(ff + 4) * b0);
  T.e_fg1 = canonical(fr(fg1 + 18) * b1);
  T.e_fg2 = canonical(fr(fg2) * b2);
  T.first = 3;
  return ipa_verify_terms(C, pr, vrs, T, ok);
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
  pair.push_back((fr(pr->foldings_ff.data()) * fr(pr->foldings_ff.data() + 4) * bch[0]).neg());
  pair.push_back((fr(pr->foldings_fg1.data() + 18) * bch[1]).neg());
  pair.push_back((fr(pr->foldings_fg2.data()) * bch[2]).neg());
  for (size_t p = 0; p < k; p++) pair.push_back(bch[3 + p].neg());
}

// every scalar the verifier of K claims multiplies is a reduced residue, the challenges of the rounds apart
bool ipa_claims_reduced(const IpaProof* pr, const uint64_t* y_mont, size_t K) {
  bool ok = true;
  for (size_t i = 0; i < K; i++)
    ok = ok && fr_reduced(y_mont + 4 * i) && fr_reduced(pr->foldings_ff.data() + 8 * i) && fr_reduced(pr->foldings_ff.data() + 8 * i + 4) &&
         fr_reduced(pr->foldings_fg1.data() + 22 * i + 18) && fr_reduced(pr->foldings_fg2.data() + 40 * i);
  for (size_t i = 0; i < pr->batch_challenges.size(); i += 4) ok = ok && fr_reduced(pr->batch_challenges.data() + i);
  return ok;
}
// every scalar the stated form multiplies is a reduced residue (the per-proof path takes limbs as they are)
bool ipa_scalars_reduced(const IpaProof* pr, const uint64_t y_mont[4]) {
  bool ok = ipa_claims_reduced(pr, y_mont, 1);
  for (size_t i = 0; i < pr->challenges.size(); i += 4) ok = ok && fr_reduced(pr->challenges.data() + i);
  return ok;
}

// an affine host record (ark-ff's Montgomery form, the identity all zero) -> the packed record of the device
void g2_record_to_device(const uint64_t in[24], uint64_t out[24]) {
  for (int c = 0; c < 4; c++) gmh::fq_to_device(gmh::Fq::from_limbs(in + 6 * c), out + 6 * c);
}

}  // namespace

int ipa_stated_terms(const IpaProof* pr, const uint64_t y_mont[4], uint64_t* gt_exp, uint64_t* pair_exp) {
  int rc = ipa_shape(pr, nullptr, 1, "ipa_stated_terms");
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
    if ((rc = ipa_shape(proofs[s], vrs, 1, "ipa_verify_many"))) return rc;
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
      j1.push_back(pr->foldings_fg1.data());
      j2.push_back(comm_b + 36 * s);
      j2.push_back(pr->foldings_fg2.data() + 4);
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

// ---- one proof for many claims ----------------------------------------------------------------------------------------------------
// InnerProductProof::generic (ipa.rs:345-531) for K claims <a_i, b_i> = y_i, <a_i, crs.g1> = comm_a_i, <b_i, crs.g2> = comm_b_i with
// every twist one and every vector of length d: ONE batched sumcheck, one set of round messages and one set of CRS-fold provers.
// Run literally that is 3 K initial provers.  The batch weights of the initial provers are powers(bc, 3 K) of the first batch
// challenge and stay fixed for the whole proof, and fold and message of a module prover are linear in its scalar side, so
//
//   the K G1Module provers over crs.g1 are ONE G1Module prover over ca = sum_i bc^(K+i) a_i, its messages entering with weight 1
//   the K G2Module provers over crs.g2 are ONE G2Module prover over cb = sum_i bc^(2K+i) b_i, likewise
//   the final scalar of G1Module prover i is the final lhs of FModule prover i (the same vector, the same challenges, twist 1), the
//   final point is the folded CRS for every i; the same holds for G2 with rhs
//
// and only the K FModule provers stay per claim: they step together (gm_sc_round_begin_many, one challenge for all).  The rounds
// are ipa_prove_rounds, as for ipa_prove; this entry does the upload and the sums for every K, 1 included.  tests/ipa_batch_ref.py states both forms on
// Python integers and holds them equal field for field.  No witness takes a twist: the reference's TimeProver uses the twist in
// `fold` and not in the message (time_prover.rs:83-123), so a proof with another twist cannot satisfy the verifier.
int ipa_prove_batch(Context* C, uint64_t transcript, const Crs* crs, const uint64_t* a_mont, const uint64_t* b_mont, size_t d, size_t K, IpaProof* proof) {
  // every refusal comes before the first challenge
  GM_CHECK(K >= 1, GM_EINVAL, "ipa_new_batch: no claims");
  size_t rounds, full;
  int rc = ipa_prover_sizes(d, crs, "ipa_new_batch", 420, &rounds, &full);
  if (rc) return rc;
  GM_CHECK(transcript_exists(transcript), GM_EHANDLE, "ipa_new_batch: unknown transcript handle %llu", (unsigned long long)transcript);
  {
    // the PModule arena and the message records, then the scalars: a_i and b_i in their FModule prover and once more for the sums
    const size_t arena = (rounds > 1 ? 4 * full * (96 + 192) : 0) + 3 * (96 + 192) + 2 * d * 32;
    size_t free_b = 0, total_b = 0;
    GM_HIP(hipMemGetInfo(&free_b, &total_b));
    const bool fits = K <= (SIZE_MAX - arena) / (4 * d * 32) && arena + 4 * K * d * 32 <= free_b;
    GM_CHECK(fits, GM_ENOMEM, "ipa_new_batch: %zu claims of d = %zu need an arena of %zu bytes and 4 K d 32 bytes of scalars, the device has %zu free", K, d, arena, free_b);
  }
  uint64_t one[4], ch[4];
  gmh::Fr::one().to_limbs(one);
  const Clock::time_point t_start = Clock::now();

  InitialClaims T{"ipa_new_batch"};
  for (size_t i = 0; i < K; i++)
    if ((rc = T.add_ff(a_mont + 4 * i * d, b_mont + 4 * i * d, d, one))) return rc;
  Scratch mem;
  uint8_t *d_ab = nullptr, *d_c = nullptr;  // d_ab: a_0 .. a_{K-1}, b_0 .. b_{K-1}; d_c: ca, cb
  if ((rc = mem.get(2 * K * d * 32, &d_ab)) || (rc = mem.get(2 * d * 32, &d_c))) return rc;
  GM_HIP(hipMemcpyAsync(d_ab, a_mont, K * d * 32, hipMemcpyHostToDevice, C->stream));
  GM_HIP(hipMemcpyAsync(d_ab + K * d * 32, b_mont, K * d * 32, hipMemcpyHostToDevice, C->stream));
  GM_HIP(hipStreamSynchronize(C->stream));

  // the first batch challenge fixes the weights of the 3 K initial provers: the sums, then the two module provers over them
  if ((rc = gm_transcript_challenge_fr(transcript, (const uint8_t*)"batch-chal", 10, ch))) return rc;
  const gmh::Fr bc = gmh::Fr::from_limbs(ch);
  std::vector<uint64_t> w(3 * K * 4);
  T.weights.assign(3 * K, gmh::Fr::one());
  for (size_t i = 0; i < 3 * K; i++) {
    if (i) T.weights[i] = T.weights[i - 1] * bc;
    T.weights[i].to_limbs(w.data() + 4 * i);
  }
  if ((rc = fr_lincomb_raw(C, d_ab, d * 32, d, w.data() + 4 * K, K, d_c))) return rc;
  if ((rc = fr_lincomb_raw(C, d_ab + K * d * 32, d * 32, d, w.data() + 8 * K, K, d_c + d * 32))) return rc;
  GM_HIP(hipStreamSynchronize(C->stream));
  if ((rc = T.add_modules(C, crs, full, d_c, d_c + d * 32, d, one, true))) return rc;

  size_t counts[3] = {0, 0, 0};
  if ((rc = ipa_prove_rounds(C, transcript, crs, rounds, T, proof, counts))) return rc;
  proof->host_ms[2] = ms_since(t_start);
  {
    GM_MSM_LOCK(C);
    memcpy(C->ipa_new_batch_last, counts, sizeof counts);
  }
  return GM_OK;
}

// verify_transcript (ipa.rs:250-343) with 3 K initial claims.  claim_0 = ip([E^y_i] ++ [e(comm_a_i, G2)] ++ [e(G1, comm_b_i)], bch[..3K])
// and the initial part of the expected value, ip over (ff_i, fg1_i, fg2_i), are bilinear in the points, so the 4 K pairings are four:
// sum_i bch[K+i] comm_a_i and sum_i bch[K+i] fg1_i.rhs fg1_i.lhs in G1, sum_i bch[2K+i] comm_b_i and sum_i bch[2K+i] fg2_i.lhs
// fg2_i.rhs in G2, each of K terms through the short linear combinations (k_term_mul, k_seg_sum with the complete addition: a hostile
// proof can make terms equal or opposite).  The FModule terms are one exponent of E each.  Launches do not depend on K.  As
// ipa_verify, it takes the points as members (gm_ipa_check says whether they are).
int ipa_verify_batch(Context* C, const IpaProof* pr, const Vrs* vrs, const uint64_t* comm_a, const uint64_t* comm_b, const uint64_t* y_mont, size_t K, int* ok) {
  int rc = ipa_shape(pr, vrs, K, "ipa_verify_batch");
  if (rc) return rc;
  GM_CHECK(ipa_claims_reduced(pr, y_mont, K), GM_EINVAL, "ipa_verify_batch: a y, a folding scalar or a batch challenge is not a reduced residue");
  if (K == 1) return ipa_verify(C, pr, vrs, comm_a, comm_b, y_mont, ok);  // gm_ipa_verify's verdict on every input

  auto fr = [](const uint64_t* p) { return gmh::Fr::from_limbs(p); };
  const uint64_t *bch = pr->batch_challenges.data(), *ff = pr->foldings_ff.data(), *fg1 = pr->foldings_fg1.data(), *fg2 = pr->foldings_fg2.data();
  // affine host records and canonical scalars; segments: comm_a, fg1 / comm_b, fg2
  std::vector<uint64_t> pts1(2 * K * 12, 0), pts2(2 * K * 24, 0), sc1(2 * K * 4), sc2(2 * K * 4);
  auto put1 = [&](size_t t, const uint64_t* jac, const gmh::Fr& e) {
    g1_to_host_record(jac, pts1.data() + 12 * t);
    e.to_canonical(sc1.data() + 4 * t);
  };
  auto put2 = [&](size_t t, const uint64_t* jac, const gmh::Fr& e) {
    g2_to_host_record(jac, pts2.data() + 24 * t);
    e.to_canonical(sc2.data() + 4 * t);
  };
  gmh::Fr ey = gmh::Fr::zero(), eff = gmh::Fr::zero();
  for (size_t i = 0; i < K; i++) {
    const gmh::Fr w0 = fr(bch + 4 * i), w1 = fr(bch + 4 * (K + i)), w2 = fr(bch + 4 * (2 * K + i));
    ey = ey + w0 * fr(y_mont + 4 * i);
    eff = eff + w0 * fr(ff + 8 * i) * fr(ff + 8 * i + 4);
    put1(i, comm_a + 18 * i, w1);
    put1(K + i, fg1 + 22 * i, w1 * fr(fg1 + 22 * i + 18));
    put2(i, comm_b + 36 * i, w2);
    put2(K + i, fg2 + 40 * i + 4, w2 * fr(fg2 + 40 * i));
  }
  const size_t offsets[3] = {0, K, 2 * K};
  uint64_t sum1[2 * 18], sum2[2 * 36];
  if ((rc = g1_lincomb_many_host(C, pts1.data(), 96, sc1.data(), offsets, 2, sum1))) return rc;
  if ((rc = g2_lincomb_many_host(C, pts2.data(), 192, sc2.data(), offsets, 2, sum2))) return rc;
  const Scalar unit = canonical(gmh::Fr::one());
  InitialTerms T;
  T.comm_a = gmh::G1::from_limbs(sum1);
  T.fg1 = gmh::G1::from_limbs(sum1 + 18);
  T.comm_b = gmh::G2::from_limbs(sum2);
  T.fg2 = gmh::G2::from_limbs(sum2 + 36);
  T.e_y = canonical(ey);
  T.e_ff = canonical(eff);
  T.e_comm_a = T.e_comm_b = T.e_fg1 = T.e_fg2 = unit;
  T.first = 3 * K;
  return ipa_verify_terms(C, pr, vrs, T, ok);
}

}  // namespace gm
