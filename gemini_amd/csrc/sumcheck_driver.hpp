// The Fiat-Shamir round loops of the sumcheck, Sumcheck::prove and Sumcheck::prove_batch (src/subprotocols/sumcheck/proof.rs:36-122),
// stated ONCE for every prover that lives on one device: the public gm_sumcheck_prove / gm_sumcheck_prove_batch (transcript.cpp),
// Sumcheck::new_time / new_elastic of the snark and psnark provers (prover_common.hpp) and the elastic psnark (psnark_elastic.cpp).
// The block-sharded provers have their loop in sumcheck_blocks.hpp.  Host C++ over the library's own C ABI.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/gemini_hip.h"
#include "host_field.hpp"

namespace gm {
void set_error(const char* fmt, ...);
}

namespace gmprover {

using gmh::Fr;

#define RC(x)            \
  do {                   \
    int rc_ = (x);       \
    if (rc_) return rc_; \
  } while (0)
// a failure of the loop itself: the text goes to gm_last_error
#define SC_CHECK(cond, code, ...)   \
  do {                              \
    if (!(cond)) {                  \
      ::gm::set_error(__VA_ARGS__); \
      return (code);                \
    }                               \
  } while (0)

inline const uint8_t* L(const char* s) { return reinterpret_cast<const uint8_t*>(s); }

constexpr size_t SPACE_TIME_THRESHOLD = 22;  // src/lib.rs:76

// `impl Prover for ElasticProver` (sumcheck/elastic_prover.rs:20-95): a space prover, a time prover, or a space prover that becomes a
// time prover once fewer than SPACE_TIME_THRESHOLD rounds remain.  next() is Prover::next_message in one call (Sumcheck::prove);
// begin() / end() are its two halves, so that prove_batch can enqueue the round of every live prover before it waits.
struct ElasticSc {
  uint64_t space = 0, time = 0;  // exactly one is in use: `space` until the switch (if ever), `time` after it
  bool allow_switch = true;  // false: Sumcheck::new_space, a SpaceProver to the end
  bool owned = true;         // false: `time` is the caller's handle (borrow)
  // round in flight
  bool pending_time = false, have_msg = false;
  uint64_t a[4], b[4];
  ElasticSc() = default;
  ElasticSc(const ElasticSc&) = delete;
  ElasticSc& operator=(const ElasticSc&) = delete;
  ~ElasticSc() { reset(); }
  void reset() {
    if (owned && time) (void)gm_sc_free(time);
    if (space) (void)gm_sp_free(space);
    time = space = 0;
  }
  int init(uint64_t f_stream, uint64_t g_stream, const uint64_t twist[4], bool elastic) {
    allow_switch = elastic;
    // no copy: the space prover reads the caller's streams until it is freed (every caller keeps them that long)
    return gm_sp_new_borrow(f_stream, g_stream, twist, &space);
  }
  // The RESIDENT schedule, and Sumcheck::new_time: the little-endian vectors are in HBM, so the prover is a time prover from its first
  // round (it reads them in place until its first fold) instead of a space prover that re-derives every message from the whole streams
  // until SPACE_TIME_THRESHOLD rounds remain.  The messages are the same field elements (sumcheck/tests.rs:42-87: space == time), and
  // it needs LESS memory than the reversed stream copies a device-side space prover reads (0.75 of them).
  int init_resident(uint64_t f_le, uint64_t g_le, const uint64_t twist[4]) {
    allow_switch = true;
    return gm_sc_new_borrow(f_le, g_le, twist, &time);
  }
  // a time prover the caller made and keeps (the gm_sc_* handles given to gm_sumcheck_prove / _prove_batch): never freed here
  void borrow(uint64_t time_handle) {
    reset();
    time = time_handle;
    owned = false;
  }
  int rounds(size_t* tot) const { return space ? gm_sp_rounds(space, tot, nullptr) : gm_sc_rounds(time, tot, nullptr); }
  // ElasticProver::fold (elastic_prover.rs:44-57) while the prover is a space prover: the challenge is consumed (a time prover folds
  // inside its round kernel instead)
  int fold_space(const uint64_t*& vm) {
    if (!vm || !space) return GM_OK;
    size_t tot = 0, rnd = 0;
    RC(gm_sp_rounds(space, &tot, &rnd));
    if (allow_switch && tot - rnd < SPACE_TIME_THRESHOLD) {
      RC(gm_sp_to_time(space, &time));
      RC(gm_sc_fold(time, vm));
      (void)gm_sp_free(space);
      space = 0;
    } else {
      RC(gm_sp_fold(space, vm));
    }
    vm = nullptr;
    return GM_OK;
  }
  // next_message(vm) of a lone prover: one fused call per round
  int next(const uint64_t* vm, uint64_t out_a[4], uint64_t out_b[4], int* has) {
    RC(fold_space(vm));
    return space ? gm_sp_round(space, vm, out_a, out_b, has) : gm_sc_round(time, vm, out_a, out_b, has);
  }
  // next_message(vm), first half: fold (switching to the time prover when it is time), launch the round
  int begin(const uint64_t* vm, int* has) {
    RC(fold_space(vm));
    if (space) {
      RC(gm_sp_round(space, nullptr, a, b, has));
      pending_time = false;
      have_msg = *has != 0;
    } else {
      RC(gm_sc_round_begin(time, vm, has));
      begun_as_time(*has);
    }
    return GM_OK;
  }
  // a prover that is a time prover already takes part in the ONE launch of its round (gm_sc_round_begin_many)
  bool is_time() const { return space == 0; }
  uint64_t time_handle() const { return time; }
  void begun_as_time(int has) {
    pending_time = has != 0;
    have_msg = false;
  }
  int end(uint64_t out_a[4], uint64_t out_b[4]) {
    if (pending_time) {
      pending_time = false;
      return gm_sc_round_end(time, out_a, out_b);
    }
    if (!have_msg) return GM_ESTATE;
    memcpy(out_a, a, 32);
    memcpy(out_b, b, 32);
    have_msg = false;
    return GM_OK;
  }
  int final(uint64_t f0[4], uint64_t g0[4], int* has) { return space ? gm_sp_final(space, f0, g0, has) : gm_sc_final(time, f0, g0, has); }
};

// Sumcheck::prove (proof.rs:36-66): message -> absorb b"evaluations" -> challenge b"challenge" -> next_message(Some(challenge)) ...,
// then the two b"final-folding" absorbs.  messages: cap_rounds x 8 u64 (a || b), challenges: cap_rounds x 4, final_foldings: 8 u64;
// *rounds_out = number of messages produced.
inline int prove(uint64_t transcript, ElasticSc& S, uint64_t* messages, uint64_t* challenges, size_t cap_rounds, uint64_t final_foldings[8],
                 size_t* rounds_out) {
  size_t k = 0;
  const uint64_t* vm = nullptr;
  for (;;) {
    uint64_t a[4], b[4];
    int has = 0;
    RC(S.next(vm, a, b, &has));
    if (!has) break;
    SC_CHECK(k < cap_rounds, GM_EINVAL, "sumcheck_prove: more than %zu rounds", cap_rounds);
    memcpy(messages + 8 * k, a, 32);
    memcpy(messages + 8 * k + 4, b, 32);
    RC(gm_transcript_append_fr(transcript, L("evaluations"), 11, messages + 8 * k, 2));
    RC(gm_transcript_challenge_fr(transcript, L("challenge"), 9, challenges + 4 * k));
    vm = challenges + 4 * k;
    k++;
  }
  int has = 0;
  RC(S.final(final_foldings, final_foldings + 4, &has));
  SC_CHECK(has, GM_ESTATE, "sumcheck_prove: final foldings unavailable");
  RC(gm_transcript_append_fr(transcript, L("final-folding"), 13, final_foldings, 1));
  RC(gm_transcript_append_fr(transcript, L("final-folding"), 13, final_foldings + 4, 1));
  *rounds_out = k;
  return GM_OK;
}
// the same with the challenges in a vector that ends up holding exactly the ones drawn
inline int prove(uint64_t transcript, ElasticSc& S, uint64_t* messages, std::vector<uint64_t>& challenges, size_t cap_rounds, uint64_t final_foldings[8],
                 size_t* rounds_out) {
  challenges.assign(cap_rounds * 4, 0);
  RC(prove(transcript, S, messages, challenges.data(), cap_rounds, final_foldings, rounds_out));
  challenges.resize(*rounds_out * 4);
  return GM_OK;
}

// Sumcheck::prove_batch (proof.rs:69-122): k provers of possibly different lengths run in lock-step for max(rounds) + 1 rounds; the
// coefficients c_j are drawn first (b"batch-sumcheck"); a prover that has run out contributes (f0 * g0, 0); the round message is
// sum_j c_j * m_j.  The reference maps its provers over rayon (:85); here the round of every live prover is enqueued before the first
// wait, the time provers among them in ONE launch (gm_sc_round_begin_many: k_sc_round_multi).  messages: cap_rounds x 8, challenges:
// cap_rounds x 4, final_foldings: k x 8 (lhs || rhs per prover).
inline int prove_batch(uint64_t transcript, ElasticSc* provers, size_t k, uint64_t* messages, uint64_t* challenges, size_t cap_rounds,
                       uint64_t* final_foldings, size_t* rounds_out) {
  size_t rounds = 0;
  for (size_t j = 0; j < k; j++) {
    size_t t = 0;
    RC(provers[j].rounds(&t));
    rounds = std::max(rounds, t);
  }
  rounds += 1;  // "+1 to get the final foldings" (:74)
  SC_CHECK(rounds <= cap_rounds, GM_EINVAL, "sumcheck_prove_batch: %zu rounds exceed capacity %zu", rounds, cap_rounds);
  std::vector<Fr> coeff(k), final_product(k);
  for (size_t j = 0; j < k; j++) {
    uint64_t c[4];
    RC(gm_transcript_challenge_fr(transcript, L("batch-sumcheck"), 14, c));
    coeff[j] = Fr::from_limbs(c);
  }
  // a prover that has run out contributes (f0 * g0, 0) in every later round: its final foldings are read once
  std::vector<char> finished(k, 0), has(k, 0);
  const uint64_t* vm = nullptr;
  for (size_t r = 0; r < rounds; r++) {
    Fr ma = Fr::zero(), mb = Fr::zero();
    {
      // the time provers among the live ones share one launch; a space prover (the literal elastic schedule) steps on its own
      std::vector<uint64_t> th;
      std::vector<size_t> at;
      for (size_t j = 0; j < k; j++) {
        if (finished[j]) continue;
        if (provers[j].is_time()) {
          th.push_back(provers[j].time_handle());
          at.push_back(j);
          continue;
        }
        int h = 0;
        RC(provers[j].begin(vm, &h));
        has[j] = (char)h;
      }
      std::vector<int> hs(th.size(), 0);
      RC(gm_sc_round_begin_many(th.data(), th.size(), vm, hs.data()));
      for (size_t t = 0; t < th.size(); t++) {
        provers[at[t]].begun_as_time(hs[t]);
        has[at[t]] = (char)hs[t];
      }
    }
    for (size_t j = 0; j < k; j++) {
      Fr fa, fb;
      if (!finished[j] && has[j]) {
        uint64_t a[4], b[4];
        RC(provers[j].end(a, b));
        fa = Fr::from_limbs(a);
        fb = Fr::from_limbs(b);
      } else {
        if (!finished[j]) {
          uint64_t f0[4], g0[4];
          int hf = 0;
          RC(provers[j].final(f0, g0, &hf));
          SC_CHECK(hf, GM_ESTATE, "If next_message is None, we expect final foldings to be available");
          final_product[j] = Fr::from_limbs(f0) * Fr::from_limbs(g0);
          finished[j] = 1;
        }
        fa = final_product[j];
        fb = Fr::zero();
      }
      ma = ma + fa * coeff[j];
      mb = mb + fb * coeff[j];
    }
    ma.to_limbs(messages + 8 * r);
    mb.to_limbs(messages + 8 * r + 4);
    RC(gm_transcript_append_fr(transcript, L("evaluations"), 11, messages + 8 * r, 2));
    RC(gm_transcript_challenge_fr(transcript, L("challenge"), 9, challenges + 4 * r));
    vm = challenges + 4 * r;
  }
  for (size_t j = 0; j < k; j++) {
    int hf = 0;
    RC(provers[j].final(final_foldings + 8 * j, final_foldings + 8 * j + 4, &hf));
    SC_CHECK(hf, GM_ESTATE, "sumcheck_prove_batch: final foldings unavailable for prover %zu", j);
    RC(gm_transcript_append_fr(transcript, L("final-folding-lhs"), 17, final_foldings + 8 * j, 1));
    RC(gm_transcript_append_fr(transcript, L("final-folding-rhs"), 17, final_foldings + 8 * j + 4, 1));
  }
  *rounds_out = rounds;
  return GM_OK;
}

}  // namespace gmprover
