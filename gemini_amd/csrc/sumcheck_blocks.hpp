// Sumcheck::prove / prove_batch (src/subprotocols/sumcheck/proof.rs:36-122) over BLOCK-SHARDED provers, one process per GPU over the
// all-gather of gm_dist: the one round loop of gm_sumcheck_prove_sharded (sharded.cpp) and of the sharded psnark (psnark_sharded.cpp).
// The provers of one device have theirs in sumcheck_driver.hpp.  Host C++ over the library's own C ABI.
#pragma once
#include <algorithm>
#include <vector>

#include "prover_common.hpp"

namespace gmprover {

inline size_t ceil_log2(size_t n) {
  size_t b = 0;
  while (((size_t)1 << b) < n) b++;
  return b;
}
inline size_t ceil_shift(size_t n, size_t k) { return k >= 63 ? (n ? 1 : 0) : (n + (((size_t)1 << k) - 1)) >> k; }

struct Sh {  // this rank's view of the block layout
  size_t r = 0, g = 1, M = 0, jmax = 0;
  size_t B(size_t s) const { return M >> s; }
  size_t lo(size_t s) const { return r * (M >> s); }
  size_t cnt(size_t len, size_t s) const { return len > lo(s) ? std::min(B(s), len - lo(s)) : 0; }
  // the level of a family whose longest member has `len` elements: the finest blocks, still foldable, whose g copies hold it
  size_t level(size_t len) const {
    size_t s = 0;
    while (s < jmax && g * (M >> (s + 1)) >= len) s++;
    return s;
  }
};

inline int blk_len(uint64_t v, size_t* n) {
  *n = 0;
  return v ? vec_len(v, n) : GM_OK;
}

// ---- Sumcheck::prove / prove_batch over blocks ---------------------------------------------------------------------------
// (src/subprotocols/sumcheck/proof.rs:36-122) k provers whose vectors are block-sharded, each at its own level.  While a prover's blocks
// hold more than `tail` elements and stay pair-aligned, its rounds are shard-local: the partial messages of ALL sharded provers -- 64 bytes
// each -- are all-gathered in ONE call per round and added mod r.  A prover whose blocks get short is gathered once (one all-gather for all
// the provers that switch in that round) and finished replicated on the whole (short) vectors.  batch = false: Sumcheck::prove of ONE
// prover (labels and round count differ).
struct ShProver {
  uint64_t f = 0, g = 0;  // this rank's blocks (length 0: nothing of the vectors falls into the block)
  const uint64_t* twist = nullptr;
  size_t len = 0;  // of the whole vectors
  size_t s = 0;    // their level
};
struct ProverSet {
  std::vector<uint64_t> h;
  ~ProverSet() {
    for (uint64_t p : h)
      if (p) (void)gm_sc_free(p);
  }
};

inline int sumcheck_blocks(const Sh& lay, uint64_t transcript, bool batch, const std::vector<ShProver>& P, size_t tail, uint64_t* messages, uint64_t* challenges,
                           size_t cap_rounds, uint64_t* final_foldings, size_t* rounds_out) {
  const size_t k = P.size();
  if (k == 0 || (!batch && k != 1)) return GM_EINVAL;
  std::vector<size_t> tot(k);
  size_t max_tot = 0;
  for (size_t j = 0; j < k; j++) {
    tot[j] = ceil_log2(P[j].len);  // time_prover.rs:35-38
    max_tot = std::max(max_tot, tot[j]);
  }
  const size_t rounds = batch ? max_tot + 1 : max_tot;  // "+1 to get the final foldings" (proof.rs:74)
  if (rounds > cap_rounds) return GM_EINVAL;
  std::vector<Fr> coeff(k, Fr::one());
  if (batch)
    for (size_t j = 0; j < k; j++) {
      uint64_t c[4];
      RC(gm_transcript_challenge_fr(transcript, L("batch-sumcheck"), 14, c));
      coeff[j] = Fr::from_limbs(c);
    }
  ProverSet S;
  S.h.assign(k, 0);
  std::vector<size_t> Mc(k);       // current block size of a sharded prover
  std::vector<char> rep(k, 0);     // finished its sharded phase: S.h[j] is a replicated prover over the whole vectors
  for (size_t j = 0; j < k; j++) {
    size_t nf = 0, ng = 0;
    RC(blk_len(P[j].f, &nf));
    RC(blk_len(P[j].g, &ng));
    Mc[j] = lay.B(P[j].s);
    if (lay.g == 1) {
      if (!nf || !ng) return GM_EINVAL;  // "sumcheck: empty vectors"
      RC(gm_sc_new_borrow(P[j].f, P[j].g, P[j].twist, &S.h[j]));
      rep[j] = 1;
      continue;
    }
    if (nf != lay.cnt(P[j].len, P[j].s) || ng != nf) return GM_EINVAL;  // the blocks of a sharded prover tile its vectors
    if (nf) {
      RC(gm_sc_new_borrow(P[j].f, P[j].g, P[j].twist, &S.h[j]));
      RC(gm_sc_set_shard_rounds(S.h[j], lay.lo(P[j].s) / 2, tot[j]));
    }
  }
  size_t rd = 0;  // messages sent so far = folds applied once the pending challenge is in
  const uint64_t* vm = nullptr;
  std::vector<Fr> final_product(k);
  std::vector<char> finished(k, 0);
  for (;;) {
    // provers that leave their sharded phase now: the pending fold is applied shard-locally, then the blocks are gathered -- the
    // replicated prover starts exactly at a message boundary (and must not fold again in this round)
    std::vector<size_t> sw;
    for (size_t j = 0; j < k; j++)
      if (!rep[j] && !(Mc[j] % 4 == 0 && Mc[j] > tail && rd < tot[j])) sw.push_back(j);
    std::vector<char> folded(k, 0);
    if (!sw.empty()) {
      size_t slots = 0;
      std::vector<size_t> off(sw.size()), bs(sw.size());
      for (size_t i = 0; i < sw.size(); i++) {
        const size_t j = sw[i];
        if (vm) {
          if (S.h[j]) RC(gm_sc_fold(S.h[j], vm));
          Mc[j] /= 2;
          folded[j] = 1;
        }
        bs[i] = Mc[j];
        off[i] = slots;
        slots += 4 + 8 * bs[i];  // [count | f | g], limbs
      }
      std::vector<uint64_t> mine(slots, 0), all(slots * lay.g);
      for (size_t i = 0; i < sw.size(); i++) {
        const size_t j = sw[i];
        if (!S.h[j]) continue;
        size_t nf = 0, ng = 0;
        RC(gm_sc_lens(S.h[j], &nf, &ng, nullptr));
        if (nf != ng || nf > bs[i]) return GM_ESTATE;
        mine[off[i]] = nf;
        RC(gm_sc_download(S.h[j], mine.data() + off[i] + 4, mine.data() + off[i] + 4 + 4 * bs[i]));
      }
      RC(gm_dist_allgather_host(mine.data(), 8 * slots, all.data()));
      const size_t folds = rd;  // (with the pending challenge applied)
      for (size_t i = 0; i < sw.size(); i++) {
        const size_t j = sw[i];
        std::vector<uint64_t> fs, gs;
        for (size_t rr = 0; rr < lay.g; rr++) {
          const uint64_t* sl = all.data() + slots * rr + off[i];
          const size_t c = (size_t)sl[0];
          if (c > bs[i]) return GM_ESTATE;
          fs.insert(fs.end(), sl + 4, sl + 4 + 4 * c);
          gs.insert(gs.end(), sl + 4 + 4 * bs[i], sl + 4 + 4 * bs[i] + 4 * c);
        }
        const size_t n = fs.size() / 4;
        if (n != ceil_shift(P[j].len, folds)) return GM_ESTATE;  // the blocks tile the folded vectors
        Fr tw = Fr::from_limbs(P[j].twist);
        for (size_t t = 0; t < folds; t++) tw = tw.sqr();
        uint64_t twl[4];
        tw.to_limbs(twl);
        if (S.h[j]) (void)gm_sc_free(S.h[j]);
        S.h[j] = 0;
        RC(gm_sc_new(fs.data(), n, gs.data(), n, twl, &S.h[j]));
        rep[j] = 1;
      }
    }
    if (batch && rd == rounds) break;
    bool any_sharded = false;
    for (size_t j = 0; j < k; j++) any_sharded = any_sharded || !rep[j];
    std::vector<char> has(k, 0);
    for (int pass = 0; pass < 2; pass++) {
      // one launch for the provers that fold with the pending challenge, one for those whose fold went into their gathering
      std::vector<uint64_t> hs;
      std::vector<size_t> at;
      for (size_t j = 0; j < k; j++)
        if (S.h[j] && !finished[j] && (folded[j] != 0) == (pass == 1)) {
          hs.push_back(S.h[j]);
          at.push_back(j);
        }
      if (hs.empty()) continue;
      std::vector<int> flags(hs.size(), 0);
      RC(gm_sc_round_begin_many(hs.data(), hs.size(), pass == 1 ? nullptr : vm, flags.data()));
      for (size_t t = 0; t < hs.size(); t++) has[at[t]] = (char)flags[t];
    }
    std::vector<uint64_t> part(8 * k, 0);
    bool any = any_sharded;  // (a sharded prover has a message in this round -- rd < tot -- on some rank)
    for (size_t j = 0; j < k; j++) {
      if (S.h[j] && !finished[j] && has[j]) {
        RC(gm_sc_round_end(S.h[j], part.data() + 8 * j, part.data() + 8 * j + 4));
        any = true;
      } else if (rep[j]) {
        if (!batch) continue;  // Sumcheck::prove: no message means the protocol is over
        if (!finished[j]) {
          uint64_t f0[4], g0[4];
          int hf = 0;
          RC(gm_sc_final(S.h[j], f0, g0, &hf));
          if (!hf) return GM_ESTATE;  // "If next_message is None, we expect final foldings to be available"
          final_product[j] = Fr::from_limbs(f0) * Fr::from_limbs(g0);
          finished[j] = 1;
        }
        final_product[j].to_limbs(part.data() + 8 * j);
      }
    }
    if (any_sharded) {
      // ONE all-gather per round for all the provers still in their sharded phase (a replicated prover's slot carries zeros)
      std::vector<uint64_t> mine(8 * k, 0), all(8 * k * lay.g);
      for (size_t j = 0; j < k; j++)
        if (!rep[j]) memcpy(mine.data() + 8 * j, part.data() + 8 * j, 64);
      RC(gm_dist_allgather_host(mine.data(), 64 * k, all.data()));
      for (size_t j = 0; j < k; j++) {
        if (rep[j]) continue;
        Fr sa = Fr::zero(), sb = Fr::zero();
        for (size_t rr = 0; rr < lay.g; rr++) {
          sa = sa + Fr::from_limbs(all.data() + 8 * (rr * k + j));
          sb = sb + Fr::from_limbs(all.data() + 8 * (rr * k + j) + 4);
        }
        sa.to_limbs(part.data() + 8 * j);
        sb.to_limbs(part.data() + 8 * j + 4);
      }
    }
    if (vm)
      for (size_t j = 0; j < k; j++)
        if (!rep[j]) Mc[j] /= 2;
    if (!batch && !any) break;
    if (rd >= cap_rounds) return GM_EINVAL;
    Fr ma = Fr::zero(), mb = Fr::zero();
    for (size_t j = 0; j < k; j++) {
      ma = ma + Fr::from_limbs(part.data() + 8 * j) * coeff[j];
      mb = mb + Fr::from_limbs(part.data() + 8 * j + 4) * coeff[j];
    }
    ma.to_limbs(messages + 8 * rd);
    mb.to_limbs(messages + 8 * rd + 4);
    RC(gm_transcript_append_fr(transcript, L("evaluations"), 11, messages + 8 * rd, 2));
    RC(gm_transcript_challenge_fr(transcript, L("challenge"), 9, challenges + 4 * rd));
    vm = challenges + 4 * rd;
    rd++;
  }
  for (size_t j = 0; j < k; j++) {
    int has = 0;
    RC(gm_sc_final(S.h[j], final_foldings + 8 * j, final_foldings + 8 * j + 4, &has));
    if (!has) return GM_ESTATE;
    if (batch) {
      RC(gm_transcript_append_fr(transcript, L("final-folding-lhs"), 17, final_foldings + 8 * j, 1));
      RC(gm_transcript_append_fr(transcript, L("final-folding-rhs"), 17, final_foldings + 8 * j + 4, 1));
    } else {
      RC(gm_transcript_append_fr(transcript, L("final-folding"), 13, final_foldings + 8 * j, 1));
      RC(gm_transcript_append_fr(transcript, L("final-folding"), 13, final_foldings + 8 * j + 4, 1));
    }
  }
  *rounds_out = rd;
  return GM_OK;
}

}  // namespace gmprover
