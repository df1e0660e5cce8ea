// What the single-device provers (snark.cpp, psnark.cpp, psnark_elastic.cpp, subprotocols.cpp) share beyond the sumcheck driver:
//   * the two committer keys -- TimeKey = CommitterKey (src/kzg/time.rs:81-159), StreamKey = CommitterKeyStream (src/kzg/space.rs:95-285)
//     -- with one face: commit_many, commit_levels, open;
//   * TensorcheckProof::new_time (src/subprotocols/tensorcheck/mod.rs:190-275) and its streaming twin (snark/elastic_prover.rs:105-168,
//     psnark/elastic_prover.rs:384-600), stated ONCE over either key: the two differ in how the levels and the final quotient are
//     committed, and both are properties of the key;
//   * the claim block of EntryProduct::new_time_batch / new_elastic_batch (entryproduct/time_prover.rs:79-102), over either key.
// Pure orchestration over the library's own C ABI.  The block-sharded provers (sharded.cpp, psnark_sharded.cpp) keep tensor checks of
// their own: levels sharded by blocks and an opening per coefficient range are another algorithm.
#pragma once
#include <algorithm>

#include "prover_common.hpp"

namespace gmprover {

// (sum_i chal^i p_i) div prod_j (x - pts[j]) as a new vector of V: what either key commits to when it opens
// (batch_open_multi_points, src/kzg/time.rs:149-159; open / open_multi_points / open_folding, src/kzg/space.rs:95-166,229-285)
inline int open_quotient(Vecs& V, const std::vector<uint64_t>& polys, const uint64_t* pts, size_t npts, const uint64_t chal[4], uint64_t* quotient) {
  std::vector<uint64_t> etas(4 * polys.size());
  Fr acc = Fr::one();
  const Fr c = Fr::from_limbs(chal);
  size_t longest = 0;
  for (size_t k = 0; k < polys.size(); k++) {
    acc.to_limbs(etas.data() + 4 * k);
    acc = acc * c;
    size_t l = 0;
    RC(vec_len(polys[k], &l));
    longest = std::max(longest, l);
  }
  uint64_t combined;
  RC(V.alloc(longest, &combined));
  RC(gm_fr_lincomb(polys.data(), etas.data(), polys.size(), combined));
  size_t lc = 0;
  RC(vec_len(combined, &lc));
  RC(V.alloc(lc ? lc - 1 : 0, quotient));
  uint64_t rem[4 * 8];
  RC(gm_fr_div_vanishing(combined, pts, npts, *quotient, rem));  // no longer than the point set: the empty quotient
  V.release(combined);
  return GM_OK;
}

// CommitterKey: the powers in time order, every vector little-endian
struct TimeKey {
  uint64_t ck;
  size_t nck;
  // ck.commit(v): msm_unchecked truncates to the shorter side (src/kzg/time.rs:82)
  int commit(Vecs&, uint64_t v, uint64_t out[18]) const {
    size_t n = 0;
    RC(vec_len(v, &n));
    return gm_ck_msm(ck, 0, 0, v, 0, std::min(n, nck), out);
  }
  int commit_many(Vecs&, const std::vector<uint64_t>& vs, uint64_t* out) const {  // batch_commit :98-107
    std::vector<size_t> ns(vs.size());
    for (size_t k = 0; k < vs.size(); k++) {
      RC(vec_len(vs[k], &ns[k]));
      ns[k] = std::min(ns[k], nck);
    }
    return gm_ck_msm_batch(ck, vs.data(), ns.data(), vs.size(), out);
  }
  // the levels of every folded tree: ONE batch, whatever the depths   tensorcheck/mod.rs:218
  int commit_levels(Vecs& V, const std::vector<uint64_t>& levels, const std::vector<size_t>&, uint64_t* out) const { return commit_many(V, levels, out); }
  int open(Vecs& V, const std::vector<uint64_t>& polys, const uint64_t* pts, size_t npts, const uint64_t chal[4], uint64_t out[18]) const {
    uint64_t q;
    RC(open_quotient(V, polys, pts, npts, chal, &q));
    const int rc = commit(V, q, out);
    V.release(q);
    return rc;
  }
};

// CommitterKeyStream: the same powers walked as Reverse(powers_of_g) + advance_by against a big-endian stream, which is the reversed /
// offset addressing of gm_ck_msm.  A ChunkedPippenger flushes every max(wanted, min_chunk) pairs: max_msm_buffer bounds HOST buffering
// in the reference, and a flush shorter than min_chunk pairs is merged into one device MSM.  The vectors arrive little-endian.
struct StreamKey {
  uint64_t ck;
  size_t nck, max_msm_buffer, min_chunk;
  size_t flush(size_t wanted) const { return std::max<size_t>(std::max<size_t>(wanted, 1), min_chunk); }
  // the vector is reversed into its stream and walked against the key; nothing to walk is the identity
  int msm_le(Vecs& V, uint64_t le, size_t wanted_flush, uint64_t out[18]) const {
    size_t n = 0;
    RC(vec_len(le, &n));
    SC_CHECK(n <= nck, GM_EINVAL, "stream key: a stream of %zu elements, a key of %zu", n, nck);  // space.rs:169-175
    if (n == 0) return gm_g1_sum(nullptr, 0, out);
    uint64_t s;
    RC(V.alloc(n, &s));
    RC(gm_fr_reverse(le, s));
    const int rc = stream_msm(ck, s, n, n - 1, flush(wanted_flush), out);
    V.release(s);
    return rc;
  }
  // several commitments: when no vector is cut by the flush size they are sum_i v[i] tau^i g whichever way the pairs are walked
  // -- one pipelined batch; otherwise stream by stream
  int commit_flushed(Vecs& V, const std::vector<uint64_t>& les, size_t wanted_flush, uint64_t* out) const {
    bool cut = false;
    std::vector<size_t> ns(les.size());
    for (size_t k = 0; k < les.size(); k++) {
      RC(vec_len(les[k], &ns[k]));
      SC_CHECK(ns[k] <= nck, GM_EINVAL, "stream key: a stream of %zu elements, a key of %zu", ns[k], nck);
      cut = cut || ns[k] > flush(wanted_flush);
    }
    if (!cut) return gm_ck_msm_batch(ck, les.data(), ns.data(), les.size(), out);
    for (size_t k = 0; k < les.size(); k++) RC(msm_le(V, les[k], wanted_flush, out + 18 * k));
    return GM_OK;
  }
  // ck.commit(stream) of each: msm_chunks of 2^20 (space.rs:169-177)
  int commit_many(Vecs& V, const std::vector<uint64_t>& les, uint64_t* out) const { return commit_flushed(V, les, (size_t)1 << 20, out); }
  // commit_folding (space.rs:192-223): one ChunkedPippenger of max_msm_buffer / depth per level of a tree.  When no level of any tree is
  // cut by its flush size the levels of all trees go through ONE pipelined batch; otherwise tree by tree, level by level, as streams
  int commit_levels(Vecs& V, const std::vector<uint64_t>& levels, const std::vector<size_t>& depths, uint64_t* out) const {
    bool cut = false;
    size_t at = 0;
    for (size_t depth : depths)
      for (size_t k = 0; k < depth; k++, at++) {
        size_t l = 0;
        RC(vec_len(levels[at], &l));
        cut = cut || l > flush(max_msm_buffer / depth);
      }
    if (!cut) return commit_flushed(V, levels, (size_t)1 << 62, out);
    at = 0;
    for (size_t depth : depths) {
      RC(commit_flushed(V, std::vector<uint64_t>(levels.begin() + at, levels.begin() + at + depth), max_msm_buffer / depth, out + 18 * at));
      at += depth;
    }
    return GM_OK;
  }
  // The reference sums its openings -- open (space.rs:95-125) or open_multi_points (:128-166) of the combined base polynomials and one
  // open_folding per tree (:229-285) -- each sum_i eta_i commit(p_i div Z), the HashMapPippenger of open_folding merging the scalars of
  // equal bases.  Division by the same Z is linear and all of them walk the same key, so the merge extends over all of them: ONE linear
  // combination, ONE division (instead of a latency-bound three-phase scan per level), one stream MSM flushed every max_msm_buffer
  // pairs.  It is the polynomial the time key opens.
  int open(Vecs& V, const std::vector<uint64_t>& polys, const uint64_t* pts, size_t npts, const uint64_t chal[4], uint64_t out[18]) const {
    uint64_t q;
    RC(open_quotient(V, polys, pts, npts, chal, &q));
    const int rc = msm_le(V, q, max_msm_buffer, out);
    V.release(q);
    return rc;
  }
};

// TensorcheckProof::new_time(transcript, ck, base_polys, bodies)   tensorcheck/mod.rs:190-275
// `spent`: vectors of the caller's V that nothing reads once the bodies are batched; they go there, before the levels are allocated.
// Each batched body goes as soon as its tree is folded.  Out: fold_commitments (cap_folds x 18), base_evaluations (|base| x 12: at
// beta^2, beta, -beta), fold_evaluations (cap_folds x 8: at beta, -beta), the opening and the number of foldings.
template <class Key>
int tensorcheck(const Key& K, uint64_t transcript, Vecs& V, const std::vector<uint64_t>& base, const std::vector<gm_tensorcheck_body>& bodies,
                const std::vector<uint64_t>& spent, size_t cap_folds, uint64_t* fold_commitments, uint64_t* base_evaluations, uint64_t* fold_evaluations,
                uint64_t evaluation_proof[18], size_t* nfold_out) {
  const size_t nbodies = bodies.size(), nbase = base.size();
  size_t max_group = 0, nfold = 0;
  for (const gm_tensorcheck_body& B : bodies) {
    max_group = std::max(max_group, B.npolys);
    nfold += B.nchallenges ? B.nchallenges - 1 : 0;
  }
  SC_CHECK(nfold <= cap_folds, GM_EINVAL, "tensorcheck: %zu foldings, room for %zu", nfold, cap_folds);
  uint64_t batch_challenge[4];
  RC(gm_transcript_challenge_fr(transcript, L("batch_challenge"), 15, batch_challenge));  // :201
  std::vector<uint64_t> bc(4 * max_group);  // powers(batch_challenge, max_len)   :202
  {
    Fr acc = Fr::one();
    const Fr c = Fr::from_limbs(batch_challenge);
    for (size_t k = 0; k < max_group; k++) {
      acc.to_limbs(bc.data() + 4 * k);
      acc = acc * c;
    }
  }
  std::vector<uint64_t> batched(nbodies);  // :208-217
  for (size_t b = 0; b < nbodies; b++) {
    const gm_tensorcheck_body& B = bodies[b];
    if (B.nchallenges < 2) continue;  // no folding: the batched polynomial is not needed
    batched[b] = B.polys[0];
    if (B.npolys == 1) continue;  // one polynomial, coefficient 1: it is its own batched polynomial
    size_t longest = 0;
    for (size_t k = 0; k < B.npolys; k++) {
      size_t l = 0;
      RC(vec_len(B.polys[k], &l));
      longest = std::max(longest, l);
    }
    RC(V.alloc(longest, &batched[b]));
    RC(gm_fr_lincomb(B.polys, bc.data(), B.npolys, batched[b]));
  }
  for (uint64_t v : spent)
    if (std::find(batched.begin(), batched.end(), v) == batched.end()) V.release(v);
  std::vector<uint64_t> foldings;
  std::vector<size_t> depths;  // of the trees that fold
  for (size_t b = 0; b < nbodies; b++) {
    const gm_tensorcheck_body& B = bodies[b];
    if (B.nchallenges < 2) continue;
    size_t len = 0;
    RC(vec_len(batched[b], &len));
    const size_t first_level = foldings.size();
    for (size_t k = 0; k + 1 < B.nchallenges; k++) {  // foldings_polynomial: all challenges but the last   :124-133
      uint64_t nxt;
      len = (len + 1) / 2;
      RC(V.alloc(len, &nxt));
      foldings.push_back(nxt);
    }
    depths.push_back(B.nchallenges - 1);
    RC(gm_fr_fold_chain(batched[b], B.challenges_mont, B.nchallenges - 1, foldings.data() + first_level));  // one wait for the whole tree
    if (B.npolys > 1) V.release(batched[b]);
  }
  *nfold_out = nfold;
  if (nfold) RC(K.commit_levels(V, foldings, depths, fold_commitments));  // :218
  for (size_t k = 0; k < nfold; k++) RC(gm_transcript_append_g1(transcript, L("commitment"), 10, fold_commitments + 18 * k, 1, 0));
  uint64_t pts[12];  // beta^2, beta, -beta   :224-226
  RC(gm_transcript_challenge_fr(transcript, L("evaluation-chal"), 15, pts + 4));
  {
    const Fr beta = Fr::from_limbs(pts + 4);
    beta.sqr().to_limbs(pts);
    beta.neg().to_limbs(pts + 8);
  }
  if (nbase) RC(gm_fr_eval_le_batch(base.data(), nbase, pts, 3, base_evaluations));           // :228-237
  if (nfold) RC(gm_fr_eval_le_batch(foldings.data(), nfold, pts + 4, 2, fold_evaluations));  // :239-247, one wait for all levels
  for (size_t k = 0; k < 3 * nbase; k++) RC(gm_transcript_append_fr(transcript, L("eval"), 4, base_evaluations + 4 * k, 1));
  for (size_t k = 0; k < 2 * nfold; k++) RC(gm_transcript_append_fr(transcript, L("eval"), 4, fold_evaluations + 4 * k, 1));
  uint64_t open_chal[4];
  RC(gm_transcript_challenge_fr(transcript, L("open-chal"), 9, open_chal));  // :261
  std::vector<uint64_t> all = base;
  all.insert(all.end(), foldings.begin(), foldings.end());
  return K.open(V, all, pts, 3, open_chal, evaluation_proof);  // :263-267
}

// The tensor check of the preprocessing SNARK (psnark/time_prover.rs:296-367, elastic_prover.rs:384-600), for either prover: 22 base
// polynomials and 4 bodies.  w, the four looked-up vectors {ralpha*, r*, alpha*, z*}, the sorted vectors, the accumulated products and
// the right rotations are little-endian; the right rotations are last read when the second body is batched and go there.
template <class Key>
int psnark_tensorcheck(const Key& K, uint64_t transcript, Vecs& V, const gm_psnark_instance* I, uint64_t w, const uint64_t star[4], const uint64_t sorted[3],
                       const std::vector<uint64_t>& acc, const std::vector<uint64_t>& shifts, const uint64_t psi[4], const std::vector<uint64_t>& ch2,
                       const std::vector<uint64_t>& ch3, gm_psnark_proof* P) {
  std::vector<uint64_t> base = {w, star[0], star[1], star[2], star[3], I->row, I->col, I->val_a, I->val_b, I->val_c, sorted[0], sorted[1], sorted[2]};
  base.insert(base.end(), acc.begin(), acc.end());
  const size_t n3 = P->rounds[2], n2 = P->rounds[1];
  std::vector<uint64_t> polys0 = acc, polys1 = shifts, ch0(4 * n3), ch3h(4 * std::min(n2, n3));
  polys0.push_back(star[1]);  // accumulated_vec + [r_star], challenges third_ch[j] * psi^(2^j)   time_prover.rs:334-349
  Fr tw = Fr::from_limbs(psi);
  for (size_t j = 0; j < n3; j++) {
    (Fr::from_limbs(ch3.data() + 4 * j) * tw).to_limbs(ch0.data() + 4 * j);
    tw = tw.sqr();
  }
  polys1.insert(polys1.end(), {I->val_a, I->val_b, I->val_c, star[2]});  // shift_monic_lookup_vec + [val_a, val_b, val_c, alpha_star], challenges third_ch
  for (size_t j = 0; j < ch3h.size() / 4; j++) (Fr::from_limbs(ch2.data() + 4 * j) * Fr::from_limbs(ch3.data() + 4 * j)).to_limbs(ch3h.data() + 4 * j);
  const std::vector<gm_tensorcheck_body> bodies = {{polys0.data(), polys0.size(), ch0.data(), n3},
                                                   {polys1.data(), polys1.size(), ch3.data(), n3},
                                                   {star + 3, 1, ch2.data(), n2},                  // [z_star], challenges second_ch
                                                   {star, 3, ch3h.data(), ch3h.size() / 4}};       // [ralpha_star, r_star, alpha_star], second_ch[j] * third_ch[j]
  return tensorcheck(K, transcript, V, base, bodies, shifts, P->cap_folds, P->fold_commitments, &P->base_evaluations[0][0], P->fold_evaluations,
                     P->evaluation_proof, &P->nfold);
}

// The claims of EntryProduct::new_time_batch (entryproduct/time_prover.rs:79-102; elastic_prover.rs:66-127 over streams): commit the
// accumulated vectors, draw the challenge, claimed_sumchecks[i] = chal * acc_i(chal) + product_i - chal^|acc_i|.  How the sumcheck
// provers over (acc_i, right rotation, chal) are made is the caller's: copies, borrowed vectors or streams.
template <class Key>
int entry_product_claims(const Key& K, uint64_t transcript, Vecs& V, const std::vector<uint64_t>& acc, const uint64_t* products_mont,
                         uint64_t* acc_v_commitments, uint64_t chal_mont[4], uint64_t* claimed_sumchecks_mont) {
  const size_t k = acc.size();
  if (k) RC(K.commit_many(V, acc, acc_v_commitments));  // :79 (:128 for one vector)
  for (size_t i = 0; i < k; i++) RC(gm_transcript_append_g1(transcript, L("acc_v"), 5, acc_v_commitments + 18 * i, 1, 0));
  RC(gm_transcript_challenge_fr(transcript, L("ep-chal"), 7, chal_mont));  // :84
  if (k == 0) return GM_OK;
  std::vector<uint64_t> acc_chal(4 * k);
  RC(gm_fr_eval_le_batch(acc.data(), k, chal_mont, 1, acc_chal.data()));  // evaluate_be of the streams
  const Fr c = Fr::from_limbs(chal_mont);
  for (size_t i = 0; i < k; i++) {  // :94-102
    size_t l = 0;
    RC(vec_len(acc[i], &l));
    (Fr::from_limbs(acc_chal.data() + 4 * i) * c + Fr::from_limbs(products_mont + 4 * i) - fr_pow(c, l)).to_limbs(claimed_sumchecks_mont + 4 * i);
  }
  return GM_OK;
}

}  // namespace gmprover
