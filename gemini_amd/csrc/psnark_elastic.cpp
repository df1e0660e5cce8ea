// psnark::Proof::new_elastic (src/psnark/elastic_prover.rs:60-634) as ONE entry point of the library: the preprocessing SNARK over
// device-resident STREAMS (big-endian reversed vectors), with
//   * CommitterKeyStream::{commit, open, open_multi_points, commit_folding, open_folding} (src/kzg/space.rs:95-285) as the StreamKey
//     of tensorcheck.hpp: chunked stream MSMs, a flush every max(max_msm_buffer [/ depth], min_device_chunk) pairs;
//   * Sumcheck::{new_space, new_elastic} (sumcheck/proof.rs:133-154) and prove_batch (:69-122) over ElasticProvers: a SpaceProver
//     that becomes a TimeProver once fewer than SPACE_TIME_THRESHOLD rounds remain (elastic_prover.rs:44-57) -- the prover adapter
//     and both round loops are those of sumcheck_driver.hpp;
//   * EntryProduct::new_elastic_batch (entryproduct/elastic_prover.rs:66-127), the plookup streams (:227-232 of the prover) and the
//     tensor check over FoldedPolynomialTrees (:384-600): the claims and the tensorcheck of tensorcheck.hpp, over the StreamKey.
// Same transcript, same bytes as gm_psnark_new_time (src/psnark/tests.rs:56-124 asserts time == elastic); the sequence is the one
// of gemini_amd/psnark.py::Proof.new_elastic, which the tests hold byte for byte equal to this.  Pure orchestration over the
// library's own C ABI, like snark.cpp / psnark.cpp.  The reference re-streams every vector from its source to stay in O(log n)
// memory; with the streams resident in HBM they are materialised once.
#include "tensorcheck.hpp"

namespace {

using namespace gmprover;

int reversed(Vecs& V, uint64_t v, uint64_t* out) {
  size_t n = 0;
  RC(vec_len(v, &n));
  RC(V.alloc(n, out));
  return gm_fr_reverse(v, *out);
}

}  // namespace

extern "C" int gm_psnark_new_elastic(const gm_psnark_instance* I, uint64_t z_stream, uint64_t w_stream, uint64_t za_stream, uint64_t zb_stream,
                                     uint64_t zc_stream, uint64_t ck_bases, size_t max_msm_buffer, size_t min_device_chunk, int g1_encoding,
                                     size_t cap_rounds, gm_psnark_proof* P) {
  if (!I || !P || !I->index_commitments || !P->messages[0] || !P->messages[1] || !P->messages[2] || !P->fold_commitments || !P->fold_evaluations)
    return GM_EINVAL;
  const auto t_all = Clock::now();
  Vecs V;
  StreamKey K{ck_bases, 0, max_msm_buffer, min_device_chunk};
  RC(gm_ck_len(ck_bases, &K.nck));
  size_t nz = 0;
  RC(vec_len(z_stream, &nz));
  const size_t nnz = I->nnz;
  RC(gm_footprint_admit(1, ck_bases, nz, nnz, min_device_chunk > 1 ? 1 : 2));
  uint64_t one[4];
  Fr::one().to_limbs(one);
  TranscriptGuard T;
  static const char protocol[] = "GEMINI-v0";
  RC(gm_transcript_new(L(protocol), sizeof protocol - 1, &T.h));
  if (g1_encoding) RC(gm_transcript_set_g1_encoding(T.h, g1_encoding));

  auto t0 = Clock::now();
  {
    size_t nw = 0;
    RC(vec_len(w_stream, &nw));
    if (nw > K.nck) return GM_EINVAL;
    RC(stream_msm(ck_bases, w_stream, nw, nw ? nw - 1 : 0, K.flush((size_t)1 << 20), P->witness_commitment));  // :82
  }
  P->spans[0] = since(t0);
  RC(gm_transcript_append_g1(T.h, L("witness"), 7, P->witness_commitment, 1, 0));  // :86-89
  RC(gm_transcript_append_message(T.h, L("ck"), 2, I->ck_g2_bytes, I->ck_g2_len));
  RC(gm_transcript_append_g1(T.h, L("instance"), 8, I->index_commitments, 5, 1));
  uint64_t alpha[4];
  RC(gm_transcript_challenge_fr(T.h, L("alpha"), 5, alpha));
  {
    uint64_t zc_le;
    RC(reversed(V, zc_stream, &zc_le));
    RC(gm_fr_eval_le(zc_le, alpha, 1, P->zc_alpha));  // evaluate_be(z_c, alpha) :92-93
    V.release(zc_le);
  }
  RC(gm_transcript_append_fr(T.h, L("zc(alpha)"), 9, P->zc_alpha, 1));

  // min_device_chunk > 1 (the default, 2^26): the embedder lets the device merge flushes, i.e. treats max_msm_buffer as advisory
  // because everything is resident -- then the sumchecks take the resident schedule too (ElasticSc::init_resident).  min_device_chunk
  // = 1 is the LITERAL elastic prover: 2^20-pair flushes, space provers until SPACE_TIME_THRESHOLD rounds remain.
  const bool resident = min_device_chunk > 1;
  t0 = Clock::now();
  std::vector<uint64_t> ch1, ch2;
  if (resident) {
    uint64_t za_le, zb_le;
    RC(reversed(V, za_stream, &za_le));
    RC(reversed(V, zb_stream, &zb_le));
    RC(sumcheck_new_time(T.h, za_le, zb_le, alpha, P->messages[0], ch1, cap_rounds, P->final_foldings[0], &P->rounds[0]));
    V.release(za_le);
    V.release(zb_le);
  } else {
    ElasticSc S1;
    RC(S1.init(za_stream, zb_stream, alpha, false));  // Sumcheck::new_space :97
    RC(prove(T.h, S1, P->messages[0], ch1, cap_rounds, P->final_foldings[0], &P->rounds[0]));
  }
  P->spans[1] = since(t0);

  t0 = Clock::now();
  const size_t nt = (size_t)1 << P->rounds[0];
  if (I->ext_fre_row_len != nt + nnz || I->ext_fre_col_len != nz + nnz) return GM_EINVAL;
  uint64_t z_le, w_le;
  RC(reversed(V, z_stream, &z_le));
  RC(reversed(V, w_stream, &w_le));
  uint64_t a_ch, b_ch, c_ch;  // Tensor(r_short), powers of alpha, their product   :150-157
  RC(V.alloc(nt, &b_ch));
  RC(gm_fr_tensor(ch1.data(), P->rounds[0], b_ch));
  RC(V.alloc(nt, &c_ch));
  RC(gm_fr_powers(alpha, nt, c_ch));
  RC(V.alloc(nt, &a_ch));
  RC(gm_fr_hadamard(b_ch, c_ch, a_ch));
  P->spans[2] = since(t0);
  uint64_t ralpha_star, r_star, alpha_star, z_star;  // lookup streams :148,159-161
  RC(V.alloc(nnz, &z_star));
  RC(gm_fr_gather(z_le, I->col_index, z_star));
  RC(V.alloc(nnz, &ralpha_star));
  RC(gm_fr_gather(a_ch, I->row_index, ralpha_star));
  V.release(a_ch);
  RC(V.alloc(nnz, &r_star));
  RC(gm_fr_gather(b_ch, I->row_index, r_star));
  RC(V.alloc(nnz, &alpha_star));
  RC(gm_fr_gather(c_ch, I->row_index, alpha_star));

  t0 = Clock::now();
  {
    uint64_t four[4 * 18];
    RC(K.commit_many(V, {ralpha_star, r_star, alpha_star, z_star}, four));  // :164-172
    memcpy(P->r_star_commitments, four, 3 * 144);
    memcpy(P->z_star_commitment, four + 54, 144);
  }
  P->spans[3] = since(t0);
  RC(gm_transcript_append_g1(T.h, L("ra*"), 3, P->r_star_commitments[0], 1, 0));
  RC(gm_transcript_append_g1(T.h, L("rb*"), 3, P->r_star_commitments[1], 1, 0));
  RC(gm_transcript_append_g1(T.h, L("rc*"), 3, P->r_star_commitments[2], 1, 0));
  RC(gm_transcript_append_g1(T.h, L("z*"), 2, P->z_star_commitment, 1, 0));
  uint64_t eta3[12];  // :181-192
  memcpy(eta3, one, 32);
  RC(gm_transcript_challenge_fr(T.h, L("chal"), 4, eta3 + 4));
  Fr::from_limbs(eta3 + 4).sqr().to_limbs(eta3 + 8);
  uint64_t rhs;
  {
    uint64_t h[3];
    const uint64_t lhs3[3] = {ralpha_star, r_star, alpha_star}, vals[3] = {I->val_a, I->val_b, I->val_c};
    for (int k = 0; k < 3; k++) {
      RC(V.alloc(nnz, &h[k]));
      RC(gm_fr_hadamard(lhs3[k], vals[k], h[k]));
    }
    RC(V.alloc(nnz, &rhs));
    RC(gm_fr_lincomb(h, eta3, 3, rhs));
    for (int k = 0; k < 3; k++) V.release(h[k]);
  }
  t0 = Clock::now();
  if (resident) {
    RC(sumcheck_new_time(T.h, z_star, rhs, one, P->messages[1], ch2, cap_rounds, P->final_foldings[1], &P->rounds[1]));
  } else {
    uint64_t zs, rs;
    RC(reversed(V, z_star, &zs));
    RC(reversed(V, rhs, &rs));
    ElasticSc S2;
    RC(S2.init(zs, rs, one, true));  // Sumcheck::new_elastic :195
    RC(prove(T.h, S2, P->messages[1], ch2, cap_rounds, P->final_foldings[1], &P->rounds[1]));
    S2.reset();
    V.release(zs);
    V.release(rs);
  }
  V.release(rhs);
  P->spans[4] = since(t0);

  uint64_t zeta[4];
  RC(gm_transcript_challenge_fr(T.h, L("zeta"), 4, zeta));  // :199
  t0 = Clock::now();
  uint64_t ahp[3], sorted[3];  // :205-214
  RC(V.alloc(nt, &ahp[0]));
  RC(gm_fr_alg_hash(b_ch, 0, zeta, ahp[0]));
  RC(V.alloc(nt, &ahp[1]));
  RC(gm_fr_alg_hash(c_ch, 0, zeta, ahp[1]));
  RC(V.alloc(nz, &ahp[2]));
  RC(gm_fr_alg_hash(z_le, 0, zeta, ahp[2]));
  RC(V.alloc(I->ext_fre_row_len, &sorted[0]));
  RC(gm_fr_gather(ahp[0], I->ext_fre_row, sorted[0]));
  RC(V.alloc(I->ext_fre_row_len, &sorted[1]));
  RC(gm_fr_gather(ahp[1], I->ext_fre_row, sorted[1]));
  RC(V.alloc(I->ext_fre_col_len, &sorted[2]));
  RC(gm_fr_gather(ahp[2], I->ext_fre_col, sorted[2]));
  for (int k = 0; k < 3; k++) V.release(ahp[k]);
  RC(K.commit_many(V, {sorted[0], sorted[1], sorted[2]}, &P->sorted_commitments[0][0]));
  P->spans[5] = since(t0);
  RC(gm_transcript_append_g1(T.h, L("sorted_alpha_commitment"), 23, P->sorted_commitments[1], 1, 0));  // :220-222
  RC(gm_transcript_append_g1(T.h, L("sorted_r_commitment"), 19, P->sorted_commitments[0], 1, 0));
  RC(gm_transcript_append_g1(T.h, L("sorted_z_commitment"), 19, P->sorted_commitments[2], 1, 0));
  uint64_t gamma[4], chi[4];
  RC(gm_transcript_challenge_fr(T.h, L("gamma"), 5, gamma));
  RC(gm_transcript_challenge_fr(T.h, L("chi"), 3, chi));

  t0 = Clock::now();
  uint64_t pls[9];
  std::vector<uint64_t> accs(9), shifts(9);  // plookup streams, ProductStream, RightRotationStreamer   :227-243
  RC(plookup(V, r_star, b_ch, I->row_index, nnz, I->ext_fre_row, I->ext_fre_row_len, gamma, chi, zeta, pls));
  RC(plookup(V, alpha_star, c_ch, I->row_index, nnz, I->ext_fre_row, I->ext_fre_row_len, gamma, chi, zeta, pls + 3));
  RC(plookup(V, z_star, z_le, I->col_index, nnz, I->ext_fre_col, I->ext_fre_col_len, gamma, chi, zeta, pls + 6));
  for (int k = 0; k < 9; k++) {
    size_t l = 0;
    RC(vec_len(pls[k], &l));
    RC(V.alloc(l + 1, &accs[k]));
    RC(gm_fr_acc_product(pls[k], accs[k]));
    RC(gm_fr_vec_download(accs[k], 0, P->products[k], 1));
    RC(V.alloc(l + 1, &shifts[k]));
    RC(gm_fr_shift_monic(pls[k], shifts[k]));
    V.release(pls[k]);
  }
  V.release(b_ch);
  V.release(c_ch);
  V.release(z_le);
  P->spans[6] = since(t0);
  RC(gm_transcript_append_fr(T.h, L("set_r_ep"), 8, P->products[3], 1));  // :245-250 (labels as in the reference)
  RC(gm_transcript_append_fr(T.h, L("subset_r_ep"), 11, P->products[4], 1));
  RC(gm_transcript_append_fr(T.h, L("set_r_ep"), 8, P->products[0], 1));
  RC(gm_transcript_append_fr(T.h, L("subset_r_ep"), 11, P->products[1], 1));
  RC(gm_transcript_append_fr(T.h, L("set_z_ep"), 8, P->products[6], 1));
  RC(gm_transcript_append_fr(T.h, L("subset_z_ep"), 11, P->products[7], 1));
  if (((size_t)1 << P->rounds[1]) < nnz) return GM_EINVAL;
  uint64_t ep_r;  // Tensor(&sumcheck2.challenges), cut to the looked-up length   :254-257
  RC(V.alloc((size_t)1 << P->rounds[1], &ep_r));
  RC(gm_fr_tensor(ch2.data(), P->rounds[1], ep_r));
  RC(gm_fr_vec_set_len(ep_r, nnz));

  // EntryProduct::new_elastic_batch (entryproduct/elastic_prover.rs:66-127)
  t0 = Clock::now();
  std::vector<ElasticSc> provers(13);
  std::vector<uint64_t> batch_streams;  // reversed streams the 13 provers read in place
  uint64_t psi[4];
  RC(entry_product_claims(K, T.h, V, accs, &P->products[0][0], &P->acc_v_commitments[0][0], psi, &P->claimed_sumchecks[0][0]));
  for (int k = 0; k < 9; k++) {
    if (resident) {
      RC(provers[k].init_resident(accs[k], shifts[k], psi));
      continue;
    }
    uint64_t as, ss;
    RC(reversed(V, accs[k], &as));
    RC(reversed(V, shifts[k], &ss));
    RC(provers[k].init(as, ss, psi, true));  // the provers read their streams in place: released after the batch
    batch_streams.push_back(as);
    batch_streams.push_back(ss);
  }
  P->spans[7] = since(t0);

  uint64_t open_chal[4];
  RC(gm_transcript_challenge_fr(T.h, L("open-chal"), 9, open_chal));  // :313-330
  t0 = Clock::now();
  {
    std::vector<uint64_t> polys = {ralpha_star};
    polys.insert(polys.end(), accs.begin(), accs.end());
    RC(K.open(V, polys, psi, 1, open_chal, P->ralpha_star_acc_mu_proof));  // CommitterKeyStream::open (space.rs:95-125): the quotient by (x - psi)
    RC(gm_fr_eval_le_batch(polys.data(), 10, psi, 1, &P->ralpha_star_acc_mu_evals[0][0]));  // :332-343
  }
  P->spans[8] = since(t0);
  {
    const uint64_t lhs3[3] = {ralpha_star, r_star, alpha_star}, vals[3] = {I->val_a, I->val_b, I->val_c};
    uint64_t lh[3];
    for (int k = 0; k < 3; k++) {
      RC(V.alloc(nnz, &lh[k]));
      RC(gm_fr_hadamard(lhs3[k], ep_r, lh[k]));
    }
    RC(gm_fr_ip(lh[0], I->val_a, P->rstars_vals[0]));  // :348-349
    RC(gm_fr_ip(lh[1], I->val_b, P->rstars_vals[1]));
    for (int k = 0; k < 10; k++) RC(gm_transcript_append_fr(T.h, L("ralpha_star_acc_mu"), 18, P->ralpha_star_acc_mu_evals[k], 1));
    RC(gm_transcript_append_g1(T.h, L("ralpha_star_mu_proof"), 20, P->ralpha_star_acc_mu_proof, 1, 0));
    for (int k = 0; k < 3; k++) {  // :358-377
      if (resident) {
        RC(provers[9 + k].init_resident(lh[k], vals[k], one));
        batch_streams.push_back(lh[k]);  // read in place until the first fold: released after the batch
        continue;
      }
      uint64_t ls, vs;
      RC(reversed(V, lh[k], &ls));
      RC(reversed(V, vals[k], &vs));
      RC(provers[9 + k].init(ls, vs, one, true));
      batch_streams.push_back(ls);
      batch_streams.push_back(vs);
      V.release(lh[k]);
    }
    if (resident) {
      RC(provers[12].init_resident(r_star, alpha_star, psi));
    } else {
      uint64_t rs, as;
      RC(reversed(V, r_star, &rs));
      RC(reversed(V, alpha_star, &as));
      RC(provers[12].init(rs, as, psi, true));
      batch_streams.push_back(rs);
      batch_streams.push_back(as);
    }
  }
  V.release(ep_r);
  t0 = Clock::now();
  std::vector<uint64_t> ch3(cap_rounds * 4, 0);
  RC(prove_batch(T.h, provers.data(), provers.size(), P->messages[2], ch3.data(), cap_rounds, &P->third_final_foldings[0][0], &P->rounds[2]));  // :380
  provers.clear();
  for (uint64_t v : batch_streams) V.release(v);
  P->spans[9] = since(t0);

  // ---- tensorcheck (:384-600): 22 base polynomials, 4 FoldedPolynomialTrees
  t0 = Clock::now();
  if (P->rounds[1] == 0 || P->rounds[2] == 0) return GM_EINVAL;  // a sumcheck of no rounds: no challenge to fold a tree with
  const uint64_t star[4] = {ralpha_star, r_star, alpha_star, z_star};
  RC(psnark_tensorcheck(K, T.h, V, I, w_le, star, sorted, accs, shifts, psi, ch2, ch3, P));
  P->spans[10] = since(t0);
  P->spans[11] = since(t_all);
  return GM_OK;
}
