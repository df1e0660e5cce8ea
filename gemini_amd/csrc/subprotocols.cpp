// The sub-protocols the reference exports on their own, as entry points of the library:
//   TensorcheckProof::new_time                 src/subprotocols/tensorcheck/mod.rs:190-275
//   EntryProduct::{new_time_batch, new_time}   src/subprotocols/entryproduct/time_prover.rs:61-147
//   plookup                                    src/subprotocols/plookup/time_prover.rs:89-112
// for a caller that builds an argument of its own from them (a grand product over its own vector, a lookup into its own table).
//
// Pure orchestration over the library's own C ABI, like snark.cpp / psnark.cpp.  The tensor check and the entry product's claims are
// the statements of tensorcheck.hpp that the whole provers call as well: the entries here add their argument checks.
#include "tensorcheck.hpp"

namespace {

using namespace gmprover;

// sumcheck provers created by an entry: freed unless the entry hands them to the caller
struct Provers {
  std::vector<uint64_t> h;
  ~Provers() {
    for (uint64_t p : h) (void)gm_sc_free(p);
  }
};

}  // namespace

extern "C" int gm_tensorcheck_new_time(uint64_t transcript, uint64_t ck_bases, const uint64_t* base_polys, size_t nbase, const gm_tensorcheck_body* bodies,
                                       size_t nbodies, gm_tensorcheck_proof* P) {
  SC_CHECK(P && (base_polys || nbase == 0) && (bodies || nbodies == 0), GM_EINVAL, "tensorcheck_new_time: null pointer");
  size_t nck = 0;
  RC(gm_ck_len(ck_bases, &nck));
  SC_CHECK(nbodies != 0, GM_EINVAL, "tensorcheck_new_time: no body polynomials");  // assert_ne!(batch_challenges.len(), 0)   :203
  size_t nfold = 0;
  for (size_t b = 0; b < nbodies; b++) {
    SC_CHECK(bodies[b].npolys != 0 && bodies[b].polys, GM_EINVAL, "tensorcheck_new_time: body %zu has no polynomials", b);  // :204-206
    SC_CHECK(bodies[b].challenges_mont || bodies[b].nchallenges == 0, GM_EINVAL, "tensorcheck_new_time: body %zu: null challenges", b);
    nfold += bodies[b].nchallenges ? bodies[b].nchallenges - 1 : 0;
  }
  SC_CHECK(nfold <= P->cap_folds, GM_EINVAL, "tensorcheck_new_time: %zu foldings, room for %zu", nfold, P->cap_folds);
  SC_CHECK(P->nbase == nbase && (nbase == 0 || P->base_evaluations) && (nfold == 0 || (P->fold_commitments && P->fold_evaluations)), GM_EINVAL,
           "tensorcheck_new_time: the proof record does not match the call (%zu bases, record %zu) or lacks an array", nbase, P->nbase);
  Vecs V;
  return tensorcheck(TimeKey{ck_bases, nck}, transcript, V, std::vector<uint64_t>(base_polys, base_polys + nbase),
                     std::vector<gm_tensorcheck_body>(bodies, bodies + nbodies), {}, P->cap_folds, P->fold_commitments, P->base_evaluations,
                     P->fold_evaluations, P->evaluation_proof, &P->nfold);
}

extern "C" int gm_entryproduct_new_time_batch(uint64_t transcript, uint64_t ck_bases, const uint64_t* vs, const uint64_t* acc_vs_or_null, size_t k,
                                              const uint64_t* claimed_products_mont, uint64_t* acc_v_commitments, uint64_t* claimed_sumchecks_mont,
                                              uint64_t chal_mont[4], uint64_t* provers) {
  SC_CHECK(chal_mont && (k == 0 || (vs && claimed_products_mont && acc_v_commitments && claimed_sumchecks_mont && provers)), GM_EINVAL,
           "entryproduct_new_time_batch: null pointer");
  size_t nck = 0;
  RC(gm_ck_len(ck_bases, &nck));
  Vecs V;
  std::vector<uint64_t> acc(k), rrot(k);
  for (size_t i = 0; i < k; i++) {  // monic, right_rotation, accumulated_product   :70-78
    size_t l = 0;
    RC(vec_len(vs[i], &l));
    if (acc_vs_or_null) {
      size_t la = 0;
      RC(vec_len(acc_vs_or_null[i], &la));
      SC_CHECK(la == l + 1, GM_EINVAL, "entryproduct_new_time_batch: accumulated vector %zu has %zu entries, its vector %zu", i, la, l);
      acc[i] = acc_vs_or_null[i];
    } else {
      RC(V.alloc(l + 1, &acc[i]));
      RC(gm_fr_acc_product(vs[i], acc[i]));
    }
    RC(V.alloc(l + 1, &rrot[i]));
    RC(gm_fr_shift_monic(vs[i], rrot[i]));
  }
  RC(entry_product_claims(TimeKey{ck_bases, nck}, transcript, V, acc, claimed_products_mont, acc_v_commitments, chal_mont, claimed_sumchecks_mont));  // :79-102
  Provers made;
  for (size_t i = 0; i < k; i++) {  // Witness::new(acc_v, rrot_v, chal) copies both   :86-93
    uint64_t h = 0;
    RC(gm_sc_new_v(acc[i], rrot[i], chal_mont, &h));
    made.h.push_back(h);
  }
  std::copy(made.h.begin(), made.h.end(), provers);
  made.h.clear();  // the caller's from here
  return GM_OK;
}

extern "C" int gm_plookup_new_time(uint64_t subset, uint64_t set, uint64_t index, uint64_t ext_fre_or_0, const uint64_t y_mont[4], const uint64_t z_mont[4],
                                   const uint64_t zeta_mont[4], uint64_t out[3]) {
  SC_CHECK(y_mont && z_mont && zeta_mont && out, GM_EINVAL, "plookup_new_time: null pointer");
  size_t nset = 0, nidx = 0, ext_len = 0;
  RC(vec_len(set, &nset));
  RC(gm_idx_len(index, &nidx));
  struct OwnedIdx {
    uint64_t h = 0;
    ~OwnedIdx() {
      if (h) (void)gm_idx_free(h);
    }
  } built;
  uint64_t ext = ext_fre_or_0;
  if (ext) {
    RC(gm_idx_len(ext, &ext_len));
    SC_CHECK(ext_len == nset + nidx, GM_EINVAL, "plookup_new_time: an extended frequency of %zu entries for a set of %zu and %zu indices", ext_len, nset, nidx);
  } else {
    RC(gm_idx_extend_frequency(index, nset, &built.h, &ext_len));  // :65-78, on the device
    ext = built.h;
  }
  Vecs V;
  uint64_t o[3];
  RC(plookup(V, subset, set, index, nidx, ext, ext_len, y_mont, z_mont, zeta_mont, o));
  for (int k = 0; k < 3; k++) {  // the three results leave the guard: the caller frees them
    V.h.erase(std::find(V.h.begin(), V.h.end(), o[k]));
    out[k] = o[k];
  }
  return GM_OK;
}
