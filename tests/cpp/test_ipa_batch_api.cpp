// Drives gm::InnerProductProof::new_batch / verify_batch / claims of include/gemini_hip.hpp on inputs written by
// tests/test_gpu_ipa_batch_cpp.py: one proof for three claims at d = 5 through the C++ mirror only, verified, rejected for an altered
// y and for swapped commitments; one claim in a batch call against the constructor's proof field by field; the refusals.
#include <cstdio>
#include <fstream>
#include <iostream>

#include "gemini_hip.hpp"

template <class T>
static std::vector<T> read_vec(std::ifstream& in) {
  uint64_t n;
  in.read((char*)&n, 8);
  std::vector<T> v(n);
  in.read((char*)v.data(), n * sizeof(T));
  return v;
}

static bool same(const gm::InnerProductProof& p, const gm::InnerProductProof& q) {
  if (p.rounds() != q.rounds() || p.challenges() != q.challenges() || p.batch_challenges() != q.batch_challenges()) return false;
  const auto mp = p.messages(), mq = q.messages();
  for (size_t i = 0; i < mp.size(); i++)
    if (mp[i].a != mq[i].a || mp[i].b != mq[i].b) return false;
  return p.final_foldings() == q.final_foldings() && p.foldings_ff() == q.foldings_ff() && p.foldings_fg1() == q.foldings_fg1() && p.foldings_fg2() == q.foldings_fg2();
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  auto g1 = read_vec<gm::G1Affine>(in);
  auto g2 = read_vec<gm::G2Affine>(in);
  const size_t K = 3;
  std::vector<std::vector<gm::Fr>> a(K), b(K);
  for (size_t i = 0; i < K; i++) {
    a[i] = read_vec<gm::Fr>(in);
    b[i] = read_vec<gm::Fr>(in);
  }
  auto y = read_vec<gm::Fr>(in);      // <a_i, b_i>
  auto y_bad = read_vec<gm::Fr>(in);  // y with y_1 + 1
  try {
    gm::init(0);
    gm::Crs crs(g1, g2);
    gm::Vrs vrs(crs);
    gm::Transcript t("gemini-tests"), t1("gemini-tests"), t2("gemini-tests"), t3("gemini-tests");
    gm::InnerProductProof proof = gm::InnerProductProof::new_batch(t, crs, a, b);
    const auto fold = proof.foldings_batch();
    printf("claims %zu\n", proof.claims());
    printf("lengths %zu %zu %zu %zu %zu\n", proof.rounds(), proof.batch_challenges().size(), fold.ff.size(), fold.fg1.size(), fold.fg2.size());
    // the final point is the folded CRS for every claim, the final scalars are those of the FModule provers
    bool shared = true;
    for (size_t i = 0; i < K; i++)
      shared = shared && fold.fg1[i].first == fold.fg1[0].first && fold.fg2[i].second == fold.fg2[0].second && fold.fg1[i].second == fold.ff[i].first &&
               fold.fg2[i].first == fold.ff[i].second;
    printf("shared %d\n", shared ? 1 : 0);
    std::vector<gm::G1Projective> ca;
    std::vector<gm::G2Projective> cb;
    for (size_t i = 0; i < K; i++) {
      ca.push_back(crs.commit_g1(a[i]));
      cb.push_back(crs.commit_g2(b[i]));
    }
    printf("verify %d\n", proof.verify_batch(vrs, ca, cb, y) ? 1 : 0);
    printf("bad_y %d\n", proof.verify_batch(vrs, ca, cb, y_bad) ? 1 : 0);
    printf("swapped %d\n", proof.verify_batch(vrs, {ca[1], ca[0], ca[2]}, cb, y) ? 1 : 0);
    printf("points %d messages %d\n", proof.check_points().ok ? 1 : 0, proof.check_messages().ok ? 1 : 0);
    const auto path = gm::InnerProductProof::new_batch_path();
    printf("path %zu %zu %zu\n", path[0], path[1], path[2]);
    // one claim: the constructor's proof and the same transcript afterwards
    gm::InnerProductProof single(t1, crs, a[0], b[0]);
    gm::InnerProductProof one = gm::InnerProductProof::new_batch(t2, crs, {a[0]}, {b[0]});
    printf("one %d %zu\n", same(one, single) && t1.get_challenge("next") == t2.get_challenge("next") ? 1 : 0, one.claims());
    printf("one_verify %d %d\n", one.verify_transcript(vrs, ca[0], cb[0], y[0]) ? 1 : 0, one.verify_batch(vrs, {ca[0]}, {cb[0]}, {y[0]}) ? 1 : 0);
    // refusals: another K at the verifier, a single-claim entry on a batch proof, no claims at the prover
    int codes[3] = {0, 0, 0};
    try {
      proof.verify_batch(vrs, {ca[0]}, {cb[0]}, {y[0]});
    } catch (const gm::Error& e) {
      codes[0] = e.code;
    }
    try {
      proof.verify_transcript(vrs, ca[0], cb[0], y[0]);
    } catch (const gm::Error& e) {
      codes[1] = e.code;
    }
    try {
      gm::InnerProductProof::new_batch(t3, crs, {}, {});
    } catch (const gm::Error& e) {
      codes[2] = e.code;
    }
    gm::Transcript fresh("gemini-tests");
    printf("refused %d %d %d %d\n", codes[0], codes[1], codes[2], t3.get_challenge("after") == fresh.get_challenge("after") ? 1 : 0);
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
