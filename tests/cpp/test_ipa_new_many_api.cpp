// Drives gm::InnerProductProof::new_many and gm::g2_lincomb_many of include/gemini_hip.hpp on inputs written by
// tests/test_gpu_ipa_new_many_cpp.py: three proofs at d = 5 are made in one call and one by one through the C++ mirror only and
// compared field by field, every proof is verified alone and in one call, and one G2 commitment is made as a short combination.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <memory>

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
  const size_t S = 3;
  std::vector<std::vector<gm::Fr>> a(S), b(S);
  for (size_t s = 0; s < S; s++) {
    a[s] = read_vec<gm::Fr>(in);
    b[s] = read_vec<gm::Fr>(in);
  }
  auto y = read_vec<gm::Fr>(in);           // <a_s, b_s>
  auto b0_canon = read_vec<gm::BigInt>(in);  // b_0 as integers
  try {
    gm::init(0);
    gm::Crs crs(g1, g2);
    gm::Vrs vrs(crs);
    const char* labels[S] = {"gemini-tests", "gemini-tests-1", "gemini-tests-2"};
    std::vector<std::unique_ptr<gm::Transcript>> ts, tm;  // one by one, in one call: three different prefixes
    for (size_t s = 0; s < S; s++) {
      ts.push_back(std::make_unique<gm::Transcript>(labels[s]));
      tm.push_back(std::make_unique<gm::Transcript>(labels[s]));
    }
    gm::InnerProductProof::set_new_many_min(1);
    std::vector<gm::InnerProductProof> many = gm::InnerProductProof::new_many({tm[0].get(), tm[1].get(), tm[2].get()}, crs, a, b);
    const auto path = gm::InnerProductProof::new_many_path();
    printf("path %zu %zu\n", path[0], path[1]);
    printf("made %zu\n", many.size());
    std::vector<const gm::InnerProductProof*> ptrs;
    std::vector<gm::G1Projective> ca;
    std::vector<gm::G2Projective> cb;
    printf("equal");
    for (size_t s = 0; s < S; s++) {
      gm::InnerProductProof single(*ts[s], crs, a[s], b[s]);
      printf(" %d", same(many[s], single) && tm[s]->get_challenge("next") == ts[s]->get_challenge("next") ? 1 : 0);
      ptrs.push_back(&many[s]);
      ca.push_back(crs.commit_g1(a[s]));
      cb.push_back(crs.commit_g2(b[s]));
    }
    printf("\nverify");
    for (size_t s = 0; s < S; s++) printf(" %d", many[s].verify_transcript(vrs, ca[s], cb[s], y[s]) ? 1 : 0);
    printf("\nverify_many");
    for (bool ok : gm::InnerProductProof::verify_many(ptrs, vrs, ca, cb, y)) printf(" %d", ok ? 1 : 0);
    printf("\nnone %zu\n", gm::InnerProductProof::new_many({}, crs, {}, {}).size());
    try {
      gm::InnerProductProof::new_many({tm[0].get(), tm[0].get(), tm[2].get()}, crs, a, b);
      printf("refused 0\n");
    } catch (const gm::Error& e) {
      printf("refused %d\n", e.code);
    }
    // comm_b of proof 0 as one short combination, an empty segment behind it
    const std::vector<gm::G2Affine> pts(g2.begin(), g2.begin() + b0_canon.size());
    const auto lc = gm::g2_lincomb_many(pts, b0_canon, {0, b0_canon.size(), b0_canon.size()});
    printf("lincomb %d %d\n", lc.size() == 2 && lc[0] == cb[0] ? 1 : 0, lc.size() == 2 && lc[1] == gm::g2_zero() ? 1 : 0);
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
