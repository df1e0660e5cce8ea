// Drives the element-wise GT part of include/gemini_hip.hpp (gm::gt_final_exp_many, gm::pairing_each, gm::check_gt,
// gm::HerringGt::check, gm::InnerProductProof::check_messages) on inputs written by tests/test_gpu_gt_device_cpp.py and prints
// results for the Python side to compare.
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
template <size_t N>
static void print(const char* tag, const std::array<uint64_t, N>& a) {
  printf("%s", tag);
  for (auto x : a) printf(" %016llx", (unsigned long long)x);
  printf("\n");
}
static void print(const char* tag, const gm::PointCheck& c) {
  printf("%s %d %zu", tag, c.ok ? 1 : 0, c.first_bad);
  for (auto s : c.status) printf(" %u", (unsigned)s);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  auto x = read_vec<gm::Gt>(in);         // members and non-members
  auto good = read_vec<gm::Gt>(in);      // 6 members
  auto g1 = read_vec<gm::G1Affine>(in);  // 16 points
  auto g2 = read_vec<gm::G2Affine>(in);
  auto s = read_vec<gm::Fr>(in);         // 8 scalars: a prover's g, the vectors of a proof
  auto tw = read_vec<gm::Fr>(in);
  try {
    gm::init(0);
    for (const auto& v : gm::gt_final_exp_many(x)) print("fe", v);
    printf("fe_empty %zu\n", gm::gt_final_exp_many({}).size());
    for (const auto& v : gm::pairing_each(g1, g2)) print("pair", v);
    {
      gm::G2Bases b2(g2);
      uint64_t h1 = 0;
      gm::check(gm_g1_bases_register(g1.data(), sizeof(gm::G1Affine), g1.size(), &h1));
      for (const auto& v : gm::pairing_each(h1, 1, 2, b2, 0, 3, 5)) print("pair_h", v);
      gm::check(gm_g1_bases_free(h1));
    }
    print("check", gm::check_gt(x));
    print("check_good", gm::check_gt(good));
    print("check_empty", gm::check_gt({}));
    printf("not_cyclotomic %u\n", (unsigned)gm::PointStatus::NotCyclotomic);
    {
      gm::HerringGt p(good, std::vector<gm::Fr>(s.begin(), s.begin() + 6), tw[0]);
      auto c = p.check();
      printf("hgt %d %zu\n", c.ok ? 1 : 0, c.first_bad);
      auto bad = good;
      bad[4] = x[0];
      gm::HerringGt q(bad, std::vector<gm::Fr>(s.begin(), s.begin() + 6), tw[0]);
      c = q.check();
      printf("hgt_bad %d %zu\n", c.ok ? 1 : 0, c.first_bad);
      q.fold(s[7]);
      c = q.check();
      printf("hgt_bad_folded %d %zu\n", c.ok ? 1 : 0, c.first_bad);
    }
    gm::Crs crs(g1, g2);
    gm::Transcript transcript("gemini-tests");
    gm::InnerProductProof proof(transcript, crs, s, std::vector<gm::Fr>(s.rbegin(), s.rend()));
    auto c = proof.check_messages();
    printf("ipa %d %zu %zu\n", c.ok ? 1 : 0, c.first_bad, proof.rounds());
  } catch (const std::exception& ex) {
    fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
  return 0;
}
