// Drives the key-generation part of include/gemini_hip.hpp (G2Bases::{fixed_base, srs, from_candidates}, CommitterKey::from_candidates,
// Crs::{from_scalars, from_candidates, truncate, halve, fold, bases, len}) on inputs written by tests/test_gpu_keygen_cpp.py and prints
// what each returns for the Python side to compare with the Python mirror.
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
static void print_words(const char* tag, const std::vector<uint64_t>& w) {
  printf("%s", tag);
  for (auto v : w) printf(" %016llx", (unsigned long long)v);
  printf("\n");
}
static void print_crs(const char* tag, const gm::Crs& c) {
  auto b = c.bases();
  const auto n = c.len();
  printf("%s_len %zu %zu\n", tag, n.first, n.second);
  print_words((std::string(tag) + "_g1").c_str(), b.first.download(0, b.first.size()));
  print_words((std::string(tag) + "_g2").c_str(), b.second.download(0, b.second.size()));
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  auto g1 = read_vec<uint64_t>(in);     // the G1 generator, 12 words
  auto g2 = read_vec<uint64_t>(in);     // the G2 generator, 24 words
  auto a = read_vec<gm::BigInt>(in);    // canonical scalars
  auto b = read_vec<gm::BigInt>(in);    // as many
  auto tau = read_vec<gm::BigInt>(in);  // one
  auto c1 = read_vec<uint8_t>(in);      // G1 candidates
  auto c2 = read_vec<uint8_t>(in);      // G2 candidates
  auto ch = read_vec<gm::Fr>(in);       // one challenge, Montgomery
  auto va = read_vec<gm::Fr>(in);       // two vectors to prove an inner product of
  auto vb = read_vec<gm::Fr>(in);
  try {
    gm::init(0);
    gm::G2Bases fb = gm::G2Bases::fixed_base(g2.data(), b);
    print_words("fixed_base", fb.download(0, fb.size()));
    gm::G2Bases srs = gm::G2Bases::srs(g2.data(), tau[0], 5);
    print_words("srs", srs.download(0, srs.size()));
    printf("srs_check %d\n", srs.check_points().ok ? 1 : 0);
    size_t used = 0, found = 0;
    auto k1 = gm::CommitterKey::from_candidates(c1, 6, &used, &found);
    printf("g1_cand %d %zu %zu\n", k1 ? 1 : 0, used, found);
    if (!k1) return 1;
    print_words("g1_cand_points", k1->download(0, k1->size()));
    auto k2 = gm::G2Bases::from_candidates(c2, 6, &used, &found);
    printf("g2_cand %d %zu %zu\n", k2 ? 1 : 0, used, found);
    if (!k2) return 1;
    print_words("g2_cand_points", k2->download(0, k2->size()));
    auto none = gm::G2Bases::from_candidates(c2, c2.size() / 96, &used, &found);  // every candidate would have to survive
    printf("g2_short %d %zu %zu\n", none ? 1 : 0, used, found);
    gm::Crs crs = gm::Crs::from_scalars(g1.data(), a, g2.data(), b);
    print_crs("crs", crs);
    print_crs("fold", crs.fold(ch[0]));
    print_crs("halve", crs.halve());
    print_crs("truncate", crs.truncate(1));
    printf("truncate_all %zu\n", crs.truncate(40).len().first);
    print_crs("crs_after", crs);
    auto fresh = gm::Crs::from_candidates(c1, c2, 16);
    printf("crs_from_candidates %d\n", fresh ? 1 : 0);
    if (!fresh) return 1;
    gm::KeyCheck kc = fresh->check();
    printf("fresh_check %d %zu %zu\n", kc.ok ? 1 : 0, kc.first_bad_g1, kc.first_bad_g2);
    gm::Transcript t("gemini-tests");
    gm::InnerProductProof proof(t, *fresh, va, vb);
    const auto msgs = proof.messages();
    print_words("msg0", std::vector<uint64_t>(msgs[0].a.begin(), msgs[0].a.end()));
    printf("crs_too_short %d\n", gm::Crs::from_candidates(c1, c2, c2.size() / 96) ? 1 : 0);
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
