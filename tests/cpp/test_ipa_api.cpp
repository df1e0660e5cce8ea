// Drives the inner-product argument of include/gemini_hip.hpp (gm::Crs, gm::Vrs, gm::InnerProductProof) on inputs written by
// tests/test_gpu_ipa_cpp.py: proves and verifies through the C++ mirror only and prints every field as hex for the Python side.
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

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  auto g1 = read_vec<gm::G1Affine>(in);
  auto g2 = read_vec<gm::G2Affine>(in);
  auto a = read_vec<gm::Fr>(in);
  auto b = read_vec<gm::Fr>(in);
  auto y = read_vec<gm::Fr>(in);  // <a, b>, then a wrong value
  try {
    gm::init(0);
    gm::Crs crs(g1, g2);
    gm::Vrs vrs(crs);
    printf("levels %zu\n", vrs.levels());
    for (size_t l = 0; l < vrs.levels(); l++) {
      auto lv = vrs.level(l);
      print("vk1e", lv.first.first);
      print("vk1o", lv.first.second);
      print("vk2e", lv.second.first);
      print("vk2o", lv.second.second);
    }
    gm::Transcript transcript("gemini-tests");
    gm::InnerProductProof proof(transcript, crs, a, b);
    printf("rounds %zu\n", proof.rounds());
    for (const auto& m : proof.messages()) {
      print("a", m.a);
      print("b", m.b);
    }
    for (const auto& c : proof.challenges()) print("challenge", c);
    for (const auto& c : proof.batch_challenges()) print("batch", c);
    for (const auto& f : proof.final_foldings()) {
      print("lhs", f.first);
      print("rhs", f.second);
    }
    print("ff0", proof.foldings_ff().first);
    print("ff1", proof.foldings_ff().second);
    print("fg1f", proof.foldings_fg1().first);
    print("fg1g", proof.foldings_fg1().second);
    print("fg2f", proof.foldings_fg2().first);
    print("fg2g", proof.foldings_fg2().second);
    print("next", transcript.get_challenge("next"));
    const gm::G1Projective comm_a = crs.commit_g1(a);
    const gm::G2Projective comm_b = crs.commit_g2(b);
    print("comm_a", comm_a);
    print("comm_b", comm_b);
    printf("verify %d\n", proof.verify_transcript(vrs, comm_a, comm_b, y[0]) ? 1 : 0);
    printf("verify_wrong_y %d\n", proof.verify_transcript(vrs, comm_a, comm_b, y[1]) ? 1 : 0);
    try {
      gm::InnerProductProof refused(transcript, crs, std::vector<gm::Fr>(a.begin(), a.begin() + 1), std::vector<gm::Fr>(b.begin(), b.begin() + 1));
      printf("refused 0\n");
    } catch (const gm::Error& e) {
      printf("refused %d\n", e.code);
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
