// Drives the pairing part of include/gemini_hip.hpp (gm::multi_pairing, gm::Gt helpers, gm::HerringP) on inputs written by
// tests/test_gpu_pairing_cpp.py and prints results as hex for the Python side to compare.
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
  auto tw = read_vec<gm::Fr>(in);
  auto ch = read_vec<gm::Fr>(in);
  auto k = read_vec<gm::BigInt>(in);
  try {
    gm::init(0);
    const gm::Gt whole = gm::multi_pairing(g1, g2);
    print("multi", whole);
    print("one", gm::gt_one());
    print("empty", gm::multi_pairing(std::vector<gm::G1Affine>(), g2));
    const gm::Gt head = gm::multi_pairing(std::vector<gm::G1Affine>(g1.begin(), g1.begin() + 3), g2);  // zip: 3 pairs
    print("head", head);
    print("mul", gm::gt_mul(whole, head));
    print("pow", gm::gt_pow(head, k[0]));
    {
      gm::G2Bases b2(g2);
      uint64_t h1 = 0;
      gm::check(gm_g1_bases_register(g1.data(), sizeof(gm::G1Affine), g1.size(), &h1));
      print("strided", gm::multi_pairing(h1, 1, 2, b2, 0, 1, 3));
      gm::check(gm_g1_bases_free(h1));
    }
    gm::HerringP p(g1, g2, tw[0]);
    printf("rounds %zu\n", p.rounds());
    std::optional<gm::Fr> vm;
    for (size_t r = 0;; r++) {
      auto m = p.next_message(vm);
      if (!m) break;
      print("a", m->a);
      print("b", m->b);
      vm = ch[r];
    }
    auto ff = p.final_foldings();
    printf("final %d\n", ff ? 1 : 0);
    if (ff) {
      print("f0", ff->first);
      print("g0", ff->second);
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
