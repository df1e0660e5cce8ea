// Drives the GtModule part of include/gemini_hip.hpp (gm::gt_multi_pow, gm::HerringGt) on inputs written by
// tests/test_gpu_gt_module_cpp.py and prints results as hex for the Python side to compare.
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
  auto x = read_vec<gm::Gt>(in);       // 5 elements
  auto e = read_vec<gm::BigInt>(in);   // 5 exponents
  auto f = read_vec<gm::Gt>(in);       // 8 elements
  auto g = read_vec<gm::Fr>(in);       // 8 scalars
  auto tw = read_vec<gm::Fr>(in);
  auto ch = read_vec<gm::Fr>(in);
  try {
    gm::init(0);
    print("multi", gm::gt_multi_pow(x, e));
    print("head", gm::gt_multi_pow(std::vector<gm::Gt>(x.begin(), x.begin() + 2), e));  // zip: 2 terms
    print("empty", gm::gt_multi_pow(std::vector<gm::Gt>(), e));
    gm::HerringGt p(f, g, tw[0]);
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
  } catch (const std::exception& ex) {
    fprintf(stderr, "error: %s\n", ex.what());
    return 1;
  }
  return 0;
}
