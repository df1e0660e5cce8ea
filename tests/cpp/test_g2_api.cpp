// Drives the G2 part of include/gemini_hip.hpp (gm::G2Bases, gm::HerringG2, g2_add) on inputs written by
// tests/test_gpu_g2_cpp.py and prints results as hex for the Python side to compare.
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
  auto points = read_vec<gm::G2Affine>(in);
  auto bigints = read_vec<gm::BigInt>(in);
  auto scalars = read_vec<gm::Fr>(in);
  auto f = read_vec<gm::Fr>(in);
  auto tw = read_vec<gm::Fr>(in);
  auto ch = read_vec<gm::Fr>(in);
  try {
    gm::init(0);
    {
      gm::G2Bases b(points);
      printf("size %zu\n", b.size());
      print("msm_bigint", b.msm_bigint(bigints));
      auto head = std::vector<gm::BigInt>(bigints.begin(), bigints.begin() + 50);
      print("msm_bigint_rev", b.msm_bigint(head, 120, true));
      print("msm_unchecked", b.msm_unchecked(scalars));
      auto rec = b.download(3, 2);
      printf("download");
      for (auto x : rec) printf(" %016llx", (unsigned long long)x);
      printf("\n");
      print("zero", gm::g2_zero());
      print("add", gm::g2_add(b.msm_bigint(head), b.msm_bigint(head, 120, true)));
    }
    gm::HerringG2 p(f, std::vector<gm::G2Affine>(points.begin(), points.begin() + 16), tw[0]);
    printf("rounds %zu\n", p.rounds());
    std::optional<gm::Fr> vm;
    for (size_t k = 0;; k++) {
      auto m = p.next_message(vm);
      if (!m) break;
      print("a", m->a);
      print("b", m->b);
      vm = ch[k];
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
