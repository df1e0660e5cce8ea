// Drives the point-validation part of include/gemini_hip.hpp (gm::check_g1 / check_g2, CommitterKey::{check_points, check_powers, from_bytes},
// G2Bases::check_points) on inputs written by tests/test_gpu_points_cpp.py and prints results for the Python side to compare.
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
static void print(const char* tag, const gm::PointCheck& r) {
  printf("%s %d %zu", tag, r.ok ? 1 : 0, r.first_bad);
  for (auto s : r.status) printf(" %u", (unsigned)s);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  auto g1 = read_vec<gm::G1Affine>(in);       // some bad points among them
  auto g2 = read_vec<gm::G2Affine>(in);       // likewise
  auto powers = read_vec<gm::G1Affine>(in);   // tau^i g
  auto g2pair = read_vec<gm::G2Affine>(in);   // g2, tau g2
  auto rho = read_vec<gm::Fr>(in);
  auto good = read_vec<uint8_t>(in);          // compressed zcash bytes of `powers`
  auto bad = read_vec<uint8_t>(in);           // the same with one point outside G1
  try {
    gm::init(0);
    print("g1", gm::check_g1(g1));
    print("g2", gm::check_g2(g2));
    {
      gm::G2Bases b(g2);
      print("g2_bases", b.check_points());
      print("g2_window", b.check_points(0, 2));
    }
    {
      gm::CommitterKey ck(powers);
      print("ck", ck.check_points());
      printf("powers %d\n", ck.check_powers(g2pair[0].x, g2pair[1].x, rho[0]) ? 1 : 0);
      printf("powers_swapped %d\n", ck.check_powers(g2pair[1].x, g2pair[0].x, rho[0]) ? 1 : 0);
    }
    gm::PointCheck rep;
    auto k = gm::CommitterKey::from_bytes(good, powers.size(), true, 1, true, &rep);
    print("from_bytes", rep);
    printf("key %d %zu\n", k ? 1 : 0, k ? k->size() : (size_t)0);
    if (k) printf("key_powers %d\n", k->check_powers(g2pair[0].x, g2pair[1].x, rho[0]) ? 1 : 0);
    auto k2 = gm::CommitterKey::from_bytes(bad, powers.size(), true, 1, true, &rep);
    print("from_bad_bytes", rep);
    printf("bad_key %d\n", k2 ? 1 : 0);
    // the C entry under the mirror: a rejected key leaves *handle = 0 whatever it held
    uint64_t h = 0xFEEDFACEull;
    size_t fb = 0;
    int ok = 1;
    gm::check(gm_g1_bases_from_bytes(bad.data(), powers.size(), 1, 1, 1, &h, nullptr, &fb, &ok));
    printf("bad_handle %llu %d %zu\n", (unsigned long long)h, ok, fb);
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
