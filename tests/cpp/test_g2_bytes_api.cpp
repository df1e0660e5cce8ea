// Drives the byte and check part of include/gemini_hip.hpp (G2Bases::{from_bytes, to_bytes}, CommitterKey::to_bytes, Crs::{from_bases,
// check}, VerifierKey::check, InnerProductProof::check_points) on inputs written by tests/test_gpu_g2_bytes_cpp.py and prints results
// for the Python side to compare.
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
static void print_bytes(const char* tag, const std::vector<uint8_t>& b) {
  printf("%s ", tag);
  for (auto c : b) printf("%02x", (unsigned)c);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  auto g1 = read_vec<gm::G1Affine>(in);   // members of G1
  auto g2 = read_vec<gm::G2Affine>(in);   // members of G2, as many
  auto good = read_vec<uint8_t>(in);      // compressed zcash bytes of `g2`
  auto bad = read_vec<uint8_t>(in);       // the same with one point outside G2
  auto a = read_vec<gm::Fr>(in);
  auto b = read_vec<gm::Fr>(in);
  try {
    gm::init(0);
    gm::PointCheck rep;
    auto k2 = gm::G2Bases::from_bytes(good, g2.size(), true, 1, true, &rep);
    print("from_bytes", rep);
    printf("key %d %zu\n", k2 ? 1 : 0, k2 ? k2->size() : (size_t)0);
    auto none = gm::G2Bases::from_bytes(bad, g2.size(), true, 1, true, &rep);
    print("from_bad_bytes", rep);
    printf("bad_key %d\n", none ? 1 : 0);
    if (!k2) return 1;
    gm::G2Bases reg(g2);
    printf("same_records %d\n", k2->download(0, g2.size()) == reg.download(0, g2.size()) ? 1 : 0);
    print_bytes("g2_compressed_zcash", k2->to_bytes(true, 1));
    print_bytes("g2_uncompressed_ark", reg.to_bytes(false, 0, 1, 2));
    gm::CommitterKey ck(g1);
    print_bytes("g1_compressed_ark", ck.to_bytes(true, 0));
    print_bytes("g1_uncompressed_zcash", ck.to_bytes(false, 1, 1, 2));
    // a CRS from the decoded keys proves like one from the records
    gm::Crs from_bases = gm::Crs::from_bases(ck, *k2);
    gm::Crs from_records(g1, g2);
    gm::KeyCheck kc = from_bases.check();
    printf("crs_check %d %zu %zu\n", kc.ok ? 1 : 0, kc.first_bad_g1, kc.first_bad_g2);
    gm::Transcript t1("gemini-tests"), t2("gemini-tests");
    gm::InnerProductProof p1(t1, from_bases, a, b), p2(t2, from_records, a, b);
    const auto m1 = p1.messages(), m2 = p2.messages();
    printf("same_proof %d\n", m1.size() == m2.size() && memcmp(m1.data(), m2.data(), 1152 * m1.size()) == 0 && p1.final_foldings() == p2.final_foldings() ? 1 : 0);
    gm::ProofCheck pc = p1.check_points();
    printf("ipa_check %d %zu\n", pc.ok ? 1 : 0, pc.first_bad);
    // the same bytes with one point outside G2 decode without validation; the checks then name it
    auto unchecked = gm::G2Bases::from_bytes(bad, g2.size(), true, 1, false, &rep);
    printf("unchecked_key %d\n", unchecked ? 1 : 0);
    if (unchecked) {
      print("unchecked_points", unchecked->check_points());
      gm::Crs c = gm::Crs::from_bases(ck, *unchecked);
      kc = c.check();
      printf("bad_crs_check %d %zu %zu\n", kc.ok ? 1 : 0, kc.first_bad_g1, kc.first_bad_g2);
    }
    std::vector<gm::G1Affine> vk1(g1.begin(), g1.begin() + 2);
    std::vector<gm::G2Affine> vk2(g2.begin(), g2.begin() + 3);
    gm::VerifierKey vk(vk1, vk2);
    kc = vk.check();
    printf("vk_check %d %zu %zu\n", kc.ok ? 1 : 0, kc.first_bad_g1, kc.first_bad_g2);
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
