// Drives gm::InnerProductProof::verify_many and gm::gt_multi_pow_many of include/gemini_hip.hpp on inputs written by
// tests/test_gpu_ipa_verify_many_cpp.py: two proofs of different rounds are made and verified through the C++ mirror only, alone and in
// one call, and the GT products are printed as hex for the Python side.
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
  auto a0 = read_vec<gm::Fr>(in);
  auto b0 = read_vec<gm::Fr>(in);
  auto a1 = read_vec<gm::Fr>(in);
  auto b1 = read_vec<gm::Fr>(in);
  auto y = read_vec<gm::Fr>(in);  // <a0, b0>, <a1, b1>, a wrong value
  auto exps = read_vec<gm::BigInt>(in);
  auto offs = read_vec<uint64_t>(in);
  try {
    gm::init(0);
    gm::Crs crs(g1, g2);
    gm::Vrs vrs(crs);
    gm::Transcript t0("gemini-tests"), t1("gemini-tests");
    gm::InnerProductProof p0(t0, crs, a0, b0), p1(t1, crs, a1, b1);
    printf("rounds %zu %zu\n", p0.rounds(), p1.rounds());
    const gm::G1Projective ca0 = crs.commit_g1(a0), ca1 = crs.commit_g1(a1);
    const gm::G2Projective cb0 = crs.commit_g2(b0), cb1 = crs.commit_g2(b1);
    // p0, p0 with a wrong y, p1, p1 under the commitment of the other proof's vector
    const std::vector<const gm::InnerProductProof*> proofs = {&p0, &p0, &p1, &p1};
    const std::vector<gm::G1Projective> ca = {ca0, ca0, ca1, ca0};
    const std::vector<gm::G2Projective> cb = {cb0, cb0, cb1, cb1};
    const std::vector<gm::Fr> ys = {y[0], y[2], y[1], y[1]};
    printf("single");
    for (size_t s = 0; s < proofs.size(); s++) printf(" %d", proofs[s]->verify_transcript(vrs, ca[s], cb[s], ys[s]) ? 1 : 0);
    printf("\nmany");
    for (bool ok : gm::InnerProductProof::verify_many(proofs, vrs, ca, cb, ys)) printf(" %d", ok ? 1 : 0);
    printf("\nnone %zu\n", gm::InnerProductProof::verify_many({}, vrs, {}, {}, {}).size());
    try {
      gm::InnerProductProof::verify_many(proofs, vrs, ca, cb, {y[0]});
      printf("refused 0\n");
    } catch (const gm::Error& e) {
      printf("refused %d\n", e.code);
    }
    // the messages of both proofs as the elements of S products
    std::vector<gm::Gt> x;
    for (const gm::InnerProductProof* p : {&p0, &p1})
      for (const auto& m : p->messages()) {
        x.push_back(m.a);
        x.push_back(m.b);
      }
    for (const auto& e : x) print("x", e);
    for (const auto& g : gm::gt_multi_pow_many(x, exps, std::vector<size_t>(offs.begin(), offs.end()))) print("prod", g);
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
