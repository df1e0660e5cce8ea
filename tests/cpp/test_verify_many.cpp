// Many proofs in one call through the C++ host mirror (include/gemini_hip.hpp) only: gm::g1_lincomb_many, gm::multi_pairing_many,
// gm::VerifierKey::verify_multi_points_many and gm::SnarkProof::verify_many.
// input file: u64 words -- n, e (4, Montgomery), 1 / e (4), tau (4, canonical), g (12), g2 (24).  Prints one `name value` per line.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gemini_hip.hpp"

static std::vector<uint64_t> read_words(const char* path) {
  std::vector<uint64_t> w;
  FILE* f = std::fopen(path, "rb");
  if (!f) std::exit(3);
  uint64_t v;
  while (std::fread(&v, 8, 1, f) == 1) w.push_back(v);
  std::fclose(f);
  return w;
}
static std::string bits(const std::vector<bool>& v) {
  std::string s;
  for (bool b : v) s += b ? '1' : '0';
  return s.empty() ? "none" : s;
}
// a normalised Jacobian point as an affine record
static gm::G1Affine affine(const gm::G1Projective& p) {
  gm::G1Affine a;
  memset(&a, 0, sizeof a);
  bool identity = true;
  for (int i = 12; i < 18; i++) identity = identity && p[i] == 0;
  if (identity) a.infinity = 1;
  else memcpy(&a, p.data(), 96);
  return a;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::vector<uint64_t> in = read_words(argv[1]);
  if (in.size() != 1 + 4 + 4 + 4 + 12 + 24) return 2;
  const size_t n = in[0];
  gm::Fr e, inv_e;
  gm::BigInt tau;
  memcpy(e.data(), &in[1], 32);
  memcpy(inv_e.data(), &in[5], 32);
  memcpy(tau.data(), &in[9], 32);
  const uint64_t* g = &in[13];
  const uint64_t* g2 = &in[25];
  try {
    gm::init(0);
    gm::G1Affine P;
    gm::G2Affine Q;
    memset(&P, 0, sizeof P);
    memset(&Q, 0, sizeof Q);
    memcpy(&P, g, 96);
    memcpy(&Q, g2, 192);
    // 2 P + 3 P = 5 P as two segments; 2 P and (r - 2) P as two more, and an empty one
    const gm::BigInt r_minus_2 = {0xfffffffeffffffffULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL};
    const std::vector<gm::G1Projective> sums =
        gm::g1_lincomb_many({P, P, P, P, P}, {gm::BigInt{2, 0, 0, 0}, gm::BigInt{3, 0, 0, 0}, gm::BigInt{5, 0, 0, 0}, gm::BigInt{2, 0, 0, 0}, r_minus_2}, {0, 2, 3, 4, 5, 5});
    std::printf("lincomb %d%d\n", (int)(sums.size() == 5 && sums[0] == sums[1]), (int)(sums[4] == gm::g1_zero()));
    // e(2 P, Q) e(-2 P, Q) = 1, e(P, Q), the empty product
    const std::vector<gm::Gt> prods = gm::multi_pairing_many({affine(sums[2]), affine(sums[3]), P}, {Q, Q, Q}, {0, 2, 3, 3});
    std::printf("pairing %d%d%d\n", (int)(prods[0] == gm::gt_one()), (int)(prods[1] == gm::multi_pairing({P}, {Q}) && !(prods[1] == gm::gt_one())),
                (int)(prods[2] == gm::gt_one()));

    gm::Matrix diag(n);
    for (size_t i = 0; i < n; i++) diag[i] = {{inv_e, i}};
    const gm::R1cs r1cs(diag, diag, diag, std::vector<gm::Fr>(n, e), std::vector<gm::Fr>(n - 1, e));
    const gm::CommitterKey ck = gm::CommitterKey::cyclic_share(g, tau, 2 * n);
    const gm::VerifierKey vk = gm::VerifierKey::from_trapdoor(g, g2, tau, 5);

    // ---- KZG: p(X) = e + X / e opened at 0 (quotient 1 / e, Z(X) = X: the constant term of Z is a dead pair) and the constant e
    // opened at two points (the proof element is the identity), with a wrong value and a wrong count between them
    const gm::Fr zero = {0, 0, 0, 0};
    gm::VerifierKey::MultiPointsCheck at_zero{{ck.commit({e, inv_e})}, {zero}, {{e}}, ck.commit({inv_e}), inv_e};
    gm::VerifierKey::MultiPointsCheck constant{{ck.commit({e})}, {e, inv_e}, {{e, e}}, gm::g1_zero(), e};
    gm::VerifierKey::MultiPointsCheck wrong_value = at_zero, wrong_count = constant;
    wrong_value.evaluations[0][0] = inv_e;
    wrong_count.commitments.push_back(wrong_count.commitments[0]);
    const std::vector<gm::VerifierKey::MultiPointsCheck> checks = {at_zero, wrong_value, wrong_count, constant};
    std::printf("kzg_many %s\n", bits(vk.verify_multi_points_many(checks)).c_str());
    std::vector<bool> singles;
    for (const auto& c : checks) singles.push_back(vk.verify_multi_points(c.commitments, c.eval_points, c.evaluations, c.proof, c.open_chal));
    std::printf("kzg_singles %s\n", bits(singles).c_str());
    std::printf("kzg_none %s\n", bits(vk.verify_multi_points_many({})).c_str());

    // ---- snark: the honest proof, one the host part rejects, one only the pairing rejects, the honest one again
    const gm::SnarkProof proof = gm::SnarkProof::new_time(r1cs, ck);
    gm::SnarkProof bad_host = proof, bad_pairing = proof;
    bad_host.zc_alpha[0] ^= 1;
    bad_pairing.tensorcheck_proof.evaluation_proof = gm::g1_add(proof.tensorcheck_proof.evaluation_proof, proof.tensorcheck_proof.evaluation_proof);
    const std::vector<const gm::SnarkProof*> batch = {&proof, &bad_host, &bad_pairing, &proof};
    std::printf("snark_many %s\n", bits(gm::SnarkProof::verify_many(batch, r1cs, vk)).c_str());
    gm::set_verify_many_min(1);
    std::printf("snark_many_min_1 %s\n", bits(gm::SnarkProof::verify_many(batch, r1cs, vk)).c_str());
    gm::set_verify_many_min(100);
    std::printf("snark_many_min_100 %s\n", bits(gm::SnarkProof::verify_many(batch, r1cs, vk)).c_str());
    gm::set_verify_many_min(3);  // the default
    singles.clear();
    for (const gm::SnarkProof* p : batch) singles.push_back(p->verify(r1cs, vk));
    std::printf("snark_singles %s\n", bits(singles).c_str());
    std::printf("snark_none %s\n", bits(gm::SnarkProof::verify_many({}, r1cs, vk)).c_str());
    const gm::VerifierKey other = gm::VerifierKey::from_trapdoor(g, g2, gm::BigInt{12345, 0, 0, 0}, 5);
    std::printf("snark_other_key %s\n", bits(gm::SnarkProof::verify_many(batch, r1cs, other)).c_str());
  } catch (const gm::Error& err) {
    std::printf("error %s\n", err.what());
    return 1;
  }
  return 0;
}
