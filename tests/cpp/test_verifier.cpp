// The verifiers through the C++ host mirror (include/gemini_hip.hpp) only: prove, verify, flip a limb, verify.
// input file: u64 words -- n, e (4, Montgomery), 1 / e (4), tau (4, canonical), g (12), g2 (24).  Prints one `name value` per line.
#include <cstdio>
#include <cstdlib>
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
    // dummy_r1cs (src/circuit.rs:349-365): A = B = C = diag(1 / e), z = [e; n], w = [e; n - 1]
    gm::Matrix diag(n);
    for (size_t i = 0; i < n; i++) diag[i] = {{inv_e, i}};
    const gm::R1cs r1cs(diag, diag, diag, std::vector<gm::Fr>(n, e), std::vector<gm::Fr>(n - 1, e));
    {
      const gm::CommitterKey ck = gm::CommitterKey::cyclic_share(g, tau, 2 * n);
      const gm::VerifierKey vk = gm::VerifierKey::from_trapdoor(g, g2, tau, 5);
      gm::SnarkProof proof = gm::SnarkProof::new_time(r1cs, ck);
      std::printf("snark %d\n", (int)proof.verify(r1cs, vk));
      std::printf("snark_elastic %d\n", (int)gm::SnarkProof::new_elastic(r1cs, ck).verify(r1cs, vk));
      proof.zc_alpha[0] ^= 1;
      std::printf("snark_zc_alpha %d\n", (int)proof.verify(r1cs, vk));
      proof.zc_alpha[0] ^= 1;
      proof.tensorcheck_proof.folded_polynomials_evaluations.back()[1][0] ^= 1;
      std::printf("snark_fold_evaluation %d\n", (int)proof.verify(r1cs, vk));
      proof.tensorcheck_proof.folded_polynomials_evaluations.back()[1][0] ^= 1;
      std::printf("snark_restored %d\n", (int)proof.verify(r1cs, vk));
      const gm::VerifierKey other = gm::VerifierKey::from_trapdoor(g, g2, gm::BigInt{12345, 0, 0, 0}, 5);
      std::printf("snark_other_key %d\n", (int)proof.verify(r1cs, other));
    }
    {
      const gm::CommitterKey ck = gm::CommitterKey::cyclic_share(g, tau, 2 * n + 1);  // 2 n + 2 powers: what a verifiable psnark proof needs
      const gm::VerifierKey vk = gm::VerifierKey::from_trapdoor(g, g2, tau, 3);
      const std::vector<uint8_t> ck_bytes = vk.g2_bytes();
      std::printf("g2_bytes ");
      for (uint8_t b : ck_bytes) std::printf("%02x", b);
      std::printf("\n");
      const gm::PsnarkInstance inst(r1cs);
      const auto index = inst.index(ck);
      gm::PsnarkProof proof = gm::PsnarkProof::new_time(ck, inst, index, ck_bytes);
      std::printf("psnark %d\n", (int)proof.verify(r1cs, vk, index, inst.num_non_zero()));
      proof.rstars_vals[1][0] ^= 1;
      std::printf("psnark_rstars %d\n", (int)proof.verify(r1cs, vk, index, inst.num_non_zero()));
      proof.rstars_vals[1][0] ^= 1;
      proof.tensorcheck_proof.base_polynomials_evaluations[17][2][0] ^= 1;
      std::printf("psnark_base_evaluation %d\n", (int)proof.verify(r1cs, vk, index, inst.num_non_zero()));
      proof.tensorcheck_proof.base_polynomials_evaluations[17][2][0] ^= 1;
      std::printf("psnark_count %d\n", (int)proof.verify(r1cs, vk, index, inst.num_non_zero() + 1));
      std::printf("psnark_restored %d\n", (int)proof.verify(r1cs, vk, index, inst.num_non_zero()));
    }
    try {  // a freed key is a stale handle: misuse throws, it is no verdict
      uint64_t stale = 0;
      {
        const gm::VerifierKey tmp = gm::VerifierKey::from_trapdoor(g, g2, tau, 1);
        stale = tmp.handle();
      }
      size_t n1 = 0;
      gm::check(gm_vk_len(stale, &n1, nullptr));
      std::printf("stale ok\n");
    } catch (const gm::Error& err) {
      std::printf("stale %d\n", err.code);
    }
  } catch (const gm::Error& err) {
    std::printf("error %d %s\n", err.code, err.what());
    return 1;
  }
  return 0;
}
