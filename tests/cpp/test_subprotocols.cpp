// Drives the stand-alone sub-protocols of include/gemini_hip.hpp -- gm::EntryProduct::new_time_batch + gm::Sumcheck::prove_batch,
// gm::TensorcheckProof::new_time, gm::plookup -- on inputs written by tests/test_gpu_subprotocols.py and prints the results as hex for
// the Python side to compare with the oracle.
#include <cstdio>
#include <fstream>

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
  auto srs = read_vec<gm::G1Affine>(in);
  auto v0 = read_vec<gm::Fr>(in);
  auto v1 = read_vec<gm::Fr>(in);
  auto products = read_vec<gm::Fr>(in);  // the claimed products of v0, v1
  auto poly = read_vec<gm::Fr>(in);      // tensor check: one base = one body polynomial
  auto randomness = read_vec<gm::Fr>(in);
  auto set = read_vec<gm::Fr>(in);       // plookup
  auto index = read_vec<uint32_t>(in);
  auto yzzeta = read_vec<gm::Fr>(in);
  try {
    gm::init(0);
    gm::CommitterKey ck(srs);
    {
      gm::Transcript t;
      std::vector<gm::TimeProver> provers;
      {
        gm::DeviceVec d0(v0), d1(v1);
        gm::EntryProduct ep = gm::EntryProduct::new_time_batch(t, ck, {&d0, &d1}, products);
        for (auto& c : ep.msgs.acc_v_commitments) print("ep_acc_v", c);
        for (auto& s : ep.msgs.claimed_sumchecks) print("ep_claimed", s);
        print("ep_chal", ep.chal);
        provers = std::move(ep.provers);
      }  // the input vectors are gone: the provers own their data
      gm::Sumcheck sc = gm::Sumcheck::prove_batch(t, provers);
      for (size_t k = 0; k < sc.messages.size(); k++) {
        print("ep_msg_a", sc.messages[k].a);
        print("ep_msg_b", sc.messages[k].b);
      }
      for (auto& ff : sc.final_foldings) {
        print("ep_ff_lhs", ff[0]);
        print("ep_ff_rhs", ff[1]);
      }
      print("ep_after", t.get_challenge("after"));
    }
    {
      gm::Transcript t;
      gm::DeviceVec p(poly);
      gm::TensorcheckProof tc = gm::TensorcheckProof::new_time(t, ck, {&p}, {gm::TensorcheckProof::Body{{&p}, randomness}});
      for (auto& c : tc.folded_polynomials_commitments) print("tc_fc", c);
      for (auto& e : tc.folded_polynomials_evaluations) {
        print("tc_fe", e[0]);
        print("tc_fe", e[1]);
      }
      print("tc_open", tc.evaluation_proof);
      for (auto& e : tc.base_polynomials_evaluations)
        for (auto& x : e) print("tc_be", x);
      print("tc_after", t.get_challenge("after"));
    }
    {
      gm::DeviceVec dset(set);
      gm::IdxVec didx(index);
      std::vector<gm::Fr> sub;
      for (uint32_t i : index) sub.push_back(set[i]);
      gm::DeviceVec dsub(sub);
      auto built = gm::plookup(dsub, dset, didx, yzzeta[0], yzzeta[1], yzzeta[2]);
      gm::IdxVec ext = didx.extend_frequency(set.size());
      auto kept = gm::plookup(dsub, dset, didx, yzzeta[0], yzzeta[1], yzzeta[2], &ext);
      bool same = ext.size() == set.size() + index.size();
      for (int k = 0; k < 3; k++) same = same && built[k].to_host() == kept[k].to_host();
      printf("plookup_ext_equal %d\n", same ? 1 : 0);
      for (auto& x : built[2].to_host()) print("plookup_sorted", x);
    }
    int code = 0;
    try {
      gm::IdxVec bad(std::vector<uint32_t>{0, 7});
      (void)bad.extend_frequency(7);  // 7 is outside a set of 7 elements
    } catch (const gm::Error& e) {
      code = e.code;
    }
    printf("error_path %d\n", code);
  } catch (const std::exception& e) {
    printf("FAILED %s\n", e.what());
    return 1;
  }
  return 0;
}
