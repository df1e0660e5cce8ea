// Drives gm::HerringG1Space and gm::HerringG2Space of include/gemini_hip.hpp (the module space provers over a registered key, and
// the time provers their to_time() returns) on inputs written by tests/test_gpu_herring_space_cpp.py and prints results as hex for
// the Python side to compare.
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

// the whole run of a space prover; after `switch_at` messages a time prover is taken and driven beside it with the same challenges
template <class Space>
static void run(const char* tag, Space& sp, const std::vector<gm::Fr>& ch, size_t switch_at) {
  printf("%s rounds %zu\n", tag, sp.rounds());
  std::optional<gm::Fr> vm;
  std::optional<decltype(sp.to_time())> tp;
  for (size_t k = 0;; k++) {
    if (k == switch_at) {
      if (vm) sp.fold(*vm);
      vm.reset();
      tp.emplace(sp.to_time());
      printf("%s time %zu %zu\n", tag, tp->round(), tp->rounds());
    }
    auto m = sp.next_message(vm);
    if (tp) {
      auto t = tp->next_message(vm);
      if (bool(t) != bool(m)) throw std::runtime_error("the time prover ends at another round");
      if (t) {
        print("ta", t->a);
        print("tb", t->b);
      }
    }
    if (!m) break;
    print("a", m->a);
    print("b", m->b);
    vm = ch[k];
  }
  auto ff = sp.final_foldings();
  if (!ff) throw std::runtime_error("no final foldings after the last round");
  print("f0", ff->first);
  print("g0", ff->second);
  if (tp) {
    auto tf = tp->final_foldings();
    if (!tf) throw std::runtime_error("no final foldings of the time prover");
    print("tf0", tf->first);
    print("tg0", tf->second);
  }
  auto p = sp.path();
  printf("%s path %zu %zu %zu %zu\n", tag, p[0], p[1], p[2], p[3]);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  auto g1 = read_vec<gm::G1Affine>(in);
  auto g2 = read_vec<gm::G2Affine>(in);
  auto stream = read_vec<gm::Fr>(in);
  auto tw = read_vec<gm::Fr>(in);
  auto ch = read_vec<gm::Fr>(in);
  try {
    gm::init(0);
    gm::CommitterKey key1(g1);
    gm::G2Bases key2(g2);
    gm::DeviceVec vec(stream);
    {
      gm::HerringG1Space sp(key1.handle(), 2, g1.size() - 2, vec, tw[0]);
      run("g1", sp, ch, 2);
    }
    {
      gm::HerringG2Space sp(key2.handle(), 1, g2.size() - 1, vec, tw[0]);
      run("g2", sp, ch, 0);
    }
    auto rec = key1.download(0, g1.size());
    printf("key1");
    for (auto x : rec) printf(" %016llx", (unsigned long long)x);
    printf("\n");
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
