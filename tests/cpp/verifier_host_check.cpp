// The host-only arithmetic of the verifiers (gemini_amd/csrc/verifier_host.hpp) as a stand-alone program, built with the host
// sanitizers by tests/test_verifier_cpu.py.  One command per input line, arguments and results as hexadecimal canonical
// integers:   <command> <hex> <hex> ...   ->   <hex> <hex> ...
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "verifier_host.hpp"

using gmverify::Fr;

static Fr parse(const std::string& s) {
  uint64_t c[4] = {0, 0, 0, 0};
  int nibble = 0;
  for (size_t i = s.size(); i-- > 0 && nibble < 64; nibble++) {
    const char ch = s[i];
    const uint64_t v = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : 0;
    c[nibble / 16] |= v << (4 * (nibble % 16));
  }
  return Fr::from_canonical(c);
}
static uint64_t count(const std::string& s) { return std::stoull(s, nullptr, 16); }
static void print(const std::vector<Fr>& v) {
  for (size_t i = 0; i < v.size(); i++) {
    uint64_t c[4];
    v[i].to_canonical(c);
    std::printf("%s%016llx%016llx%016llx%016llx", i ? " " : "", (unsigned long long)c[3], (unsigned long long)c[2], (unsigned long long)c[1],
                (unsigned long long)c[0]);
  }
  std::printf("\n");
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, tok;
    in >> cmd;
    std::vector<std::string> a;
    while (in >> tok) a.push_back(tok);
    auto F = [&](size_t i) { return parse(a.at(i)); };
    auto Fs = [&](size_t from, size_t n) {
      std::vector<Fr> v;
      for (size_t i = 0; i < n; i++) v.push_back(parse(a.at(from + i)));
      return v;
    };
    if (cmd == "reduce") {
      print({gmverify::reduce(F(0), F(1), F(2), F(3))});
    } else if (cmd == "vanishing") {  // k points
      print(gmverify::vanishing(Fs(1, count(a.at(0)))));
    } else if (cmd == "interpolate") {  // k nrows open_chal points[k] evaluations[nrows * k]
      const size_t k = count(a.at(0)), rows = count(a.at(1));
      const std::vector<Fr> ev = Fs(3 + k, rows * k);
      print(gmverify::interpolate_combination(Fs(3, k), ev.data(), rows, F(2)));
    } else if (cmd == "sq_fp") {  // pos neg rho beta
      print({gmverify::evaluate_sq_fp(F(0), F(1), F(2), gmverify::fr_u64(2).inv(), F(3).dbl().inv())});
    } else if (cmd == "tensor_poly") {  // k x elements[k]
      const std::vector<Fr> el = Fs(2, count(a.at(0)));
      print({gmverify::evaluate_tensor_poly(el.data(), el.size(), F(1))});
    } else if (cmd == "geometric_poly") {
      print({gmverify::evaluate_geometric_poly(F(0), count(a.at(1)))});
    } else if (cmd == "index_poly") {
      print({gmverify::evaluate_index_poly(F(0), count(a.at(1)))});
    } else if (cmd == "plookup_subset") {  // subset_eval index_eval x y zeta n
      print({gmverify::plookup_subset_eval(F(0), F(1), F(2), F(3), F(4), count(a.at(5)))});
    } else if (cmd == "plookup_set") {  // set_eval x y z n
      print({gmverify::plookup_set_eval(F(0), F(1), F(2), F(3), count(a.at(4)))});
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
