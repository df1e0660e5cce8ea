// The G1 point check of gemini_amd/csrc/points.hip (canonical limbs, y^2 = x^3 + 4, (beta x, y) == -[x^2] P) on the library's own
// host arithmetic (gmh:: of host_field.hpp), one thread: the host side of the comparison in profiles/point_check.md.
// Built and started by tools/point_check_bench.py.  Input file: u64 n, 6 limbs of beta (ark-ff Montgomery form), n x 12 limbs.
// Prints "<points that pass> <milliseconds>".
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_field.hpp"

using gmh::Fq;
using gmh::G1;

static const uint64_t X_ABS = 0xd201000000010000ull;

static G1 mul_x(const G1& p) {
  G1 acc = p;
  for (int bit = 62; bit >= 0; bit--) {
    acc = acc.dbl();
    if ((X_ABS >> bit) & 1) acc = acc.add(p);
  }
  return acc;
}

static bool check(const uint64_t* rec, const Fq& beta) {
  bool zero = true;
  for (int i = 0; i < 12; i++) zero = zero && rec[i] == 0;
  if (zero) return true;
  if (gmh::geq<6>(rec, gmh::FqP::MOD) || gmh::geq<6>(rec + 6, gmh::FqP::MOD)) return false;
  const Fq x = Fq::from_limbs(rec), y = Fq::from_limbs(rec + 6);
  const Fq one = Fq::one(), four = one.dbl().dbl();
  if (!(y.sqr() == x.sqr() * x + four)) return false;
  G1 p;
  p.x = x;
  p.y = y;
  p.z = one;
  const G1 u = mul_x(mul_x(p));
  if (u.is_identity()) return false;
  const Fq zz = u.z.sqr();
  return beta * x * zz == u.x && (y * zz * u.z + u.y).is_zero();
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t n = 0, b[6];
  if (fread(&n, 8, 1, f) != 1 || fread(b, 8, 6, f) != 6) return 2;
  std::vector<uint64_t> rec(n * 12);
  if (fread(rec.data(), 96, n, f) != n) return 2;
  fclose(f);
  const Fq beta = Fq::from_limbs(b);
  const auto t0 = std::chrono::steady_clock::now();
  size_t pass = 0;
  for (uint64_t i = 0; i < n; i++) pass += check(rec.data() + 12 * i, beta) ? 1 : 0;
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  printf("%zu %.3f\n", pass, ms);
  return 0;
}
