// The host-only field arithmetic of the verifiers (verifier.cpp): the sumcheck's `reduce`, the vanishing polynomial and the
// Lagrange interpolation of KZG's verify_multi_points, the folding relation of the tensor check and the closed-form polynomial
// evaluations of the preprocessing verifier.  Nothing here touches the device or the C ABI: tests/cpp/verifier_host_check.cpp
// runs it under the host sanitizers against values from the Python restatement.
#pragma once
#include <vector>

#include "host_field.hpp"

namespace gmverify {

using gmh::Fr;

inline Fr fr_u64(uint64_t v) {
  const uint64_t c[4] = {v, 0, 0, 0};
  return Fr::from_canonical(c);
}
inline Fr fr_pow_u64(Fr base, uint64_t e) {
  Fr acc = Fr::one();
  for (; e; e >>= 1) {
    if (e & 1) acc = acc * base;
    base = base.sqr();
  }
  return acc;
}

// Subclaim::reduce (sumcheck/subclaim.rs:77-96): the round polynomial a + b x + c x^2 with c = claim - a, at the challenge
inline Fr reduce(const Fr& claim, const Fr& a, const Fr& b, const Fr& r) { return a + r * b + (claim - a) * r.sqr(); }

// prod_j (x - points[j]), little-endian, monic: npoints + 1 coefficients                src/kzg/mod.rs:192-197
inline std::vector<Fr> vanishing(const std::vector<Fr>& points, size_t skip = (size_t)-1) {
  std::vector<Fr> z{Fr::one()};
  for (size_t j = 0; j < points.size(); j++) {
    if (j == skip) continue;
    z.push_back(Fr::zero());
    for (size_t d = z.size() - 1; d > 0; d--) z[d] = z[d - 1] - points[j] * z[d];
    z[0] = Fr::zero() - points[j] * z[0];
  }
  return z;
}

// sum_i etas[i] * (the interpolation of row i of `evaluations` at `points`), npoints coefficients  src/kzg/mod.rs:199-232
// evaluations: nrows x npoints; linear in the rows, so the rows are combined first and interpolated once
inline std::vector<Fr> interpolate_combination(const std::vector<Fr>& points, const Fr* evaluations, size_t nrows, const Fr& open_chal) {
  const size_t k = points.size();
  std::vector<Fr> y(k, Fr::zero()), out(k, Fr::zero());
  Fr eta = Fr::one();
  for (size_t i = 0; i < nrows; i++) {
    for (size_t j = 0; j < k; j++) y[j] = y[j] + eta * evaluations[i * k + j];
    eta = eta * open_chal;
  }
  for (size_t j = 0; j < k; j++) {
    Fr sca = Fr::one();
    for (size_t t = 0; t < k; t++)
      if (t != j) sca = sca * (points[j] - points[t]);
    const Fr f = sca.inv() * y[j];
    const std::vector<Fr> lang = vanishing(points, j);
    for (size_t d = 0; d < lang.size(); d++) out[d] = out[d] + lang[d] * f;
  }
  return out;
}

// f'(beta^2) = (f(beta) + f(-beta)) / 2 + rho (f(beta) - f(-beta)) / (2 beta)                tensorcheck/mod.rs:96-107
inline Fr evaluate_sq_fp(const Fr& pos, const Fr& neg, const Fr& rho, const Fr& two_inv, const Fr& two_beta_inv) {
  return (pos + neg) * two_inv + (pos - neg) * rho * two_beta_inv;
}

// <powers(x), tensor(elements)> = prod_j (1 + elements[j] x^(2^j))                            src/misc.rs:373-382
inline Fr evaluate_tensor_poly(const Fr* elements, size_t k, Fr x) {
  Fr res = Fr::one();
  for (size_t j = 0; j < k; j++) {
    res = res * (Fr::one() + elements[j] * x);
    x = x.sqr();
  }
  return res;
}
// 1 + x + ... + x^(n - 1)                                                                      src/misc.rs:387-389
inline Fr evaluate_geometric_poly(const Fr& x, uint64_t n) { return (fr_pow_u64(x, n) - Fr::one()) * (x - Fr::one()).inv(); }
// 0 + x + 2 x^2 + ... + (n - 1) x^(n - 1), x != 1                                              src/misc.rs:394-399
inline Fr evaluate_index_poly(const Fr& x, uint64_t n) {
  const Fr x1 = Fr::one() - x, x_n = fr_pow_u64(x, n - 1);
  return x * (Fr::one() - x_n) * x1.sqr().inv() - fr_u64(n - 1) * x_n * x * x1.inv();
}
// shift(f + zeta * index + y * geometric)(x)                                                   src/psnark/verifier.rs:37-63
inline Fr plookup_subset_eval(const Fr& subset_eval, const Fr& index_eval, const Fr& x, const Fr& y, const Fr& zeta, uint64_t n) {
  return x * (subset_eval + zeta * index_eval + y * evaluate_geometric_poly(x, n)) + Fr::one();
}
// shift((1 + z) y geometric(n + 1) + (x + z) f)(x)                                             src/psnark/verifier.rs:68-84
inline Fr plookup_set_eval(const Fr& set_eval, const Fr& x, const Fr& y, const Fr& z, uint64_t n) {
  return x * ((Fr::one() + z) * y * evaluate_geometric_poly(x, n + 1) + (x + z) * set_eval) + Fr::one();
}

}  // namespace gmverify
