// The Fq12 tower of BLS12-381 on the device, for the Miller loop of pairing.hip (gfx950).
//
// Fq12 = Fq6[w] / (w^2 - v), Fq6 = Fq2[v] / (v^3 - xi), xi = 1 + u, on the Fq2 of g2.cuh; every component is fully reduced.
// Replaces: `Fp12::mul_assign` / `square_in_place` / `mul_by_014` / `conjugate_in_place` of ark-ff 0.4.2 as
// `Bls12::multi_miller_loop` uses them (ark-ec 0.4.2 models/bls12/mod.rs) behind PModule::ip (src/herring/module.rs:60-79).
// Products: Fq12 = 3 Fq6 (Karatsuba) = 54 Fq, square = 2 Fq6 (complex) = 36 Fq, product by a line = 13 Fq2 = 39 Fq.
#pragma once
#include "g2.cuh"

namespace gm {

struct Fq6 {
  Fq2 c0, c1, c2;
};
struct Fq12 {
  Fq6 c0, c1;
};

// (a0 + a1 u)(1 + u) = (a0 - a1) + (a0 + a1) u
GM_DEV Fq2 fq2_mul_xi(const Fq2& a) {
  Fq2 r;
  r.c0 = fq_sub(a.c0, a.c1);
  r.c1 = fq_add(a.c0, a.c1);
  return r;
}
GM_DEV Fq2 fq2_neg(const Fq2& a) { return fq2_sub(fq2_zero(), a); }
// a * s for s in Fq
GM_DEV Fq2 fq2_mul_fq(const Fq2& a, const FqE& s) {
  Fq2 r;
  r.c0 = fq_mul(a.c0, s);
  r.c1 = fq_mul(a.c1, s);
  return r;
}
// 12 a = 8 a + 4 a
GM_DEV Fq2 fq2_mul12(const Fq2& a) {
  const Fq2 a4 = fq2_dbl(fq2_dbl(a));
  return fq2_add(fq2_dbl(a4), a4);
}

GM_DEV Fq6 fq6_zero() {
  Fq6 r;
  r.c0 = fq2_zero();
  r.c1 = fq2_zero();
  r.c2 = fq2_zero();
  return r;
}
GM_DEV Fq6 fq6_add(const Fq6& a, const Fq6& b) {
  Fq6 r;
  r.c0 = fq2_add(a.c0, b.c0);
  r.c1 = fq2_add(a.c1, b.c1);
  r.c2 = fq2_add(a.c2, b.c2);
  return r;
}
GM_DEV Fq6 fq6_sub(const Fq6& a, const Fq6& b) {
  Fq6 r;
  r.c0 = fq2_sub(a.c0, b.c0);
  r.c1 = fq2_sub(a.c1, b.c1);
  r.c2 = fq2_sub(a.c2, b.c2);
  return r;
}
// a v = xi a2 + a0 v + a1 v^2
GM_DEV Fq6 fq6_mul_v(const Fq6& a) {
  Fq6 r;
  r.c0 = fq2_mul_xi(a.c2);
  r.c1 = a.c0;
  r.c2 = a.c1;
  return r;
}
// Karatsuba, 6 Fq2 products
GM_DEV Fq6 fq6_mul(const Fq6& a, const Fq6& b) {
  const Fq2 v0 = fq2_mul(a.c0, b.c0), v1 = fq2_mul(a.c1, b.c1), v2 = fq2_mul(a.c2, b.c2);
  const Fq2 t0 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c1, a.c2), fq2_add(b.c1, b.c2)), v1), v2);
  Fq6 r;
  r.c0 = fq2_add(v0, fq2_mul_xi(t0));
  r.c1 = fq2_add(fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c0, a.c1), fq2_add(b.c0, b.c1)), v0), v1), fq2_mul_xi(v2));
  r.c2 = fq2_add(fq2_sub(fq2_sub(fq2_mul(fq2_add(a.c0, a.c2), fq2_add(b.c0, b.c2)), v0), v2), v1);
  return r;
}
// a (b0 + b1 v), 5 Fq2 products
GM_DEV Fq6 fq6_mul_01(const Fq6& a, const Fq2& b0, const Fq2& b1) {
  const Fq2 aa = fq2_mul(a.c0, b0), bb = fq2_mul(a.c1, b1);
  const Fq2 t1 = fq2_sub(fq2_mul(fq2_add(a.c1, a.c2), b1), bb);
  Fq6 r;
  r.c0 = fq2_add(fq2_mul_xi(t1), aa);
  r.c1 = fq2_sub(fq2_sub(fq2_mul(fq2_add(b0, b1), fq2_add(a.c0, a.c1)), aa), bb);
  r.c2 = fq2_add(fq2_sub(fq2_mul(fq2_add(a.c0, a.c2), b0), aa), bb);
  return r;
}
// a (b1 v) = xi a2 b1 + a0 b1 v + a1 b1 v^2, 3 Fq2 products
GM_DEV Fq6 fq6_mul_1(const Fq6& a, const Fq2& b1) {
  Fq6 r;
  r.c0 = fq2_mul_xi(fq2_mul(a.c2, b1));
  r.c1 = fq2_mul(a.c0, b1);
  r.c2 = fq2_mul(a.c1, b1);
  return r;
}

GM_DEV Fq12 fq12_one() {
  Fq12 r;
  r.c0 = fq6_zero();
  r.c0.c0 = fq2_one();
  r.c1 = fq6_zero();
  return r;
}
GM_DEV Fq12 fq12_mul(const Fq12& a, const Fq12& b) {
  const Fq6 aa = fq6_mul(a.c0, b.c0), bb = fq6_mul(a.c1, b.c1);
  const Fq6 m = fq6_mul(fq6_add(a.c0, a.c1), fq6_add(b.c0, b.c1));
  Fq12 r;
  r.c0 = fq6_add(aa, fq6_mul_v(bb));
  r.c1 = fq6_sub(fq6_sub(m, aa), bb);
  return r;
}
// (a0 + a1 w)^2 = (a0 + a1)(a0 + v a1) - a0 a1 - v a0 a1 + 2 a0 a1 w
GM_DEV Fq12 fq12_sqr(const Fq12& a) {
  const Fq6 ab = fq6_mul(a.c0, a.c1);
  const Fq6 m = fq6_mul(fq6_add(a.c0, a.c1), fq6_add(a.c0, fq6_mul_v(a.c1)));
  Fq12 r;
  r.c0 = fq6_sub(fq6_sub(m, ab), fq6_mul_v(ab));
  r.c1 = fq6_add(ab, ab);
  return r;
}
GM_DEV Fq12 fq12_conj(const Fq12& a) {  // a0 - a1 w
  Fq12 r;
  r.c0 = a.c0;
  r.c1 = fq6_sub(fq6_zero(), a.c1);
  return r;
}
// a (l0 + l1 v + l4 v w): the product by a line of the M-type twist (ark-ff `mul_by_014`), 13 Fq2 products
GM_DEV Fq12 fq12_mul_014(const Fq12& a, const Fq2& l0, const Fq2& l1, const Fq2& l4) {
  const Fq6 aa = fq6_mul_01(a.c0, l0, l1);
  const Fq6 bb = fq6_mul_1(a.c1, l4);
  const Fq6 m = fq6_mul_01(fq6_add(a.c0, a.c1), l0, fq2_add(l1, l4));
  Fq12 r;
  r.c0 = fq6_add(aa, fq6_mul_v(bb));
  r.c1 = fq6_sub(fq6_sub(m, aa), bb);
  return r;
}

// ---- Frobenius maps, inverse, and the arithmetic of the cyclotomic subgroup: what the final exponentiation and the GT membership
// test of pairing.hip are made of.  Replaces `Fp12::frobenius_map_in_place`, `inverse`, `cyclotomic_square_in_place` and
// `Bls12::exp_by_x` of ark-ff / ark-ec 0.4.2 as `Bls12::final_exponentiation` uses them.
#include "gt_consts_gen.inc"  // GT_FROB1, GT_FROB2 (gen_gt_consts.py)

GM_DEV FqE gt_const(const uint32_t (&c)[12]) {
  FqE r;
#pragma unroll
  for (int i = 0; i < 12; i++) r.l[i] = c[i];
  return r;
}
GM_DEV Fq2 fq2_conj(const Fq2& a) {
  Fq2 r;
  r.c0 = a.c0;
  r.c1 = fq_sub(fqe_zero(), a.c1);
  return r;
}
GM_DEV bool fq12_is_zero(const Fq12& a) {
  return fq2_is_zero(a.c0.c0) && fq2_is_zero(a.c0.c1) && fq2_is_zero(a.c0.c2) && fq2_is_zero(a.c1.c0) && fq2_is_zero(a.c1.c1) && fq2_is_zero(a.c1.c2);
}
GM_DEV bool fq12_eq(const Fq12& a, const Fq12& b) {  // on fully reduced coefficients
  const FqE* x = reinterpret_cast<const FqE*>(&a);
  const FqE* y = reinterpret_cast<const FqE*>(&b);
  bool eq = true;
#pragma unroll
  for (int k = 0; k < 12; k++) eq = eq && x[k] == y[k];
  return eq;
}

// a^q: the coefficient c at w^k (k = 2 j + h for c_h.c_j) goes to conj(c) xi^(k (q - 1) / 6).  5 Fq2 products.
GM_DEV Fq2 fq12_frob1_coef(const Fq2& c, int k) {
  Fq2 g;
  g.c0 = gt_const(GT_FROB1[k][0]);
  g.c1 = gt_const(GT_FROB1[k][1]);
  return fq2_mul(fq2_conj(c), g);
}
GM_DEV Fq12 fq12_frobenius1(const Fq12& a) {
  Fq12 r;
  r.c0.c0 = fq2_conj(a.c0.c0);
  r.c0.c1 = fq12_frob1_coef(a.c0.c1, 2);
  r.c0.c2 = fq12_frob1_coef(a.c0.c2, 4);
  r.c1.c0 = fq12_frob1_coef(a.c1.c0, 1);
  r.c1.c1 = fq12_frob1_coef(a.c1.c1, 3);
  r.c1.c2 = fq12_frob1_coef(a.c1.c2, 5);
  return r;
}
// a^(q^2): Fq2 is fixed, the coefficient at w^k picks up delta^k for the sixth root of unity delta = xi^((q^2 - 1) / 6) of Fq.  10 Fq products.
GM_DEV Fq12 fq12_frobenius2(const Fq12& a) {
  Fq12 r;
  r.c0.c0 = a.c0.c0;
  r.c0.c1 = fq2_mul_fq(a.c0.c1, gt_const(GT_FROB2[2]));
  r.c0.c2 = fq2_mul_fq(a.c0.c2, gt_const(GT_FROB2[4]));
  r.c1.c0 = fq2_mul_fq(a.c1.c0, gt_const(GT_FROB2[1]));
  r.c1.c1 = fq2_mul_fq(a.c1.c1, gt_const(GT_FROB2[3]));
  r.c1.c2 = fq2_mul_fq(a.c1.c2, gt_const(GT_FROB2[5]));
  return r;
}

// 1 / a through the norms Fq12 -> Fq6 -> Fq2 -> Fq (the formulas of gmh::Fq12::inv), ONE Fermat inversion in Fq (fq2_inv of g2.cuh).
// Zero gives zero: 0^(q - 2) = 0 and every product downstream is a product by it.
GM_DEV Fq6 fq6_inv(const Fq6& a) {
  const Fq2 t0 = fq2_sub(fq2_sqr(a.c0), fq2_mul_xi(fq2_mul(a.c1, a.c2)));
  const Fq2 t1 = fq2_sub(fq2_mul_xi(fq2_sqr(a.c2)), fq2_mul(a.c0, a.c1));
  const Fq2 t2 = fq2_sub(fq2_sqr(a.c1), fq2_mul(a.c0, a.c2));
  const Fq2 di = fq2_inv(fq2_add(fq2_mul(a.c0, t0), fq2_mul_xi(fq2_add(fq2_mul(a.c2, t1), fq2_mul(a.c1, t2)))));
  Fq6 r;
  r.c0 = fq2_mul(t0, di);
  r.c1 = fq2_mul(t1, di);
  r.c2 = fq2_mul(t2, di);
  return r;
}
GM_DEV Fq12 fq12_inv(const Fq12& a) {
  const Fq6 di = fq6_inv(fq6_sub(fq6_mul(a.c0, a.c0), fq6_mul_v(fq6_mul(a.c1, a.c1))));
  Fq12 r;
  r.c0 = fq6_mul(a.c0, di);
  r.c1 = fq6_sub(fq6_zero(), fq6_mul(a.c1, di));
  return r;
}

// (a + b s)^2 in Fq4 = Fq2[s] / (s^2 - xi): (a + b)(a + xi b) - a b - xi a b, 2 a b.  2 Fq2 products.
GM_DEV void fq4_sqr(const Fq2& a, const Fq2& b, Fq2& r0, Fq2& r1) {
  const Fq2 ab = fq2_mul(a, b);
  r0 = fq2_sub(fq2_sub(fq2_mul(fq2_add(a, b), fq2_add(fq2_mul_xi(b), a)), ab), fq2_mul_xi(ab));
  r1 = fq2_dbl(ab);
}
GM_DEV Fq2 fq2_3t_minus_2z(const Fq2& t, const Fq2& z) { return fq2_add(fq2_dbl(fq2_sub(t, z)), t); }
GM_DEV Fq2 fq2_3t_plus_2z(const Fq2& t, const Fq2& z) { return fq2_add(fq2_dbl(fq2_add(t, z)), t); }
// a^2 by Granger-Scott ("Faster squaring in the cyclotomic subgroup of sixth degree extensions", PKC 2010) over Fq2: three Fq4
// squarings, 18 Fq products for the 36 of fq12_sqr.  VALID ON THE CYCLOTOMIC SUBGROUP ONLY (a^(q^4 - q^2 + 1) = 1, i.e. behind
// the easy part of the final exponentiation); on any other element the result is NOT the square.
GM_DEV Fq12 fq12_cyclotomic_sqr(const Fq12& a) {
  Fq2 t0, t1, t2, t3, t4, t5;
  fq4_sqr(a.c0.c0, a.c1.c1, t0, t1);
  fq4_sqr(a.c1.c0, a.c0.c2, t2, t3);
  fq4_sqr(a.c0.c1, a.c1.c2, t4, t5);
  Fq12 r;
  r.c0.c0 = fq2_3t_minus_2z(t0, a.c0.c0);
  r.c0.c1 = fq2_3t_minus_2z(t2, a.c0.c1);
  r.c0.c2 = fq2_3t_minus_2z(t4, a.c0.c2);
  r.c1.c0 = fq2_3t_plus_2z(fq2_mul_xi(t5), a.c1.c0);
  r.c1.c1 = fq2_3t_plus_2z(t1, a.c1.c1);
  r.c1.c2 = fq2_3t_plus_2z(t3, a.c1.c2);
  return r;
}

// One Fq12 per lane as a column of 32-bit words: limb j at col[j * stride] (LDS or a device workspace; a wave reads 64 consecutive
// words per limb when its lanes' columns are consecutive)
GM_DEV void fq12_col_store(uint32_t* col, int stride, const Fq12& a) {
  const FqE* e = reinterpret_cast<const FqE*>(&a);  // 12 FqE back to back, tower order
#pragma unroll
  for (int k = 0; k < 12; k++) {
#pragma unroll
    for (int i = 0; i < Fq::N; i++) col[(k * Fq::N + i) * stride] = e[k].l[i];
  }
}
GM_DEV Fq12 fq12_col_load(const uint32_t* col, int stride) {
  Fq12 a;
  FqE* e = reinterpret_cast<FqE*>(&a);
#pragma unroll
  for (int k = 0; k < 12; k++) {
#pragma unroll
    for (int i = 0; i < Fq::N; i++) e[k].l[i] = col[(k * Fq::N + i) * stride];
  }
  return a;
}

constexpr uint64_t BLS_X_ABS_GT = 0xd201000000010000ull;        // the curve parameter is x = -|x|
constexpr uint64_t BLS_X_ABS_P1_DIV3 = 0x460055555555aaabull;   // (|x| + 1) / 3: x = 1 mod 3
// acc <- base^e for a CONSTANT e, on the cyclotomic subgroup (fq12_cyclotomic_sqr).  Two operands of 144 registers do not stay
// resident beside a product's temporaries: the accumulator is parked in the column `acc` (LDS), the base is read from the column
// `base` (a device workspace) for every set bit.  The bits are those of a constant, so the branch is a scalar one, as in miller_lane.
GM_DEV void fq12_pow_const(uint32_t* acc, const uint32_t* base, int stride, uint64_t e) {
  fq12_col_store(acc, stride, fq12_col_load(base, stride));
#pragma unroll 1
  for (int bit = 62 - __builtin_clzll(e); bit >= 0; bit--) {
    Fq12 f = fq12_cyclotomic_sqr(fq12_col_load(acc, stride));
    if ((e >> bit) & 1ull) f = fq12_mul(f, fq12_col_load(base, stride));
    fq12_col_store(acc, stride, f);
  }
}
// acc <- base^|x|: 63 cyclotomic squarings and 5 products = 1404 Fq products.  Callers conjugate for the sign of x.
GM_DEV void fq12_pow_x(uint32_t* acc, const uint32_t* base, int stride) { fq12_pow_const(acc, base, stride, BLS_X_ABS_GT); }

constexpr int GT_BYTES = 576;  // 12 Fq records of 48 bytes in tower order, the device form of g1.cuh, fully reduced
GM_DEV Fq12 fq12_load(const void* p) {
  const char* c = reinterpret_cast<const char*>(p);
  Fq12 r;
  r.c0.c0 = fq2_load(c);
  r.c0.c1 = fq2_load(c + 96);
  r.c0.c2 = fq2_load(c + 192);
  r.c1.c0 = fq2_load(c + 288);
  r.c1.c1 = fq2_load(c + 384);
  r.c1.c2 = fq2_load(c + 480);
  return r;
}
GM_DEV void fq12_store(void* p, const Fq12& a) {
  char* c = reinterpret_cast<char*>(p);
  fq2_store(c, a.c0.c0);
  fq2_store(c + 96, a.c0.c1);
  fq2_store(c + 192, a.c0.c2);
  fq2_store(c + 288, a.c1.c0);
  fq2_store(c + 384, a.c1.c1);
  fq2_store(c + 480, a.c1.c2);
}

}  // namespace gm
