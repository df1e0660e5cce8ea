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
