// BLS12-381 G2 group arithmetic for the G2 MSM and the herring G2Module prover (gfx950).
//
// Fq2 = Fq[u] / (u^2 + 1) on the `FqE` element layer of g1.cuh, so it follows the shipped GM_FQ30 = 2 representation
// (canonical 12 x 32-bit records, a * 2^390 at rest, the product in radix 2^30) and compiles under GM_FQ30 = 0 / 1.
// The curve is y^2 = x^3 + 4 (1 + u); a = 0, so the XYZZ formulas of g1.cuh (EFD madd-2008-s / add-2008-s / dbl-2008-s-1)
// carry over with Fq2 in the place of Fq.  A product is 3 Fq products (Karatsuba), a square 2: (a0 + a1)(a0 - a1), 2 a0 a1.
//
// Replaces: `Projective<g2::Config>::add_assign(&Affine)` / `add_assign(&Projective)` / `double_in_place` of ark-ec 0.4.2
// as used by `P::G2::msm_unchecked` (src/herring/ipa.rs:107-118, module.rs:114-124) and split_fold (time_prover.rs:72-76).
//
// Slack bounds (GM_FQ30 = 1 only; the other modes keep every element canonical and ignore K).  "< k" below means every
// component < k q.  Rules of field30.cuh: values stay < 32; fq_sub<K> needs K in {1, 2, 4, 8} and a subtrahend < K; an Fq
// product of operands < a, < b is < 2 when a b <= 512; fq_is_zero_mod needs < 16.  Hence
//   fq2_mul  : operands < A, < B with A B <= 128 (the Karatsuba sums are < 2A, < 2B)   -> c0 < 4, c1 < 6
//   fq2_sqr<K>: operand < K <= 8 (sum < 2K, difference < 2K: 4 K^2 <= 256)             -> c0 < 2, c1 < 4
// Three subtractions more per addition than in Fq push the coordinates past what the next subtraction could absorb, so the
// group law calls fq2_tighten (one product by R' mod q per component, < 2; a no-op in the canonical modes) where noted.
#pragma once
#include "g1.cuh"

namespace gm {

struct Fq2 {
  FqE c0, c1;
};

// any value < 32 -> < 2 (GM_FQ30 = 1); the canonical modes have nothing to do
GM_DEV FqE fq_tighten(const FqE& a) {
#if GM_FQ30 == 1
  return fq30_mul_fn(a, fq30_const(Fq30Consts::ONE));
#else
  return a;
#endif
}

GM_DEV Fq2 fq2_zero() {
  Fq2 r;
  r.c0 = fqe_zero();
  r.c1 = fqe_zero();
  return r;
}
GM_DEV Fq2 fq2_one() {
  Fq2 r;
  r.c0 = fqe_one();
  r.c1 = fqe_zero();
  return r;
}
GM_DEV bool fq2_is_exact_zero(const Fq2& a) { return fq_is_exact_zero(a.c0) && fq_is_exact_zero(a.c1); }
GM_DEV bool fq2_is_zero_mod(const Fq2& a) { return fq_is_zero_mod(a.c0) && fq_is_zero_mod(a.c1); }  // components < 16
GM_DEV Fq2 fq2_add(const Fq2& a, const Fq2& b) {
  Fq2 r;
  r.c0 = fq_add(a.c0, b.c0);
  r.c1 = fq_add(a.c1, b.c1);
  return r;
}
GM_DEV Fq2 fq2_dbl(const Fq2& a) { return fq2_add(a, a); }
template <int K>  // b < K
GM_DEV Fq2 fq2_sub(const Fq2& a, const Fq2& b) {
  Fq2 r;
  r.c0 = fq_sub<K>(a.c0, b.c0);
  r.c1 = fq_sub<K>(a.c1, b.c1);
  return r;
}
GM_DEV Fq2 fq2_tighten(const Fq2& a) {
  Fq2 r;
  r.c0 = fq_tighten(a.c0);
  r.c1 = fq_tighten(a.c1);
  return r;
}
// (a0 + a1 u)(b0 + b1 u) = (a0 b0 - a1 b1) + ((a0 + a1)(b0 + b1) - a0 b0 - a1 b1) u
GM_DEV Fq2 fq2_mul(const Fq2& a, const Fq2& b) {
  const FqE v0 = fq_mul(a.c0, b.c0);                                   // < 2
  const FqE v1 = fq_mul(a.c1, b.c1);                                   // < 2
  const FqE t = fq_mul(fq_add(a.c0, a.c1), fq_add(b.c0, b.c1));        // 2A 2B <= 512 -> < 2
  Fq2 r;
  r.c0 = fq_sub<2>(v0, v1);                                            // < 4
  r.c1 = fq_sub<4>(t, fq_add(v0, v1));                                 // v0 + v1 < 4 -> < 6
  return r;
}
// (a0 + a1 u)^2 = (a0 + a1)(a0 - a1) + 2 a0 a1 u
template <int K>  // a < K <= 8
GM_DEV Fq2 fq2_sqr(const Fq2& a) {
  const FqE s = fq_add(a.c0, a.c1);                                    // < 2K
  const FqE d = fq_sub<K>(a.c0, a.c1);                                 // < 2K
  const FqE m = fq_mul(a.c0, a.c1);                                    // K^2 <= 64 -> < 2
  Fq2 r;
  r.c0 = fq_mul(s, d);                                                 // 4 K^2 <= 256 -> < 2
  r.c1 = fq_dbl(m);                                                    // < 4
  return r;
}
// -a for a fully reduced a (as loaded); -0 stays the exact zero of the identity record
GM_DEV Fq2 fq2_neg_canonical(const Fq2& a) {
  Fq2 r;
  r.c0 = fq_neg_canonical(a.c0);
  r.c1 = fq_neg_canonical(a.c1);
  return r;
}
// Fq inversion by Fermat (a^(q-2)), a < 8; one per normalised point
GM_DEV FqE g2_fq_inv(const FqE& a) {
  uint32_t e[12];
#pragma unroll
  for (int i = 0; i < 12; i++) e[i] = FqParams::MOD[i];
  e[0] -= 2u;
  FqE acc = fqe_one();
  for (int i = 380; i >= 0; i--) {
    acc = fq_sqr(acc);                                                 // < 2
    if ((e[i >> 5] >> (i & 31)) & 1u) acc = fq_mul(acc, a);            // 2 * 8 -> < 2
  }
  return acc;
}
// 1 / (a0 + a1 u) = (a0 - a1 u) / (a0^2 + a1^2), a < 6 and non-zero
GM_DEV Fq2 fq2_inv(const Fq2& a) {
  const FqE n = fq_add(fq_sqr(a.c0), fq_sqr(a.c1));                    // 36 <= 512 -> < 4
  const FqE ni = g2_fq_inv(n);
  Fq2 r;
  r.c0 = fq_mul(a.c0, ni);                                             // < 2
  r.c1 = fq_sub<2>(fqe_zero(), fq_mul(a.c1, ni));                      // < 2: 0 - . + 2q
  return r;
}
GM_DEV Fq2 fq2_load(const void* p) {
  Fq2 r;
  r.c0 = fqe_load(p);
  r.c1 = fqe_load(reinterpret_cast<const char*>(p) + 48);
  return r;
}
GM_DEV void fq2_store(void* p, const Fq2& a) {
  fqe_store(p, a.c0);
  fqe_store(reinterpret_cast<char*>(p) + 48, a.c1);
}

constexpr int G2_AFF_BYTES = 192;   // x.c0 | x.c1 | y.c0 | y.c1
constexpr int G2_XYZZ_BYTES = 384;  // X | Y | ZZ | ZZZ, each c0 | c1

// Affine point, identity encoded as the all-zero record -- not on y^2 = x^3 + 4 (1 + u).  Coordinates of a loaded point are
// fully reduced (< 1).
struct G2Affine {
  Fq2 x, y;
  GM_DEV bool is_identity() const { return fq2_is_exact_zero(x) && fq2_is_exact_zero(y); }
};
GM_DEV G2Affine g2_neg_affine(const G2Affine& p) {
  G2Affine r;
  r.x = p.x;
  r.y = fq2_neg_canonical(p.y);
  return r;
}

// Invariants kept by every routine below: x, y < 2 (tightened), zz, zzz < 6; the identity is zz == 0 exactly (a
// non-identity point never has zz = 0 mod q).
struct G2Xyzz {
  Fq2 x, y, zz, zzz;
  GM_DEV bool is_identity() const { return fq2_is_exact_zero(zz); }
  static GM_DEV G2Xyzz identity() {
    G2Xyzz r;
    r.x = fq2_zero();
    r.y = fq2_zero();
    r.zz = fq2_zero();
    r.zzz = fq2_zero();
    return r;
  }
  static GM_DEV G2Xyzz from_affine(const G2Affine& p) {  // p is not the identity
    G2Xyzz r;
    r.x = p.x;
    r.y = p.y;
    r.zz = fq2_one();
    r.zzz = fq2_one();
    return r;
  }
};

// the tail shared by the two doublings: u = 2 y1 < 4, x1, y1 < 2; zz1 / zzz1 are multiplied in by the caller
GM_DEV void g2_dbl_core(const Fq2& x1, const Fq2& y1, const Fq2& u, Fq2& x3, Fq2& y3, Fq2& v, Fq2& w) {
  v = fq2_sqr<4>(u);                                                   // < 4
  w = fq2_mul(u, v);                                                   // 4 * 4 -> < 6
  const Fq2 s = fq2_mul(x1, v);                                        // 2 * 4 -> < 6
  const Fq2 xx = fq2_tighten(fq2_sqr<2>(x1));                          // < 2 (canonical modes: as computed)
  const Fq2 m = fq2_add(fq2_dbl(xx), xx);                              // < 6
  x3 = fq2_tighten(fq2_sub<8>(fq2_sub<8>(fq2_sqr<8>(m), s), s));       // 4 + 8 + 8 = 20 -> < 2
  y3 = fq2_tighten(fq2_sub<8>(fq2_mul(m, fq2_sub<2>(s, x3)), fq2_mul(w, y1)));  // (s - x3) < 8: 6 * 8; w y1: 6 * 2 -> 6 + 8 -> < 2
}

// 2 * (affine p), EFD mdbl-2008-s (a = 0)
GM_DEV G2Xyzz g2_dbl_affine(const G2Affine& p) {
  G2Xyzz r = G2Xyzz::identity();  // (one return: a second one leaves the result behind a pointer, i.e. in scratch)
  if (!(p.is_identity() || fq2_is_exact_zero(p.y))) g2_dbl_core(p.x, p.y, fq2_dbl(p.y), r.x, r.y, r.zz, r.zzz);
  return r;
}

// 2 * p, EFD dbl-2008-s-1 (a = 0)
GM_DEV G2Xyzz g2_dbl(const G2Xyzz& p) {
  G2Xyzz r = G2Xyzz::identity();
  if (!(p.is_identity() || fq2_is_zero_mod(p.y))) {
    Fq2 v, w;
    g2_dbl_core(p.x, p.y, fq2_dbl(p.y), r.x, r.y, v, w);
    r.zz = fq2_mul(v, p.zz);                                           // 4 * 6 -> < 6
    r.zzz = fq2_mul(w, p.zzz);                                         // 6 * 6 -> < 6
  }
  return r;
}

// acc += q (affine), EFD madd-2008-s with the exceptional cases resolved: accumulator identity, base identity,
// P + P -> doubling, P + (-P) -> identity.
GM_DEV void g2_madd(G2Xyzz& acc, const G2Affine& q) {
  if (q.is_identity()) return;
  if (acc.is_identity()) {
    acc = G2Xyzz::from_affine(q);
    return;
  }
  const Fq2 u2 = fq2_mul(q.x, acc.zz);                                 // 1 * 6 -> < 6
  const Fq2 s2 = fq2_mul(q.y, acc.zzz);                                // < 6
  const Fq2 p = fq2_sub<2>(u2, acc.x);                                 // < 8
  const Fq2 r = fq2_sub<2>(s2, acc.y);                                 // < 8
  if (fq2_is_zero_mod(p)) {
    if (fq2_is_zero_mod(r)) {
      acc = g2_dbl_affine(q);
    } else {
      acc = G2Xyzz::identity();
    }
    return;
  }
  // order as in xyzz_madd of g1.cuh: every Fq product is an opaque call, so this is the order that runs
  const Fq2 pp = fq2_sqr<8>(p);                                        // < 4
  acc.zz = fq2_mul(acc.zz, pp);                                        // 6 * 4 -> < 6
  const Fq2 ppp = fq2_mul(p, pp);                                      // 8 * 4 -> < 6      (p dead)
  acc.zzz = fq2_mul(acc.zzz, ppp);                                     // 6 * 6 -> < 6
  const Fq2 qq = fq2_mul(acc.x, pp);                                   // 2 * 4 -> < 6      (x, pp dead)
  const Fq2 yp = fq2_mul(acc.y, ppp);                                  // 2 * 6 -> < 6      (y dead)
  const Fq2 x3 = fq2_tighten(fq2_sub<8>(fq2_sub<8>(fq2_sub<8>(fq2_sqr<8>(r), ppp), qq), qq));  // 4 + 3 * 8 = 28 -> < 2
  acc.y = fq2_tighten(fq2_sub<8>(fq2_mul(r, fq2_sub<2>(qq, x3)), yp));  // (qq - x3) < 8: 8 * 8 -> 6 + 8 -> < 2
  acc.x = x3;
}

// acc += q (XYZZ), EFD add-2008-s with the exceptional cases resolved.
GM_DEV void g2_add(G2Xyzz& acc, const G2Xyzz& q) {
  if (q.is_identity()) return;
  if (acc.is_identity()) {
    acc = q;
    return;
  }
  const Fq2 u1 = fq2_mul(acc.x, q.zz);                                 // 2 * 6 -> < 6
  const Fq2 u2 = fq2_mul(q.x, acc.zz);
  const Fq2 s1 = fq2_mul(acc.y, q.zzz);
  const Fq2 s2 = fq2_mul(q.y, acc.zzz);
  const Fq2 p = fq2_tighten(fq2_sub<8>(u2, u1));                       // 14 -> < 2
  const Fq2 r = fq2_tighten(fq2_sub<8>(s2, s1));                       // < 2
  if (fq2_is_zero_mod(p)) {
    if (fq2_is_zero_mod(r)) {
      acc = g2_dbl(acc);
    } else {
      acc = G2Xyzz::identity();
    }
    return;
  }
  const Fq2 pp = fq2_sqr<2>(p);                                        // < 4
  const Fq2 ppp = fq2_mul(p, pp);                                      // < 6
  const Fq2 qq = fq2_mul(u1, pp);                                      // 6 * 4 -> < 6
  const Fq2 x3 = fq2_tighten(fq2_sub<8>(fq2_sub<8>(fq2_sub<8>(fq2_sqr<2>(r), ppp), qq), qq));  // 28 -> < 2
  const Fq2 y3 = fq2_tighten(fq2_sub<8>(fq2_mul(r, fq2_sub<2>(qq, x3)), fq2_mul(s1, ppp)));    // 2 * 8; 6 * 6 -> 14 -> < 2
  acc.zz = fq2_mul(fq2_mul(acc.zz, q.zz), pp);                         // 6 * 6 -> 6 * 4 -> < 6
  acc.zzz = fq2_mul(fq2_mul(acc.zzz, q.zzz), ppp);                     // < 6
  acc.x = x3;
  acc.y = y3;
}

// (X / ZZ, Y / ZZZ) with one inversion of ZZ * ZZZ; the identity gives the all-zero record
GM_DEV G2Affine g2_to_affine(const G2Xyzz& p) {
  G2Affine a;
  a.x = fq2_zero();
  a.y = fq2_zero();
  if (!p.is_identity()) {
    const Fq2 ti = fq2_inv(fq2_mul(p.zz, p.zzz));                      // 36 -> < 6; inverse < 2
    a.x = fq2_mul(p.x, fq2_mul(ti, p.zzz));                            // 2 * 6 -> 2 * 6
    a.y = fq2_mul(p.y, fq2_mul(ti, p.zz));
  }
  return a;
}

// 192-byte affine / 384-byte XYZZ memory images (16-byte aligned); values at rest are fully reduced
GM_DEV G2Affine g2_load_affine(const void* p) {
  G2Affine r;
  r.x = fq2_load(p);
  r.y = fq2_load(reinterpret_cast<const char*>(p) + 96);
  return r;
}
GM_DEV void g2_store_affine(void* p, const G2Affine& a) {
  fq2_store(p, a.x);
  fq2_store(reinterpret_cast<char*>(p) + 96, a.y);
}
GM_DEV G2Xyzz g2_load_xyzz(const void* p) {
  const char* c = reinterpret_cast<const char*>(p);
  G2Xyzz r;
  r.x = fq2_load(c);
  r.y = fq2_load(c + 96);
  r.zz = fq2_load(c + 192);
  r.zzz = fq2_load(c + 288);
  return r;
}
GM_DEV void g2_store_xyzz(void* p, const G2Xyzz& a) {
  char* c = reinterpret_cast<char*>(p);
  if (a.is_identity()) {  // keep the all-zero encoding exact
    const Fq z = Fq::zero();
#pragma unroll
    for (int k = 0; k < 8; k++) fp_store<FqParams>(c + 48 * k, z);
    return;
  }
  fq2_store(c, a.x);
  fq2_store(c + 96, a.y);
  fq2_store(c + 192, a.zz);
  fq2_store(c + 288, a.zzz);
}

}  // namespace gm
