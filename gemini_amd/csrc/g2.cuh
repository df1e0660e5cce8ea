// BLS12-381 G2 group arithmetic for the G2 MSM and the herring G2Module prover (gfx950).
//
// Fq2 = Fq[u] / (u^2 + 1) on the `FqE` element layer of g1.cuh: canonical 12 x 32-bit records, a * 2^390 at rest, the product
// in radix 2^30.  Every value below -- coordinates and temporaries alike -- is fully reduced (< q per component).
// The curve is y^2 = x^3 + 4 (1 + u); a = 0, so the XYZZ formulas of g1.cuh (EFD madd-2008-s / add-2008-s / dbl-2008-s-1)
// carry over with Fq2 in the place of Fq.  A product is 3 Fq products (Karatsuba), a square 2: (a0 + a1)(a0 - a1), 2 a0 a1.
//
// Replaces: `Projective<g2::Config>::add_assign(&Affine)` / `add_assign(&Projective)` / `double_in_place` of ark-ec 0.4.2
// as used by `P::G2::msm_unchecked` (src/herring/ipa.rs:107-118, module.rs:114-124) and split_fold (time_prover.rs:72-76).
#pragma once
#include "g1.cuh"

namespace gm {

struct Fq2 {
  FqE c0, c1;
};

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
GM_DEV bool fq2_is_zero(const Fq2& a) { return fq_is_zero(a.c0) && fq_is_zero(a.c1); }
GM_DEV Fq2 fq2_add(const Fq2& a, const Fq2& b) {
  Fq2 r;
  r.c0 = fq_add(a.c0, b.c0);
  r.c1 = fq_add(a.c1, b.c1);
  return r;
}
GM_DEV Fq2 fq2_dbl(const Fq2& a) { return fq2_add(a, a); }
GM_DEV Fq2 fq2_sub(const Fq2& a, const Fq2& b) {
  Fq2 r;
  r.c0 = fq_sub(a.c0, b.c0);
  r.c1 = fq_sub(a.c1, b.c1);
  return r;
}
// (a0 + a1 u)(b0 + b1 u) = (a0 b0 - a1 b1) + ((a0 + a1)(b0 + b1) - a0 b0 - a1 b1) u
GM_DEV Fq2 fq2_mul(const Fq2& a, const Fq2& b) {
  const FqE v0 = fq_mul(a.c0, b.c0);
  const FqE v1 = fq_mul(a.c1, b.c1);
  const FqE t = fq_mul(fq_add(a.c0, a.c1), fq_add(b.c0, b.c1));
  Fq2 r;
  r.c0 = fq_sub(v0, v1);
  r.c1 = fq_sub(t, fq_add(v0, v1));
  return r;
}
// (a0 + a1 u)^2 = (a0 + a1)(a0 - a1) + 2 a0 a1 u
GM_DEV Fq2 fq2_sqr(const Fq2& a) {
  const FqE s = fq_add(a.c0, a.c1);
  const FqE d = fq_sub(a.c0, a.c1);
  const FqE m = fq_mul(a.c0, a.c1);
  Fq2 r;
  r.c0 = fq_mul(s, d);
  r.c1 = fq_dbl(m);
  return r;
}
// -a for a fully reduced a (as loaded); -0 stays the exact zero of the identity record
GM_DEV Fq2 fq2_neg_canonical(const Fq2& a) {
  Fq2 r;
  r.c0 = fq_neg_canonical(a.c0);
  r.c1 = fq_neg_canonical(a.c1);
  return r;
}
// 1 / (a0 + a1 u) = (a0 - a1 u) / (a0^2 + a1^2), a non-zero
GM_DEV Fq2 fq2_inv(const Fq2& a) {
  const FqE n = fq_add(fq_sqr(a.c0), fq_sqr(a.c1));
  const FqE ni = fq_inv(n);
  Fq2 r;
  r.c0 = fq_mul(a.c0, ni);
  r.c1 = fq_sub(fqe_zero(), fq_mul(a.c1, ni));
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

// Affine point, identity encoded as the all-zero record -- not on y^2 = x^3 + 4 (1 + u).
struct G2Affine {
  Fq2 x, y;
  GM_DEV bool is_identity() const { return fq2_is_zero(x) && fq2_is_zero(y); }
};
GM_DEV G2Affine g2_neg_affine(const G2Affine& p) {
  G2Affine r;
  r.x = p.x;
  r.y = fq2_neg_canonical(p.y);
  return r;
}

// The identity is zz == 0 (a non-identity point never has zz = 0).
struct G2Xyzz {
  Fq2 x, y, zz, zzz;
  GM_DEV bool is_identity() const { return fq2_is_zero(zz); }
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

// the tail shared by the two doublings: u = 2 y1; zz1 / zzz1 are multiplied in by the caller
GM_DEV void g2_dbl_core(const Fq2& x1, const Fq2& y1, const Fq2& u, Fq2& x3, Fq2& y3, Fq2& v, Fq2& w) {
  v = fq2_sqr(u);
  w = fq2_mul(u, v);
  const Fq2 s = fq2_mul(x1, v);
  const Fq2 xx = fq2_sqr(x1);
  const Fq2 m = fq2_add(fq2_dbl(xx), xx);
  x3 = fq2_sub(fq2_sub(fq2_sqr(m), s), s);
  y3 = fq2_sub(fq2_mul(m, fq2_sub(s, x3)), fq2_mul(w, y1));
}

// 2 * (affine p), EFD mdbl-2008-s (a = 0)
GM_DEV G2Xyzz g2_dbl_affine(const G2Affine& p) {
  G2Xyzz r = G2Xyzz::identity();  // (one return: a second one leaves the result behind a pointer, i.e. in scratch)
  if (!(p.is_identity() || fq2_is_zero(p.y))) g2_dbl_core(p.x, p.y, fq2_dbl(p.y), r.x, r.y, r.zz, r.zzz);
  return r;
}

// 2 * p, EFD dbl-2008-s-1 (a = 0)
GM_DEV G2Xyzz g2_dbl(const G2Xyzz& p) {
  G2Xyzz r = G2Xyzz::identity();
  if (!(p.is_identity() || fq2_is_zero(p.y))) {
    Fq2 v, w;
    g2_dbl_core(p.x, p.y, fq2_dbl(p.y), r.x, r.y, v, w);
    r.zz = fq2_mul(v, p.zz);
    r.zzz = fq2_mul(w, p.zzz);
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
  const Fq2 u2 = fq2_mul(q.x, acc.zz);
  const Fq2 s2 = fq2_mul(q.y, acc.zzz);
  const Fq2 p = fq2_sub(u2, acc.x);
  const Fq2 r = fq2_sub(s2, acc.y);
  if (fq2_is_zero(p)) {
    if (fq2_is_zero(r)) {
      acc = g2_dbl_affine(q);
    } else {
      acc = G2Xyzz::identity();
    }
    return;
  }
  // order as in xyzz_madd of g1.cuh: every Fq product is an opaque call, so this is the order that runs
  const Fq2 pp = fq2_sqr(p);
  acc.zz = fq2_mul(acc.zz, pp);
  const Fq2 ppp = fq2_mul(p, pp);  // (p dead)
  acc.zzz = fq2_mul(acc.zzz, ppp);
  const Fq2 qq = fq2_mul(acc.x, pp);  // (x, pp dead)
  const Fq2 yp = fq2_mul(acc.y, ppp);  // (y dead)
  const Fq2 x3 = fq2_sub(fq2_sub(fq2_sub(fq2_sqr(r), ppp), qq), qq);
  acc.y = fq2_sub(fq2_mul(r, fq2_sub(qq, x3)), yp);
  acc.x = x3;
}

// acc += q (XYZZ), EFD add-2008-s with the exceptional cases resolved.
GM_DEV void g2_add(G2Xyzz& acc, const G2Xyzz& q) {
  if (q.is_identity()) return;
  if (acc.is_identity()) {
    acc = q;
    return;
  }
  const Fq2 u1 = fq2_mul(acc.x, q.zz);
  const Fq2 u2 = fq2_mul(q.x, acc.zz);
  const Fq2 s1 = fq2_mul(acc.y, q.zzz);
  const Fq2 s2 = fq2_mul(q.y, acc.zzz);
  const Fq2 p = fq2_sub(u2, u1);
  const Fq2 r = fq2_sub(s2, s1);
  if (fq2_is_zero(p)) {
    if (fq2_is_zero(r)) {
      acc = g2_dbl(acc);
    } else {
      acc = G2Xyzz::identity();
    }
    return;
  }
  const Fq2 pp = fq2_sqr(p);
  const Fq2 ppp = fq2_mul(p, pp);
  const Fq2 qq = fq2_mul(u1, pp);
  const Fq2 x3 = fq2_sub(fq2_sub(fq2_sub(fq2_sqr(r), ppp), qq), qq);
  const Fq2 y3 = fq2_sub(fq2_mul(r, fq2_sub(qq, x3)), fq2_mul(s1, ppp));
  acc.zz = fq2_mul(fq2_mul(acc.zz, q.zz), pp);
  acc.zzz = fq2_mul(fq2_mul(acc.zzz, q.zzz), ppp);
  acc.x = x3;
  acc.y = y3;
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
