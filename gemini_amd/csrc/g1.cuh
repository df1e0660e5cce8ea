// BLS12-381 G1 group arithmetic for the MSM kernels (gfx950).
//
// Buckets are kept in extended Jacobian ("XYZZ") coordinates: x = X/ZZ, y = Y/ZZZ with
// ZZ^3 = ZZZ^2.  A bucket += affine base costs 8M + 2S and a bucket += bucket 12M + 2S
// (EFD madd-2008-s / add-2008-s), versus 7M + 4S / 11M + 5S for the Jacobian formulas ark-ec
// uses on the CPU.  All additions are COMPLETE through explicit branches: the benchmark
// inputs of the reference are exactly the degenerate ones (dummy_r1cs makes every scalar
// equal, src/circuit.rs:349-365; the elastic example makes every base the generator,
// examples/snark.rs:59-63), so P + P and P - P do occur inside buckets.
//
// Replaces: `Projective<P>::add_assign(&Affine)` / `add_assign(&Projective)` /
// `double_in_place` of ark-ec 0.4.2 as used by VariableBaseMSM::msm_bigint
// (in-tree statement: src/kzg/msm/variable_base.rs:125-175).
//
// Coordinate arithmetic goes through the `FqE` element layer below.  There is ONE representation: an element is the
// canonical (fully reduced) 12 x 32-bit record of field.cuh, and only the PRODUCT runs in radix 2^30 (field30.cuh) -- with
// 30-bit limbs a partial product is one v_mad_u64_u32 and no carry instruction, which beats the 32-bit multiplier's
// mad + addc pair, both half rate on gfx950.  That product's Montgomery factor is 2^390, so every device-resident
// coordinate (bases, buckets, partials, tables) is a * 2^390 mod q; conversion from / to ark-ff's a * 2^384 happens once
// at the boundary (k_pack_bases, k_export_bases, host plane conversion).  The two alternatives that were measured and
// dropped (the 32-bit multiplier; 13-limb loose elements held in registers) are recorded in HISTORY.md.
#pragma once
#include "field.cuh"
#include "field30.cuh"

namespace gm {

// ---- element layer.  FqE is an Fq in the device's Montgomery form, a * 2^390 mod q: the same C++ type as the ark-ff form
// a * 2^384 and a different number, hence the name.  Additions, subtractions, comparisons and memory are those of
// field.cuh; the product unpacks both operands to 13 x 30-bit limbs, runs the lazy-carry Montgomery product with
// R' = 2^390, subtracts q once if needed (canonical inputs give < 1.002 q) and repacks.
using FqE = Fq;
// fq30h_mul_fn / fq30h_sqr_fn: one asm statement each on physical registers (gen_field_mul30.py)
#include "field_mul30_gen.inc"
GM_DEV FqE fq_mul(const FqE& a, const FqE& b) {
  return fq30h_mul_fn(a.l[0], a.l[1], a.l[2], a.l[3], a.l[4], a.l[5], a.l[6], a.l[7], a.l[8], a.l[9], a.l[10], a.l[11], b.l[0], b.l[1], b.l[2], b.l[3],
                      b.l[4], b.l[5], b.l[6], b.l[7], b.l[8], b.l[9], b.l[10], b.l[11]);
}
GM_DEV FqE fq_sqr(const FqE& a) {
  return fq30h_sqr_fn(a.l[0], a.l[1], a.l[2], a.l[3], a.l[4], a.l[5], a.l[6], a.l[7], a.l[8], a.l[9], a.l[10], a.l[11]);
}
GM_DEV FqE fq_add(const FqE& a, const FqE& b) { return fp_add<FqParams>(a, b); }
GM_DEV FqE fq_dbl(const FqE& a) { return fp_add<FqParams>(a, a); }
GM_DEV FqE fq_sub(const FqE& a, const FqE& b) { return fp_sub<FqParams>(a, b); }
GM_DEV FqE fq_neg_canonical(const FqE& y) { return fp_neg<FqParams>(y); }
GM_DEV bool fq_is_zero(const FqE& a) { return a.is_zero(); }
// the limbs as an integer: >= q?  (untrusted host input: the point checks of points.hip, the GT check of pairing.hip)
GM_DEV bool pt_raw_ge_q(const Fq& a) {
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 12; i++) {
    uint32_t b;
    (void)__builtin_subc(a.l[i], FqParams::MOD[i], borrow, &b);
    borrow = b;
  }
  return borrow == 0;
}
GM_DEV FqE fqe_zero() { return Fq::zero(); }
GM_DEV FqE fqe_one() { return fq30_pack(fq30_const(Fq30Consts::ONE)); }  // 2^390 mod q -- NOT Fq::one(), which is 2^384 mod q
GM_DEV FqE fqe_load(const void* p) { return fp_load<FqParams>(p); }
GM_DEV void fqe_store(void* p, const FqE& a) { fp_store<FqParams>(p, a); }
// ark-ff form (a * 2^384) <-> device form (a * 2^390)
GM_DEV FqE fqe_import(const Fq& ark) { return fq_mul(ark, fq30_pack(fq30_const(Fq30Consts::CIN))); }
GM_DEV Fq fqe_export(const FqE& dev) { return fq_mul(dev, fq30_pack(fq30_const(Fq30Consts::COUT))); }
// Fq inversion by Fermat (a^(q-2)): one per normalised point or group of points
GM_DEV FqE fq_inv(const FqE& a) {
  // q - 2, little-endian 32-bit limbs
  uint32_t e[12];
#pragma unroll
  for (int i = 0; i < 12; i++) e[i] = FqParams::MOD[i];
  e[0] -= 2u;
  FqE acc = fqe_one();
  for (int i = 380; i >= 0; i--) {
    acc = fq_sqr(acc);
    if ((e[i >> 5] >> (i & 31)) & 1u) acc = fq_mul(acc, a);
  }
  return acc;
}

// ---- the bucket accumulator of k_acc0 lives in the product's own representation: 13 x 30-bit LOOSE limbs (field30.cuh),
// the whole mixed addition one asm statement (gen_madd30.py).  Buckets and level-0 partials are written as 208-byte
// records of 4 x 13 limbs (X, Y, ZZ, ZZZ; any representative < 2^386 of the residue; the identity is ZZ == 0 exactly)
// and canonicalised by their consumers (k_merge, k_group_sum) on load: one product by R' mod q per coordinate.
#include "field_mul30l_gen.inc"  // fq30_mul_asm / fq30_sqr_asm: the loose product on registers, out of line
#include "g1_madd30_gen.inc"     // Acc30, g1_madd30_asm
constexpr int XYZZ30_BYTES = 208;

GM_DEV Fq fq30_loose_to_canonical(const Fq30& v) {
  const uint32_t* o = Fq30Consts::ONE;
  Fq30 t = fq30_mul_asm(v.l[0], v.l[1], v.l[2], v.l[3], v.l[4], v.l[5], v.l[6], v.l[7], v.l[8], v.l[9], v.l[10], v.l[11], v.l[12],
                        o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], o[10], o[11], o[12]);
  return fq30_pack(fq30_canonical_tail(t));  // < q + v q / 2^390 < 1.07 q before the conditional subtraction
}
GM_DEV uint32_t acc30_limb(const Acc30& A, int i) {
  return i < 8 ? A.a0[i] : i < 16 ? A.a1[i - 8] : i < 24 ? A.a2[i - 16] : i < 32 ? A.a3[i - 24] : i < 40 ? A.a4[i - 32] : i < 48 ? A.a5[i - 40] : A.a6[i - 48];
}
GM_DEV void acc30_set_limb(Acc30& A, int i, uint32_t v) {
  if (i < 8) A.a0[i] = v;
  else if (i < 16) A.a1[i - 8] = v;
  else if (i < 24) A.a2[i - 16] = v;
  else if (i < 32) A.a3[i - 24] = v;
  else if (i < 40) A.a4[i - 32] = v;
  else if (i < 48) A.a5[i - 40] = v;
  else A.a6[i - 48] = v;
}
GM_DEV void acc30_zero(Acc30& A) {
  A.a0 = A.a1 = A.a2 = A.a3 = A.a4 = A.a5 = gm_u8v{0, 0, 0, 0, 0, 0, 0, 0};
  A.a6 = gm_u4v{0, 0, 0, 0};
}
// limbs 26..38 are ZZ
GM_DEV void acc30_set_identity(Acc30& A) {
#pragma unroll
  for (int i = 26; i < 39; i++) acc30_set_limb(A, i, 0u);
}
GM_DEV void acc30_store(void* p, const Acc30& A) {
  gm_u4v* o = reinterpret_cast<gm_u4v*>(p);
  o[0] = A.a0.lo; o[1] = A.a0.hi; o[2] = A.a1.lo; o[3] = A.a1.hi; o[4] = A.a2.lo; o[5] = A.a2.hi; o[6] = A.a3.lo;
  o[7] = A.a3.hi; o[8] = A.a4.lo; o[9] = A.a4.hi; o[10] = A.a5.lo; o[11] = A.a5.hi; o[12] = A.a6;
}

// Affine point, identity encoded as (0, 0) -- not on y^2 = x^3 + 4, hence unambiguous.
struct G1Affine {
  FqE x, y;
  GM_DEV bool is_identity() const { return fq_is_zero(x) && fq_is_zero(y); }
};

// Every value in the group law below -- coordinates and temporaries alike -- is fully reduced (< q).  The identity is
// the all-zero record (zz == 0 -- a non-identity point never has zz = 0).
struct G1Xyzz {
  FqE x, y, zz, zzz;
  GM_DEV bool is_identity() const { return fq_is_zero(zz); }
  static GM_DEV G1Xyzz identity() {
    G1Xyzz r;
    r.x = fqe_zero();
    r.y = fqe_zero();
    r.zz = fqe_zero();
    r.zzz = fqe_zero();
    return r;
  }
  static GM_DEV G1Xyzz from_affine(const G1Affine& p) {
    G1Xyzz r;
    if (p.is_identity()) return identity();
    r.x = p.x;
    r.y = p.y;
    r.zz = fqe_one();
    r.zzz = fqe_one();
    return r;
  }
};

// 2 * (affine p), EFD mdbl-2008-s (a = 0)
GM_DEV G1Xyzz xyzz_dbl_affine(const G1Affine& p) {
  if (p.is_identity() || fq_is_zero(p.y)) return G1Xyzz::identity();
  G1Xyzz r;
  FqE u = fq_dbl(p.y);
  FqE v = fq_sqr(u);
  FqE w = fq_mul(u, v);
  FqE s = fq_mul(p.x, v);
  FqE xx = fq_sqr(p.x);
  FqE m = fq_add(fq_dbl(xx), xx);
  r.x = fq_sub(fq_sqr(m), fq_dbl(s));
  r.y = fq_sub(fq_mul(m, fq_sub(s, r.x)), fq_mul(w, p.y));
  r.zz = v;
  r.zzz = w;
  return r;
}

// 2 * p, EFD dbl-2008-s-1 (a = 0)
GM_DEV G1Xyzz xyzz_dbl(const G1Xyzz& p) {
  if (p.is_identity() || fq_is_zero(p.y)) return G1Xyzz::identity();
  G1Xyzz r;
  FqE u = fq_dbl(p.y);
  FqE v = fq_sqr(u);
  FqE w = fq_mul(u, v);
  FqE s = fq_mul(p.x, v);
  FqE xx = fq_sqr(p.x);
  FqE m = fq_add(fq_dbl(xx), xx);
  r.x = fq_sub(fq_sqr(m), fq_dbl(s));
  r.y = fq_sub(fq_mul(m, fq_sub(s, r.x)), fq_mul(w, p.y));
  r.zz = fq_mul(v, p.zz);
  r.zzz = fq_mul(w, p.zzz);
  return r;
}

// acc += q (affine), EFD madd-2008-s with the exceptional cases resolved.
GM_DEV void xyzz_madd(G1Xyzz& acc, const G1Affine& q) {
  if (q.is_identity()) return;
  if (acc.is_identity()) {
    acc = G1Xyzz::from_affine(q);
    return;
  }
  FqE u2 = fq_mul(q.x, acc.zz);
  FqE s2 = fq_mul(q.y, acc.zzz);
  FqE p = fq_sub(u2, acc.x);
  FqE r = fq_sub(s2, acc.y);
  if (fq_is_zero(p)) {
    if (fq_is_zero(r)) {
      acc = xyzz_dbl_affine(q);
    } else {
      acc = G1Xyzz::identity();
    }
    return;
  }
  // Order chosen for register pressure (every product is an opaque call, so this is the order that runs): at most
  // eight field elements are live at any call -- k_acc0 fits three waves per SIMD only below 168 VGPRs.
  FqE pp = fq_sqr(p);
  acc.zz = fq_mul(acc.zz, pp);
  FqE ppp = fq_mul(p, pp);  // (p dead)
  acc.zzz = fq_mul(acc.zzz, ppp);
  FqE qq = fq_mul(acc.x, pp);  // (x, pp dead)
  FqE yp = fq_mul(acc.y, ppp);  // (y dead)
  FqE x3 = fq_sub(fq_sub(fq_sqr(r), ppp), fq_dbl(qq));  // (ppp dead)
  acc.y = fq_sub(fq_mul(r, fq_sub(qq, x3)), yp);
  acc.x = x3;
}

// acc += q (XYZZ), EFD add-2008-s with the exceptional cases resolved.
GM_DEV void xyzz_add(G1Xyzz& acc, const G1Xyzz& q) {
  if (q.is_identity()) return;
  if (acc.is_identity()) {
    acc = q;
    return;
  }
  FqE u1 = fq_mul(acc.x, q.zz);
  FqE u2 = fq_mul(q.x, acc.zz);
  FqE s1 = fq_mul(acc.y, q.zzz);
  FqE s2 = fq_mul(q.y, acc.zzz);
  FqE p = fq_sub(u2, u1);
  FqE r = fq_sub(s2, s1);
  if (fq_is_zero(p)) {
    if (fq_is_zero(r)) {
      acc = xyzz_dbl(acc);
    } else {
      acc = G1Xyzz::identity();
    }
    return;
  }
  FqE pp = fq_sqr(p);
  FqE ppp = fq_mul(p, pp);
  FqE qq = fq_mul(u1, pp);
  FqE x3 = fq_sub(fq_sub(fq_sqr(r), ppp), fq_dbl(qq));
  FqE y3 = fq_sub(fq_mul(r, fq_sub(qq, x3)), fq_mul(s1, ppp));
  acc.zz = fq_mul(fq_mul(acc.zz, q.zz), pp);
  acc.zzz = fq_mul(fq_mul(acc.zzz, q.zzz), ppp);
  acc.x = x3;
  acc.y = y3;
}

// k * p for the 256-bit integer k at s8 (8 x u32, least significant first), most significant bit first.  Nothing here is secret:
// the doublings in front of the first set bit return at once (the identity), so a short scalar is a short loop.  k = 0 and the
// identity give the identity; the additions are xyzz_madd's, complete.
GM_DEV G1Xyzz xyzz_scalar_mul(const G1Affine& p, const uint32_t* __restrict__ s8) {
  G1Xyzz acc = G1Xyzz::identity();
  if (p.is_identity()) return acc;
#pragma unroll 1
  for (int w = 7; w >= 0; w--) {
    const uint32_t word = s8[w];
#pragma unroll 1
    for (int bit = 31; bit >= 0; bit--) {
      acc = xyzz_dbl(acc);
      if ((word >> bit) & 1u) xyzz_madd(acc, p);
    }
  }
  return acc;
}

// 96-byte affine / 192-byte XYZZ memory images (AoS, 16-byte aligned -> dwordx4 accesses); values at
// rest are fully reduced
GM_DEV G1Affine g1_load_affine(const void* p) {
  G1Affine r;
  r.x = fqe_load(p);
  r.y = fqe_load(reinterpret_cast<const char*>(p) + 48);
  return r;
}
GM_DEV void g1_store_affine(void* p, const G1Affine& a) {
  fqe_store(p, a.x);
  fqe_store(reinterpret_cast<char*>(p) + 48, a.y);
}
GM_DEV G1Xyzz g1_load_xyzz(const void* p) {
  const char* c = reinterpret_cast<const char*>(p);
  G1Xyzz r;
  r.x = fqe_load(c);
  r.y = fqe_load(c + 48);
  r.zz = fqe_load(c + 96);
  r.zzz = fqe_load(c + 144);
  return r;
}
GM_DEV void g1_store_xyzz(void* p, const G1Xyzz a) {
  char* c = reinterpret_cast<char*>(p);
  if (a.is_identity()) {  // keep the all-zero encoding exact
    const Fq z = Fq::zero();
    fp_store<FqParams>(c, z);
    fp_store<FqParams>(c + 48, z);
    fp_store<FqParams>(c + 96, z);
    fp_store<FqParams>(c + 144, z);
    return;
  }
  fqe_store(c, a.x);
  fqe_store(c + 48, a.y);
  fqe_store(c + 96, a.zz);
  fqe_store(c + 144, a.zzz);
}

// 208-byte loose record (see Acc30) -> canonical XYZZ
GM_DEV G1Xyzz g1_load_xyzz30(const void* p) {
  const gm_u4v* s = reinterpret_cast<const gm_u4v*>(p);
  uint32_t w[52];
#pragma unroll
  for (int i = 0; i < 13; i++) {
    const gm_u4v v = s[i];
    w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
  }
  uint32_t zz = 0;
#pragma unroll
  for (int i = 26; i < 39; i++) zz |= w[i];
  if (zz == 0) return G1Xyzz::identity();
  G1Xyzz r;
  Fq30 t;
#pragma unroll
  for (int i = 0; i < 13; i++) t.l[i] = w[i];
  r.x = fq30_loose_to_canonical(t);
#pragma unroll
  for (int i = 0; i < 13; i++) t.l[i] = w[13 + i];
  r.y = fq30_loose_to_canonical(t);
#pragma unroll
  for (int i = 0; i < 13; i++) t.l[i] = w[26 + i];
  r.zz = fq30_loose_to_canonical(t);
#pragma unroll
  for (int i = 0; i < 13; i++) t.l[i] = w[39 + i];
  r.zzz = fq30_loose_to_canonical(t);
  return r;
}
// canonical XYZZ -> 208-byte record (limbs of the canonical values)
GM_DEV void g1_store_xyzz30(void* p, const G1Xyzz& a) {
  gm_u4v* o = reinterpret_cast<gm_u4v*>(p);
  uint32_t w[52];
  if (a.is_identity()) {
#pragma unroll
    for (int i = 0; i < 52; i++) w[i] = 0;
  } else {
    const Fq30 x = fq30_unpack(a.x), y = fq30_unpack(a.y), zz = fq30_unpack(a.zz), zzz = fq30_unpack(a.zzz);
#pragma unroll
    for (int i = 0; i < 13; i++) {
      w[i] = x.l[i]; w[13 + i] = y.l[i]; w[26 + i] = zz.l[i]; w[39 + i] = zzz.l[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 13; i++) o[i] = gm_u4v{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]};
}
GM_DEV G1Xyzz acc30_to_canonical(const Acc30& A) {
  uint32_t zz = 0;
#pragma unroll
  for (int i = 26; i < 39; i++) zz |= acc30_limb(A, i);
  if (zz == 0) return G1Xyzz::identity();
  G1Xyzz r;
  Fq30 t;
#pragma unroll
  for (int i = 0; i < 13; i++) t.l[i] = acc30_limb(A, i);
  r.x = fq30_loose_to_canonical(t);
#pragma unroll
  for (int i = 0; i < 13; i++) t.l[i] = acc30_limb(A, 13 + i);
  r.y = fq30_loose_to_canonical(t);
#pragma unroll
  for (int i = 0; i < 13; i++) t.l[i] = acc30_limb(A, 26 + i);
  r.zz = fq30_loose_to_canonical(t);
#pragma unroll
  for (int i = 0; i < 13; i++) t.l[i] = acc30_limb(A, 39 + i);
  r.zzz = fq30_loose_to_canonical(t);
  return r;
}
GM_DEV void acc30_from_canonical(Acc30& A, const G1Xyzz& c) {
  if (c.is_identity()) {
    acc30_zero(A);
    return;
  }
  const Fq30 x = fq30_unpack(c.x), y = fq30_unpack(c.y), zz = fq30_unpack(c.zz), zzz = fq30_unpack(c.zzz);
#pragma unroll
  for (int i = 0; i < 13; i++) {
    acc30_set_limb(A, i, x.l[i]);
    acc30_set_limb(A, 13 + i, y.l[i]);
    acc30_set_limb(A, 26 + i, zz.l[i]);
    acc30_set_limb(A, 39 + i, zzz.l[i]);
  }
}
GM_DEV void acc30_load(Acc30& A, const void* p) {
  const gm_u4v* s = reinterpret_cast<const gm_u4v*>(p);
  const gm_u4v v0 = s[0], v1 = s[1], v2 = s[2], v3 = s[3], v4 = s[4], v5 = s[5], v6 = s[6], v7 = s[7], v8 = s[8], v9 = s[9], v10 = s[10], v11 = s[11];
  A.a0 = __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
  A.a1 = __builtin_shufflevector(v2, v3, 0, 1, 2, 3, 4, 5, 6, 7);
  A.a2 = __builtin_shufflevector(v4, v5, 0, 1, 2, 3, 4, 5, 6, 7);
  A.a3 = __builtin_shufflevector(v6, v7, 0, 1, 2, 3, 4, 5, 6, 7);
  A.a4 = __builtin_shufflevector(v8, v9, 0, 1, 2, 3, 4, 5, 6, 7);
  A.a5 = __builtin_shufflevector(v10, v11, 0, 1, 2, 3, 4, 5, 6, 7);
  A.a6 = s[12];
}
GM_DEV bool acc30_is_identity(const Acc30& A) {
  uint32_t zz = 0;
#pragma unroll
  for (int i = 26; i < 39; i++) zz |= acc30_limb(A, i);
  return zz == 0;
}
GM_DEV void acc30_shfl_xor(Acc30& d, const Acc30& s, int m) {
#pragma unroll
  for (int i = 0; i < 52; i++) acc30_set_limb(d, i, __shfl_xor(acc30_limb(s, i), m));
}
// acc += o, both loose XYZZ (o is consumed).  The statement (gen_madd30.py: gen_add) is complete: identity operands,
// doubling and cancellation are handled inside it.
GM_DEV void acc30_add(Acc30& acc, Acc30& o) { (void)g1_add30_asm(acc, o); }

}  // namespace gm
