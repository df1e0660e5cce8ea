// Fq in radix 2^30: 13 limbs, lazy carries, Montgomery factor R' = 2^390 -- the representation INSIDE the Fq product of
// g1.cuh and inside the bucket accumulator of k_acc0.  Elements everywhere else are the canonical 12 x 32-bit records of
// field.cuh.
//
// Why the product runs here: on gfx950 v_mad_u64_u32 AND v_addc_co_u32 both issue at half rate
// (tools/ubench_isa.hip), so the 32-bit-limb product-scanning multiplier of field.cuh pays two
// half-rate instructions per partial product (accumulate + carry fold).  With 30-bit limbs thirteen
// 60-bit products fit a 64-bit accumulator, so a partial product is ONE v_mad_u64_u32 and carries
// are extracted once per column with full-rate shifts/ands: 2 x 169 mads instead of 2 x (144 mads
// + 144 addc).  fq30_mul below is the plain-C statement of that product; the kernels call the generated
// asm statements (gen_field_mul30.py, gen_madd30.py), which compute the same thing on physical registers.
//
// "Loose" values: the integer v = sum l_i 2^(30 i) represents v mod q and is only required to stay below
// 2^386 (32 q); R' = 2^390 leaves so much headroom that the Montgomery product of two loose values is < 3q
// WITHOUT any conditional subtraction.  That discipline applies only to the Acc30 accumulator of k_acc0, its
// generated statements and the 208-byte records they write (g1.cuh); their consumers canonicalise on load
// (fq30_canonical_tail) and everything else on the device is fully reduced.
//
// Memory/ABI note: ark-ff keeps a*2^384 mod q.  Device-resident data (bases, buckets, partials, tables)
// holds a*2^390 mod q instead; conversion is one multiplication by a constant at the boundary
// (k_pack_bases on the way in, the host on the way out).
#pragma once
#include "field.cuh"

namespace gm {

struct Fq30Params {
  static constexpr int N = 13;
  static constexpr uint32_t MASK = (1u << 30) - 1u;
  // q in radix 2^30
  static constexpr uint32_t MOD[13] = {0x3fffaaabu, 0x27fbffffu, 0x153ffffbu, 0x2affffacu, 0x30f6241eu, 0x034a83dau, 0x112bf673u, 0x12e13ce1u, 0x2cd76477u, 0x1ed90d2eu, 0x29a4b1bau, 0x3a8e5ff9u, 0x001a0111u};
  static constexpr uint32_t INV = 0x3ffcfffdu;  // -q^{-1} mod 2^30
};

struct Fq30 {
  uint32_t l[13];
  static GM_DEV Fq30 zero() {
    Fq30 r;
#pragma unroll
    for (int i = 0; i < 13; i++) r.l[i] = 0;
    return r;
  }
};

// Montgomery product a*b*2^-390 for normalised inputs (every limb < 2^30, value < 2^386); output
// normalised, value < 3q.  13*2^60 + 2^35 < 2^64 bounds every column accumulator.
GM_DEV Fq30 fq30_mul(const Fq30& a, const Fq30& b) {
  using P = Fq30Params;
  uint32_t t[26];
  uint64_t acc = 0;
#pragma unroll
  for (int k = 0; k < 25; k++) {
#pragma unroll
    for (int i = (k > 12 ? k - 12 : 0); i <= (k < 12 ? k : 12); i++) acc += (uint64_t)a.l[i] * b.l[k - i];
    t[k] = (uint32_t)acc & P::MASK;
    acc >>= 30;
  }
  t[25] = (uint32_t)acc;
  // reduction: for k < 13 choose m_k so that column k vanishes mod 2^30
  uint32_t m[13];
  Fq30 r;
  acc = 0;
#pragma unroll
  for (int k = 0; k < 26; k++) {
    acc += t[k];
#pragma unroll
    for (int i = (k > 12 ? k - 12 : 0); i <= (k < 13 ? k - 1 : 12); i++) acc += (uint64_t)m[i] * P::MOD[k - i];
    if (k < 13) {
      m[k] = ((uint32_t)acc * P::INV) & P::MASK;
      acc += (uint64_t)m[k] * P::MOD[0];
    } else {
      r.l[k - 13] = (uint32_t)acc & P::MASK;
    }
    acc >>= 30;
  }
  return r;
}
GM_DEV Fq30 fq30_sqr(const Fq30& a) { return fq30_mul(a, a); }

struct Fq30Consts {
  // R' mod q (the Montgomery one), 2^396 mod q (ark-ff 2^384-form -> 2^390-form), 2^384 mod q (back)
  static constexpr uint32_t ONE[13] = {0x00d1ff2eu, 0x19d80000u, 0x34800ac4u, 0x2e00cde6u, 0x02431c84u, 0x269f83a2u, 0x3dcf80ddu, 0x09b42da0u, 0x25eec26cu, 0x15d98f12u, 0x04b29f14u, 0x259fcfa0u, 0x00015de9u};
  static constexpr uint32_t CIN[13] = {0x3480cb7fu, 0x3e0c0000u, 0x2042b126u, 0x3f337aafu, 0x3de4b4d1u, 0x1e015cf1u, 0x005c540du, 0x3467b19au, 0x352a6da3u, 0x19d89d19u, 0x2fb9afe6u, 0x3848c817u, 0x0009772fu};
  static constexpr uint32_t COUT[13] = {0x0002fffdu, 0x18240000u, 0x00c00027u, 0x3d0002f1u, 0x0758baebu, 0x22615d4fu, 0x257455f4u, 0x1614dc14u, 0x2c6d77ceu, 0x2a5e895bu, 0x0935c071u, 0x30fea039u, 0x0015f65eu};
};
GM_DEV Fq30 fq30_const(const uint32_t (&c)[13]) {
  Fq30 r;
#pragma unroll
  for (int i = 0; i < 13; i++) r.l[i] = c[i];
  return r;
}

// fully reduced representative (< q) of a normalised loose value < 16 q: one product by R' mod q
// brings it below 1.04 q, then a single conditional subtraction
// fq30_canonical_tail takes the product a * ONE (computed by the caller, possibly out of line)
GM_DEV Fq30 fq30_canonical_tail(Fq30 r) {
  uint32_t d[13];
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 13; i++) {
    const uint32_t v = r.l[i] - Fq30Params::MOD[i] - borrow;
    borrow = v >> 31;
    d[i] = i < 12 ? (v & Fq30Params::MASK) : v;
  }
#pragma unroll
  for (int i = 0; i < 13; i++) r.l[i] = borrow ? r.l[i] : d[i];
  return r;
}
GM_DEV Fq30 fq30_canonical(const Fq30& a) { return fq30_canonical_tail(fq30_mul(a, fq30_const(Fq30Consts::ONE))); }

// 12 x u32 packed (the record layout in memory) <-> 13 x 30-bit limbs
GM_DEV Fq30 fq30_unpack(const Fq& x) {
  Fq30 r;
#pragma unroll
  for (int i = 0; i < 13; i++) {
    const int bit = 30 * i, w = bit >> 5, sh = bit & 31;
    uint32_t v = x.l[w] >> sh;
    if (sh > 2 && w + 1 < 12) v |= x.l[w + 1] << (32 - sh);
    r.l[i] = v & Fq30Params::MASK;
  }
  return r;
}
// requires normalised limbs and a value < 2^384
GM_DEV Fq fq30_pack(const Fq30& a) {
  Fq r;
#pragma unroll
  for (int w = 0; w < 12; w++) {
    // word w holds bits [32w, 32w+32): limb i0 = floor(32w/30) shifted down, plus the next limb(s)
    const int bit = 32 * w, i0 = bit / 30, off = bit - 30 * i0;
    uint32_t v = a.l[i0] >> off;
    v |= a.l[i0 + 1] << (30 - off);
    if (60 - off < 32 && i0 + 2 < 13) v |= a.l[i0 + 2] << (60 - off);
    r.l[w] = v;
  }
  return r;
}

}  // namespace gm
