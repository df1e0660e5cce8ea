// The two groups by name, for the code that is stated once for G1 and G2: the key kernels and entries of bases.hip, the point
// kernels of points.hip (whose PtG1 / PtG2 derive from these), the key entries of capi.hip.
//
// A description names the types, the record sizes, the element arithmetic and the group law -- the laws themselves are g1.cuh's
// xyzz_* and g2.cuh's g2_* --, the launch shape of the key kernels, and the handle table of the group.  A coordinate is NC
// elements of Fq, c0 first; el() / parts() pass between an element and its NC components in the device form.
#pragma once
#include "ctx.hpp"
#include "g2.cuh"

namespace gm {

int bases_build_phi(Context* C, Bases* b);  // msm.hip

struct GrpG1 {
  using El = FqE;
  using Affine = G1Affine;
  using Xyzz = G1Xyzz;
  using Held = Bases;  // what a handle names
  using Grp = GrpG1;   // this description, for a struct that derives from it (points.hip) and calls an instance of bases.hip
  static constexpr const char* NAME = "g1";
  static constexpr const char* WHO = "";  // in front of an entry's name in its messages: bases_register, g2_bases_register
  static constexpr int NC = 1;
  static constexpr int KEY_BLOCK = 256, KEY_WAVES = 0;  // the key kernels: blocks of 256, waves per SIMD left to the compiler
  static constexpr bool PREFIX_IN_REGS = true;           // k_normalise (bases.hip): the prefix products wait in the lane
  // points to an inversion for the 8192 entries of the fixed-base table: one, as k_xyzz_to_affine had them -- every generation
  // call waits for this launch, whose lanes are chains of dependent products, and eight to a lane is the longer chain
  static constexpr int TABLE_NORM_K = 1;
  static constexpr size_t EL_BYTES = 48, AFF_BYTES = 96, XYZZ_BYTES = 192;
  static GM_DEV El zero() { return fqe_zero(); }
  static GM_DEV El one() { return fqe_one(); }
  static GM_DEV El el(const FqE* c) { return c[0]; }
  static GM_DEV void parts(const El& a, FqE* c) { c[0] = a; }
  static GM_DEV El neg(const El& a) { return fq_neg_canonical(a); }
  static GM_DEV El mul(const El& a, const El& b) { return fq_mul(a, b); }
  static GM_DEV El inv(const El& a) { return fq_inv(a); }
  static GM_DEV bool is_zero(const El& a) { return fq_is_zero(a); }
  static GM_DEV El el_load(const void* p) { return fqe_load(p); }
  static GM_DEV void el_store(void* p, const El& a) { fqe_store(p, a); }
  static GM_DEV Affine load_affine(const void* p) { return g1_load_affine(p); }
  static GM_DEV void store_affine(void* p, const Affine& a) { g1_store_affine(p, a); }
  static GM_DEV Xyzz load_xyzz(const void* p) { return g1_load_xyzz(p); }
  static GM_DEV void store_xyzz(void* p, const Xyzz& a) { g1_store_xyzz(p, a); }
  static GM_DEV Xyzz identity() { return G1Xyzz::identity(); }
  static GM_DEV bool is_identity(const Xyzz& a) { return a.is_identity(); }
  static GM_DEV Xyzz dbl(const Xyzz& a) { return xyzz_dbl(a); }
  static GM_DEV void madd(Xyzz& acc, const Affine& p) { xyzz_madd(acc, p); }
  static GM_DEV void add(Xyzz& acc, const Xyzz& p) { xyzz_add(acc, p); }
  static Held* find(Context*, uint64_t h) { return find_bases(h); }
  static uint64_t put(Context*, std::unique_ptr<Held> b) { return put_bases(std::move(b)); }
  static std::unique_ptr<Held> take(Context* C, uint64_t h) { return take_from(C, C->bases, h); }
  static int before_put(Context* C, Held* b) { return bases_build_phi(C, b); }
};

struct GrpG2 {
  using El = Fq2;
  using Affine = G2Affine;
  using Xyzz = G2Xyzz;
  using Held = G2Bases;
  using Grp = GrpG2;
  static constexpr const char* NAME = "g2";
  static constexpr const char* WHO = "g2_";
  static constexpr int NC = 2;
  static constexpr int KEY_BLOCK = 64, KEY_WAVES = 1;  // one wave per SIMD, the whole register file (as k_g2_acc)
  static constexpr bool PREFIX_IN_REGS = false;         // k_normalise: eight Fq2 prefixes are 192 VGPRs; they wait in the output records
  static constexpr int TABLE_NORM_K = 8;                // (as the G2 table always was)
  static constexpr size_t EL_BYTES = 96, AFF_BYTES = G2_AFF_BYTES, XYZZ_BYTES = G2_XYZZ_BYTES;
  static GM_DEV El zero() { return fq2_zero(); }
  static GM_DEV El one() { return fq2_one(); }
  static GM_DEV El el(const FqE* c) {
    El r;
    r.c0 = c[0];
    r.c1 = c[1];
    return r;
  }
  static GM_DEV void parts(const El& a, FqE* c) {
    c[0] = a.c0;
    c[1] = a.c1;
  }
  static GM_DEV El neg(const El& a) { return fq2_neg_canonical(a); }
  static GM_DEV El mul(const El& a, const El& b) { return fq2_mul(a, b); }
  static GM_DEV El inv(const El& a) { return fq2_inv(a); }
  static GM_DEV bool is_zero(const El& a) { return fq2_is_zero(a); }
  static GM_DEV El el_load(const void* p) { return fq2_load(p); }
  static GM_DEV void el_store(void* p, const El& a) { fq2_store(p, a); }
  static GM_DEV Affine load_affine(const void* p) { return g2_load_affine(p); }
  static GM_DEV void store_affine(void* p, const Affine& a) { g2_store_affine(p, a); }
  static GM_DEV Xyzz load_xyzz(const void* p) { return g2_load_xyzz(p); }
  static GM_DEV void store_xyzz(void* p, const Xyzz& a) { g2_store_xyzz(p, a); }
  static GM_DEV Xyzz identity() { return G2Xyzz::identity(); }
  static GM_DEV bool is_identity(const Xyzz& a) { return a.is_identity(); }
  static GM_DEV Xyzz dbl(const Xyzz& a) { return g2_dbl(a); }
  static GM_DEV void madd(Xyzz& acc, const Affine& p) { g2_madd(acc, p); }
  static GM_DEV void add(Xyzz& acc, const Xyzz& p) { g2_add(acc, p); }
  static Held* find(Context* C, uint64_t h) { return find_in(C, C->g2_bases, h); }
  static uint64_t put(Context* C, std::unique_ptr<Held> b) { return put_in(C, C->g2_bases, std::move(b)); }
  static std::unique_ptr<Held> take(Context* C, uint64_t h) { return take_from(C, C->g2_bases, h); }
  static int before_put(Context*, Held*) { return GM_OK; }
};

// (X / ZZ, Y / ZZZ) with one inversion of ZZ ZZZ; the identity gives the all-zero record
template <class G>
GM_DEV typename G::Affine grp_to_affine(const typename G::Xyzz& p) {
  typename G::Affine a;
  a.x = G::zero();
  a.y = G::zero();
  if (!G::is_identity(p)) {
    const typename G::El ti = G::inv(G::mul(p.zz, p.zzz));
    a.x = G::mul(p.x, G::mul(ti, p.zzz));
    a.y = G::mul(p.y, G::mul(ti, p.zz));
  }
  return a;
}

// The key code of bases.hip, stated once over a description and instantiated there for both; ctx.hpp declares the instances
// under their own names for the files that do not see the descriptions.
template <class G>
int bases_from_host(Context* C, const void* bases, size_t stride, size_t n, std::unique_ptr<typename G::Held>& out);
template <class G>
int bases_export(Context* C, const typename G::Held* b, size_t offset, size_t n, void* out);
template <class G>
int fixed_base_generate(Context* C, const uint64_t* base_affine, const void* d_scalars, int mont, size_t n, std::unique_ptr<typename G::Held>& out);
constexpr int NORM_K = 8;  // points to an inversion in the batched normalisation (k_normalise), at most
template <class G>
int pack_launch(hipStream_t st, const uint8_t* src, size_t stride, size_t n, uint8_t* dst);
template <class G>
int split_fold_launch(hipStream_t st, const uint8_t* in, size_t n, const uint32_t* d_s8, uint8_t* out);
template <class G>
int normalise_launch(hipStream_t st, const uint8_t* in, const uint32_t* d_idx, size_t n, uint8_t* out, int group = NORM_K);

}  // namespace gm
