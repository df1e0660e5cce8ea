// gemini_hip.hpp -- header-only C++ host layer over the C ABI (gemini_hip.h), mirroring the
// reference's Rust interface for the hot path: same names, argument meaning and failure
// behaviour (the reference panics -> these throw gm::Error).  This is what a C++ embedder links;
// the Rust shim of INTEGRATION.md has the same shape.
//
//   gm::VariableBaseMSM::{msm, msm_unchecked, msm_bigint}   ark-ec 0.4.2 (in-tree: src/kzg/msm/variable_base.rs)
//   gm::ChunkedPippenger / gm::HashMapPippenger             src/kzg/msm/stream_pippenger.rs:143-271
//   gm::msm_chunks                                          src/kzg/space.rs:22-55
//   gm::CommitterKey::{commit, batch_commit}                src/kzg/time.rs:81-107
//   gm::TimeProver (trait Prover)                           src/subprotocols/sumcheck/prover.rs:30-45
//   gm::Transcript (GeminiTranscript over merlin)           src/transcript.rs:8-34
//   gm::Sumcheck::{prove, new_time}                         src/subprotocols/sumcheck/proof.rs:36-66,125-130
//   gm::TensorcheckProof::new_time                          src/subprotocols/tensorcheck/mod.rs:190-275
//   gm::EntryProduct::{new_time, new_time_batch}            src/subprotocols/entryproduct/time_prover.rs:61-147
//   gm::plookup, gm::DeviceVec, gm::IdxVec                  src/subprotocols/plookup/time_prover.rs:65-112
//   gm::R1cs, gm::SnarkProof::{new_time, new_elastic}       src/circuit.rs, src/snark/time_prover.rs:19-117, elastic_prover.rs:174-266
//   gm::dist::{init_rccl, init_shm, init_hook, ...}         the all-gather between the per-GPU processes (no reference counterpart:
//                                                           the reference is single-device; gemini_amd/csrc/dist.cpp)
//   gm::CommitterKey::cyclic_share                          CommitterKey::new (src/kzg/time.rs:49-72), every rank its powers i = rank (mod world)
//   gm::check_g1 / check_g2, CommitterKey::{check_points, check_powers, from_bytes, to_bytes}, G2Bases::{check_points, from_bytes,
//   to_bytes}, Crs::{from_bases, check}, VerifierKey::check, check_points of SnarkProof / PsnarkProof / InnerProductProof
//                                                           deserialize_with_mode(.., Validate::Yes) of ark-ec for whole keys, on the
//                                                           device (gemini_amd/csrc/points.hip); the powers check has no counterpart
//   gm::G2Bases::{fixed_base, srs}                          the powers_of_g2 loop of CommitterKey::new (src/kzg/time.rs:60-67)
//   gm::CommitterKey::from_candidates, G2Bases::from_candidates, Crs::{from_scalars, from_candidates, truncate, halve, fold, bases}
//                                                           Crs::{new, truncate, halve, fold} (src/herring/ipa.rs:173-212); the points
//                                                           come from candidate bytes, not from an arkworks rng (no SHAKE here: the
//                                                           caller brings the bytes)
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "gemini_hip.h"

namespace gm {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc) {
  if (rc != GM_OK) throw Error(rc, gm_last_error());
}
inline void init(int device = 0) { check(gm_init(device)); }
// give the prefix tables of every committer key back (the library does so by itself when a device allocation fails twice)
inline void release_spare_tables() { check(gm_g1_release_spare_tables()); }
// The library's device-memory bookkeeping (gm_mem_stats) and the footprint contract: what a proof will allocate, before it starts
// (the reference's memory story is its constants, README.md:38-46; a prover that keeps its vectors resident owes the number)
struct MemStats {
  uint64_t device_total, device_free, held, held_peak, pool_cached, in_use, in_use_peak, tables, keys, spare_table_releases, msm_workspaces, reserved;
};
inline MemStats mem_stats() {
  uint64_t v[12];
  check(gm_mem_stats(v));
  return MemStats{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11]};
}
inline void mem_reset_peak() { check(gm_mem_reset_peak()); }
struct Footprint {
  uint64_t vectors, workspaces_to_grow, needed, available;
};
inline Footprint snark_footprint(uint64_t ck_handle, size_t num_constraints, bool elastic = false) {
  uint64_t v[4];
  check(gm_snark_footprint(ck_handle, num_constraints, elastic ? 1 : 0, v));
  return Footprint{v[0], v[1], v[2], v[3]};
}
inline Footprint psnark_footprint(uint64_t ck_handle, size_t num_variables, size_t nnz, int elastic = 0) {  // 0 time, 1 elastic (resident), 2 literal
  uint64_t v[4];
  check(gm_psnark_footprint(ck_handle, num_variables, nnz, elastic, v));
  return Footprint{v[0], v[1], v[2], v[3]};
}

// one rank of gm_psnark_new_time_sharded (block = psnark_shard_block(longest vector, world)); z and the instance's blocks are the caller's
inline size_t psnark_shard_block(size_t longest, int world) { return gm_psnark_shard_block(longest, world); }
inline size_t psnark_shard_level(size_t family_len, size_t block, size_t tail_log, int world) { return gm_psnark_shard_level(family_len, block, tail_log, world); }
inline Footprint psnark_shard_footprint(uint64_t key_handle, size_t num_constraints, size_t num_variables, size_t nnz, size_t block, int world) {
  uint64_t v[4];
  check(gm_psnark_shard_footprint(key_handle, num_constraints, num_variables, nnz, block, world, 0, v));
  return Footprint{v[0], v[1], v[2], v[3]};
}

// One process per GPU: after gm::init(local_rank) pick the transport of the library's all-gathers.  Every native prover
// (SnarkProof::new_time ..., gm_snark_new_time_sharded) then runs on N GPUs when its key is a cyclic share / a shard key.
namespace dist {
inline std::array<uint8_t, 128> rccl_unique_id() {  // rank 0; the 128 bytes reach the peers out of band
  std::array<uint8_t, 128> id{};
  check(gm_dist_rccl_unique_id(id.data()));
  return id;
}
inline void init_rccl(int rank, int world, const std::array<uint8_t, 128>& id) { check(gm_dist_init_rccl(rank, world, id.data())); }
inline void init_rccl_node(int rank, int world, const std::string& name) { check(gm_dist_init_rccl_node(rank, world, name.c_str())); }
inline void init_shm(int rank, int world, const std::string& name, size_t slot_bytes = 0) { check(gm_dist_init_shm(rank, world, name.c_str(), slot_bytes)); }
inline void init_hook(int rank, int world, gm_allgather_fn fn, void* ctx) { check(gm_dist_init_hook(rank, world, fn, ctx)); }
inline void selftest() { check(gm_dist_selftest()); }
inline void finalize() { check(gm_dist_finalize()); }
// this rank failed OUTSIDE a collective: release the peers waiting for it (they get GM_ESTATE), poison this rank's transport (round 6)
inline void abort() { check(gm_dist_abort()); }
inline int rank() {
  int r = 0;
  check(gm_dist_info(&r, nullptr, nullptr));
  return r;
}
inline int world() {
  int w = 1;
  check(gm_dist_info(nullptr, &w, nullptr));
  return w;
}
template <class T>
inline std::vector<T> allgather(const T& mine) {  // trivially copyable host values, rank order
  std::vector<T> all((size_t)world());
  check(gm_dist_allgather_host(&mine, sizeof(T), all.data()));
  return all;
}
}  // namespace dist

using Fr = std::array<uint64_t, 4>;        // Montgomery limbs (ark-ff memory image)
using BigInt = std::array<uint64_t, 4>;    // canonical integer (Fr::into_bigint)
using G1Projective = std::array<uint64_t, 18>;  // Jacobian X, Y, Z
struct G1Affine {                          // Rust layout: x, y, infinity (104-byte stride)
  uint64_t x[6], y[6];
  uint64_t infinity;  // bool at byte 96, padded
};
static_assert(sizeof(G1Affine) == 104, "G1Affine must match the 104-byte Rust record");

// ---- point validation (the block of the same name in gemini_hip.h).  A bad point is a result, never an exception ---------------
enum class PointStatus : uint8_t { Ok = GM_PT_OK, BadEncoding = GM_PT_BAD_ENCODING, NonCanonical = GM_PT_NONCANONICAL, NotOnCurve = GM_PT_NOT_ON_CURVE, NotInSubgroup = GM_PT_NOT_IN_SUBGROUP, NotCyclotomic = GM_PT_NOT_CYCLOTOMIC /* check_gt only */ };
struct PointCheck {
  bool ok = false;
  size_t first_bad = 0;         // the smallest bad index; n when every point passes
  std::vector<uint8_t> status;  // PointStatus values, one per point
  explicit operator bool() const { return ok; }
};
// gm_crs_check / gm_vk_check: the smallest bad index of each group (its length when every point passes)
struct KeyCheck {
  bool ok = false;
  size_t first_bad_g1 = 0, first_bad_g2 = 0;
  explicit operator bool() const { return ok; }
};
// gm_snark_proof_check / gm_psnark_proof_check / gm_ipa_check: first_bad in the order gemini_hip.h lists the elements
struct ProofCheck {
  bool ok = false;
  size_t first_bad = 0;
  explicit operator bool() const { return ok; }
};
namespace detail {
template <class F>
inline PointCheck point_check(size_t n, F&& call) {
  PointCheck r;
  r.status.assign(n, 0);
  int ok = 0;
  check(call(r.status.data(), &r.first_bad, &ok));
  r.ok = ok != 0;
  return r;
}
}  // namespace detail
inline PointCheck check_g1(const std::vector<G1Affine>& points) {
  return detail::point_check(points.size(), [&](uint8_t* st, size_t* fb, int* ok) { return gm_g1_check(points.data(), sizeof(G1Affine), points.size(), st, fb, ok); });
}
inline PointCheck check_g1_bases(uint64_t handle, size_t offset, size_t n) {
  return detail::point_check(n, [&](uint8_t* st, size_t* fb, int* ok) { return gm_g1_bases_check(handle, offset, n, st, fb, ok); });
}
// bases[offset + i + 1] = tau bases[offset + i] for the tau of (g2, tau g2): 24 Montgomery limbs each.  rho must be unpredictable to
// whoever made the key
inline bool check_powers(uint64_t handle, size_t offset, size_t n, const uint64_t g2_affine[24], const uint64_t tau_g2_affine[24], const Fr& rho) {
  int ok = 0;
  check(gm_g1_powers_check(handle, offset, n, g2_affine, tau_g2_affine, rho.data(), &ok));
  return ok != 0;
}

inline G1Projective g1_zero() {
  G1Projective z;
  check(gm_g1_sum(nullptr, 0, z.data()));
  return z;
}
inline G1Projective g1_add(const G1Projective& a, const G1Projective& b) {
  uint64_t two[36];
  memcpy(two, a.data(), 144);
  memcpy(two + 18, b.data(), 144);
  G1Projective r;
  check(gm_g1_sum(two, 2, r.data()));
  return r;
}

// S short linear combinations in a fixed number of launches (gm_g1_lincomb_many): out[s] = sum of bigints[t] * points[t] over
// offsets[s] <= t < offsets[s + 1]; offsets has S + 1 entries and starts at 0; an empty segment is the identity
inline std::vector<G1Projective> g1_lincomb_many(const std::vector<G1Affine>& points, const std::vector<BigInt>& bigints, const std::vector<size_t>& offsets) {
  if (offsets.size() < 2) return {};
  if (offsets.back() > points.size() || offsets.back() > bigints.size()) throw Error(GM_EINVAL, "g1_lincomb_many: the offsets run past the terms");
  std::vector<G1Projective> out(offsets.size() - 1);
  check(gm_g1_lincomb_many(points.data(), sizeof(G1Affine), bigints.empty() ? nullptr : bigints[0].data(), offsets.data(), out.size(), out[0].data()));
  return out;
}

struct VariableBaseMSM {
  static G1Projective msm_bigint(const std::vector<G1Affine>& bases, const std::vector<BigInt>& bigints) {
    size_t n = bases.size() < bigints.size() ? bases.size() : bigints.size();
    G1Projective out;
    check(gm_g1_msm(bases.data(), sizeof(G1Affine), n ? bigints[0].data() : nullptr, n, out.data()));
    return out;
  }
  // silently truncates to the shorter input (src/kzg/time.rs:82)
  static G1Projective msm_unchecked(const std::vector<G1Affine>& bases, const std::vector<Fr>& scalars) {
    size_t n = bases.size() < scalars.size() ? bases.size() : scalars.size();
    G1Projective out;
    if (n == 0) return g1_zero();
    uint64_t hb = 0, hv = 0;
    check(gm_g1_bases_register(bases.data(), sizeof(G1Affine), n, &hb));
    int rc = gm_fr_vec_alloc(n, &hv);
    if (!rc) rc = gm_fr_vec_upload(hv, 0, scalars[0].data(), n);
    if (!rc) rc = gm_g1_msm_v(hb, 0, 0, hv, 0, n, out.data());  // into_bigint happens on the device
    if (hv) gm_fr_vec_free(hv);
    gm_g1_bases_free(hb);
    check(rc);
    return out;
  }
  // Ok(result) or Err(min_len): std::pair<optional<result>, size_t>
  static std::pair<std::optional<G1Projective>, size_t> msm(const std::vector<G1Affine>& bases, const std::vector<Fr>& scalars) {
    if (bases.size() != scalars.size()) return {std::nullopt, bases.size() < scalars.size() ? bases.size() : scalars.size()};
    return {msm_unchecked(bases, scalars), 0};
  }
};

// src/kzg/msm/stream_pippenger.rs:209-271.  The buffer is the device slot of a gm_g1_msm_stream (chunk =
// max_msm_buffer pairs, two slots: the copy of one flush runs under the kernels of the previous one); pairs
// added one at a time are staged on the host and pushed in blocks, add_pairs pushes a whole block.
class ChunkedPippenger {
 public:
  explicit ChunkedPippenger(size_t max_msm_buffer) {
    check(gm_g1_msm_stream_new(max_msm_buffer < kMaxChunk ? max_msm_buffer : kMaxChunk, sizeof(G1Affine), 0, &h_));
    stage_ = max_msm_buffer < kStage ? max_msm_buffer : kStage;
    scalars_.reserve(stage_);
    bases_.reserve(stage_);
  }
  ChunkedPippenger(const ChunkedPippenger&) = delete;
  ChunkedPippenger& operator=(const ChunkedPippenger&) = delete;
  ChunkedPippenger(ChunkedPippenger&& o) noexcept : h_(o.h_), stage_(o.stage_), scalars_(std::move(o.scalars_)), bases_(std::move(o.bases_)) { o.h_ = 0; }
  ~ChunkedPippenger() {
    if (h_) gm_g1_msm_stream_free(h_);
  }
  static ChunkedPippenger with_size(size_t buf_size) { return ChunkedPippenger(buf_size); }
  void add(const G1Affine& base, const BigInt& scalar) {
    scalars_.push_back(scalar);
    bases_.push_back(base);
    if (scalars_.size() == stage_) push();
  }
  void add_pairs(const G1Affine* bases, const BigInt* scalars, size_t n) {
    push();
    if (n) check(gm_g1_msm_stream_add(h_, bases, scalars, n));
  }
  G1Projective finalize() {
    push();
    G1Projective r;
    check(gm_g1_msm_stream_finalize(h_, r.data(), nullptr));
    return r;
  }

 private:
  static constexpr size_t kMaxChunk = (size_t)1 << 26, kStage = (size_t)1 << 14;
  void push() {
    if (!scalars_.empty()) check(gm_g1_msm_stream_add(h_, bases_.data(), scalars_.data(), scalars_.size()));
    scalars_.clear();
    bases_.clear();
  }
  uint64_t h_ = 0;
  size_t stage_ = 0;
  std::vector<BigInt> scalars_;
  std::vector<G1Affine> bases_;
};

// src/kzg/space.rs:22-55: skip len(bases) - len(scalars) bases, then 2^20-pair MSMs, summed; the streams stay on the host
inline G1Projective msm_chunks(const std::vector<G1Affine>& bases_stream, const std::vector<Fr>& scalars_stream) {
  if (scalars_stream.size() > bases_stream.size()) throw Error(GM_EINVAL, "msm_chunks: bases not long enough");
  if (scalars_stream.empty()) return g1_zero();
  uint64_t h = 0;
  check(gm_g1_msm_stream_new((size_t)1 << 20, sizeof(G1Affine), 1, &h));
  int rc = gm_g1_msm_stream_add(h, bases_stream.data() + (bases_stream.size() - scalars_stream.size()), scalars_stream.data(), scalars_stream.size());
  G1Projective r;
  if (!rc) rc = gm_g1_msm_stream_finalize(h, r.data(), nullptr);
  gm_g1_msm_stream_free(h);
  check(rc);
  return r;
}

// src/kzg/msm/stream_pippenger.rs:143-206: scalars of equal bases are added in Fr before the MSM
class HashMapPippenger {
 public:
  explicit HashMapPippenger(size_t max_msm_buffer) : cap_(max_msm_buffer), result_(g1_zero()) {}
  void add(const G1Affine& base, const Fr& scalar) {
    Key k;
    memcpy(k.data(), &base, 104);
    auto it = buffer_.find(k);
    if (it == buffer_.end()) {
      buffer_.emplace(k, scalar);
    } else {
      it->second = fr_add(it->second, scalar);
    }
    if (buffer_.size() == cap_) flush();
  }
  G1Projective finalize() {
    if (!buffer_.empty()) flush();
    return result_;
  }

 private:
  using Key = std::array<uint64_t, 13>;
  static Fr fr_add(const Fr& a, const Fr& b) {  // modular addition of Montgomery residues
    static const uint64_t R[4] = {0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL};
    Fr r;
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; i++) {
      c += (unsigned __int128)a[i] + b[i];
      r[i] = (uint64_t)c;
      c >>= 64;
    }
    bool ge = c != 0;
    if (!ge) {
      ge = true;
      for (int i = 3; i >= 0; i--) {
        if (r[i] != R[i]) {
          ge = r[i] > R[i];
          break;
        }
      }
    }
    if (ge) {
      unsigned __int128 br = 0;
      for (int i = 0; i < 4; i++) {
        unsigned __int128 d = (unsigned __int128)r[i] - R[i] - (uint64_t)br;
        r[i] = (uint64_t)d;
        br = (d >> 64) & 1;
      }
    }
    return r;
  }
  void flush() {
    std::vector<G1Affine> bases;
    std::vector<Fr> scalars;
    for (auto& kv : buffer_) {
      G1Affine b;
      memcpy(&b, kv.first.data(), 104);
      bases.push_back(b);
      scalars.push_back(kv.second);
    }
    result_ = g1_add(result_, VariableBaseMSM::msm_unchecked(bases, scalars));
    buffer_.clear();
  }
  size_t cap_;
  std::map<Key, Fr> buffer_;
  G1Projective result_;
};

// SRS resident in HBM + the commit path of src/kzg/time.rs:81-107
class CommitterKey {
 public:
  explicit CommitterKey(const std::vector<G1Affine>& powers_of_g) : n_(powers_of_g.size()) {
    check(gm_g1_bases_register(powers_of_g.data(), sizeof(G1Affine), n_, &h_));
    check(gm_g1_bases_precompute(h_, -1));  // a committer key stays resident: fixed-base tables when they fit (gm_set_auto_tables)
  }
  // this rank's ELEMENT-CYCLIC share of CommitterKey::new(max_degree, ..) with trapdoor tau (canonical) and generator g: powers
  // i = rank (mod world), generated on the device; commit / batch_commit and every prover handed this key then shard their MSMs
  // over the ranks (gm::dist::init_* first).  One rank: the whole key.
  static CommitterKey cyclic_share(const uint64_t g_affine[12], const BigInt& tau, size_t max_degree) {
    CommitterKey k;
    k.n_ = max_degree + 1;
    check(gm_g1_srs_register_cyclic(g_affine, tau.data(), k.n_, dist::rank(), dist::world(), &k.h_));
    return k;
  }
  // n points of 48 (compressed) or 96 bytes in the framing `encoding` (0 ark-ec, 1 zcash), decoded -- and with `validate` checked --
  // on the device (gm_g1_bases_from_bytes).  No key when a point is rejected: *report says which and why
  static std::optional<CommitterKey> from_bytes(const std::vector<uint8_t>& bytes, size_t n, bool compressed, int encoding, bool validate = true,
                                                PointCheck* report = nullptr) {
    if (bytes.size() != n * (compressed ? 48 : 96)) throw Error(GM_EINVAL, "CommitterKey::from_bytes: the byte count does not match n");
    CommitterKey k;
    PointCheck r = detail::point_check(n, [&](uint8_t* st, size_t* fb, int* ok) {
      return gm_g1_bases_from_bytes(bytes.data(), n, compressed ? 1 : 0, encoding, validate ? 1 : 0, &k.h_, st, fb, ok);
    });
    const bool ok = r.ok;
    if (report) *report = std::move(r);
    if (ok != (k.h_ != 0)) throw Error(GM_ESTATE, "CommitterKey::from_bytes: the library hands out a handle exactly when every point is accepted");
    if (!ok) return std::nullopt;
    k.n_ = n;
    return std::optional<CommitterKey>(std::move(k));
  }
  // n points of G1 whose logarithms nobody knows: the first n of the 48-byte candidates in `cand` that survive, cofactor-cleared on
  // the device (gm_g1_bases_from_candidates; the header has the candidate format).  *used: the index after the n-th survivor, or
  // the number of candidates; *found: the survivors before it.  No key on a shortfall (found < n).  No tables are built.
  static std::optional<CommitterKey> from_candidates(const std::vector<uint8_t>& cand, size_t n, size_t* used = nullptr, size_t* found = nullptr) {
    if (cand.size() % 48) throw Error(GM_EINVAL, "CommitterKey::from_candidates: a G1 candidate is 48 bytes");
    CommitterKey k;
    size_t u = 0, f = 0;
    check(gm_g1_bases_from_candidates(cand.data(), cand.size() / 48, n, &k.h_, &u, &f));
    if (used) *used = u;
    if (found) *found = f;
    if ((f >= n) != (k.h_ != 0)) throw Error(GM_ESTATE, "CommitterKey::from_candidates: the library hands out a handle exactly when n candidates survive");
    if (!k.h_) return std::nullopt;
    k.n_ = n;
    return std::optional<CommitterKey>(std::move(k));
  }
  // 96-byte records x | y (the identity all zero), 12 words each
  std::vector<uint64_t> download(size_t offset, size_t n) const {
    std::vector<uint64_t> out(n * 12);
    check(gm_g1_bases_download(h_, offset, n, out.data()));
    return out;
  }
  PointCheck check_points() const { return check_g1_bases(h_, 0, n_); }  // every power on the curve and in G1
  // the canonical encodings of powers [offset, offset + n), 48 / 96 bytes each, made on the device (gm_g1_bases_to_bytes)
  std::vector<uint8_t> to_bytes(bool compressed, int encoding, size_t offset, size_t n) const {
    std::vector<uint8_t> out(n * (compressed ? 48 : 96));
    check(gm_g1_bases_to_bytes(h_, offset, n, compressed ? 1 : 0, encoding, out.data(), out.size()));
    return out;
  }
  std::vector<uint8_t> to_bytes(bool compressed, int encoding = 0) const { return to_bytes(compressed, encoding, 0, n_); }
  bool check_powers(const uint64_t g2_affine[24], const uint64_t tau_g2_affine[24], const Fr& rho) const { return gm::check_powers(h_, 0, n_, g2_affine, tau_g2_affine, rho); }
  size_t size() const { return n_; }
  CommitterKey(CommitterKey&& o) noexcept : h_(o.h_), n_(o.n_) { o.h_ = 0; }
  ~CommitterKey() {
    if (h_) gm_g1_bases_free(h_);
  }
  CommitterKey(const CommitterKey&) = delete;
  CommitterKey& operator=(const CommitterKey&) = delete;
  uint64_t handle() const { return h_; }
  G1Projective commit(const std::vector<Fr>& polynomial) const {
    size_t n = polynomial.size() < n_ ? polynomial.size() : n_;
    if (n == 0) return g1_zero();
    uint64_t hv = 0;
    check(gm_fr_vec_alloc(n, &hv));
    G1Projective out;
    int rc = gm_fr_vec_upload(hv, 0, polynomial[0].data(), n);
    if (!rc) rc = gm_ck_msm(h_, 0, 0, hv, 0, n, out.data());  // a whole key: gm_g1_msm_v; a cyclic share: local MSM + all-gather
    gm_fr_vec_free(hv);
    check(rc);
    return out;
  }
  // src/kzg/time.rs:98-107: ONE pipelined call (gm_g1_msm_v_batch: two calls in flight, the host tail of one under the kernels of
  // the next, small ones on four lanes side by side) instead of a loop of commits
  std::vector<G1Projective> batch_commit(const std::vector<std::vector<Fr>>& polynomials) const {
    const size_t k = polynomials.size();
    std::vector<G1Projective> out(k, g1_zero());
    std::vector<uint64_t> hv(k, 0);
    std::vector<size_t> ns(k, 0);
    int rc = GM_OK;
    for (size_t j = 0; j < k && !rc; j++) {
      ns[j] = polynomials[j].size() < n_ ? polynomials[j].size() : n_;
      rc = gm_fr_vec_alloc(ns[j], &hv[j]);
      if (!rc && ns[j]) rc = gm_fr_vec_upload(hv[j], 0, polynomials[j][0].data(), ns[j]);
    }
    if (!rc && k) rc = gm_ck_msm_batch(h_, hv.data(), ns.data(), k, out[0].data());
    for (uint64_t h : hv)
      if (h) gm_fr_vec_free(h);
    check(rc);
    return out;
  }

 private:
  friend class Crs;  // Crs::bases hands out device copies of its arrays
  CommitterKey() = default;
  uint64_t h_ = 0;
  size_t n_ = 0;  // powers of the WHOLE key
};

struct RoundMsg {
  Fr a, b;
};

// trait Prover, src/subprotocols/sumcheck/prover.rs:30-45 / time_prover.rs:42-137
class TimeProver {
 public:
  TimeProver(const std::vector<Fr>& f, const std::vector<Fr>& g, const Fr& twist) {
    check(gm_sc_new(f.empty() ? nullptr : f[0].data(), f.size(), g.empty() ? nullptr : g[0].data(), g.size(), twist.data(), &h_));
  }
  // a gm_sc_* prover the library created (EntryProduct::new_time_batch); owned from here
  static TimeProver from_handle(uint64_t handle) {
    TimeProver p;
    p.h_ = handle;
    return p;
  }
  TimeProver(TimeProver&& o) noexcept : h_(o.h_) { o.h_ = 0; }
  ~TimeProver() {
    if (h_) gm_sc_free(h_);
  }
  TimeProver(const TimeProver&) = delete;
  TimeProver& operator=(const TimeProver&) = delete;
  std::optional<RoundMsg> next_message(const std::optional<Fr>& verifier_message) {
    RoundMsg m;
    int has = 0;
    check(gm_sc_round(h_, verifier_message ? verifier_message->data() : nullptr, m.a.data(), m.b.data(), &has));
    if (!has) return std::nullopt;
    return m;
  }
  void fold(const Fr& challenge) { check(gm_sc_fold(h_, challenge.data())); }
  size_t rounds() const {
    size_t t = 0;
    check(gm_sc_rounds(h_, &t, nullptr));
    return t;
  }
  size_t round() const {
    size_t r = 0;
    check(gm_sc_rounds(h_, nullptr, &r));
    return r;
  }
  std::optional<std::array<Fr, 2>> final_foldings() const {
    std::array<Fr, 2> ff;
    int has = 0;
    check(gm_sc_final(h_, ff[0].data(), ff[1].data(), &has));
    if (!has) return std::nullopt;
    return ff;
  }
  uint64_t handle() const { return h_; }

 private:
  TimeProver() = default;
  uint64_t h_ = 0;
};

// ---- BLS12-381 G2: `P::G2::msm_unchecked` (src/herring/ipa.rs:107-118,185-189) and TimeProver<G2Module> (src/herring) -----------
using G2Projective = std::array<uint64_t, 36>;  // Jacobian X, Y, Z over Fq2, c0 before c1
struct G2Affine {                               // Rust layout: x.c0, x.c1, y.c0, y.c1, infinity (200-byte stride)
  uint64_t x[12], y[12];
  uint64_t infinity;  // bool at byte 192, padded
};
static_assert(sizeof(G2Affine) == 200, "G2Affine must match the 200-byte Rust record");

inline PointCheck check_g2(const std::vector<G2Affine>& points) {
  return detail::point_check(points.size(), [&](uint8_t* st, size_t* fb, int* ok) { return gm_g2_check(points.data(), sizeof(G2Affine), points.size(), st, fb, ok); });
}

inline G2Projective g2_zero() {
  G2Projective z;
  check(gm_g2_sum(nullptr, 0, z.data()));
  return z;
}
inline G2Projective g2_add(const G2Projective& a, const G2Projective& b) {
  uint64_t two[72];
  memcpy(two, a.data(), 288);
  memcpy(two + 36, b.data(), 288);
  G2Projective r;
  check(gm_g2_sum(two, 2, r.data()));
  return r;
}

// the G2 twin of g1_lincomb_many (gm_g2_lincomb_many): S short linear combinations in a fixed number of launches, an empty segment is the identity
inline std::vector<G2Projective> g2_lincomb_many(const std::vector<G2Affine>& points, const std::vector<BigInt>& bigints, const std::vector<size_t>& offsets) {
  if (offsets.size() < 2) return {};
  if (offsets.back() > points.size() || offsets.back() > bigints.size()) throw Error(GM_EINVAL, "g2_lincomb_many: the offsets run past the terms");
  std::vector<G2Projective> out(offsets.size() - 1);
  check(gm_g2_lincomb_many(points.data(), sizeof(G2Affine), bigints.empty() ? nullptr : bigints[0].data(), offsets.data(), out.size(), out[0].data()));
  return out;
}

// G2 points resident in HBM (the `g2s` of herring's Crs); commit_g2 is msm_unchecked against them
class G2Bases {
 public:
  explicit G2Bases(const std::vector<G2Affine>& points) : n_(points.size()) { check(gm_g2_bases_register(points.data(), sizeof(G2Affine), n_, &h_)); }
  G2Bases(G2Bases&& o) noexcept : h_(o.h_), n_(o.n_) { o.h_ = 0; }
  ~G2Bases() {
    if (h_) gm_g2_bases_free(h_);
  }
  G2Bases(const G2Bases&) = delete;
  G2Bases& operator=(const G2Bases&) = delete;
  uint64_t handle() const { return h_; }
  size_t size() const { return n_; }
  PointCheck check_points(size_t offset, size_t n) const {
    return detail::point_check(n, [&](uint8_t* st, size_t* fb, int* ok) { return gm_g2_bases_check(h_, offset, n, st, fb, ok); });
  }
  PointCheck check_points() const { return check_points(0, n_); }
  // n points of 96 (compressed) or 192 bytes in the framing `encoding`, decoded -- and with `validate` checked -- on the device
  // (gm_g2_bases_from_bytes).  No bases when a point is rejected: *report says which and why
  static std::optional<G2Bases> from_bytes(const std::vector<uint8_t>& bytes, size_t n, bool compressed, int encoding, bool validate = true, PointCheck* report = nullptr) {
    if (bytes.size() != n * (compressed ? 96 : 192)) throw Error(GM_EINVAL, "G2Bases::from_bytes: the byte count does not match n");
    G2Bases b;
    PointCheck r = detail::point_check(n, [&](uint8_t* st, size_t* fb, int* ok) {
      return gm_g2_bases_from_bytes(bytes.data(), n, compressed ? 1 : 0, encoding, validate ? 1 : 0, &b.h_, st, fb, ok);
    });
    const bool ok = r.ok;
    if (report) *report = std::move(r);
    if (ok != (b.h_ != 0)) throw Error(GM_ESTATE, "G2Bases::from_bytes: the library hands out a handle exactly when every point is accepted");
    if (!ok) return std::nullopt;
    b.n_ = n;
    return std::optional<G2Bases>(std::move(b));
  }
  std::vector<uint8_t> to_bytes(bool compressed, int encoding, size_t offset, size_t n) const {
    std::vector<uint8_t> out(n * (compressed ? 96 : 192));
    check(gm_g2_bases_to_bytes(h_, offset, n, compressed ? 1 : 0, encoding, out.data(), out.size()));
    return out;
  }
  std::vector<uint8_t> to_bytes(bool compressed, int encoding = 0) const { return to_bytes(compressed, encoding, 0, n_); }
  // [s_i base], generated on the device (gm_g2_fixed_base_register): base a 192-byte record, scalars canonical -- any 256-bit value,
  // taken as that integer; a zero scalar gives the identity record
  static G2Bases fixed_base(const uint64_t base_affine[24], const std::vector<BigInt>& scalars) {
    G2Bases b;
    check(gm_g2_fixed_base_register(base_affine, scalars.empty() ? nullptr : scalars[0].data(), scalars.size(), &b.h_));
    b.n_ = scalars.size();
    return b;
  }
  // tau^i base, i < n: the powers_of_g2 of CommitterKey::new (src/kzg/time.rs:60-67), tau canonical (gm_g2_srs_register)
  static G2Bases srs(const uint64_t base_affine[24], const BigInt& tau, size_t n) {
    G2Bases b;
    check(gm_g2_srs_register(base_affine, tau.data(), n, &b.h_));
    b.n_ = n;
    return b;
  }
  // the G2 twin of CommitterKey::from_candidates: 96-byte candidates x.c0 | x.c1 (gm_g2_bases_from_candidates)
  static std::optional<G2Bases> from_candidates(const std::vector<uint8_t>& cand, size_t n, size_t* used = nullptr, size_t* found = nullptr) {
    if (cand.size() % 96) throw Error(GM_EINVAL, "G2Bases::from_candidates: a G2 candidate is 96 bytes");
    G2Bases b;
    size_t u = 0, f = 0;
    check(gm_g2_bases_from_candidates(cand.data(), cand.size() / 96, n, &b.h_, &u, &f));
    if (used) *used = u;
    if (found) *found = f;
    if ((f >= n) != (b.h_ != 0)) throw Error(GM_ESTATE, "G2Bases::from_candidates: the library hands out a handle exactly when n candidates survive");
    if (!b.h_) return std::nullopt;
    b.n_ = n;
    return std::optional<G2Bases>(std::move(b));
  }
  // 192-byte records x.c0 | x.c1 | y.c0 | y.c1 (the identity all zero), 24 words each
  std::vector<uint64_t> download(size_t offset, size_t n) const {
    std::vector<uint64_t> out(n * 24);
    check(gm_g2_bases_download(h_, offset, n, out.data()));
    return out;
  }
  G2Projective msm_bigint(const std::vector<BigInt>& bigints, size_t offset = 0, bool reversed = false) const {
    G2Projective out;
    check(gm_g2_msm_h(h_, offset, reversed ? 1 : 0, bigints.empty() ? nullptr : bigints[0].data(), bigints.size(), out.data()));
    return out;
  }
  // silently truncates to the shorter input, like the reference (src/herring/ipa.rs:117)
  G2Projective msm_unchecked(const std::vector<Fr>& scalars) const {
    const size_t n = scalars.size() < n_ ? scalars.size() : n_;
    if (n == 0) return g2_zero();
    uint64_t hv = 0;
    check(gm_fr_vec_alloc(n, &hv));
    G2Projective out;
    int rc = gm_fr_vec_upload(hv, 0, scalars[0].data(), n);
    if (!rc) rc = gm_g2_msm_v(h_, 0, 0, hv, 0, n, out.data());  // into_bigint happens on the device
    gm_fr_vec_free(hv);
    check(rc);
    return out;
  }
  G2Projective msm_device(const void* d_scalars, bool mont, size_t n, size_t offset = 0, bool reversed = false) const {
    G2Projective out;
    check(gm_g2_msm_d(h_, offset, reversed ? 1 : 0, d_scalars, mont ? 1 : 0, n, out.data()));
    return out;
  }

 private:
  friend class Crs;
  G2Bases() = default;
  uint64_t h_ = 0;
  size_t n_ = 0;
};

struct G2RoundMsg {
  G2Projective a, b;
};
namespace detail {
// TimeProver<M> of herring over a bilinear module (src/herring/time_prover.rs:42-137).  T names the module: the vector, message and
// final-pair types, `create`, and the five C functions behind the other members
template <class T>
class HerringModuleProver {
 public:
  HerringModuleProver(const typename T::Lhs& f, const typename T::Rhs& g, const Fr& twist) { check(T::create(f, g, twist, &h_)); }
  HerringModuleProver(HerringModuleProver&& o) noexcept : h_(o.h_) { o.h_ = 0; }
  ~HerringModuleProver() {
    if (h_) T::free(h_);
  }
  HerringModuleProver(const HerringModuleProver&) = delete;
  HerringModuleProver& operator=(const HerringModuleProver&) = delete;
  std::optional<typename T::Msg> next_message(const std::optional<Fr>& verifier_message) {
    typename T::Msg m;
    int has = 0;
    check(T::round(h_, verifier_message ? verifier_message->data() : nullptr, m.a.data(), m.b.data(), &has));
    if (!has) return std::nullopt;
    return m;
  }
  void fold(const Fr& challenge) { check(T::fold(h_, challenge.data())); }
  size_t rounds() const {
    size_t t = 0;
    check(T::rounds(h_, &t, nullptr));
    return t;
  }
  size_t round() const {
    size_t r = 0;
    check(T::rounds(h_, nullptr, &r));
    return r;
  }
  std::optional<typename T::Final> final_foldings() const {
    typename T::Final ff;
    int has = 0;
    check(T::final_foldings(h_, ff.first.data(), ff.second.data(), &has));
    if (!has) return std::nullopt;
    return ff;
  }
  uint64_t handle() const { return h_; }
  static HerringModuleProver from_handle(uint64_t handle) {  // a prover the library created (a space prover's to_time); owned from here
    HerringModuleProver p;
    p.h_ = handle;
    return p;
  }

 private:
  HerringModuleProver() = default;
  uint64_t h_ = 0;
};
// TimeProver<G1Module> (module.rs:81-102): f in G1, g in Fr
struct G1ModuleRoundMsg {
  G1Projective a, b;
};
struct HerringG1Module {
  using Lhs = std::vector<G1Affine>;
  using Rhs = std::vector<Fr>;
  using Msg = G1ModuleRoundMsg;
  using Final = std::pair<G1Projective, Fr>;
  static int create(const Lhs& f, const Rhs& g, const Fr& twist, uint64_t* h) {
    return gm_hg1_new(f.data(), sizeof(G1Affine), f.size(), g.empty() ? nullptr : g[0].data(), g.size(), twist.data(), h);
  }
  static constexpr auto round = gm_hg1_round;
  static constexpr auto fold = gm_hg1_fold;
  static constexpr auto rounds = gm_hg1_rounds;
  static constexpr auto final_foldings = gm_hg1_final;
  static constexpr auto free = gm_hg1_free;
};
// TimeProver<G2Module> (module.rs:104-125): f in Fr, g in G2
struct HerringG2Module {
  using Lhs = std::vector<Fr>;
  using Rhs = std::vector<G2Affine>;
  using Msg = G2RoundMsg;
  using Final = std::pair<Fr, G2Projective>;
  static int create(const Lhs& f, const Rhs& g, const Fr& twist, uint64_t* h) {
    return gm_hg2_new(f.empty() ? nullptr : f[0].data(), f.size(), g.data(), sizeof(G2Affine), g.size(), twist.data(), h);
  }
  static constexpr auto round = gm_hg2_round;
  static constexpr auto fold = gm_hg2_fold;
  static constexpr auto rounds = gm_hg2_rounds;
  static constexpr auto final_foldings = gm_hg2_final;
  static constexpr auto free = gm_hg2_free;
};
}  // namespace detail
using HerringG1 = detail::HerringModuleProver<detail::HerringG1Module>;
using HerringG2 = detail::HerringModuleProver<detail::HerringG2Module>;

// ---- pairings: `P::multi_pairing` behind PModule::ip (src/herring/module.rs:60-79) and TimeProver<PModule> ----------------------
using Gt = std::array<uint64_t, 72>;  // 12 Fq in tower order c0.c0.c0, c0.c0.c1, ..., c1.c2.c1 (ark-ff Fp12); multiplicative

inline Gt gt_one() {
  Gt r;
  check(gm_gt_one(r.data()));
  return r;
}
inline Gt gt_mul(const Gt& a, const Gt& b) {  // herring's "+" on GT
  Gt r;
  check(gm_gt_mul(a.data(), b.data(), r.data()));
  return r;
}
inline Gt gt_pow(const Gt& a, const BigInt& scalar) {
  Gt r;
  check(gm_gt_pow(a.data(), scalar.data(), r.data()));
  return r;
}
// prod_i e(g1[i], g2[i]) over the shorter input (zip); a pair with a point at infinity contributes 1
inline Gt multi_pairing(const std::vector<G1Affine>& g1, const std::vector<G2Affine>& g2) {
  Gt r;
  check(gm_pairing_multi(g1.data(), sizeof(G1Affine), g2.data(), sizeof(G2Affine), g1.size() < g2.size() ? g1.size() : g2.size(), r.data()));
  return r;
}
// the same over registered bases (handles of gm_g1_bases_register / gm::G2Bases): g1[off1 + step1 i] against g2[off2 + step2 i], i < n
inline Gt multi_pairing(uint64_t g1_handle, size_t off1, size_t step1, const G2Bases& g2, size_t off2, size_t step2, size_t n) {
  Gt r;
  check(gm_pairing_multi_h(g1_handle, off1, step1, g2.handle(), off2, step2, n, r.data()));
  return r;
}
// S independent products in one segmented launch (gm_pairing_multi_many): out[s] = prod e(g1[t], g2[t]) over offsets[s] <= t < offsets[s + 1],
// each bit-identical to multi_pairing on that slice; an empty product is 1
inline std::vector<Gt> multi_pairing_many(const std::vector<G1Affine>& g1, const std::vector<G2Affine>& g2, const std::vector<size_t>& offsets) {
  if (offsets.size() < 2) return {};
  if (offsets.back() > g1.size() || offsets.back() > g2.size()) throw Error(GM_EINVAL, "multi_pairing_many: the offsets run past the pairs");
  std::vector<Gt> out(offsets.size() - 1);
  check(gm_pairing_multi_many(g1.data(), sizeof(G1Affine), g2.data(), sizeof(G2Affine), offsets.data(), out.size(), out[0].data()));
  return out;
}
// fewer stated KZG checks than this run one by one, as the single verifiers run them (gm_set_verify_many_min); verdicts do not depend on it
inline void set_verify_many_min(size_t checks) { check(gm_set_verify_many_min(checks)); }

struct GtRoundMsg {
  Gt a, b;
};
namespace detail {
// TimeProver<PModule> (module.rs:60-79): f in G1, g in G2, messages in GT
struct HerringPModule {
  using Lhs = std::vector<G1Affine>;
  using Rhs = std::vector<G2Affine>;
  using Msg = GtRoundMsg;
  using Final = std::pair<G1Projective, G2Projective>;
  static int create(const Lhs& f, const Rhs& g, const Fr& twist, uint64_t* h) {
    return gm_hp_new(f.data(), sizeof(G1Affine), f.size(), g.data(), sizeof(G2Affine), g.size(), twist.data(), h);
  }
  static constexpr auto round = gm_hp_round;
  static constexpr auto fold = gm_hp_fold;
  static constexpr auto rounds = gm_hp_rounds;
  static constexpr auto final_foldings = gm_hp_final;
  static constexpr auto free = gm_hp_free;
};
}  // namespace detail
using HerringP = detail::HerringModuleProver<detail::HerringPModule>;

// ---- GtModule (src/herring/module.rs:49-58): prod_i x_i^e_i on the device and TimeProver<GtModule> ------------------------------
// exponents are 256-bit integers as given (not reduced mod r), like gt_pow; the shorter input ends the product, none gives 1
inline Gt gt_multi_pow(const std::vector<Gt>& x, const std::vector<BigInt>& scalars) {
  Gt r;
  const size_t n = x.size() < scalars.size() ? x.size() : scalars.size();
  check(gm_gt_multi_pow(n ? x[0].data() : nullptr, n, n ? scalars[0].data() : nullptr, r.data()));
  return r;
}
// S = offsets.size() - 1 independent products in one launch (gm_gt_multi_pow_many): out[s] is over the terms offsets[s] <= i <
// offsets[s + 1], bit for bit gt_multi_pow on that range; an empty product is 1
inline std::vector<Gt> gt_multi_pow_many(const std::vector<Gt>& x, const std::vector<BigInt>& scalars, const std::vector<size_t>& offsets) {
  if (offsets.empty()) throw Error(GM_EINVAL, "gt_multi_pow_many: offsets needs S + 1 entries");
  if (offsets.back() > x.size() || offsets.back() > scalars.size()) throw Error(GM_EINVAL, "gt_multi_pow_many: the offsets run past the terms");
  std::vector<Gt> out(offsets.size() - 1);
  check(gm_gt_multi_pow_many(x.empty() ? nullptr : x[0].data(), scalars.empty() ? nullptr : scalars[0].data(), offsets.data(), out.size(),
                             out.empty() ? nullptr : out[0].data()));
  return out;
}
namespace detail {
// TimeProver<GtModule>: f in GT, g in Fr, messages in GT
struct HerringGtModule {
  using Lhs = std::vector<Gt>;
  using Rhs = std::vector<Fr>;
  using Msg = GtRoundMsg;
  using Final = std::pair<Gt, Fr>;
  static int create(const Lhs& f, const Rhs& g, const Fr& twist, uint64_t* h) {
    return gm_hgt_new(f.empty() ? nullptr : f[0].data(), f.size(), g.empty() ? nullptr : g[0].data(), g.size(), twist.data(), h);
  }
  static constexpr auto round = gm_hgt_round;
  static constexpr auto fold = gm_hgt_fold;
  static constexpr auto rounds = gm_hgt_rounds;
  static constexpr auto final_foldings = gm_hgt_final;
  static constexpr auto free = gm_hgt_free;
};
}  // namespace detail
// check(): GT membership of the CURRENT f vector, where it lies on the device (gm_hgt_check); first_bad is its length when all pass
class HerringGt : public detail::HerringModuleProver<detail::HerringGtModule> {
 public:
  using detail::HerringModuleProver<detail::HerringGtModule>::HerringModuleProver;
  ProofCheck check() const {
    ProofCheck r;
    int ok = 0;
    gm::check(gm_hgt_check(handle(), &r.first_bad, &ok));
    r.ok = ok != 0;
    return r;
  }
};

// ---- GT element by element on the device (the block of the same name in gemini_hip.h) --------------------------------------------
// out[i] = in[i]^((q^12 - 1) / r), no conjugation: gm_gt_final_exp's value bit for bit, on any reduced coefficients
inline std::vector<Gt> gt_final_exp_many(const std::vector<Gt>& in) {
  std::vector<Gt> out(in.size());
  check(gm_gt_final_exp_many(in.empty() ? nullptr : in[0].data(), in.size(), out.empty() ? nullptr : out[0].data()));
  return out;
}
// out[i] = e(g1[i], g2[i]) over the shorter input (zip): one launch of Miller loops, one of final exponentiations
inline std::vector<Gt> pairing_each(const std::vector<G1Affine>& g1, const std::vector<G2Affine>& g2) {
  std::vector<Gt> out(g1.size() < g2.size() ? g1.size() : g2.size());
  check(gm_pairing_each(g1.data(), sizeof(G1Affine), g2.data(), sizeof(G2Affine), out.size(), out.empty() ? nullptr : out[0].data()));
  return out;
}
// the same over registered bases: out[i] = e(g1[off1 + step1 i], g2[off2 + step2 i]), i < n
inline std::vector<Gt> pairing_each(uint64_t g1_handle, size_t off1, size_t step1, const G2Bases& g2, size_t off2, size_t step2, size_t n) {
  std::vector<Gt> out(n);
  check(gm_pairing_each_h(g1_handle, off1, step1, g2.handle(), off2, step2, n, out.empty() ? nullptr : out[0].data()));
  return out;
}
// gm_gt_check: is every element a member of GT?  status holds GM_PT_OK / GM_PT_NONCANONICAL / GM_PT_NOT_CYCLOTOMIC / GM_PT_NOT_IN_SUBGROUP
inline PointCheck check_gt(const std::vector<Gt>& x) {
  return detail::point_check(x.size(), [&](uint8_t* st, size_t* fb, int* ok) { return gm_gt_check(x.empty() ? nullptr : x[0].data(), x.size(), st, fb, ok); });
}

// merlin::Transcript + GeminiTranscript, src/transcript.rs
class Transcript {
 public:
  explicit Transcript(const std::string& label = "GEMINI-v0") { check(gm_transcript_new((const uint8_t*)label.data(), label.size(), &h_)); }
  ~Transcript() {
    if (h_) gm_transcript_free(h_);
  }
  Transcript(const Transcript&) = delete;
  Transcript& operator=(const Transcript&) = delete;
  void append_message(const std::string& label, const std::vector<uint8_t>& msg) {
    check(gm_transcript_append_message(h_, (const uint8_t*)label.data(), label.size(), msg.data(), msg.size()));
  }
  void append_serializable(const std::string& label, const Fr& x) { check(gm_transcript_append_fr(h_, (const uint8_t*)label.data(), label.size(), x.data(), 1)); }
  void append_serializable(const std::string& label, const RoundMsg& m) {
    uint64_t ab[8];
    memcpy(ab, m.a.data(), 32);
    memcpy(ab + 4, m.b.data(), 32);
    check(gm_transcript_append_fr(h_, (const uint8_t*)label.data(), label.size(), ab, 2));
  }
  void append_serializable(const std::string& label, const G1Projective& c) {
    check(gm_transcript_append_g1(h_, (const uint8_t*)label.data(), label.size(), c.data(), 1, 0));
  }
  void append_serializable(const std::string& label, const Gt& x) { check(gm_transcript_append_gt(h_, (const uint8_t*)label.data(), label.size(), x.data(), 1)); }
  void append_serializable(const std::string& label, const GtRoundMsg& m) {  // SumcheckMsg<PairingOutput>: a || b
    uint64_t ab[144];
    memcpy(ab, m.a.data(), 576);
    memcpy(ab + 72, m.b.data(), 576);
    check(gm_transcript_append_gt(h_, (const uint8_t*)label.data(), label.size(), ab, 2));
  }
  Fr get_challenge(const std::string& label) {
    Fr r;
    check(gm_transcript_challenge_fr(h_, (const uint8_t*)label.data(), label.size(), r.data()));
    return r;
  }
  uint64_t handle() const { return h_; }

 private:
  uint64_t h_ = 0;
};

// ---- herring's inner-product argument (src/herring/ipa.rs): Crs, Vrs, InnerProductProof ------------------------------------------
// `InnerProductProof::generic` (pub(crate)) and `CrsStream` (its fold is a todo!() in the reference) are out of scope.
class Crs {  // ipa.rs:62-66,172-213: G1 and G2 points resident in HBM
 public:
  Crs(const std::vector<G1Affine>& g1s, const std::vector<G2Affine>& g2s) {
    gm::check(gm_crs_new(g1s.data(), sizeof(G1Affine), g1s.size(), g2s.data(), sizeof(G2Affine), g2s.size(), &h_));
  }
  // from two registered keys by device-to-device copy (gm_crs_from_bases): a CRS decoded by the two from_bytes never visits the
  // host; the keys stay the caller's
  static Crs from_bases(const CommitterKey& g1s, const G2Bases& g2s) {
    Crs c;
    gm::check(gm_crs_from_bases(g1s.handle(), g2s.handle(), &c.h_));
    return c;
  }
  // g1s[i] = a_i g1, g2s[i] = b_i g2 (canonical scalars), generated on the device.  FOR TESTS AND BENCHMARKS ONLY: whoever knows a
  // and b knows every logarithm of this CRS and can break the binding of its commitments; from_candidates is the one to use
  static Crs from_scalars(const uint64_t g1_affine[12], const std::vector<BigInt>& a, const uint64_t g2_affine[24], const std::vector<BigInt>& b) {
    CommitterKey k1;
    gm::check(gm_g1_fixed_base_register(g1_affine, a.empty() ? nullptr : a[0].data(), a.size(), &k1.h_));
    k1.n_ = a.size();
    return from_bases(k1, G2Bases::fixed_base(g2_affine, b));
  }
  // `Crs::new(rng, d)` (ipa.rs:173-177) with candidate bytes in the place of the rng: the first d survivors of each stream
  // (CommitterKey::from_candidates, G2Bases::from_candidates); no Crs when either stream runs short
  static std::optional<Crs> from_candidates(const std::vector<uint8_t>& g1_cand, const std::vector<uint8_t>& g2_cand, size_t d) {
    std::optional<CommitterKey> k1 = CommitterKey::from_candidates(g1_cand, d);
    if (!k1) return std::nullopt;
    std::optional<G2Bases> k2 = G2Bases::from_candidates(g2_cand, d);
    if (!k2) return std::nullopt;
    return std::optional<Crs>(from_bases(*k1, *k2));
  }
  std::pair<size_t, size_t> len() const {
    std::pair<size_t, size_t> n{0, 0};
    gm::check(gm_crs_len(h_, &n.first, &n.second));
    return n;
  }
  // Crs::truncate / halve / fold (ipa.rs:191-212), each as a NEW Crs: this one stays valid
  Crs truncate(size_t rounds) const {
    Crs c;
    gm::check(gm_crs_truncate(h_, rounds, &c.h_));
    return c;
  }
  Crs halve() const {
    Crs c;
    gm::check(gm_crs_halve(h_, &c.h_));
    return c;
  }
  Crs fold(const Fr& challenge) const {  // groups of different lengths are refused (GM_EINVAL)
    Crs c;
    gm::check(gm_crs_fold(h_, challenge.data(), &c.h_));
    return c;
  }
  // device copies of both arrays (gm_crs_to_bases), the inverse of from_bases
  std::pair<CommitterKey, G2Bases> bases() const {
    const std::pair<size_t, size_t> n = len();
    CommitterKey k1;
    G2Bases k2;
    gm::check(gm_crs_to_bases(h_, &k1.h_, &k2.h_));
    k1.n_ = n.first;
    k2.n_ = n.second;
    return std::pair<CommitterKey, G2Bases>(std::move(k1), std::move(k2));
  }
  KeyCheck check() const {  // curve and subgroup over both arrays (gm_crs_check)
    KeyCheck r;
    int ok = 0;
    gm::check(gm_crs_check(h_, &r.first_bad_g1, &r.first_bad_g2, &ok));
    r.ok = ok != 0;
    return r;
  }
  Crs(Crs&& o) noexcept : h_(o.h_) { o.h_ = 0; }
  ~Crs() {
    if (h_) gm_crs_free(h_);
  }
  Crs(const Crs&) = delete;
  Crs& operator=(const Crs&) = delete;
  // the CRS must be longer than the scalars (ipa.rs:180,186)
  G1Projective commit_g1(const std::vector<Fr>& scalars) const {
    G1Projective out;
    gm::check(gm_crs_commit_g1(h_, scalars.empty() ? nullptr : scalars[0].data(), scalars.size(), out.data()));
    return out;
  }
  G2Projective commit_g2(const std::vector<Fr>& scalars) const {
    G2Projective out;
    gm::check(gm_crs_commit_g2(h_, scalars.empty() ? nullptr : scalars[0].data(), scalars.size(), out.data()));
    return out;
  }
  uint64_t handle() const { return h_; }

 private:
  Crs() = default;
  uint64_t h_ = 0;
};

class Vrs {  // ipa.rs:68-71,215-247
 public:
  explicit Vrs(const Crs& crs) { check(gm_vrs_from_crs(crs.handle(), &h_)); }
  Vrs(Vrs&& o) noexcept : h_(o.h_) { o.h_ = 0; }
  ~Vrs() {
    if (h_) gm_vrs_free(h_);
  }
  Vrs(const Vrs&) = delete;
  Vrs& operator=(const Vrs&) = delete;
  size_t levels() const {
    size_t n = 0;
    check(gm_vrs_levels(h_, &n));
    return n;
  }
  // (vk1, vk2) of a level, each (even, odd)
  std::pair<std::pair<Gt, Gt>, std::pair<Gt, Gt>> level(size_t l) const {
    uint64_t a[144], b[144];
    check(gm_vrs_get(h_, l, a, b));
    std::pair<std::pair<Gt, Gt>, std::pair<Gt, Gt>> r;
    memcpy(r.first.first.data(), a, 576);
    memcpy(r.first.second.data(), a + 72, 576);
    memcpy(r.second.first.data(), b, 576);
    memcpy(r.second.second.data(), b + 72, 576);
    return r;
  }
  uint64_t handle() const { return h_; }

 private:
  uint64_t h_ = 0;
};

class InnerProductProof {  // ipa.rs:54-60
 public:
  // InnerProductProof::new(transcript, crs, (a, b)): |a| = |b| >= 2, the CRS holds max(|a| + 1, 2^rounds) points
  InnerProductProof(Transcript& transcript, const Crs& crs, const std::vector<Fr>& a, const std::vector<Fr>& b) {
    if (a.size() != b.size()) throw Error(GM_EINVAL, "InnerProductProof: |a| != |b|");
    check(gm_ipa_new(transcript.handle(), crs.handle(), a.empty() ? nullptr : a[0].data(), b.empty() ? nullptr : b[0].data(), a.size(), &h_));
  }
  InnerProductProof(InnerProductProof&& o) noexcept : h_(o.h_) { o.h_ = 0; }
  ~InnerProductProof() {
    if (h_) gm_ipa_free(h_);
  }
  InnerProductProof(const InnerProductProof&) = delete;
  InnerProductProof& operator=(const InnerProductProof&) = delete;
  size_t rounds() const {
    size_t r = 0;
    check(gm_ipa_rounds(h_, &r));
    return r;
  }
  std::vector<GtRoundMsg> messages() const {  // sumcheck.messages
    std::vector<GtRoundMsg> m(rounds());
    static_assert(sizeof(GtRoundMsg) == 1152, "GtRoundMsg is a || b");
    check(gm_ipa_messages(h_, (uint64_t*)m.data()));
    return m;
  }
  std::vector<Fr> challenges() const {  // sumcheck.challenges
    std::vector<Fr> c(rounds());
    check(gm_ipa_challenges(h_, c[0].data()));
    return c;
  }
  std::vector<Fr> batch_challenges() const {  // 3 K + 2 (rounds - 1): 2 rounds + 1 for one claim
    std::vector<Fr> c(3 * claims() + 2 * (rounds() - 1));
    check(gm_ipa_batch_challenges(h_, c[0].data()));
    return c;
  }
  std::vector<std::pair<G1Projective, G2Projective>> final_foldings() const {  // sumcheck.final_foldings
    const size_t k = 2 * (rounds() - 1);
    std::vector<G1Projective> l(k);
    std::vector<G2Projective> r(k);
    check(gm_ipa_final_foldings(h_, k ? l[0].data() : nullptr, k ? r[0].data() : nullptr));
    std::vector<std::pair<G1Projective, G2Projective>> out(k);
    for (size_t i = 0; i < k; i++) out[i] = {l[i], r[i]};
    return out;
  }
  std::pair<Fr, Fr> foldings_ff() const {
    uint64_t v[8];
    check(gm_ipa_foldings_ff(h_, v));
    std::pair<Fr, Fr> r;
    memcpy(r.first.data(), v, 32);
    memcpy(r.second.data(), v + 4, 32);
    return r;
  }
  std::pair<G1Projective, Fr> foldings_fg1() const {
    std::pair<G1Projective, Fr> r;
    check(gm_ipa_foldings_fg1(h_, r.first.data(), r.second.data()));
    return r;
  }
  std::pair<Fr, G2Projective> foldings_fg2() const {
    std::pair<Fr, G2Projective> r;
    check(gm_ipa_foldings_fg2(h_, r.first.data(), r.second.data()));
    return r;
  }
  // every G1 and G2 element verify_transcript reads from the proof, the G1 ones first (gm_ipa_check); the GT elements: check_messages
  ProofCheck check_points() const {
    ProofCheck r;
    int ok = 0;
    check(gm_ipa_check(h_, &r.first_bad, &ok));
    r.ok = ok != 0;
    return r;
  }
  // GT membership of the 2 rounds message elements (gm_ipa_check_gt): a of round i is index 2 i, b is 2 i + 1
  ProofCheck check_messages() const {
    ProofCheck r;
    int ok = 0;
    check(gm_ipa_check_gt(h_, &r.first_bad, &ok));
    r.ok = ok != 0;
    return r;
  }
  // verify_transcript (ipa.rs:250-343): true for Ok(())
  bool verify_transcript(const Vrs& vrs, const G1Projective& comm_a, const G2Projective& comm_b, const Fr& y) const {
    int ok = 0;
    check(gm_ipa_verify(h_, vrs.handle(), comm_a.data(), comm_b.data(), y.data(), &ok));
    return ok != 0;
  }
  // [proofs[s]->verify_transcript(vrs, comm_a[s], comm_b[s], y[s]) for every s] from ONE launch group whatever their number
  // (gm_ipa_verify_many); the proofs may differ in their rounds, and the answers are the single entry's for every input
  static std::vector<bool> verify_many(const std::vector<const InnerProductProof*>& proofs, const Vrs& vrs, const std::vector<G1Projective>& comm_a,
                                       const std::vector<G2Projective>& comm_b, const std::vector<Fr>& y) {
    const size_t S = proofs.size();
    if (comm_a.size() != S || comm_b.size() != S || y.size() != S) throw Error(GM_EINVAL, "InnerProductProof::verify_many: one commitment pair and one y per proof");
    std::vector<uint64_t> h(S);
    for (size_t s = 0; s < S; s++) h[s] = proofs[s]->handle();
    std::vector<int> ok(S, 0);
    check(gm_ipa_verify_many(h.data(), vrs.handle(), S ? comm_a[0].data() : nullptr, S ? comm_b[0].data() : nullptr, S ? y[0].data() : nullptr, S, ok.data()));
    std::vector<bool> r(S);
    for (size_t s = 0; s < S; s++) r[s] = ok[s] != 0;
    return r;
  }
  // [InnerProductProof(*transcripts[s], crs, a[s], b[s]) for every s], byte for byte, the rounds of all proofs in lockstep: one
  // launch group per round whatever their number (gm_ipa_new_many).  One length for all vectors; a transcript per proof
  static std::vector<InnerProductProof> new_many(const std::vector<Transcript*>& transcripts, const Crs& crs, const std::vector<std::vector<Fr>>& a,
                                                 const std::vector<std::vector<Fr>>& b) {
    const size_t S = transcripts.size(), d = S ? a.at(0).size() : 0;
    if (a.size() != S || b.size() != S) throw Error(GM_EINVAL, "InnerProductProof::new_many: one pair of vectors per transcript");
    std::vector<uint64_t> t(S), h(S, 0);
    std::vector<Fr> fa, fb;
    for (size_t s = 0; s < S; s++) {
      if (a[s].size() != d || b[s].size() != d) throw Error(GM_EINVAL, "InnerProductProof::new_many: the vectors of one call have one length");
      t[s] = transcripts[s]->handle();
      fa.insert(fa.end(), a[s].begin(), a[s].end());
      fb.insert(fb.end(), b[s].begin(), b[s].end());
    }
    check(gm_ipa_new_many(t.data(), crs.handle(), fa.empty() ? nullptr : fa[0].data(), fb.empty() ? nullptr : fb[0].data(), d, S, h.data()));
    std::vector<InnerProductProof> out;
    out.reserve(S);
    for (size_t s = 0; s < S; s++) out.push_back(InnerProductProof(h[s]));
    return out;
  }
  // ONE proof for the K claims <a[i], b[i]> = y[i], <a[i], crs.g1> = comm_a[i], <b[i], crs.g2> = comm_b[i] (gm_ipa_new_batch:
  // InnerProductProof::generic, ipa.rs:345-531, over the CRS with every twist one): one transcript, one set of round messages.
  // One length for all vectors.  K = 1 is the constructor's proof byte for byte
  static InnerProductProof new_batch(Transcript& transcript, const Crs& crs, const std::vector<std::vector<Fr>>& a, const std::vector<std::vector<Fr>>& b) {
    const size_t K = a.size(), d = K ? a[0].size() : 0;
    if (b.size() != K) throw Error(GM_EINVAL, "InnerProductProof::new_batch: one b per a");
    std::vector<Fr> fa, fb;
    for (size_t i = 0; i < K; i++) {
      if (a[i].size() != d || b[i].size() != d) throw Error(GM_EINVAL, "InnerProductProof::new_batch: the vectors of one proof have one length");
      fa.insert(fa.end(), a[i].begin(), a[i].end());
      fb.insert(fb.end(), b[i].begin(), b[i].end());
    }
    uint64_t h = 0;
    Fr none{};  // K = 0 or d = 0 is refused by the library, which wants pointers to say so
    check(gm_ipa_new_batch(transcript.handle(), crs.handle(), fa.empty() ? none.data() : fa[0].data(), fb.empty() ? none.data() : fb[0].data(), d, K, &h));
    return InnerProductProof(h);
  }
  // K of a new_batch proof, 1 for every other (gm_ipa_claims)
  size_t claims() const {
    size_t K = 0;
    check(gm_ipa_claims(h_, &K));
    return K;
  }
  // the foldings of all K claims (gm_ipa_foldings_batch); foldings_ff / _fg1 / _fg2 above are for proofs of one claim
  struct BatchFoldings {
    std::vector<std::pair<Fr, Fr>> ff;
    std::vector<std::pair<G1Projective, Fr>> fg1;
    std::vector<std::pair<Fr, G2Projective>> fg2;
  };
  BatchFoldings foldings_batch() const {
    const size_t K = claims();
    std::vector<uint64_t> ff(K * 8), fg1(K * 22), fg2(K * 40);
    check(gm_ipa_foldings_batch(h_, ff.data(), fg1.data(), fg2.data()));
    BatchFoldings r;
    r.ff.resize(K);
    r.fg1.resize(K);
    r.fg2.resize(K);
    for (size_t i = 0; i < K; i++) {
      memcpy(r.ff[i].first.data(), ff.data() + 8 * i, 32);
      memcpy(r.ff[i].second.data(), ff.data() + 8 * i + 4, 32);
      memcpy(r.fg1[i].first.data(), fg1.data() + 22 * i, 18 * 8);
      memcpy(r.fg1[i].second.data(), fg1.data() + 22 * i + 18, 32);
      memcpy(r.fg2[i].first.data(), fg2.data() + 40 * i, 32);
      memcpy(r.fg2[i].second.data(), fg2.data() + 40 * i + 4, 36 * 8);
    }
    return r;
  }
  // verify_transcript with 3 K initial claims (gm_ipa_verify_batch): true for Ok(()); K = y.size() must be the proof's
  bool verify_batch(const Vrs& vrs, const std::vector<G1Projective>& comm_a, const std::vector<G2Projective>& comm_b, const std::vector<Fr>& y) const {
    const size_t K = y.size();
    if (K == 0 || comm_a.size() != K || comm_b.size() != K) throw Error(GM_EINVAL, "InnerProductProof::verify_batch: one commitment pair and one y per claim");
    int ok = 0;
    check(gm_ipa_verify_batch(h_, vrs.handle(), comm_a[0].data(), comm_b[0].data(), y[0].data(), K, &ok));
    return ok != 0;
  }
  // of the last new_batch call: split-fold launches, MSM calls, Miller launches (gm_debug_ipa_new_batch_path); none depends on K
  static std::array<size_t, 3> new_batch_path() {
    std::array<size_t, 3> c{};
    check(gm_debug_ipa_new_batch_path(c.data()));
    return c;
  }
  // fewer proofs than this are made one by one (gm_set_ipa_new_many_min); the bytes do not depend on it
  static void set_new_many_min(size_t proofs) { check(gm_set_ipa_new_many_min(proofs)); }
  // of the last new_many call: proofs on the lockstep path, on the per-proof path, kernel launches and stream waits of the lockstep path
  static std::array<size_t, 4> new_many_path() {
    std::array<size_t, 4> c{};
    check(gm_debug_ipa_new_many_path(c.data()));
    return c;
  }
  uint64_t handle() const { return h_; }

 private:
  explicit InnerProductProof(uint64_t h) : h_(h) {}
  uint64_t h_ = 0;
};

// src/subprotocols/sumcheck/proof.rs:19-66,125-130
struct Sumcheck {
  std::vector<RoundMsg> messages;
  std::vector<Fr> challenges;
  size_t rounds = 0;
  std::vector<std::array<Fr, 2>> final_foldings;

  static Sumcheck prove(Transcript& transcript, TimeProver& prover) {
    Sumcheck s;
    std::optional<Fr> verifier_message;
    while (auto message = prover.next_message(verifier_message)) {
      transcript.append_serializable("evaluations", *message);
      Fr challenge = transcript.get_challenge("challenge");
      verifier_message = challenge;
      s.messages.push_back(*message);
      s.challenges.push_back(challenge);
    }
    s.rounds = prover.rounds();
    auto ff = prover.final_foldings();
    if (!ff) throw Error(GM_ESTATE, "final foldings unavailable");
    s.final_foldings.push_back(*ff);
    transcript.append_serializable("final-folding", (*ff)[0]);
    transcript.append_serializable("final-folding", (*ff)[1]);
    return s;
  }
  static Sumcheck new_time(Transcript& transcript, const std::vector<Fr>& f, const std::vector<Fr>& g, const Fr& twist) {
    TimeProver prover(f, g, twist);
    return prove(transcript, prover);
  }
  // proof.rs:69-122, the round loop inside the library (gm_sumcheck_prove_batch); final_foldings: one (lhs, rhs) per prover
  static Sumcheck prove_batch(Transcript& transcript, std::vector<TimeProver>& provers) {
    size_t cap = 1;
    std::vector<uint64_t> handles;
    for (auto& p : provers) {
      cap = p.rounds() + 1 > cap ? p.rounds() + 1 : cap;
      handles.push_back(p.handle());
    }
    std::vector<uint64_t> msgs(cap * 8), chs(cap * 4), ff(provers.size() * 8 + 8);
    size_t rounds = 0;
    check(gm_sumcheck_prove_batch(transcript.handle(), handles.data(), handles.size(), msgs.data(), chs.data(), cap, ff.data(), &rounds));
    Sumcheck s;
    s.rounds = rounds;
    s.messages.resize(rounds);
    s.challenges.resize(rounds);
    for (size_t i = 0; i < rounds; i++) {
      memcpy(s.messages[i].a.data(), msgs.data() + 8 * i, 32);
      memcpy(s.messages[i].b.data(), msgs.data() + 8 * i + 4, 32);
      memcpy(s.challenges[i].data(), chs.data() + 4 * i, 32);
    }
    s.final_foldings.resize(provers.size());
    for (size_t j = 0; j < provers.size(); j++) memcpy(s.final_foldings[j].data(), ff.data() + 8 * j, 64);
    return s;
  }
};

// `Matrix<F> = Vec<Vec<(F, usize)>>` (src/circuit.rs:43) resident in HBM as CSR, together with its transpose (the
// prover needs column sums, src/snark/time_prover.rs:63-81)
using Matrix = std::vector<std::vector<std::pair<Fr, size_t>>>;
class DeviceMatrix {
 public:
  DeviceMatrix(const Matrix& rows, size_t ncols, bool transpose) {
    const size_t out_rows = transpose ? ncols : rows.size(), out_cols = transpose ? rows.size() : ncols;
    std::vector<uint64_t> rowptr(out_rows + 1, 0);
    for (size_t i = 0; i < rows.size(); i++)
      for (auto& e : rows[i]) rowptr[(transpose ? e.second : i) + 1]++;
    for (size_t i = 0; i < out_rows; i++) rowptr[i + 1] += rowptr[i];
    const size_t nnz = rowptr[out_rows];
    std::vector<uint32_t> cols(nnz);
    std::vector<Fr> vals(nnz);
    std::vector<uint64_t> cur(rowptr.begin(), rowptr.end() - 1);
    for (size_t i = 0; i < rows.size(); i++)
      for (auto& e : rows[i]) {
        const size_t r = transpose ? e.second : i, c = transpose ? i : e.second;
        cols[cur[r]] = (uint32_t)c;
        vals[cur[r]++] = e.first;
      }
    check(gm_spm_register(rowptr.data(), cols.data(), nnz ? vals[0].data() : nullptr, out_rows, out_cols, nnz, &h_));
  }
  ~DeviceMatrix() {
    if (h_) gm_spm_free(h_);
  }
  DeviceMatrix(const DeviceMatrix&) = delete;
  DeviceMatrix& operator=(const DeviceMatrix&) = delete;
  uint64_t handle() const { return h_; }

 private:
  uint64_t h_ = 0;
};

// src/circuit.rs `R1cs { a, b, c, z, w, x }` with everything the prover touches on the device
class R1cs {
 public:
  R1cs(const Matrix& a, const Matrix& b, const Matrix& c, const std::vector<Fr>& z, const std::vector<Fr>& w)
      : a_(a, z.size(), false), b_(b, z.size(), false), c_(c, z.size(), false), at_(a, z.size(), true), bt_(b, z.size(), true),
        ct_(c, z.size(), true), nz_(z.size()) {
    check(gm_fr_vec_alloc(z.size(), &z_));
    check(gm_fr_vec_alloc(w.size(), &w_));
    if (!z.empty()) check(gm_fr_vec_upload(z_, 0, z[0].data(), z.size()));
    if (!w.empty()) check(gm_fr_vec_upload(w_, 0, w[0].data(), w.size()));
  }
  ~R1cs() {
    if (z_) gm_fr_vec_free(z_);
    if (w_) gm_fr_vec_free(w_);
  }
  R1cs(const R1cs&) = delete;
  R1cs& operator=(const R1cs&) = delete;

 private:
  friend struct SnarkProof;
  friend class PsnarkInstance;
  friend struct PsnarkProof;
  DeviceMatrix a_, b_, c_, at_, bt_, ct_;
  uint64_t z_ = 0, w_ = 0;
  size_t nz_;
};

// `Vec<F>` / `&[usize]` resident in HBM: what the stand-alone sub-protocols below take and return
class DeviceVec {
 public:
  explicit DeviceVec(const std::vector<Fr>& v) {
    check(gm_fr_vec_alloc(v.size(), &h_));
    if (!v.empty()) {
      const int rc = gm_fr_vec_upload(h_, 0, v[0].data(), v.size());
      if (rc) {
        gm_fr_vec_free(h_);
        check(rc);
      }
    }
  }
  static DeviceVec from_handle(uint64_t handle) {  // a vector the library created; owned from here
    DeviceVec d;
    d.h_ = handle;
    return d;
  }
  DeviceVec(DeviceVec&& o) noexcept : h_(o.h_) { o.h_ = 0; }
  DeviceVec(const DeviceVec&) = delete;
  DeviceVec& operator=(const DeviceVec&) = delete;
  ~DeviceVec() {
    if (h_) gm_fr_vec_free(h_);
  }
  size_t size() const {
    size_t n = 0;
    check(gm_fr_vec_len(h_, &n));
    return n;
  }
  std::vector<Fr> to_host() const {
    std::vector<Fr> out(size());
    if (!out.empty()) check(gm_fr_vec_download(h_, 0, out[0].data(), out.size()));
    return out;
  }
  uint64_t handle() const { return h_; }

 private:
  DeviceVec() = default;
  uint64_t h_ = 0;
};
// ---- herring: SpaceProver over G1Module / G2Module (src/herring/space_prover.rs:39-316; the block of the same name in gemini_hip.h) ----
// The point side is a run of a registered key, read where it lies; the Fr side a DeviceVec holding the big-endian stream.  Key and
// vector outlive the prover.  The messages carry the twist, a TimeProver's do not: the two agree at twist = 1
namespace detail {
template <class T>
class HerringModuleSpaceProver {
 public:
  // the points key[offset .. offset + n) of a key handle (CommitterKey::handle / G2Bases::handle) and an Fr stream
  HerringModuleSpaceProver(uint64_t key_handle, size_t offset, size_t n, const DeviceVec& fr_stream, const Fr& twist) {
    check(T::create(key_handle, offset, n, fr_stream.handle(), twist.data(), &h_));
  }
  HerringModuleSpaceProver(HerringModuleSpaceProver&& o) noexcept : h_(o.h_) { o.h_ = 0; }
  ~HerringModuleSpaceProver() {
    if (h_) T::free(h_);
  }
  HerringModuleSpaceProver(const HerringModuleSpaceProver&) = delete;
  HerringModuleSpaceProver& operator=(const HerringModuleSpaceProver&) = delete;
  std::optional<typename T::Time::Msg> next_message(const std::optional<Fr>& verifier_message) {
    typename T::Time::Msg m;
    int has = 0;
    check(T::round(h_, verifier_message ? verifier_message->data() : nullptr, m.a.data(), m.b.data(), &has));
    if (!has) return std::nullopt;
    return m;
  }
  void fold(const Fr& challenge) { check(T::fold(h_, challenge.data())); }
  size_t rounds() const {
    size_t t = 0;
    check(T::rounds(h_, &t, nullptr));
    return t;
  }
  size_t round() const {
    size_t r = 0;
    check(T::rounds(h_, nullptr, &r));
    return r;
  }
  std::optional<typename T::Time::Final> final_foldings() const {
    typename T::Time::Final ff;
    int has = 0;
    check(T::final_foldings(h_, ff.first.data(), ff.second.data(), &has));
    if (!has) return std::nullopt;
    return ff;
  }
  // TimeProver::from(&SpaceProver): the folded points in an allocation of its own; this prover stays valid
  HerringModuleProver<typename T::Time> to_time() const {
    uint64_t t = 0;
    check(T::to_time(h_, &t));
    return HerringModuleProver<typename T::Time>::from_handle(t);
  }
  // MSM calls, launches of k_hsp_scalars, point bytes allocated, scalar bytes allocated, so far (gm_debug_hsp_path)
  std::array<size_t, 4> path() const {
    std::array<size_t, 4> c{};
    check(gm_debug_hsp_path(h_, c.data()));
    return c;
  }
  uint64_t handle() const { return h_; }

 private:
  uint64_t h_ = 0;
};
struct HerringG1SpaceModule {
  using Time = HerringG1Module;
  static int create(uint64_t key, size_t offset, size_t n, uint64_t vec, const uint64_t* twist, uint64_t* h) { return gm_hsp1_new_borrow(key, offset, n, vec, twist, h); }
  static constexpr auto round = gm_hsp1_round;
  static constexpr auto fold = gm_hsp1_fold;
  static constexpr auto rounds = gm_hsp1_rounds;
  static constexpr auto final_foldings = gm_hsp1_final;
  static constexpr auto to_time = gm_hsp1_to_time;
  static constexpr auto free = gm_hsp1_free;
};
struct HerringG2SpaceModule {
  using Time = HerringG2Module;
  static int create(uint64_t key, size_t offset, size_t n, uint64_t vec, const uint64_t* twist, uint64_t* h) { return gm_hsp2_new_borrow(vec, key, offset, n, twist, h); }
  static constexpr auto round = gm_hsp2_round;
  static constexpr auto fold = gm_hsp2_fold;
  static constexpr auto rounds = gm_hsp2_rounds;
  static constexpr auto final_foldings = gm_hsp2_final;
  static constexpr auto to_time = gm_hsp2_to_time;
  static constexpr auto free = gm_hsp2_free;
};
}  // namespace detail
using HerringG1Space = detail::HerringModuleSpaceProver<detail::HerringG1SpaceModule>;
using HerringG2Space = detail::HerringModuleSpaceProver<detail::HerringG2SpaceModule>;

class IdxVec {
 public:
  explicit IdxVec(const std::vector<uint32_t>& index) { check(gm_idx_register(index.data(), index.size(), &h_)); }
  // extend_frequency(compute_frequency(set_len, index)) built on the device   plookup/time_prover.rs:65-78
  IdxVec extend_frequency(size_t set_len) const {
    IdxVec e;
    size_t n = 0;
    check(gm_idx_extend_frequency(h_, set_len, &e.h_, &n));
    return e;
  }
  IdxVec(IdxVec&& o) noexcept : h_(o.h_) { o.h_ = 0; }
  IdxVec(const IdxVec&) = delete;
  IdxVec& operator=(const IdxVec&) = delete;
  ~IdxVec() {
    if (h_) gm_idx_free(h_);
  }
  size_t size() const {
    size_t n = 0;
    check(gm_idx_len(h_, &n));
    return n;
  }
  std::vector<uint32_t> to_host() const {
    std::vector<uint32_t> out(size());
    check(gm_idx_download(h_, out.data()));
    return out;
  }
  uint64_t handle() const { return h_; }

 private:
  IdxVec() = default;
  uint64_t h_ = 0;
};

// src/subprotocols/tensorcheck/mod.rs:110-121
struct TensorcheckProof {
  std::vector<G1Projective> folded_polynomials_commitments;
  std::vector<std::array<Fr, 2>> folded_polynomials_evaluations;
  G1Projective evaluation_proof;
  std::vector<std::array<Fr, 3>> base_polynomials_evaluations;

  // :190-275 (gm_tensorcheck_new_time).  A body: the polynomials batched together and the tensor challenges they fold by
  struct Body {
    std::vector<const DeviceVec*> polynomials;
    std::vector<Fr> challenges;
  };
  static TensorcheckProof new_time(Transcript& transcript, const CommitterKey& ck, const std::vector<const DeviceVec*>& base_polynomials,
                                   const std::vector<Body>& body_polynomials) {
    std::vector<uint64_t> bases;
    for (auto* p : base_polynomials) bases.push_back(p->handle());
    std::vector<std::vector<uint64_t>> polys(body_polynomials.size());
    std::vector<gm_tensorcheck_body> bodies(body_polynomials.size());
    size_t nfold = 0;
    for (size_t b = 0; b < body_polynomials.size(); b++) {
      const Body& B = body_polynomials[b];
      for (auto* p : B.polynomials) polys[b].push_back(p->handle());
      bodies[b] = gm_tensorcheck_body{polys[b].data(), polys[b].size(), B.challenges.empty() ? nullptr : B.challenges[0].data(), B.challenges.size()};
      nfold += B.challenges.empty() ? 0 : B.challenges.size() - 1;
    }
    TensorcheckProof out;
    out.folded_polynomials_commitments.resize(nfold);
    out.folded_polynomials_evaluations.resize(nfold);
    out.base_polynomials_evaluations.resize(bases.size());
    gm_tensorcheck_proof p;
    memset(&p, 0, sizeof p);
    p.cap_folds = nfold;
    p.fold_commitments = nfold ? out.folded_polynomials_commitments[0].data() : nullptr;
    p.fold_evaluations = nfold ? out.folded_polynomials_evaluations[0][0].data() : nullptr;
    p.nbase = bases.size();
    p.base_evaluations = bases.empty() ? nullptr : out.base_polynomials_evaluations[0][0].data();
    check(gm_tensorcheck_new_time(transcript.handle(), ck.handle(), bases.data(), bases.size(), bodies.data(), bodies.size(), &p));
    memcpy(out.evaluation_proof.data(), p.evaluation_proof, 144);
    return out;
  }
};

// src/subprotocols/entryproduct/mod.rs:21-31 + time_prover.rs:61-147 (gm_entryproduct_new_time_batch): the provers own their data
struct EntryProduct {
  struct ProverMsgs {
    std::vector<G1Projective> acc_v_commitments;
    std::vector<Fr> claimed_sumchecks;
  };
  ProverMsgs msgs;
  Fr chal;
  std::vector<TimeProver> provers;

  static EntryProduct new_time_batch(Transcript& transcript, const CommitterKey& ck, const std::vector<const DeviceVec*>& vs,
                                     const std::vector<Fr>& claimed_products) {
    if (vs.size() != claimed_products.size()) throw Error(GM_EINVAL, "EntryProduct::new_time_batch: one claimed product per vector");
    const size_t k = vs.size();
    std::vector<uint64_t> hv, hp(k, 0);
    for (auto* v : vs) hv.push_back(v->handle());
    EntryProduct ep;
    ep.msgs.acc_v_commitments.resize(k);
    ep.msgs.claimed_sumchecks.resize(k);
    check(gm_entryproduct_new_time_batch(transcript.handle(), ck.handle(), hv.data(), nullptr, k, k ? claimed_products[0].data() : nullptr,
                                         k ? ep.msgs.acc_v_commitments[0].data() : nullptr, k ? ep.msgs.claimed_sumchecks[0].data() : nullptr,
                                         ep.chal.data(), hp.data()));
    for (uint64_t h : hp) ep.provers.push_back(TimeProver::from_handle(h));
    return ep;
  }
  static EntryProduct new_time(Transcript& transcript, const CommitterKey& ck, const DeviceVec& v, const Fr& claimed_product) {
    return new_time_batch(transcript, ck, {&v}, {claimed_product});
  }
};

// plookup(subset, set, index, y, z, zeta) -> {lookup_set, lookup_subset, lookup_sorted}   plookup/time_prover.rs:89-112
// ext_fre: index.extend_frequency(set.size()) when the caller keeps it across proofs; null: built on the device inside the call
inline std::array<DeviceVec, 3> plookup(const DeviceVec& subset, const DeviceVec& set, const IdxVec& index, const Fr& y, const Fr& z, const Fr& zeta,
                                        const IdxVec* ext_fre = nullptr) {
  uint64_t out[3] = {0, 0, 0};
  check(gm_plookup_new_time(subset.handle(), set.handle(), index.handle(), ext_fre ? ext_fre->handle() : 0, y.data(), z.data(), zeta.data(), out));
  return {DeviceVec::from_handle(out[0]), DeviceVec::from_handle(out[1]), DeviceVec::from_handle(out[2])};
}

// kzg::VerifierKey (src/kzg/mod.rs:141-149) held by the library: the first max_eval_points powers of g and max_eval_points + 1 of g2.
// verify / verify_multi_points answer true (accepted) or false (rejected); misuse throws gm::Error like everything else here
class VerifierKey {
 public:
  VerifierKey(const std::vector<G1Affine>& powers_of_g, const std::vector<G2Affine>& powers_of_g2) {
    gm::check(gm_vk_new(powers_of_g.data(), sizeof(G1Affine), powers_of_g.size(), powers_of_g2.data(), sizeof(G2Affine), powers_of_g2.size(), &h_));
  }
  // the setup aid that pairs with gm_g1_srs_register: tau canonical, g and g2 as 12 / 24 Montgomery limbs
  static VerifierKey from_trapdoor(const uint64_t g_affine[12], const uint64_t g2_affine[24], const BigInt& tau, size_t max_eval_points) {
    VerifierKey k;
    gm::check(gm_vk_from_trapdoor(g_affine, g2_affine, tau.data(), max_eval_points, &k.h_));
    return k;
  }
  VerifierKey(VerifierKey&& o) noexcept : h_(o.h_) { o.h_ = 0; }
  ~VerifierKey() {
    if (h_) gm_vk_free(h_);
  }
  VerifierKey(const VerifierKey&) = delete;
  VerifierKey& operator=(const VerifierKey&) = delete;
  uint64_t handle() const { return h_; }
  // every power of both halves canonical, on its curve and in its subgroup (gm_vk_check): run it on a key from elsewhere BEFORE verify
  KeyCheck check() const {
    KeyCheck r;
    int ok = 0;
    gm::check(gm_vk_check(h_, &r.first_bad_g1, &r.first_bad_g2, &ok));
    r.ok = ok != 0;
    return r;
  }
  // serialize_uncompressed(&powers_of_g2): what psnark absorbs as b"ck" (PsnarkProof::new_time's ck_g2_bytes)
  std::vector<uint8_t> g2_bytes(int encoding = 0) const {
    size_t n = 0;
    gm::check(gm_vk_g2_bytes(h_, encoding, nullptr, 0, &n));
    std::vector<uint8_t> out(n);
    gm::check(gm_vk_g2_bytes(h_, encoding, out.data(), n, &n));
    return out;
  }
  bool verify(const G1Projective& commitment, const Fr& alpha, const Fr& evaluation, const G1Projective& proof) const {  // src/kzg/mod.rs:155-175
    int ok = 0;
    gm::check(gm_kzg_verify(h_, commitment.data(), alpha.data(), evaluation.data(), proof.data(), &ok));
    return ok != 0;
  }
  // :181-244; evaluations: one row of eval_points.size() values per commitment
  bool verify_multi_points(const std::vector<G1Projective>& commitments, const std::vector<Fr>& eval_points, const std::vector<std::vector<Fr>>& evaluations,
                           const G1Projective& proof, const Fr& open_chal) const {
    std::vector<Fr> flat;
    for (auto& row : evaluations) {
      if (row.size() != eval_points.size()) throw Error(GM_EINVAL, "verify_multi_points: one value per evaluation point in every row");
      flat.insert(flat.end(), row.begin(), row.end());
    }
    int ok = 0;
    gm::check(gm_kzg_verify_multi_points(h_, commitments.empty() ? nullptr : commitments[0].data(), commitments.size(), eval_points.empty() ? nullptr : eval_points[0].data(),
                                     eval_points.size(), flat.empty() ? nullptr : flat[0].data(), evaluations.size(), proof.data(), open_chal.data(), &ok));
    return ok != 0;
  }
  // one verify_multi_points per entry, all of them in ONE batch of device work (gm_kzg_verify_multi_points_many): a verdict per check
  struct MultiPointsCheck {
    std::vector<G1Projective> commitments;
    std::vector<Fr> eval_points;
    std::vector<std::vector<Fr>> evaluations;
    G1Projective proof;
    Fr open_chal;
  };
  std::vector<bool> verify_multi_points_many(const std::vector<MultiPointsCheck>& checks) const {
    std::vector<uint64_t> cm, pts, ev, pr, ch;
    std::vector<size_t> co{0}, po{0}, ro{0};
    for (const MultiPointsCheck& c : checks) {
      for (auto& x : c.commitments) cm.insert(cm.end(), x.begin(), x.end());
      for (auto& x : c.eval_points) pts.insert(pts.end(), x.begin(), x.end());
      for (auto& row : c.evaluations) {
        if (row.size() != c.eval_points.size()) throw Error(GM_EINVAL, "verify_multi_points_many: one value per evaluation point in every row");
        for (auto& x : row) ev.insert(ev.end(), x.begin(), x.end());
      }
      pr.insert(pr.end(), c.proof.begin(), c.proof.end());
      ch.insert(ch.end(), c.open_chal.begin(), c.open_chal.end());
      co.push_back(co.back() + c.commitments.size());
      po.push_back(po.back() + c.eval_points.size());
      ro.push_back(ro.back() + c.evaluations.size());
    }
    std::vector<int> ok(checks.size() + 1, 0);
    cm.push_back(0), pts.push_back(0), ev.push_back(0), pr.push_back(0), ch.push_back(0);  // never null
    gm::check(gm_kzg_verify_multi_points_many(h_, checks.size(), cm.data(), co.data(), pts.data(), po.data(), ev.data(), ro.data(), pr.data(), ch.data(), ok.data()));
    return std::vector<bool>(ok.begin(), ok.begin() + checks.size());
  }

 private:
  VerifierKey() = default;
  uint64_t h_ = 0;
};

// src/snark/mod.rs:76-82 + Proof::new_time (src/snark/time_prover.rs:19-117): one call into the library
struct SnarkProof {
  G1Projective witness_commitment;
  Fr zc_alpha;
  std::vector<RoundMsg> first_sumcheck_msgs, second_sumcheck_msgs;
  std::array<Fr, 2> first_final_foldings, second_final_foldings;
  TensorcheckProof tensorcheck_proof;

  static SnarkProof new_time(const R1cs& r1cs, const CommitterKey& ck, int g1_encoding = 0) {
    Buffers b(r1cs.nz_);
    const uint64_t mats[6] = {r1cs.a_.handle(), r1cs.b_.handle(), r1cs.c_.handle(), r1cs.at_.handle(), r1cs.bt_.handle(), r1cs.ct_.handle()};
    check(gm_snark_new_time(mats, r1cs.z_, r1cs.w_, ck.handle(), g1_encoding, b.cap, &b.p));
    return b.unpack();
  }

  // Proof::new_elastic(r1cs_stream, ck_stream, max_msm_buffer) (src/snark/elastic_prover.rs:174-266): the streams of
  // R1csStream (`Reverse(..)` of z, w, A z, B z, C z: src/snark/tests.rs:38-52) are built here as reversed device vectors,
  // outside the prover like the reference's stream construction; the proof equals new_time's (src/snark/tests.rs:56)
  static SnarkProof new_elastic(const R1cs& r1cs, const CommitterKey& ck, size_t max_msm_buffer = (size_t)1 << 20,
                                size_t min_device_chunk = (size_t)1 << 26, int g1_encoding = 0) {
    struct Vec {
      uint64_t h = 0;
      explicit Vec(size_t n) { check(gm_fr_vec_alloc(n, &h)); }
      ~Vec() {
        if (h) gm_fr_vec_free(h);
      }
    };
    const size_t nz = r1cs.nz_;
    size_t nw = 0;
    check(gm_fr_vec_len(r1cs.w_, &nw));
    Vec z_be(nz), w_be(nw), tmp(nz), za(nz), zb(nz), zc(nz);
    check(gm_fr_reverse(r1cs.z_, z_be.h));
    check(gm_fr_reverse(r1cs.w_, w_be.h));
    const DeviceMatrix* m[3] = {&r1cs.a_, &r1cs.b_, &r1cs.c_};
    Vec* out[3] = {&za, &zb, &zc};
    for (int k = 0; k < 3; k++) {
      check(gm_spm_mul(m[k]->handle(), r1cs.z_, tmp.h));
      check(gm_fr_reverse(tmp.h, out[k]->h));
    }
    Buffers b(nz);
    const uint64_t mats_t[3] = {r1cs.at_.handle(), r1cs.bt_.handle(), r1cs.ct_.handle()};
    check(gm_snark_new_elastic(mats_t, z_be.h, w_be.h, za.h, zb.h, zc.h, ck.handle(), max_msm_buffer, min_device_chunk, g1_encoding, b.cap, &b.p));
    return b.unpack();
  }

  // every G1 element the verifier reads is canonical, on the curve and in G1 (gm_snark_proof_check); verify() does not call it
  ProofCheck check_points() const {
    const auto& tc = tensorcheck_proof;
    const size_t nf = tc.folded_polynomials_commitments.size();
    gm_snark_proof p;
    memset(&p, 0, sizeof p);
    std::vector<uint64_t> fc(18 * nf + 1);
    memcpy(p.witness_commitment, witness_commitment.data(), 144);
    for (size_t i = 0; i < nf; i++) memcpy(fc.data() + 18 * i, tc.folded_polynomials_commitments[i].data(), 144);
    p.nfold = nf;
    p.fold_commitments = fc.data();
    memcpy(p.evaluation_proof, tc.evaluation_proof.data(), 144);
    ProofCheck r;
    int ok = 0;
    check(gm_snark_proof_check(&p, &r.first_bad, &ok));
    r.ok = ok != 0;
    return r;
  }

  // Proof::verify(&r1cs, &vk) (src/snark/verifier.rs:19-119): true = accepted.  The proof may come from a prover or from its fields
  bool verify(const R1cs& r1cs, const VerifierKey& vk, int g1_encoding = 0) const {
    Packed P;
    if (!P.pack(*this)) return false;
    const PublicInput x(r1cs);
    const uint64_t mats[3] = {r1cs.a_.handle(), r1cs.b_.handle(), r1cs.c_.handle()};
    int ok = 0;
    check(gm_snark_verify(mats, x.h, vk.handle(), g1_encoding, &P.p, &ok));
    return ok != 0;
  }

  // The proofs under one set of matrices and one key in ONE call (gm_snark_verify_many): a verdict per proof, what verify() answers for
  // each.  x_vecs: the public input of every proof as a vector handle (0 = empty); empty = the instance's own for all of them
  static std::vector<bool> verify_many(const std::vector<const SnarkProof*>& proofs, const R1cs& r1cs, const VerifierKey& vk, const std::vector<uint64_t>& x_vecs = {},
                                       int g1_encoding = 0) {
    if (!x_vecs.empty() && x_vecs.size() != proofs.size()) throw Error(GM_EINVAL, "verify_many: one public input per proof");
    std::vector<bool> out(proofs.size(), false);
    std::vector<Packed> packed(proofs.size());
    std::vector<gm_snark_proof> recs;
    std::vector<uint64_t> xs;
    std::vector<size_t> live;
    const PublicInput x(r1cs);
    for (size_t i = 0; i < proofs.size(); i++) {
      if (!packed[i].pack(*proofs[i])) continue;  // verify() rejects these without a call
      live.push_back(i);
      recs.push_back(packed[i].p);
      xs.push_back(x_vecs.empty() ? x.h : x_vecs[i]);
    }
    if (live.empty()) return out;
    const uint64_t mats[3] = {r1cs.a_.handle(), r1cs.b_.handle(), r1cs.c_.handle()};
    std::vector<int> ok(live.size(), 0);
    check(gm_snark_verify_many(mats, xs.data(), vk.handle(), g1_encoding, recs.data(), live.size(), ok.data()));
    for (size_t k = 0; k < live.size(); k++) out[live[k]] = ok[k] != 0;
    return out;
  }

  // the gm_snark_proof record of a proof and the arrays it points into
  struct Packed {
    gm_snark_proof p;
    std::vector<uint64_t> m[2], fc, fe;
    bool pack(const SnarkProof& s) {
      if (s.tensorcheck_proof.base_polynomials_evaluations.size() != 1) return false;
      const auto& tc = s.tensorcheck_proof;
      const size_t nf = tc.folded_polynomials_commitments.size();
      if (tc.folded_polynomials_evaluations.size() != nf) return false;
      memset(&p, 0, sizeof p);
      memcpy(p.witness_commitment, s.witness_commitment.data(), 144);
      memcpy(p.zc_alpha, s.zc_alpha.data(), 32);
      fc.assign(18 * nf + 1, 0);
      fe.assign(8 * nf + 1, 0);
      const std::vector<RoundMsg>* msgs[2] = {&s.first_sumcheck_msgs, &s.second_sumcheck_msgs};
      for (int k = 0; k < 2; k++) {
        m[k].assign(8 * msgs[k]->size() + 1, 0);
        for (size_t i = 0; i < msgs[k]->size(); i++) {
          memcpy(m[k].data() + 8 * i, (*msgs[k])[i].a.data(), 32);
          memcpy(m[k].data() + 8 * i + 4, (*msgs[k])[i].b.data(), 32);
        }
        p.rounds[k] = msgs[k]->size();
        p.messages[k] = m[k].data();
      }
      memcpy(p.final_foldings[0], s.first_final_foldings.data(), 64);
      memcpy(p.final_foldings[1], s.second_final_foldings.data(), 64);
      for (size_t i = 0; i < nf; i++) {
        memcpy(fc.data() + 18 * i, tc.folded_polynomials_commitments[i].data(), 144);
        memcpy(fe.data() + 8 * i, tc.folded_polynomials_evaluations[i].data(), 64);
      }
      p.nfold = nf;
      p.fold_commitments = fc.data();
      p.fold_evaluations = fe.data();
      memcpy(p.evaluation_proof, tc.evaluation_proof.data(), 144);
      memcpy(p.base_evaluations, tc.base_polynomials_evaluations[0].data(), 96);
      return true;
    }
  };

  // x = the entries of z in front of the witness (src/circuit.rs: z = x || w), as a vector of its own for the verifiers
  struct PublicInput {
    uint64_t h = 0;
    explicit PublicInput(const R1cs& r1cs) {
      size_t nw = 0;
      check(gm_fr_vec_len(r1cs.w_, &nw));
      const size_t nx = r1cs.nz_ > nw ? r1cs.nz_ - nw : 0;
      check(gm_fr_vec_alloc(nx, &h));
      if (nx) {
        const int rc = gm_fr_stride(r1cs.z_, 0, 1, nx, h);
        if (rc) {
          gm_fr_vec_free(h);
          check(rc);
        }
      }
    }
    ~PublicInput() {
      if (h) gm_fr_vec_free(h);
    }
    PublicInput(const PublicInput&) = delete;
    PublicInput& operator=(const PublicInput&) = delete;
  };

 private:
  // the plain-C proof record of the library and its caller-owned arrays
  struct Buffers {
    size_t cap = 2;
    std::vector<uint64_t> m0, m1, fc, fe;
    gm_snark_proof p;
    explicit Buffers(size_t nz) {
      for (size_t n = nz; n > 1; n = (n + 1) / 2) cap++;
      m0.resize(cap * 8);
      m1.resize(cap * 8);
      fc.resize(cap * 18);
      fe.resize(cap * 8);
      memset(&p, 0, sizeof p);
      p.messages[0] = m0.data();
      p.messages[1] = m1.data();
      p.fold_commitments = fc.data();
      p.fold_evaluations = fe.data();
    }
    SnarkProof unpack() const {
      SnarkProof out;
      memcpy(out.witness_commitment.data(), p.witness_commitment, 144);
      memcpy(out.zc_alpha.data(), p.zc_alpha, 32);
      auto msgs = [](const uint64_t* m, size_t rounds) {
        std::vector<RoundMsg> v(rounds);
        for (size_t i = 0; i < rounds; i++) {
          memcpy(v[i].a.data(), m + 8 * i, 32);
          memcpy(v[i].b.data(), m + 8 * i + 4, 32);
        }
        return v;
      };
      out.first_sumcheck_msgs = msgs(m0.data(), p.rounds[0]);
      out.second_sumcheck_msgs = msgs(m1.data(), p.rounds[1]);
      memcpy(out.first_final_foldings.data(), p.final_foldings[0], 64);
      memcpy(out.second_final_foldings.data(), p.final_foldings[1], 64);
      auto& tc = out.tensorcheck_proof;
      tc.folded_polynomials_commitments.resize(p.nfold);
      tc.folded_polynomials_evaluations.resize(p.nfold);
      for (size_t i = 0; i < p.nfold; i++) {
        memcpy(tc.folded_polynomials_commitments[i].data(), fc.data() + 18 * i, 144);
        memcpy(tc.folded_polynomials_evaluations[i].data(), fe.data() + 8 * i, 64);
      }
      memcpy(tc.evaluation_proof.data(), p.evaluation_proof, 144);
      tc.base_polynomials_evaluations.resize(1);
      memcpy(tc.base_polynomials_evaluations[0].data(), p.base_evaluations, 96);
      return out;
    }
  };
};

// The preprocessing SNARK (src/psnark/mod.rs:29-51): the matrix-only part of the instance (`sum_matrices`, `joint_matrices`, the
// lookup frequencies; src/misc.rs:269-366) is built inside the library once per circuit and stays in HBM; `index` and `new_time`
// are one call each (src/psnark/time_prover.rs:49-64, 69-384).
class PsnarkInstance {
 public:
  explicit PsnarkInstance(const R1cs& r1cs) : r1cs_(r1cs) {
    memset(&rec_, 0, sizeof rec_);
    check(gm_psnark_preprocess(r1cs.a_.handle(), r1cs.b_.handle(), r1cs.c_.handle(), r1cs.nz_, &rec_));
    rec_.z = r1cs.z_;
    rec_.w = r1cs.w_;
  }
  ~PsnarkInstance() { gm_psnark_preprocess_free(&rec_); }
  PsnarkInstance(const PsnarkInstance&) = delete;
  PsnarkInstance& operator=(const PsnarkInstance&) = delete;
  size_t num_non_zero() const { return rec_.nnz; }
  // Proof::index: commitments to row, col, val_a, val_b, val_c
  std::array<G1Projective, 5> index(const CommitterKey& ck) const {
    std::array<G1Projective, 5> out;
    check(gm_psnark_index(&rec_, ck.handle(), out[0].data()));
    return out;
  }

 private:
  friend struct PsnarkProof;
  const R1cs& r1cs_;
  gm_psnark_instance rec_;
};

struct PsnarkProof {
  G1Projective witness_commitment;
  Fr zc_alpha;
  std::vector<RoundMsg> first_sumcheck_msgs, second_sumcheck_msgs, third_sumcheck_msgs;
  std::array<Fr, 2> first_final_foldings, second_final_foldings;
  std::array<std::array<Fr, 2>, 13> third_final_foldings;
  std::array<G1Projective, 3> r_star_commitments;
  G1Projective z_star_commitment;
  std::array<G1Projective, 3> sorted_commitments;  // r, alpha, z
  std::array<Fr, 9> products;                      // r (set, subset, sorted), alpha (..), z (..)
  std::array<G1Projective, 9> acc_v_commitments;
  std::array<Fr, 9> claimed_sumchecks;
  std::array<Fr, 10> ralpha_star_acc_mu_evals;
  G1Projective ralpha_star_acc_mu_proof;
  std::array<Fr, 2> rstars_vals;
  TensorcheckProof tensorcheck_proof;

  // `ck_g2_bytes`: the serialised G2 powers of the key as the transcript absorbs them (src/psnark/time_prover.rs:86-88)
  static PsnarkProof new_time(const CommitterKey& ck, const PsnarkInstance& inst, const std::array<G1Projective, 5>& index,
                              const std::vector<uint8_t>& ck_g2_bytes, int g1_encoding = 0) {
    gm_psnark_instance I = inst.rec_;
    I.index_commitments = index[0].data();
    I.ck_g2_bytes = ck_g2_bytes.data();
    I.ck_g2_len = ck_g2_bytes.size();
    size_t cap = 4;
    for (size_t n = 2 * (inst.r1cs_.nz_ > I.nnz ? inst.r1cs_.nz_ : I.nnz) + 4; n > 1; n = (n + 1) / 2) cap++;
    std::vector<uint64_t> m[3], fc(4 * cap * 18), fe(4 * cap * 8);
    gm_psnark_proof p;
    memset(&p, 0, sizeof p);
    for (int k = 0; k < 3; k++) {
      m[k].resize(cap * 8);
      p.messages[k] = m[k].data();
    }
    p.cap_folds = 4 * cap;
    p.fold_commitments = fc.data();
    p.fold_evaluations = fe.data();
    check(gm_psnark_new_time(&I, ck.handle(), g1_encoding, cap, &p));
    PsnarkProof out;
    auto msgs = [](const std::vector<uint64_t>& mm, size_t rounds) {
      std::vector<RoundMsg> v(rounds);
      for (size_t i = 0; i < rounds; i++) {
        memcpy(v[i].a.data(), mm.data() + 8 * i, 32);
        memcpy(v[i].b.data(), mm.data() + 8 * i + 4, 32);
      }
      return v;
    };
    memcpy(out.witness_commitment.data(), p.witness_commitment, 144);
    memcpy(out.zc_alpha.data(), p.zc_alpha, 32);
    out.first_sumcheck_msgs = msgs(m[0], p.rounds[0]);
    out.second_sumcheck_msgs = msgs(m[1], p.rounds[1]);
    out.third_sumcheck_msgs = msgs(m[2], p.rounds[2]);
    memcpy(out.first_final_foldings.data(), p.final_foldings[0], 64);
    memcpy(out.second_final_foldings.data(), p.final_foldings[1], 64);
    memcpy(out.third_final_foldings.data(), p.third_final_foldings, sizeof p.third_final_foldings);
    memcpy(out.r_star_commitments.data(), p.r_star_commitments, sizeof p.r_star_commitments);
    memcpy(out.z_star_commitment.data(), p.z_star_commitment, 144);
    memcpy(out.sorted_commitments.data(), p.sorted_commitments, sizeof p.sorted_commitments);
    memcpy(out.products.data(), p.products, sizeof p.products);
    memcpy(out.acc_v_commitments.data(), p.acc_v_commitments, sizeof p.acc_v_commitments);
    memcpy(out.claimed_sumchecks.data(), p.claimed_sumchecks, sizeof p.claimed_sumchecks);
    memcpy(out.ralpha_star_acc_mu_evals.data(), p.ralpha_star_acc_mu_evals, sizeof p.ralpha_star_acc_mu_evals);
    memcpy(out.ralpha_star_acc_mu_proof.data(), p.ralpha_star_acc_mu_proof, 144);
    memcpy(out.rstars_vals.data(), p.rstars_vals, sizeof p.rstars_vals);
    TensorcheckProof& tc = out.tensorcheck_proof;
    tc.folded_polynomials_commitments.resize(p.nfold);
    tc.folded_polynomials_evaluations.resize(p.nfold);
    for (size_t i = 0; i < p.nfold; i++) {
      memcpy(tc.folded_polynomials_commitments[i].data(), fc.data() + 18 * i, 144);
      memcpy(tc.folded_polynomials_evaluations[i].data(), fe.data() + 8 * i, 64);
    }
    memcpy(tc.evaluation_proof.data(), p.evaluation_proof, 144);
    tc.base_polynomials_evaluations.resize(22);
    memcpy(tc.base_polynomials_evaluations[0].data(), p.base_evaluations, sizeof p.base_evaluations);
    return out;
  }

  // every G1 element the verifier reads is canonical, on the curve and in G1 (gm_psnark_proof_check); verify() does not call it
  ProofCheck check_points() const {
    const TensorcheckProof& tc = tensorcheck_proof;
    const size_t nf = tc.folded_polynomials_commitments.size();
    gm_psnark_proof p;
    memset(&p, 0, sizeof p);
    std::vector<uint64_t> fc(18 * nf + 1);
    memcpy(p.witness_commitment, witness_commitment.data(), 144);
    memcpy(p.r_star_commitments, r_star_commitments.data(), sizeof p.r_star_commitments);
    memcpy(p.z_star_commitment, z_star_commitment.data(), 144);
    memcpy(p.sorted_commitments, sorted_commitments.data(), sizeof p.sorted_commitments);
    memcpy(p.acc_v_commitments, acc_v_commitments.data(), sizeof p.acc_v_commitments);
    memcpy(p.ralpha_star_acc_mu_proof, ralpha_star_acc_mu_proof.data(), 144);
    for (size_t i = 0; i < nf; i++) memcpy(fc.data() + 18 * i, tc.folded_polynomials_commitments[i].data(), 144);
    p.nfold = p.cap_folds = nf;
    p.fold_commitments = fc.data();
    memcpy(p.evaluation_proof, tc.evaluation_proof.data(), 144);
    ProofCheck r;
    int ok = 0;
    check(gm_psnark_proof_check(&p, &r.first_bad, &ok));
    r.ok = ok != 0;
    return r;
  }

  // Proof::verify(&r1cs, &vk, &index, num_non_zero) (src/psnark/verifier.rs:88-565): true = accepted.  The key needs max_eval_points >= 3
  bool verify(const R1cs& r1cs, const VerifierKey& vk, const std::array<G1Projective, 5>& index, size_t num_non_zero, int g1_encoding = 0) const {
    Packed P;
    if (!P.pack(*this)) return false;
    const SnarkProof::PublicInput x(r1cs);
    int ok = 0;
    check(gm_psnark_verify(x.h, r1cs.nz_, num_non_zero, index[0].data(), vk.handle(), g1_encoding, &P.p, &ok));
    return ok != 0;
  }

  // The proofs under one index and one key in ONE call (gm_psnark_verify_many): a verdict per proof, what verify() answers for each; the two
  // KZG checks of every proof run in one batch.  x_vecs as for SnarkProof::verify_many
  static std::vector<bool> verify_many(const std::vector<const PsnarkProof*>& proofs, const R1cs& r1cs, const VerifierKey& vk, const std::array<G1Projective, 5>& index,
                                       size_t num_non_zero, const std::vector<uint64_t>& x_vecs = {}, int g1_encoding = 0) {
    if (!x_vecs.empty() && x_vecs.size() != proofs.size()) throw Error(GM_EINVAL, "verify_many: one public input per proof");
    std::vector<bool> out(proofs.size(), false);
    std::vector<Packed> packed(proofs.size());
    std::vector<gm_psnark_proof> recs;
    std::vector<uint64_t> xs;
    std::vector<size_t> live;
    const SnarkProof::PublicInput x(r1cs);
    for (size_t i = 0; i < proofs.size(); i++) {
      if (!packed[i].pack(*proofs[i])) continue;
      live.push_back(i);
      recs.push_back(packed[i].p);
      xs.push_back(x_vecs.empty() ? x.h : x_vecs[i]);
    }
    if (live.empty()) return out;
    std::vector<int> ok(live.size(), 0);
    check(gm_psnark_verify_many(xs.data(), r1cs.nz_, num_non_zero, index[0].data(), vk.handle(), g1_encoding, recs.data(), live.size(), ok.data()));
    for (size_t k = 0; k < live.size(); k++) out[live[k]] = ok[k] != 0;
    return out;
  }

  // the gm_psnark_proof record of a proof and the arrays it points into
  struct Packed {
    gm_psnark_proof p;
    std::vector<uint64_t> m[3], fc, fe;
    bool pack(const PsnarkProof& s) {
      const TensorcheckProof& tc = s.tensorcheck_proof;
      const size_t nf = tc.folded_polynomials_commitments.size();
      if (tc.base_polynomials_evaluations.size() != 22 || tc.folded_polynomials_evaluations.size() != nf) return false;
      memset(&p, 0, sizeof p);
        fc.assign(18 * nf + 1, 0);
        fe.assign(8 * nf + 1, 0);
      const std::vector<RoundMsg>* msgs[3] = {&s.first_sumcheck_msgs, &s.second_sumcheck_msgs, &s.third_sumcheck_msgs};
      for (int k = 0; k < 3; k++) {
        m[k].assign(8 * msgs[k]->size() + 1, 0);
        for (size_t i = 0; i < msgs[k]->size(); i++) {
          memcpy(m[k].data() + 8 * i, (*msgs[k])[i].a.data(), 32);
          memcpy(m[k].data() + 8 * i + 4, (*msgs[k])[i].b.data(), 32);
        }
        p.rounds[k] = msgs[k]->size();
        p.messages[k] = m[k].data();
      }
      memcpy(p.witness_commitment, s.witness_commitment.data(), 144);
      memcpy(p.zc_alpha, s.zc_alpha.data(), 32);
      memcpy(p.final_foldings[0], s.first_final_foldings.data(), 64);
      memcpy(p.final_foldings[1], s.second_final_foldings.data(), 64);
      memcpy(p.third_final_foldings, s.third_final_foldings.data(), sizeof p.third_final_foldings);
      memcpy(p.r_star_commitments, s.r_star_commitments.data(), sizeof p.r_star_commitments);
      memcpy(p.z_star_commitment, s.z_star_commitment.data(), 144);
      memcpy(p.sorted_commitments, s.sorted_commitments.data(), sizeof p.sorted_commitments);
      memcpy(p.products, s.products.data(), sizeof p.products);
      memcpy(p.acc_v_commitments, s.acc_v_commitments.data(), sizeof p.acc_v_commitments);
      memcpy(p.claimed_sumchecks, s.claimed_sumchecks.data(), sizeof p.claimed_sumchecks);
      memcpy(p.ralpha_star_acc_mu_evals, s.ralpha_star_acc_mu_evals.data(), sizeof p.ralpha_star_acc_mu_evals);
      memcpy(p.ralpha_star_acc_mu_proof, s.ralpha_star_acc_mu_proof.data(), 144);
      memcpy(p.rstars_vals, s.rstars_vals.data(), sizeof p.rstars_vals);
      for (size_t i = 0; i < nf; i++) {
        memcpy(fc.data() + 18 * i, tc.folded_polynomials_commitments[i].data(), 144);
        memcpy(fe.data() + 8 * i, tc.folded_polynomials_evaluations[i].data(), 64);
      }
      p.nfold = p.cap_folds = nf;
      p.fold_commitments = fc.data();
      p.fold_evaluations = fe.data();
      memcpy(p.evaluation_proof, tc.evaluation_proof.data(), 144);
      memcpy(p.base_evaluations, tc.base_polynomials_evaluations[0].data(), sizeof p.base_evaluations);
      return true;
    }
  };
};

}  // namespace gm
