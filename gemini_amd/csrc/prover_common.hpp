// Helpers shared by the provers compiled into the library, single-device and sharded: pure orchestration over the library's own C ABI.
// The committer keys and the tensor check of the single-device provers are in tensorcheck.hpp.
#pragma once
#include <chrono>
#include <cstring>
#include <vector>

#include "sumcheck_driver.hpp"

namespace gmprover {

using Clock = std::chrono::steady_clock;

inline double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// device vectors owned by one proof: freed on every exit path
struct Vecs {
  std::vector<uint64_t> h;
  ~Vecs() {
    for (uint64_t v : h) (void)gm_fr_vec_free(v);
  }
  int alloc(size_t n, uint64_t* out) {
    int rc = gm_fr_vec_alloc(n, out);
    if (!rc) h.push_back(*out);
    return rc;
  }
  // free one vector before the end of the proof (temporaries of a phase: the preprocessing prover at 2^26 constraints
  // holds ~100 GB of live vectors as it is)
  void release(uint64_t v) {
    for (size_t i = 0; i < h.size(); i++)
      if (h[i] == v) {
        (void)gm_fr_vec_free(v);
        h[i] = h.back();
        h.pop_back();
        return;
      }
  }
};
struct TranscriptGuard {
  uint64_t h = 0;
  ~TranscriptGuard() {
    if (h) (void)gm_transcript_free(h);
  }
};

inline int vec_len(uint64_t v, size_t* n) { return gm_fr_vec_len(v, n); }

// Sumcheck::new_time (proof.rs:125-130): the prover reads f and g in place (the round loop runs inside this call and the
// callers do not touch the vectors meanwhile), its folds go to buffers of its own
inline int sumcheck_new_time(uint64_t transcript, uint64_t f, uint64_t g, const uint64_t twist[4], uint64_t* messages, std::vector<uint64_t>& challenges,
                             size_t cap_rounds, uint64_t final_foldings[8], size_t* rounds) {
  ElasticSc S;
  RC(S.init_resident(f, g, twist));
  return prove(transcript, S, messages, challenges, cap_rounds, final_foldings, rounds);
}
// Sumcheck::new_elastic (proof.rs:145-154): a SpaceProver over the streams that becomes a TimeProver when fewer than
// SPACE_TIME_THRESHOLD rounds remain
inline int sumcheck_new_elastic(uint64_t transcript, uint64_t f_stream, uint64_t g_stream, const uint64_t twist[4], uint64_t* messages,
                                std::vector<uint64_t>& challenges, size_t cap_rounds, uint64_t final_foldings[8], size_t* rounds) {
  ElasticSc S;
  RC(S.init(f_stream, g_stream, twist, true));
  return prove(transcript, S, messages, challenges, cap_rounds, final_foldings, rounds);
}

// sum over stream positions k < len: stream[k] * power[top - k], flushed every max(chunk, min_chunk) pairs
// (msm_chunks / ChunkedPippenger composition, src/kzg/space.rs:22-55)
inline int stream_msm(uint64_t bases, uint64_t stream, size_t len, size_t top, size_t chunk, uint64_t out[18]) {
  if (len == 0) return gm_g1_sum(nullptr, 0, out);
  if (chunk == 0) chunk = 1;
  if (len <= chunk) return gm_ck_msm(bases, top, 1, stream, 0, len, out);
  std::vector<uint64_t> parts;
  for (size_t off = 0; off < len; off += chunk) {
    const size_t m = len - off < chunk ? len - off : chunk;
    parts.resize(parts.size() + 18);
    RC(gm_ck_msm(bases, top - off, 1, stream, off, m, parts.data() + parts.size() - 18));
  }
  return gm_g1_sum(parts.data(), parts.size() / 18, out);
}

inline Fr fr_pow(Fr base, size_t e) {
  Fr acc = Fr::one();
  while (e) {
    if (e & 1) acc = acc * base;
    base = base.sqr();
    e >>= 1;
  }
  return acc;
}

// plookup (plookup/time_prover.rs:89-112) -> lookup_set, lookup_subset, lookup_sorted
inline int plookup(Vecs& V, uint64_t subset, uint64_t set_, uint64_t index, size_t index_len, uint64_t ext_fre, size_t ext_len, const uint64_t y[4],
            const uint64_t z[4], const uint64_t zeta[4], uint64_t out[3]) {
  size_t nset = 0, nsub = 0;
  RC(vec_len(set_, &nset));
  RC(vec_len(subset, &nsub));
  uint64_t set_h = set_, subset_h = subset;
  if (!Fr::from_limbs(zeta).is_zero()) {
    RC(V.alloc(nset, &set_h));
    RC(gm_fr_alg_hash(set_, 0, zeta, set_h));
    const size_t n = nsub < index_len ? nsub : index_len;
    RC(V.alloc(n, &subset_h));
    RC(gm_fr_alg_hash(subset, index, zeta, subset_h));
    nsub = n;
  }
  RC(V.alloc(nset ? nset + 1 : 0, &out[0]));
  RC(gm_fr_plookup_set(set_h, y, z, out[0]));
  RC(V.alloc(nsub, &out[1]));
  RC(gm_fr_add_scalar(subset_h, y, out[1]));
  uint64_t srt;
  RC(V.alloc(ext_len, &srt));
  RC(gm_fr_gather(set_h, ext_fre, srt));
  RC(V.alloc(ext_len ? ext_len + 1 : 0, &out[2]));
  RC(gm_fr_plookup_set(srt, y, z, out[2]));
  V.release(srt);
  if (set_h != set_) V.release(set_h);
  if (subset_h != subset) V.release(subset_h);
  return GM_OK;
}

}  // namespace gmprover
