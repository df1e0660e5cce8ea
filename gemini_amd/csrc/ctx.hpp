// Process-wide state of libgemini_hip.so: one GPU per process, opaque u64 handles for
// device-resident bases / Fr vectors / sumcheck provers, grow-only workspaces, error strings.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/gemini_hip.h"

namespace gmh {
struct Fq12;  // host_field.hpp
}

namespace gm {

void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what, const char* file, int line);

#define GM_HIP(expr)                                                     \
  do {                                                                   \
    hipError_t _e = (expr);                                              \
    if (_e != hipSuccess) return ::gm::hip_fail(_e, #expr, __FILE__, __LINE__); \
  } while (0)

#define GM_CHECK(cond, code, ...)  \
  do {                             \
    if (!(cond)) {                 \
      ::gm::set_error(__VA_ARGS__); \
      return (code);               \
    }                              \
  } while (0)

// grow-only device buffer
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes);
  void release();
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

struct Bases {
  uint8_t* d = nullptr;  // n x 96 bytes: x, y Montgomery; identity = all zero
  // phi(P_i) = (beta x_i, y_i) = lambda P_i, the image under the curve's endomorphism, same layout; built at
  // registration (bases_build_phi) for the GLV split of the MSM, nullptr for one-shot / borrowed bases
  uint8_t* phi = nullptr;
  size_t n = 0;
  // optional fixed-base window tables: table[w * n + i] = 2^(tab_c * w) * base[i], w < tab_W
  // (table row 0 is a copy of d so one pointer serves every window)
  uint8_t* table = nullptr;
  int tab_c = 0, tab_W = 0;
  size_t tab_min = 0;  // smallest call the tables pay off for (depends on their window width)
  // PREFIX tables for the calls the main tables do not serve: a wide-window table (c = 22: 2^21 buckets to reduce) loses below
  // 2^22 pairs, but the short calls of a prover -- the low levels of a folding tree -- walk the FIRST powers of the key, so a second
  // table over that prefix with a narrower window costs a few GB (13 x 2^22 x 96 B).  A call [first, first + step * n) inside
  // the prefix with min_n <= n < max_n takes the set.
  struct TableSet {
    uint8_t* t = nullptr;
    int c = 0, W = 0;
    size_t n = 0, min_n = 0, max_n = 0;
  };
  std::vector<TableSet> extra;
  bool extras_released = false;  // the prefix sets were given back under memory pressure (release_spare_tables); gm_g1_bases_precompute(handle, -1) rebuilds them
  // a CYCLIC SHARE of a committer key (gm_g1_bases_set_cyclic): these n points are the powers i = cyc_rank (mod cyc_world)
  // of a key of cyclic_n powers; gm_ck_* and the provers commit through the all-gather of dist.cpp.  0 = a whole key
  size_t cyclic_n = 0;
  int cyc_rank = 0, cyc_world = 1;
};

struct FrVec {
  uint8_t* d = nullptr;  // cap x 32 bytes, Montgomery
  size_t cap = 0;
  size_t len = 0;
  size_t cap_bytes = 0;  // size of the pooled allocation behind d
};

// CSR sparse matrix resident in HBM (`Matrix<F> = Vec<Vec<(F, usize)>>`, src/circuit.rs:43)
struct SparseMatrix {
  uint64_t* rowptr = nullptr;  // nrows + 1
  uint32_t* cols = nullptr;    // nnz
  uint8_t* vals = nullptr;     // nnz x 32 bytes Montgomery
  size_t nrows = 0, ncols = 0, nnz = 0;
};

// index vector resident in HBM (`&[usize]` arguments of plookup / lookup: row_index, col_index, ...)
struct IdxVec {
  uint32_t* d = nullptr;
  size_t n = 0;
  size_t max_plus_1 = 0;  // 1 + the largest index (0 for an empty vector)
  size_t pool_cap = 0;    // != 0: d is a block of the vector pool (gm_idx_extend_frequency builds its result on the device)
};

struct Sumcheck {
  // ping-pong state of TimeProver (src/subprotocols/sumcheck/time_prover.rs:42-52)
  uint8_t* f[2] = {nullptr, nullptr};
  uint8_t* g[2] = {nullptr, nullptr};
  size_t fcap[2] = {0, 0}, gcap[2] = {0, 0};  // pooled allocation sizes
  // gm_sc_new_borrow: f[0] / g[0] are the CALLER's vectors, read until the first fold has written the halves into f[1] / g[1]; the
  // slot gets a quarter-size buffer of the prover's own when the second fold needs somewhere to write
  bool borrowed = false;
  int cur = 0;
  size_t nf = 0, ng = 0;
  uint64_t twist[4];  // Montgomery
  size_t round = 0, tot_rounds = 0;
  uint64_t pair_offset = 0;  // shard origin (gm_sc_set_shard)
  bool herring = false;      // herring FModule prover: messages carry no twist (src/herring/time_prover.rs:91-123)
  uint8_t* partials = nullptr;   // per-block (a, b) partial sums
  uint64_t* host_partials = nullptr;  // pinned
  unsigned pending_blocks = 0;        // blocks of the round whose partial sums are on their way to host_partials
  // the TAIL on the host: once the vectors are down to SC_HOST_TAIL elements they are copied out once and the remaining rounds --
  // a launch, a copy and a wait each on the device, ~45 us for microseconds of arithmetic -- run on the host (fr.hip: sc_host_step)
  bool on_host = false;
  std::vector<uint64_t> hf, hg;  // 4 limbs per element, Montgomery
  uint64_t host_msg[8];          // the message of the round in flight (split-phase rounds)
  bool host_msg_pending = false;
  std::mutex mu;
};
constexpr size_t SC_HOST_TAIL = 256;
// the descriptor ring of k_sc_round_multi (Context::sc_desc_*): a launch takes as many provers as one slot holds descriptors
constexpr size_t SC_DESC_SLOT = (size_t)32 << 10;
constexpr unsigned SC_DESC_SLOTS = 8;

struct SpaceProver {
  // src/subprotocols/sumcheck/space_prover.rs:20-40: the witness streams (big-endian, never modified),
  // the challenges and the twisted challenges
  uint8_t* f = nullptr;
  uint8_t* g = nullptr;
  size_t nf = 0, ng = 0, fcap = 0, gcap = 0;
  bool borrowed = false;  // gm_sp_new_borrow: f / g are the caller's stream vectors (a space prover never writes them)
  std::vector<uint64_t> challenges, twisted;  // 4 limbs each, Montgomery
  uint64_t twist[4];
  size_t round = 0, tot_rounds = 0;
  uint8_t* tables = nullptr;  // weight tables + reduced ping / pong vectors of the current message: a block of the vector pool
  size_t tables_cap = 0;       // (hipMalloc / hipFree per prover cost a device-wide synchronisation each)
  uint8_t *wf_lo = nullptr, *wf_hi = nullptr, *wg_lo = nullptr, *wg_hi = nullptr;
  uint8_t* partials = nullptr;
  uint64_t* host_partials = nullptr;
  std::mutex mu;
};

// herring TimeProver over a bilinear module (src/herring/time_prover.rs:42-137; herring.hip): f is the Lhs vector, g the Rhs vector,
// each an Fr vector (32 B, a block of the vector pool), affine G1 points (96 B), affine G2 points (192 B) or GT elements (576 B)
enum HerringModule { HERRING_G1 = 0, HERRING_G2, HERRING_P, HERRING_GT };  // G1 x F -> G1, F x G2 -> G2, G1 x G2 -> GT, GT x F -> GT (module.rs:49-125)
struct HerringProver {
  HerringModule module = HERRING_G1;
  uint8_t* f[2] = {nullptr, nullptr};
  uint8_t* g[2] = {nullptr, nullptr};
  size_t fcap[2] = {0, 0}, gcap[2] = {0, 0};  // pooled allocation sizes (Fr sides)
  int cur = 0;
  size_t nf = 0, ng = 0;
  uint64_t twist[4];  // Montgomery
  size_t round = 0, tot_rounds = 0;
  uint8_t* tmp = nullptr;  // compacted scalars of the module's messages
  size_t tmpcap = 0;
  bool finished = false;  // PModule: the call that folded the last challenge has answered "no message", every later one is GM_ESTATE
  std::mutex mu;
};

// herring's inner-product argument (src/herring/ipa.rs; ipa.hip).  Crs: the two point vectors resident on the device, packed as
// Bases / G2Bases hold them.  Vrs and a proof are host values: GT elements are 72 limbs (gemini_hip.h), points normalised Jacobian
struct Crs {
  uint8_t* g1 = nullptr;  // n1 x 96 bytes
  uint8_t* g2 = nullptr;  // n2 x 192 bytes
  size_t n1 = 0, n2 = 0;
};
struct Vrs {
  std::vector<uint64_t> vk1, vk2;  // levels x (even || odd), 144 limbs per level
  size_t levels = 0;
};
struct IpaProof {
  size_t rounds = 0;
  std::vector<uint64_t> messages;          // rounds x (a || b), 144 limbs each
  std::vector<uint64_t> challenges;        // rounds x 4, Montgomery
  size_t K = 1;                            // claims: 1 for every proof but one of gm_ipa_new_batch / gm_ipa_from_fields_batch
  std::vector<uint64_t> batch_challenges;  // (3 K + 2 (rounds - 1)) x 4
  std::vector<uint64_t> final_g1, final_g2;  // 2 (rounds - 1) x 18 / x 36: Sumcheck::final_foldings
  std::vector<uint64_t> foldings_ff, foldings_fg1, foldings_fg2;  // K x 8 / K x 22 / K x 40: (lhs || rhs) of the three initial provers of every claim
  double host_ms[3] = {0, 0, 0};  // of gm_ipa_new: host GT multi-exponentiations, host final exponentiations, the whole call (gm_ipa_host_times)
};

// kzg::VerifierKey (src/kzg/mod.rs:141-149; verifier.cpp): host records, Montgomery, identity = all zero
struct VerifierKey {
  std::vector<uint64_t> g1;  // n1 x 12 limbs: the first max_eval_points powers of g
  std::vector<uint64_t> g2;  // n2 x 24 limbs: max_eval_points + 1 powers of g2
  size_t n1 = 0, n2 = 0;
  uint8_t* d_g2 = nullptr;  // the same n2 powers of g2 resident on the device (192-byte records): the batched checks pair against them
};

// G2 bases (g2msm.hip): n x 192 bytes, x.c0 | x.c1 | y.c0 | y.c1 in the device form of g1.cuh; identity = all zero
struct G2Bases {
  uint8_t* d = nullptr;
  size_t n = 0;
};
// herring SpaceProver over G1Module / G2Module (src/herring/space_prover.rs:39-276; herring.hip): the point side is `np` points of a
// key, read where they lie as the big-endian stream key[offset + i] and never written or copied; the scalar side is kept folded,
// little-endian, in two ping-pong blocks of the vector pool.  A message is one launch of k_hsp_scalars and two MSMs over the key
struct HerringSpace {
  HerringModule module = HERRING_G1;  // HERRING_G1 (points are the Lhs) or HERRING_G2 (points are the Rhs)
  const Bases* g1 = nullptr;          // the key: the caller's registered handle, or own_g1 / own_g2 (gm_hsp1_new / gm_hsp2_new)
  const G2Bases* g2 = nullptr;
  std::unique_ptr<Bases> own_g1;
  std::unique_ptr<G2Bases> own_g2;
  size_t offset = 0, np = 0;  // the points key[offset .. offset + np)
  size_t ns = 0;              // length of the scalar stream
  uint8_t* s[2] = {nullptr, nullptr};  // the folded scalar vector S (little-endian, Montgomery) and the block the next fold writes
  size_t scap[2] = {0, 0};
  int cur = 0;
  size_t ls = 0;              // current length of S: ceil(ns / 2^k)
  uint8_t* work = nullptr;    // the expanded scalars of a message (2 x np x 32 B, canonical), the half tensor tables, the challenges
  size_t work_cap = 0;
  std::vector<uint64_t> pt_ch;        // the challenges that fold the point side, 4 limbs each, Montgomery (twisted for G1Module)
  std::vector<uint64_t> pt_ch_canon;  // the same as canonical integers, for split_fold (gm_hsp*_to_time)
  uint64_t twist[4];
  size_t round = 0, tot_rounds = 0;
  size_t path[4] = {0, 0, 0, 0};  // gm_debug_hsp_path: MSM calls, expansion launches, point bytes allocated, scalar bytes allocated
  std::mutex mu;
};
// what one launch of k_hsp_scalars is told (fr.hip: hsp_scalars_raw).  Lane t serves the point key[offset + t], whose little-endian
// index is i = np - 1 - t, block m = i >> k, place u = i & (2^k - 1) inside it
struct HspArgs {
  const uint8_t* S = nullptr;  // folded scalars, little-endian, Montgomery; entries at and past `ls` count as zero
  size_t ls = 0;
  const uint8_t *lo = nullptr, *hi = nullptr;  // tensor(point-side challenges) = lo[u & (2^klo - 1)] hi[u >> klo]
  uint32_t k = 0, klo = 0;
  size_t np = 0;      // points of the stream
  size_t lanes = 0;   // lanes of the launch: the first `lanes` points of the stream
  size_t npairs = 0;  // blocks 2j and 2j + 1 with j >= npairs carry zero scalars
  uint64_t twist[4];  // Montgomery
  int rhs_points = 0;  // G2Module: the points are the Rhs, so the twist factor of b sits on the even block
  int final_only = 0;  // out_a[t] = the weight of point t alone (final_foldings: the caller launches the lanes of the top block only)
  uint8_t *out_a = nullptr, *out_b = nullptr;  // np x 32 B each, canonical
};

// What a G2 MSM holds beyond the sort buffers it shares with G1 (MsmWorkspace counts / offsets / cursor / entries / ...):
// buckets and chunk partials in 384-byte XYZZ records, the two ping-pong levels of the bucket reduction, the pinned window sums
struct G2Workspace {
  DevBuf buckets, part, red[2], longs;
  uint64_t* host_out = nullptr;  // pinned: W window sums (48 u64 each) + the scalar-range flag
  size_t host_out_cap = 0;
};

// What a multi-pairing holds (pairing.hip): the two ping-pong levels of Miller partial products (576-byte Fq12 records) and the
// pinned copy of the last few.  Single-flight under msm_mu
struct PairingWorkspace {
  DevBuf part[2];
  uint64_t* host_out = nullptr;
  // the segmented form (miller_products): the span and segment tables of a call, and the pinned copy of its S results
  DevBuf seg_tab;
  uint64_t* host_seg = nullptr;
  size_t host_seg_cap = 0;  // in GT elements
  // GtModule (k_gt_multi_pow, k_gt_split_fold): the window table x, x^2, x^3 of every lane of a launch, [block][entry][limb][lane]
  DevBuf gt_tab;
};
// ChunkedPippenger / msm_chunks over HOST-resident pairs (src/kzg/msm/stream_pippenger.rs:209-272, src/kzg/space.rs:22-55):
// the device holds two chunks; chunk i + 1 is copied in while the MSM of chunk i runs (msm.hip: msm_stream_*)
struct MsmWorkspace;
// k_sort2_group (msm.hip): 4-byte entries one block stages in its 160 KiB of LDS beside three arrays of 1024 counters and the
// wave sums of its scan; at least one entry per thread
constexpr size_t MSM_SORT_GROUP_CAP_MAX = (160 * 1024 - 3 * 1024 * 4 - 64) / 4;
constexpr size_t MSM_SORT_GROUP_CAP_MIN = 1024;
// One MSM between its enqueue (all kernels + the async copy of the window bit-planes) and its finish (host Horner)
struct MsmPending {
  MsmWorkspace* ws = nullptr;  // the workspace (and stream) the call was enqueued on
  int slot = 0;
  bool empty = true;
  int Wb = 0, c = 0, m = 0;
  uint32_t nbits = 0, wf[3] = {0, 0, 0};
  size_t plane_off[3] = {0, 0, 0};
  size_t plane_count = 0;
  int multi_levels = 0;  // > 0: several small MSMs in ONE pass (msm.hip: MsmMulti); bucket sets [l W, (l + 1) W) belong to call l
  int multi_W = 0;
  bool sort_compact = false;  // the block sort took the 4-byte pass-1 entries + k_sort2_group (gm_debug_msm_sort_path)
  int opt = 0;                // parts of the optimistic one-call path this enqueue took (MSM_OPT_*), checked by the flags of its trailer
  uint32_t L = 0;             // chunk length of k_acc0
};
// the optimistic one-call path (gm_set_msm_optimistic): pass 1 of the block sort into fixed-capacity bins, one boundary pass in
// place of the merge levels; the same values name the flag a failed attempt raised
enum { MSM_OPT_BINS = 1, MSM_OPT_BOUNDARY = 2 };
struct MsmStreamSlot {
  uint8_t *raw = nullptr, *packed = nullptr, *scalars = nullptr;  // staged records, device-form bases, scalars
  size_t raw_cap = 0, packed_cap = 0, scalars_cap = 0;
  hipEvent_t copied;
  bool have_ev = false;
  bool inflight = false;
  MsmPending P;
};
struct MsmStream {
  std::mutex mu;
  size_t chunk = 0, stride = 96;
  int mont = 0;
  uint64_t bases_handle = 0;  // 0: the pairs carry their bases; else scalars only, against registered bases
  int64_t base0 = 0, next_base = 0, step = 1;
  MsmStreamSlot s[2];
  int cur = 0;
  size_t fill = 0, total = 0;
  hipStream_t copy = nullptr;
  uint64_t acc[18];  // running sum (Jacobian, host)
  bool acc_set = false;
};

constexpr int MSM_SLOTS = 4;
constexpr int MSM_SMALL_LANES = 6;  // small calls of a batch in flight side by side (GM_MSM_SMALL_LANES uses fewer); a lane's workspace is ~150 MB.
// Measured on one box, snark -i 18 / -i 20 / sharded -i 21 / -i 22 (ms): 2 lanes 14.6 / 21.5 / 36.0 / 50.7, 4 lanes 13.1 / 19.8 / 33.5 / 48.1,
// 6 lanes 11.7 / 18.7 / 32.0 / 47.4, 8 lanes 17.0 / 21.1 / 33.6 / 48.5, 12 lanes 17.6 / 22.5 / 35.0 / 51.3: beyond six the chains only get in each other's way
struct MsmWorkspace {
  DevBuf scalars, counts, offsets, cursor, entries, tmp_entries, sortmeta, buckets, pk[2], pp[2], rows, cols, planes, misc;
  DevBuf clk;  // {shader cycles, 100 MHz ticks} of the first wave of the last k_acc0 (read only while profiling: gm_prof_read_clock)
  DevBuf lvl_cnt, lvl_pos, lvl_pts[2], lvl_keys[2], lvl_prefix, lvl_lane, lvl_entries, lvl_n;  // affine tree levels
  // pinned staging for the D2H of window bit-planes + the event behind it, per result slot: MSM_SLOTS calls of a lane can be enqueued
  // behind one another before the host finishes the first (big lanes use two, small lanes all of them)
  uint64_t* host_planes[MSM_SLOTS] = {};
  size_t host_planes_cap[MSM_SLOTS] = {};
  hipEvent_t done_ev[MSM_SLOTS];
  hipEvent_t sort_ev, acc_ev;  // phase hand-over between the streams of a split call
  bool have_done_ev = false;
};

// per-stage kernel timing with HIP events on the library's own stream (bench.py's roofline leg)
enum ProfStage { PROF_DIGITS = 0, PROF_SCAN, PROF_SCATTER, PROF_ACC0, PROF_MERGE, PROF_REDUCE, PROF_SC_ROUND, PROF_EXTFREQ, PROF_NSTAGES };
struct Profiler {
  bool on = false;
  int only_stage = -1;  // >= 0: events around that stage only (gm_prof_enable(2): the accumulation; every event record is a ~10 us bubble)
  hipEvent_t ev[2][2 * PROF_NSTAGES];  // [window group of a split MSM call][stage begin / end]
  bool have_events = false;
  bool pending[2][PROF_NSTAGES] = {};
  double ms[PROF_NSTAGES] = {};     // summed over calls AND over the window groups of a call
  uint64_t count[PROF_NSTAGES] = {};  // launches of the stage (a split call counts two)
  double acc0_cycles = 0, acc0_ticks = 0;  // clock64() / wall_clock64() spans of k_acc0's first wave, summed over calls
  void begin(int part, int stage, hipStream_t st);
  void end(int part, int stage, hipStream_t st);
  void begin(int stage, hipStream_t st) { begin(0, stage, st); }
  void end(int stage, hipStream_t st) { end(0, stage, st); }
  void collect();  // after the streams of the call have been waited for
};

// Caching allocator for device vectors: the prover allocates and drops O(100) multi-hundred-MB
// vectors per proof; hipMalloc/hipFree are synchronous and cost milliseconds at that size.
struct DevPool {
  std::mutex mu;
  std::multimap<size_t, void*> free_list;  // capacity -> pointer
  size_t pooled_bytes = 0;
  size_t max_pooled = (size_t)96 << 30;  // GM_POOL_MAX_GB overrides (gm_init)
  int alloc(size_t bytes, void** p, size_t* cap);
  void free(void* p, size_t cap);
  void release_all();
};

// the (device, pinned host) buffer pair a sumcheck / space prover collects its per-block partial sums in: 32 KiB each.  hipMalloc,
// hipHostMalloc and above all hipFree (a device-wide synchronisation) cost 0.1-0.3 ms apiece -- the preprocessing prover creates 15
// provers per proof -- so freed pairs are kept for the next prover
struct PartialBufs {
  std::mutex mu;
  std::vector<std::pair<uint8_t*, uint64_t*>> free_pairs;
  int take(uint8_t** dev, uint64_t** host);
  void give(uint8_t* dev, uint64_t* host);
  void release_all();
};
constexpr size_t PARTIAL_BUF_BYTES = 512 * 2 * 32;

struct Context {
  int device = -1;
  PartialBufs partial_bufs;
  DevPool pool;
  Profiler prof;
  hipStream_t stream = nullptr;
  std::mutex mu;       // guards handle tables
  // The MSM workspaces are single-flight (the reference's MSM calls are sequential): msm_mu is held from the
  // staging of host scalars to the end of the call (recursive: msm_host_scalars -> msm_run).
  std::recursive_mutex msm_mu;
  // Vector entry points (gm_fr_*) stage per-call parameters and partial results in fr_scratch / host_small and
  // share one stream: fr_mu serialises them, so calls from different threads are safe (and ordered).
  std::recursive_mutex fr_mu;
  uint64_t next_handle = 1;
  std::unordered_map<uint64_t, std::unique_ptr<Bases>> bases;
  std::unordered_map<uint64_t, std::unique_ptr<FrVec>> vecs;
  std::unordered_map<uint64_t, std::unique_ptr<Sumcheck>> provers;
  std::unordered_map<uint64_t, std::unique_ptr<SparseMatrix>> matrices;
  std::unordered_map<uint64_t, std::unique_ptr<SpaceProver>> space_provers;
  std::unordered_map<uint64_t, std::unique_ptr<HerringProver>> herring;
  std::unordered_map<uint64_t, std::unique_ptr<HerringSpace>> herring_space;
  std::unordered_map<uint64_t, std::unique_ptr<Crs>> crs;
  std::unordered_map<uint64_t, std::unique_ptr<Vrs>> vrs;
  std::unordered_map<uint64_t, std::unique_ptr<IpaProof>> ipa;
  std::unordered_map<uint64_t, std::unique_ptr<G2Bases>> g2_bases;
  std::unordered_map<uint64_t, std::unique_ptr<VerifierKey>> vks;
  std::unordered_map<uint64_t, std::unique_ptr<MsmStream>> msm_streams;
  std::unordered_map<uint64_t, std::unique_ptr<IdxVec>> indices;
  MsmWorkspace msm;
  G2Workspace g2;  // single-flight under msm_mu, like msm
  PairingWorkspace pairing;  // likewise
  // extra workspaces + streams for the small calls of a batch (msm_run_batch)
  MsmWorkspace msm_small[MSM_SMALL_LANES];
  hipStream_t small_stream[MSM_SMALL_LANES] = {};
  // second full-size workspace + stream: the big calls of a batch alternate between the two so that the
  // sort / merge / reduce of one overlap the (ALU-bound) accumulation of the other
  MsmWorkspace msm_b;
  hipStream_t stream_b = nullptr;
  // XCD PARTITION of a batch (GM_CU_SPLIT, default one XCD; capi.hip: gm_init): the latency-bound tail of every call of a batch
  // (k_merge, the bucket reduction, the copy-out) runs on streams created with a CU mask that covers ONE whole XCD, the
  // accumulations (and sorts) on streams masked to the other seven.  Without it a small kernel does not progress beside an
  // accumulation: the SIMD arbiter serves the oldest waves first and a k_acc0 grid keeps every SIMD supplied with older ones
  // (HISTORY section 4.1), so the tails of a batch end up serialised behind the accumulations they were meant to hide under.
  // Index 0 / 1 / 2.. = main, second big, small lanes
  int cu_split = 0;
  hipStream_t part_acc[2 + MSM_SMALL_LANES] = {};
  hipStream_t part_tail[2 + MSM_SMALL_LANES] = {};
  hipEvent_t start_ev;  // recorded on `stream` when an MSM call starts: its other streams wait for the producer of the scalars
  bool have_start_ev = false;
  DevBuf lincomb;  // gm_g1_lincomb_many and the batched KZG checks: staged terms, their multiples and the sums of a call (under msm_mu)
  size_t verify_many_min = 3;  // fewer stated KZG checks than this take the per-check path (gm_set_verify_many_min); 2 is a tie: profiles/verify_many.md
  // gm_ipa_verify_many: fewer proofs than this take ipa_verify one by one (gm_set_ipa_verify_many_min); what the last call did
  // (gm_debug_ipa_verify_many_path): proofs on the batched path, proofs on the per-proof path
  size_t ipa_verify_many_min = 2;  // S = 1 is a tie (69.6 against 71.2 ms), S = 2 wins 66 against 140 ms: profiles/ipa_verify_many.md
  size_t ipa_verify_many_last[2] = {0, 0};
  // gm_ipa_new_many: fewer proofs than this take ipa_prove one by one (gm_set_ipa_new_many_min); what the last call did
  // (gm_debug_ipa_new_many_path): proofs on the lockstep path, proofs on the per-proof path, kernel launches and stream waits of
  // the lockstep path
  size_t ipa_new_many_min = 2;  // S = 1 loses (1004 against 670 ms), S = 2 wins 1014 (max 1017) against 1337 (min 1334) ms at d = 2^10: profiles/ipa_new_many.md
  size_t ipa_new_many_last[4] = {0, 0, 0, 0};
  // gm_ipa_new_batch: what the last call issued (gm_debug_ipa_new_batch_path): split-fold launches, MSM calls, Miller launches
  size_t ipa_new_batch_last[3] = {0, 0, 0};
  DevBuf fr_scratch;
  uint64_t* host_small = nullptr;  // pinned, 64 KiB, for small results
  // the descriptor arrays of k_sc_round_multi: a RING of SC_DESC_SLOTS slots of SC_DESC_SLOT bytes, one per launch, pinned on the host
  // and mirrored in a device buffer of their own.  The copy to the device is asynchronous and the round is split-phase, so the source must
  // outlive the call (a local vector would not) and must not be rewritten by the next launch of the same round (a sharded batch makes up to
  // four per round).  A slot that comes round again is rewritten only once the event recorded behind its last copy has completed: rounds
  // enqueued by several threads, or one batch split over more launches than there are slots, never read another launch's descriptors
  uint8_t* sc_desc_host = nullptr;
  uint8_t* sc_desc_dev = nullptr;
  hipEvent_t sc_desc_copied[SC_DESC_SLOTS] = {};
  unsigned sc_desc_next = 0;
  uint64_t* host_batch = nullptr;  // pinned, grow-only: partial sums of a batch of evaluations (fr_eval_le_batch)
  size_t host_batch_cap = 0;
  int msm_c_override = 0;
  int msm_glv = 0;            // build phi(P) at registration and split scalars by the GLV endomorphism (gm_set_msm_glv)
  int msm_split = 0;          // one-call MSMs as two window groups over three streams (gm_set_msm_split)
  int msm_affine_levels = 0;  // affine tree levels in front of the XYZZ accumulation; -1 = automatic
  // block sort of a plain call (gm_set_msm_sort_group): 1 = 4-byte pass-1 entries and one block per coarse group where that
  // applies, 0 = the 8-byte passes; cap = entries a block of k_sort2_group loads at once (0 = all that fits beside its counters)
  int msm_sort_group = 1;
  size_t msm_sort_group_cap = 0;
  int msm_sort_path_last = 0;  // what the last finished call took: 0 old, 1 compact, 2 compact with a chunked group
  // the optimistic path of an unsplit one-call MSM (msm.hip: msm_run_one; gm_set_msm_optimistic): MSM_OPT_* bits that are switched on,
  // the back-off after failed attempts (the next `msm_opt_skip` one-calls go straight to the general path; 2^msm_opt_k after the next
  // failure), and the read-out of the last finished one-call (gm_debug_msm_optimistic)
  int msm_opt = MSM_OPT_BINS | MSM_OPT_BOUNDARY;
  int msm_opt_k = 0;
  uint32_t msm_opt_skip = 0;
  int msm_opt_last[5] = {0, 0, 0, 0, 0};
  size_t msm_table_min = (size_t)1 << 17;  // smallest MSM that uses fixed-base tables when present
  // small results (per-block partial sums, the bit-plane sums of an MSM) are written by their kernels straight into pinned host
  // memory instead of a device buffer that a blit kernel then copies (GM_ZERO_COPY=0 restores the copies; bit 0 field paths, bit 1 MSM planes.  Two A/B runs on one box: snark -i 20 14.9 -> 14.5 ms, -i 24 117.8 -> 117.0, psnark -i 20 129 -> 127, same proof bytes: profiles/r4_zero_copy_probe.txt)
  int zero_copy = 3;
  std::atomic<int> msm_busy{0};  // open GM_MSM_LOCK scopes
  bool auto_tables = true;    // build fixed-base tables when bases are registered, if they fit (gm_set_auto_tables)
  size_t auto_tables_max = 0;  // byte budget of one key's tables; 0 = 30 % of the device memory
  int cu_count = 256;
};

Context* context();  // nullptr before gm_init
// Every device allocation of the library goes through these two (hipMalloc / hipFree + bookkeeping): what the process holds from the
// driver, its high-water mark, and -- minus the vector pool's cached blocks -- what is IN USE and its peak (gm_mem_stats; the
// footprint contract of the provers is checked against these figures, tests/test_gpu_footprint.py)
struct MemStats {
  std::mutex mu;
  std::unordered_map<void*, size_t> sizes;
  size_t live = 0, peak_live = 0;  // bytes obtained from the driver and not given back
  size_t cached = 0;               // of those: freed blocks the vector pool keeps for reuse
  size_t peak_in_use = 0;          // high-water mark of live - cached
  uint64_t spare_table_releases = 0;  // release_spare_tables() calls that freed something (no silent degradation)
  void note_cached(ptrdiff_t delta);  // the pool took (+) or handed out (-) a cached block
};
MemStats& mem_stats();
hipError_t raw_malloc_v(void** p, size_t bytes);
template <class T>
inline hipError_t raw_malloc(T** p, size_t bytes) {
  return raw_malloc_v(reinterpret_cast<void**>(p), bytes);
}
hipError_t raw_free(void* p);
hipError_t dev_malloc(void** p, size_t bytes);  // raw_malloc that gives the vector pool's freed blocks back on OOM
struct DevTmp {  // device memory of one call, freed on every path out
  void* p = nullptr;
  ~DevTmp() {
    if (p) (void)raw_free(p);
  }
  uint8_t* u8() const { return static_cast<uint8_t*>(p); }
};
// last resort of an allocation that failed twice: the PREFIX tables of every key (Bases::extra) go, the calls they served take the
// plain path from then on.  False when nothing was freed or an MSM may be reading them (any open GM_MSM_LOCK scope).
bool release_spare_tables(Context* C);

Bases* find_bases(uint64_t h);
FrVec* find_vec(uint64_t h);
Sumcheck* find_prover(uint64_t h);
uint64_t put_bases(std::unique_ptr<Bases> b);
uint64_t put_vec(std::unique_ptr<FrVec> v);
uint64_t put_prover(std::unique_ptr<Sumcheck> p);

// a handle table of the context: look up, take out, put in (under C->mu)
template <class T>
inline T* find_in(Context* C, std::unordered_map<uint64_t, std::unique_ptr<T>>& table, uint64_t h) {
  std::lock_guard<std::mutex> lk(C->mu);
  auto it = table.find(h);
  return it == table.end() ? nullptr : it->second.get();
}
template <class T>
inline std::unique_ptr<T> take_from(Context* C, std::unordered_map<uint64_t, std::unique_ptr<T>>& table, uint64_t h) {
  std::lock_guard<std::mutex> lk(C->mu);
  auto it = table.find(h);
  if (it == table.end()) return nullptr;
  std::unique_ptr<T> p = std::move(it->second);
  table.erase(it);
  return p;
}
template <class T>
inline uint64_t put_in(Context* C, std::unordered_map<uint64_t, std::unique_ptr<T>>& table, std::unique_ptr<T> p) {
  std::lock_guard<std::mutex> lk(C->mu);
  const uint64_t h = C->next_handle++;
  table[h] = std::move(p);
  return h;
}

#define GM_FR_LOCK(C) std::lock_guard<std::recursive_mutex> gm_fr_lock_((C)->fr_mu)
// (the guard also counts the MSM scopes that are open: release_spare_tables must not free a table an MSM in flight reads)
struct MsmBusyGuard {
  std::atomic<int>& n;
  explicit MsmBusyGuard(std::atomic<int>& c) : n(c) { n.fetch_add(1); }
  ~MsmBusyGuard() { n.fetch_sub(1); }
};
#define GM_MSM_LOCK(C)                                                \
  std::lock_guard<std::recursive_mutex> gm_msm_lock_((C)->msm_mu); \
  ::gm::MsmBusyGuard gm_msm_busy_((C)->msm_busy)

#define GM_CTX()                                            \
  ::gm::Context* C = ::gm::context();                       \
  GM_CHECK(C != nullptr, GM_ENOTINIT, "gm_init has not been called")

// MSM engine (msm.hip)
int bases_build_prefix_sets(Context* C, Bases* b);
size_t msm_workspace_held(const MsmWorkspace& ws);
size_t msm_workspace_bound(Context* C, const Bases* bases, size_t n);
int msm_run(Context* C, const Bases* bases, int64_t first, int64_t step, const void* d_scalars, int mont, size_t n,
            bool normalize, uint64_t out_jac[18]);
int msm_run_batch(Context* C, const Bases* bases, int64_t first, int64_t step, const void* const* d_scalars, int mont, const size_t* ns,
                  size_t k, bool normalize, uint64_t* out_jac);
// call j walks the bases from index pair_offsets[j] (step +1) or DOWN from it (step -1)
int msm_run_batch_offsets(Context* C, const Bases* bases, const size_t* pair_offsets, int64_t step, const void* const* d_scalars, int mont,
                          const size_t* ns, size_t k, bool normalize, uint64_t* out_jac);
// The digit and sort stage of ONE plain call (no tables, no GLV, no window groups) for a second group: the digit, sort and scan
// kernels of msm_enqueue (the direct scatter variants of the block sort) and the same choice between the flat and the block sort,
// on `ws` and `st`.  Entries are (key << 32 | sign << 31 | pair index),
// grouped by key = window * B + |digit| - 1; offsets[k] is where key k starts, offsets[nbuckets] the entry count.
struct MsmSorted {
  const uint64_t* entries = nullptr;
  const uint32_t* offsets = nullptr;
  const uint32_t* err = nullptr;  // != 0 after the sort: a scalar was >= 2^255
  int W = 0;
  uint32_t B = 0;
  size_t nbuckets = 0;
};
int msm_sort_plain(Context* C, MsmWorkspace& ws, hipStream_t st, const void* d_scalars, int mont, size_t n, int c, MsmSorted* out);
int msm_ceil_log2(size_t n);
// pair_offsets[j] (optional): call j starts at base pair_offsets[j] (absolute, whatever the step) and walks step from there
// firsts[j] (optional): call j starts at base firsts[j] instead of `first` (herring: even / odd halves of one array)
int msm_run_batch_at(Context* C, const Bases* bases, int64_t first, int64_t step, const size_t* pair_offsets, const void* const* d_scalars,
                     int mont, const size_t* ns, size_t k, bool normalize, uint64_t* out_jac, const int64_t* firsts = nullptr);

// keys of either group (bases.hip; stated once over the descriptions of groups.cuh, these are the instances the other files call)
int bases_from_host(Context* C, const void* bases, size_t stride, size_t n, std::unique_ptr<Bases>& out);
int g2_bases_from_host(Context* C, const void* bases, size_t stride, size_t n, std::unique_ptr<G2Bases>& out);
int g1_pack_launch(hipStream_t st, const uint8_t* src, size_t stride, size_t n, uint8_t* dst);  // host records -> packed device records, no wait
// n XYZZ records -> packed affine records, eight points per inversion, no wait; `out` must lie apart from `in`
int g1_normalise_launch(hipStream_t st, const uint8_t* in, size_t n, uint8_t* out);
// out[i] = in[2i] + s in[2i+1] over packed affine records (an odd tail folds against the identity), s at d_s8 (canonical, 8 x u32), on C->stream
int g1_split_fold_launch(Context* C, const uint8_t* in, size_t n, const uint32_t* d_s8, uint8_t* out);
int g2_split_fold_launch(Context* C, const uint8_t* in, size_t n, const uint32_t* d_s8, uint8_t* out);
// the same over records read backwards, in[n - 1 - j] in place of in[j]: the first level over a key that holds a big-endian stream
int g1_split_fold_rev_launch(Context* C, const uint8_t* in, size_t n, const uint32_t* d_s8, uint8_t* out);
int g2_split_fold_rev_launch(Context* C, const uint8_t* in, size_t n, const uint32_t* d_s8, uint8_t* out);
// out[i] = in[n - 1 - i] over records of rec_bytes (a multiple of 16), `out` apart from `in`
int records_reverse_launch(Context* C, const uint8_t* in, size_t n, size_t rec_bytes, uint8_t* out);
// The segmented form (k_split_fold_seg): span k folds its n records at `in` to (n + 1) / 2 records at `out` by the canonical scalar
// in row `ch` of the table d_s8 (8 x u32 a row) -- the spans of many proofs in one launch, every proof under its own challenge.
// All spans of a launch have the same length n; the table of spans is on the device.  On C->stream without a wait.
struct FoldSpan {
  const uint8_t* in;
  uint8_t* out;
  uint32_t ch, pad;
};
int g1_split_fold_seg_launch(Context* C, const FoldSpan* d_spans, size_t nspans, size_t n, const uint32_t* d_s8);
int g2_split_fold_seg_launch(Context* C, const FoldSpan* d_spans, size_t nspans, size_t n, const uint32_t* d_s8);
// Short linear combinations over vectors that are on the device already (k_term_mul, k_seg_sum, k_normalise; bases.hip), each a
// launch on C->stream without a wait.  term_mul: out[t] = scalar[sidx ? sidx[t] : t] * point[pidx ? pidx[t] : t] in XYZZ, the
// scalars 32-byte records, Fr in Montgomery form when `mont`, else canonical.  seg_sum: out[s] = the sum of in[off[s] .. off[s + 1])
// with the complete addition.  g2_normalise_launch: as g1_normalise_launch.
int g1_term_mul_launch(Context* C, const uint8_t* d_points, const uint32_t* d_pidx, const uint8_t* d_scalars, const uint32_t* d_sidx, int mont, size_t T, uint8_t* d_out_xyzz);
int g2_term_mul_launch(Context* C, const uint8_t* d_points, const uint32_t* d_pidx, const uint8_t* d_scalars, const uint32_t* d_sidx, int mont, size_t T, uint8_t* d_out_xyzz);
int g1_seg_sum_launch(Context* C, const uint8_t* d_in_xyzz, const unsigned long long* d_off, size_t S, uint8_t* d_out_xyzz);
int g2_seg_sum_launch(Context* C, const uint8_t* d_in_xyzz, const unsigned long long* d_off, size_t S, uint8_t* d_out_xyzz);
int g2_normalise_launch(hipStream_t st, const uint8_t* in, size_t n, uint8_t* out);
// gm_g2_lincomb_many: the G2 twin of g1_lincomb_many_host (192-byte records, 36-limb results); three launches and one wait
int g2_lincomb_many_host(Context* C, const void* points, size_t stride, const uint64_t* scalars_canonical, const size_t* offsets, size_t S, uint64_t* out_jac);

// S short linear combinations out[s] = sum_{offsets[s] <= t < offsets[s+1]} scalar[t] P[t] (k_g1_term_mul, k_g1_seg_sum,
// k_normalise): host records of `stride` bytes and canonical scalars in, S packed affine device records at *d_aff (a
// region of C->lincomb), on C->stream without a wait.  Caller holds the MSM lock and keeps the three host arrays until it has waited.
int g1_lincomb_many_launch(Context* C, const void* points, size_t stride, const uint64_t* scalars_canonical, const size_t* offsets, size_t S, uint8_t** d_aff);
int g1_lincomb_many_host(Context* C, const void* points, size_t stride, const uint64_t* scalars_canonical, const size_t* offsets, size_t S, uint64_t* out_jac);

// Fr vectors (fr.hip), on C->stream without a wait
int fr_stride_raw(Context* C, const uint8_t* in, size_t start, size_t stride, size_t count, uint8_t* out);
int fr_fold_raw(Context* C, const uint8_t* f, size_t n, const uint64_t r[4], uint8_t* out);  // r is read by an asynchronous copy: the caller waits
int fr_reverse_raw(Context* C, const uint8_t* in, size_t n, uint8_t* out);                  // out[i] = in[n - 1 - i]
// the half tables of tensor(challenges): lo over the first klo of the k challenges at d_ch (Montgomery, 32 B each), hi over the rest
int fr_tensor_tables_raw(Context* C, const uint8_t* d_ch, uint32_t k, uint32_t klo, uint8_t* lo, uint8_t* hi);
int hsp_scalars_raw(Context* C, const HspArgs& A);  // k_hsp_scalars: the scalars of a message of the module space prover
// out[i] = sum_j c_j v_j[i], v_j = base + j * pitch_bytes, k vectors of n elements; launches only, the caller waits
int fr_lincomb_raw(Context* C, const uint8_t* base, size_t pitch_bytes, size_t n, const uint64_t* coeffs_mont, size_t k, uint8_t* out);

// G2 engine (g2msm.hip)
int g2_msm_run(Context* C, const G2Bases* bases, int64_t first, int64_t step, const void* d_scalars, int mont, size_t n, uint64_t out_jac[36]);
void g2_workspace_release(G2Workspace& w);

// pairings (pairing.hip): GT values are 72 limbs, 12 Fq in tower order, Montgomery
int pairing_run(Context* C, const uint8_t* d_g1, int64_t first1, int64_t step1, const uint8_t* d_g2, int64_t first2, int64_t step2, size_t n, uint64_t out_gt[72]);
int pairing_run_host(Context* C, const void* g1, size_t stride1, const void* g2, size_t stride2, size_t n, uint64_t out_gt[72]);
void pairing_workspace_release(PairingWorkspace& w);
struct PairSpan {  // n pairs (g1[first1 + step1 i], g2[first2 + step2 i]) of packed device records; ranges checked by the caller
  const uint8_t* g1 = nullptr;
  const uint8_t* g2 = nullptr;
  int64_t first1 = 0, step1 = 1, first2 = 0, step2 = 1;
  size_t n = 0;
};
// The Miller product of both spans, NOT conjugated, not exponentiated.  Caller holds the MSM lock.
int miller_product(Context* C, const PairSpan& s0, const PairSpan& s1, gmh::Fq12* out);
// S independent products in one launch per level of the reduction, however many products there are (pairing.hip: k_miller_seg)
struct PairProduct {
  PairSpan s0, s1;
};
int miller_products(Context* C, const PairProduct* prods, size_t S, gmh::Fq12* out);
// the same S products as GT elements (S x 72 limbs): conjugation and ONE k_gt_final_exp launch over the Miller values on the device
int pairing_products(Context* C, const PairProduct* prods, size_t S, uint64_t* out_gt);
// gm_pairing_multi_many: product s is over the host pairs [offsets[s], offsets[s + 1])
int pairing_products_host(Context* C, const void* g1, size_t stride1, const void* g2, size_t stride2, const size_t* offsets, size_t S, uint64_t* out_gt);
// The batched KZG checks (verifier.cpp): one g1_lincomb_many_launch over all segments, then check s is the product of the pairs
// (sum[check_seg[s] + j], d_g2[j == 0 ? 0 : j - 1]), j < check_seg[s + 1] - check_seg[s]: ONE k_miller_seg, ONE k_gt_final_exp, one wait.
// ok[s] = the product is 1.
int kzg_checks_run(Context* C, const uint8_t* d_g2, const void* points, size_t stride, const uint64_t* scalars_canonical, const size_t* seg_offsets,
                   size_t nseg, const size_t* check_seg, size_t S, int* ok);
// Miller product -> GT: conjugation (the loop parameter is negative), then the one final exponentiation
void pairing_finish(const gmh::Fq12& miller, uint64_t out_gt[72]);

// GtModule (pairing.hip): GT elements on the device are 576-byte records, 12 Fq in tower order in the device form of g1.cuh
struct GtSpan {  // n terms x[first_x + step_x i] ^ e[first_e + step_e i]: 576-byte elements, 32-byte exponents; ranges checked by the caller
  const uint8_t* x = nullptr;
  const uint8_t* e = nullptr;
  int64_t first_x = 0, step_x = 1, first_e = 0, step_e = 1;
  size_t n = 0;
};
// The product over three spans in one launch, no final exponentiation and no conjugation.  mont: the exponents are Fr in Montgomery
// form (the canonical integer is taken on the device); else 8 canonical words as they are, not reduced.  Caller holds the MSM lock.
int gt_multi_pow(Context* C, const GtSpan spans[3], int mont, gmh::Fq12* out);
int gt_multi_pow_host(Context* C, const uint64_t* x, const uint64_t* scalars_canonical, size_t n, uint64_t out_gt[72]);
// The segmented form (k_gt_multi_pow_seg): S independent products in one launch per level.  A term names a row of a table of 576-byte
// elements and a row of a table of 32-byte canonical exponents, so many terms may raise the same element.
struct GtTerm {
  uint32_t x, e;
};
// gm_gt_multi_pow_many: product s is over the host terms [offsets[s], offsets[s + 1])
int gt_multi_pow_many_host(Context* C, const uint64_t* x, const uint64_t* scalars_canonical, const size_t* offsets, size_t S, uint64_t* out_gt);
// The two halves of S batched inner-product checks (ipa.hip) in one launch group and one wait: out_gt[s] = FE(conj(Miller product of
// prods[s])), out_gt[S + s] = the product of the terms [offsets[s], offsets[s + 1]) over the device tables d_x (rows < nx) and d_e
// (rows < ne).  Every product is non-empty.  Caller holds the MSM lock.
int gt_checks_run(Context* C, const PairProduct* prods, const uint8_t* d_x, size_t nx, const uint8_t* d_e, size_t ne, const GtTerm* terms, const size_t* offsets, size_t S,
                  uint64_t* out_gt);
// One round of many inner-product provers (ipa.hip: ipa_prove_many): the P non-empty Miller products stay on the device and are the
// rows the terms name; out_gt[s] = FE(conj(prod over the terms [offsets[s], offsets[s + 1]) of Miller[t.x]^e[t.e])), e the ne host
// rows of 4 canonical limbs.  One k_miller_seg, one k_gt_multi_pow_seg, their reduction levels, one k_gt_final_exp, one export and
// ONE wait; *launches gets the number of kernels enqueued.  Every product and every term range is non-empty.  Caller holds the MSM lock.
int miller_gt_products(Context* C, const PairProduct* prods, size_t P, const uint64_t* exps_canonical, size_t ne, const GtTerm* terms, const size_t* offsets, size_t S,
                       uint64_t* out_gt, size_t* launches);
int gt_from_host(Context* C, const uint64_t* x, size_t n, uint8_t** d);  // n x 72 limbs -> a dev_malloc block of device records
// out[i] = in[2i] in[2i+1]^s (an odd tail is in[2i]), s at d_s8 (canonical, 8 x u32), on C->stream; caller holds the MSM lock
int gt_split_fold_launch(Context* C, const uint8_t* in, size_t n, const uint32_t* d_s8, uint8_t* out);
// GT element by element (pairing.hip: k_gt_final_exp, k_miller_each, k_gt_check).  The *_launch / *_run forms work on device records
// under the caller's MSM lock; the others take it.
int gt_final_exp_launch(Context* C, const uint8_t* in, size_t n, int conj, uint8_t* out);  // out[i] = (conj ? conj(in[i]) : in[i])^((q^12 - 1) / r), no wait
int gt_final_exp_many(Context* C, const uint64_t* in, size_t n, uint64_t* out);
int pairing_each_run(Context* C, const uint8_t* d_g1, int64_t first1, int64_t step1, const uint8_t* d_g2, int64_t first2, int64_t step2, size_t n, uint64_t* out_gt);
int pairing_each_host(Context* C, const void* g1, size_t stride1, const void* g2, size_t stride2, size_t n, uint64_t* out_gt);
int gt_check_run(Context* C, const uint8_t* d_src, int host_form, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok);
int gt_check_host(Context* C, const uint64_t* x, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok);
int gt_debug_op(Context* C, int op, const uint64_t* in, size_t n, uint64_t* out);
// test aids for the Miller-loop half: one tower function, one step, one raw Miller value per lane
int gt_debug_op2(Context* C, int op, const uint64_t* a, const uint64_t* b_or_null, size_t n, uint64_t* out);
int miller_debug_step(Context* C, int op, const uint64_t* in, size_t n, uint64_t* out);
int miller_debug_each(Context* C, const void* g1, size_t stride1, const void* g2, size_t stride2, size_t n, uint64_t* out);

// herring module provers (herring.hip).  f / g are host arrays: Fr vectors in Montgomery form (the stride is ignored) or point
// records of f_stride / g_stride bytes; messages and final foldings have the module's limb counts (include/gemini_hip.h).
// on_device: bit 0 / bit 1 say that f / g is a packed DEVICE vector of the side's element size, which is copied (ipa.hip: the CRS)
int herring_create(Context* C, HerringModule module, const void* f, size_t f_stride, size_t nf, const void* g, size_t g_stride, size_t ng,
                   const uint64_t twist[4], uint64_t* handle, int on_device = 0);
void herring_destroy(Context* C, HerringProver* H);
int herring_fold(Context* C, HerringProver* H, const uint64_t r[4]);
int herring_round(Context* C, HerringProver* H, const uint64_t* challenge, uint64_t* a, uint64_t* b, int* has_msg);
int herring_final(Context* C, HerringProver* H, uint64_t* f0, uint64_t* g0, int* has);
int herring_gt_check(Context* C, HerringProver* H, size_t* first_bad, int* ok);  // GtModule: k_gt_check over the current f
// the space prover of G1Module / G2Module (herring.hip).  `key` is a Bases (HERRING_G1) or a G2Bases (HERRING_G2) that outlives the
// prover, or nullptr with host records `host_points` of `stride` bytes, which become a key of the prover's own; the scalar stream
// is a device vector (on_device) or a host array, Montgomery, big-endian like the points
int hsp_create(Context* C, HerringModule module, const void* key, size_t offset, const void* host_points, size_t stride, size_t np,
               const void* scalars, size_t ns, bool on_device, const uint64_t twist[4], uint64_t* handle);
void hsp_destroy(Context* C, HerringSpace* H);
int hsp_fold(Context* C, HerringSpace* H, const uint64_t r[4]);
int hsp_round(Context* C, HerringSpace* H, const uint64_t* challenge, uint64_t* a, uint64_t* b, int* has_msg);
int hsp_final(Context* C, HerringSpace* H, uint64_t* point0, uint64_t* scalar0, int* has);
int hsp_to_time(Context* C, HerringSpace* H, uint64_t* time_handle);

// herring's inner-product argument (ipa.hip)
int crs_create(Context* C, const void* g1, size_t stride1, size_t n1, const void* g2, size_t stride2, size_t n2, uint64_t* handle);
void crs_destroy(Crs* c);
int crs_commit(Context* C, const Crs* crs, int group, const uint64_t* scalars_mont, size_t n, uint64_t* out_jac);
int vrs_from_crs(Context* C, const Crs* crs, Vrs* out);
int ipa_prove(Context* C, uint64_t transcript, const Crs* crs, const uint64_t* a_mont, const uint64_t* b_mont, size_t d, IpaProof* proof);
int ipa_verify(Context* C, const IpaProof* proof, const Vrs* vrs, const uint64_t comm_a[18], const uint64_t comm_b[36], const uint64_t y_mont[4], int* ok);
// S proofs in one launch group; ok[s] is ipa_verify's answer for every input
int ipa_verify_many(Context* C, const IpaProof* const* proofs, const Vrs* vrs, const uint64_t* comm_a /* S x 18 */, const uint64_t* comm_b /* S x 36 */,
                    const uint64_t* y_mont /* S x 4 */, size_t S, int* ok);
// gm_ipa_new_many: proofs[s] = ipa_prove(transcripts[s], crs, a_s, b_s, d), the rounds of all proofs in lockstep (one launch group a
// round) from C->ipa_new_many_min proofs on.  The caller has checked the handles; nothing is absorbed on a refusal.
int ipa_prove_many(Context* C, const uint64_t* transcripts, const Crs* crs, const uint64_t* a_mont, const uint64_t* b_mont, size_t d, size_t S, IpaProof* const* proofs);
bool transcript_exists(uint64_t handle);  // transcript.cpp
// gm_ipa_new_batch: ONE proof for K claims over the same CRS (InnerProductProof::generic, ipa.rs:345-531, every twist one, one d);
// gm_ipa_verify_batch: verify_transcript with 3 K initial claims.  Nothing is absorbed on a refusal.
int ipa_prove_batch(Context* C, uint64_t transcript, const Crs* crs, const uint64_t* a_mont /* K x d x 4 */, const uint64_t* b_mont, size_t d, size_t K, IpaProof* proof);
int ipa_verify_batch(Context* C, const IpaProof* proof, const Vrs* vrs, const uint64_t* comm_a /* K x 18 */, const uint64_t* comm_b /* K x 36 */, const uint64_t* y_mont /* K x 4 */,
                     size_t K, int* ok);
// gm_debug_ipa_stated_terms: the canonical exponents of the stated form of one proof, 6 R - 4 GT terms then 2 R + 4 pairing terms
int ipa_stated_terms(const IpaProof* proof, const uint64_t y_mont[4], uint64_t* gt_exp, uint64_t* pair_exp);
// Jacobian points of both groups -> the host records of the proof checks and a GM_PT_* status byte each (points.hip), one launch per group
int jac_points_status(Context* C, const std::vector<const uint64_t*>& g1, const std::vector<const uint64_t*>& g2, std::vector<uint64_t>& r1, std::vector<uint64_t>& r2,
                      std::vector<uint8_t>& st1, std::vector<uint8_t>& st2);

}  // namespace gm
