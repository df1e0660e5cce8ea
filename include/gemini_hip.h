/*
 * gemini_hip.h -- C ABI of libgemini_hip.so, the MI355X (gfx950) implementation of Gemini's
 * prover hot path.  Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * arkworks-rs/gemini checkout; ark-ec/ark-ff are third-party crates pinned in Cargo.lock:44-64).
 * INTEGRATION.md shows the Rust `extern "C"` block and the feature-gated call sites.
 *
 * Conventions
 *   - Fr elements: 4 x u64 little-endian limbs.  "mont" = Montgomery form a*2^256 mod r, exactly
 *     the in-memory image of ark-ff `Fr` (zero-copy from `&[Fr]`).  "canonical" = the integer
 *     itself, i.e. `Fr::into_bigint()` / `BigInt<4>`.
 *   - G1 affine bases: x, y as 6 x u64 Montgomery limbs each (96 bytes).  `stride` >= 96; if
 *     stride >= 97, byte 96 is ark-ec's `infinity: bool` (Rust `G1Affine` has stride 104).
 *     With stride 96 the identity is encoded as x = y = 0.
 *   - G1 results: Jacobian X, Y, Z (18 x u64, Montgomery) = the image of ark-ec
 *     `Projective<g1::Config>`.  Results are normalised (Z = R, or (R, R, 0) for the identity)
 *     so equal group elements always produce equal bytes.
 *   - G2 affine bases: x.c0 | x.c1 | y.c0 | y.c1, each 6 x u64 Montgomery limbs (192 bytes), an Fq2 element being
 *     c0 + c1 u with u^2 = -1: the image of ark-ec `Affine<g2::Config>` without its flag.  `stride` >= 192 and a multiple
 *     of 8 (anything else gives GM_EINVAL); from stride 200 on, byte 192 is ark-ec's `infinity: bool` (the Rust record's stride).  With stride 192 the
 *     identity is the all-zero record.
 *   - G2 results: Jacobian X, Y, Z over Fq2 (36 x u64, Montgomery, c0 before c1) = the image of ark-ec
 *     `Projective<g2::Config>`, normalised like the G1 results (Z = (R, 0), or ((R, 0), (R, 0), 0) for the identity).
 *   - Return value: 0 = ok, negative = GM_E*.  Nothing throws or aborts across the boundary;
 *     gm_last_error() gives a message for the calling thread.
 *   - Ownership: the caller owns every host buffer for the duration of the call only; registered
 *     bases and vectors are copied to device memory owned by the library until *_free.
 *   - Threading: one process per GPU.  Every entry point may be called from any thread.  Calls on
 *     different prover handles run concurrently (sumcheck::prove_batch calls next_message on distinct
 *     provers from different rayon threads, src/subprotocols/sumcheck/proof.rs:85; `Prover: Send + Sync`,
 *     prover.rs:30); calls on the SAME prover handle are serialised by a per-handle lock.  MSM calls
 *     (gm_g1_msm*, gm_g2_msm*, gm_pairing_*, herring G1 / G2 / P rounds) share the device workspaces and are serialised by one library
 *     lock held from the staging of host scalars to the result (the reference's MSM calls are
 *     sequential too, src/kzg/time.rs:103-106); the vector entry points (gm_fr_*) are serialised by a
 *     second lock because they stage per-call parameters in one scratch buffer.  Results never depend
 *     on the interleaving (tests/test_gpu_threads.py).  Freeing a handle another thread is still using
 *     is the caller's error, as with any Rust `Drop`.
 *   - Scalars passed as canonical integers (mont = 0) must be < r, as ark-ff's BigInt images of Fr
 *     always are; the library rejects a call holding a scalar >= 2^255 with GM_EINVAL and does not
 *     otherwise check (the reference panics on the out-of-range bucket index such a value produces).
 */
#ifndef GEMINI_HIP_H
#define GEMINI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GM_OK 0
#define GM_EINVAL (-1)    /* bad length / null pointer / bad stride */
#define GM_ENOTINIT (-2)  /* gm_init not called */
#define GM_EHANDLE (-3)   /* unknown or freed handle */
#define GM_EHIP (-4)      /* HIP runtime error, see gm_last_error() */
#define GM_ENOMEM (-5)
#define GM_ESTATE (-6)    /* call sequence error (e.g. round message after the last round) */

/* ---- lifecycle -------------------------------------------------------------------------- */
/* Bind this process to GPU `device` (hipSetDevice) and create the library's streams. */
int gm_init(int device);
void gm_shutdown(void);
const char* gm_last_error(void);
/* ABI version, bumped on any signature change. */
int gm_abi_version(void);

/* ---- G1 multi-scalar multiplication ------------------------------------------------------- */
/* Replaces VariableBaseMSM::msm_bigint(bases, bigints) of ark-ec 0.4.2 -- the function every
 * MSM call site of the reference bottoms out in (src/kzg/time.rs:82,129; src/kzg/space.rs:52;
 * ChunkedPippenger/HashMapPippenger flushes, in-tree copy src/kzg/msm/stream_pippenger.rs:180,250,264;
 * algorithm statement src/kzg/msm/variable_base.rs:99-176).
 * scalars: n x 4 u64 canonical (< r).  Like msm_unchecked, the caller passes n = min(lengths). */
int gm_g1_msm(const void* bases, size_t base_stride, const uint64_t* scalars, size_t n, uint64_t out_jac[18]);
/* S independent SHORT linear combinations (tens of terms each, where an MSM has millions): out[s] = sum over
 * offsets[s] <= t < offsets[s + 1] of scalars[t] * points[t]; records and canonical scalars as for gm_g1_msm, offsets[0] = 0, S + 1
 * entries, out_jac: S x 18 limbs, normalised.  One lane per term, then one per segment: three launches and one wait whatever S is.
 * The additions are complete (equal terms double, opposite ones cancel); an empty segment, a zero scalar and the all-zero record
 * give the identity. */
int gm_g1_lincomb_many(const void* points, size_t stride, const uint64_t* scalars_canonical, const size_t* offsets, size_t S, uint64_t* out_jac);
/* The G2 twin: records of at least 192 bytes as for gm_g2_msm, out_jac: S x 36 limbs, normalised.  The same contract -- complete
 * additions, so equal terms double and opposite terms cancel; an empty segment, a zero scalar and the all-zero record give the
 * identity -- and the same three launches (one lane per term, one per segment, the batched normalisation) and one wait whatever
 * S is. */
int gm_g2_lincomb_many(const void* points, size_t stride, const uint64_t* scalars_canonical, const size_t* offsets, size_t S, uint64_t* out_jac);

/* SRS resident in HBM: replaces the `powers_of_g: Vec<G1Affine>` field of CommitterKey
 * (src/kzg/time.rs:24-27) as the MSM operand.  The bases are copied; `handle` is opaque.  Cost: one upload and one
 * repacking pass; NO fixed-base tables are built here (a registration may serve a single MSM) -- a key that stays
 * resident asks for them with gm_g1_bases_precompute(handle, -1). */
int gm_g1_bases_register(const void* bases, size_t base_stride, size_t n, uint64_t* handle);
int gm_g1_bases_free(uint64_t handle);
int gm_g1_bases_len(uint64_t handle, size_t* n);
/* Copy registered bases back (96-byte stride): used by tests and by CommitterKey::index_by. */
int gm_g1_bases_download(uint64_t handle, size_t offset, size_t n, void* out96);

/* Fixed-base window tables for a registered SRS: table[w][i] = 2^(c*w) * base[i] for w < ceil(256/c),
 * kept in HBM (W x n x 96 bytes -- 40 GB for the 2^25-point SRS of `snark -i 24`; this is what 288 GB
 * per GPU buys).  Afterwards MSMs of >= 2^17 pairs against this handle use ONE bucket set shared by
 * all windows: c = 20 instead of 16 (13 instead of 16 base additions per pair), no per-window bucket
 * reduction and c instead of 256 doublings at the end.  Results are identical (tests compare both
 * paths).  Setup cost is comparable to generating the SRS; like CommitterKey::new it is outside the
 * prover timer.  c = 0 picks the default (20 below 2^23 points; 22 from there on, which serves calls from 2^22 pairs on, PLUS a
 * c = 20 table over the first 2^22 points -- 5.2 GB -- for the calls of 2^17 .. 2^22 - 1 pairs whose index range stays inside that
 * prefix: the low levels of a folding tree -- and, for every key, a c = 16 table over the first 2^17 points, 201 MB, for the
 * latency-bound calls of 2^11 .. 2^17 - 1 pairs: one bucket set, 16 final doublings); c = -1 is AUTOMATIC: the rule of gm_set_auto_tables below (2^17 .. 2^26 - 1
 * points, byte budget, free memory; a no-op returning GM_OK when the tables do not fit or exist already).
 * No reference counterpart: ark-ec recomputes. */
int gm_g1_bases_precompute(uint64_t handle, int c);
/* Tables BY DEFAULT (on = 1 at gm_init) for the KEY CONSTRUCTORS: gm_g1_fixed_base_register, gm_g1_srs_register and
 * gm_g1_srs_register_segments (the CommitterKey::new analogues) build the tables above for 2^17 .. 2^26 - 1 points (a key of
 * 2^26 .. 2^28 - 1 points gets tables over its first 2^25 / 2^22 / 2^17 points only: 44 GB, spare memory -- see
 * gm_g1_release_spare_tables) when
 * W x n x 96 bytes fit `max_bytes` (0 = 30 % of the device memory) and the free memory; otherwise, silently, the plain path
 * serves the key.  Cost at registration: ~240 doublings per point and W x n x 96 bytes (1.3 GB at 2^20 points).
 * gm_g1_bases_register (points uploaded from the host) never builds them on its own: gm_g1_bases_precompute(handle, -1).
 * A committer key is registered once and serves ~3 N pairs of MSMs per proof; the build is setup, like
 * CommitterKey::new (src/kzg/time.rs:49-72, which builds a window table of its own to generate the key). */
int gm_set_auto_tables(int on, size_t max_bytes);
/* Window width of the main tables (0 = no tables) and size in bytes of all tables of a handle (prefix table included). */
int gm_g1_bases_table_info(uint64_t handle, int* c, size_t* bytes);
/* Give the freed blocks of the device-vector pool (up to 55 % of the device memory) back to the driver -- for a host
 * process that shares the GPU with another allocator (torch, a second rank). */
int gm_pool_trim(void);
/* Device-memory bookkeeping of the library (every allocation it makes is counted): out[0] = device total, [1] = device free
 * (hipMemGetInfo), [2] = bytes the library holds from the driver, [3] = high-water mark of [2], [4] = of [2]: freed blocks cached by
 * the vector pool, [5] = in use = [2] - [4], [6] = high-water mark of [5], [7] = fixed-base tables of all keys, [8] = the keys
 * themselves, [9] = how many times the prefix tables were released under memory pressure (they are not rebuilt: the calls they
 * served take the plain path), [10] = what the MSM workspaces hold (grow-only), [11] = 0.  gm_mem_reset_peak() restarts both
 * high-water marks from the current values.  The reference's memory
 * story is its constants (README.md:38-46: SPACE_TIME_THRESHOLD, MAX_MSM_BUFFER_LOG); on the device it is these figures and the
 * footprint contract below (gm_snark_footprint / gm_psnark_footprint). */
int gm_mem_stats(uint64_t out[12]);
/* out[0] = compute units of the device, [1] = of those: set aside for the tails of a batch (the XCD partition, GM_CU_SPLIT; 0 = off),
 * [2] = zero-copy result paths in use (bit 0 field kernels, bit 1 MSM planes), [3] = small-call lanes of a batch */
int gm_runtime_info(int out[4]);
int gm_mem_reset_peak(void);
/* THE FOOTPRINT CONTRACT.  What a proof will allocate beyond what is resident when it is called (the key and its tables, the
 * instance, the caller's vectors): out[0] = high-water mark of its device vectors and prover buffers, out[1] = what the MSM
 * workspaces may still have to grow by for its largest calls (an upper bound; it shrinks as they grow), out[2] = out[0] + out[1], out[3] =
 * what can be had right now (device free + the vector pool's cached blocks + the prefix tables, which are spare memory).  Upper
 * bounds, within ~25 % of the measured peaks (tests/test_gpu_footprint.py, profiles/r5_footprint.txt).  Every prover compiled into
 * the library checks the same figures before its first allocation: if the proof only fits without the prefix tables they are
 * released THEN (not by reflex after an allocation has failed half-way), and if it does not fit at all the prover returns
 * GM_ENOMEM with the numbers in gm_last_error() (GM_FOOTPRINT_CHECK=0 switches the admission off).
 *   gm_snark_footprint   snark::Proof::new_time / new_elastic on num_constraints = |z|; elastic != 0: gm_snark_new_elastic
 *   gm_psnark_footprint  psnark::Proof::new_time (elastic 0), new_elastic in the resident schedule (1, min_device_chunk > 1) or
 *                        the literal one (2: space provers over reversed streams, min_device_chunk = 1)
 * ck_bases: the key the proof will commit under (its tables decide the window widths, a cyclic share divides the MSM sizes). */
int gm_snark_footprint(uint64_t ck_bases, size_t num_constraints, int elastic, uint64_t out[4]);
int gm_psnark_footprint(uint64_t ck_bases, size_t num_variables, size_t nnz, int elastic, uint64_t out[4]);
int gm_footprint_admit(int psnark, uint64_t ck_bases, size_t n, size_t nnz, int elastic);
/* Frees the PREFIX tables of every key (the c = 22 / 20 / 16 tables over the first 2^25 / 2^22 / 2^17 points; up to 44 GB for a key of
 * 2^26+ points): the calls they served take the plain path from then on, with the same results.  The library does this by itself
 * when a device allocation fails twice (after the vector pool has given its freed blocks back); never while an MSM is running. */
int gm_g1_release_spare_tables(void);

/* MSM against registered bases.  Pair i uses base[offset + i] (reversed = 0) or base[offset - i]
 * (reversed = 1).  reversed/offset express CommitterKey::commit's prefix slice
 * (src/kzg/time.rs:81-83) and CommitterKeyStream's Reverse(..) + advance_by alignment
 * (src/kzg/space.rs:36-40,108-113,291-296) without moving the SRS. */
int gm_g1_msm_h(uint64_t handle, size_t offset, int reversed, const uint64_t* scalars, size_t n, uint64_t out_jac[18]);

/* Same, scalars taken from a device-resident Fr vector (see gm_fr_vec_*), elements
 * [voffset, voffset + n).  The vector is in Montgomery form; into_bigint happens on device. */
int gm_g1_msm_v(uint64_t bases_handle, size_t offset, int reversed, uint64_t vec_handle, size_t voffset, size_t n,
                uint64_t out_jac[18]);

/* k MSMs against the same bases (CommitterKey::batch_commit, src/kzg/time.rs:98-107): MSM j pairs
 * elements [0, ns[j]) of vector j with bases[offset ...].  Same results as k gm_g1_msm_v calls; the
 * host tail of call j overlaps the kernels of call j+1.  out_jac: k x 18 limbs. */
int gm_g1_msm_v_batch(uint64_t bases_handle, size_t offset, int reversed, const uint64_t* vec_handles, const size_t* ns, size_t k,
                      uint64_t* out_jac);
/* The same with UN-NORMALISED results (any Jacobian representative, no field inversion): the per-rank partials of a
 * sharded batch_commit -- all-gathered k x 144 bytes at a time, summed and normalised once per commitment (gm_g1_sum). */
int gm_g1_msm_v_batch_partial(uint64_t bases_handle, size_t offset, int reversed, const uint64_t* vec_handles, const size_t* ns, size_t k,
                              uint64_t* out_jac);

/* The same with a base offset PER CALL: call j pairs vector j with bases[offsets[j] ...] (reversed: walking down from it).
 * One key that holds several ranges of powers back to back -- the per-level slices of a block-sharded key
 * (gm_g1_srs_register_segments) -- serves every level through one pipelined batch.  partial != 0: un-normalised results. */
int gm_g1_msm_v_batch_at(uint64_t bases_handle, const size_t* offsets, int reversed, const uint64_t* vec_handles, const size_t* ns, size_t k,
                         int partial, uint64_t* out_jac);

/* Same, raw device pointer to n x 32-byte scalars already in HBM (mont != 0: Montgomery form).
 * This is the entry bench.py times: inputs resident, result = 144 bytes. */
int gm_g1_msm_d(uint64_t bases_handle, size_t offset, int reversed, const void* d_scalars, int mont, size_t n,
                uint64_t out_jac[18]);

/* Partial-result form for sharded MSMs: identical to gm_g1_msm_d but the
 * result is NOT normalised, so ranks can all-gather 144-byte partial points and combine them
 * with gm_g1_sum. */
int gm_g1_msm_d_partial(uint64_t bases_handle, size_t offset, int reversed, const void* d_scalars, int mont, size_t n,
                        uint64_t out_jac[18]);
/* out = normalise(sum of k Jacobian points): the local EC-add after the all-gather, and
 * ChunkedPippenger's `result += chunk` (src/kzg/msm/stream_pippenger.rs:248-256). */
int gm_g1_sum(const uint64_t* points_jac, size_t k, uint64_t out_jac[18]);

/* ---- streaming MSM over HOST-resident pairs: bounded device memory ---------------------------------
 * ChunkedPippenger (src/kzg/msm/stream_pippenger.rs:209-272: with_size / add / finalize) and msm_chunks
 * (src/kzg/space.rs:22-55) collect a buffer of pairs from the streams, run one MSM, add it to the running sum
 * and start over.  Here the buffer is two device slots of `chunk_pairs` pairs: the stream (a key and a
 * polynomial that may be larger than HBM) stays in host memory, blocks of any size are pushed with _add, the
 * copy of chunk i + 1 runs under the kernels of chunk i, and _finalize returns the normalised sum -- equal to
 * the one-call MSM of the whole stream wherever it is cut.  chunk_pairs <= 2^26.  Overlap happens inside one
 * _add call (nothing of a stream stays in flight on the shared MSM lanes when a call returns): push blocks of
 * several chunks.  Host buffers may be pageable or page-locked (gm_host_alloc: copied by DMA, several times
 * faster) and are free to be reused when _add returns.  A stream is used by one thread at a time; distinct
 * streams from distinct threads are safe (their MSMs queue behind each other).
 *   _new:   every pair carries its base: records of base_stride bytes as in gm_g1_bases_register
 *           (x, y Montgomery; optional infinity flag at byte 96), scalars 32-byte integers < r
 *           (scalars_mont != 0: ark-ff Montgomery form instead).
 *   _new_h: scalars only, against registered bases starting at `offset` and walking up (reversed != 0: down,
 *           the big-endian stream view of src/kzg/space.rs:287-296); bases_host of _add is ignored.
 *   _finalize also resets the stream (the reference's finalize consumes the object); pairs_or_null receives
 *           the number of pairs summed.  A failed _add (scalar >= 2^255, bases exhausted, ...) resets it as well. */
int gm_g1_msm_stream_new(size_t chunk_pairs, size_t base_stride, int scalars_mont, uint64_t* stream);
int gm_g1_msm_stream_new_h(uint64_t bases_handle, size_t offset, int reversed, size_t chunk_pairs, int scalars_mont, uint64_t* stream);
int gm_g1_msm_stream_add(uint64_t stream, const void* bases_host, const void* scalars_host, size_t n);
int gm_g1_msm_stream_finalize(uint64_t stream, uint64_t out_jac[18], size_t* pairs_or_null);
int gm_g1_msm_stream_free(uint64_t stream);
/* page-locked host memory for the streams above (hipHostMalloc / hipHostFree) */
int gm_host_alloc(size_t bytes, void** p);
int gm_host_free(void* p);

/* Fixed-base generation on device: out[i] = scalars[i] * base (affine, 96-byte stride), registered
 * directly as a bases handle.  Replaces FixedBase::msm + normalize_batch in CommitterKey::new
 * (src/kzg/time.rs:49-59; setup, outside the prover timer) and builds benchmark inputs.
 * scalars: n x 4 u64 canonical on the host. */
int gm_g1_fixed_base_register(const uint64_t base_affine[12], const uint64_t* scalars, size_t n, uint64_t* handle);
/* powers_of_g[i] = tau^i * g for i < n, entirely on device (tau canonical). */
int gm_g1_srs_register(const uint64_t base_affine[12], const uint64_t tau[4], size_t n, uint64_t* handle);
/* Several ranges of the same powers back to back in ONE handle: segment s = tau^(starts[s] + i) * g, i < counts[s]
 * (exponents below 2^39).  What a rank of a block-sharded prover holds of CommitterKey::powers_of_g (src/kzg/time.rs:24-27):
 * its block of every folding level, addressed by gm_g1_msm_v_batch_at. */
int gm_g1_srs_register_segments(const uint64_t base_affine[12], const uint64_t tau[4], const size_t* starts, const size_t* counts, size_t nseg,
                                uint64_t* handle);

/* Tuning knob (0 = automatic): window width c of the bucket method.  The result does not depend
 * on it (tests sweep it). */
int gm_set_msm_window(int c);
/* Smallest pair count for which an MSM uses the fixed-base tables of its handle (default 2^17:
 * below that the MSM is latency-bound and few buckets win).  Tuning/test knob. */
int gm_set_msm_table_min(size_t n);
/* Tuning knob (default 0), read when bases are REGISTERED: also store phi(P_i) = (beta x_i, y_i) = lambda P_i and run
 * MSMs on those bases with every scalar split as s = v1 + v2 lambda, |v1|, |v2| < 2^127 (GLV): half the windows, twice
 * the base memory.  Same results; no net gain on MI355X as measured.  A round-3 EXPERIMENT: the code
 * (gemini_amd/csrc/msm_glv.inc) is only in builds with -DGM_EXPERIMENTS; otherwise on != 0 returns GM_EINVAL. */
int gm_set_msm_glv(int on);
/* The bucket sort of a plain one-call MSM (no tables) above 2^21 entries whose pair index, sign and 10 fine key bits fit 32 bits
 * (2^17 < n <= 2^21 pairs at c = 16).  mode 1 (default): the first pass writes 4-byte entries and ONE block finishes each coarse
 * group of the second; mode 0: the 8-byte passes every other call takes.  cap: entries such a block loads at once -- 0 = all its
 * LDS holds (37 872); a smaller value (>= 1024) makes ordinary inputs take the chunked branch that oversized groups take.
 * GM_EINVAL for a cap outside that range.  The result does not depend on either.  Test / A-B knob. */
int gm_set_msm_sort_group(int mode, size_t cap);
/* Which sort the last finished MSM call took: 0 = the 8-byte passes (or no block sort at all), 1 = 4-byte entries with every
 * coarse group loaded once, 2 = 4-byte entries with at least one group chunked.  Travels with the call's result: no extra sync. */
int gm_debug_msm_sort_path(int* out);
/* The optimistic path of an unsplit one-call MSM (batches, fused passes, streams and G2 do not take it).  sort_bins (default 1):
 * where gm_set_msm_sort_group's 4-byte sort applies and the mean coarse group leaves room, its first pass writes into one
 * fixed-capacity bin per group, without the counting pass and the scan in front of it.  boundary_pass (default 1): the buckets
 * that cross a chunk boundary of the accumulation are finished by one full-width pass in place of the merge levels.  The device
 * checks what each part relies on (every group fits its bin; no bucket is spread over three or more chunks); a call whose check
 * fails is run again without that part, and the next 2^k one-calls (k = 0 .. 10, one more per consecutive failure, reset by a
 * success) go straight to the general path.  The result does not depend on either.  Setting resets the back-off.  GM_EINVAL for
 * values outside {0, 1}.  Test / A-B knob. */
int gm_set_msm_optimistic(int sort_bins, int boundary_pass);
/* The last finished one-call MSM: out[0] = fixed bins gave the result, out[1] = the boundary pass gave the result, out[2] = 0 or
 * the parts whose check failed and made the call run again (1 = a bin overflowed, 2 = a bucket of three or more chunks, 3 = both),
 * out[3] = calls run again since gm_init, out[4] = the chunk length L of the accumulation. */
int gm_debug_msm_optimistic(int out[5]);
/* Tuning knob (default 0): run one-call MSMs of >= 2^17 pairs as two window groups pipelined over three streams.
 * Same results; slower on MI355X as measured.  Builds with -DGM_EXPERIMENTS only; otherwise on != 0 returns GM_EINVAL. */
int gm_set_msm_split(int on);
/* Affine tree levels in front of the XYZZ bucket accumulation (0 = none, -1 = automatic, <= 8): every
 * level adds the sorted entries of each bucket pairwise in affine coordinates with one shared field
 * inversion (6 instead of 10 field products per addition).  The result does not depend on it.
 * A round-2 EXPERIMENT, slower at every size: the kernels are only in builds with -DGM_EXPERIMENTS
 * (gemini_amd/csrc/msm_levels.inc); otherwise -1 and 0 both mean "none" and any levels > 0 returns GM_EINVAL. */
int gm_set_msm_affine_levels(int levels);

/* Per-stage device timing (HIP events on the library's stream).  Stages, in order:
 * 0 digits+histogram, 1 scan, 2 scatter, 3 bucket accumulate (k_acc0), 4 partial merge,
 * 5 bucket reduce, 6 sumcheck round, 7 the kernels of gm_idx_extend_frequency.  gm_prof_enable(1) resets and starts accumulating; gm_prof_enable(2): stage 3 only (every
 * event record between two kernels of a call is a ~10 us bubble on the stream: five stages cost an MSM ~60 us, one ~20 us);
 * gm_prof_read returns total milliseconds and launch-group counts per stage.  No reference
 * counterpart (the reference only has start_timer!/end_timer! spans, src/snark/time_prover.rs:23). */
#define GM_PROF_NSTAGES 8
int gm_prof_enable(int on);
int gm_prof_read(double* ms_out, uint64_t* count_out, int n);
/* The shader clock (MHz) the bucket accumulation ran at while profiling was on: clock64() against the constant 100 MHz
 * wall_clock64() inside the kernel, summed over the calls since gm_prof_enable(1).  The issue bound of the accumulation is
 * proportional to it, and it is NOT the nominal clock (1.9 .. 2.3 GHz under this load). 0 if none ran. */
int gm_prof_read_clock(double* acc0_mhz);

/* ---- device-resident Fr vectors ------------------------------------------------------------ */
/* Stand in for the `Vec<F>` values the time prover keeps in RAM (src/snark/time_prover.rs:32-106). */
int gm_fr_vec_alloc(size_t n, uint64_t* handle);
int gm_fr_vec_free(uint64_t handle);
int gm_fr_vec_len(uint64_t handle, size_t* n);
int gm_fr_vec_upload(uint64_t handle, size_t offset, const uint64_t* mont, size_t n);
int gm_fr_vec_download(uint64_t handle, size_t offset, uint64_t* mont, size_t n);
int gm_fr_vec_fill(uint64_t handle, const uint64_t value_mont[4]);
/* raw device pointer (for torch.from_blob-style interop and RCCL); valid until free */
int gm_fr_vec_ptr(uint64_t handle, void** dptr);
/* shrink the logical length (DensePolynomial trims trailing zeros; fold halves lengths) */
int gm_fr_vec_set_len(uint64_t handle, size_t n);

/* ---- field vector helpers (src/misc.rs) ------------------------------------------------------ */
/* out[i] = in[n-1-i]: big-endian stream <-> little-endian vector        src/iterable/slice.rs:17-39 */
int gm_fr_reverse(uint64_t in, uint64_t out);
/* out[k] = in[start + k * stride], k < count: the scalars a rank multiplies against its share of a key sharded
 * element-cyclically over the GPUs (power i lives on rank i mod g; gemini_amd/dist.py), herring's even / odd halves. */
int gm_fr_stride(uint64_t in, size_t start, size_t stride, size_t count, uint64_t out);
/* out = [f[2i] + r * f[2i+1]], len ceil(n/2)                       src/misc.rs:52-56 */
int gm_fr_fold(uint64_t f, const uint64_t r_mont[4], uint64_t out);
/* foldings_polynomial (src/subprotocols/tensorcheck/mod.rs:124-133): outs[j] = fold(outs[j - 1], challenge j) with outs[-1] = f;
 * k launches behind one another, ONE wait.  outs[j] needs capacity ceil(len / 2^(j + 1)). */
int gm_fr_fold_chain(uint64_t f, const uint64_t* challenges_mont, size_t k, const uint64_t* outs);
/* out = [1, x, x^2, ...]                                          src/misc.rs:59-65 */
int gm_fr_powers(const uint64_t x_mont[4], size_t n, uint64_t out);
/* out[sum b_j 2^j] = prod rho_j^{b_j}, len 2^k                    src/misc.rs:133-149 */
int gm_fr_tensor(const uint64_t* rhos_mont, size_t k, uint64_t out);
/* out = a . b elementwise (equal lengths, else GM_EINVAL)          src/misc.rs:205-208 */
int gm_fr_hadamard(uint64_t a, uint64_t b, uint64_t out);
/* result = sum_i a_i b_i                                           src/misc.rs:215-218 */
int gm_fr_ip(uint64_t a, uint64_t b, uint64_t result_mont[4]);
/* results[j] = sum_i p_i x_j^i for up to 3 points in one pass      src/misc.rs:194-199
 * (tensorcheck evaluates every polynomial at beta^2, beta, -beta: tensorcheck/mod.rs:228-247) */
int gm_fr_eval_le(uint64_t poly, const uint64_t* xs_mont, size_t npoints, uint64_t* results_mont);
/* The same for k polynomials at the same points, one wait for all (results: k x npoints x 4 limbs) -- the foldings of a
 * tensor check at +-beta                                            tensorcheck/mod.rs:236-247 */
int gm_fr_eval_le_batch(const uint64_t* polys, size_t k, const uint64_t* xs_mont, size_t npoints, uint64_t* results_mont);
/* out = sum_j c_j p_j padded to the longest; logical length trimmed of high zeros
 *                                                                  src/misc.rs:37-48 */
int gm_fr_lincomb(const uint64_t* polys, const uint64_t* coeffs_mont, size_t k, uint64_t out);
/* out[out_offset + i] = c * in[i] for i < len(in), inside out's current length: scaled vectors laid out side by side in one
 * vector (the per-level quotients of the block-sharded opening, committed by ONE MSM against the back-to-back key slices) */
int gm_fr_scale_into(uint64_t in, const uint64_t c_mont[4], uint64_t out, size_t out_offset);
/* the same for k vectors into disjoint ranges of `out`: k launches, one wait */
int gm_fr_scale_into_many(const uint64_t* ins, const uint64_t* coeffs_mont, size_t k, uint64_t out, const size_t* out_offsets);
/* v[positions[j]] += values[j] for k <= 4096 DISTINCT positions inside the vector (seam corrections of the laid-out opening) */
int gm_fr_add_at(uint64_t v, const size_t* positions, const uint64_t* values_mont, size_t k);
/* quotient of f by the monic vanishing polynomial of `points` (degree k <= 3); rem gets k values.
 * Replaces DensePolynomial::div in open_multi_points           src/kzg/time.rs:134-145 */
int gm_fr_div_vanishing(uint64_t f, const uint64_t* points_mont, size_t k, uint64_t quotient, uint64_t* rem_mont);

/* ---- index vectors and the entry-product / plookup vector builders (preprocessing SNARK) ---------- */
/* `&[usize]` arguments (row_index, col_index, extended frequencies) copied to HBM once. */
int gm_idx_register(const uint32_t* index, size_t n, uint64_t* handle);
int gm_idx_free(uint64_t handle);
int gm_idx_len(uint64_t handle, size_t* n);
/* the n entries of an index vector (tests, and a caller's own checks of a vector that was built on the device) */
int gm_idx_download(uint64_t handle, uint32_t* out);
/* extend_frequency(compute_frequency(set_len, index))                           plookup/time_prover.rs:65-78
 * index: a gm_idx handle with k entries, every entry < set_len (else GM_EINVAL and nothing is registered: the entries are range-checked
 * on the device before they address a counter).  *ext: a NEW gm_idx handle (gm_idx_free) with the non-decreasing sequence in which every
 * v in [0, set_len) appears 1 + #{j : index[j] == v} times; *ext_len = set_len + k, which must fit the 32-bit index vectors.
 * Built in HBM -- integer-atomic histogram, exclusive scan, expansion -- with no host pass over the index and no upload. */
int gm_idx_extend_frequency(uint64_t index, size_t set_len, uint64_t* ext, size_t* ext_len);
/* out[j] = src[index[j]]: `lookup` and `sorted`        src/subprotocols/plookup/time_prover.rs:5-8,67-74 */
int gm_fr_gather(uint64_t src, uint64_t index, uint64_t out);
/* out[i] = v[i] + F::from(index[i]) * zeta; index = 0 means the range 0..len   plookup/time_prover.rs:11-21 */
int gm_fr_alg_hash(uint64_t v, uint64_t index, const uint64_t zeta_mont[4], uint64_t out);
/* plookup_set: len + 1 entries (1+z)y + v[i-1] + z v[i]                         plookup/time_prover.rs:23-35 */
int gm_fr_plookup_set(uint64_t v, const uint64_t y_mont[4], const uint64_t z_mont[4], uint64_t out);
/* plookup_subset: out[i] = v[i] + y                                             plookup/time_prover.rs:62-64 */
int gm_fr_add_scalar(uint64_t v, const uint64_t y_mont[4], uint64_t out);
/* right_rotation(monic(v)) = [1, v...]                         src/subprotocols/entryproduct/time_prover.rs:14-23,47-51 */
int gm_fr_shift_monic(uint64_t v, uint64_t out);
/* accumulated_product(monic(v)): out[i] = prod_{j>=i} v[j], out[len] = 1 (reverse prefix-product scan)
 *                                                              src/subprotocols/entryproduct/time_prover.rs:25-45 */
int gm_fr_acc_product(uint64_t v, uint64_t out);
/* The same builders on ONE BLOCK of a block-sharded vector (gm_psnark_new_time_sharded; a block = the elements [lo, lo + M) that exist):
 *   gm_fr_tensor_range / gm_fr_powers_range   out[i] = tensor(rhos)[start + i] / x^(start + i), i < count
 *   gm_fr_plookup_set_block   plookup_set (plookup/time_prover.rs:23-35) for the outputs [lo, lo + out_count): v[v_offset .. + v_count) = the
 *                             elements lo .. of the hashed set that exist, prev = element lo - 1 (null at lo = 0)
 *   gm_fr_shift_block         right_rotation(monic(v)) (entryproduct/time_prover.rs:14-51): out[0] = first (1 on the lowest block, else the
 *                             last element of the block below), out[t] = v[t - 1]
 *   gm_fr_product             the product of the elements of v (the carry a higher block hands down)
 *   gm_fr_acc_product_block   accumulated_product(monic(v)) of a block: the suffix scan started from `carry` (the product of the blocks
 *                             above; null: one); write_monic: position |whole v| -- the entry 1 -- falls into this block */
int gm_fr_tensor_range(const uint64_t* rhos_mont, size_t k, size_t start, size_t count, uint64_t out);
/* `lookup(v, index)` (plookup/time_prover.rs:5-8) of a vector that is a FUNCTION of the index, without the vector: out[i] = tensor(rhos)[index[i]]
 * resp. x^index[i] (index[i] < 2^k / 2^log_len) -- one multiplication per element from two half tables that stay in L2.  gm_fr_alg_hash_from: the
 * algebraic hash of a RANGE of a vector, out[i] = v[i] + (first_index + i) zeta. */
int gm_fr_tensor_gather(const uint64_t* rhos_mont, size_t k, uint64_t index, uint64_t out);
int gm_fr_powers_gather(const uint64_t x_mont[4], size_t log_len, uint64_t index, uint64_t out);
int gm_fr_alg_hash_from(uint64_t v, size_t first_index, const uint64_t zeta_mont[4], uint64_t out);
int gm_fr_powers_range(const uint64_t x_mont[4], size_t start, size_t count, uint64_t out);
int gm_fr_plookup_set_block(uint64_t v, size_t v_offset, size_t v_count, const uint64_t* prev_or_null, size_t out_count, const uint64_t y_mont[4],
                            const uint64_t z_mont[4], uint64_t out);
int gm_fr_shift_block(uint64_t v, const uint64_t first_mont[4], size_t out_count, uint64_t out);
int gm_fr_product(uint64_t v, uint64_t total_mont[4]);
int gm_fr_acc_product_block(uint64_t v, const uint64_t* carry_or_null, int write_monic, uint64_t out);

/* ---- sparse R1CS matrices ------------------------------------------------------------------------ */
/* `Matrix<F> = Vec<Vec<(F, usize)>>` (src/circuit.rs:43) as CSR, copied to HBM once.  gm_spm_mul is
 * product_matrix_vector (src/misc.rs:100-110): y = M x.  Registering the TRANSPOSE turns the
 * abc_tensored scatter-add of src/snark/time_prover.rs:63-81 into three products M^T r. */
int gm_spm_register(const uint64_t* rowptr, const uint32_t* cols, const uint64_t* vals_mont, size_t nrows, size_t ncols,
                    size_t nnz, uint64_t* handle);
int gm_spm_free(uint64_t handle);
int gm_spm_mul(uint64_t matrix, uint64_t x, uint64_t y);
/* The bilinear form of the snark verifier (src/snark/verifier.rs:63-88: product_matrix_vector against powers(beta) and powers(-beta),
 * then ip against a weight vector) in ONE pass over the matrix, no n-element intermediate:
 *   out_pos = sum_r weights[r] * sum_{(v, c) in row r} v * powers[c],   out_neg = the same with (-1)^c * powers[c]
 * (powers(-beta)[c] = (-1)^c beta^c: the row sums are kept by the parity of the column).  Bit for bit the values of gm_fr_powers ->
 * gm_spm_mul -> gm_fr_ip with +-beta.  A column index >= len(powers) contributes zero (as in gm_spm_mul); weights may be LONGER than
 * the rows (tensor(rho) has 2^k >= n entries and the reference's ip_unsafe zip-truncates), shorter is GM_EINVAL; no rows or no
 * entries give (0, 0). */
int gm_spm_bilinear_pm(uint64_t matrix, uint64_t powers, uint64_t weights, uint64_t out_pos_mont[4], uint64_t out_neg_mont[4]);
int gm_spm_shape(uint64_t matrix, size_t* nrows_or_null, size_t* ncols_or_null, size_t* nnz_or_null);
/* The CSR arrays back on the host (rowptr: nrows + 1, cols: nnz, vals: nnz x 4 Montgomery limbs; any pointer may be NULL). */
int gm_spm_download(uint64_t matrix, uint64_t* rowptr, uint32_t* cols, uint64_t* vals_mont);

/* Split-phase round for callers that drive MANY provers in lock-step (Sumcheck::prove_batch maps its provers over
 * rayon, src/subprotocols/sumcheck/proof.rs:85): _begin does what gm_sc_round does up to the launch of the kernel
 * and the asynchronous copy of its partial sums, _end waits for the stream and returns the message.  Begin the
 * round of every prover, then end them: one wait instead of one per prover.  has_msg = 0 means the prover is out
 * of rounds (no _end call then); a second _begin before the _end of the same prover is GM_ESTATE. */
int gm_sc_round_begin(uint64_t handle, const uint64_t* challenge_or_null, int* has_msg);
int gm_sc_round_end(uint64_t handle, uint64_t a_mont[4], uint64_t b_mont[4]);
/* gm_sc_round_begin for k provers with the SAME challenge (the provers of Sumcheck::prove_batch, proof.rs:85): those on the device with
 * the same (fold, message) combination share a kernel launch instead of one each, up to 22 provers per launch (any k is accepted: more
 * provers make more launches); has_msg: k flags.  Collect each with gm_sc_round_end. */
int gm_sc_round_begin_many(const uint64_t* handles, size_t k, const uint64_t* challenge_or_null, int* has_msg);

/* ---- sumcheck time prover --------------------------------------------------------------------- */
/* Replaces TimeProver<F> behind `trait Prover<F>` (src/subprotocols/sumcheck/prover.rs:30-45,
 * src/subprotocols/sumcheck/time_prover.rs:42-137).  f, g are copied (Witness::new copies too,
 * time_prover.rs:26-32). */
int gm_sc_new(const uint64_t* f_mont, size_t nf, const uint64_t* g_mont, size_t ng, const uint64_t twist_mont[4],
              uint64_t* handle);
/* from device vectors (copied), for a prover that keeps its state in HBM */
int gm_sc_new_v(uint64_t f_vec, uint64_t g_vec, const uint64_t twist_mont[4], uint64_t* handle);
/* the same WITHOUT the copy: the prover reads f_vec and g_vec in place until its first fold has written their halves into its own
 * buffers -- the caller keeps both vectors alive and unmodified until then (the provers compiled into the library do: the vectors
 * are theirs).  2 x n x 32 bytes less to move and to hold per prover. */
int gm_sc_new_borrow(uint64_t f_vec, uint64_t g_vec, const uint64_t twist_mont[4], uint64_t* handle);
/* next_message(verifier_message): challenge_or_null == NULL is `None`.  *has_msg = 0 means the
 * reference returned None (round == tot_rounds).                     time_prover.rs:83-123 */
int gm_sc_round(uint64_t handle, const uint64_t* challenge_or_null, uint64_t a_mont[4], uint64_t b_mont[4], int* has_msg);
/* Prover::fold                                                        time_prover.rs:75-80 */
int gm_sc_fold(uint64_t handle, const uint64_t challenge_mont[4]);
/* rounds() / round()                                                  time_prover.rs:125-131 */
int gm_sc_rounds(uint64_t handle, size_t* tot_rounds, size_t* round);
/* final_foldings(): *has = 0 if round != tot_rounds                   time_prover.rs:133-137 */
int gm_sc_final(uint64_t handle, uint64_t f0_mont[4], uint64_t g0_mont[4], int* has);
int gm_sc_free(uint64_t handle);
/* partial-message form for sharded sumchecks: the shard holds pairs
 * [pair_offset, pair_offset + len/2) of the global vectors; twist powers start at tau^(2*pair_offset) */
int gm_sc_set_shard(uint64_t handle, uint64_t pair_offset);
/* the same for a block whose length says nothing about the rounds of the WHOLE vectors (a partial block of a block-sharded
 * prover): the prover keeps producing messages for tot_rounds rounds */
int gm_sc_set_shard_rounds(uint64_t handle, uint64_t pair_offset, size_t tot_rounds);
/* current state of the prover (TimeProver's pub fields f, g, twist: time_prover.rs:42-52): lengths and
 * twist, then the vectors themselves -- used when sharded provers hand their tails to one rank */
int gm_sc_lens(uint64_t handle, size_t* nf, size_t* ng, uint64_t twist_mont[4]);
int gm_sc_download(uint64_t handle, uint64_t* f_mont, uint64_t* g_mont);

/* ---- sumcheck space prover / elastic hand-off --------------------------------------------------- */
/* Replaces SpaceProver<F, S1, S2> behind `trait Prover<F>` (src/subprotocols/sumcheck/space_prover.rs).
 * f_stream / g_stream are the BIG-ENDIAN coefficient streams the reference consumes (Reverse(slice),
 * src/iterable/slice.rs:17-39).  Only the streams and the challenges are kept; every message is
 * recomputed from the streams (:117-240).  rounds = ceil(log2(min(len))) as in :74-77.
 * gm_sp_to_time is `TimeProver::from(&SpaceProver)` (:269-307), the switch ElasticProver::fold makes
 * when rounds - round < SPACE_TIME_THRESHOLD = 22 (elastic_prover.rs:44-57, src/lib.rs:76). */
int gm_sp_new(const uint64_t* f_stream_mont, size_t nf, const uint64_t* g_stream_mont, size_t ng, const uint64_t twist_mont[4],
              uint64_t* handle);
/* same, the streams taken from device-resident vectors (copied, like gm_sc_new_v) */
int gm_sp_new_v(uint64_t f_stream_vec, uint64_t g_stream_vec, const uint64_t twist_mont[4], uint64_t* handle);
/* without the copy: a space prover never writes its streams, so it reads the caller's vectors for its whole life -- they
 * stay alive and unmodified until gm_sp_free (gm_sp_to_time materialises the time prover in vectors of its own). */
int gm_sp_new_borrow(uint64_t f_stream_vec, uint64_t g_stream_vec, const uint64_t twist_mont[4], uint64_t* handle);
int gm_sp_round(uint64_t handle, const uint64_t* challenge_or_null, uint64_t a_mont[4], uint64_t b_mont[4], int* has_msg);
int gm_sp_fold(uint64_t handle, const uint64_t challenge_mont[4]);
int gm_sp_rounds(uint64_t handle, size_t* tot_rounds, size_t* round);
int gm_sp_final(uint64_t handle, uint64_t f0_mont[4], uint64_t g0_mont[4], int* has);
int gm_sp_to_time(uint64_t handle, uint64_t* time_handle);
int gm_sp_free(uint64_t handle);

/* ---- herring: sumcheck over a bilinear module (src/herring) --------------------------------------- */
/* FModule (F x F -> F, module.rs:127-146): the gm_sc_* prover with herring semantics -- the twist is
 * used when folding only, the message is a = <f_e, g_e>, b = <f_e, g_o> + <f_o, g_e>
 * (src/herring/time_prover.rs:91-123) and rounds = ceil(log2(min(len))) (:36-39).  Call right after
 * gm_sc_new. */
int gm_sc_set_herring(uint64_t handle, int on);
/* G1Module (G1 x F -> G1, module.rs:81-102): f is a vector of G1 points (affine records as in
 * gm_g1_bases_register), g a vector of Fr.  Each message is three device MSMs over the even/odd
 * halves (`M::ip` = msm_unchecked); fold is split_fold (time_prover.rs:72-76): f'[i] = f[2i] +
 * (r*twist) f[2i+1] on the device, g folds in Fr.  Messages / final f are normalised Jacobian. */
int gm_hg1_new(const void* f_bases, size_t base_stride, size_t nf, const uint64_t* g_mont, size_t ng, const uint64_t twist_mont[4],
               uint64_t* handle);
int gm_hg1_round(uint64_t handle, const uint64_t* challenge_or_null, uint64_t a_jac[18], uint64_t b_jac[18], int* has_msg);
int gm_hg1_fold(uint64_t handle, const uint64_t challenge_mont[4]);
int gm_hg1_rounds(uint64_t handle, size_t* tot_rounds, size_t* round);
int gm_hg1_final(uint64_t handle, uint64_t f0_jac[18], uint64_t g0_mont[4], int* has);
int gm_hg1_free(uint64_t handle);

/* ---- BLS12-381 G2: MSM and the herring G2Module prover ------------------------------------------- */
/* Replaces `P::G2::msm_unchecked` as Crs::commit_g2 / CrsStream::commit_g2 call it (src/herring/ipa.rs:107-118,185-189)
 * and `G2Module::ip` (src/herring/module.rs:114-124): the signed-digit bucket method over Fq2, same semantics as the G1
 * entry points of the same names (n = min(lengths); canonical scalars, a scalar >= 2^255 gives GM_EINVAL; results
 * normalised).  A null pointer or a bad stride (< 192, or not a multiple of 8) gives GM_EINVAL, an unknown handle GM_EHANDLE.
 * A call of more than 2^25 pairs is cut into 2^25-pair MSMs whose results are added on the host.
 * OUT OF SCOPE for G2: fixed-base tables, GLV, the streaming form, batches, sharding.  Pairings and the PModule prover are
 * in the next block, InnerProductProof in the one after it. */
int gm_g2_msm(const void* bases, size_t base_stride, const uint64_t* scalars, size_t n, uint64_t out_jac[36]);
int gm_g2_bases_register(const void* bases, size_t base_stride, size_t n, uint64_t* handle);
int gm_g2_bases_free(uint64_t handle);
int gm_g2_bases_len(uint64_t handle, size_t* n);
/* Copy registered bases back (192-byte stride). */
int gm_g2_bases_download(uint64_t handle, size_t offset, size_t n, void* out192);
/* bases[offset + i] (reversed: bases[offset - i]) against host scalars (canonical), an Fr vector (Montgomery) or device
 * scalars (mont = 0 canonical, 1 Montgomery) */
int gm_g2_msm_h(uint64_t handle, size_t offset, int reversed, const uint64_t* scalars, size_t n, uint64_t out_jac[36]);
int gm_g2_msm_v(uint64_t bases_handle, size_t offset, int reversed, uint64_t vec_handle, size_t voffset, size_t n, uint64_t out_jac[36]);
int gm_g2_msm_d(uint64_t bases_handle, size_t offset, int reversed, const void* d_scalars, int mont, size_t n, uint64_t out_jac[36]);
/* Sum of k Jacobian points on the host (no GPU needed, like gm_g1_sum); normalised. */
int gm_g2_sum(const uint64_t* points_jac, size_t k, uint64_t out_jac[36]);
/* G2Module (F x G2 -> G2, module.rs:104-125): f is a vector of Fr, g a vector of G2 points (affine records as in
 * gm_g2_bases_register).  Each message is three device MSMs over the even / odd halves; fold (time_prover.rs:83-88) is
 * f' = split_fold(f, r * twist) in Fr and g'[i] = g[2i] + r g[2i+1] on the device.  Messages / final g are normalised
 * Jacobian. */
int gm_hg2_new(const uint64_t* f_mont, size_t nf, const void* g_bases, size_t base_stride, size_t ng, const uint64_t twist_mont[4],
               uint64_t* handle);
int gm_hg2_round(uint64_t handle, const uint64_t* challenge_or_null, uint64_t a_jac[36], uint64_t b_jac[36], int* has_msg);
int gm_hg2_fold(uint64_t handle, const uint64_t challenge_mont[4]);
int gm_hg2_rounds(uint64_t handle, size_t* tot_rounds, size_t* round);
int gm_hg2_final(uint64_t handle, uint64_t f0_mont[4], uint64_t g0_jac[36], int* has);
int gm_hg2_free(uint64_t handle);

/* ---- pairings: multi-Miller loop, GT, the herring PModule prover ----------------------------------- */
/* Replaces `P::multi_pairing` behind PModule::ip (src/herring/module.rs:60-79), i.e. the messages of TimeProver<PModule>
 * (src/herring/ipa.rs:533-685) and the multi-pairings of Vrs::from (ipa.rs:215-247).  e(P, Q) is the reduced ate pairing as
 * ark-ec 0.4.2 states it for BLS12: Miller loop over |x| = 0xd201000000010000 (f <- f^2 l_{T,T}(P), and l_{T,Q}(P) on the set
 * bits below the top one), conjugation because x < 0, then f^((q^12 - 1) / r).  A pair with either point at infinity
 * contributes 1.  NOT PINNED: whether ark-ec's final_exponentiation carries the extra factor 3 of the
 * Hayashida-Hayasaka-Teruya hard part; this library raises to exactly (q^12 - 1) / r (README).
 * GT elements: 12 Fq values, 72 x u64 Montgomery limbs (the limb form of the coordinates of out_jac), in tower order
 * c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1 of Fq12 = Fq6[w] / (w^2 - v), Fq6 = Fq2[v] / (v^3 - (1 + u)),
 * Fq2 = Fq[u] / (u^2 + 1): the image of ark-ff `Fp12`.  GT is written multiplicatively; herring's "+" on GT is gm_gt_mul.
 * One lane per pair runs the Miller loop; the product is reduced on the device down to a handful of partials, the host
 * multiplies those and does the conjugation and ONE final exponentiation per call (a few ms, profiles/pairing.md).
 * Pairing calls share the MSM lock of the Threading paragraph above.
 * OUT OF SCOPE here: subgroup checks (points are taken as members of G1 / G2, as ark-ec's pairing takes them) -- a caller with
 * points it has no reason to trust runs them through the point-validation block (gm_g1_check / gm_g2_check) first; of herring's
 * InnerProductProof (next block) the pub(crate) `generic` and CrsStream. */
/* host records as gm_g1_bases_register / gm_g2_bases_register accept them (strides >= 96 / >= 192, multiples of 8; the
 * infinity flag at byte 96 / 192 when the stride has room); n = 0 gives 1 */
int gm_pairing_multi(const void* g1, size_t g1_stride, const void* g2, size_t g2_stride, size_t n, uint64_t out_gt[72]);
/* prod_i e(g1[off1 + step1 i], g2[off2 + step2 i]), i < n, over registered bases (steps >= 1: Vrs::from pairs
 * step_by(2) against take(size)).  A range outside the bases or a zero step gives GM_EINVAL, an unknown handle GM_EHANDLE. */
/* S independent products in one call: product s is over the pairs [offsets[s], offsets[s + 1]) (offsets[0] = 0, S + 1 entries), an
 * empty one is 1; out_gt: S x 72 limbs, each bit-identical to gm_pairing_multi on that product.  ONE segmented Miller launch, the
 * reduction levels of products longer than a block, ONE final-exponentiation launch and one wait, whatever S is.  The _h form
 * pairs (g1[off1 + t], g2[off2 + t]) of registered bases. */
int gm_pairing_multi_many(const void* g1, size_t g1_stride, const void* g2, size_t g2_stride, const size_t* offsets, size_t S, uint64_t* out_gt);
int gm_pairing_multi_many_h(uint64_t g1_handle, size_t off1, uint64_t g2_handle, size_t off2, const size_t* offsets, size_t S, uint64_t* out_gt);
int gm_pairing_multi_h(uint64_t g1_handle, size_t off1, size_t step1, uint64_t g2_handle, size_t off2, size_t step2, size_t n,
                       uint64_t out_gt[72]);
/* GT on the host (no GPU needed, like gm_g2_sum): a b, a^s for a canonical 256-bit integer s, 1 */
int gm_gt_mul(const uint64_t a[72], const uint64_t b[72], uint64_t out_gt[72]);
int gm_gt_pow(const uint64_t a[72], const uint64_t scalar_canonical[4], uint64_t out_gt[72]);
int gm_gt_one(uint64_t out_gt[72]);
/* A test and integration aid, not a protocol step: in^((q^12 - 1) / r) for any Fq12 element (no conjugation), the one
 * host function that holds the exponent.  No GPU needed. */
int gm_gt_final_exp(const uint64_t in[72], uint64_t out_gt[72]);
/* PModule (G1 x G2 -> GT, module.rs:60-79) under TimeProver (src/herring/time_prover.rs:55-138): f is a vector of G1
 * records, g a vector of G2 records.  a = ip(f_e, g_e); b = ip(f_e, g_o) + ip(f_o, g_e) is ONE Miller product over both
 * halves and ONE final exponentiation.  fold: f'[i] = f[2i] + (r twist) f[2i+1] in G1, g'[i] = g[2i] + r g[2i+1] in G2 (an odd
 * tail folds against the identity), twist <- twist^2.  rounds = ceil(log2(min(len f, len g))).  gm_hp_round folds by the
 * challenge first when one is given; the call that folds the last challenge answers has_msg = 0, and any round or fold
 * after it is GM_ESTATE.  gm_hp_final: f[0] (18 limbs) and g[0] (36 limbs), normalised Jacobian, once the rounds are done. */
int gm_hp_new(const void* f_g1, size_t g1_stride, size_t nf, const void* g_g2, size_t g2_stride, size_t ng, const uint64_t twist_mont[4],
              uint64_t* handle);
int gm_hp_round(uint64_t handle, const uint64_t* challenge_or_null, uint64_t a_gt[72], uint64_t b_gt[72], int* has_msg);
int gm_hp_fold(uint64_t handle, const uint64_t challenge_mont[4]);
int gm_hp_rounds(uint64_t handle, size_t* tot_rounds, size_t* round);
int gm_hp_final(uint64_t handle, uint64_t f0_jac[18], uint64_t g0_jac[36], int* has);
int gm_hp_free(uint64_t handle);

/* ---- GtModule: GT multi-exponentiation on the device and the herring GtModule prover (gemini_amd/csrc/pairing.hip) ------
 * GtModule (GT x Fr -> GT, src/herring/module.rs:49-58): p(a, b) = a^b in the multiplicative notation of this header,
 * ip = prod_i a_i^b_i.  One lane per element raises it by a fixed 2-bit window (no branch on exponent bits), the block
 * multiplies its 64 powers, the reduction levels of the pairing block and the host finish the product.  There is no final
 * exponentiation, no conjugation and no membership check: the entries take any 12 reduced Fq coefficients on trust and agree
 * bit for bit with the composition of gm_gt_pow / gm_gt_mul on every such input.  A launch is tens of milliseconds deep whatever
 * n is (profiles/gt_module.md gives the n from which it beats the host loop).  Calls share the MSM lock.
 * gm_gt_multi_pow: prod_i x_i^e_i for host elements and exponents that are 256-bit integers AS GIVEN (4 x u64, least
 * significant first, not reduced mod r), like gm_gt_pow; n = 0 gives 1.
 * gm_hgt_*: TimeProver<GtModule>: f is a vector of GT elements (nf x 72 limbs), g a vector of Fr (Montgomery).
 * a = prod_{i} f[2i]^g[2i]; b = prod f[2i]^g[2i+1] * prod f[2i+1]^g[2i] is ONE launch over both halves (a zip: the shorter
 * side ends a product).  fold: f'[i] = f[2i] * f[2i+1]^(r twist) (an odd tail is f[2i]), g'[i] = g[2i] + r g[2i+1], twist <- twist^2.
 * rounds = ceil(log2(min(nf, ng))).  gm_hgt_round folds by the challenge first when one is given; after the call that answered
 * has_msg = 0 further rounds answer has_msg = 0 and folds are applied, as for gm_hg1_* / gm_hg2_*.  gm_hgt_final: f[0] (72 limbs)
 * and g[0] (4 limbs) once the rounds are done.  A handle of another module is GM_EHANDLE. */
int gm_gt_multi_pow(const uint64_t* x /* n x 72 */, size_t n, const uint64_t* scalars_canonical /* n x 4 */, uint64_t out_gt[72]);
/* S independent products: out[s] = prod_{i in [offsets[s], offsets[s+1])} x_i^e_i; offsets[0] = 0, S + 1 entries, an empty
 * product is 1.  Each out[s] is bit for bit gm_gt_multi_pow on that range, on ANY 12 reduced Fq coefficients.  ONE
 * exponentiation launch (k_gt_multi_pow_seg: one lane per term, the block multiplies per product), the reduction levels of the
 * longest product, one wait, whatever S is.  S = 0 does nothing.  GM_EINVAL: descending offsets, offsets[0] != 0, null pointers with
 * terms to read, more than 2^20 terms.  Shares the MSM lock. */
int gm_gt_multi_pow_many(const uint64_t* x /* n x 72 */, const uint64_t* scalars_canonical /* n x 4 */, const size_t* offsets, size_t S, uint64_t* out_gt /* S x 72 */);
int gm_hgt_new(const uint64_t* f_gt /* nf x 72 */, size_t nf, const uint64_t* g_mont, size_t ng, const uint64_t twist_mont[4], uint64_t* handle);
int gm_hgt_round(uint64_t handle, const uint64_t* challenge_or_null, uint64_t a_gt[72], uint64_t b_gt[72], int* has_msg);
int gm_hgt_fold(uint64_t handle, const uint64_t challenge_mont[4]);
int gm_hgt_rounds(uint64_t handle, size_t* tot_rounds, size_t* round);
int gm_hgt_final(uint64_t handle, uint64_t f0_gt[72], uint64_t g0_mont[4], int* has);
int gm_hgt_free(uint64_t handle);

/* ---- herring: space prover over G1Module / G2Module (gemini_amd/csrc/herring.hip) ------------------------------------------
 * The streaming SpaceProver of src/herring/space_prover.rs:39-316 for the two modules whose p(point, scalar) = scalar * point
 * is linear in the point.  The point side is a run of a REGISTERED key, read where it lies and never written or copied: the
 * nf points bases[offset .. offset + nf) are the big-endian stream the reference consumes, stream item i = bases[offset + i],
 * so f_le[i] = bases[offset + nf - 1 - i].  After k folds the folded vectors are F[m] = sum_{u < 2^k} w_u f_le[m 2^k + u]
 * with w the tensor of the side's challenges (twisted on the Lhs; past the end of the stream f_le is zero, streams.rs:79-95),
 * and every sum of a message is ONE multi-scalar multiplication over the original points: a kernel (k_hsp_scalars) expands
 * the scalars, the MSMs are the engine's (with the fixed-base tables of a G1 key that has them).  Two MSM calls a message,
 * one more for final_foldings; no folded point vector exists until gm_hsp*_to_time.  The scalar side, 32 bytes an element,
 * is copied once (as the little-endian vector) and kept folded.
 *   gm_hsp1_new_borrow  G1Module: Lhs = points of a gm_g1_bases_* handle, Rhs = a gm_fr_vec_* vector holding the big-endian
 *                       stream.  Key and vector stay alive and unmodified until gm_hsp1_free
 *   gm_hsp1_new         the same from host records (as gm_hg1_new takes them) and a host stream: a key of the prover's own
 *   gm_hsp1_round       next_message: an optional fold, then (a, b); has_msg = 0 after log2(min(nf, ng)) messages (ark-std's
 *                       ceiling log, as gm_sp_new).  Pair j is (F[2j], F[2j+1]) against (G[2j], G[2j+1]), as many pairs as the
 *                       shorter folded side has, a missing odd element is zero:
 *                         a = sum_j t^(2j) p(F[2j], G[2j]),  b = sum_j t^(2j) (p(F[2j], G[2j+1]) + t p(F[2j+1], G[2j])),
 *                       t the current twist -- space_prover.rs:188-207 (twist_runner = t^(2 pairs) stepping by t^-2; on the
 *                       first pair it multiplies p, in the loop the Rhs: the same value).  The reference's own alignment
 *                       (:152-164) fails its assertion f_pairs == g_pairs when the folded lengths differ and the shorter one
 *                       is odd; everywhere else its pairs are these.  GM_ESTATE when folds and rounds are out of step.
 *   gm_hsp1_fold        Prover::fold: stores r (Rhs) and r t (Lhs), t <- t^2
 *   gm_hsp1_final       final_foldings: the FIRST item of each folded stream (:270-276), i.e. the block of the HIGHEST index
 *                       -- element 0 only when that side has folded down to one element, as both have for equal lengths
 *   gm_hsp1_to_time     TimeProver::from(&SpaceProver) (:279-316): an ordinary gm_hg1_* prover at the same round, twist and
 *                       tot_rounds; its f is the folded points in an allocation of its own (k out-of-place split-folds, the
 *                       first one reading the key), its g the folded scalars.  The space prover stays valid
 *   gm_hsp2_*           G2Module: Lhs = the Fr stream, Rhs = points of a gm_g2_bases_* handle; points are jac[36]
 * Outputs are normalised Jacobian, as gm_hg1_* / gm_hg2_* give them.  herring's TimeProver uses the twist when it folds only
 * (time_prover.rs:83-123), the SpaceProver also in its messages: the two agree at twist = 1 and nowhere else, in the reference
 * and here; a prover from to_time goes on as a TimeProver.  Null pointers or a bad stride: GM_EINVAL; nf = 0 or ng = 0:
 * GM_EINVAL; an unknown handle: GM_EHANDLE; rounds past the end and further folds as gm_hg1_round / gm_hg1_fold take them.
 * Not covered: PModule and GtModule (their p is no scalar multiple, so a message is no MSM), FModule under this twist
 * placement, the space prover inside gm_ipa_new, CrsStream. */
int gm_hsp1_new_borrow(uint64_t g1_bases_handle, size_t offset, size_t nf, uint64_t g_stream_vec, const uint64_t twist_mont[4], uint64_t* handle);
int gm_hsp1_new(const void* f_bases, size_t base_stride, size_t nf, const uint64_t* g_stream_mont, size_t ng, const uint64_t twist_mont[4],
                uint64_t* handle);
int gm_hsp1_round(uint64_t handle, const uint64_t* challenge_or_null, uint64_t a_jac[18], uint64_t b_jac[18], int* has_msg);
int gm_hsp1_fold(uint64_t handle, const uint64_t challenge_mont[4]);
int gm_hsp1_rounds(uint64_t handle, size_t* tot_rounds, size_t* round);
int gm_hsp1_final(uint64_t handle, uint64_t f0_jac[18], uint64_t g0_mont[4], int* has);
int gm_hsp1_to_time(uint64_t handle, uint64_t* hg1_handle);
int gm_hsp1_free(uint64_t handle);
int gm_hsp2_new_borrow(uint64_t f_stream_vec, uint64_t g2_bases_handle, size_t offset, size_t ng, const uint64_t twist_mont[4], uint64_t* handle);
int gm_hsp2_new(const uint64_t* f_stream_mont, size_t nf, const void* g_bases, size_t base_stride, size_t ng, const uint64_t twist_mont[4],
                uint64_t* handle);
int gm_hsp2_round(uint64_t handle, const uint64_t* challenge_or_null, uint64_t a_jac[36], uint64_t b_jac[36], int* has_msg);
int gm_hsp2_fold(uint64_t handle, const uint64_t challenge_mont[4]);
int gm_hsp2_rounds(uint64_t handle, size_t* tot_rounds, size_t* round);
int gm_hsp2_final(uint64_t handle, uint64_t f0_mont[4], uint64_t g0_jac[36], int* has);
int gm_hsp2_to_time(uint64_t handle, uint64_t* hg2_handle);
int gm_hsp2_free(uint64_t handle);
/* of a gm_hsp1_* or gm_hsp2_* prover so far: MSM calls, launches of k_hsp_scalars, point bytes the prover allocated (0 for the
 * borrow forms until to_time), scalar bytes it allocated */
int gm_debug_hsp_path(uint64_t handle, size_t out[4]);

/* ---- GT element by element on the device: final exponentiation, pairings, membership (gemini_amd/csrc/pairing.hip) ------
 * Vectors of GT elements: `BilinearModule::p` of PModule is P::pairing(a, b) (src/herring/module.rs:67), and the GtModule prover
 * above consumes 2^10 .. 2^14 of them.  One lane per element, 64 lanes per block; a launch is milliseconds deep whatever n is
 * (profiles/gt_device.md gives the n from which the device beats the host loop; calls that make ONE final exponentiation --
 * gm_pairing_multi*, gm_hp_round, gm_ipa_new, gm_ipa_verify, the verifiers -- stay on the host function; gm_ipa_new_many does
 * not: the 2 S products of a round of S proofs go through one k_gt_final_exp launch).  At most 2^20 elements
 * per call.  Calls share the MSM lock.
 * The final exponentiation splits (q^12 - 1) / r = (q^6 - 1)(q^2 + 1) h with, for x = -0xd201000000010000,
 *   h = (q^4 - q^2 + 1) / r = ((x - 1)^2 / 3)(x + q)(x^2 + q^2 - 1) + 1,
 * an exact identity: the value is gm_gt_final_exp's bit for bit on ANY 12 reduced Fq coefficients (0 gives 0), not its cube.
 * gm_gt_final_exp_many: out[i] = in[i]^((q^12 - 1) / r), no conjugation; n = 0 is a no-op.
 * gm_pairing_each / _h: out[i] = e(P_i, Q_i) -- ONE launch of Miller loops and ONE of final exponentiations, the Miller values
 * never leave the device.  Records, ranges and steps as for gm_pairing_multi / gm_pairing_multi_h; a pair with a point at
 * infinity gives 1.
 * gm_gt_check / gm_hgt_check / gm_ipa_check_gt: is every element a member of GT, the subgroup of order r of Fq12*?  Conventions of
 * the point-validation block below: *ok = 0 is written before anything else, a bad element is a result (GM_OK, *ok = 0, *first_bad
 * the smallest bad index; all good: *ok = 1, *first_bad = n), negative codes are for misuse only.  One status per element, the FIRST
 * test that fails:
 *   GM_PT_NONCANONICAL      a coefficient >= q (host input only)
 *   GM_PT_NOT_CYCLOTOMIC    f = 0 or f^(q^4) f != f^(q^2): not in the cyclotomic subgroup
 *   GM_PT_NOT_IN_SUBGROUP   f^q != f^x
 * The last two together give f^(x^4 - x^2 + 1) = f^r = 1 (r = x^4 - x^2 + 1 for BLS12).  1 is a member.
 * gm_hgt_check: the CURRENT f vector of a GtModule prover (folded as far as the rounds went), where it lies, no copy.
 * gm_ipa_check_gt: the 2 rounds message elements of a proof; a of round i is index 2 i, b is index 2 i + 1. */
int gm_gt_final_exp_many(const uint64_t* in /* n x 72 */, size_t n, uint64_t* out /* n x 72 */);
int gm_pairing_each(const void* g1, size_t g1_stride, const void* g2, size_t g2_stride, size_t n, uint64_t* out_gt /* n x 72 */);
int gm_pairing_each_h(uint64_t g1_handle, size_t off1, size_t step1, uint64_t g2_handle, size_t off2, size_t step2, size_t n, uint64_t* out_gt /* n x 72 */);
int gm_gt_check(const uint64_t* x /* n x 72 */, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok);
int gm_hgt_check(uint64_t handle, size_t* first_bad, int* ok);
int gm_ipa_check_gt(uint64_t proof, size_t* first_bad, int* ok);
/* A test aid: ONE device function of gt.cuh per lane over n x 72 limbs.  op 0: in^q, 1: in^(q^2), 2: 1 / in (0 gives 0),
 * 3: the cyclotomic squaring (in^2 on the cyclotomic subgroup ONLY), 4: in^|x| by cyclotomic squarings (likewise). */
int gm_debug_gt_op(int op, const uint64_t* in, size_t n, uint64_t* out);
/* Test aids for the Miller-loop half of gt.cuh / pairing.hip, same conventions: records of 72 limbs (12 Fq in ark-ff's Montgomery
 * form), one lane per record, 64 lanes per block, under the MSM lock; an unknown op or a missing operand is GM_EINVAL, n = 0 a no-op.
 * gm_debug_gt_op2: ONE tower function per lane.  b is read by the ops marked (b) and may be NULL for the others.
 *   0 fq12_mul(a, b) (b)   1 fq12_sqr(a)   2 fq12_conj(a)   3 fq12_mul_014(a, l0, l1, l4) (b: the line in its first three Fq2 slots)
 *   4 fq6_mul (b)   5 fq6_mul_v   6 fq6_mul_01(., b0, b1) (b: its first two Fq2 slots)   7 fq6_mul_1(., b1) (b: its first Fq2 slot)
 *     -- 4 .. 7 on both halves: out.c0 from a.c0 (and b.c0 for 4), out.c1 from a.c1 (and b.c1 for 4)
 *   8 fq2_mul_xi   9 fq2_mul12   10 fq2_mul_fq(., s) (b: s is the c0 of b's Fq2 slot)   11 fq2_conj   -- 8 .. 11 on each of the six Fq2 slots
 * gm_debug_miller_step: ONE step of the Miller loop per lane, op 0 miller_dbl_step, 1 miller_add_step.  in: T (X | Y | Z over Fq2,
 *   homogeneous projective, any Z), Q (x | y over Fq2), P (x | y, two field elements taken as they are, not checked against the
 *   curve) = 72 limbs; out: the new T (X | Y | Z) and the line (l0 | l1 | l4) = 72 limbs.  The addition step requires T != +-Q.
 * gm_debug_miller_each: out[i] = f_{|x|, Q_i}(P_i), the lane's Miller value as the loop leaves it: no conjugation, no product, no
 *   final exponentiation (1 when either point is the identity).  Records as for gm_pairing_each. */
int gm_debug_gt_op2(int op, const uint64_t* a /* n x 72 */, const uint64_t* b /* n x 72 or NULL */, size_t n, uint64_t* out /* n x 72 */);
int gm_debug_miller_step(int op, const uint64_t* in /* n x 72 */, size_t n, uint64_t* out /* n x 72 */);
int gm_debug_miller_each(const void* g1, size_t g1_stride, const void* g2, size_t g2_stride, size_t n, uint64_t* out /* n x 72 */);

/* ---- herring's inner-product argument: Crs, Vrs, InnerProductProof (gemini_amd/csrc/ipa.hip) -------------------------
 * src/herring/ipa.rs: InnerProductProof::new (:533-685) proves <a, b> = y together with comm_a = <a, crs.g1> and
 * comm_b = <b, crs.g2> in one batched sumcheck over GT; verify_transcript (:250-343) checks it against the Vrs of the CRS.
 * The three claims run on the FModule / G1Module / G2Module provers above.  The PModule provers the rounds add (two per round,
 * every live one asked for a message in every round) live in one device arena per group: per round ONE G1 and ONE G2 fold launch
 * and ONE segmented Miller launch (plus its reduction levels) whatever the number of live provers; the GT multi-exponentiation
 * of SumcheckMsg::ip runs on the host over the Miller values, so each half of a round message takes one final exponentiation
 * (profiles/herring_ipa.md).  Values are bit for bit those of the composition of gm_sc_* / gm_hg1_* / gm_hg2_* / gm_hp_* with
 * gm_gt_mul / gm_gt_pow (tests/test_gpu_ipa_stepwise.py).
 * Scalars are Montgomery limbs, points normalised Jacobian, GT elements 72 limbs as in the pairing block.  The reference defines no
 * wire format for this proof and none is claimed: the getters return the fields.
 * InnerProductProof::generic (:345-531) is in as the CRS-shaped batch, gm_ipa_new_batch below: K claims over the same CRS, every
 * twist one, one d.  OUT OF SCOPE: generic over witnesses whose point vectors are not the CRS, twists other than one, a different
 * d per claim, and CrsStream (its fold is a todo!() in the reference, ipa.rs:143-145). */
/* Crs over resident G1 and G2 arrays; records and strides as gm_g1_bases_register / gm_g2_bases_register take them */
int gm_crs_new(const void* g1, size_t g1_stride, size_t n1, const void* g2, size_t g2_stride, size_t n2, uint64_t* handle);
int gm_crs_free(uint64_t handle);
int gm_crs_len(uint64_t handle, size_t* n1, size_t* n2);
/* Crs::commit_g1 / commit_g2 (ipa.rs:179-189): the MSM of the first n points.  The reference asserts that the CRS is LONGER
 * than the scalars; n >= the CRS length gives GM_EINVAL. */
int gm_crs_commit_g1(uint64_t handle, const uint64_t* scalars_mont, size_t n, uint64_t out_jac[18]);
int gm_crs_commit_g2(uint64_t handle, const uint64_t* scalars_mont, size_t n, uint64_t out_jac[36]);
/* Vrs::from(&crs) (ipa.rs:215-247): levels = ceil(log2(n1)) - 1; level l holds, for size = 2^(l + 1), vk1 = (ip(g1 even, g2), ip(g1 odd, g2))
 * and vk2 = (ip(g1, g2 even), ip(g1, g2 odd)) over the first `size` pairs (zips end with the shorter side).  All 4 levels
 * Miller products are one segmented launch.  gm_vrs_get: even || odd, 144 limbs each. */
int gm_vrs_from_crs(uint64_t crs, uint64_t* vrs);
int gm_vrs_levels(uint64_t vrs, size_t* levels);
int gm_vrs_get(uint64_t vrs, size_t level, uint64_t vk1_even_odd[144], uint64_t vk2_even_odd[144]);
int gm_vrs_free(uint64_t vrs);
/* InnerProductProof::new(transcript, crs, (a, b)) for two vectors of d scalars; rounds = ceil(log2(d)).  The transcript (a
 * gm_transcript handle) absorbs and answers under the reference's labels in its order: batch-chal, prover_message, then per round
 * sumcheck-chal, batch-chal, sumcheck-round, and the last sumcheck-chal; it is the caller's to hand on.
 * GM_EINVAL for d < 2 (the reference's round loop underflows at rounds - 1) and for a CRS with fewer than max(d + 1, 2^rounds)
 * points in either group (commitments need d + 1, the truncation of ipa.rs:581 needs 2^rounds). */
int gm_ipa_new(uint64_t transcript, uint64_t crs, const uint64_t* a_mont, const uint64_t* b_mont, size_t d, uint64_t* proof);
/* S proofs against one CRS in one call: proofs[s] is what gm_ipa_new(transcripts[s], crs, a_s, b_s, d, .) returns, every field of
 * every proof byte for byte, and transcript s is left in the state the single call leaves it in.  One d per call (callers group
 * their work by length); a_mont / b_mont: S x d x 4 limbs.  S = 0 does nothing.
 * Refused with nothing absorbed by any transcript and no proof handle created: GM_EINVAL for what gm_ipa_new refuses (d < 2, a
 * CRS shorter than max(d + 1, 2^rounds) in either group), for null pointers with S > 0 and for a transcript handle named twice in
 * one call (two proofs cannot share a transcript); GM_EHANDLE for a stale transcript or CRS handle; GM_ENOMEM when the arena does
 * not fit the free device memory (the message has both numbers).  On a failure AFTER the first challenge (an allocation failure,
 * say) no proof handle is returned and the states of the transcripts are unspecified.
 * The S proofs run their rounds in lockstep.  Every proof draws its own challenges from its own transcript, in the single entry's
 * order and under its labels, and the device work of one round of ALL proofs is one launch group: one segmented split-fold per
 * group of the curve over every point vector of every proof (the PModule arena, the chopped CRS, the vectors of the G1Module and
 * G2Module provers; k_split_fold_seg reads each span's challenge through a table and tests its bits lane by lane, so one wave may
 * hold several proofs), the G1Module and G2Module messages of all proofs as segments of one short-linear-combination group per
 * group of the curve (one lane per term, the sums in two levels), one k_miller_seg launch over the 5 + 2 live segments of every
 * proof with the message points where the combinations left them, one k_gt_multi_pow_seg launch for the 2 S products of the round
 * messages on the Miller values, one k_gt_final_exp launch, one download of S x 144 limbs and one stream wait.  The number of
 * launches and waits does not depend on S.  The Fr side of a round -- the fold and the two inner products of the FModule prover,
 * whose vectors are also the scalars of the other two -- is 5 d / 2^j products per proof and runs on the host between the
 * challenges and the launches: the multi-prover sumcheck launch folds all its provers by ONE challenge, and here every proof has
 * its own.  Values are exact group and field elements normalised on the way out, so the bytes are the host path's.
 * Memory: one arena for all proofs, taken when the call starts and given back when it ends; its peak is
 * about S x (1480 x 2^rounds + 64 d) bytes plus tables of a few KiB per proof, checked against the free memory before the first
 * transcript is touched.  The MSM lock is taken per round, as gm_ipa_new takes it, so other threads' calls interleave.
 * gm_set_ipa_new_many_min: fewer proofs than this are made one by one by gm_ipa_new's own code; the bytes never depend on it.
 * Default 2, from profiles/ipa_new_many.md at d = 2^10: a lockstep call takes one proof's launch groups whatever S is, about a
 * second, so S = 1 loses, 1004.0 (991.0-1016.3) ms against 669.9 (669.0-674.5) ms for gm_ipa_new; S = 2 is the first measured row
 * where the slowest lockstep call beats the fastest loop, 1013.9 (1008.9-1017.3) ms against 1337.2 (1334.0-1339.7) ms; at S = 16
 * it is 1007.4 (1001.8-1011.2) ms against 10700.6 (10673.7-10723.8) ms.  gm_debug_ipa_new_many_path, for the last call on the context: counts[0] = proofs that
 * took the lockstep path, counts[1] = proofs that took the per-proof path, counts[2] = kernel launches the lockstep path enqueued,
 * counts[3] = stream waits it made, both counted where they are issued.  Scalars that are not reduced residues send the call to
 * the per-proof path, which takes limbs as they are. */
int gm_ipa_new_many(const uint64_t* transcripts /* S handles */, uint64_t crs, const uint64_t* a_mont /* S x d x 4 */, const uint64_t* b_mont /* S x d x 4 */, size_t d,
                    size_t S, uint64_t* proofs /* S handles out */);
int gm_set_ipa_new_many_min(size_t proofs);
int gm_debug_ipa_new_many_path(size_t counts[4]);
/* The fields of the proof.  messages: rounds x (a || b) = 144 limbs; challenges: rounds x 4; batch_challenges: (2 rounds + 1) x 4;
 * final_foldings (Sumcheck::final_foldings): 2 (rounds - 1) x 18 limbs (Lhs, G1) and x 36 limbs (Rhs, G2);
 * foldings_ff: lhs || rhs; foldings_fg1: (G1, Fr); foldings_fg2: (Fr, G2). */
int gm_ipa_rounds(uint64_t proof, size_t* rounds);
int gm_ipa_messages(uint64_t proof, uint64_t* messages);
int gm_ipa_challenges(uint64_t proof, uint64_t* challenges);
int gm_ipa_batch_challenges(uint64_t proof, uint64_t* batch_challenges);
int gm_ipa_final_foldings(uint64_t proof, uint64_t* lhs_jac, uint64_t* rhs_jac);
int gm_ipa_foldings_ff(uint64_t proof, uint64_t lhs_rhs_mont[8]);
int gm_ipa_foldings_fg1(uint64_t proof, uint64_t lhs_jac[18], uint64_t rhs_mont[4]);
int gm_ipa_foldings_fg2(uint64_t proof, uint64_t lhs_mont[4], uint64_t rhs_jac[36]);
int gm_ipa_free(uint64_t proof);
/* A measurement aid (tools/ipa_bench.py, profiles/herring_ipa.md): what gm_ipa_new spent on the HOST making this proof, in
 * milliseconds -- ms[0] the GT multi-exponentiations, ms[1] the final exponentiations -- and ms[2] the whole call.  Zeros for a
 * proof that came from gm_ipa_from_fields. */
int gm_ipa_host_times(uint64_t proof, double ms[3]);
/* A proof object from its fields, laid out as the getters return them (a verifier that did not run the prover);
 * foldings_fg1 = lhs_jac || rhs_mont (22 limbs), foldings_fg2 = lhs_mont || rhs_jac (40 limbs). */
int gm_ipa_from_fields(size_t rounds, const uint64_t* messages, const uint64_t* challenges, const uint64_t* batch_challenges, const uint64_t* final_lhs_jac,
                       const uint64_t* final_rhs_jac, const uint64_t foldings_ff[8], const uint64_t foldings_fg1[22], const uint64_t foldings_fg2[40],
                       uint64_t* proof);
/* InnerProductProof::verify_transcript(vrs, comm_a, comm_b, y): *ok = 1 iff the proof verifies.  Its pairings are one segmented
 * launch on the device.  A Vrs with fewer than rounds - 1 levels gives GM_EINVAL. */
int gm_ipa_verify(uint64_t proof, uint64_t vrs, const uint64_t comm_a_jac[18], const uint64_t comm_b_jac[36], const uint64_t y_mont[4], int* ok);
/* ok[s] = what gm_ipa_verify answers for proofs[s] with comm_a[s], comm_b[s], y[s] under `vrs`, for every s; fails as a whole
 * (negative code) exactly where one of the single calls, made in order, would.  Proofs may differ in their number of rounds.
 * verify_transcript is linear in the claim, so a proof of R rounds is ONE product in GT: 6 R - 4 powers of elements the verifier is
 * handed (the messages, the Vrs entries) times the final exponentiation of 2 R + 1 pairs whose exponents have moved onto the G1 side
 * (gemini_amd/csrc/ipa.hip states the terms, tests/ipa_flat_ref.py repeats them on integers).  All proofs share one launch group:
 * one gm_g1_lincomb_many group, one segmented Miller launch with a segment per proof, one final-exponentiation launch, one
 * k_gt_multi_pow_seg launch, the reduction levels of the longest proof; launches and waits do not depend on S.
 * Equal verdicts hold for EVERY input: the unrolling is valid for members only, so the entry first runs the GT membership test over
 * every message and the curve-and-subgroup tests over every G1 and G2 point the proofs and the caller supply (one launch each for
 * all proofs), and a proof with a failing element, or a scalar that is not reduced, gets its verdict from gm_ipa_verify's own path.
 * Only elements that passed reach the batched kernels, and none of those addresses memory by the value of an element.  The Vrs is
 * the library's own (gm_vrs_from_crs) and is trusted, as gm_ipa_verify trusts it.
 * gm_set_ipa_verify_many_min: fewer proofs than this run one by one; verdicts never depend on it.  Default 2, from
 * profiles/ipa_verify_many.md at d = 2^10: S = 1 is a tie, 69.6 (66.4-71.3) ms batched against 71.2 (69.3-72.5) ms single; S = 2 is the
 * first row where the batched call wins beyond the spread, 66.2 (66.1-67.3) ms against 140.5 (140.3-144.4) ms.  gm_debug_ipa_verify_many_path: counts[0] = proofs of the last call that took the batched path, counts[1] = proofs
 * that took the per-proof path.  gm_debug_ipa_stated_terms, a test aid: the canonical exponents (4 limbs each) the host states for
 * one proof, 6 R - 4 for the GT terms and 2 R + 4 for the pairing terms, in the order ipa.hip lists them; no kernel runs. */
int gm_ipa_verify_many(const uint64_t* proofs /* S handles */, uint64_t vrs, const uint64_t* comm_a_jac /* S x 18 */, const uint64_t* comm_b_jac /* S x 36 */,
                       const uint64_t* y_mont /* S x 4 */, size_t S, int* ok);
int gm_set_ipa_verify_many_min(size_t proofs);
int gm_debug_ipa_verify_many_path(size_t counts[2]);
int gm_debug_ipa_stated_terms(uint64_t proof, const uint64_t y_mont[4], uint64_t* gt_exponents, uint64_t* pairing_exponents);
/* ONE proof for K claims <a_i, b_i> = y_i, comm_a_i = <a_i, crs.g1>, comm_b_i = <b_i, crs.g2>: InnerProductProof::generic
 * (ipa.rs:345-531) with f_ip = [Witness(a_i, b_i, 1)], g1_ip = [Witness(crs.g1s, a_i, 1)], g2_ip = [Witness(b_i, crs.g2s, 1)] and
 * every vector of length d -- one batched sumcheck, one set of round messages and one set of CRS-fold provers, where S calls of
 * gm_ipa_new (or gm_ipa_new_many) make S proofs and S transcripts.  a_mont / b_mont: K x d x 4 limbs.
 * Labels and their order are gm_ipa_new's.  batch_challenges = powers(bc, 3 K) of the first batch challenge, then (c, c^2) per
 * round: 3 K + 2 (rounds - 1) entries, the weights in the order ff_0 .. ff_{K-1}, fg1_0 .., fg2_0 .., then the PModule provers in
 * push order.  The other fields keep their meaning; foldings_ff / _fg1 / _fg2 have K entries each.  K = 1 is gm_ipa_new byte for
 * byte and leaves the transcript in the same state.
 * No entry takes a twist.  The reference's Witness carries one, but its TimeProver uses it in `fold` and not in the message
 * (time_prover.rs:83-123): a proof with another twist cannot satisfy the verifier's a + b c + (claim - a) c^2.  `generic` unwraps a
 * message from every prover in every round, so all claims need the same number of rounds in any case; here they have the same d.
 * Only the scalar side grows with K.  The batch weights of the initial provers are fixed for the whole proof, and fold and message
 * of a module prover are linear in its scalars: the K G1Module provers over the CRS are ONE over sum_i bc^(K+i) a_i, the K
 * G2Module provers ONE over sum_i bc^(2K+i) b_i (both sums are formed on the device after the first challenge), their messages
 * enter the round message with weight one, the final scalar of G1Module prover i is the final lhs of FModule prover i and its final
 * point the folded CRS for every i.  The K FModule provers step together (gm_sc_round_begin_many: one launch per 22 provers); the
 * PModule arena, its two fold launches and the one segmented Miller launch of a round are gm_ipa_new's.  The numbers of split-fold
 * launches, MSM calls and Miller launches do not depend on K: gm_debug_ipa_new_batch_path gives them for the last call on the
 * context, counted where they are issued.  The MSM lock is taken per round.  tests/ipa_batch_ref.py states the literal 3 K-prover
 * form and this one on Python integers and holds them equal; tests/stepwise/ipa_generic.py composes the literal form from the
 * single provers of this library.
 * Refused before the first challenge, with nothing absorbed and no handle made: GM_EINVAL for K = 0, d < 2, a CRS shorter than
 * max(d + 1, 2^rounds) in either group and null pointers; GM_EHANDLE for a stale transcript or CRS; GM_ENOMEM (the message has both
 * numbers) when the arena plus 4 K d 32 bytes of scalars does not fit the free device memory.
 * gm_ipa_claims: K (1 for every proof made by another entry).  gm_ipa_foldings_batch: the layouts of the single-claim getters
 * repeated K times, ff K x 8, fg1 K x (lhs_jac || rhs_mont) = K x 22, fg2 K x (lhs_mont || rhs_jac) = K x 40.  gm_ipa_rounds,
 * _messages, _challenges, _final_foldings, _free and _check_gt work on a batch proof as they are; gm_ipa_batch_challenges writes
 * 3 K + 2 (rounds - 1) entries; gm_ipa_check visits the fg1 and fg2 points of claims 0 .. K - 1 where it visits those of the one
 * claim.  gm_ipa_verify, gm_ipa_verify_many, gm_ipa_foldings_ff / _fg1 / _fg2, gm_debug_ipa_stated_terms and gm_ipa_host_times
 * answer GM_EINVAL for a proof with K > 1 and are unchanged for K = 1.
 * gm_ipa_from_fields_batch: a proof object from its fields, laid out as the getters return them.
 * gm_ipa_verify_batch: verify_transcript (ipa.rs:250-343) with the constant 3 replaced by 3 K -- claim_0 = ip([E^y_i] ++
 * [e(comm_a_i, G2)] ++ [e(G1, comm_b_i)], batch_challenges[..3K]), the round loop reads batch_challenges[3K + 2i] and [3K + 2i + 1],
 * the final foldings are all ff, all fg1, all fg2, then the PModule pairs.  The reference has no verifier for `generic`; this
 * generalisation is the library's own.  The 4 K pairings of the initial claims are four: sum_i w_i comm_a_i, sum_i w_i comm_b_i,
 * sum_i w_i rhs_i P_i and sum_i w_i lhs_i Q_i go through the short linear combinations of both groups (complete addition: a hostile
 * proof can make terms equal or opposite), the FModule terms are one exponent of E each, and one segmented pairing launch follows;
 * launches do not depend on K.  *ok = 0 for a proof that fails.  GM_EINVAL when K differs from the proof's, for a Vrs with fewer
 * than rounds - 1 levels, and for a y, a folding scalar or a batch challenge that is not a reduced residue.  For K = 1 the verdict is
 * gm_ipa_verify's on every input.  Like gm_ipa_verify it takes points as members: gm_ipa_check tests the proof's. */
int gm_ipa_new_batch(uint64_t transcript, uint64_t crs, const uint64_t* a_mont /* K x d x 4 */, const uint64_t* b_mont /* K x d x 4 */, size_t d, size_t K,
                     uint64_t* proof);
int gm_ipa_claims(uint64_t proof, size_t* K);
int gm_ipa_foldings_batch(uint64_t proof, uint64_t* ff /* K x 8 */, uint64_t* fg1 /* K x 22 */, uint64_t* fg2 /* K x 40 */);
int gm_ipa_from_fields_batch(size_t rounds, size_t K, const uint64_t* messages, const uint64_t* challenges, const uint64_t* batch_challenges /* (3 K + 2 (rounds - 1)) x 4 */,
                             const uint64_t* final_lhs_jac, const uint64_t* final_rhs_jac, const uint64_t* ff /* K x 8 */, const uint64_t* fg1 /* K x 22 */,
                             const uint64_t* fg2 /* K x 40 */, uint64_t* proof);
int gm_ipa_verify_batch(uint64_t proof, uint64_t vrs, const uint64_t* comm_a_jac /* K x 18 */, const uint64_t* comm_b_jac /* K x 36 */, const uint64_t* y_mont /* K x 4 */,
                        size_t K, int* ok);
int gm_debug_ipa_new_batch_path(size_t counts[3]);

/* ---- Fiat-Shamir transcript (host; no GPU needed) ------------------------------------------------ */
/* merlin::Transcript::new(label) (merlin 3.0.0, Cargo.lock:606-608); the prover uses
 * Transcript::new(PROTOCOL_NAME) with PROTOCOL_NAME = b"GEMINI-v0" (src/lib.rs:74). */
int gm_transcript_new(const uint8_t* label, size_t len, uint64_t* handle);
int gm_transcript_free(uint64_t handle);
/* Transcript::append_message / challenge_bytes */
int gm_transcript_append_message(uint64_t handle, const uint8_t* label, size_t llen, const uint8_t* msg, size_t mlen);
int gm_transcript_challenge_bytes(uint64_t handle, const uint8_t* label, size_t llen, uint8_t* out, size_t n);
/* GeminiTranscript::append_serializable (src/transcript.rs:16-24) for `count` consecutive Fr
 * (an Fr, a RoundMsg(a, b), an [F; 2]) and for G1 elements (Commitment; with_len != 0 prefixes the
 * u64 length like Vec<Commitment>). */
int gm_transcript_append_fr(uint64_t handle, const uint8_t* label, size_t llen, const uint64_t* mont, size_t count);
int gm_transcript_append_g1(uint64_t handle, const uint8_t* label, size_t llen, const uint64_t* jac, size_t count, int with_len);
/* append_serializable for `count` consecutive GT elements (72 limbs each): a PairingOutput, or herring's
 * SumcheckMsg<PairingOutput> (a || b, count = 2).  576 bytes per element: the 12 Fq coefficients in tower order, 48 bytes
 * little-endian canonical each (ark-serialize of Fp12; a recalled convention like the other two, README). */
int gm_transcript_append_gt(uint64_t handle, const uint8_t* label, size_t llen, const uint64_t* gt, size_t count);
/* The ark-serialize framing gm_transcript_append_g1 uses, fixed by the curve crate of the build: 0 (default) =
 * ark-ec's short-Weierstrass default as in ark-test-curves' bls12_381 -- what the reference's examples and tests
 * link (x || y little-endian, flags in the top bits of the last byte); 1 = the zcash framing that ark-bls12-381
 * substitutes (big-endian, flags in the top bits of the first byte) -- what the reference's benches link.  A shim
 * may instead pass pre-serialised bytes through gm_transcript_append_message. */
int gm_transcript_set_g1_encoding(uint64_t handle, int encoding);
/* GeminiTranscript::get_challenge::<Fr> (src/transcript.rs:26-34) */
int gm_transcript_challenge_fr(uint64_t handle, const uint8_t* label, size_t llen, uint64_t out_mont[4]);
/* Sumcheck::prove round loop (src/subprotocols/sumcheck/proof.rs:36-66) over a gm_sc_* prover.
 * messages: cap_rounds x 8 u64 (a || b), challenges: cap_rounds x 4, final_foldings: f0 || g0. */
int gm_sumcheck_prove(uint64_t transcript, uint64_t prover, uint64_t* messages, uint64_t* challenges, size_t cap_rounds,
                      uint64_t final_foldings[8], size_t* rounds_out);

/* Sumcheck::prove_batch (src/subprotocols/sumcheck/proof.rs:69-122) over k gm_sc_* provers.
 * messages: cap_rounds x 8, challenges: cap_rounds x 4, final_foldings: k x 8 (lhs || rhs). */
int gm_sumcheck_prove_batch(uint64_t transcript, const uint64_t* provers, size_t k, uint64_t* messages, uint64_t* challenges,
                            size_t cap_rounds, uint64_t* final_foldings, size_t* rounds_out);

/* ---- the sub-protocols on their own (gemini_amd/csrc/subprotocols.cpp) ---------------------------------------------------
 * What the reference exports under subprotocols:: for a caller that composes an argument of its own: the same orchestration over the
 * entry points above as the whole-prover entries below run inline, the same transcript labels in the same order.
 *
 * TensorcheckProof::new_time(transcript, ck, base_polynomials, body_polynomials)        tensorcheck/mod.rs:190-275
 * A body = the polynomials that are batched with powers of the batch challenge (linear_combination pads to the longest, so unequal
 * lengths are fine) and the tensor challenges they are folded by; all challenges but the last fold (strip_last, :124-133), so a body
 * with one challenge contributes no folding.  nbodies = 0 or a body without polynomials: GM_EINVAL (the reference asserts).
 * The caller sets cap_folds, nbase and the three arrays; nfold = sum_b (nchallenges_b - 1) comes back, GM_EINVAL when it exceeds cap_folds. */
typedef struct gm_tensorcheck_body {
  const uint64_t* polys;           /* gm_fr_vec handles */
  size_t npolys;
  const uint64_t* challenges_mont; /* 4 limbs each */
  size_t nchallenges;
} gm_tensorcheck_body;
typedef struct gm_tensorcheck_proof {
  size_t nfold, cap_folds;
  uint64_t* fold_commitments;  /* caller-owned, cap_folds x 18 */
  uint64_t* fold_evaluations;  /* caller-owned, cap_folds x 8: at beta, -beta */
  uint64_t evaluation_proof[18];
  size_t nbase;
  uint64_t* base_evaluations;  /* caller-owned, nbase x 12: at beta^2, beta, -beta */
} gm_tensorcheck_proof;
int gm_tensorcheck_new_time(uint64_t transcript, uint64_t ck_bases, const uint64_t* base_polys, size_t nbase, const gm_tensorcheck_body* bodies,
                            size_t nbodies, gm_tensorcheck_proof* proof);
/* EntryProduct::new_time_batch (entryproduct/time_prover.rs:61-114); k = 1 is new_time (:117-147).
 * vs: k vectors; acc_vs_or_null: accumulated_product(monic(v_i)) where the caller already holds them, else they are built here.
 * Out: the commitments to the accumulated vectors (k x 18), the claimed sums chal * acc_v(chal) + product - chal^(len + 1) (k x 4),
 * the challenge, and k gm_sc_* provers Witness(acc_v, right_rotation(monic(v)), chal) for gm_sumcheck_prove_batch (gm_sc_free each).
 * The provers OWN their data: gm_sc_new_v semantics, one copy of both vectors (2 x (len + 1) x 32 bytes) per prover, so every input
 * vector may be freed as soon as this returns. */
int gm_entryproduct_new_time_batch(uint64_t transcript, uint64_t ck_bases, const uint64_t* vs, const uint64_t* acc_vs_or_null, size_t k,
                                   const uint64_t* claimed_products_mont, uint64_t* acc_v_commitments, uint64_t* claimed_sumchecks_mont,
                                   uint64_t chal_mont[4], uint64_t* provers);
/* plookup(subset, set, index, y, z, zeta) -> out = {lookup_set, lookup_subset, lookup_sorted}       plookup/time_prover.rs:89-112
 * Three NEW vectors the caller frees.  With zeta != 0 set and subset are hashed first and the subset is cut to min(|subset|, |index|) by
 * the zip (:11-21); with zeta = 0 neither.  ext_fre_or_0 = 0: the extended frequency of `index` is built on the device
 * (gm_idx_extend_frequency) and dropped; non-zero: the gm_idx handle of it that the caller keeps across proofs over the same index. */
int gm_plookup_new_time(uint64_t subset, uint64_t set, uint64_t index, uint64_t ext_fre_or_0, const uint64_t y_mont[4], const uint64_t z_mont[4],
                        const uint64_t zeta_mont[4], uint64_t out[3]);

/* ---- the whole prover in one call ---------------------------------------------------------------------
 * snark::Proof::new_time (src/snark/time_prover.rs:19-117) with its tensor check (tensorcheck/mod.rs:190-275) and KZG
 * openings (src/kzg/time.rs:81-159): the orchestration the reference compiles into the prover, compiled into the
 * library over the entry points above (gemini_amd/csrc/snark.cpp) -- one FFI call per proof for a shim that replaces
 * `Proof::new_time(&r1cs, &ck)`.  matrices = {A, B, C, A^T, B^T, C^T} (gm_spm_register handles; the transposes serve
 * the column sums of :63-81), z and w vector handles, ck_bases the registered powers_of_g, g1_encoding as in
 * gm_transcript_set_g1_encoding.  The caller provides messages[k] (cap_rounds x 8), fold_commitments (cap_rounds x 18)
 * and fold_evaluations (cap_rounds x 8); cap_rounds >= ceil(log2 |z|) + 1.  Everything is in the memory images of the
 * rest of this header (Montgomery Fr limbs, 18-limb Jacobian points).  spans: seconds of the reference's
 * start_timer! spans -- matrix products, commitment to w, first sumcheck, tensor/powers/hadamard/abc_tensored, second
 * sumcheck, tensor check, the whole prover.  Same bytes as the step-by-step drivers (tests/test_gpu_snark.py). */
typedef struct gm_snark_proof {
  uint64_t witness_commitment[18];
  uint64_t zc_alpha[4];
  size_t rounds[2];            /* messages of the first / second sumcheck */
  uint64_t* messages[2];       /* RoundMsg(a, b) = 8 limbs per round */
  uint64_t final_foldings[2][8];
  size_t nfold;                /* folded polynomials of the tensor check = rounds[1] - 1 */
  uint64_t* fold_commitments;
  uint64_t* fold_evaluations;  /* at beta and -beta */
  uint64_t evaluation_proof[18];
  uint64_t base_evaluations[12]; /* w at beta^2, beta, -beta */
  double spans[7];
} gm_snark_proof;
int gm_snark_new_time(const uint64_t matrices[6], uint64_t z, uint64_t w, uint64_t ck_bases, int g1_encoding, size_t cap_rounds,
                      gm_snark_proof* proof);

/* snark::Proof::new_elastic(r1cs_stream, ck_stream, max_msm_buffer) (src/snark/elastic_prover.rs:174-266) as one call.
 * matrices_t: gm_spm handles of A^T, B^T, C^T (the MatrixTensor streams, :233-238); z_stream, w_stream, za/zb/zc_stream:
 * the BIG-ENDIAN streams of R1csStream (`Reverse(..)`, src/snark/tests.rs:38-52) as device vectors; ck_bases: the key in time
 * order (its stream view Reverse(powers_of_g) is the reversed addressing of the MSMs), at least as long as every stream.
 * min_device_chunk = 1: the LITERAL elastic prover -- sumchecks on the space prover until fewer than SPACE_TIME_THRESHOLD = 22
 * rounds remain, flushes of max_msm_buffer pairs.  min_device_chunk > 1 (the mirror's default 2^26): everything is resident and
 * max_msm_buffer advisory -- every flush of a streaming MSM shorter than `min_device_chunk` pairs is merged, and the sumchecks
 * take the RESIDENT schedule: time provers on the little-endian vectors from the first round (the same field elements,
 * sumcheck/tests.rs:42-87; less memory than reversed stream copies; the elastic prover then costs what the time prover costs).
 * Same proof bytes as gm_snark_new_time on the same instance and key (src/snark/tests.rs:56).  spans[0] is 0: the matrix
 * products belong to the construction of the streams. */
int gm_snark_new_elastic(const uint64_t matrices_t[3], uint64_t z_stream, uint64_t w_stream, uint64_t za_stream, uint64_t zb_stream,
                         uint64_t zc_stream, uint64_t ck_bases, size_t max_msm_buffer, size_t min_device_chunk, int g1_encoding,
                         size_t cap_rounds, gm_snark_proof* proof);

/* psnark::Proof::new_time(&ck, &r1cs, &index) (src/psnark/time_prover.rs:69-384) as one call: the preprocessing prover's
 * orchestration -- three sumchecks (the third a 13-prover batch), three lookups with their nine entry products, ~25
 * commitments, the 22-polynomial tensor check -- compiled into the library (gemini_amd/csrc/psnark.cpp).
 * The instance record holds what depends on the R1CS only and is resident before the prover starts: the matrices, z and w,
 * the joint support of A, B, C walked column-major (src/misc.rs:269-366) as index vectors (gm_idx_register) and as field
 * vectors, the three value vectors over it, the extended-frequency index vectors of the row / column lookups
 * (plookup/time_prover.rs:66-79), the five index commitments of Proof::index (:49-64) and the bytes the reference absorbs as
 * b"ck" (the serialised G2 powers of the key).  All caller-owned arrays: messages (cap_rounds x 8 limbs each),
 * fold_commitments (cap_folds x 18), fold_evaluations (cap_folds x 8).  products: the full products of the nine lookup
 * vectors in the order r (set, subset, sorted), alpha (..), z (..).  Same bytes as gemini_amd/psnark.py (tests). */
typedef struct gm_psnark_instance {
  uint64_t a, b, c;                 /* gm_spm handles */
  uint64_t z, w;                    /* vectors */
  uint64_t row_index, col_index;    /* gm_idx handles over the joint support */
  size_t nnz;
  uint64_t row, col, val_a, val_b, val_c; /* vectors of length nnz */
  uint64_t ext_fre_row, ext_fre_col;      /* gm_idx handles */
  size_t ext_fre_row_len, ext_fre_col_len;
  const uint64_t* index_commitments;      /* 5 x 18 limbs */
  const uint8_t* ck_g2_bytes;
  size_t ck_g2_len;
} gm_psnark_instance;
typedef struct gm_psnark_proof {
  uint64_t witness_commitment[18];
  uint64_t zc_alpha[4];
  size_t rounds[3];
  uint64_t* messages[3];
  uint64_t final_foldings[2][8];        /* first and second sumcheck */
  uint64_t third_final_foldings[13][8]; /* one (lhs, rhs) per prover of the batch */
  uint64_t r_star_commitments[3][18];
  uint64_t z_star_commitment[18];
  uint64_t sorted_commitments[3][18];   /* r, alpha, z */
  uint64_t products[9][4];
  uint64_t acc_v_commitments[9][18];
  uint64_t claimed_sumchecks[9][4];
  uint64_t ralpha_star_acc_mu_evals[10][4];
  uint64_t ralpha_star_acc_mu_proof[18];
  uint64_t rstars_vals[2][4];
  size_t nfold;
  size_t cap_folds;
  uint64_t* fold_commitments;
  uint64_t* fold_evaluations;
  uint64_t evaluation_proof[18];
  uint64_t base_evaluations[22][12];
  double spans[12];
} gm_psnark_proof;
int gm_psnark_new_time(const gm_psnark_instance* instance, uint64_t ck_bases, int g1_encoding, size_t cap_rounds, gm_psnark_proof* proof);
/* psnark::Proof::new_elastic (src/psnark/elastic_prover.rs:60-634) over device-resident big-endian streams (reversed vectors: z,
 * the witness, A z, B z, C z -- R1csStream, src/circuit.rs), everything else of `instance` as for gm_psnark_new_time (its z / w
 * fields are not read).  Commitments and openings are the chunked stream MSMs of CommitterKeyStream (src/kzg/space.rs:95-285)
 * with the flush rule of gm_snark_new_elastic (max_msm_buffer [/ depth], never below min_device_chunk); with min_device_chunk = 1
 * the sumchecks run on space provers that become time provers below SPACE_TIME_THRESHOLD rounds (sumcheck/elastic_prover.rs:44-57),
 * otherwise on time provers from the first round (the resident schedule, as for gm_snark_new_elastic); the third one as
 * prove_batch over 13 of them.  Same bytes as gm_psnark_new_time (src/psnark/tests.rs:56-124); spans as there. */
int gm_psnark_new_elastic(const gm_psnark_instance* instance, uint64_t z_stream, uint64_t w_stream, uint64_t za_stream, uint64_t zb_stream,
                          uint64_t zc_stream, uint64_t ck_bases, size_t max_msm_buffer, size_t min_device_chunk, int g1_encoding, size_t cap_rounds,
                          gm_psnark_proof* proof);

/* Everything of `instance` that depends on the MATRICES only, built inside the library from the three registered matrices
 * (`sum_matrices` + `joint_matrices`, src/misc.rs:269-366: the union of the supports of A, B, C walked column-major, the three value
 * vectors with zeros where a matrix has no entry, the last of repeated (row, column) entries kept as BTreeMap::collect does; `row` /
 * `col` as field vectors; the extended frequencies of the two lookups, plookup/time_prover.rs:66-79) and left resident in HBM:
 * fills a, b, c, row_index, col_index, nnz, row, col, val_a, val_b, val_c, ext_fre_row, ext_fre_col and their lengths.  z, w,
 * index_commitments and the G2 bytes stay the caller's.  Setup like `Proof::index` (src/psnark/time_prover.rs:49-64), once per
 * circuit; gm_psnark_preprocess_free releases what it created (not the matrices). */
int gm_psnark_preprocess(uint64_t a, uint64_t b, uint64_t c, size_t num_variables, gm_psnark_instance* instance);
int gm_psnark_preprocess_free(gm_psnark_instance* instance);
/* psnark::Proof::index (src/psnark/time_prover.rs:49-64): commitments to row, col, val_a, val_b, val_c; out = 5 x 18 limbs */
int gm_psnark_index(const gm_psnark_instance* instance, uint64_t ck_bases, uint64_t* out_jac);

/* ---- the verifiers (gemini_amd/csrc/verifier.cpp) ---------------------------------------------------------------------------
 * What replaces `proof.verify(&r1cs, &vk)`: the reference's verifiers as host orchestration over the entry points above.  Every
 * group operation is a device MSM, every KZG check ONE multi-pairing of two pairs with one final exponentiation compared with 1
 * (so the check is indifferent to the factor-3 question of the pairing block), the O(n) part of the snark verifier is
 * gm_fr_powers / gm_fr_tensor / gm_fr_hadamard, three gm_spm_bilinear_pm and one gm_fr_eval_le.
 * Scalars are Montgomery limbs, G1 elements Jacobian (18 limbs, any representative).  *ok = 1: accepted, 0: REJECTED -- a rejected proof
 * is a result (return value GM_OK), negative codes are for misuse only.  The transcripts are replayed with the framings of the
 * transcript block (NOT PINNED, README).  OUT OF SCOPE: subgroup and on-curve checks of proof elements (the reference makes none) --
 * the verifiers do NOT call the point-validation block below; a caller that wants them checks the proof's points and the key itself
 * first (gm_snark_proof_check, gm_psnark_proof_check, gm_ipa_check, gm_vk_check, gm_crs_check, gm_g1_powers_check) --, a sharded verifier. */
/* kzg::VerifierKey (src/kzg/mod.rs:141-149): the first max_eval_points powers of g and max_eval_points + 1 powers of g2, records and
 * strides as gm_g1_bases_register / gm_g2_bases_register take them (copied to the host side of the library). */
int gm_vk_new(const void* g1, size_t g1_stride, size_t n1, const void* g2, size_t g2_stride, size_t n2, uint64_t* vk);
/* `VerifierKey::from(&CommitterKey::new(..))` from the trapdoor (src/kzg/time.rs:29-72), the setup aid that pairs with
 * gm_g1_srs_register: powers tau^i g, i < max_eval_points, and tau^i g2, i <= max_eval_points (tau canonical). */
int gm_vk_from_trapdoor(const uint64_t g1_affine[12], const uint64_t g2_affine[24], const uint64_t tau[4], size_t max_eval_points, uint64_t* vk);
int gm_vk_free(uint64_t vk);
int gm_vk_len(uint64_t vk, size_t* n1_or_null, size_t* n2_or_null);
/* serialize_uncompressed(&powers_of_g2) -- u64 length, 192 bytes per point, framing as gm_transcript_set_g1_encoding -- what psnark
 * absorbs as b"ck".  out = NULL: *len only. */
int gm_vk_g2_bytes(uint64_t vk, int encoding, uint8_t* out, size_t cap, size_t* len);
/* VerifierKey::verify (src/kzg/mod.rs:155-175): e(C - [evaluation] g, g2) == e(proof, [tau - alpha] g2) */
int gm_kzg_verify(uint64_t vk, const uint64_t commitment_jac[18], const uint64_t alpha_mont[4], const uint64_t evaluation_mont[4], const uint64_t proof_jac[18],
                  int* ok);
/* VerifierKey::verify_multi_points (:181-244): evaluations = nrows x npoints.  More points than the key holds powers for is GM_EINVAL;
 * ncommitments != nrows is a rejection (the reference's msm(..).unwrap() fails). */
int gm_kzg_verify_multi_points(uint64_t vk, const uint64_t* commitments_jac, size_t ncommitments, const uint64_t* eval_points_mont, size_t npoints,
                               const uint64_t* evaluations_mont, size_t nrows, const uint64_t proof_jac[18], const uint64_t open_chal_mont[4], int* ok);
/* Subclaim::new / new_batch (src/subprotocols/sumcheck/subclaim.rs:23-97) over a gm_transcript handle: messages = rounds x (a || b),
 * final_foldings = lhs || rhs (k of them for the batch); challenges_mont receives rounds x 4 limbs. */
int gm_sumcheck_subclaim(uint64_t transcript, const uint64_t* messages, size_t rounds, const uint64_t final_foldings[8], const uint64_t asserted_sum_mont[4],
                         uint64_t* challenges_mont, int* ok);
int gm_sumcheck_subclaim_batch(uint64_t transcript, const uint64_t* messages, size_t rounds, const uint64_t* final_foldings, const uint64_t* asserted_sums_mont, size_t k,
                               uint64_t* challenges_mont, int* ok);
/* TensorcheckProof::verify (src/subprotocols/tensorcheck/mod.rs:286-385): one claim per tensor-check instance -- the asserted results
 * that are batched with powers of the batch challenge, the folding randomness (two challenges or more, else GM_EINVAL) and the
 * evaluations of the instance's base combination at beta and -beta.  base_commitments_jac: ncommitments x 18. */
typedef struct gm_tensorcheck_claim {
  const uint64_t* asserted_res_mont;
  size_t nasserted;
  const uint64_t* fold_randomness_mont;
  size_t nrandomness;
  uint64_t direct_base_evals_mont[8];
} gm_tensorcheck_claim;
int gm_tensorcheck_verify(uint64_t transcript, uint64_t vk, const gm_tensorcheck_proof* proof, const uint64_t* base_commitments_jac, size_t ncommitments,
                          const gm_tensorcheck_claim* claims, size_t nclaims, const uint64_t eval_chal_mont[4], const uint64_t batch_challenge_mont[4], int* ok);
/* snark::Proof::verify (src/snark/verifier.rs:19-119).  matrices = {A, B, C} (gm_spm handles), x_vec the public input (a vector
 * handle; 0 = empty), the proof's arrays filled by a prover or from deserialised bytes (spans are not read). */
int gm_snark_verify(const uint64_t matrices[3], uint64_t x_vec, uint64_t vk, int g1_encoding, const gm_snark_proof* proof, int* ok);
/* psnark::Proof::verify (src/psnark/verifier.rs:88-565): O(log n) host field arithmetic around two KZG checks.  index_commitments:
 * 5 x 18 limbs (gm_psnark_index).  The key must hold max_eval_points >= 3. */
int gm_psnark_verify(uint64_t x_vec, size_t num_variables, size_t nnz, const uint64_t* index_commitments, uint64_t vk, int g1_encoding,
                     const gm_psnark_proof* proof, int* ok);

/* ---- Many proofs in one call.  Every *_many entry answers ok[s] = what the single entry answers for proof s, for every s, and fails
 * as a whole (a negative code) exactly where one of the single calls, made in order, would fail.  The KZG checks of all proofs are
 * STATED by the host part of each proof and run together: with Z(X) = sum_d z_d X^d the monic vanishing polynomial of a check's m points,
 *   e(L, g2) e(-proof, [Z(tau)] g2) = e(L, g2) prod_{d <= m} e((r - z_d) proof, [tau^d] g2),
 * m + 2 pairs against the key's G2 powers as they stand.  Every G1 point of every check comes out of one gm_g1_lincomb_many launch
 * group, then ONE segmented Miller launch, ONE final-exponentiation launch and one wait for all of them: the number of launches and
 * waits does not depend on S.  (Equal verdicts need proof elements ON the curve, as everything here does: the identity above is the
 * pairing's bilinearity.)  Below gm_set_verify_many_min stated checks (default 3, the measured break-even: profiles/verify_many.md) the checks run one by
 * one as the single entries run them: one host final exponentiation is cheaper than the device's launch.  Verdicts never depend on that knob. */
int gm_set_verify_many_min(size_t checks);
/* S checks of gm_kzg_verify_multi_points: check s has the commitments [commitment_offsets[s], commitment_offsets[s + 1]) of
 * commitments_jac (18 limbs each), the points [point_offsets[s], point_offsets[s + 1]) of eval_points_mont (at least one) and the
 * evaluation rows [row_offsets[s], row_offsets[s + 1]); evaluations_mont is the concatenation of the checks' row-major nrows x npoints
 * blocks.  proofs_jac: S x 18, open_chals_mont: S x 4.  A check whose commitment and row counts differ is ok[s] = 0. */
int gm_kzg_verify_multi_points_many(uint64_t vk, size_t S, const uint64_t* commitments_jac, const size_t* commitment_offsets, const uint64_t* eval_points_mont,
                                    const size_t* point_offsets, const uint64_t* evaluations_mont, const size_t* row_offsets, const uint64_t* proofs_jac,
                                    const uint64_t* open_chals_mont, int* ok);
/* S proofs under one set of matrices / one index and one key, each with its own public input x_vecs[s] (0 = empty).  The host part
 * of every proof runs as in the single entry; a proof it rejects states no further check. */
int gm_snark_verify_many(const uint64_t matrices[3], const uint64_t* x_vecs, uint64_t vk, int g1_encoding, const gm_snark_proof* proofs, size_t S, int* ok);
int gm_psnark_verify_many(const uint64_t* x_vecs, size_t num_variables, size_t nnz, const uint64_t* index_commitments, uint64_t vk, int g1_encoding,
                          const gm_psnark_proof* proofs, size_t S, int* ok);

/* ---- Multi-GPU: the collective layer (gemini_amd/csrc/dist.cpp) ------------------------------------------------------
 * One process per GPU (gm_init(LOCAL_RANK)).  The reference has no multi-device code: what shards is its own loop structure --
 * the MSM behind every commitment (src/kzg/time.rs:81-107: pairs split across ranks, 144-byte partial points all-gathered and
 * added on every rank), the rounds of Sumcheck::prove (src/subprotocols/sumcheck/proof.rs:36-66: 64 bytes per round), the
 * O(n) vector passes of snark::Proof::new_time (src/snark/time_prover.rs:19-117).  The ONE primitive is an all-gather; three
 * transports provide it:
 *   gm_dist_init_rccl  ncclAllGather over xGMI on a communicator of the library's own (librccl dlopen'ed at this call).
 *                      Rank 0 draws the id with gm_dist_rccl_unique_id and hands the 128 bytes to its peers out of band
 *                      (the launcher's store, a file, MPI ...).
 *   gm_dist_init_hook  the embedder's all-gather of host buffers: fn(ctx, send, bytes, recv) fills recv with the `world`
 *                      payloads in rank order and returns 0.
 *   gm_dist_init_shm   ranks of one node over a POSIX shared-memory segment `name` ("/something", the same on every rank;
 *                      slot_bytes = 0: 1 MiB per rank and call, longer payloads are cut): the payloads of this path are
 *                      host results of <= 1 KiB, which cross processes in ~1 us this way.  A name may be reused: rank 0 poisons
 *                      and removes a stale segment of that name before creating its own, a peer trusts a segment only after the
 *                      rank 0 OF THIS RUN has echoed the peer's fresh nonce, and every wait accepts a peer's call counter only at
 *                      the one or two values it can legitimately have (anything else is GM_ESTATE, never stale data).
 * Without any of them (or world = 1) an all-gather is a copy.  Collective calls must be made by every rank in the same order. */
typedef int (*gm_allgather_fn)(void* ctx, const void* send, size_t bytes, void* recv);
int gm_dist_init_hook(int rank, int world, gm_allgather_fn fn, void* ctx);
int gm_dist_rccl_unique_id(uint8_t out[128]);
int gm_dist_init_rccl(int rank, int world, const uint8_t unique_id[128]);
int gm_dist_init_shm(int rank, int world, const char* name, size_t slot_bytes);
/* RCCL on one node without any out-of-band channel: the ranks meet in the shared-memory segment `name`, which carries rank 0's
 * unique id to the peers, then build the communicator (gm_dist_rccl_unique_id + gm_dist_init_rccl in one call per rank).  The
 * segment stays open as the side channel of small host payloads (gm_dist_allgather_host_class).  A rank whose RCCL call FAILS
 * aborts the communicator (ncclCommAbort), so its peers return with an error instead of waiting inside the collective. */
int gm_dist_init_rccl_node(int rank, int world, const char* name);
int gm_dist_finalize(void);
/* A prover that fails on this rank OUTSIDE a collective would leave its peers waiting in their next all-gather until a timeout.  gm_dist_abort raises a
 * flag in the node's segment (every wait on it, and every bounded wait on an RCCL collective with the segment as side channel, returns GM_ESTATE at
 * once), aborts the communicator and poisons this rank's transport (transport 4) until it is initialised again.  The sharded provers call it on every
 * failure.  No effect with one rank; a hook transport has no channel for it. */
int gm_dist_abort(void);
/* transport: 0 none, 1 hook, 2 RCCL, 3 shm */
int gm_dist_info(int* rank, int* world, int* transport);
/* recv = world x bytes, rank order.  Host buffers (an MSM partial is finished by the host Horner; sumcheck messages and
 * evaluations are host values too). */
int gm_dist_allgather_host(const void* send, size_t bytes, void* recv);
/* The same with the payload's class.  It matters under gm_dist_init_rccl_node only, whose rendezvous segment stays open as a side
 * channel: FIELD values (sumcheck messages, evaluations, gathered tails; what gm_dist_allgather_host sends) cross it as a store and a
 * load, a few microseconds, where host staging around ncclAllGather costs H2D + collective + D2H + a stream wait; partial G1 POINTS
 * -- the all-gather behind every sharded commitment, north_star's "final RCCL reduce of partial G1 points over xGMI" -- go through
 * ncclAllGather (GM_DIST_G1_ROUTE=shm / GM_DIST_FIELD_ROUTE=rccl override either).  Measured: profiles/r5_collective_latency.txt. */
#define GM_DIST_CLASS_FIELD 0
#define GM_DIST_CLASS_G1 1
int gm_dist_allgather_host_class(const void* send, size_t bytes, void* recv, int payload_class);
/* out = the local vectors of ranks 0 .. world - 1 back to back (equal lengths; out needs capacity world x len and is
 * resized): device to device over RCCL, staged through the host on the other transports. */
int gm_dist_allgather_vec(uint64_t local_vec, uint64_t out_vec);
/* RE-BLOCKING: k device vectors, each block-distributed with equal blocks (rank p holds elements [p b, (p + 1) b), b = its local
 * length); out j (capacity >= new_block) = the elements [rank new_block, (rank + 1) new_block) of global vector j that exist, its
 * length set accordingly (0 past the end).  One group of ncclSend / ncclRecv over xGMI (every element crosses one link once); staged
 * through the host on the shm / hook transports; a copy with one rank.  What the n / g opening of gm_snark_new_time_sharded needs. */
int gm_dist_reblock_vecs(const uint64_t* local_vecs, size_t k, size_t new_block, const uint64_t* out_vecs);
/* collectives issued by this rank so far, the bytes they received and the wall time spent inside them */
int gm_dist_stats(uint64_t* calls, uint64_t* bytes, double* seconds, int reset_counters);
/* the same split by route: [0] copy (world 1), [1] hook, [2] RCCL with host staging, [3] RCCL device vectors, [4] shared memory */
int gm_dist_stats_routes(uint64_t calls[5], uint64_t bytes[5], double seconds[5]);
/* `iters` back-to-back all-gathers of `bytes` per rank -> microseconds per call.  route -1: wherever the class goes; 2 / 4: force RCCL
 * with host staging / the side segment (RCCL transport only).  Collective: every rank calls it with the same arguments. */
int gm_dist_bench(size_t bytes, int iters, int payload_class, int route, double* usec_per_call);
/* Patterns of 8 B .. 64 KiB through the active transport, checked on every rank.  With NO transport initialised it opens
 * a one-rank RCCL communicator for the test, so the binding runs on a single-GPU box too. */
int gm_dist_selftest(void);

/* A committer key SHARDED ELEMENT-CYCLICALLY over the ranks: power i of the key lives on rank i mod world, local index
 * i / world.  Every polynomial the provers commit to is a prefix of the key, foldings of length n/2, n/4, ... included, so
 * every rank gets len / world pairs (+-1) of EVERY commitment.  gm_g1_bases_set_cyclic marks a registered handle as such a
 * share (its length must be the rank's count); gm_g1_srs_register_cyclic generates the share on the device (base tau^rank g,
 * ratio tau^world: CommitterKey::new, src/kzg/time.rs:49-72, every rank its own powers).
 * gm_ck_*: CommitterKey::{commit, batch_commit} (:81-107) and the stream view of src/kzg/space.rs:95-125 against a key
 * handle that is either a whole key (then these are gm_g1_msm_v / gm_g1_msm_v_batch) or a cyclic share: strided gather of the
 * rank's scalars (the polynomials are replicated), local MSMs as one pipelined batch, ONE all-gather of k x 144 bytes, the EC
 * adds -- identical bytes on every rank.  offset / reversed address the GLOBAL key as in gm_g1_msm_v.
 * gm_snark_new_time, gm_snark_new_elastic, gm_psnark_new_time and gm_psnark_index commit through these: handed a cyclic
 * share they run on N GPUs with the MSMs sharded and the field arithmetic replicated. */
int gm_g1_bases_set_cyclic(uint64_t handle, size_t n_global, int rank, int world);
int gm_g1_srs_register_cyclic(const uint64_t base_affine[12], const uint64_t tau[4], size_t n_global, int rank, int world, uint64_t* handle);
int gm_ck_len(uint64_t ck, size_t* n_global);
int gm_ck_msm(uint64_t ck, size_t offset, int reversed, uint64_t vec, size_t voffset, size_t n, uint64_t out_jac[18]);
int gm_ck_msm_batch(uint64_t ck, const uint64_t* vecs, const size_t* ns, size_t k, uint64_t* out_jac);

/* Sumcheck::prove (src/subprotocols/sumcheck/proof.rs:36-66) with f and g BLOCK-sharded: this rank holds elements
 * [lo, lo + len) (lo even) of vectors of n_global elements.  Per round the rank's partial message (64 bytes) is all-gathered
 * and summed mod r; when the blocks get short (<= 2^10 elements) they are gathered once and every rank finishes the protocol
 * on the whole vectors.  Same outputs as gm_sumcheck_prove, on every rank. */
int gm_sumcheck_prove_sharded(uint64_t transcript, uint64_t f_block, uint64_t g_block, const uint64_t twist_mont[4], size_t lo, size_t n_global,
                              uint64_t* messages, uint64_t* challenges, size_t cap_rounds, uint64_t final_foldings[8], size_t* rounds);

/* snark::Proof::new_time (src/snark/time_prover.rs:19-117) with the FIELD ARITHMETIC sharded as well: rank r of g (powers of
 * two) holds elements [r m, (r + 1) m), m = n / g, of every vector of the prover.
 *   matrices     row blocks [r m, (r + 1) m) of A, B, C and of A^T, B^T, C^T (gm_spm handles, m rows each), either with GLOBAL
 *                column indices (m x n: any Matrix<F>, src/misc.rs:100-110, src/circuit.rs:43 -- then z is the WHOLE z on every
 *                rank, and tensor(rho) / powers(alpha) are computed whole on every rank: an O(n) pass at HBM speed is cheaper
 *                than n elements over xGMI) or with LOCAL ones (m x m: a block-diagonal instance such as dummy_r1cs,
 *                src/circuit.rs:349-365 -- then z is this rank's block and nothing of size n is ever touched)
 *   w_block      elements [r m, (r + 1) m) of w (the top rank's block is shorter: |w| = n - |x|)
 *   key          gm_snark_shard_key_new: this rank's slice of the key for every block-sharded level of the folding tree plus the
 *                replicated prefix for the gathered levels, ONE handle (offsets / counts: key_segments entries)
 * Sumchecks through gm_sumcheck_prove_sharded; foldings keep the top index bits, so level j stays block-sharded while its
 * blocks hold >= 2^tail_log elements and is gathered after that; commitments are one pipelined batch against the slices and
 * one all-gather; evaluations are block evaluations scaled on the host; the opening is sum_i eta_i commit(p_i div Z) with the
 * carry between blocks interpolated from the evaluations already gathered.  The proof is byte-identical to
 * gm_snark_new_time's on every rank (tests/test_gpu_dist_native.py: 1 / 2 / 4 / 8 ranks). */
typedef struct gm_snark_shard {
  uint64_t matrices[6];
  uint64_t z;
  uint64_t w_block;
  uint64_t key;
  const size_t* key_offsets;
  const size_t* key_counts;
  size_t key_segments;
  size_t n;
  size_t tail_log;
} gm_snark_shard;
int gm_snark_shard_key_new(const uint64_t base_affine[12], const uint64_t tau[4], size_t n, size_t tail_log, uint64_t* key, size_t offsets[64],
                           size_t counts[64], size_t* segments);
int gm_snark_new_time_sharded(const gm_snark_shard* shard, int g1_encoding, size_t cap_rounds, gm_snark_proof* proof);
/* snark::Proof::new_elastic (src/snark/elastic_prover.rs:174-266; BASELINE configs[3]: `snark -i 28`, elastic, 8 GPUs) over the same blocks: the
 * RESIDENT schedule of gm_snark_new_elastic (min_device_chunk > 1: time provers on the little-endian vectors, every stream MSM one call) over
 * blocks is the block-sharded time prover.  min_device_chunk = 1 (the literal schedule) is refused: it is single-GPU.  The DummyStreamer key of
 * examples/snark.rs:59-63 in slices: gm_snark_shard_key_new with tau = 1.  Same bytes as gm_snark_new_elastic / gm_snark_new_time. */
int gm_snark_new_elastic_sharded(const gm_snark_shard* shard, size_t max_msm_buffer, size_t min_device_chunk, int g1_encoding, size_t cap_rounds,
                                 gm_snark_proof* proof);

/* psnark::Proof::new_time (src/psnark/time_prover.rs:69-384; the resident schedule of new_elastic, elastic_prover.rs:60-634, is the same
 * entry) with the FIELD ARITHMETIC block-sharded as well -- BASELINE configs[4] on N GPUs.  One block size B for the proof
 * (gm_psnark_shard_block(longest vector, world); any world, no power-of-two requirement) and a level per family of vectors
 * (gm_psnark_shard_level, below): rank r of g holds the elements [r (B >> s), (r + 1) (B >> s)) THAT EXIST of a vector of level s (a block may
 * be partial or empty: handle 0 or a vector of length 0).
 *   a, b, c        the row blocks of A, B, C with GLOBAL column indices (gm_spm handles; 0 when no row falls into the block)
 *   z              the WHOLE z on every rank (the lookups of z* and the matrix products read arbitrary entries)
 *   w_block        this rank's block of w, w_len its whole length
 *   row_index .. ext_fre_col   this rank's blocks of the joint-matrix index vectors, field vectors and extended frequencies
 *                  (gm_psnark_instance, whole lengths nnz / ext_fre_*_len)
 *   key            gm_psnark_shard_key_new: this rank's slices of the key, key_len = powers of the whole key
 *   index_commitments   gm_psnark_index_sharded (Proof::index over the same blocks)
 * What crosses ranks: partial G1 points (144 B per commitment), 64 B per prover and sumcheck round (the 13 provers of the third
 * sumcheck in ONE all-gather per round), the products of the blocks of the nine lookup vectors (the carries of the suffix scans of
 * accumulated_product, entryproduct/time_prover.rs:34-45) and 32-byte halos (right_rotation, plookup_set read element i - 1),
 * evaluations, short gathered tails, the re-blocked level sums of the opening.  `lookup(v, index)` (plookup/time_prover.rs:5-8)
 * needs no exchange and no whole vector: tensor(rho) and powers(alpha) are functions of the index (gm_fr_tensor_gather / gm_fr_powers_gather).
 * The proof is byte-identical to gm_psnark_new_time's on every rank (tests/test_gpu_dist_native.py: 1 / 2 / 3 / 4 / 8 ranks). */
typedef struct gm_psnark_shard {
  uint64_t a, b, c;
  uint64_t z;
  uint64_t w_block;
  size_t w_len;
  uint64_t row_index, col_index;
  uint64_t row, col, val_a, val_b, val_c;
  uint64_t ext_fre_row, ext_fre_col;
  size_t ext_fre_row_len, ext_fre_col_len;
  size_t num_constraints, num_variables, nnz;
  size_t block;
  size_t tail_log;
  uint64_t key;
  const size_t* key_offsets;
  const size_t* key_counts;
  size_t key_segments;
  size_t key_len;
  const uint64_t* index_commitments; /* 5 x 18 limbs */
  const uint8_t* ck_g2_bytes;
  size_t ck_g2_len;
} gm_psnark_shard;
size_t gm_psnark_shard_block(size_t longest, int world);
/* LEVELS.  The prover's vectors come in several lengths (dummy_r1cs: ~n and ~2 n; a general instance: n, nnz ~ 6 n, n + nnz): with one block size
 * the short ones would sit on the lower ranks only.  A FAMILY of vectors whose longest member has `len` elements lives in blocks of
 * block >> level, level = the largest one (up to the number of folding levels that stay sharded) whose `world` blocks still hold it: every rank
 * holds ~1 / world of every vector.  The caller cuts its inputs accordingly:
 *   a, b, c          level(num_constraints)        w_block                     level(w_len)
 *   row_index, col_index, row, col, val_a, val_b, val_c                        level(nnz + 1)
 *   ext_fre_row      level(ext_fre_row_len + 2)    ext_fre_col                 level(ext_fre_col_len + 2)
 * (a vector of level s is cut at multiples of block >> s).  Combinations across levels are re-blocked inside the prover. */
size_t gm_psnark_shard_level(size_t len, size_t block, size_t tail_log, int world);
int gm_psnark_shard_key_new(const uint64_t base_affine[12], const uint64_t tau[4], size_t n_key, size_t block, size_t tail_log, uint64_t* key,
                            size_t offsets[64], size_t counts[64], size_t* segments);
int gm_psnark_index_sharded(const gm_psnark_shard* shard, uint64_t* out_jac);
/* The footprint contract (gm_psnark_footprint) of ONE RANK of the block-sharded prover: out = {vectors and prover buffers, MSM workspaces still
 * to grow, needed, what can be had}, bytes.  admit != 0: also make room (prefix tables are given back) or fail with GM_ENOMEM and the numbers --
 * what gm_psnark_new_time_sharded does before its first allocation.  z (whole on every rank) and the instance's blocks are the caller's. */
int gm_psnark_shard_footprint(uint64_t key, size_t num_constraints, size_t num_variables, size_t nnz, size_t block, int world, int admit, uint64_t out[4]);
int gm_psnark_new_time_sharded(const gm_psnark_shard* shard, int g1_encoding, size_t cap_rounds, gm_psnark_proof* proof);

/* ---- point validation: untrusted G1 / G2 points and an SRS (gemini_amd/csrc/points.hip) ------------------------------------------
 * What `deserialize_with_mode(.., Validate::Yes)` of ark-ec does per point, for whole keys on the device: canonical coordinates,
 * the curve equation (y^2 = x^3 + 4, on the twist y^2 = x^3 + 4 (1 + u)) and membership of the prime-order subgroup by the
 * endomorphism tests ark-bls12-381 uses -- G1: (beta x, y) == -[x^2] P, G2: psi(Q) == [x] Q, x = -0xd201000000010000 -- one lane
 * per point, no inversion (DESIGN.md "Point validation").  The identity is a valid point.  Nothing else in this header calls
 * these checks: registration, the pairings and the verifiers keep taking their points on trust.  A caller whose inputs it did not
 * make runs, BEFORE the verifier: gm_vk_check on the key, gm_snark_proof_check / gm_psnark_proof_check / gm_ipa_check on the proof,
 * gm_crs_check on a CRS (or builds key and CRS with the two _from_bytes decoders and validate != 0).
 * Every point gets ONE status, the FIRST check that fails in the order below.  A bad point is a result, not an error: the return
 * value is GM_OK, *ok = 0 and *first_bad the smallest bad index; when every point passes *ok = 1 and *first_bad = n.  status_or_null
 * (n bytes) and first_bad may be null.  Negative codes are for misuse only: null pointers, a bad stride, a range outside the handle
 * (GM_EINVAL), an unknown handle (GM_EHANDLE), no gm_init (GM_ENOTINIT).  Every entry writes *ok = 0 (and gm_g1_bases_from_bytes
 * *handle = 0) before it does anything else, gm_init or not, so a negative return value always comes with *ok = 0: the checks fail
 * closed.  Only status bytes and one word per block of points come back from the device.  The calls share the MSM lock of the Threading paragraph above. */
enum { GM_PT_OK = 0, GM_PT_BAD_ENCODING = 1, GM_PT_NONCANONICAL = 2, GM_PT_NOT_ON_CURVE = 3, GM_PT_NOT_IN_SUBGROUP = 4, GM_PT_NOT_CYCLOTOMIC = 5 /* gm_gt_check only */ };
/* Host records as gm_g1_bases_register / gm_g2_bases_register take them (ark-ff Montgomery limbs, stride >= 96 / 192 and a multiple
 * of 8, the infinity byte at 96 / 192 when the stride has room).  A record is the identity exactly when registration reads it as
 * the identity: the infinity byte is set (whatever the coordinates hold) or every coordinate limb is zero.  GM_PT_NONCANONICAL: the
 * limbs of a coordinate are >= q. */
int gm_g1_check(const void* points, size_t stride, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok);
int gm_g2_check(const void* points, size_t stride, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok);
/* The same over bases[offset .. offset + n) of a registered handle.  What is resident is canonical by construction, so these report
 * curve and subgroup failures only. */
int gm_g1_bases_check(uint64_t handle, size_t offset, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok);
int gm_g2_bases_check(uint64_t handle, size_t offset, size_t n, uint8_t* status_or_null, size_t* first_bad, int* ok);
/* n G1 points from bytes, decoded on the device: 48 (compressed != 0) or 96 bytes each, back to back, in the framing `encoding`
 * names (the values of gm_transcript_set_g1_encoding: 0 ark-ec little-endian with the flags in the last byte, 1 zcash big-endian
 * with the flags in the first).  A compressed point costs one square root, y = (x^3 + 4)^((q + 1) / 4), its sign chosen by the flag.
 * validate != 0 adds the curve equation (uncompressed points; a decompressed one is on the curve by construction) and the subgroup
 * test, in the same pass.  Acceptance is the canonical encoding only, point for point that of gemini_amd/wire.py's
 * g1_deserialize(strict = True): flag errors, a y-sign flag that does not match y, and infinity with non-zero coordinate bytes are
 * GM_PT_BAD_ENCODING; a coordinate >= q GM_PT_NONCANONICAL; an x whose x^3 + 4 is no square, or a point off the curve,
 * GM_PT_NOT_ON_CURVE.  On *ok = 0 nothing stays registered and *handle = 0; on success the handle is one of gm_g1_bases_register
 * (no tables are built here either; gm_g1_bases_precompute(handle, -1) asks for them). */
int gm_g1_bases_from_bytes(const uint8_t* bytes, size_t n, int compressed, int encoding, int validate, uint64_t* handle, uint8_t* status_or_null,
                           size_t* first_bad, int* ok);
/* The G2 twin: 96 (compressed) or 192 bytes per point; enc 0 x.c0 | x.c1 [| y.c0 | y.c1] little-endian, enc 1 x.c1 | x.c0 [| y.c1 |
 * y.c0] big-endian, flags as for G1 (the last byte is the top of the last c1, the first byte the top of x.c1).  y > -y is ark-ff's
 * order of Fq2: c1 first, then c0.  A compressed point costs one square root in Fq2 by the norm method -- two Fq exponentiations,
 * 1221 Fq products (DESIGN.md "Point validation").  Acceptance is point for point that of gemini_amd/g2.py's deserialize(strict =
 * True), statuses as above with x^3 + 4 (1 + u) in the place of x^3 + 4.  On success the handle is one of gm_g2_bases_register. */
int gm_g2_bases_from_bytes(const uint8_t* bytes, size_t n, int compressed, int encoding, int validate, uint64_t* handle, uint8_t* status_or_null,
                           size_t* first_bad, int* ok);
/* bases[offset .. offset + n) of a registered handle as n x {48 | 96} (G1) or n x {96 | 192} (G2) bytes in the canonical encoding
 * the decoders accept, back to back, no length prefix; encoded on the device (one Montgomery exit per coordinate and the y > -y
 * compare).  cap: the bytes `out` holds.  A range outside the handle, an unknown encoding or a cap too small is GM_EINVAL.  A cyclic
 * share (gm_g1_bases_set_cyclic) is encoded as it is held: the points of the share, not the key it was cut from. */
int gm_g1_bases_to_bytes(uint64_t handle, size_t offset, size_t n, int compressed, int encoding, uint8_t* out, size_t cap);
int gm_g2_bases_to_bytes(uint64_t handle, size_t offset, size_t n, int compressed, int encoding, uint8_t* out, size_t cap);
/* A gm_crs from two registered handles by device-to-device copy: a CRS decoded by the two _from_bytes calls never visits the host.
 * The handles stay the caller's (free them, or keep them).  *crs = 0 is written first. */
int gm_crs_from_bases(uint64_t g1_handle, uint64_t g2_handle, uint64_t* crs);
/* The curve and subgroup checks over both arrays of a CRS / over the host records of a verifier key (there also the canonical
 * test).  first_bad_g1 / first_bad_g2 (either may be null): the smallest bad index of each group, its length when all pass. */
int gm_crs_check(uint64_t crs, size_t* first_bad_g1, size_t* first_bad_g2, int* ok);
int gm_vk_check(uint64_t vk, size_t* first_bad_g1, size_t* first_bad_g2, int* ok);
/* Every group element the corresponding verifier reads from a proof: canonical limbs, on the curve, in the subgroup.  The elements
 * are Jacobian, any representative: they are normalised on the host (a handful of points; a coordinate >= q counts as
 * GM_PT_NONCANONICAL) and checked in ONE launch per group and call.  *first_bad (may be null) indexes the elements in this order,
 * and is their number when all pass:
 *   snark    witness_commitment, fold_commitments[0 .. nfold), evaluation_proof
 *   psnark   witness_commitment, r_star_commitments[3], z_star_commitment, sorted_commitments[3], acc_v_commitments[9],
 *            ralpha_star_acc_mu_proof, fold_commitments[0 .. nfold), evaluation_proof
 *   ipa      G1: foldings_fg1's lhs, the Lhs final foldings; then G2: foldings_fg2's rhs, the Rhs final foldings
 * The commitments a caller passes to gm_ipa_verify beside the proof are its own to check (gm_g1_check, gm_g2_check).  The GT
 * elements of an IPA proof (its messages) are not checked here: gm_ipa_check_gt (the GT block above) runs the membership test
 * over them. */
int gm_snark_proof_check(const gm_snark_proof* proof, size_t* first_bad, int* ok);
int gm_psnark_proof_check(const gm_psnark_proof* proof, size_t* first_bad, int* ok);
int gm_ipa_check(uint64_t proof, size_t* first_bad, int* ok);
/* A test aid: the Fq2 square root of the G2 decoder, one lane per element, on inputs no curve point produces.  a_mont: n x 12 limbs
 * (c0 | c1, ark-ff Montgomery); root_mont the same; is_square[i] = 1 when a_i is a square, and then root_i^2 = a_i. */
int gm_debug_fq2_sqrt(const uint64_t* a_mont, size_t n, uint64_t* root_mont, uint8_t* is_square);
/* A test aid: the device's field and group arithmetic element by element.  Each call applies ONE device function per lane, 64 lanes
 * per block, to records in DEVICE form -- 12 x u32 words holding a * 2^390 mod q, or 13 loose 30-bit limbs -- read and written as
 * they are: no conversion at the boundary, so the caller controls the exact limbs the function sees.  Operands must be valid inputs
 * of the function (canonical where it requires that; loose values normalised and below 2^386).  b is read only by the ops that take
 * a second operand and may be null otherwise.  n = 0 gives GM_OK; an unknown op or a null pointer with n > 0 GM_EINVAL.
 *   gm_debug_fq_op     n x 12 words.  0 fq_mul  1 fq_sqr  2 fq_add  3 fq_sub  4 fq_dbl  5 fq_neg_canonical  6 fqe_import  7 fqe_export
 *                      8 fq_inv (0 gives 0)      9 pt_raw_ge_q (0 / 1 in word 0, the others 0; the ONLY op that takes words >= q)
 *                      10 fq30_pack(fq30_unpack(a))
 *   gm_debug_fq30_op   n x 13 limbs.  0 fq30_mul_asm  1 fq30_sqr_asm  2 fq30_mul (plain C)  3 fq30_loose_to_canonical (12 words and a
 *                      zero)  4 fq30_canonical_tail alone (a < 2 q)
 *   gm_debug_fq2_op    n x 24 words (c0 | c1).  0 fq2_mul  1 fq2_sqr  2 fq2_add  3 fq2_sub  4 fq2_neg_canonical  5 fq2_inv (a != 0)
 *   gm_debug_g1_op     a: n x 48 words, X | Y | ZZ | ZZZ canonical.  0 xyzz_madd (b: n x 24, affine)  1 xyzz_add (b: n x 48)  2 xyzz_dbl
 *                      3 xyzz_dbl_affine (of the affine point in a's first 24 words)  4 g1_store_xyzz30 then g1_load_xyzz30.
 *                      out: n x 48, the four coordinates as the function leaves them.
 *   gm_debug_g2_op     the same over Fq2: a n x 96.  0 g2_madd (b: n x 48)  1 g2_add (b: n x 96)  2 g2_dbl  3 g2_dbl_affine
 *                      4 grp_to_affine<GrpG2> (x | y in the first 48 words of out, zeros behind)
 *   gm_debug_acc30_op  the two statements of the bucket accumulator, under the hot kernel's launch attributes.  acc: n x 52 loose
 *                      limbs (the 208-byte record; X < 7 q, Y, ZZ, ZZZ < 2 q; ZZ == 0 exactly marks the identity).  0 g1_madd30_asm:
 *                      other n x 24 canonical words (an affine point, not the identity), neg n x u32 (!= 0 adds the negative)
 *                      1 acc30_add: other n x 52 loose limbs, neg not read.  out: the 52 limbs the statement leaves;
 *                      out_canonical: acc30_to_canonical of them, n x 48 words. */
int gm_debug_fq_op(int op, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out);
int gm_debug_fq30_op(int op, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out);
int gm_debug_fq2_op(int op, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out);
int gm_debug_g1_op(int op, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out);
int gm_debug_g2_op(int op, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out);
int gm_debug_acc30_op(int op, const uint32_t* acc, const uint32_t* other, const uint32_t* neg, size_t n, uint32_t* out, uint32_t* out_canonical);
/* Do bases[offset .. offset + n) hold consecutive powers of ONE tau -- bases[offset + i + 1] = tau bases[offset + i] for i < n - 1 --,
 * the tau of (g2, tau g2)?  With A = sum rho^i P_i and B = sum rho^i P_{i+1} over i < n - 1 the test is e(A, tau g2) e(-B, g2) == 1:
 * gm_fr_powers, two gm_g1_msm_v and ONE two-pair multi-pairing.  g2_affine / tau_g2_affine: 192-byte records as
 * gm_g2_bases_register takes them.  A key that fails some pair passes with probability at most (n - 2) / r over rho, so rho MUST be
 * unpredictable to whoever made the key (draw it after the key is fixed); rho = 0 is GM_EINVAL, and so is a cyclic share
 * (gm_g1_bases_set_cyclic: it holds powers of tau^world; sharded checks are out of scope).  n <= 1 gives *ok = 1.  The points
 * are taken as members of their groups: run gm_g1_bases_check first. */
int gm_g1_powers_check(uint64_t handle, size_t offset, size_t n, const uint64_t g2_affine[24], const uint64_t tau_g2_affine[24],
                       const uint64_t rho_mont[4], int* ok);

/* ---- key generation: G2 fixed-base keys, points without a known logarithm, Crs operations (bases.hip, points.hip, ipa.hip) --------
 * The G2 twins of gm_g1_fixed_base_register / gm_g1_srs_register: out[i] = scalars[i] * base, resp. tau^i * base, i < n, through a
 * table of 32 windows x 256 affine multiples of the base, one lane per scalar (at most 32 mixed additions over Fq2), normalised by
 * Montgomery's trick over Fq2 -- one Fq inversion per 8 points -- in slabs of at most 2^22 points.  base_affine: a 192-byte record
 * as gm_g2_bases_register takes it.  Scalars are canonical, n x 4 u64 on the host; ANY 256-bit value is accepted and multiplies as
 * that integer.  A zero scalar gives the all-zero identity record, n = 0 an empty handle.  The handle is one of
 * gm_g2_bases_register.  No tables are kept: G2 MSMs have none. */
int gm_g2_fixed_base_register(const uint64_t base_affine[24], const uint64_t* scalars, size_t n, uint64_t* handle);
int gm_g2_srs_register(const uint64_t base_affine[24], const uint64_t tau[4], size_t n, uint64_t* handle);
/* Points whose discrete logarithms nobody knows (what Crs::new(rng, d) draws, ipa.rs:173-177): the first n of m CANDIDATES that
 * survive, in candidate order, cofactor-cleared and normalised on the device.
 *   G1 candidate   48 bytes, one little-endian integer: bits 0 .. 380 are x, bits 381 and 382 are ignored, bit 383 chooses the
 *                  larger of y and -y (ark-ff's order: y > q - y as integers)
 *   G2 candidate   96 bytes, x.c0 | x.c1, each 48 bytes masked the same way; the choice bit is bit 383 of the c1 half, the order
 *                  that of Fq2 (c1 first, c0 when c1 = 0)
 * A candidate is SKIPPED when, in this order, (1) a coordinate is >= q, (2) x^3 + 4 -- on the twist x^3 + 4 (1 + u) -- is no
 * square, (3) the cleared point is the identity.  Clearing: G1 P -> [1 - x] P = [|x|] P + P; G2 P -> [x^2 - x - 1] P +
 * [x - 1] psi(P) + psi^2([2] P) (Budroni-Pintore), x = -0xd201000000010000.  *found: the survivors among the candidates read;
 * *used: the index after the n-th survivor, or m -- a caller continues its stream from there.  Fewer than n survivors is a
 * result, not an error: GM_OK, *handle = 0, *found < n.  *handle = 0 is written first.  n = 0 gives an empty handle and
 * *used = 0.  The handles are those of gm_g1_bases_register (no tables built) / gm_g2_bases_register.
 * NO parity with an arkworks `rand` is claimed: the candidate format and the skip rules are this library's own. */
int gm_g1_bases_from_candidates(const uint8_t* cand, size_t m, size_t n, uint64_t* handle, size_t* used, size_t* found);
int gm_g2_bases_from_candidates(const uint8_t* cand, size_t m, size_t n, uint64_t* handle, size_t* used, size_t* found);
/* Crs::truncate / halve / fold (ipa.rs:191-212).  Each call returns a NEW handle (*out = 0 is written first); the input stays the
 * caller's.  truncate: the first min(len, 2^rounds) points of each group; halve: the first ceil(len / 2).  fold: g[i] = g[2i] +
 * c g[2i+1] in both groups (the split-fold kernels of the module provers), an odd tail folds against the identity; c in Montgomery
 * form.  The reference indexes g2s[2i] over g1s' length: n1 != n2 is GM_EINVAL. */
int gm_crs_truncate(uint64_t crs, size_t rounds, uint64_t* out);
int gm_crs_halve(uint64_t crs, uint64_t* out);
int gm_crs_fold(uint64_t crs, const uint64_t challenge_mont[4], uint64_t* out);
/* The inverse of gm_crs_from_bases: device copies of both arrays as a G1 and a G2 bases handle (either pointer may be null: that
 * half is not copied).  Both handles are written 0 first. */
int gm_crs_to_bases(uint64_t crs, uint64_t* g1_handle, uint64_t* g2_handle);

#ifdef __cplusplus
}
#endif
#endif /* GEMINI_HIP_H */
