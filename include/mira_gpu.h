/*
 * mira_gpu.h -- C ABI of libmira_gpu.so, the MI355X (gfx950) MSM + NTT engine that drops in
 * behind joshbeal/mira's commitment and FFT functions.
 *
 * The reference has no FFI for this path; these entry points are what a `cfg(feature="gpu")`
 * shim in the reference would bind (INTEGRATION.md shows the Rust side).  Each one cites the
 * reference interface it replaces (paths relative to the reference repository root).
 *
 * Data layout (the in-memory representation of halo2curves types, passed by pointer cast):
 *   field element  = 4 x uint64_t little-endian limbs, Montgomery form, R = 2^256   (32 bytes)
 *   affine point   = x || y                                                        (64 bytes)
 *   identity point = all-zero bytes (src/poseidon/poseidon_hash.rs:137-140)
 *   curve ids      : MIRA_CURVE_BN256 (G1, y^2 = x^3 + 3 over Fq, scalars Fr)
 *                    MIRA_CURVE_GRUMPKIN (y^2 = x^3 - 17 over Fr, scalars Fq)
 *
 * Ownership: the caller owns every buffer; the library borrows it for the duration of a call.
 * Registered bases are copied into a library-owned device buffer; the caller's copy is never
 * retained.  Errors: every function returns MIRA_OK (0) or a negative MIRA_E_* code and
 * never throws or aborts across the ABI; mira_last_error() describes the last failure on the
 * calling thread.  Threading: all entry points are re-entrant (one process-wide lock).
 * There is no CPU fallback: without a usable gfx950 device every compute call fails with
 * MIRA_E_NO_DEVICE.
 */
#ifndef MIRA_GPU_H
#define MIRA_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIRA_CURVE_BN256 0
#define MIRA_CURVE_GRUMPKIN 1

#define MIRA_OK 0
#define MIRA_E_NO_DEVICE (-1)     /* no HIP device / HIP runtime error */
#define MIRA_E_BAD_ARG (-2)       /* null pointer, unknown curve or handle, size out of range */
#define MIRA_E_TOO_LONG (-3)      /* scalars longer than the registered key: Error::TooLongInput */
#define MIRA_E_ALLOC (-4)         /* device allocation failed */
#define MIRA_E_UNSUPPORTED (-5)   /* size not supported by this build */
#define MIRA_E_INVALID_POINT (-6) /* a base is not on the curve */
#define MIRA_E_IO (-7)            /* key file missing, unreadable or shorter than 2^k points */
#define MIRA_E_JIT_UNAVAILABLE (-8) /* mira_graph_specialize: no run-time compiler on this machine (no libhiprtc.so); the graphs stay interpreted */
#define MIRA_E_JIT_FAILED (-9)    /* mira_graph_specialize: the compiler or the module loader failed (mira_last_error has its log); the graphs stay interpreted */

/* Largest number of windows any MSM configuration uses; sizes mira_msm_partial buffers. */
#define MIRA_MAX_WINDOWS 64
/* One partial = W XYZZ points of 16 u64 each (X, Y, ZZ, ZZZ), W <= MIRA_MAX_WINDOWS. */
#define MIRA_PARTIAL_U64 (MIRA_MAX_WINDOWS * 16)

/* ---- device / stream ------------------------------------------------------------------- */
int mira_device_count(void);
/* Bind the library to a HIP device (default 0) -- one process per GPU. */
int mira_init(int device);
/* Run all work on the caller's hipStream_t (e.g. torch's current stream); NULL = own stream. */
int mira_set_stream(void *hip_stream);
const char *mira_last_error(void);

/* ---- MSM: CommitmentKey::commit (src/commitment.rs:78-87) ------------------------------
 * register = upload the key once (`CommitmentKey { ck: Box<[C]> }`, src/commitment.rs:26-29;
 * it is immutable and outlives every fold step, src/ivc/public_params.rs:50).               */
int mira_msm_register_bases(int curve, const uint64_t *bases /* n * 8 limbs */, size_t n, uint64_t *handle_out);
/* Same, for bases already in device memory.  Either way the library keeps its own resident copy
 * in the engine's layout, so the caller's buffer is free again when the call returns. */
int mira_msm_register_bases_device(int curve, const void *d_bases, size_t n, uint64_t *handle_out);
int mira_msm_unregister(uint64_t handle);
/* Optional, once per key: build the fixed-base window tables 2^(20 w) * P_i, w < 13, in HBM
 * (13 x the key size: 3.3 GiB at 2^22 points).  Later MSMs of >= 2^18 pairs on this handle then use
 * one shared set of 2^19 buckets and 13 instead of 16 additions per pair.  Results are unchanged
 * (bit-identical); mira_msm_partial_device then reports window_bits = 0, num_windows = 64 (64
 * partial sums to be added).  MIRA_E_ALLOC if the tables do not fit. */
int mira_msm_precompute(uint64_t handle);
/* Same with the window width named: 20 (as above), 22 (12 tables, 2^21 buckets, 12 additions per
 * pair: for commits of 2^24 pairs and more) -- one of the two per key -- or any of 8 .. 16: a SHARED-BUCKET
 * set of W = ceil(256 / c) tables 2^(c w) * P_i (W x the key size: 16 bits = 1.9 GB, 12 bits = 2.6 GB for the
 * 1.8 M-point key of a k = 17 fold step).  All W windows of a commit then share ONE set of 2^(c-1) buckets:
 * W additions per pair, the fix-up and bucket reduction of one window instead of W, and no Horner
 * epilogue on the host -- the latency-bound part of the small commits of a fold step.  Several shared
 * widths may be built beside each other (and beside the wide tables): every commit of >= 2^12 pairs
 * picks the set that is fastest for its length (narrow for 2^17 pairs, 16 bits for 2^21) and -- from the second commit of
 * a shape on -- for the bit lengths of its scalars (a witness vector of mostly zeros is served like the short dense one it amounts to), commits of
 * >= 2^18 pairs the wide tables when the key has them.  mira_msm_partial_device reports window_bits = 0,
 * num_windows = 16; a rank of a sharded MSM takes the wide tables if
 * present, else the widest shared set, whatever its chunk length.  Results are bit-identical whichever
 * set serves a commit.  Building a width twice is a no-op.
 * window_bits = MIRA_TABLE_GLV: not a table but the ENDOMORPHISM COPY of the key, [P_0, phi(P_0), P_1, phi(P_1), ...] with
 * phi(x, y) = (beta x, y) (2 x the key's memory).  Both curves have j = 0, so phi(P) = lambda P for a cube root of unity
 * lambda of the scalar field: a single commit through the per-window path then splits every scalar into two 128-bit halves
 * (k = k1 + k2 lambda, k P = k1 P + k2 phi(P)) -- the same bucket additions over half the windows: half the bucket reduction,
 * half the chain of doublings on the host.  The same points bit for bit; mira_msm_last_plan reports ceil(129 / c) windows.
 * Single commits and batches through the per-window path use it; commits served by a table set and ranks of a sharded MSM
 * (whose partials must have one shape on every rank) do not.  Since round 4 the library builds the copy by itself for keys of
 * up to 2^26 points the first time a commit of at most 2^21 pairs can use it (MIRA_TUNE_GLV_AUTO_MAX_LOG; an allocation
 * failure just leaves the key without one): the call is only needed for longer keys or to pay the cost up front. */
#define MIRA_TABLE_GLV 2
int mira_msm_precompute_ex(uint64_t handle, int32_t window_bits);
/* Validate every registered base against the curve equation on the GPU, as
 * load_or_setup_cache does with is_on_curve (src/commitment.rs:145-154). */
int mira_msm_check_bases(uint64_t handle);
/* The commitment-key cache file straight into HBM: CommitmentKey::load_from_file (src/commitment.rs:110-127)
 * and, with validate != 0, the is_on_curve pass of load_or_setup_cache (:145-154) -- the raw in-memory
 * `[C]` dump save_to_file writes (:96-101), 2^k points of 64 bytes.  The file is read in 64 MiB chunks
 * by several threads into two pinned buffers; chunk i + 1 is read and copied while chunk i is converted to
 * the resident layout and checked on the GPU.  A file shorter than 2^k points -> MIRA_E_IO ("failed to fill
 * whole buffer", read_exact); a point off the curve -> MIRA_E_INVALID_POINT ("Wrong file in cache, some
 * ptr out of curve"), no handle.  mira_msm_save_bases_file writes that file from a registered key. */
int mira_msm_register_bases_file(int curve, const char *path, uint32_t k, int validate, uint64_t *handle_out);
int mira_msm_save_bases_file(uint64_t handle, const char *path);

/* out_affine = sum_i scalars[i] * bases[i], i < n <= registered length (the key's PREFIX is
 * used, src/commitment.rs:80).  n > registered length -> MIRA_E_TOO_LONG (src/commitment.rs:21-24,
 * 81-86).  Replaces best_multiexp(v, &ck[..v.len()]).to_affine().                            */
int mira_msm(uint64_t handle, const uint64_t *scalars /* n * 4 limbs */, size_t n, uint64_t out_affine[8]);
int mira_msm_device(uint64_t handle, const void *d_scalars, size_t n, uint64_t out_affine[8]);

/* `count` commitments over the same key in one submission -- the cross-term commits of one
 * fold step (`cross_terms.iter().map(|v| ck.commit(v))`, src/nifs/vanilla/mod.rs:124-127) are
 * count vectors of equal length n.  Each result is bit-identical to a separate mira_msm call.
 * scalars[b] = host pointer of vector b; device form: vector b starts at element b * stride_elems.
 * out_affine = count * 8 limbs. */
int mira_msm_batch(uint64_t handle, const uint64_t *const *scalars, size_t n, size_t count, uint64_t *out_affine);
int mira_msm_batch_device(uint64_t handle, const void *d_scalars, size_t n, size_t count, size_t stride_elems, uint64_t *out_affine);

/* Point-chunk sharding across GPUs (one process per GPU): each rank runs mira_msm_partial on
 * its chunk, the ranks all-gather the MIRA_PARTIAL_U64 words, and every rank combines.
 * `first` = index of the chunk's first base inside the registered key.  Every rank must make the
 * same choices: the same window width -- *window_bits on entry (4..20), or, if that is 0, the
 * mira_msm_set_window_bits value, or 16: a partial's width never depends on the chunk length,
 * which differs between ranks -- and either all or none with mira_msm_precompute'd keys (a handle
 * with tables answers with table-mode partials here whatever its chunk length, unless a width is
 * requested).  On return *window_bits / *num_windows describe the partial (0 / 64 for tables). */
int mira_msm_partial_device(uint64_t handle, size_t first, const void *d_scalars, size_t n,
                            uint64_t out_partial[MIRA_PARTIAL_U64], int32_t *window_bits, int32_t *num_windows);
int mira_msm_combine(int curve, const uint64_t *partials /* nparts * MIRA_PARTIAL_U64 */, size_t nparts,
                     int32_t window_bits, int32_t num_windows, uint64_t out_affine[8]);
/* Same, with the partial left in DEVICE memory (d_out_partial: MIRA_PARTIAL_U64 * 8 bytes, e.g. a tensor an
 * RCCL all-gather reads): nothing crosses PCIe before the exchange.  Words beyond the partial's windows are zero. */
int mira_msm_partial_to_device(uint64_t handle, size_t first, const void *d_scalars, size_t n,
                               void *d_out_partial, int32_t *window_bits, int32_t *num_windows);
/* Window width c (4..20) of every later commit over THIS key (CommitmentKey::commit, src/commitment.rs:78-87); 0 = let
 * the planner choose from n and the scalar statistics.  Per handle, so two caller threads working on two keys never see each
 * other's choice.  Widths of 17 to 20 bits commit on the plain path (never the GLV split, no table set) and need
 * W * 2^(c-1) * 144 bytes of bucket workspace: 1 GB at c = 20 (13 windows of 2^19 buckets). */
int mira_msm_set_handle_window_bits(uint64_t handle, int32_t c);
/* The widest window cmax (16..20) the planner and the width trials may pick for the commits of THIS key
 * (CommitmentKey::commit, src/commitment.rs:78-87).  16, the default, changes nothing; 17..20 let the planner take a wide width
 * on the plain path where its measured table puts it at least 2 % ahead (large commits: fewer windows, fewer additions per
 * pair, W * 2^(c-1) * 144 bytes of bucket workspace).  mira_msm_plan_window_bits does not look at it. */
int mira_msm_set_handle_max_window_bits(uint64_t handle, int32_t cmax);
/* Process-wide default width (4..16) for keys without one of their own (tests, benchmarks; 0 = planner).  A process
 * whose threads want different widths uses the per-handle call above.  All ranks of a sharded MSM must use the
 * same c.  Wider windows cost W * 2^(c-1) * 144 bytes of bucket workspace per commit: they are a decision about one key
 * (mira_msm_set_handle_window_bits, mira_msm_set_handle_max_window_bits), not the process. */
int mira_msm_set_window_bits(int32_t c);
/* The width the planner picks for a commit of n uniform scalars when it has no statistics of the data (a pure
 * function of n: every rank of a sharded MSM derives the same width from the same global length). */
int mira_msm_plan_window_bits(size_t n, int32_t *window_bits);
/* Diagnostics: the window width and count the planner used for the most recent commit of this
 * process (0 / the number of partial sums in fixed-base table mode). */
int mira_msm_last_plan(int32_t *window_bits, int32_t *num_windows);
/* ... and the width of the table set that commit went through (8 .. 16 shared buckets, 20 or 22 wide tables), 0 = none. */
int mira_msm_last_table_bits(int32_t *table_bits);

/* ---- a key's tuning, from one process to the next ----------------------------------------
 * A key tunes itself while it works: the first ~10 commits of every shape (pairs, commitments per submission, path) run at the
 * planner's width and its four neighbours, each twice (MIRA_TUNE_WIDTH_TRIALS), the first commits over several shared-bucket sets
 * go through every set twice, and the planner works from the bit lengths of the PREVIOUS commit of a length.  None of it outlives
 * the process; the reference's drivers fold one or two steps (examples/groth16/main.rs:285-298, benches/trivial/main.rs:111-148).
 * mira_msm_tuning_export writes what the key has settled as a blob of bytes, mira_msm_tuning_import installs such a blob in a
 * key registered later (right after mira_msm_register_bases* -- and after mira_msm_set_handle_max_window_bits and the table
 * builds of mira_msm_precompute*, if the key gets any: they are part of the identity below; the caller keeps the bytes where it keeps the key's
 * .cache/{label}/{k}.bin, src/commitment.rs:134-166).  A blob NEVER changes a result, only which width or set a commit runs at, and it
 * records what was measured under the MIRA_TUNE_* knobs in force when the trials ran.  An imported record of the GLV split does
 * not build the endomorphism copy early: mira_msm_precompute_ex(handle, MIRA_TABLE_GLV) does.  Neither call launches anything or
 * touches device memory.
 *
 * export: *len_out is always the blob's full length; cap = 0 asks for it (buf may be NULL).  0 < cap < length -> MIRA_E_BAD_ARG,
 * nothing written.  The same state gives the same bytes: no timestamps, no pointers.
 *
 * import, three outcomes:
 *   malformed bytes            -> MIRA_E_BAD_ARG, the reason in mira_last_error(), *accepted_out = 0, the key unchanged
 *   well-formed, other identity -> MIRA_OK, *accepted_out = 0, the key unchanged (a stale file costs nothing and is no error)
 *   accepted                   -> MIRA_OK, *accepted_out = 1: every record is the finished trial of its shape (replacing the key's own
 *                                 record of that shape, a running one included; the key still keeps 12 shapes, least recently
 *                                 used out first), and the statistics slot, when present, is the key's
 * The whole blob is validated before the key is touched.
 *
 * Layout, little-endian, no padding:
 *   offset  size
 *   0       8       magic "MIRATUNE"
 *   8       4       u32 format version, 1
 *   -- identity
 *   12      4       u32 A, length of the architecture string, 1 .. 64
 *   16      A       the device's architecture name up to the first ':' ("gfx950"; "emu" in the test-only emulation), no NUL
 *   +0      8       u64 fingerprint of the planner's model: FNV-1a 64 over the bytes of its measured tables and trial schedule
 *                   (a re-measured table retires every older blob by itself)
 *   +8      4       u32 curve (MIRA_CURVE_*)
 *   +12     8       u64 key length in points
 *   +20     4       u32 max_c (mira_msm_set_handle_max_window_bits)
 *   +24     4       u32 S, the number of shared-bucket sets, <= 32
 *   +28     4 S     u32 their widths, in the order they were built
 *   +0      4       u32 width of the wide tables (20 / 22), 0 = none
 *   -- records: the FINISHED trials, sorted by (n, count, kind)
 *   +4      4       u32 R <= 12
 *   +8      32 R    per record: u64 n (pairs), u32 count (commitments per launch), u32 kind (bit 0 = GLV split, bit 1 = host
 *                   scalars, bit 2 = a trial among the key's sets), u32 c0 (the model's width), u32 best_c (the width kept),
 *                   f64 best_us (its measured wall time, IEEE 754 binary64)
 *   -- statistics slot
 *   +0      4       u32 1 = present (the key has statistics), 0 = absent
 *   +4      8       u64 stat_n, the length of the commit they came from      } only when present
 *   +12     4       u32 stat_kind: 0 = whole scalars, 1 = halves of the split }
 *   +16     1024    256 x u32 counters, [b] = sampled values of bit length b  }
 *   -- end
 *   +0      8       u64 FNV-1a 64 (offset basis cbf29ce484222325, prime 100000001b3) over every byte before it
 * Malformed: bad magic, version, length or checksum; trailing bytes; R > 12; two records of one shape; n = 0, n > key length,
 * count = 0, kind > 7; a best_c no trial of that kind can have produced (plain: 4 .. max_c; GLV split: 5 .. 16; set trial: one of
 * the S widths); a best_us that is negative or no number; a statistics flag other than 0 / 1, stat_n = 0 or > key length,
 * stat_kind > 1, or counters that sum to more than twice the values histogrammed, 2 (stat_kind + 1) stat_n (the counters are a
 * weighted sample of the scalars, so they add up to about, not exactly, stat_n values -- or 2 stat_n halves).  A blob is judged
 * against the identity it states itself. */
int mira_msm_tuning_export(uint64_t handle, void *buf, size_t cap, size_t *len_out);
int mira_msm_tuning_import(uint64_t handle, const void *buf, size_t len, int32_t *accepted_out);

/* Thresholds of the engine's internal choices, for tests and tuning runs (they never change a
 * result): the smallest MSM that takes the LDS-staged two-level sort, the smallest MSM that uses a
 * handle's window tables, the smallest commit whose scalar-length statistics plan the next one, and
 * the longest NTT line (log2) -- shorter lines make the two- and three-pass schedules reachable at
 * small sizes -- and whether lines of up to 256 points take the wave-level kernel (1: wherever it
 * can; 0: never; default: by size); the smallest commit of HOST scalars that is cut into point chunks so
 * that the copy of one chunk overlaps the kernels of the previous one; the largest post-twiddle exponent
 * range (log2) an NTT serves from one table -- beyond it pass 1 reads a table of n entries, or, above
 * 2^24 points, multiplies two table entries.  value < 0 restores the default. */
#define MIRA_TUNE_STAGED_MIN_N 0
#define MIRA_TUNE_TABLE_MIN_N 1
#define MIRA_TUNE_PLAN_HIST_MIN_N 2
#define MIRA_TUNE_NTT_MAX_LOG_LINE 3
#define MIRA_TUNE_NTT_WAVE 4
#define MIRA_TUNE_HOST_CHUNK_MIN_N 5
#define MIRA_TUNE_NTT_SINGLE_TW_LOG 6
/* largest transform (log2) whose first post-twiddle is served from a table of n entries (48 n bytes per cached
 * table set); default 24, 0 = never */
#define MIRA_TUNE_NTT_FULL_TW_MAX_LOG 7
/* serve commits from the shared-bucket table set of exactly this width (calibration, tests); 0 / default = choose by length */
#define MIRA_TUNE_TABLE_WIDTH 8
/* column reads a specialised cross-term kernel keeps in flight ahead of their use (mira_graph_specialize); default 4 */
#define MIRA_TUNE_JIT_LOADS_AHEAD 9
/* smallest number of sorted entries one lane of k_accumulate adds (shorter segments: more lanes busy on a small commit,
 * more cut runs for the fix-up); 1 .. 2^20, default 10 (negative: the default; 0 and longer ones: MIRA_E_BAD_ARG -- the
 * planner divides by it and keeps it in 32 bits) */
#define MIRA_TUNE_MIN_SEGMENT 10
/* 0: do not use a key's endomorphism copy (MIRA_TABLE_GLV) -- same-key A/B runs and tests; default 1 */
#define MIRA_TUNE_GLV 11
/* bucket reduction (csrc/reduce_kernels.cuh): results per bucket set handed to the host's chain of doublings (default: by
 * shape; 1 = plain window sums), log2 of the buckets per running-sum chunk (default 2 by quads / 3 by lanes), and whether
 * the running sums are taken by quads of lanes (1) or single lanes (0; default: quads while the chunks are few) */
#define MIRA_TUNE_REDUCE_PIECES 12
#define MIRA_TUNE_REDUCE_LAMBDA 13
#define MIRA_TUNE_REDUCE_QUAD 14
/* smallest commit served from a key's shared-bucket table sets (default 2^12); MIRA_TUNE_TABLE_MIN_N is the wide tables' */
#define MIRA_TUNE_SHARED_MIN_N 15
/* log2 of the sorted entries (pairs x windows) one pass of the pipeline takes; a longer commit is cut into point chunks that
 * add into one set of buckets (default and maximum 32: the entry offsets are 32-bit; tests cut small commits with it) */
#define MIRA_TUNE_PASS_ENTRIES_LOG 16
/* log2 of the longest key whose endomorphism copy (MIRA_TABLE_GLV, 2 x the key's memory) the library builds BY ITSELF, at the
 * first single commit or batch that can use it (commits of at most 2^21 pairs over keys of at least 2^12 points); default 26,
 * 0 = only where mira_msm_precompute_ex(handle, MIRA_TABLE_GLV) was called */
#define MIRA_TUNE_GLV_AUTO_MAX_LOG 17
/* 1 (default): the window width the planner picks for a shape of commit (pairs, commitments per submission, path) over a key is
 * checked against its four neighbours on the first ten commits of that shape -- each candidate timed twice -- and the fastest
 * measured is kept for the rest of the key's life (commits of >= 2^12 pairs, unforced widths, not the ranks of a sharded MSM); 0: the
 * planner's tables alone decide */
#define MIRA_TUNE_WIDTH_TRIALS 18
/* workgroups in the persistent grid of the NTT kernels (default: 256 CUs x the workgroups that fit one).  A pass with at least
 * four block-groups (wave-level kernel) or lines (workgroup-level kernel) per workgroup hands them out through per-XCD counters;
 * tests set a small grid so that this path, its ranges without a home workgroup included, runs at sizes the CPU emulation reaches */
#define MIRA_TUNE_NTT_GRID 19
/* smallest window width whose commits take the two-level front of the wide windows (int32 digits, a coarse histogram and sort
 * by the top 9 bits of the bucket, bucket counts from that output; csrc/msm_host.cuh); default 17, the first width whose bucket
 * histogram does not fit LDS.  Tests set it low so that narrow widths run through that front at sizes the CPU emulation reaches */
#define MIRA_TUNE_WIDE_FRONT_MIN_C 20
/* mira_lookup_m_device: 1 = every key starts probing its hash table at slot 0 (tests: long probe chains at small sizes);
 * default / 0 = hashed.  Never changes a result */
#define MIRA_TUNE_LOOKUP_HASH 21
/* elements per lane of every level of a batch inversion (mira_batch_invert_device, mira_lookup_h_g_device), 2 .. 64, default 8.
 * Never changes a result */
#define MIRA_TUNE_INV_CHUNK 22
/* workgroups of one sweep of the deciders (mira_count_ne_device, mira_sum_sub_device, mira_graph_check_compiled,
 * mira_perm_check_device), 1 .. 2048 (0 or more -> MIRA_E_BAD_ARG; negative restores the default: one per 256 elements, at
 * most 2048).  Tests use it to reach several workgroups at small sizes.
 * Never changes a result */
#define MIRA_TUNE_DECIDE_GRID 23
/* points per chunk of mira_setup_bases_device / mira_msm_setup_bases: the host squeezes 32 bytes of SHAKE256 per point into one of
 * two pinned buffers while the kernels of the chunk before run; 16 .. 2^24, default 2^18 (anything else that is not negative ->
 * MIRA_E_BAD_ARG).  Tests set it small so that chunk boundaries fall inside the sponge's 136-byte blocks.  Never changes a result */
#define MIRA_TUNE_SETUP_CHUNK 24
/* row-block workgroups per (point, gate) of mira_graph_eval_folded_device / mira_graph_eval_folded_reduce: each walks the blocks of
 * 256 rows b, b + value, ...; 0 or negative: the default (about 2048 workgroups over all points and gates, at most one per row
 * block).  Tests use it to make one workgroup walk several row blocks at small sizes.  Never changes a result */
#define MIRA_TUNE_FOLDED_GRID 25
int mira_set_tuning(int knob, int64_t value);

/* Read a range of the registered key back in the reference layout (cache file writing,
 * save_to_file, src/commitment.rs:96-101). */
int mira_msm_download_bases(uint64_t handle, size_t first, size_t n, uint64_t *bases_out /* n * 8 limbs */);

/* ---- the step after the MSM in one fold: RelaxedPlonkWitness::fold (src/plonk/mod.rs:1097-1134)
 * field: MIRA_FIELD_FQ / MIRA_FIELD_FR.  Vectors stay in HBM between the commits and the fold.
 *   mira_fold_witness_device:  out[i] = w1[i] + r * w2[i]
 *   mira_fold_error_device:    e[i]  += sum_k r^(k+1) * cross_terms[k][i],  k < num_terms <= 16
 * mira_g1_mul_add: out = acc + scalar * point on affine points -- the single-scalar best_multiexp
 * calls of RelaxedPlonkInstance::fold (src/plonk/mod.rs:986-999, 1049-1053); host, O(256).   */
#define MIRA_FIELD_FQ 0
#define MIRA_FIELD_FR 1
int mira_fold_witness_device(int field, void *d_out, const void *d_w1, const void *d_w2, const uint64_t r[4], size_t n);
int mira_fold_error_device(int field, void *d_e, const void *const *d_cross_terms, size_t num_terms, const uint64_t r[4], size_t n);
/* Both halves of RelaxedPlonkWitness::fold in one submission (src/plonk/mod.rs:1097-1134): w_out[i] = w1[i] + r * w2[i], i < n_w,
 * and e_out[i] = e[i] + sum_k r^(k+1) * cross_terms[k][i], i < n, k < num_terms <= 16 (d_e_out may be d_e: in place) -- the values
 * of the two calls above, with one copy of constants and one synchronisation instead of two each. */
int mira_fold_relaxed_witness_device(int field, void *d_w_out, const void *d_w1, const void *d_w2, size_t n_w, void *d_e_out, const void *d_e,
                                     const void *const *d_cross_terms, size_t num_terms, const uint64_t r[4], size_t n);
int mira_g1_mul_add(int curve, const uint64_t acc[8], const uint64_t scalar[4], const uint64_t point[8], uint64_t out[8]);
/* out = acc + sum_i scalars[i] * points[i], count <= 64: E_commit + sum_k r^(k+1) T_k over the cross-term
 * commitments (src/plonk/mod.rs:1049-1053); host: width-5 NAFs, the terms dealt to the library's resident host
 * threads, one chain of doublings per thread. */
int mira_g1_lincomb(int curve, const uint64_t acc[8], const uint64_t *scalars /* count * 4 */, const uint64_t *points /* count * 8 */,
                    size_t count, uint64_t out[8]);
/* The commitment side of RelaxedPlonkInstance::fold in one call (src/plonk/mod.rs:986-999, 1049-1053):
 *   w_out[i] = w1[i] + r * w2[i], i < nw <= 64;   e_out = e + sum_k r^(k+1) * t_commits[k], k < count <= 64
 * -- the same points as nw calls of mira_g1_mul_add and one of mira_g1_lincomb over the powers of r, as ONE parallel
 * region on the host threads (every W commitment and every group of cross-term commitments is a task). */
int mira_g1_fold_commitments(int curve, const uint64_t r[4], const uint64_t *w1 /* nw * 8 */, const uint64_t *w2 /* nw * 8 */, size_t nw,
                             const uint64_t e[8], const uint64_t *t_commits /* count * 8 */, size_t count, uint64_t *w_out /* nw * 8 */, uint64_t e_out[8]);

/* ---- the lookup argument's witness rounds (src/plonk/lookup.rs:278-321) --------------------------
 * Vectors of 32-byte Montgomery elements in HBM, field MIRA_FIELD_FQ / MIRA_FIELD_FR.  n = 0 is a no-op.  A null pointer with
 * n > 0, an unknown field, or an output overlapping an input (other than in-place inversion) -> MIRA_E_BAD_ARG; a length of 2^32
 * or more -> MIRA_E_UNSUPPORTED; a workspace that does not fit -> MIRA_E_ALLOC.  An input element >= the modulus (equality is
 * decided on the representation) -> MIRA_E_BAD_ARG, the outputs are then unspecified.  Results do not depend on scheduling.
 *
 * mira_batch_invert_device: out[i] = in[i]^-1, 0 -> 0; d_out == d_in allowed.  The per-element `invert()` of evaluate_h_g
 * (lookup.rs:309-321), by Montgomery's trick: one Fermat inversion per call.
 * mira_lookup_m_device: evaluate_m (lookup.rs:278-307): m[i] = F::from_u128(#{j : l[j] == t[i]}) if t[i] is the first
 * occurrence of its value in t, else 0 (an l value absent from t counts nowhere).  Replaces the HashMap / HashSet pass.
 * mira_lookup_h_g_device: evaluate_h_g (lookup.rs:309-321): h[i] = 1 / (l[i] + r), g[i] = m[i] / (t[i] + r), 0 where the
 * denominator is 0; both vectors share one batch inversion.  r: Montgomery form, canonical. */
int mira_batch_invert_device(int field, void *d_out, const void *d_in, size_t n);
int mira_lookup_m_device(int field, void *d_m /* n_t */, const void *d_l, size_t n_l, const void *d_t, size_t n_t);
int mira_lookup_h_g_device(int field, void *d_h /* n_l */, void *d_g /* n_t */, const void *d_l, size_t n_l,
                           const void *d_t, const void *d_m, size_t n_t, const uint64_t r[4] /* Montgomery */);

/* ---- the step before the MSM in one fold: cross-term evaluation ----------------------------
 * GraphEvaluator::evaluate over all rows (src/polynomial/graph_evaluator.rs:361-390, called per
 * row from commit_cross_terms, src/nifs/vanilla/mod.rs:100-121): out[row] = value of the last
 * calculation, for row < num_rows.  The output stays in HBM, ready for mira_msm_batch_device and
 * mira_fold_error_device.
 *
 * mira_graph is the reference structure flattened (graph_evaluator.rs:165-185):
 *   constants   num_constants field elements (Montgomery, as the reference holds them)
 *   rotations   num_rotations i32; a column read at rotation index k uses row
 *               (row + rotations[k]).rem_euclid(num_rows)                  (:51-53)
 *   code        the calculations in order; calculation i writes intermediate i (its `target`).
 *               One header word  op | nparts << 8,  then the operands as value sources:
 *                 ADD, SUB, MUL: a, b.   SQUARE, DOUBLE, NEGATE, STORE: a.
 *                 HORNER: start, factor, parts[nparts]   (value = start; value = value*factor + part)
 *   value source  kind << 29 | payload                                   (ValueSource, :56-68)
 *                 CONSTANT: index into constants.  INTERMEDIATE: index of an earlier calculation.
 *                 CHALLENGE: index into challenges.
 *                 COLUMN: column | rotation_index << 20 -- Fixed{index, rotation} and
 *                 Poly{index, rotation} after the caller has resolved the column (selector, fixed
 *                 or witness slice: eval_column_var, src/plonk/eval.rs:57-69 and :136-229) to an
 *                 entry of `columns`.
 * columns[k]: device pointer to num_rows values; kind MIRA_COL_FIELD = field elements,
 * MIRA_COL_BOOL = bytes (a selector: non-zero -> ONE, zero -> ZERO).  A null pointer marks a column
 * index that does not resolve; using it is ColumnVariableIndexOutOfBoundary / InvalidWitnessIndex
 * -> MIRA_E_BAD_ARG, as are a challenge or constant index out of range
 * (ChallengeIndexOutOfBoundary) and malformed code.  No calculations -> out = 0 (:386-389).    */
#define MIRA_OP_ADD 0u
#define MIRA_OP_SUB 1u
#define MIRA_OP_MUL 2u
#define MIRA_OP_SQUARE 3u
#define MIRA_OP_DOUBLE 4u
#define MIRA_OP_NEGATE 5u
#define MIRA_OP_HORNER 6u
#define MIRA_OP_STORE 7u
#define MIRA_SRC_CONSTANT 0u
#define MIRA_SRC_INTERMEDIATE 1u
#define MIRA_SRC_COLUMN 2u
#define MIRA_SRC_CHALLENGE 3u
#define MIRA_COL_FIELD 0u
#define MIRA_COL_BOOL 1u
typedef struct mira_graph {
    const uint32_t *code;
    size_t code_words;
    uint32_t num_calculations;
    uint32_t num_constants;
    const uint64_t *constants;   /* num_constants * 4 limbs */
    const int32_t *rotations;
    uint32_t num_rotations;
    uint32_t reserved;
} mira_graph;
typedef struct mira_eval_column {
    const void *d_data;
    uint32_t kind;
    uint32_t reserved;
} mira_eval_column;
int mira_graph_eval_device(int field, const mira_graph *graph, const mira_eval_column *columns, uint32_t num_columns,
                           const uint64_t *challenges /* num_challenges * 4 limbs, host */, uint32_t num_challenges,
                           size_t num_rows, void *d_out /* num_rows field elements */);
/* The same in two steps.  A GraphEvaluator is built once per circuit (GraphEvaluator::new,
 * graph_evaluator.rs:196-206) and evaluated at every fold step with new witnesses and challenges:
 * mira_graph_compile validates the structure (everything above except the columns' pointers),
 * allocates the intermediates and uploads the program once; mira_graph_eval_compiled then costs one
 * small copy (challenges, column pointers) and one launch.  The counts of challenges and columns are
 * fixed at compile time; a null column that the code reads is the error described above. */
int mira_graph_compile(int field, const mira_graph *graph, uint32_t num_challenges, uint32_t num_columns, uint64_t *handle_out);
int mira_graph_eval_compiled(uint64_t handle, const mira_eval_column *columns, uint32_t num_columns,
                             const uint64_t *challenges, uint32_t num_challenges, size_t num_rows, void *d_out);
int mira_graph_free(uint64_t handle);
/* The d - 1 cross-term graphs of one fold step (src/nifs/vanilla/mod.rs:100-121 evaluates them one
 * after the other over the same witnesses and challenges) in one submission: count compiled graphs
 * of one field, compiled for the same numbers of challenges and columns, over the same columns;
 * graph k writes d_outs[k].  Row for row the values of count mira_graph_eval_compiled calls. */
int mira_graph_eval_batch(const uint64_t *handles, uint32_t count, const mira_eval_column *columns, uint32_t num_columns,
                          const uint64_t *challenges, uint32_t num_challenges, size_t num_rows, void *const *d_outs);
/* Optional, once per circuit: give every one of these compiled graphs a kernel of its own.  The engine writes the
 * graph's instruction stream out as straight-line HIP and compiles it for the device at run time (hiprtc, one host
 * thread per graph, ~5 s for one evaluation point of a MainGate<5> gate): intermediates live in registers instead of
 * LDS / workspace slots, there is no decoding, a rotated row is reduced once per row instead of once per column read.
 * Evaluation then runs at about twice the interpreter's rate; every value is the interpreter's (the same field
 * operations in the same order).  The gate polynomial of a circuit is fixed for the whole IVC run
 * (src/ivc/public_params.rs: the PlonkStructure is built once), so this belongs where the GraphEvaluators are built.
 * The call blocks for the compilation but releases the library's lock meanwhile: other threads keep committing and
 * evaluating (interpreted), and a handle freed before the compiler is done is skipped.
 * Soft failures, each with its own code and the reason in mira_last_error(): MIRA_E_JIT_UNAVAILABLE (no libhiprtc.so on this
 * machine), MIRA_E_UNSUPPORTED (a graph of more than 1536 instructions), MIRA_E_JIT_FAILED (the compiler or the module loader
 * failed: the text carries the compiler's log).  In all three nothing has changed and the graphs keep being interpreted --
 * on the GPU, there is no host path.  The three kernel headers the generated source includes are embedded in the library.
 * `columns`: the column table the graphs will be evaluated over -- only the KINDS are read (which columns are selector
 * bytes is a property of the circuit); an evaluation over columns of other kinds than the kernel was built for is
 * interpreted.
 * mira_graph_is_specialized reports 1 / 0; mira_graph_jit_source copies the generated source (NUL-terminated, at most
 * cap bytes; *len_out = its full length) for inspection and for tests. */
int mira_graph_specialize(const uint64_t *handles, uint32_t count, const mira_eval_column *columns, uint32_t num_columns);
int mira_graph_is_specialized(uint64_t handle, int32_t *out);
int mira_graph_jit_source(uint64_t handle, const mira_eval_column *columns, uint32_t num_columns, char *buf, size_t cap, size_t *len_out);
/* Code objects on disk.  mira_graph_set_cache_dir(dir): every kernel mira_graph_specialize compiles from now on is also
 * written to `dir` (which must exist), and a graph whose kernel lies there is loaded instead of compiled -- the second
 * process of an IVC run over the same circuit specialises in milliseconds.  A file is taken only if the generated source
 * and the build environment -- the kernel headers embedded in libmira_gpu.so, the compiler options, the GPU architecture
 * of the bound device, the HIP runtime and hiprtc versions -- are the ones it was built from, byte for byte, and its code
 * hashes to what its header says; writing is best effort (an unwritable directory costs compilations, not errors).  A code
 * object is executed as found, so the directory must belong to the calling user and be writable by nobody else (else
 * MIRA_E_BAD_ARG; not a directory: MIRA_E_IO), and a file there that is somebody else's or group / world-writable is
 * ignored.  NULL or "" (the default): no files.  The reference keeps its commitment keys the same way
 * (src/commitment.rs:96-167, `.cache/`).
 * mira_graph_jit_stats: how many kernels the last mira_graph_specialize compiled / read from the directory.
 * mira_graph_jit_compile_check: compile a source text through the library's own path (hiprtc + the embedded headers) and
 * report the size of the code object; needs no GPU (build checks, tests). */
int mira_graph_set_cache_dir(const char *dir);
int mira_graph_jit_stats(uint32_t *compiled_out, uint32_t *from_disk_out);
int mira_graph_jit_compile_check(const char *source, size_t *code_size_out);

/* ---- ProtoGalaxy's compute_G: the gates of a circuit over a Lagrange combination of traces ----------------------------
 * compute_G (src/nifs/protogalaxy/poly/mod.rs:218-303) evaluates every gate over every row of FoldedTrace(X_p) for every
 * evaluation point X_p and reduces the values through a weighted tree.  The reference materialises a folded trace per point
 * (folded_trace.rs:69: "TODO Create on the fly to avoid multiple rows iterations"); here the fold happens in the column
 * fetch of the interpreter and, in the reduce form, the leaves never leave the workgroup.
 *
 * handles[g], g < num_gates: compiled graphs (mira_graph_compile) of one field, all compiled for num_columns / num_challenges:
 *   S.gates in the order of plonk::iter_evaluate_witness (src/plonk/mod.rs:1158-1178).
 * columns[j * num_columns + c]: column c of trace j, j < num_traces (trace 0 = the accumulator), 1 <= num_traces <= 16.
 * column_folded[c] != 0: a witness column -- the value the program reads at (c, row) is
 *       sum_j coeffs[p * num_traces + j] * columns[j][c][row]          (FoldedTrace, folded_trace.rs:53-131)
 *   and must be MIRA_COL_FIELD in every trace;  == 0: a column of the circuit (selector, fixed): read from trace 0 as it is.
 * coeffs: host, num_points x num_traces elements, Montgomery: L_j(X_p).  challenges: host, num_points x num_challenges,
 *   the caller's fold_plonk_challenges (:135-179: O(points) scalar work, it stays with the caller).
 * 1 <= num_points <= 256.
 * Every value equals the one mira_lincomb_device + mira_graph_eval_compiled (+ mira_pow_tree_reduce_device) give, bit for bit.
 * Errors: an unknown handle, graphs of different fields or compiled for other column / challenge counts, a null column that
 * some gate reads (in any trace for a folded column: "column variable index out of boundary"), a folded column of kind
 * MIRA_COL_BOOL, num_traces or num_points out of range -> MIRA_E_BAD_ARG; num_rows > 2^31 -> MIRA_E_UNSUPPORTED; nothing is
 * written then.  num_rows == 0: success (`out` all zero).  A gate with no calculations contributes zero leaves.
 * A handle with a specialised kernel (mira_graph_specialize) is INTERPRETED by these two calls: the generated kernels read
 * plain columns only.  MIRA_TUNE_FOLDED_GRID sets the workgroups per (point, gate). */
int mira_graph_eval_folded_device(const uint64_t *handles, uint32_t num_gates, const mira_eval_column *columns, uint32_t num_columns,
                                  uint32_t num_traces, const uint8_t *column_folded, const uint64_t *coeffs, const uint64_t *challenges,
                                  uint32_t num_challenges, uint32_t num_points, size_t num_rows,
                                  void *d_out /* [(p * num_gates + g) * num_rows + row], canonical Montgomery */);
/* The same evaluation reduced through compute_G's tree (:263-290) without writing the leaves:
 *   out[p] = sum_i leaf[p][i] * prod_{j : bit j of i} weights[j],  i = g * num_rows + row,  levels = log2(num_gates * num_rows)
 * weights: host, `levels` elements (betas_stroke, the same for every point).  out: host, num_points elements.
 * num_gates * num_rows not a power of two -> MIRA_E_UNSUPPORTED (the reference's tree is `unreachable!` there).
 * A workgroup folds the first min(8, log2 num_rows) levels of its 256 rows in LDS; one node per (point, gate, row block) goes to
 * library scratch (released by mira_trim) and the rounds of mira_pow_tree_reduce_device finish from there. */
int mira_graph_eval_folded_reduce(const uint64_t *handles, uint32_t num_gates, const mira_eval_column *columns, uint32_t num_columns,
                                  uint32_t num_traces, const uint8_t *column_folded, const uint64_t *coeffs, const uint64_t *challenges,
                                  uint32_t num_challenges, uint32_t num_points, size_t num_rows, const uint64_t *weights, uint64_t *out);

/* ---- the deciders on device-resident vectors (src/plonk/mod.rs:434-622) ------------------------
 * What IVC::verify (src/ivc/incrementally_verifiable_computation.rs:617-680) runs over the witness vectors a fold step left
 * in HBM, without copying them to the host.  Vectors of 32-byte Montgomery elements, field MIRA_FIELD_FQ / MIRA_FIELD_FR;
 * equality is decided on the representation, as PartialEq on the canonical limbs does.  n = 0 is a no-op with count 0 and sum 0;
 * a null pointer with n > 0 or an unknown field -> MIRA_E_BAD_ARG; an input element >= the modulus -> MIRA_E_BAD_ARG, the
 * outputs are then unspecified.  Counts, first indices and sums are exact and do not depend on scheduling (no global atomics:
 * one partial record per workgroup, folded by one more workgroup; field addition is associative).
 *
 * mira_count_ne_device: the count of i < n with a[i] != b[i] (d_b NULL: a[i] != 0) and the smallest such i (UINT64_MAX if
 * none; the reference warn!s the row, mod.rs:526) -- the compare half of the row sweeps and of any vector comparison.
 * mira_sum_sub_device: out = sum a[i] - sum b[i] (d_b NULL: sum a[i]), canonical Montgomery: the per-lookup sum of
 * is_sat_log_derivative (mod.rs:592-622), zero iff the lookup is satisfied.
 * mira_graph_check_compiled: the row sweep of is_sat (d_expected NULL, mod.rs:458-478) / is_sat_relaxed (d_expected = W.E,
 * mod.rs:516-541): evaluates a compiled graph over all rows into library scratch -- through a specialised kernel when the
 * handle has one, exactly as mira_graph_eval_compiled does -- and counts the rows that differ from 0 / from d_expected:
 * Error::EvaluationMismatch { mismatch_count, total_row = num_rows }. */
int mira_count_ne_device(int field, const void *d_a, const void *d_b /* may be NULL */, size_t n, uint64_t *count_out, uint64_t *first_out /* may be NULL */);
int mira_sum_sub_device(int field, const void *d_a, const void *d_b /* may be NULL */, size_t n, uint64_t out[4]);
int mira_graph_check_compiled(uint64_t handle, const mira_eval_column *columns, uint32_t num_columns, const uint64_t *challenges,
                              uint32_t num_challenges, size_t num_rows, const void *d_expected /* may be NULL */, uint64_t *mismatch_out,
                              uint64_t *first_row_out /* may be NULL */);
/* is_sat_perm (mod.rs:563-589): y = P Z by matrix_multiply (src/polynomial/sparse.rs:7-19), count of y_i != Z_i ->
 * Error::PermCheckFail { mismatch_count }.
 * mira_perm_compile, once per circuit (PlonkStructure::permutation_matrix is fixed): the triples (row, col, value) of an
 * n x n SparseMatrix, host memory; values: nnz * 4 limbs, Montgomery, or NULL = all ONE.  row >= n or col >= n ->
 * MIRA_E_BAD_ARG (the reference panics "invalid matrix multiply"); n or nnz >= 2^32 -> MIRA_E_UNSUPPORTED.  Triples in any
 * order; duplicates of (row, col) add, as the reference's loop does; a row without a triple gives y_i = 0.  A matrix whose
 * every row holds exactly one entry of value ONE (construct_permutation_matrix + fill_sparse_matrix, src/plonk/util.rs:44-71,
 * 128-174) is kept as one u32 per row, any other as CSR with the values in multiplier form.
 * mira_perm_check_device: Z = instance (host, num_io elements) || d_w (device, n_w elements: W[0][..2^k * num_advice]); Z is
 * never materialised.  num_io + n_w != n -> MIRA_E_BAD_ARG.
 * mira_perm_free: releases the compiled matrix. */
int mira_perm_compile(int field, const uint64_t *rows, const uint64_t *cols, const uint64_t *values /* nnz * 4 or NULL */, size_t nnz, size_t n,
                      uint64_t *handle_out);
int mira_perm_check_device(uint64_t handle, const uint64_t *instance, size_t num_io, const void *d_w, size_t n_w, uint64_t *mismatch_out,
                           uint64_t *first_out /* may be NULL */);
int mira_perm_free(uint64_t handle);


/* ---- ProtoGalaxy's polynomial pipeline around the NTT (src/nifs/protogalaxy/poly/mod.rs) -------
 * mira_pow_tree_reduce_device: the weighted tree reduction of compute_F (:131-166) and compute_G
 * (:263-290), itertools::tree_reduce with node(left, right) = left + right * weights[p][height]:
 *     out[p] = sum_i leaves[p][i] * prod_{j : bit j of i} weights[p][j],   i < n_leaves = 2^levels
 * leaves: device; point p's leaves start at element p * leaf_point_stride, 0 = every point reads
 * the same leaves (compute_F: the challenge sits on the edges; compute_G: in the leaves).
 * weights: host, num_points x levels elements.  out: host, num_points elements -- the input of
 * the small ifft that yields the coefficients.  n_leaves must be a power of two (the reference's
 * tree is `unreachable!` otherwise) -> MIRA_E_UNSUPPORTED.
 * mira_lincomb_device: out[i] = sum_k coeffs[k] * vecs[k][i], k < num_vecs <= 16 -- the witness of
 * FoldedTrace at one challenge, L_0(X) * acc + sum_j L_j(X) * trace_j (folded_trace.rs:54-131). */
int mira_pow_tree_reduce_device(int field, const void *d_leaves, size_t n_leaves, size_t leaf_point_stride,
                                const uint64_t *weights, uint32_t num_points, uint64_t *out);
int mira_lincomb_device(int field, void *d_out, const void *const *d_vecs, const uint64_t *coeffs /* num_vecs * 4 limbs, host */,
                        size_t num_vecs, size_t n);
/* num_outs <= 8 linear combinations of the same num_vecs <= 16 vectors in one sweep: outs[m][i] = sum_k coeffs[m][k] * vecs[k][i]
 * (coeffs: num_outs x num_vecs elements, row-major, host).  An output must not alias an input.  The interpolation step of the
 * cross terms: commit_cross_terms' d vectors (src/nifs/vanilla/mod.rs:100-121) are the coefficients of
 * f(W1 + X W2, c1 + X c2) in X, i.e. fixed linear combinations of d + 1 values of that polynomial per row. */
int mira_lincomb_multi_device(int field, void *const *d_outs, size_t num_outs, const void *const *d_vecs, size_t num_vecs,
                              const uint64_t *coeffs, size_t n);

/* ---- NTT over bn256::Fr (src/fft.rs) -----------------------------------------------------
 * In place, natural order in and out.  `a` = 2^log_n elements, log_n <= 28 = Fr::S as in the
 * reference (src/fft.rs:13); the device needs a second buffer of the same size above 2^12.      */
/* best_fft(a, omega, log_n), src/fft.rs:51 */
int mira_ntt_bn256_fr(uint64_t *a, uint32_t log_n, const uint64_t omega[4]);
int mira_ntt_bn256_fr_device(void *d_a, uint32_t log_n, const uint64_t omega[4]);
/* fft / ifft, src/fft.rs:160-174 (omega from get_omega_or_inv, ifft scales by TWO_INV^log_n) */
int mira_fft_bn256_fr(uint64_t *a, uint32_t log_n);
int mira_ifft_bn256_fr(uint64_t *a, uint32_t log_n);
int mira_fft_bn256_fr_device(void *d_a, uint32_t log_n);
int mira_ifft_bn256_fr_device(void *d_a, uint32_t log_n);
/* coset_fft / coset_ifft, src/fft.rs:178-196 (ZETA pattern of distribute_powers_zeta, :205-226) */
int mira_coset_fft_bn256_fr(uint64_t *a, uint32_t log_n);
int mira_coset_ifft_bn256_fr(uint64_t *a, uint32_t log_n);
/* get_omega_or_inv(k, is_inverse), src/fft.rs:12-23; Montgomery form out */
int mira_get_omega_or_inv(uint32_t k, int is_inverse, uint64_t out[4]);

/* ---- synthetic inputs for benchmarks and tests -------------------------
 * kind 0 = uniform field elements, 1 = witness-like (70 % zero, 20 % < 2^32, 10 % uniform).
 * index0 = global index of the first element (lets ranks generate their own chunk).          */
int mira_synth_scalars_device(int curve, size_t n, uint64_t index0, uint64_t seed, int kind, void *d_out);
int mira_synth_bases_device(int curve, size_t n, uint64_t index0, uint64_t seed, void *d_out);

/* ---- CommitmentKey::setup(k, label), src/commitment.rs:52-76: a transparent key by hash-to-curve ------------------------
 * Point i of the key of `label` comes from bytes [32 i, 32 i + 32) of SHAKE256(label) (src/commitment.rs:58-65):
 *   hash_to_field  expand_message_xmd over BLAKE2b-512, DST = "from_uniform_bytes-" curve_id "_XMD:BLAKE2b_SVDW_RO_" byte(length),
 *                  curve_id = "bn256_g1" / "grumpkin_g1": two field elements u_0, u_1 (512 bits each, reduced mod p)
 *   map            Shallue-van de Woestijne (RFC 9380 appendix F.1, Z = 1) of each, and P_i = map(u_0) + map(u_1) by the full group law
 * Nobody knows a discrete logarithm between two such points -- unlike the bases of mira_synth_bases_device, which are public
 * multiples of the generator and serve benchmarks only.  The curve hashing the reference calls lives in halo2curves, which is not
 * part of it: these keys equal the project's own restatement (tests/setup_ref.py) and its recorded checksums and are UNPINNED
 * AGAINST halo2curves.  The reference's load_from_file / load_or_setup_cache read what mira_msm_save_bases_file writes of them.
 * Points leave in the reference layout (x * 2^256, y * 2^256, 4 x u64 each; the identity as 64 zero bytes); device pointers are
 * 16-byte aligned.  The stream is squeezed on the host in chunks of MIRA_TUNE_SETUP_CHUNK points beside the kernels; with timing
 * on, mira_get_timings reports setup_squeeze_host (host time), setup_hash and setup_map (device, summed over the first 63 chunks; a
 * chunk's setup_hash interval includes its wait for the chunk's bytes -- the two stages on their own report the kernel alone). */
/* setup, src/commitment.rs:52-76: points [first, first + n) of the key of `label` (any n; the same bytes as that slice of a longer
 * key: a shard generates its own range).  first + n > 2^32 or a null pointer with a non-zero length -> MIRA_E_BAD_ARG */
int mira_setup_bases_device(int curve, const void *label, size_t label_len, uint64_t first, size_t n, void *d_out /* n * 64 B */);
/* setup, src/commitment.rs:52-76, then registered as a resident key of 2^k points (as mira_msm_register_bases_device of the
 * above, without the intermediate copy).  k >= 32 -> MIRA_E_BAD_ARG (the reference asserts k < 32, src/commitment.rs:53) */
int mira_msm_setup_bases(int curve, uint32_t k, const void *label, size_t label_len, uint64_t *handle_out);
/* the two stages of setup, src/commitment.rs:52-76, on their own (neither hashing nor the stream reaches the map's exceptional
 * inputs): n messages of 32 bytes -> n x 2 field elements (Montgomery form, canonical); n x 2 canonical field elements -> n points.
 * d_points may be d_u */
int mira_hash_to_field_device(int curve, const void *d_msgs /* n * 32 B */, size_t n, void *d_u /* n * 2 elements */);
int mira_map_to_curve_device(int curve, const void *d_u /* n * 2 elements */, size_t n, void *d_points /* n * 64 B */);

/* ---- library-held device memory ------------------------------------------------------------
 * Workspaces (digit, sort and bucket buffers; NTT temporaries and the four cached twiddle-table sets,
 * up to 805 MB each at 2^24 points) grow on demand and are reused by later calls: after one commit of
 * 2^26 pairs the library holds about 6 GiB.  mira_trim releases the largest of them until at most
 * keep_bytes remain (0 = everything; registered keys, their window tables and compiled graphs are never
 * touched) and reports the bytes released; the next call re-allocates what it needs.
 * mira_dev_mem_info: hipMemGetInfo of the bound device. */
int mira_trim(size_t keep_bytes, size_t *released_out /* may be NULL */);
int mira_dev_mem_info(size_t *free_bytes, size_t *total_bytes);

/* ---- device memory helpers (thin hipMalloc/hipMemcpy wrappers for non-torch callers) ---- */
int mira_dev_alloc(size_t bytes, void **d_out);
int mira_dev_free(void *d);
int mira_dev_upload(void *d_dst, const void *h_src, size_t bytes);
int mira_dev_download(void *h_dst, const void *d_src, size_t bytes);
int mira_dev_copy(void *d_dst, const void *d_src, size_t bytes);   /* device to device */
int mira_dev_sync(void);

/* ---- measurement ------------------------------------------------------------------------
 * With timing on, every stage of the next MSM / NTT is bracketed by HIP events on the work
 * stream.  mira_get_timings returns the stage count and fills names/ms (ms[i] = device time of
 * stage i of the most recent call).  Stage names are static strings.                         */
int mira_set_timing(int enabled);
int mira_get_timings(const char **names, float *ms, int capacity);

#ifdef __cplusplus
}
#endif
#endif /* MIRA_GPU_H */
