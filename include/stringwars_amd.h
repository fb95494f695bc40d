/*
 * stringwars_amd.h -- C ABI of the MI355X-native batched edit-distance backend.
 *
 * This is the drop-in boundary for the similarity hot path of ashvardanian/StringWars
 * (`similarities/bench.rs`, `similarities/bench.py`). Every entry point below replaces one call
 * the reference makes into `stringzilla::szs` (whose own C ABI, `stringzillas.h`, is not vendored
 * under /root/reference) or into the per-pair CPU baselines. The `file:line` in each comment is
 * the reference call site that the symbol serves. Plain pointers and sizes only; no C++ or torch
 * types cross this boundary. All functions are `extern "C"`, return a status code and, when
 * `error` is non-NULL, leave a pointer to a static NUL-terminated message in `*error`.
 *
 * Memory: every pointer inside a tape and every `out` pointer may be DEVICE memory (hipMalloc,
 * torch CUDA tensors) -- used in place, the steady state the benchmark times -- or HOST memory
 * (pageable, pinned, managed), in which case the call stages it through PCIe itself. Calls are
 * synchronous (results are visible on return, like `compute_into`, bench.rs:478-486) unless the
 * scope was switched to asynchronous mode with `swh_scope_set_async`. "Visible on return" for an
 * output in device memory: every result has been written through to memory and acknowledged, any
 * stream, device or copy may read it; the scope's own stream may still be retiring the kernel
 * (the call returns on the kernel's summary, not on the stream: DESIGN.md section 3).
 *
 * Null handles and a missing device. No scope, engine or prepared tape can exist without a gfx950 device: `swh_scope_init_gpu`,
 * `swh_scope_init_gpu_stream` and `swh_scope_init_gpus` return swh_no_device_k and leave `*scope` NULL. What a caller then holds is a
 * NULL handle, and every call refuses one, writes none of its outputs and, where it has an `error` parameter, sets a message:
 *  - a NULL scope or engine (or a prepared view whose `tape` is NULL) is swh_invalid_argument_k;
 *  - the infix, OSA, LCS, partial-ratio and Jaro calls first ask whether a device is visible and return swh_no_device_k for a NULL scope or engine
 *    where there is none (swh_invalid_argument_k where there is one);
 *  - the `*_free` calls accept NULL and return swh_success_k; `swh_device_count` returns swh_success_k and a count of 0;
 *  - `swh_version` and `swh_capabilities` need no device.
 * The calls without an `error` parameter (`swh_scope_set_async`, `swh_scope_forget`, `swh_scope_describe`, the timing getters, ...)
 * return the status alone. `swh_scope_describe` with `capacity` below the length of the text returns swh_success_k and writes the first
 * `capacity - 1` characters and a NUL, nothing behind them; a NULL `text` or a `capacity` of 0 is swh_invalid_argument_k.
 */
#ifndef STRINGWARS_AMD_H_
#define STRINGWARS_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWH_VERSION_MAJOR 0
#define SWH_VERSION_MINOR 1
#define SWH_VERSION_PATCH 0

/* Status codes. 0 is success; the rest map onto the `Result<_, E: Display>` errors of the szs
 * wrappers (bench.rs:390-399 `.ok()`, :480-485 `panic!("{}", error)`, :632-635 SKIPPED). */
typedef enum swh_status_t {
    swh_success_k = 0,
    swh_bad_alloc_k = 1,
    swh_invalid_argument_k = 2,
    swh_invalid_utf8_k = 3,        /* C callers can pass bytes that Rust `&str` never could */
    swh_unsupported_length_k = 4,  /* "the engine may decline inputs beyond its supported length" bench.rs:394 */
    swh_no_device_k = 5,           /* no gfx950 device / HIP runtime unavailable */
    swh_device_error_k = 6,        /* a HIP call failed; message carries hipGetErrorString */
    swh_not_implemented_k = 7,
    swh_rccl_error_k = 8           /* RCCL could not be loaded, or a collective failed; message carries ncclGetErrorString */
} swh_status_t;

#define SWH_UNBOUNDED UINT32_MAX

/* Which DP algorithm a Levenshtein engine runs for unit costs (0,1,1,1). */
typedef enum swh_algorithm_t {
    swh_algorithm_auto_k = 0,        /* fastest measured path per length class */
    swh_algorithm_wavefront_k = 1,   /* anti-diagonal wavefront, register-tiled, DPP hand-off */
    swh_algorithm_bitparallel_k = 2, /* Myers/Hyyro bit-vectors, systolic over 32-row blocks; globally planned (device pre-pass) */
    swh_algorithm_tiled_k = 3        /* the same recurrence, every workgroup plans its own tile: no pre-pass, no host round trip */
} swh_algorithm_t;

/* ---- Device scope: replaces `DeviceScope::gpu_device(0)` (bench.rs:379, :652, :978). ------- */
typedef struct swh_scope_s *swh_scope_t;

/* Creates a scope on HIP device `device` with its own stream and scratch arena. */
swh_status_t swh_scope_init_gpu(int device, swh_scope_t *scope, const char **error);
/* Same, but work is enqueued on a caller-owned `hipStream_t` (e.g. torch's current stream). */
swh_status_t swh_scope_init_gpu_stream(int device, void *hip_stream, swh_scope_t *scope, const char **error);
/* `DeviceScope::cpu_cores(n)` (bench.rs:376-378). This backend has no CPU path: always returns
 * swh_not_implemented_k so a harness prints SKIPPED instead of silently running a fallback. */
swh_status_t swh_scope_init_cpu(size_t cores, swh_scope_t *scope, const char **error);
/* Several GPUs of ONE node behind one scope (single process): a member scope per device and an RCCL communicator
 * (`ncclCommInitAll`); the `<Ngpu>` rows beside the reference's `<1gpu>` ones (bench.rs:581-606). Ordinary engine calls on
 * such a scope run on its first device; the `*_sharded` calls below split a batch over all of them. `devices` may name one
 * device several times (members then share it and exchange by copies instead of RCCL -- a testing arrangement). */
swh_status_t swh_device_count(int *count);
swh_status_t swh_scope_init_gpus(const int *devices, int count, swh_scope_t *scope, const char **error);
swh_status_t swh_scope_device_count(swh_scope_t scope, size_t *devices);
swh_status_t swh_scope_free(swh_scope_t scope);
/* Compute-unit count for `auto_batch_size` (utils.rs:815-819, :826-836: one SM == one core). */
swh_status_t swh_scope_compute_units(swh_scope_t scope, size_t *compute_units);
/* async != 0: engine calls only enqueue; `swh_scope_synchronize` makes results visible. */
swh_status_t swh_scope_set_async(swh_scope_t scope, int async);
swh_status_t swh_scope_synchronize(swh_scope_t scope, const char **error);
/* Pipelined mode (implies async): successive engine calls alternate between two internal lanes (stream + scratch), so
 * the host-side planning of one call overlaps the DP kernel of the previous one. Ordering: a call starts after
 * everything that was enqueued on the scope's own stream (the one given to swh_scope_init_gpu_stream) before it --
 * producers of its inputs AND earlier consumers of the output buffer it overwrites. `swh_scope_join` makes that stream
 * wait for the latest call, for consumers ordered on it (e.g. an RCCL gather); `swh_scope_synchronize` waits for
 * everything. Buffers touched by streams the scope does not know about must be idle. */
swh_status_t swh_scope_set_pipelined(swh_scope_t scope, int enabled, const char **error);
swh_status_t swh_scope_join(swh_scope_t scope, const char **error);

/* What a scope REMEMBERS between calls. A scope learns from its calls -- the longest strings of the previous batch (raw tapes
 * then run without a planning pre-pass), the byte totals and ASCII-ness of the raw UTF-8 tapes it last staged, whether the
 * two-stage (band first) schedule paid off, which engine / tapes the small-alphabet alignment kernels could not take -- and
 * every belief is CHECKED on the device: a wrong one costs the call a redo, never a result. The reference's engines keep no
 * such state (`compute_into` is a pure function of its arguments, bench.rs:478-486); a caller who wants that -- or a timing
 * that does not depend on what ran before -- calls `swh_scope_forget` first. `swh_scope_describe` writes the beliefs as one
 * line of text (`key=value` pairs; truncated to `capacity`, always NUL-terminated) for logs and tests. */
swh_status_t swh_scope_forget(swh_scope_t scope);
swh_status_t swh_scope_describe(swh_scope_t scope, char *text, size_t capacity);

/* Kernel timing (hipEvents on the scope's stream around every kernel of the last engine call).
 * Used by bench.py's roofline object; off by default. */
typedef struct swh_timing_t {
    double total_ms;          /* all kernels of the last call, first-start to last-stop */
    double dominant_ms;       /* longest single kernel */
    double compute_ms;        /* time covered by the DP kernels (union of their intervals; everything but the planning / staging pre-pass) */
    char dominant_name[64];   /* its name */
    uint64_t cells;           /* nominal DP cells of the call (sum len_s(a)*len_s(b)) */
    uint64_t bytes;           /* algorithmic HBM bytes: symbols + offsets + results */
    uint32_t kernels;         /* number of kernel launches */
} swh_timing_t;
swh_status_t swh_scope_set_profiling(swh_scope_t scope, int enabled);
swh_status_t swh_scope_last_timing(swh_scope_t scope, swh_timing_t *timing);
/* Sums over every engine call since profiling was last switched on -- also the asynchronous and pipelined ones, whose
 * events are read when their lane is next used or the scope is synchronized. bench.py's roofline uses the mean of
 * `dominant_ms` over a pipelined run, i.e. kernel durations under the same conditions rocprofv3 sees them. */
typedef struct swh_timing_totals_t {
    double total_ms, dominant_ms, compute_ms;   /* sums of the per-call figures of swh_timing_t */
    uint64_t calls;
} swh_timing_totals_t;
swh_status_t swh_scope_timing_totals(swh_scope_t scope, swh_timing_totals_t *totals);

/* ---- Memory: `UnifiedAlloc` / `UnifiedMat` parity (bench.rs:292-295, :466-468). ------------ */
/* Host-visible, device-readable allocation (pinned + mapped). */
swh_status_t swh_unified_alloc(swh_scope_t scope, size_t bytes, void **pointer, const char **error);
swh_status_t swh_unified_free(swh_scope_t scope, void *pointer);
/* Explicit device allocation / copies for device-resident tapes (the timed steady state). */
swh_status_t swh_device_alloc(swh_scope_t scope, size_t bytes, void **pointer, const char **error);
swh_status_t swh_device_free(swh_scope_t scope, void *pointer);
swh_status_t swh_copy_to_device(swh_scope_t scope, void *device_dst, const void *host_src, size_t bytes,
                                const char **error);
swh_status_t swh_copy_to_host(swh_scope_t scope, void *host_dst, const void *device_src, size_t bytes,
                              const char **error);

/* ---- Tapes: `BytesTapeView<u64>` / `AnyBytesTape::View64` (bench.rs:62, :134-143, :292-306). */
/* Arrow-style: `offsets` has `count + 1` entries, string i is data[offsets[i] .. offsets[i+1]).
 *  - offsets[0] may be non-zero: a tape may be a window of a larger buffer (`BytesTapeView::subview`, bench.rs:134-139) -- `data`
 *    is then the BUFFER's first byte, not the window's.
 *  - data[0 .. offsets[count]) must be readable, the bytes in front of offsets[0] included: the kernels read in wide, clamped
 *    windows around a string, never outside [0, offsets[count]), and a raw UTF-8 call or `swh_tape_prepare_*(utf8 = 1)` validates and
 *    decodes that whole range (so the bytes in front of a window must be valid UTF-8 as well).
 *  - Totals are 64-bit with u64 offsets, and up to 2^32 - 1 with u32 offsets (entries at or above 2^31 are plain unsigned values).
 *  - One string holds fewer than 2^30 bytes (hence fewer than 2^30 symbols). A longer one is refused with
 *    swh_unsupported_length_k: by `swh_tape_prepare_*` (and so by every call that prepares its raw tapes: top-k, within, align,
 *    infix, OSA, LCS, partial ratio, Jaro) on the offsets alone, and by the pairwise and cross-product calls on raw tapes as soon as they have
 *    measured the batch (lengths are measured as 64-bit differences: an entry of 2^32 bytes or more does not wrap into a short
 *    one) -- no kernel scores a pair with such a string; the call's outputs may have been written and mean nothing. */
typedef struct swh_tape_u32_t { const uint8_t *data; const uint32_t *offsets; size_t count; } swh_tape_u32_t;
typedef struct swh_tape_u64_t { const uint8_t *data; const uint64_t *offsets; size_t count; } swh_tape_u64_t;

/* ---- Prepared tapes: `BytesTape<u64, UnifiedAlloc>` filled once and `CharsTapeView::try_from(bytes_view)` validated
 *      once, both OUTSIDE the timed closures (bench.rs:292-306), then sub-viewed per iteration (bench.rs:134-139).
 * `swh_tape_prepare_*` makes a tape resident on the scope's device (host tapes are uploaded; device tapes are used in
 * place and must outlive the handle), measures it (count, symbols, longest string) and, with `utf8 != 0`, validates
 * and decodes it to code points -- invalid UTF-8 fails HERE with swh_invalid_utf8_k, as `try_into` does, not in every
 * engine call. Engine calls on prepared views skip the per-call decode and, knowing the longest string, the planning
 * pre-pass and its host round trip. */
typedef struct swh_prepared_s *swh_prepared_t;
typedef struct swh_prepared_info_t {
    size_t count;             /* strings */
    uint64_t bytes, symbols;  /* tape bytes; symbols = bytes, or code points for a UTF-8 tape */
    uint32_t longest;         /* longest string in symbols */
    int utf8, ascii;          /* prepared as UTF-8; every code point is a single byte */
} swh_prepared_info_t;
swh_status_t swh_tape_prepare_u32(swh_scope_t scope, const swh_tape_u32_t *tape, int utf8, swh_prepared_t *prepared,
                                  const char **error);
swh_status_t swh_tape_prepare_u64(swh_scope_t scope, const swh_tape_u64_t *tape, int utf8, swh_prepared_t *prepared,
                                  const char **error);
swh_status_t swh_prepared_info(swh_prepared_t prepared, swh_prepared_info_t *info);
swh_status_t swh_prepared_free(swh_prepared_t prepared);
/* Strings [first, first + count) of a prepared tape: `BytesTapeView::subview(lo, hi)` (bench.rs:134-139). */
typedef struct swh_prepared_view_t { swh_prepared_t tape; size_t first, count; } swh_prepared_view_t;

/* ---- Levenshtein: `LevenshteinDistances::new(&scope, 0, 1, 1, 1)` (bench.rs:382-393). ------ */
typedef struct swh_levenshtein_s *swh_levenshtein_t;
/* Costs are non-negative; gap of length k costs open + (k-1)*extend. */
swh_status_t swh_levenshtein_init(swh_scope_t scope, int match, int mismatch, int open, int extend,
                                  swh_levenshtein_t *engine, const char **error);
swh_status_t swh_levenshtein_free(swh_levenshtein_t engine);
swh_status_t swh_levenshtein_set_algorithm(swh_levenshtein_t engine, swh_algorithm_t algorithm);

/* Pairwise batch, bytes as symbols: out[i] = min(d(a_i, b_i), bound + 1); bound == SWH_UNBOUNDED
 * disables the cutoff. Replaces the per-pair loops `rapidfuzz::levenshtein::distance`
 * (bench.rs:404-423) / `bio::levenshtein` (bench.rs:443-459) and the batched pairwise
 * `cudf ... str.edit_distance` (similarities/bench.py:596-604). `a.count == b.count`.
 * `out_stride_bytes` is the distance between consecutive results (>= 4; 0 means 4). */
swh_status_t swh_levenshtein_pairs_u32tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u32_t *a,
                                           const swh_tape_u32_t *b, uint32_t bound, uint32_t *out,
                                           size_t out_stride_bytes, const char **error);
swh_status_t swh_levenshtein_pairs_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                           const swh_tape_u64_t *b, uint32_t bound, uint32_t *out,
                                           size_t out_stride_bytes, const char **error);
/* Same with Unicode scalar values as symbols: `LevenshteinDistancesUtf8` (bench.rs:386-399),
 * `rapidfuzz::levenshtein<Chars>` (bench.rs:425-441). Invalid UTF-8 -> swh_invalid_utf8_k. */
swh_status_t swh_levenshtein_utf8_pairs_u32tape(swh_levenshtein_t engine, swh_scope_t scope,
                                                const swh_tape_u32_t *a, const swh_tape_u32_t *b, uint32_t bound,
                                                uint32_t *out, size_t out_stride_bytes, const char **error);
swh_status_t swh_levenshtein_utf8_pairs_u64tape(swh_levenshtein_t engine, swh_scope_t scope,
                                                const swh_tape_u64_t *a, const swh_tape_u64_t *b, uint32_t bound,
                                                uint32_t *out, size_t out_stride_bytes, const char **error);
/* Dense cross-product `a.count x b.count`, row-major `size_t`, the literal shape of
 * `engine.compute_into(&scope, AnyBytesTape::View64(q), Some(AnyBytesTape::View64(c)), &mut matrix)`
 * (bench.rs:478-486, :599-603). `b == NULL` means the symmetric self-product. */
swh_status_t swh_levenshtein_cross_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                           const swh_tape_u64_t *b, size_t *out, size_t row_stride_bytes,
                                           const char **error);
swh_status_t swh_levenshtein_utf8_cross_u64tape(swh_levenshtein_t engine, swh_scope_t scope,
                                                const swh_tape_u64_t *a, const swh_tape_u64_t *b, size_t *out,
                                                size_t row_stride_bytes, const char **error);

/* The same calls on prepared views (both tapes prepared on the scope's device, both as bytes or both as UTF-8 -- the
 * symbols are then code points, as for `LevenshteinDistancesUtf8`). `b == NULL` in the cross-product means a x a. */
swh_status_t swh_levenshtein_pairs_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *a,
                                            const swh_prepared_view_t *b, uint32_t bound, uint32_t *out,
                                            size_t out_stride_bytes, const char **error);
swh_status_t swh_levenshtein_cross_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *a,
                                            const swh_prepared_view_t *b, size_t *out, size_t row_stride_bytes,
                                            const char **error);

/* ---- Top-k search: the k nearest candidates of every query (rapidfuzz `process.extract(query, choices, limit=k,
 *      score_cutoff=bound)` with the Levenshtein distance as the scorer, for every query at once). --------------------------
 * For every query i, the k candidates j with the smallest key (d(i, j), j) among those with d(i, j) <= bound:
 *  - ascending by distance; ties break by the SMALLER candidate index, so every row is unique and exactly checkable;
 *  - d is the engine's own cost model (unit costs or match / mismatch / open / extend); symbols are bytes, or code points in
 *    the UTF-8 variant (invalid UTF-8 -> swh_invalid_utf8_k); the prepared variant takes what the tapes were prepared as;
 *  - bound == SWH_UNBOUNDED means no cutoff;
 *  - a row with fewer than k admissible candidates is padded with index 0xFFFFFFFF and distance 0xFFFFFFFF;
 *  - 1 <= k <= SWH_TOPK_MAX; any other k returns swh_invalid_argument_k;
 *  - candidates == NULL means queries x queries, diagonal included (a string's distance to itself is 0);
 *  - candidates->count must be below 0xFFFFFFFF; queries->count x candidates->count has NO 2^32 limit (the matrix is never built);
 *  - `indices` and `distances` are uint32_t arrays of queries->count x k, row-major and contiguous, in host or device memory;
 *  - queries->count == 0 succeeds and does nothing; candidates->count == 0 makes every row padding.
 * The call is synchronous on every scope: on an asynchronous or pipelined scope it first joins the outstanding work (as
 * swh_scope_synchronize) and returns with the results visible. With profiling on, swh_scope_last_timing describes the whole
 * search: `cells` = sum len(q) len(c) over all pairs; `dominant_name` is "cross_topk" for the fused word-sized kernel, or
 * "topk_select/<kernel>" for the general path (the candidates scored in slices, <kernel> the longest scoring kernel). */
#define SWH_TOPK_MAX 64
swh_status_t swh_levenshtein_topk_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *queries,
                                          const swh_tape_u64_t *candidates, size_t k, uint32_t bound,
                                          uint32_t *indices, uint32_t *distances, const char **error);
swh_status_t swh_levenshtein_utf8_topk_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *queries,
                                               const swh_tape_u64_t *candidates, size_t k, uint32_t bound,
                                               uint32_t *indices, uint32_t *distances, const char **error);
swh_status_t swh_levenshtein_topk_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *queries,
                                           const swh_prepared_view_t *candidates, size_t k, uint32_t bound,
                                           uint32_t *indices, uint32_t *distances, const char **error);

/* ---- Range search: EVERY candidate within `bound` edits of every query, as CSR (rapidfuzz `process.extract(query, choices,
 *      score_cutoff=bound, limit=None)` / `process.cdist(..., score_cutoff=bound)` with the Levenshtein distance as the scorer). ----
 * Engines, symbols, tapes and the self-product are those of the top-k calls above; what differs is the result:
 *  - row i holds every candidate j with d(q_i, c_j) <= bound, in ASCENDING j, at entries [row_offsets[i], row_offsets[i + 1]) of
 *    `indices` and `distances`; `distances` holds the true distance, never clamped;
 *  - `row_offsets` has queries->count + 1 entries, row_offsets[0] = 0; the output is bit-for-bit deterministic;
 *  - candidates == NULL means queries x queries, diagonal and both orientations included;
 *  - bound == SWH_UNBOUNDED returns swh_invalid_argument_k (that is the dense cross-product); a bound at or above every possible
 *    distance is accepted and returns every pair;
 *  - counting protocol: `row_offsets` is ALWAYS written in full, with the true counts. `indices` and `distances` (`capacity` entries
 *    each) are written only if row_offsets[count] <= capacity; otherwise they are left untouched and the call still returns
 *    swh_success_k -- the caller compares row_offsets[count] with `capacity`. indices == NULL && distances == NULL && capacity == 0 is
 *    the counting call. One of the two arrays NULL and the other not, both NULL with a capacity, or a NULL `row_offsets`, is
 *    swh_invalid_argument_k and nothing is written;
 *  - candidates->count must be below 0xFFFFFFFF; queries->count x candidates->count has NO 2^32 limit and the hit total is a size_t;
 *    queries->count == 0 writes row_offsets[0] = 0 only; candidates->count == 0 makes every row empty;
 *  - each of the three outputs may be host or device memory, independently;
 *  - two prepared byte tapes must share one offset width, as for top-k; multi-device scopes are treated as top-k treats them.
 * The call is synchronous on every scope (outstanding asynchronous / pipelined work is joined first). The pairs are walked twice --
 * counted, then, if the arrays hold them, stored -- and nothing is kept between the walks but the counts. With profiling on,
 * swh_scope_last_timing describes the whole search: `cells` = sum len(q) len(c) over all pairs, counted once although the pairs of
 * a filled call are walked twice; `dominant_name` is "cross_within" for the fused word-sized kernel, or "within_select/<kernel>"
 * for the general path (<kernel> the longest scoring kernel); on the fused route `bytes` = the two tapes + 12 bytes for every
 * (query, candidate slice) count + the row offsets + 8 bytes per stored hit. */
swh_status_t swh_levenshtein_within_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *queries,
                                            const swh_tape_u64_t *candidates, uint32_t bound, size_t *row_offsets,
                                            uint32_t *indices, uint32_t *distances, size_t capacity, const char **error);
swh_status_t swh_levenshtein_utf8_within_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *queries,
                                                 const swh_tape_u64_t *candidates, uint32_t bound, size_t *row_offsets,
                                                 uint32_t *indices, uint32_t *distances, size_t capacity, const char **error);
swh_status_t swh_levenshtein_within_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *queries,
                                             const swh_prepared_view_t *candidates, uint32_t bound, size_t *row_offsets,
                                             uint32_t *indices, uint32_t *distances, size_t capacity, const char **error);

/* ---- Alignments: the edit operations of every pair (rapidfuzz `Levenshtein.editops`, edlib `task="path"`, bio
 *      `Aligner::global(a, b).operations`), unit costs only. -------------------------------------------------------------
 * For every pair i of a pairwise batch (a->count == b->count, else swh_invalid_argument_k):
 *  - distances[i] = min(d(a_i, b_i), bound + 1), bit-identical to swh_levenshtein_pairs_* on the same pairs and bound;
 *    bound == SWH_UNBOUNDED means no cutoff;
 *  - the operations of pair i are ops[ops_offsets[i] .. ops_offsets[i + 1]), one SWH_OP_* byte each, in forward order;
 *    ops_offsets has count + 1 entries, ops_offsets[0] = 0, and the layout is compact; a pair over the bound gets an empty range;
 *  - for an in-bound pair: #'=' + #'X' + #'D' = len(a_i), #'=' + #'X' + #'I' = len(b_i), and the non-'=' ops number d;
 *  - the script is the CANONICAL one among the optimal ones: walking back over the Wagner-Fischer matrix D from (m, n) to
 *    (0, 0), each cell takes '=' if i, j > 0 and a_i = b_j; else 'X' if i, j > 0 and D[i-1][j-1] + 1 = D[i][j]; else 'D'
 *    if i > 0 and D[i-1][j] + 1 = D[i][j]; else 'I'. kitten -> sitting: "X===X=I"; aa -> a: "D=";
 *  - symbols, and the lengths above, are bytes, or code points in the UTF-8 variant (invalid UTF-8 -> swh_invalid_utf8_k); the
 *    prepared variant takes what the tapes were prepared as;
 *  - ops_capacity must be at least sum len(a_i) + len(b_i) in symbols (the byte totals of the two tapes always are), else
 *    swh_invalid_argument_k and nothing is written;
 *  - a pair with len(a_i) * len(b_i) > SWH_ALIGN_MAX_CELLS makes the call return swh_unsupported_length_k before any output is
 *    written; the message names the first such pair;
 *  - an engine whose costs are not (match 0, mismatch 1, open 1, extend 1) returns swh_not_implemented_k;
 *  - `distances` (uint32_t), `ops_offsets` (size_t, 64-bit) and `ops` (one char per op) may each be in host or device memory;
 *  - count == 0 succeeds and writes only ops_offsets[0] = 0.
 * The call is synchronous on every scope: on an asynchronous or pipelined scope it first joins the outstanding work (as
 * swh_scope_synchronize) and returns with the results visible. With profiling on, swh_scope_last_timing describes the whole call:
 * `cells` = sum len(a_i) len(b_i); `dominant_name` is its longest kernel ("align" for bytes, "align_u32" for code points, when
 * the forward pass and the walk dominate). */
#define SWH_ALIGN_MAX_CELLS (1ull << 30)   /* len(a_i) * len(b_i) accepted per pair */
#define SWH_OP_MATCH '='  /* consumes a symbol of a and of b; they are equal */
#define SWH_OP_SUBST 'X'  /* consumes a symbol of a and of b; they differ */
#define SWH_OP_DEL 'D'    /* consumes a symbol of a only */
#define SWH_OP_INS 'I'    /* consumes a symbol of b only */
swh_status_t swh_levenshtein_align_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                           const swh_tape_u64_t *b, uint32_t bound, uint32_t *distances,
                                           size_t *ops_offsets, char *ops, size_t ops_capacity, const char **error);
swh_status_t swh_levenshtein_utf8_align_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                                const swh_tape_u64_t *b, uint32_t bound, uint32_t *distances,
                                                size_t *ops_offsets, char *ops, size_t ops_capacity, const char **error);
swh_status_t swh_levenshtein_align_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *a,
                                            const swh_prepared_view_t *b, uint32_t bound, uint32_t *distances,
                                            size_t *ops_offsets, char *ops, size_t ops_capacity, const char **error);

/* ---- Infix search: the best approximate occurrence of every pattern in its text (edlib `mode="HW"`, rapidfuzz
 *      `partial_ratio_alignment`, bio `Aligner::semiglobal`), unit costs only. -----------------------------------------------
 * For every pair i of a pairwise batch (patterns->count == texts->count, else swh_invalid_argument_k), pattern p_i of m symbols
 * and text t_i of n symbols:
 *  - d_i = min over 0 <= s <= e <= n of d(p_i, t_i[s..e)), the unit-cost Levenshtein distance to the best substring;
 *    distances[i] = min(d_i, bound + 1); bound == SWH_UNBOUNDED means no cutoff, bound == 0 is exact substring search;
 *  - the occurrence reported is the CANONICAL one: ends[i] is the smallest e for which some s reaches d_i, starts[i] the largest
 *    s <= e with d(p_i, t_i[s..e)) = d_i -- the shortest occurrence that ends there. So an empty pattern gives (0, 0, 0), an empty
 *    text (m, 0, 0), and a pattern that matches nowhere better than by deleting all of it (m, 0, 0).
 *    kitten in "the sitting cat": (2, 5, 10); abc in xxabcxx: (0, 2, 5); lawn in "flaw in law": (1, 1, 4); ab in ba: (1, 0, 1);
 *    aaa in bbb: (3, 0, 0);
 *  - a pair with d_i > bound gets distances[i] = bound + 1 and starts[i] = ends[i] = SWH_INFIX_NONE;
 *  - symbols and positions are bytes, or code points in the UTF-8 variant (invalid UTF-8 -> swh_invalid_utf8_k); the prepared
 *    variant takes what the tapes were prepared as (both of the same kind, any mix of 32- and 64-bit offsets);
 *  - a pattern of more than SWH_INFIX_MAX_PATTERN symbols makes the call return swh_unsupported_length_k before any output is
 *    written; the message names the first such pair. Texts have no limit beyond the tapes' own;
 *  - an engine whose costs are not (match 0, mismatch 1, open 1, extend 1) returns swh_not_implemented_k;
 *  - `distances`, `starts` and `ends` (uint32_t, one entry per pair) may each be in host or device memory;
 *  - count == 0 succeeds and writes nothing.
 * The call is synchronous on every scope: on an asynchronous or pipelined scope it first joins the outstanding work (as
 * swh_scope_synchronize) and returns with the results visible. With profiling on, swh_scope_last_timing describes the whole call:
 * `cells` = sum m n; `dominant_name` is its longest kernel ("infix" for bytes, "infix_u32" for code points, when the forward
 * pass dominates). The edit script of an occurrence: swh_levenshtein_align_* on p_i against t_i[starts[i]..ends[i]). */
#define SWH_INFIX_MAX_PATTERN 2048u     /* symbols per pattern: one wave's 64 blocks of 32 rows */
#define SWH_INFIX_NONE 0xFFFFFFFFu      /* start / end of a pair whose best occurrence is over the bound */
swh_status_t swh_levenshtein_infix_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *patterns,
                                           const swh_tape_u64_t *texts, uint32_t bound, uint32_t *distances, uint32_t *starts,
                                           uint32_t *ends, const char **error);
swh_status_t swh_levenshtein_utf8_infix_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *patterns,
                                                const swh_tape_u64_t *texts, uint32_t bound, uint32_t *distances, uint32_t *starts,
                                                uint32_t *ends, const char **error);
swh_status_t swh_levenshtein_infix_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *patterns,
                                            const swh_prepared_view_t *texts, uint32_t bound, uint32_t *distances, uint32_t *starts,
                                            uint32_t *ends, const char **error);

/* ---- Infix search for EVERY occurrence within a bound, as CSR rows (edlib `mode="HW"` `locations`, Myers' "every column whose
 *      score is within k", an approximate grep's line positions), unit costs only. --------------------------------------------
 * Pairs, symbols, tapes and the pattern limit are those of the infix search above; what differs is the result. For pattern p of
 * m symbols and text t of n symbols let D(e) = min over 0 <= s <= e of d(p, t[s..e)) for e = 0 .. n -- the last row of the
 * semi-global Wagner-Fischer matrix, D(0) = m -- and d* = min over e of D(e). A hit is an end e with D(e) <= bound that passes
 * `select`:
 *  - SWH_INFIX_SELECT_ALL: every such e;
 *  - SWH_INFIX_SELECT_BEST: those with D(e) = d* (edlib's `locations`, whose ends are inclusive); the row is empty if d* > bound;
 *  - SWH_INFIX_SELECT_MINIMA: one hit per dip of the score curve -- with D(-1) = D(n + 1) = +infinity, e is reported iff
 *    D(e) <= bound, D(e - 1) > D(e), and the first f > e with D(f) != D(e) has D(f) > D(e): the first column of every plateau that
 *    is a weak local minimum;
 *  - any other `select` is swh_invalid_argument_k.
 * Row i holds pair i's hits in ASCENDING e at entries [row_offsets[i], row_offsets[i + 1]): ends[h] = e (exclusive),
 * distances[h] = D(e), the true value, never clamped, and -- if `starts` is given -- starts[h] = the largest s <= e with
 * d(p, t[s..e)) = D(e), the infix search's rule applied to this end. bound == SWH_UNBOUNDED is accepted and means no cutoff.
 * abc in xxabcxx, bound 1: ALL (2,4,1) (2,5,0) (2,6,1) as (start, end, d), BEST and MINIMA (2,5,0); lawn in "flaw in law", bound 1:
 * ALL (1,4,1) (1,5,1) (8,11,1), MINIMA (1,4,1) (8,11,1); aaa in bbb: nothing at bound 2, ALL (0,0,3) (1,1,3) (2,2,3) (3,3,3) and
 * MINIMA (0,0,3) at bound 3; an empty pattern in abc: ALL (0,0,0) (1,1,0) (2,2,0) (3,3,0), MINIMA (0,0,0). Whenever the infix
 * search's d_i <= bound, its (d_i, starts[i], ends[i]) is the first hit of the BEST row.
 * The counting protocol is that of swh_levenshtein_within_*: `row_offsets` (count + 1 entries, row_offsets[0] = 0) is ALWAYS
 * written in full, with the true counts. `ends` and `distances` (and `starts`; `capacity` entries each) are written only if
 * row_offsets[count] <= capacity; otherwise they are left untouched and the call still returns swh_success_k. starts == ends ==
 * distances == NULL with capacity == 0 is the counting call (one walk). `starts` alone may be NULL: the start pass is skipped.
 * `ends` and `distances` come together; any other NULL mix, or a NULL `row_offsets`, is swh_invalid_argument_k and nothing is
 * written. Each output may be host or device memory, independently; the output is bit-for-bit deterministic.
 * Refusals are the infix search's: a count mismatch, a pattern over SWH_INFIX_MAX_PATTERN symbols (before any output is written;
 * the message names the first such pair), costs other than (0, 1, 1, 1), invalid UTF-8, no device. count == 0 writes
 * row_offsets[0] = 0 only. The call is synchronous on every scope. A filled call walks the texts twice -- counted, then stored --
 * and nothing is kept between the walks but a count per pair (and d* for SELECT_BEST). With profiling on, `cells` = sum m n,
 * counted once; the kernels are stamped "infix_hits" / "infix_hits_u32" (the walks) and "infix_hit_starts" /
 * "infix_hit_starts_u32" (the start pass). */
#define SWH_INFIX_SELECT_ALL 0u
#define SWH_INFIX_SELECT_BEST 1u
#define SWH_INFIX_SELECT_MINIMA 2u
swh_status_t swh_levenshtein_infix_all_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *patterns,
                                               const swh_tape_u64_t *texts, uint32_t bound, uint32_t select, size_t *row_offsets,
                                               uint32_t *starts, uint32_t *ends, uint32_t *distances, size_t capacity,
                                               const char **error);
swh_status_t swh_levenshtein_utf8_infix_all_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *patterns,
                                                    const swh_tape_u64_t *texts, uint32_t bound, uint32_t select, size_t *row_offsets,
                                                    uint32_t *starts, uint32_t *ends, uint32_t *distances, size_t capacity,
                                                    const char **error);
swh_status_t swh_levenshtein_infix_all_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *patterns,
                                                const swh_prepared_view_t *texts, uint32_t bound, uint32_t select, size_t *row_offsets,
                                                uint32_t *starts, uint32_t *ends, uint32_t *distances, size_t capacity,
                                                const char **error);

/* ---- Damerau-Levenshtein (OSA) distances: a swap of two neighbouring symbols costs one edit (rapidfuzz `distance.OSA`,
 *      `process.cdist(..., scorer=OSA.distance)`), unit costs only. -----------------------------------------------------------
 * The optimal-string-alignment distance, also called restricted Damerau-Levenshtein: for a of m symbols and b of n symbols, D is
 * the unit-cost Wagner-Fischer recurrence plus one case -- when i, j >= 2, a[i-1] = b[j-2] and a[i-2] = b[j-1], then also
 * D[i][j] <= D[i-2][j-2] + 1 -- and osa(a, b) = D[m][n]. No substring is edited twice, so this is NOT the unrestricted
 * Damerau-Levenshtein distance. ab / ba: 1; abcd / acbd: 1; kitten / sitting: 3; ca / abc: 3 (unrestricted Damerau gives 2).
 * osa(a, b) = osa(b, a), and osa <= Levenshtein <= 2 osa.
 * Pairs (swh_levenshtein_osa_pairs_*):
 *  - a->count == b->count, else swh_invalid_argument_k;
 *  - out[i] = min(osa(a_i, b_i), bound + 1); bound == SWH_UNBOUNDED means no cutoff;
 *  - `out_stride_bytes` is the distance between consecutive results (>= 4; 0 means 4), as for swh_levenshtein_pairs_*.
 * Cross (swh_levenshtein_osa_cross_*):
 *  - row-major `size_t`, out[i][j] = osa(a_i, b_j), rows `row_stride_bytes` apart (0 means b->count * 8), no bound: the shape of
 *    swh_levenshtein_cross_*;
 *  - b == NULL means a x a: symmetric, with a zero diagonal;
 *  - the matrix is filled in slices of whole rows, so the call's scratch memory does not grow with the matrix.
 * Both:
 *  - symbols are bytes, or code points in the UTF-8 variant (invalid UTF-8 -> swh_invalid_utf8_k); the prepared variant takes
 *    what the tapes were prepared as (both of the same kind, any mix of 32- and 64-bit offsets);
 *  - a pair whose SHORTER string has more than SWH_OSA_MAX_SHORTER symbols makes the call return swh_unsupported_length_k before
 *    any output is written; the message names the first such pair. The longer string has no limit beyond the tapes' own;
 *  - an engine whose costs are not (match 0, mismatch 1, open 1, extend 1) returns swh_not_implemented_k;
 *  - `out` may be in host or device memory;
 *  - count == 0 (an empty matrix) succeeds and writes nothing.
 * The call is synchronous on every scope: on an asynchronous or pipelined scope it first joins the outstanding work (as
 * swh_scope_synchronize) and returns with the results visible. With profiling on, swh_scope_last_timing describes the whole call:
 * `cells` = sum m n; `dominant_name` is its longest kernel ("osa" for bytes, "osa_u32" for code points). */
#define SWH_OSA_MAX_SHORTER 2048u     /* symbols of a pair's shorter string: one wave's 64 blocks of 32 rows */
swh_status_t swh_levenshtein_osa_pairs_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                               const swh_tape_u64_t *b, uint32_t bound, uint32_t *out, size_t out_stride_bytes,
                                               const char **error);
swh_status_t swh_levenshtein_utf8_osa_pairs_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                                    const swh_tape_u64_t *b, uint32_t bound, uint32_t *out, size_t out_stride_bytes,
                                                    const char **error);
swh_status_t swh_levenshtein_osa_pairs_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *a,
                                                const swh_prepared_view_t *b, uint32_t bound, uint32_t *out, size_t out_stride_bytes,
                                                const char **error);
swh_status_t swh_levenshtein_osa_cross_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                               const swh_tape_u64_t *b, size_t *out, size_t row_stride_bytes, const char **error);
swh_status_t swh_levenshtein_utf8_osa_cross_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                                    const swh_tape_u64_t *b, size_t *out, size_t row_stride_bytes, const char **error);
swh_status_t swh_levenshtein_osa_cross_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *a,
                                                const swh_prepared_view_t *b, size_t *out, size_t row_stride_bytes, const char **error);

/* ---- LCS lengths and Indel distances: insertions and deletions only (rapidfuzz `distance.LCSseq`, `distance.Indel`, `fuzz.ratio`,
 *      `process.cdist(..., scorer=ratio)`), unit costs only. ------------------------------------------------------------------
 * For a of m symbols and b of n symbols, LCS(a, b) is the length of their longest common subsequence, and the Indel distance
 * indel(a, b) = m + n - 2 LCS(a, b) is the least number of single-symbol insertions and deletions that turn a into b (a
 * substitution counts as two: the Levenshtein distance at costs match 0, mismatch 2, open 1, extend 1). Both are symmetric.
 * rapidfuzz's `fuzz.ratio` is the normalised form 100 (1 - indel / (m + n)) = 200 LCS / (m + n), and 100 where m + n = 0; callers
 * compute it from the two outputs.
 *   kitten / sitting: LCS 4 (ittn), indel 5, ratio 61.53...;  ab / ba: 1, 2, 50;  abc / abc: 3, 0, 100;
 *   "" / "": 0, 0, 100;  abc / "": 0, 3, 0.
 * Pairs (swh_levenshtein_lcs_pairs_*):
 *  - a->count == b->count, else swh_invalid_argument_k;
 *  - indel[i] = min(m + n - 2 LCS(a_i, b_i), bound + 1); bound == SWH_UNBOUNDED means no cutoff;
 *  - lcs[i] = LCS(a_i, b_i), never clamped by the bound;
 *  - either of `indel` and `lcs` may be NULL (that output is not wanted), not both: swh_invalid_argument_k;
 *  - `out_stride_bytes` is the distance between consecutive results of either output (>= 4; 0 means 4); each output may be in host
 *    or device memory, independently of the other.
 * Cross (swh_levenshtein_lcs_cross_*):
 *  - row-major `size_t`, indel[i][j] and lcs[i][j] of (a_i, b_j), rows `row_stride_bytes` apart in both matrices (0 means
 *    b->count * 8), no bound: the shape of swh_levenshtein_osa_cross_*; either matrix may be NULL, not both;
 *  - b == NULL means a x a: symmetric, the diagonal holds indel = 0 and lcs = len(a_i);
 *  - the matrix is filled in slices of whole rows, so the call's scratch memory does not grow with the matrix.
 * Both:
 *  - symbols are bytes, or code points in the UTF-8 variant (invalid UTF-8 -> swh_invalid_utf8_k); the prepared variant takes
 *    what the tapes were prepared as (both of the same kind, any mix of 32- and 64-bit offsets);
 *  - a pair whose SHORTER string has more than SWH_LCS_MAX_SHORTER symbols makes the call return swh_unsupported_length_k before
 *    any output is written; the message names the first such pair. The longer string has no limit beyond the tapes' own;
 *  - an engine whose costs are not (match 0, mismatch 1, open 1, extend 1) returns swh_not_implemented_k;
 *  - count == 0 (an empty matrix) succeeds and writes nothing.
 * The call is synchronous on every scope: on an asynchronous or pipelined scope it first joins the outstanding work (as
 * swh_scope_synchronize) and returns with the results visible. With profiling on, swh_scope_last_timing describes the whole call:
 * `cells` = sum m n; `dominant_name` is its longest kernel ("lcs" for bytes, "lcs_u32" for code points). */
#define SWH_LCS_MAX_SHORTER 2048u     /* symbols of a pair's shorter string: one wave's 64 blocks of 32 rows */
swh_status_t swh_levenshtein_lcs_pairs_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                               const swh_tape_u64_t *b, uint32_t bound, uint32_t *indel, uint32_t *lcs,
                                               size_t out_stride_bytes, const char **error);
swh_status_t swh_levenshtein_utf8_lcs_pairs_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                                    const swh_tape_u64_t *b, uint32_t bound, uint32_t *indel, uint32_t *lcs,
                                                    size_t out_stride_bytes, const char **error);
swh_status_t swh_levenshtein_lcs_pairs_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *a,
                                                const swh_prepared_view_t *b, uint32_t bound, uint32_t *indel, uint32_t *lcs,
                                                size_t out_stride_bytes, const char **error);
swh_status_t swh_levenshtein_lcs_cross_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                               const swh_tape_u64_t *b, size_t *indel, size_t *lcs, size_t row_stride_bytes,
                                               const char **error);
swh_status_t swh_levenshtein_utf8_lcs_cross_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                                    const swh_tape_u64_t *b, size_t *indel, size_t *lcs, size_t row_stride_bytes,
                                                    const char **error);
swh_status_t swh_levenshtein_lcs_cross_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *a,
                                                const swh_prepared_view_t *b, size_t *indel, size_t *lcs, size_t row_stride_bytes,
                                                const char **error);

/* ---- Partial ratio: the best Indel ratio of the shorter string against the windows of the longer one (rapidfuzz
 *      `fuzz.partial_ratio`, `fuzz.partial_ratio_alignment`, `process.cdist(..., scorer=fuzz.partial_ratio)`), unit costs only. ----
 * Unlike the infix search above -- a Levenshtein distance to the best substring of ANY length -- this is the best `fuzz.ratio` over
 * windows of the needle's length: lawn in "flaw in law" is infix (1, 1, 4), but partial window (8, 11) with score 85.71.
 * For a pair (a, b) the needle p (m symbols) is the shorter string and the haystack t (n symbols) the longer one. The windows of t
 * are t[max(0, o) .. min(n, o + m)) for every offset o in -(m - 1) .. n - 1: every full-length window and the shorter prefixes and
 * suffixes an overhanging needle leaves, n + m - 1 windows, each of some length l.
 *  - A window scores 200 L / (m + l), L = LCS(p, window): `fuzz.ratio(p, window)`.
 *  - Windows are compared exactly, as the rationals L / (m + l) (cross-multiplied in 64-bit integers); among equals the window of
 *    the smallest offset o is the result (rapidfuzz's scan order with strict improvement).
 *  - len(a) < len(b): the needle is a, the window lies in b, side 0. len(a) > len(b): the needle is b, the window lies in a, side 1.
 *    len(a) == len(b): the two directions differ (abbb / abab: 75 with needle a, 85.71 with needle b) and both are evaluated; side 1
 *    wins only on a strictly larger rational.
 *  - If no window shares a symbol with the needle: L = 0, window (0, m), the side as above.
 *  - m == 0: L = 0, window (0, 0), the side as above (two empty strings: side 0); the score is 100 if n == 0, else 0.
 * Per pair: lcs = L, starts / ends = the window in the haystack (in symbols), sides = 0 or 1. Callers evaluate the float64 score
 * 100 * (2 L) / (m + (end - start)) from them (and the m == 0 rule).
 *      a / b                      score     L  start end side
 *      kitten / the sitting cat   66.66...  4  4     10  0
 *      abc / xxabcxx              100       3  2     5   0
 *      lawn / flaw in law         85.714... 3  8     11  0
 *      yankees / new york yankees 100       7  9     16  0
 *      ab / ba                    66.66...  1  0     1   0    (a three-way tie: the smallest offset)
 *      abcx / xabc                85.714... 3  1     4   0
 *      aab / baa                  80        2  1     3   0
 *      abbb / abab                85.714... 3  0     3   1    (the window lies in a)
 *      aaa / bbb                  0         0  0     3   0
 *      "" / ""                    100       0  0     0   0
 *      "" / abc                   0         0  0     0   0
 * rapidfuzz filters windows by character set before it scores them and may therefore report a later window of the same score:
 * the scores correspond, the windows only up to ties.
 * Pairs (swh_levenshtein_partial_pairs_*):
 *  - a->count == b->count, else swh_invalid_argument_k;
 *  - any of the four outputs may be NULL (that output is not wanted), not all: swh_invalid_argument_k;
 *  - `out_stride_bytes` is the distance between consecutive results of every output (>= 4; 0 means 4); each output may be in host
 *    or device memory, independently of the others.
 * Cross (swh_levenshtein_partial_cross_*):
 *  - four row-major `size_t` matrices, [i][j] of (a_i, b_j), rows `row_stride_bytes` apart in all of them (0 means b->count * 8);
 *    any may be NULL, not all;
 *  - b == NULL means a x a: the diagonal holds L = len(a_i), window (0, len(a_i)), side 0;
 *  - the matrices are filled in slices of whole rows; the call's scratch memory follows the slice's windows, not the matrix.
 * Both:
 *  - symbols are bytes, or code points in the UTF-8 variant (invalid UTF-8 -> swh_invalid_utf8_k); the prepared variant takes
 *    what the tapes were prepared as (both of the same kind, any mix of 32- and 64-bit offsets);
 *  - a pair whose SHORTER string has more than SWH_PARTIAL_MAX_NEEDLE symbols makes the call return swh_unsupported_length_k before
 *    any output is written; the message names the first such pair. The haystack has no limit beyond the tapes' own;
 *  - an engine whose costs are not (match 0, mismatch 1, open 1, extend 1) returns swh_not_implemented_k;
 *  - there is no score cutoff;
 *  - count == 0 (an empty matrix) succeeds and writes nothing.
 * The call is synchronous on every scope: on an asynchronous or pipelined scope it first joins the outstanding work (as
 * swh_scope_synchronize) and returns with the results visible. The same inputs give the same bytes on every run. With profiling on,
 * swh_scope_last_timing describes the whole call: `cells` = sum m n (the nominal accounting: the windows cost about m times that);
 * `dominant_name` is its longest kernel ("partial" for bytes, "partial_u32" for code points). */
#define SWH_PARTIAL_MAX_NEEDLE 2048u  /* symbols of a pair's shorter string: one wave's 64 blocks of 32 rows */
swh_status_t swh_levenshtein_partial_pairs_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                                   const swh_tape_u64_t *b, uint32_t *lcs, uint32_t *starts, uint32_t *ends,
                                                   uint32_t *sides, size_t out_stride_bytes, const char **error);
swh_status_t swh_levenshtein_utf8_partial_pairs_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                                        const swh_tape_u64_t *b, uint32_t *lcs, uint32_t *starts, uint32_t *ends,
                                                        uint32_t *sides, size_t out_stride_bytes, const char **error);
swh_status_t swh_levenshtein_partial_pairs_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *a,
                                                    const swh_prepared_view_t *b, uint32_t *lcs, uint32_t *starts, uint32_t *ends,
                                                    uint32_t *sides, size_t out_stride_bytes, const char **error);
swh_status_t swh_levenshtein_partial_cross_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                                   const swh_tape_u64_t *b, size_t *lcs, size_t *starts, size_t *ends, size_t *sides,
                                                   size_t row_stride_bytes, const char **error);
swh_status_t swh_levenshtein_utf8_partial_cross_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                                        const swh_tape_u64_t *b, size_t *lcs, size_t *starts, size_t *ends,
                                                        size_t *sides, size_t row_stride_bytes, const char **error);
swh_status_t swh_levenshtein_partial_cross_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *a,
                                                    const swh_prepared_view_t *b, size_t *lcs, size_t *starts, size_t *ends,
                                                    size_t *sides, size_t row_stride_bytes, const char **error);

/* ---- Token-sorted tapes, token_sort_ratio and token_set_ratio (rapidfuzz `fuzz.token_sort_ratio`, `fuzz.token_set_ratio`). --------
 * Tokens are the maximal runs of non-whitespace symbols of a string: what Python's split() without an argument returns.
 *  - On a tape prepared with utf8 = 0 whitespace is the six bytes of bytes.split(): 09 0A 0B 0C 0D 20.
 *  - On a tape prepared with utf8 = 1 it is the 29 code points of str.isspace(): U+0009-000D, U+001C-001F, U+0020, U+0085, U+00A0,
 *    U+1680, U+2000-200A, U+2028, U+2029, U+202F, U+205F, U+3000 -- in UTF-8 the single bytes 09-0D and 1C-20, C2 85, C2 A0,
 *    E1 9A 80, E2 80 80..8A, E2 80 A8, E2 80 A9, E2 80 AF, E2 81 9F and E3 80 80. U+200B, U+180E, U+FEFF, U+0084 and U+00A1 are no
 *    whitespace; neither are 1C-1F and the raw bytes 85 and A0 on a byte tape.
 * Tokens are ordered by symbol value, a proper prefix first: Python's sorted() on bytes or str (on valid UTF-8 byte order is
 * code-point order). The two normal forms of a string s:
 *  - SWH_TOKENS_SORTED: b" ".join(sorted(s.split())), duplicates kept;
 *  - SWH_TOKENS_UNIQUE: b" ".join(sorted(set(s.split()))).
 * The separator is one 0x20, none leads or trails, a string without a token becomes the empty string, and a normal form is never
 * longer than its string.
 *
 * swh_tape_token_sort derives the tape of normal forms of a prepared view's strings on the device. The result is a new prepared tape
 * like any other: in the view's mode, with offsets[0] = 0 and offsets of the view's tape's width, measured (swh_prepared_info),
 * accepted by every call that takes a prepared view, and the owner of its buffers -- freeing the source does not touch it. So
 *      token_sort_ratio(a, b)         = ratio (swh_levenshtein_lcs_pairs_prepared) of the two SWH_TOKENS_SORTED tapes,
 *      cdist(scorer=token_sort_ratio) = swh_levenshtein_lcs_cross_prepared of them,
 *      process.extract(scorer=token_sort_ratio) = swh_levenshtein_extract_prepared(SWH_SCORER_RATIO) of them,
 *      partial_token_sort_ratio       = swh_levenshtein_partial_pairs_prepared of them.
 *  - a string of more than SWH_TOKEN_MAX_BYTES bytes makes the call return swh_unsupported_length_k, the message naming the first such
 *    string of the view; *out is NULL then;
 *  - a view of no strings gives a valid empty tape; a `form` that is neither of the two is swh_invalid_argument_k;
 *  - the call is synchronous on every scope, and the same input gives the same bytes on every run.
 * swh_prepared_read copies a prepared tape's count + 1 byte offsets, rebased so that offsets[0] = 0, and -- unless `data` is NULL --
 * its offsets[count] bytes to the host: call it with NULL first to size `data`. It reads any prepared tape, derived or not.
 *
 * token_set_ratio. Let A and B be the token sets of a and b, S the SWH_TOKENS_UNIQUE join of A & B, X that of A - B and Y that of
 * B - A, s, x and y their lengths in symbols (bytes, or code points on a UTF-8 tape) and L = LCS(X, Y). The calls return the four
 * integers per pair -- sect = s, ab = x, ba = y, lcs = L -- and callers evaluate the float64 score, with
 * q(d, t) = t > 0 ? 100.0 * (double)(t - d) / (double)t : 100.0:
 *      if s == 0 and (x == 0 or y == 0): 0.0        (a side without tokens; two empty strings score 0, not 100)
 *      elif x == 0 or y == 0:            100.0      (one token set contains the other)
 *      else: e = s > 0 ? 1 : 0; sab = s + e + x; sba = s + e + y;
 *            r = q(x + y - 2 L, sab + sba);
 *            score = s == 0 ? r : max(r, q(e + x, s + sab), q(e + y, s + sba))
 *      a / b                                                                     token_sort   s  x  y  L   token_set
 *      fuzzy was a bear / fuzzy fuzzy was a bear                                 84.2105...   16 0  0  0   100
 *      mariners vs angels / los angeles angels of anaheim at seattle mariners    50.7462...   15 2  33 1   90.9090...
 *      york new / new jersey                                                     33.3333...   3  4  6  1   55.5555...
 *      a a b / b c                                                               25           1  1  1  0   66.6666...
 *      "  b  a " / "a\tb\n"                                                      100          3  0  0  0   100
 *      "" / ""                                                                   100          0  0  0  0   0
 *      "   " / a                                                                 0            0  0  1  0   0
 * Pairs (swh_levenshtein_token_set_pairs_*):
 *  - the tapes may be any tapes: the call derives the SWH_TOKENS_UNIQUE forms itself, and uses a prepared tape that
 *    swh_tape_token_sort made in that form as it stands; every string holds at most SWH_TOKEN_MAX_BYTES bytes;
 *  - a->count == b->count, else swh_invalid_argument_k;
 *  - any of the four outputs may be NULL, not all: swh_invalid_argument_k; `out_stride_bytes` is the distance between consecutive
 *    results of every output (>= 4; 0 means 4); each output may be in host or device memory;
 *  - a pair of which the SHORTER normal form has more than SWH_LCS_MAX_SHORTER symbols makes the call return
 *    swh_unsupported_length_k before any output is written; the message names the first such pair and both lengths;
 *  - an engine whose costs are not (match 0, mismatch 1, open 1, extend 1) returns swh_not_implemented_k; invalid UTF-8 is
 *    swh_invalid_utf8_k; count == 0 succeeds and writes nothing; the call is synchronous on every scope. */
#define SWH_TOKEN_MAX_BYTES 4096u     /* bytes of a string whose tokens are sorted: one wave holds it and its token table in LDS */
#define SWH_TOKENS_SORTED 0
#define SWH_TOKENS_UNIQUE 1
swh_status_t swh_tape_token_sort(swh_scope_t scope, const swh_prepared_view_t *view, int form, swh_prepared_t *out, const char **error);
swh_status_t swh_prepared_read(swh_scope_t scope, swh_prepared_t prepared, void *data, size_t *offsets, const char **error);
swh_status_t swh_levenshtein_token_set_pairs_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                                     const swh_tape_u64_t *b, uint32_t *sect, uint32_t *ab, uint32_t *ba, uint32_t *lcs,
                                                     size_t out_stride_bytes, const char **error);
swh_status_t swh_levenshtein_utf8_token_set_pairs_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                                          const swh_tape_u64_t *b, uint32_t *sect, uint32_t *ab, uint32_t *ba,
                                                          uint32_t *lcs, size_t out_stride_bytes, const char **error);
swh_status_t swh_levenshtein_token_set_pairs_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *a,
                                                      const swh_prepared_view_t *b, uint32_t *sect, uint32_t *ab, uint32_t *ba,
                                                      uint32_t *lcs, size_t out_stride_bytes, const char **error);

/* ---- Jaro and Jaro-Winkler similarities (rapidfuzz `distance.Jaro` / `distance.JaroWinkler`, jellyfish `jaro_similarity` /
 *      `jaro_winkler_similarity`), unit-cost engines only. The calls return the integer counts; callers evaluate the two
 *      similarity expressions below. ---------------------------------------------------------------------------------------------
 * Let a hold m symbols and b hold n symbols (bytes, or code points in the UTF-8 variant).
 *  - Search range: R = max(0, max(m, n) / 2 - 1), integer division.
 *  - Matching: a's symbols are taken in order, i = 0 .. m - 1. For each, the smallest j with max(0, i - R) <= j <= min(n - 1, i + R),
 *    b[j] == a[i] and b[j] not yet flagged is looked for; if there is one, b[j] is flagged and a[i] is matched. This is the order
 *    of Winkler's strcmp95 and of jellyfish: the outer loop runs over the FIRST string. The definition is one-sided -- a drives, b
 *    is flagged -- and the library never swaps the two sides of a pair.
 *  - Counts: M is the number of matches; h is the number of k < M at which the k-th matched symbol of a (in a's order) differs
 *    from the k-th flagged symbol of b (in b's order); t = h / 2, floored (h can be odd: bbcaba / cab gives M = 3, h = 3, t = 1);
 *    l is the length of the common prefix of a and b, at most 4.
 *  - Similarities, in IEEE double, evaluated exactly as written:
 *        jaro = 1.0 if m = n = 0;  0.0 if M = 0;  otherwise (M / m + M / n + (M - t) / M) / 3.0
 *        jaro_winkler = jaro + l * p * (1.0 - jaro) if jaro > 0.7, else jaro;  p the prefix weight, 0 <= p <= 0.25, usually 0.1
 *      a / b                    M  t  jaro                 jaro_winkler (p = 0.1)
 *      MARTHA / MARHTA          6  1  0.9444444444444445   0.9611111111111111
 *      DWAYNE / DUANE           4  0  0.8222222222222223   0.8400000000000001
 *      DIXON / DICKSONX         4  0  0.7666666666666666   0.8133333333333332
 *      CRATE / TRACE            3  0  0.7333333333333334   0.7333333333333334
 *      JELLYFISH / SMELLYFISH   8  0  0.8962962962962964   0.8962962962962964  (l = 0)
 *      ab / ba                  0  0  0.0                  0.0                 (R = 0)
 *      a / a                    1  0  1.0                  1.0
 *      a / b                    0  0  0.0                  0.0
 *      "" / ""                  0  0  1.0                  1.0
 * Pairs (swh_levenshtein_jaro_pairs_*):
 *  - a->count == b->count, else swh_invalid_argument_k;
 *  - matches[i] = M, transpositions[i] = t, prefix[i] = l of (a_i, b_i);
 *  - any of the three outputs may be NULL (that output is not wanted), not all: swh_invalid_argument_k;
 *  - `out_stride_bytes` is the distance between consecutive results of every output (a multiple of 4; 0 means 4; anything else is
 *    swh_invalid_argument_k); each output may be in host or device memory, independently of the others.
 * Cross (swh_levenshtein_jaro_cross_*):
 *  - row-major `size_t`, [i][j] of (a_i, b_j) -- a_i drives, b_j is flagged --, rows `row_stride_bytes` apart in all matrices (a
 *    multiple of 8, at least b->count * 8; 0 means b->count * 8); any matrix may be NULL, not all;
 *  - b == NULL means a x a: the diagonal holds M = len(a_i), t = 0, l = min(len(a_i), 4);
 *  - the matrix is filled in slices of whole rows, so the call's scratch memory does not grow with the matrix.
 * Both:
 *  - symbols are bytes, or code points in the UTF-8 variant (invalid UTF-8 -> swh_invalid_utf8_k); the prepared variant takes
 *    what the tapes were prepared as (both of the same kind, any mix of 32- and 64-bit offsets);
 *  - a pair either of whose strings has more than SWH_JARO_MAX_LENGTH symbols makes the call return swh_unsupported_length_k before
 *    any output is written; the message names the first such pair and both lengths;
 *  - an engine whose costs are not (match 0, mismatch 1, open 1, extend 1) returns swh_not_implemented_k;
 *  - count == 0 (an empty matrix) succeeds and writes nothing.
 * The call is synchronous on every scope: on an asynchronous or pipelined scope it first joins the outstanding work (as
 * swh_scope_synchronize) and returns with the results visible. With profiling on, swh_scope_last_timing describes the whole call:
 * `cells` = sum m n; `dominant_name` is its longest kernel ("jaro" for bytes, "jaro_u32" for code points). */
#define SWH_JARO_MAX_LENGTH 2048u     /* symbols of either string of a pair: one wave's 64 blocks of 32 rows */
swh_status_t swh_levenshtein_jaro_pairs_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                                const swh_tape_u64_t *b, uint32_t *matches, uint32_t *transpositions,
                                                uint32_t *prefix, size_t out_stride_bytes, const char **error);
swh_status_t swh_levenshtein_utf8_jaro_pairs_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                                     const swh_tape_u64_t *b, uint32_t *matches, uint32_t *transpositions,
                                                     uint32_t *prefix, size_t out_stride_bytes, const char **error);
swh_status_t swh_levenshtein_jaro_pairs_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *a,
                                                 const swh_prepared_view_t *b, uint32_t *matches, uint32_t *transpositions,
                                                 uint32_t *prefix, size_t out_stride_bytes, const char **error);
swh_status_t swh_levenshtein_jaro_cross_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                                const swh_tape_u64_t *b, size_t *matches, size_t *transpositions, size_t *prefix,
                                                size_t row_stride_bytes, const char **error);
swh_status_t swh_levenshtein_utf8_jaro_cross_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                                     const swh_tape_u64_t *b, size_t *matches, size_t *transpositions, size_t *prefix,
                                                     size_t row_stride_bytes, const char **error);
swh_status_t swh_levenshtein_jaro_cross_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *a,
                                                 const swh_prepared_view_t *b, size_t *matches, size_t *transpositions, size_t *prefix,
                                                 size_t row_stride_bytes, const char **error);

/* ---- Score search: the k best candidates of every query by an OSA, Indel, LCS, ratio, Jaro or Jaro-Winkler score (rapidfuzz
 *      `process.extract(query, choices, scorer=..., limit=k, score_cutoff=cutoff)`, for every query at once), unit-cost engines
 *      only. The top-k search above is the Levenshtein form of this call; what differs is the score, a float64. ------------------
 *      scorer                     score (float64)                                                            better is
 *      SWH_SCORER_OSA             the OSA distance d                                                         smaller
 *      SWH_SCORER_INDEL           the Indel distance m + n - 2 LCS                                           smaller
 *      SWH_SCORER_LCS             the LCS length L                                                           larger
 *      SWH_SCORER_RATIO           100.0 * (2.0 * L) / (d + 2.0 * L), d the Indel distance; 100.0 if m = n = 0   larger
 *      SWH_SCORER_JARO            the Jaro expression above, as written                                      larger
 *      SWH_SCORER_JARO_WINKLER    the Jaro-Winkler expression above with prefix weight p, as written         larger
 * For every query i, the k candidates j with the best key (score(i, j), j) among those that pass the cutoff:
 *  - best score first; equal scores -- equal as float64, nothing narrower -- in order of the SMALLER candidate index;
 *  - a score leaves with the 64 bits that the expressions above, evaluated in IEEE double operation by operation as written, give
 *    for the counts the pairwise and cross calls return for that pair (the query drives the Jaro matching, the candidate is
 *    flagged; the sides are never swapped);
 *  - `cutoff_bits` is the cutoff, a double, as its binary64 bit pattern (what memcpy of the double into a uint64_t gives): the
 *    distance scorers admit d <= cutoff, the similarity scorers s >= cutoff, a score at the cutoff is admitted; +infinity
 *    (distances) or 0.0 (similarities) means no cutoff; a NaN or a negative cutoff returns swh_invalid_argument_k;
 *  - `prefix_weight_bits` is p, a double passed the same way, 0 <= p <= 0.25, else swh_invalid_argument_k; the scorers other than
 *    SWH_SCORER_JARO_WINKLER ignore it;
 *  - 1 <= k <= SWH_TOPK_MAX and a scorer from the table; anything else returns swh_invalid_argument_k;
 *  - a row with fewer than k admitted candidates is padded with index 0xFFFFFFFF and a score whose 64 bits are all ones (a quiet
 *    NaN: what memset 0xFF writes);
 *  - candidates == NULL means queries x queries, diagonal included;
 *  - candidates->count must be below 0xFFFFFFFF; queries->count x candidates->count has NO 2^32 limit: the pairs are scored in
 *    slices of rows and columns, and the call's scratch memory does not grow with their number;
 *  - `indices` is a uint32_t array and `scores` a double array (`double[queries->count * k]`), both of queries->count x k,
 *    row-major and contiguous, each in host or device memory;
 *  - queries->count == 0 succeeds and does nothing; candidates->count == 0 makes every row padding;
 *  - symbols are bytes, or code points in the UTF-8 variant (invalid UTF-8 -> swh_invalid_utf8_k); the prepared variant takes
 *    what the tapes were prepared as;
 *  - the families' length limits hold: a pair whose SHORTER string has more than SWH_OSA_MAX_SHORTER symbols (OSA, Indel, LCS,
 *    ratio), or either of whose strings has more than SWH_JARO_MAX_LENGTH (Jaro, Jaro-Winkler), makes the call return
 *    swh_unsupported_length_k before any output is written; the message names such a (query, candidate) pair and both lengths;
 *  - an engine whose costs are not (match 0, mismatch 1, open 1, extend 1) returns swh_not_implemented_k.
 * Worked row: query MARTHA, candidates (MARHTA, DWAYNE, MARTHA, MARTHA), SWH_SCORER_JARO_WINKLER, p = 0.1, k = 3, no cutoff:
 * indices 2, 3, 0 and scores 1.0, 1.0, 0.9611111111111111.
 * The call is synchronous on every scope, as the other searches are. With profiling on, swh_scope_last_timing describes the whole
 * search: `cells` = sum m n over all pairs; `dominant_name` is "extract_select/<kernel>", <kernel> the scoring kernel ("osa",
 * "lcs", "jaro", or their "_u32" forms for code points) and `dominant_ms` its time over all slices. */
#define SWH_SCORER_OSA 0
#define SWH_SCORER_INDEL 1
#define SWH_SCORER_LCS 2
#define SWH_SCORER_RATIO 3
#define SWH_SCORER_JARO 4
#define SWH_SCORER_JARO_WINKLER 5
swh_status_t swh_levenshtein_extract_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *queries,
                                             const swh_tape_u64_t *candidates, int scorer, size_t k, uint64_t cutoff_bits,
                                             uint64_t prefix_weight_bits, uint32_t *indices, void *scores, const char **error);
swh_status_t swh_levenshtein_utf8_extract_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *queries,
                                                  const swh_tape_u64_t *candidates, int scorer, size_t k, uint64_t cutoff_bits,
                                                  uint64_t prefix_weight_bits, uint32_t *indices, void *scores,
                                                  const char **error);
swh_status_t swh_levenshtein_extract_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *queries,
                                              const swh_prepared_view_t *candidates, int scorer, size_t k, uint64_t cutoff_bits,
                                              uint64_t prefix_weight_bits, uint32_t *indices, void *scores, const char **error);

/* ---- Score range search: EVERY candidate whose score passes the cutoff, as CSR (rapidfuzz `process.extract(query, choices,
 *      scorer=..., score_cutoff=cutoff, limit=None)` / `process.cdist(..., score_cutoff=cutoff)`, for every query at once),
 *      unit-cost engines only. The call takes its scores and its admission rule from the score search above and its result shape
 *      and counting protocol from the range search (swh_levenshtein_within_*). -------------------------------------------------
 * Scores and admission, as in swh_levenshtein_extract_*:
 *  - `scorer` is one of SWH_SCORER_*; a score leaves with exactly the 64 bits the score search gives for that pair -- the bits of
 *    the table's expressions, evaluated in IEEE double operation by operation as written, on the counts the pairwise and cross
 *    calls return (the query drives the Jaro matching, the candidate is flagged; the sides are never swapped);
 *  - `cutoff_bits` is the cutoff, a double, as its binary64 bit pattern: the distance scorers admit d <= cutoff, the similarity
 *    scorers s >= cutoff, a score at the cutoff is admitted -- any cutoff admits the same pairs here and in the score search;
 *  - a NaN or a negative cutoff returns swh_invalid_argument_k; so does +infinity with a distance scorer (that is the dense
 *    cross-product, as the range search refuses SWH_UNBOUNDED). Any finite cutoff is accepted: a similarity cutoff of 0.0 returns
 *    every pair;
 *  - `prefix_weight_bits` is p, a double passed the same way, 0 <= p <= 0.25, else swh_invalid_argument_k; the scorers other than
 *    SWH_SCORER_JARO_WINKLER ignore it;
 *  - the families' length limits hold as in the score search (swh_unsupported_length_k, the message names a pair and both
 *    lengths), and an engine whose costs are not (match 0, mismatch 1, open 1, extend 1) returns swh_not_implemented_k: both
 *    before any output is written.
 * Result and counting protocol, as in swh_levenshtein_within_*:
 *  - row i holds every candidate j that passes the cutoff, in ASCENDING j, at entries [row_offsets[i], row_offsets[i + 1]) of
 *    `indices` (uint32_t) and `scores` (double: `double[capacity]`); the output is bit-for-bit deterministic;
 *  - `row_offsets` has queries->count + 1 entries, row_offsets[0] = 0, and is ALWAYS written in full, with the true counts.
 *    `indices` and `scores` (`capacity` entries each) are written only if row_offsets[count] <= capacity; otherwise they are left
 *    untouched and the call still returns swh_success_k -- the caller compares row_offsets[count] with `capacity`.
 *    indices == NULL && scores == NULL && capacity == 0 is the counting call. One of the two arrays NULL and the other not, both
 *    NULL with a capacity, or a NULL `row_offsets`, is swh_invalid_argument_k and nothing is written;
 *  - candidates == NULL means queries x queries, diagonal and both orientations included;
 *  - candidates->count must be below 0xFFFFFFFF; queries->count x candidates->count has NO 2^32 limit and the hit total is a size_t;
 *    queries->count == 0 writes row_offsets[0] = 0 only; candidates->count == 0 makes every row empty;
 *  - each of the three outputs may be host or device memory, independently;
 *  - symbols are bytes, or code points in the UTF-8 variant (invalid UTF-8 -> swh_invalid_utf8_k); the prepared variant takes
 *    what the tapes were prepared as.
 * Worked row: query MARTHA, candidates (MARHTA, DWAYNE, MARTHA, MARTHA), SWH_SCORER_JARO_WINKLER, p = 0.1: cutoff 0.97 gives
 * indices 2, 3 and scores 1.0, 1.0; cutoff 0.9611111111111111 gives indices 0, 2, 3 and scores 0.9611111111111111, 1.0, 1.0.
 * The call is synchronous on every scope. The pairs are walked twice -- counted, then, if the arrays hold them, stored -- and BOTH
 * walks score them: nothing is kept between the walks but a count per query, so a filled call costs about twice the scoring of
 * the score search on the same shape, a counting call about once. The scratch memory does not grow with queries x candidates.
 * With profiling on, swh_scope_last_timing describes the whole search: `cells` = sum m n over all pairs, counted once although the
 * pairs of a filled call are walked twice; `dominant_name` is "extract_within/<kernel>", <kernel> the scoring kernel ("osa",
 * "lcs", "jaro", or their "_u32" forms for code points) and `dominant_ms` its time over all slices of both walks. */
swh_status_t swh_levenshtein_extract_within_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *queries,
                                                    const swh_tape_u64_t *candidates, int scorer, uint64_t cutoff_bits,
                                                    uint64_t prefix_weight_bits, size_t *row_offsets, uint32_t *indices,
                                                    void *scores, size_t capacity, const char **error);
swh_status_t swh_levenshtein_utf8_extract_within_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *queries,
                                                         const swh_tape_u64_t *candidates, int scorer, uint64_t cutoff_bits,
                                                         uint64_t prefix_weight_bits, size_t *row_offsets, uint32_t *indices,
                                                         void *scores, size_t capacity, const char **error);
swh_status_t swh_levenshtein_extract_within_prepared(swh_levenshtein_t engine, swh_scope_t scope, const swh_prepared_view_t *queries,
                                                     const swh_prepared_view_t *candidates, int scorer, uint64_t cutoff_bits,
                                                     uint64_t prefix_weight_bits, size_t *row_offsets, uint32_t *indices,
                                                     void *scores, size_t capacity, const char **error);

/* ---- One batch over the GPUs of a multi-device scope (BASELINE config 5). --------------------------------
 * `swh_sharded_prepare_*`: HOST tapes of equal count are cut into contiguous shards balanced on the prefix sum of
 * len(a_i)*len(b_i) (DP cells, not pair counts); shard r is uploaded to and prepared on device r. The handle is the steady
 * state: every `swh_levenshtein_pairs_sharded` call scores each shard on its device (no exchange during the DP), gathers
 * the u32 distances to the first device with one ncclSend / ncclRecv group over xGMI and copies them to `out` (host or
 * first-device memory, pair order). `swh_scope_shard_timing`: slowest shard and the gather of the last call. */
typedef struct swh_sharded_s *swh_sharded_t;
swh_status_t swh_sharded_prepare_u32tape(swh_scope_t scope, const swh_tape_u32_t *a, const swh_tape_u32_t *b, int utf8,
                                         swh_sharded_t *sharded, const char **error);
swh_status_t swh_sharded_prepare_u64tape(swh_scope_t scope, const swh_tape_u64_t *a, const swh_tape_u64_t *b, int utf8,
                                         swh_sharded_t *sharded, const char **error);
swh_status_t swh_sharded_free(swh_sharded_t sharded);
/* the `devices + 1` pair indices where the shards begin / end */
swh_status_t swh_sharded_cuts(swh_sharded_t sharded, size_t *cuts, size_t capacity);
swh_status_t swh_levenshtein_pairs_sharded(swh_levenshtein_t engine, swh_scope_t scope, swh_sharded_t sharded, uint32_t bound,
                                           uint32_t *out, const char **error);
/* one-shot: shard + upload + score + gather + free */
swh_status_t swh_levenshtein_pairs_sharded_u64tape(swh_levenshtein_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                                   const swh_tape_u64_t *b, uint32_t bound, uint32_t *out, const char **error);
typedef struct swh_shard_timing_t {
    double compute_ms;   /* slowest shard, first kernel start to last kernel end on its device */
    double gather_ms;    /* the RCCL gather on the first device's stream */
    uint64_t cells, pairs;
} swh_shard_timing_t;
swh_status_t swh_scope_shard_timing(swh_scope_t scope, swh_shard_timing_t *timing);

/* ---- Needleman-Wunsch: `NeedlemanWunschScores::new(&scope, &byte_to_class, &class_costs,
 *      open, extend)` (bench.rs:658-670, :985-997); scores are max-plus, gaps usually negative. */
typedef struct swh_nw_s *swh_nw_t;
/* Full 256x256 `i8` substitution matrix, row = symbol of a, column = symbol of b (config C4). */
swh_status_t swh_nw_init(swh_scope_t scope, const int8_t *substitution_256x256, int open, int extend,
                         swh_nw_t *engine, const char **error);
/* The reference's 32-class form (`unary_class_costs`, bench.rs:95-108): expands to 256x256. */
swh_status_t swh_nw_init_classes(swh_scope_t scope, const uint8_t *byte_to_class_256,
                                 const int8_t *class_costs_32x32, int open, int extend, swh_nw_t *engine,
                                 const char **error);
swh_status_t swh_nw_free(swh_nw_t engine);
/* Pairwise batch of global alignment scores (`bio ... Aligner::global(a, b).score`,
 * bench.rs:746-765, batched). */
swh_status_t swh_nw_pairs_u32tape(swh_nw_t engine, swh_scope_t scope, const swh_tape_u32_t *a,
                                  const swh_tape_u32_t *b, int32_t *out, size_t out_stride_bytes,
                                  const char **error);
swh_status_t swh_nw_pairs_u64tape(swh_nw_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                  const swh_tape_u64_t *b, int32_t *out, size_t out_stride_bytes,
                                  const char **error);
/* Cross-product into `isize` (`UnifiedMat<isize>`, bench.rs:814-821, :872-876). */
swh_status_t swh_nw_cross_u64tape(swh_nw_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                  const swh_tape_u64_t *b, ptrdiff_t *out, size_t row_stride_bytes,
                                  const char **error);

swh_status_t swh_nw_pairs_prepared(swh_nw_t engine, swh_scope_t scope, const swh_prepared_view_t *a,
                                   const swh_prepared_view_t *b, int32_t *out, size_t out_stride_bytes, const char **error);
swh_status_t swh_nw_cross_prepared(swh_nw_t engine, swh_scope_t scope, const swh_prepared_view_t *a,
                                   const swh_prepared_view_t *b, ptrdiff_t *out, size_t row_stride_bytes, const char **error);

/* ---- Smith-Waterman: `SmithWatermanScores::new(&scope, &byte_to_class, &class_costs, open, extend)`
 *      (bench.rs:882-963). Local alignment score: max over all cells, floored at 0;
 *      same matrix / gap conventions as Needleman-Wunsch. */
typedef struct swh_sw_s *swh_sw_t;
swh_status_t swh_sw_init(swh_scope_t scope, const int8_t *substitution_256x256, int open, int extend,
                         swh_sw_t *engine, const char **error);
swh_status_t swh_sw_init_classes(swh_scope_t scope, const uint8_t *byte_to_class_256,
                                 const int8_t *class_costs_32x32, int open, int extend, swh_sw_t *engine,
                                 const char **error);
swh_status_t swh_sw_free(swh_sw_t engine);
swh_status_t swh_sw_pairs_u32tape(swh_sw_t engine, swh_scope_t scope, const swh_tape_u32_t *a,
                                  const swh_tape_u32_t *b, int32_t *out, size_t out_stride_bytes,
                                  const char **error);
swh_status_t swh_sw_pairs_u64tape(swh_sw_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                  const swh_tape_u64_t *b, int32_t *out, size_t out_stride_bytes,
                                  const char **error);
swh_status_t swh_sw_cross_u64tape(swh_sw_t engine, swh_scope_t scope, const swh_tape_u64_t *a,
                                  const swh_tape_u64_t *b, ptrdiff_t *out, size_t row_stride_bytes,
                                  const char **error);

swh_status_t swh_sw_pairs_prepared(swh_sw_t engine, swh_scope_t scope, const swh_prepared_view_t *a,
                                   const swh_prepared_view_t *b, int32_t *out, size_t out_stride_bytes, const char **error);
swh_status_t swh_sw_cross_prepared(swh_sw_t engine, swh_scope_t scope, const swh_prepared_view_t *a,
                                   const swh_prepared_view_t *b, ptrdiff_t *out, size_t row_stride_bytes, const char **error);

/* The reference's own call shape -- `compute_into(queries, candidates, &mut matrix)`, bench.rs:478-486 -- over every GPU of a
 * multi-device scope: the queries are cut into row blocks of equal symbol counts, block r and all candidates are prepared on
 * device r, every device fills its rows and copies them straight into `matrix` (host memory, or memory of the first device).
 * No collective: the row blocks are disjoint. Levenshtein engines take bytes or (utf8 = 1) code points. */
typedef struct swh_sharded_cross_s *swh_sharded_cross_t;
swh_status_t swh_sharded_cross_prepare_u64tape(swh_scope_t scope, const swh_tape_u64_t *queries, const swh_tape_u64_t *candidates, int utf8,
                                               swh_sharded_cross_t *product, const char **error);
swh_status_t swh_sharded_cross_free(swh_sharded_cross_t product);
swh_status_t swh_levenshtein_cross_sharded(swh_levenshtein_t engine, swh_scope_t scope, swh_sharded_cross_t product, size_t *matrix,
                                           size_t row_stride_bytes, const char **error);
swh_status_t swh_nw_cross_sharded(swh_nw_t engine, swh_scope_t scope, swh_sharded_cross_t product, ptrdiff_t *matrix, size_t row_stride_bytes,
                                  const char **error);
swh_status_t swh_sw_cross_sharded(swh_sw_t engine, swh_scope_t scope, swh_sharded_cross_t product, ptrdiff_t *matrix, size_t row_stride_bytes,
                                  const char **error);

/* Needleman-Wunsch / Smith-Waterman scores of a sharded batch (swh_sharded_prepare_*): the engine's matrix is cloned to every
 * device of the scope on first use -- the `<Ngpu>` twin of the bench.rs:658-670 / :882-963 rows (the engines'
 * read-only state is replicated); scores gathered to the first device like the distances of swh_levenshtein_pairs_sharded */
swh_status_t swh_nw_pairs_sharded(swh_nw_t engine, swh_scope_t scope, swh_sharded_t sharded, int32_t *out, const char **error);
swh_status_t swh_sw_pairs_sharded(swh_sw_t engine, swh_scope_t scope, swh_sharded_t sharded, int32_t *out, const char **error);

/* ---- Introspection: `log_stringzilla_metadata` (utils.rs:78-92). --------------------------- */
const char *swh_version(void);
/* Comma-separated capability string, e.g. "gfx950,hip,wavefront,bitparallel,banded,utf8,...";
 * "topk" when the swh_levenshtein_topk_* calls are present, "within" when the swh_levenshtein_within_* calls are, "align" when the swh_levenshtein_align_* calls are,
 * "infix" when the swh_levenshtein_infix_* calls are, "osa" when the swh_levenshtein_osa_* calls are,
 * "lcs" when the swh_levenshtein_lcs_* calls are, "partial" when the swh_levenshtein_partial_* calls are, "jaro" when the swh_levenshtein_jaro_* calls are, "extract" when the
 * swh_levenshtein_extract_* calls are, "extract_within" when the swh_levenshtein_extract_within_* calls are. */
const char *swh_capabilities(void);

#ifdef __cplusplus
}
#endif
#endif /* STRINGWARS_AMD_H_ */
