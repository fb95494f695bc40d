// two_tape.hip -- the synchronous two-tape calls of include/stringwars_amd.h: top-k, range, score and score range searches,
// alignments, infix search, the scored families (OSA, LCS / Indel, partial ratio, Jaro) and the token-sorted tapes with token_set_ratio.
// Host code only: the kernels are the families' own files,
// the engine-call path the searches score their slices on is api.hip (api.hpp: what the two files share).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "api.hpp"
#include "within.hpp"
#include "scan.hpp"
#include "align.hpp"
#include "infix.hpp"
#include "osa.hpp"
#include "lcs.hpp"
#include "partial.hpp"
#include "tokens.hpp"
#include "jaro.hpp"
#include "extract.hpp"

using namespace swh;

// ---- the synchronous two-tape calls: one front end ------------------------------------------------------------------------------------
// Top-k and range searches, alignments, infix search and the scored families (OSA, LCS, Jaro) are synchronous on every scope:
// outstanding asynchronous / pipelined work is joined first, and the call runs on the scope itself (not on a pipeline lane) with the
// asynchronous mode held off until it returns. Every export runs its own null tests and argument checks in its own order -- which
// refusal wins is its contract (DESIGN.md lists where the calls differ on purpose) -- and between them resolves its two sides here,
// into the TapePair its *_run takes.
struct TapePair {
    const Prepared *pa = nullptr, *pb = nullptr;   // null where a raw call prepared nothing: every *_run returns before it looks at them
    size_t a_first = 0, a_count = 0, b_first = 0, b_count = 0;
};
struct PreparedOwner {
    Prepared *p = nullptr;
    ~PreparedOwner() { free_prepared(p); }
};
static swh_status_t join_outstanding(Scope *scope, const char **error) {
    if (!scope->async && !scope->pipelined) return swh_success_k;
    return swh_scope_synchronize((swh_scope_t)scope, error);
}

struct HoldSynchronous {
    Scope *scope = nullptr;
    bool async = false, pipelined = false;
    void hold(Scope *s) { scope = s; async = s->async; pipelined = s->pipelined; s->async = false; s->pipelined = false; }
    ~HoldSynchronous() {
        if (scope) { scope->async = async; scope->pipelined = pipelined; }
    }
};
struct TwoTapeCall {
    HoldSynchronous mode;             // declared first, so the scope's mode comes back last: after what the call prepared is freed
    Scope *scope = nullptr;           // set once the call has begun
    PreparedOwner owned_a, owned_b;   // what a raw call prepared: it lives as long as the call
    TapePair pair;

    // joins what is outstanding and holds the scope synchronous until the call returns
    swh_status_t begin(swh_scope_t s, const char **error) {
        const swh_status_t status = join_outstanding((Scope *)s, error);
        if (status != swh_success_k) return status;
        scope = (Scope *)s;
        mode.hold(scope);
        return swh_success_k;
    }
    // Raw tapes, after begin(): the sides named are made resident and measured for the call (prepare_tape: device tapes in place, host
    // tapes uploaded; UTF-8 validated and decoded), so the route is chosen on lengths that are known, not believed. Without `b` the
    // second side is the first. A call without pairs names no side: its pair keeps the counts and null tapes.
    swh_status_t prepare(const swh_tape_u64_t *a, const swh_tape_u64_t *b, bool utf8, bool prepare_a, bool prepare_b, const char **error) {
        pair = TapePair{nullptr, nullptr, 0, a->count, 0, (b ? b : a)->count};
        swh_status_t status = swh_success_k;
        if (prepare_a && (status = prepare_tape(scope, SWH_TAPE(a, 1), utf8, (swh_prepared_t *)&owned_a.p, error)) != swh_success_k) return status;
        if (b && prepare_b && (status = prepare_tape(scope, SWH_TAPE(b, 1), utf8, (swh_prepared_t *)&owned_b.p, error)) != swh_success_k) return status;
        pair.pa = owned_a.p; pair.pb = b ? owned_b.p : owned_a.p;
        return swh_success_k;
    }
    // Prepared views, before the call's own checks: the null tests and the bounds of both. A missing b is a (the self-search, the
    // self-product) where `b_optional`.
    swh_status_t views(const swh_prepared_view_t *a, const swh_prepared_view_t *b, bool b_optional, const char **error) {
        if (!a || !a->tape) return fail(error, swh_invalid_argument_k, "null prepared view");
        const swh_prepared_view_t *bb = (b && b->tape) ? b : (b_optional ? a : nullptr);
        if (!bb) return fail(error, swh_invalid_argument_k, "null prepared view");
        if (!view_fits(a) || !view_fits(bb)) return fail(error, swh_invalid_argument_k, "view exceeds the prepared tape");
        pair = TapePair{(const Prepared *)a->tape, (const Prepared *)bb->tape, a->first, a->count, bb->first, bb->count};
        return swh_success_k;
    }
    // ... and after them: the two tapes go together and live on the scope's device, and the call begins
    swh_status_t begin_on_views(swh_scope_t s, const char **error) {
        const swh_status_t status = check_prepared_pair((Scope *)s, pair.pa, pair.pb, error);
        return status != swh_success_k ? status : begin(s, error);
    }
};

// What every *_run is wrapped in: the previous call's timing is harvested and this call's begins empty; a HIP or allocation failure
// anywhere in `body` becomes the call's status.
template <typename Body> static swh_status_t synchronous_run(Scope *scope, const char **error, Body body) {
    harvest_timing(scope, false);
    scope->stamps_used = 0;
    scope->last_timing = swh_timing_t{};
    try {
        return body();
    } catch (const HipFailure &f) {
        return fail_hip(error, f);
    } catch (const std::bad_alloc &) {
        return fail(error, swh_bad_alloc_k, "host allocation failed");
    }
}

// ---- the phases the *_run bodies share ------------------------------------------------------------------------------------------------
// An output of the caller's that may live on the host. The kernels write a device array: the caller's own in place (a null output
// counts as one: nothing is staged for it), or staging in the call's scratch, which copy_back() sends on -- asynchronously: the call
// waits once, for all its outputs. Contiguous outputs only (scored_run copies its strided ones itself).
template <typename T> struct Staged {
    T *out; bool on_device;
    T *dev = nullptr;   // what to launch on, once placed
    explicit Staged(T *caller) : out(caller), on_device(is_device_pointer(caller)) {}
    size_t need(size_t n) const { return on_device ? 0 : pad(n * sizeof(T)); }   // of the scratch
    T *place(Carver &sc, size_t n) { return dev = on_device ? out : sc.take<T>(n); }
    void copy_back(hipStream_t stream, size_t n) const {
        if (!on_device) SWH_HIP_CHECK(hipMemcpyAsync(out, dev, n * sizeof(T), hipMemcpyDeviceToHost, stream));
    }
    void fill_zero(hipStream_t stream, size_t n) const {      // "no row, or every row empty", where the caller's array is; waits
        if (on_device) { SWH_HIP_CHECK(hipMemsetAsync(out, 0, n * sizeof(T), stream)); SWH_HIP_CHECK(hipStreamSynchronize(stream)); }
        else memset(out, 0, n * sizeof(T));
    }
    void fill_padding(hipStream_t stream, size_t n) const {   // "every row is padding": all 0xFF, where the caller's array is
        if (on_device) SWH_HIP_CHECK(hipMemsetAsync(out, 0xFF, n * sizeof(T), stream)); else memset(out, 0xFF, n * sizeof(T));
    }
};
// a scratch buffer grown to `need` bytes, ready to be carved
static Carver carve(char *&buf, size_t &cap, size_t need) {
    ensure(buf, cap, need);
    return Carver{buf, 0, cap};
}

// Measure, then decide: the family's Sizes struct starts on the device with no string over the limit, `launch` enqueues the sizes
// kernel (and what is scanned with it), and one read-back and wait bring the measurements to the host, before any output is written.
template <typename Sizes, typename Launch> static Sizes measure(Scope *scope, Sizes *device_sizes, Launch launch) {
    Sizes init{}, got{};
    init.first_oversize = ~0ull;
    SWH_HIP_CHECK(hipMemcpyAsync(device_sizes, &init, sizeof init, hipMemcpyHostToDevice, scope->stream));
    launch();
    SWH_HIP_CHECK(hipMemcpyAsync(&got, device_sizes, sizeof got, hipMemcpyDeviceToHost, scope->stream));
    SWH_HIP_CHECK(hipStreamSynchronize(scope->stream));
    return got;
}

// Count, scan, fill: the rows of a CSR call (within, extract_within, infix_all), whose lengths nobody knows before the pairs are
// walked. The site's count pass leaves a count per (row, slice); scan_counts() turns them into a cursor each and the row offsets
// (the offsets scan, scan.hpp) and reads their last word, the total (8 bytes: one read and wait); publish() sends the offsets on to a
// host caller and says whether the site's fill pass runs: only if there are hits and the caller's arrays hold them. Two steps, since a
// site looks at its call's summary or closes the scan's stamps between them.
struct CsrRows {
    Staged<uint64_t> offs;         // the caller's row offsets: rows + 1
    uint64_t rows, capacity, total = 0;
    uint32_t *counts = nullptr;    // [row][slice]
    uint64_t *cursors = nullptr;   // [row][slice]: where the hits of that count begin
    ScanScratch scan;

    CsrRows(size_t *row_offsets, uint64_t rows_, size_t capacity_) : offs((uint64_t *)row_offsets), rows(rows_), capacity(capacity_) {
        static_assert(sizeof(size_t) == sizeof(uint64_t), "row offsets are scanned as 64-bit words");
    }
    void fill_empty(hipStream_t stream) const { offs.fill_zero(stream, rows + 1); }   // no row, or every row empty
    size_t need(uint64_t slices = 1) const {   // of the scratch
        return pad(rows * slices * 4) + pad(rows * slices * 8) + ScanScratch::need(rows * slices) + offs.need(rows + 1);
    }
    void place(Carver &sc, uint64_t slices = 1) {
        counts = sc.take<uint32_t>(rows * slices); cursors = sc.take<uint64_t>(rows * slices);
        scan.place(sc, rows * slices);
        offs.place(sc, rows + 1);
    }
    void scan_counts(Scope *scope, uint32_t slices = 1) {
        launch_offsets_scan(scope, counts, rows, slices, scan, cursors, offs.dev);
        total = read_offset(offs.dev, 1, rows, true, scope->stream);
    }
    bool publish(hipStream_t stream) const {
        offs.copy_back(stream, rows + 1);
        return total && total <= capacity;
    }
};
// Where a fill pass writes `total` hits: the caller's device arrays, or staging for its host arrays in scope->within_out, sized now
// that the total is known, with `extra` bytes for the site to carve after them.
template <typename... T> static Carver carve_hits(Scope *scope, uint64_t total, size_t extra, Staged<T> &...outs) {
    Carver oc = carve(scope->within_out, scope->within_out_bytes, (outs.need(total) + ... + extra));
    (outs.place(oc, total), ...);
    return oc;
}
// The output rules the CSR calls share, in the order they are tested: the row offsets always, the per-hit arrays `a` and `b` (`names`:
// "a and b") both or neither, and no capacity without them (`three_arrays`: the call has a third per-hit array, so one more NULL).
static swh_status_t csr_output_checks(const void *row_offsets, const void *a, const void *b, const char *names, bool three_arrays, size_t capacity,
                                      const char **error) {
    if (!row_offsets) return fail(error, swh_invalid_argument_k, "null row_offsets");
    if (!a != !b) return fail(error, swh_invalid_argument_k, "%s must both be given, or neither", names);
    if (!a && capacity)
        return fail(error, swh_invalid_argument_k, "a capacity without arrays: the counting call passes %sNULL, NULL, 0", three_arrays ? "NULL, " : "");
    return swh_success_k;
}

// One side of a launch on prepared tapes as the lane-per-block and alignment kernels read it: strings [first, first + count) as code
// points (`cp`: u64 offsets) or as bytes at the tape's own offset width, which goes to `off64`.
static TapeRef tape_side(const Prepared *p, bool cp, size_t first, size_t count, uint32_t &off64) {
    off64 = cp ? 1u : p->off64;
    return prepared_view(p, cp, first, count);
}
// the symbols of string i of a device tape, for an error text (two reads and waits: refusals only)
static uint64_t string_symbols(const TapeRef &tape, uint32_t off64, size_t i, hipStream_t stream) {
    return read_offset(tape.offsets, (int)off64, i + 1, true, stream) - read_offset(tape.offsets, (int)off64, i, true, stream);
}

// The common end of a call whose kernels have completed on the scope's stream: with profiling on they are the call's timing, once in
// the totals. (SearchSweep::close, ExtractSweep::close and within's fused path end in their own ways.)
static void close_call(Scope *scope, uint64_t cells, uint64_t bytes) {
    if (scope->profiling && scope->stamps_used) { collect_timing(scope); add_to_totals(scope->totals, scope->last_timing); }
    scope->stamps_used = 0;
    scope->last_timing.cells = cells; scope->last_timing.bytes = bytes;
}

// ---- the search planner: what top-k and the range search decide alike ---------------------------------------------------------------
// Both searches run word-sized byte strings on unit costs through a fused kernel of their own (k_cross_topk, k_cross_within): the
// searches a dense cross-product of the same views would run on k_cross_short (pick_route for prepared tapes). Everything else takes
// the general path: the candidates in slices, each slice scored by the ordinary cross-product routes into a u32 matrix in scratch
// (with the caller's bound, so long strings may take the banded kernel) and handed to the search's own kernels. What differs between
// the two comes in as a value or a callback.
// `force_select`: the search's STRINGWARS_AMD_*_ROUTE=select hook; `dev_out`: its results go to device memory
static bool search_is_fused(const Scope *scope, const Engine *engine, const TapePair &p, uint32_t bound, bool force_select, bool dev_out) {
    const bool utf8 = p.pa->utf8 && !(p.pa->ascii && p.pb->ascii && p.pa->off64 == p.pb->off64);
    CallSpec whole{};   // the dense cross-product of the two views, as run_call_on would route it
    whole.a.count = p.a_count; whole.b.count = p.b_count; whole.cross = true; whole.bound = bound; whole.pa = p.pa; whole.pb = p.pb;
    return !force_select && !utf8 && engine->algorithm == swh_algorithm_auto_k && p.pa->off64 == p.pb->off64 &&
           pick_route(scope, engine, whole, false, dev_out, call_lengths(scope, engine, whole, false)).route == kRouteCrossShort;
}

// The fused kernels' candidate slices per block of 16 queries: enough for ~32 items per compute unit (a few rounds of its 12 wave
// slots: 65 536 x 1 M words ran top-k at 4.6 TCUPS with 16, 5.9 with 32), while what the search keeps per (row, slice) --
// `row_slice_bytes` -- stays under 256 MB; at most one per chunk of 64 candidates. `forced`: a test hook's count, 0 without one.
struct SearchSlices { uint64_t slices, slice_chunks; };
static SearchSlices search_slices(uint64_t nq, uint64_t nc, uint64_t compute_units, uint64_t row_slice_bytes, uint64_t forced) {
    const uint64_t qblocks = (nq + 15) / 16, chunks = (nc + 63) / 64;
    const uint64_t target = compute_units * 32;
    uint64_t slices = std::min<uint64_t>(std::max<uint64_t>((target + qblocks - 1) / qblocks, 1), chunks);
    slices = std::max<uint64_t>(1, std::min<uint64_t>(slices, ((uint64_t)256 << 20) / (nq * row_slice_bytes)));
    if (forced) slices = std::min<uint64_t>(forced, chunks);
    const uint64_t slice_chunks = (chunks + slices - 1) / slices;
    return SearchSlices{(chunks + slice_chunks - 1) / slice_chunks, slice_chunks};
}

// The general path: query blocks of at most 2^18 rows x candidate slices of at most 2^26 pairs (a 256 MB u32 matrix), and the search
// reported as one call whose name says which path ran and which kernel scored the pairs.
struct SearchSweep {
    Scope *scope; const Engine *engine; const TapePair &pair; uint32_t bound;
    uint64_t q_step, c_step;
    swh_timing_totals_t totals_before;
    swh_timing_t sum{};
    char scoring_name[64] = "";

    SearchSweep(Scope *s, const Engine *e, const TapePair &p, uint32_t bound_)
        : scope(s), engine(e), pair(p), bound(bound_), q_step(std::min<uint64_t>(p.a_count, (uint64_t)1 << 18)),
          c_step(std::max<uint64_t>(1, std::min<uint64_t>(p.b_count, ((uint64_t)1 << 26) / q_step))), totals_before(s->totals) {}

    // One walk over the blocks. rows_begin(q0, rows) opens every block of queries, before its first slice is scored; each slice is then
    // scored into `matrix` (q_step * c_step entries) and handed to block(q0, rows, c0, columns, last_slice) with the stamps reset.
    // `counted`: the walk's cells and bytes go into the sum (a second walk of the same pairs: not again).
    template <typename Rows, typename Block>
    swh_status_t walk(uint32_t *matrix, bool counted, const char **error, Rows rows_begin, Block block) {
        const uint64_t nq = pair.a_count, nc = pair.b_count;
        for (uint64_t q0 = 0; q0 < nq; q0 += q_step) {
            const uint64_t rows = std::min<uint64_t>(q_step, nq - q0);
            rows_begin(q0, rows);
            for (uint64_t c0 = 0; c0 < nc; c0 += c_step) {
                const uint64_t columns = std::min<uint64_t>(c_step, nc - c0);
                CallSpec spec{};
                spec.a = HostTape{nullptr, nullptr, (size_t)rows, 0};
                spec.b = HostTape{nullptr, nullptr, (size_t)columns, 0};
                spec.cross = true; spec.utf8 = pair.pa->utf8; spec.bound = bound;
                spec.out = matrix; spec.out_stride = 4; spec.row_stride = columns * 4; spec.out64 = false;
                spec.pa = pair.pa; spec.pb = pair.pb; spec.a_first = pair.a_first + q0; spec.b_first = pair.b_first + c0;
                const swh_status_t status = run_call_on(scope, engine, spec, error);
                if (status != swh_success_k) return status;
                const swh_timing_t &dp = scope->last_timing;
                if (counted) { sum.cells += dp.cells; sum.bytes += dp.bytes; }
                sum.total_ms += dp.total_ms; sum.compute_ms += dp.compute_ms; sum.kernels += dp.kernels;
                if (dp.dominant_ms > sum.dominant_ms) { sum.dominant_ms = dp.dominant_ms; snprintf(scoring_name, sizeof scoring_name, "%s", dp.dominant_name); }
                scope->stamps_used = 0;
                scope->stamps_pending = false;
                block(q0, rows, c0, columns, c0 + columns == nc);
            }
        }
        return swh_success_k;
    }
    // with profiling on, the time of the `launched` kernels of the search's own since the last scoring call
    void time_own_kernels(uint32_t launched) {
        if (!scope->profiling) return;
        SWH_HIP_CHECK(hipStreamSynchronize(scope->stream));
        collect_timing(scope);
        sum.total_ms += scope->last_timing.total_ms; sum.compute_ms += scope->last_timing.compute_ms; sum.kernels += launched;
        scope->stamps_used = 0;
    }
    // the search as one call, "<search>_select/<scoring kernel>", once in the scope's totals
    void close(const char *search) {
        scope->summary_pending = false;
        scope->stamps_pending = false;
        snprintf(sum.dominant_name, sizeof sum.dominant_name, "%s_select/%s", search, scoring_name);
        scope->last_timing = sum;
        if (scope->profiling) {
            scope->totals = totals_before;
            add_to_totals(scope->totals, sum);
        }
    }
};

extern "C" {
// ---- top-k search (topk.hip) ----------------------------------------------------------------------------------------------------------
// The fused kernel keeps a list of k per (row, slice) and merges them; the general path folds each scored slice into the running
// lists with k_topk_select.
// STRINGWARS_AMD_TOPK_PRUNE=0 (test library): the fused kernel walks every chunk, also those the length bound rules out (the comparison knob)
static uint32_t topk_prune() {
    static const uint32_t on = [] { const char *e = test_hook("STRINGWARS_AMD_TOPK_PRUNE"); return !e || atoi(e) != 0 ? 1u : 0u; }();
    return on;
}
// STRINGWARS_AMD_TOPK_ROUTE=select (test library): every search on the general path
static bool topk_force_select() {
    static const bool on = [] { const char *e = test_hook("STRINGWARS_AMD_TOPK_ROUTE"); return e && !strcmp(e, "select"); }();
    return on;
}

static swh_status_t topk_run(Scope *scope, const Engine *engine, const TapePair &p, uint32_t k32, uint32_t bound, uint32_t *indices,
                             uint32_t *distances, const char **error) {
    return synchronous_run(scope, error, [&]() -> swh_status_t {
        const uint64_t nq = p.a_count, nc = p.b_count, k = k32;
        if (nq == 0) return swh_success_k;
        const uint64_t cap = bound == SWH_UNBOUNDED ? ~0ull : ((uint64_t)bound + 1) << 32;
        const size_t out_bytes = nq * k * sizeof(uint32_t);
        SWH_HIP_CHECK(hipSetDevice(scope->device));
        hipStream_t stream = scope->stream;
        Staged<uint32_t> ind(indices), dist(distances);
        if (nc == 0) {   // every row is padding
            ind.fill_padding(stream, nq * k); dist.fill_padding(stream, nq * k);
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            return swh_success_k;
        }
        const size_t ow = p.pa->off64 ? 8 : 4;
        auto finish_outputs = [&] {
            ind.copy_back(stream, nq * k); dist.copy_back(stream, nq * k);
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
        };

        if (search_is_fused(scope, engine, p, bound, topk_force_select(), ind.on_device)) {
            // ---- fused: a partial list of k (index, distance) words per (row, slice) ------------------------------------------------------
            const SearchSlices cut = search_slices(nq, nc, scope->compute_units, k * 8, 0);
            const uint64_t slices = cut.slices;
            const size_t need = (slices > 1 ? pad(nq * slices * k * 8) : 0) + ind.need(nq * k) + dist.need(nq * k);
            Carver sc = carve(scope->topk_scratch, scope->topk_scratch_bytes, need);
            TopkLaunch t{};
            t.a = prepared_view(p.pa, false, p.a_first, nq); t.b = prepared_view(p.pb, false, p.b_first, nc);
            t.off64 = p.pa->off64; t.k = (uint32_t)k; t.slices = (uint32_t)slices; t.prune = topk_prune();
            t.slice_chunks = cut.slice_chunks; t.cap = cap;
            t.partial = slices > 1 ? sc.take<uint64_t>(nq * slices * k) : nullptr;
            t.indices = ind.place(sc, nq * k);
            t.distances = dist.place(sc, nq * k);
            scope->summary_slot = 0;
            launch_cross_topk(scope, t);
            finish_outputs();
            const CallSummary sm = scope->summary_host[0];
            if (!sm.violation) {
                close_call(scope, sm.cells, p.pa->total_bytes + p.pb->total_bytes + (nq + nc) * ow + 2 * out_bytes);
                return swh_success_k;
            }
            // a string longer than the kernel takes (the memory of a prepared tape changed since it was measured): the general path
            scope->stamps_used = 0;
            scope->last_timing = swh_timing_t{};
        }

        // ---- general path: each slice folded into the block's running lists ---------------------------------------------------------------
        SearchSweep sweep(scope, engine, p, bound);
        const size_t need = pad(sweep.q_step * sweep.c_step * 4) + pad(sweep.q_step * k * 8) + ind.need(nq * k) + dist.need(nq * k);
        Carver sc = carve(scope->topk_scratch, scope->topk_scratch_bytes, need);
        uint32_t *matrix = sc.take<uint32_t>(sweep.q_step * sweep.c_step);
        uint64_t *lists = sc.take<uint64_t>(sweep.q_step * k);
        ind.place(sc, nq * k); dist.place(sc, nq * k);
        auto pad_lists = [&](uint64_t, uint64_t rows) { SWH_HIP_CHECK(hipMemsetAsync(lists, 0xFF, rows * k * 8, stream)); };   // every row is padding
        const swh_status_t status = sweep.walk(matrix, true, error, pad_lists, [&](uint64_t q0, uint64_t rows, uint64_t c0, uint64_t columns, bool last_slice) {
            launch_topk_select(scope, matrix, rows, columns, q0, c0, (uint32_t)k, cap, lists, last_slice, ind.dev, dist.dev);
            sweep.time_own_kernels(1);
        });
        if (status != swh_success_k) return status;
        finish_outputs();
        sweep.close("topk");
        return swh_success_k;
    });
}

static swh_status_t topk_checks(swh_levenshtein_t e, swh_scope_t s, size_t k, size_t queries, size_t candidates, const uint32_t *indices,
                                const uint32_t *distances, const char **error) {
    if (!s || !e) return fail(error, swh_invalid_argument_k, "null scope or engine");
    if (((Engine *)e)->kind != 0) return fail(error, swh_invalid_argument_k, "not a Levenshtein engine");
    if (k < 1 || k > SWH_TOPK_MAX) return fail(error, swh_invalid_argument_k, "k must lie in [1, SWH_TOPK_MAX]");
    if (candidates >= 0xFFFFFFFFull) return fail(error, swh_unsupported_length_k, "2^32 - 1 candidates or more");
    if (queries && (!indices || !distances)) return fail(error, swh_invalid_argument_k, "null output pointer");
    return swh_success_k;
}

static swh_status_t topk_tapes(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *q, const swh_tape_u64_t *c, bool utf8, size_t k,
                               uint32_t bound, uint32_t *indices, uint32_t *distances, const char **error) {
    if (!q) return fail(error, swh_invalid_argument_k, "null tape");
    swh_status_t status = topk_checks(e, s, k, q->count, (c ? c : q)->count, indices, distances, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.begin(s, error)) != swh_success_k) return status;
    if (q->count == 0) return swh_success_k;
    if ((status = call.prepare(q, c, utf8, true, true, error)) != swh_success_k) return status;
    return topk_run(call.scope, (Engine *)e, call.pair, (uint32_t)k, bound, indices, distances, error);
}
swh_status_t swh_levenshtein_topk_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *queries, const swh_tape_u64_t *candidates,
                                          size_t k, uint32_t bound, uint32_t *indices, uint32_t *distances, const char **error) {
    return topk_tapes(e, s, queries, candidates, false, k, bound, indices, distances, error);
}
swh_status_t swh_levenshtein_utf8_topk_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *queries,
                                               const swh_tape_u64_t *candidates, size_t k, uint32_t bound, uint32_t *indices,
                                               uint32_t *distances, const char **error) {
    return topk_tapes(e, s, queries, candidates, true, k, bound, indices, distances, error);
}
swh_status_t swh_levenshtein_topk_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *queries,
                                           const swh_prepared_view_t *candidates, size_t k, uint32_t bound, uint32_t *indices,
                                           uint32_t *distances, const char **error) {
    TwoTapeCall call;
    swh_status_t status = call.views(queries, candidates, true, error);
    if (status != swh_success_k) return status;
    if ((status = topk_checks(e, s, k, call.pair.a_count, call.pair.b_count, indices, distances, error)) != swh_success_k) return status;
    if ((status = call.begin_on_views(s, error)) != swh_success_k) return status;
    return topk_run(call.scope, (Engine *)e, call.pair, (uint32_t)k, bound, indices, distances, error);
}

// ---- range search (within.hip) ---------------------------------------------------------------------------------------------------------
// Every candidate within `bound` of every query, as CSR, on the search planner's routes. Both count first, scan the counts into the row
// offsets on the device, read the total (8 bytes) and fill only if the caller's arrays hold it.
// STRINGWARS_AMD_WITHIN_PRUNE=0 (test library): the fused kernel walks every chunk, also those the length gap rules out
static uint32_t within_prune() {
    static const uint32_t on = [] { const char *e = test_hook("STRINGWARS_AMD_WITHIN_PRUNE"); return !e || atoi(e) != 0 ? 1u : 0u; }();
    return on;
}
// STRINGWARS_AMD_WITHIN_ROUTE=select (test library): every search on the general path
static bool within_force_select() {
    static const bool on = [] { const char *e = test_hook("STRINGWARS_AMD_WITHIN_ROUTE"); return e && !strcmp(e, "select"); }();
    return on;
}
// STRINGWARS_AMD_WITHIN_SLICES=n (test library): the fused kernel's candidate slices per query block (at most one per chunk)
static uint64_t within_slices_hook() {
    static const uint64_t n = [] { const char *e = test_hook("STRINGWARS_AMD_WITHIN_SLICES"); return e && atoll(e) > 0 ? (uint64_t)atoll(e) : 0; }();
    return n;
}

struct WithinOutputs {
    size_t *row_offsets;
    uint32_t *indices, *distances;
    size_t capacity;
};

static swh_status_t within_run(Scope *scope, const Engine *engine, const TapePair &p, uint32_t bound, const WithinOutputs &r, const char **error) {
    return synchronous_run(scope, error, [&]() -> swh_status_t {
        const uint64_t nq = p.a_count, nc = p.b_count;
        SWH_HIP_CHECK(hipSetDevice(scope->device));
        hipStream_t stream = scope->stream;
        CsrRows csr(r.row_offsets, nq, r.capacity);
        Staged<uint32_t> ind(r.indices), dist(r.distances);   // (both null in a counting call: nothing is staged, nothing filled)
        if (nq == 0 || nc == 0) {
            csr.fill_empty(stream);
            return swh_success_k;
        }
        const size_t ow = p.pa->off64 ? 8 : 4;

        if (search_is_fused(scope, engine, p, bound, within_force_select(), ind.on_device)) {
            // ---- fused: a count (4 bytes) and a start (8) per (row, slice) ----------------------------------------------------------------
            const SearchSlices cut = search_slices(nq, nc, scope->compute_units, 12, within_slices_hook());
            const uint64_t slices = cut.slices;
            Carver sc = carve(scope->topk_scratch, scope->topk_scratch_bytes, csr.need(slices));
            csr.place(sc, slices);
            WithinLaunch w{};
            w.a = prepared_view(p.pa, false, p.a_first, nq); w.b = prepared_view(p.pb, false, p.b_first, nc);
            w.off64 = p.pa->off64; w.slices = (uint32_t)slices; w.bound = bound; w.prune = within_prune(); w.slice_chunks = cut.slice_chunks;
            w.counts = csr.counts; w.starts = csr.cursors;
            scope->summary_slot = 0;
            launch_cross_within(scope, w, false);
            csr.scan_counts(scope, (uint32_t)slices);
            const CallSummary sm = scope->summary_host[0];
            if (!sm.violation) {
                if (csr.publish(stream)) {
                    carve_hits(scope, csr.total, 0, ind, dist);
                    w.total = csr.total; w.indices = ind.dev; w.distances = dist.dev;
                    launch_cross_within(scope, w, true);
                    ind.copy_back(stream, csr.total); dist.copy_back(stream, csr.total);
                }
                SWH_HIP_CHECK(hipStreamSynchronize(stream));
                if (scope->profiling && scope->stamps_used) {
                    collect_timing(scope);
                    // the search is named after its walk, also where a tiny call's scan takes longer: the longer of the two passes
                    swh_timing_t &t = scope->last_timing;
                    t.dominant_ms = 0;
                    for (size_t i = 0; i < scope->stamps_used; ++i) {
                        float ms = 0;
                        if (!strcmp(scope->stamps[i].name, "cross_within")) (void)hipEventElapsedTime(&ms, scope->stamps[i].start, scope->stamps[i].stop);
                        if (ms > t.dominant_ms) t.dominant_ms = ms;
                    }
                    snprintf(t.dominant_name, sizeof t.dominant_name, "cross_within");
                    add_to_totals(scope->totals, scope->last_timing);
                }
                scope->last_timing.cells = sm.cells;
                // the tapes, a count and a start per (row, slice), the row offsets and the hits
                scope->last_timing.bytes = p.pa->total_bytes + p.pb->total_bytes + (nq + nc) * ow + nq * slices * 12 + (nq + 1) * 8 +
                                           (csr.total <= r.capacity ? csr.total * 8 : 0);
                return swh_success_k;
            }
            // a string longer than the kernel takes (the memory of a prepared tape changed since it was measured): the general path
            scope->stamps_used = 0;
            scope->last_timing = swh_timing_t{};
        }

        // ---- general path: every block scored twice, once to count and once to fill -------------------------------------------------------
        SearchSweep sweep(scope, engine, p, bound);
        Carver sc = carve(scope->topk_scratch, scope->topk_scratch_bytes, pad(sweep.q_step * sweep.c_step * 4) + csr.need());
        uint32_t *matrix = sc.take<uint32_t>(sweep.q_step * sweep.c_step);
        csr.place(sc);
        SWH_HIP_CHECK(hipMemsetAsync(csr.counts, 0, nq * 4, stream));
        auto no_rows_begin = [](uint64_t, uint64_t) {};   // (counts and cursors span all queries: nothing to open per block)
        swh_status_t status = sweep.walk(matrix, true, error, no_rows_begin, [&](uint64_t q0, uint64_t rows, uint64_t, uint64_t columns, bool) {
            launch_within_count(scope, matrix, rows, columns, bound, csr.counts + q0);
            sweep.time_own_kernels(1);
        });
        if (status != swh_success_k) return status;
        csr.scan_counts(scope);
        sweep.time_own_kernels(2);
        if (csr.publish(stream)) {
            carve_hits(scope, csr.total, 0, ind, dist);
            status = sweep.walk(matrix, false, error, no_rows_begin, [&](uint64_t q0, uint64_t rows, uint64_t c0, uint64_t columns, bool) {
                launch_within_fill(scope, matrix, rows, columns, c0, bound, csr.cursors + q0, csr.total, ind.dev, dist.dev);
                sweep.time_own_kernels(1);
            });
            if (status != swh_success_k) return status;
            ind.copy_back(stream, csr.total); dist.copy_back(stream, csr.total);
        }
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        sweep.close("within");
        return swh_success_k;
    });
}

static swh_status_t within_checks(swh_levenshtein_t e, swh_scope_t s, size_t candidates, uint32_t bound, const size_t *row_offsets,
                                  const uint32_t *indices, const uint32_t *distances, size_t capacity, const char **error) {
    if (!s || !e) return fail(error, swh_invalid_argument_k, "null scope or engine");
    if (((Engine *)e)->kind != 0) return fail(error, swh_invalid_argument_k, "not a Levenshtein engine");
    if (bound == SWH_UNBOUNDED) return fail(error, swh_invalid_argument_k, "a range search needs a bound: without one it is the dense cross-product");
    if (candidates >= 0xFFFFFFFFull) return fail(error, swh_unsupported_length_k, "2^32 - 1 candidates or more");
    return csr_output_checks(row_offsets, indices, distances, "indices and distances", false, capacity, error);
}

static swh_status_t within_tapes(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *q, const swh_tape_u64_t *c, bool utf8, uint32_t bound,
                                 const WithinOutputs &outs, const char **error) {
    if (!q) return fail(error, swh_invalid_argument_k, "null tape");
    const size_t candidates = (c ? c : q)->count;
    swh_status_t status = within_checks(e, s, candidates, bound, outs.row_offsets, outs.indices, outs.distances, outs.capacity, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.begin(s, error)) != swh_success_k) return status;
    // (a search without queries prepares nothing, one without candidates the queries alone: the offsets are still written)
    if ((status = call.prepare(q, c, utf8, q->count != 0, q->count && candidates, error)) != swh_success_k) return status;
    return within_run(call.scope, (Engine *)e, call.pair, bound, outs, error);
}
swh_status_t swh_levenshtein_within_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *queries, const swh_tape_u64_t *candidates,
                                            uint32_t bound, size_t *row_offsets, uint32_t *indices, uint32_t *distances, size_t capacity,
                                            const char **error) {
    return within_tapes(e, s, queries, candidates, false, bound, WithinOutputs{row_offsets, indices, distances, capacity}, error);
}
swh_status_t swh_levenshtein_utf8_within_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *queries,
                                                 const swh_tape_u64_t *candidates, uint32_t bound, size_t *row_offsets, uint32_t *indices,
                                                 uint32_t *distances, size_t capacity, const char **error) {
    return within_tapes(e, s, queries, candidates, true, bound, WithinOutputs{row_offsets, indices, distances, capacity}, error);
}
swh_status_t swh_levenshtein_within_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *queries,
                                             const swh_prepared_view_t *candidates, uint32_t bound, size_t *row_offsets, uint32_t *indices,
                                             uint32_t *distances, size_t capacity, const char **error) {
    TwoTapeCall call;
    swh_status_t status = call.views(queries, candidates, true, error);
    if (status != swh_success_k) return status;
    if ((status = within_checks(e, s, call.pair.b_count, bound, row_offsets, indices, distances, capacity, error)) != swh_success_k) return status;
    if ((status = call.begin_on_views(s, error)) != swh_success_k) return status;
    return within_run(call.scope, (Engine *)e, call.pair, bound, WithinOutputs{row_offsets, indices, distances, capacity}, error);
}

// ---- alignments (align.hip) ----------------------------------------------------------------------------------------------------------
// k_align_sizes measures the batch (stored bytes, symbols, cells, the first pair over SWH_ALIGN_MAX_CELLS) and the stored bytes and slot
// sizes are scanned on the device; one read-back of the measurements decides the errors and the chunks, before any output is written.
// Then per chunk of consecutive pairs the forward pass + walk (k_align), the counts scanned into the offsets, and k_align_emit places
// the ops -- no host round trip between the forward pass and the outputs.
// A chunk holds enough pairs to fill the device -- kAlignFillWaves waves per compute unit, a lane per pair -- and, beyond that, as many
// as keep its stored delta vectors near 128 MiB, where the walk still reads the forward pass's stores from the Infinity Cache. Long
// pairs therefore give up the residency rather than the parallelism (1 K protein pairs of 4 K symbols store 6 GB: one chunk).
// STRINGWARS_AMD_ALIGN_CHUNK_KB=n (test library) sets the byte target and drops the fill minimum, to put many chunks in a small test.
constexpr uint64_t kAlignFillWaves = 8;
static const char *align_chunk_hook() {
    static const char *e = test_hook("STRINGWARS_AMD_ALIGN_CHUNK_KB");
    return e;
}
static uint64_t align_chunk_pairs(const Scope *scope, uint64_t count, uint64_t store_total) {
    const char *hook = align_chunk_hook();
    const uint64_t target = hook ? (uint64_t)atol(hook) << 10 : (uint64_t)128 << 20;
    const uint64_t fill = hook ? 1 : (uint64_t)scope->compute_units * kAlignFillWaves * 64;
    const uint64_t mean = std::max<uint64_t>(1, store_total / std::max<uint64_t>(count, 1));
    uint64_t pairs = std::max<uint64_t>(fill, target / mean);
    // no chunk asks for more than half the device memory that is free
    size_t free_bytes = 0, total_bytes = 0;
    if (hipMemGetInfo(&free_bytes, &total_bytes) == hipSuccess && free_bytes)
        pairs = std::min<uint64_t>(pairs, std::max<uint64_t>(1, (uint64_t)(free_bytes / 2) / mean));
    return std::max<uint64_t>(1, std::min<uint64_t>(pairs, count));
}

struct AlignOutputs {
    uint32_t *distances;
    uint64_t *offsets;
    uint8_t *ops;
    size_t capacity;
};

static swh_status_t align_run(Scope *scope, const TapePair &p, uint32_t bound, const AlignOutputs &r, const char **error) {
    return synchronous_run(scope, error, [&]() -> swh_status_t {
        const uint64_t count = p.a_count;
        SWH_HIP_CHECK(hipSetDevice(scope->device));
        hipStream_t stream = scope->stream;
        Staged<uint32_t> distances(r.distances); Staged<uint64_t> offsets(r.offsets); Staged<uint8_t> ops(r.ops);
        if (count == 0) {
            const uint64_t zero = 0;
            if (offsets.on_device) SWH_HIP_CHECK(hipMemcpyAsync(r.offsets, &zero, sizeof zero, hipMemcpyHostToDevice, stream)); else r.offsets[0] = 0;
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            return swh_success_k;
        }
        const bool cp = p.pa->utf8;
        AlignTapes t{};
        t.a = tape_side(p.pa, cp, p.a_first, count, t.a_off64);
        t.b = tape_side(p.pb, cp, p.b_first, count, t.b_off64);
        t.cp = cp ? 1 : 0;
        t.count = count;

        AlignScratch *sc_entry = call_scratch(scope);
        // fixed part: sizes | store_base | slot_base | counts | offsets | distances | the scans' scratch
        const size_t fixed = pad(sizeof(AlignSizes)) + 2 * pad((count + 1) * 8) + pad(count * 4) + offsets.need(count + 1) + distances.need(count) +
                             ScanScratch::need(count);
        ensure(sc_entry->buf, sc_entry->bytes, fixed);
        Carver sc{};
        AlignSizes *sizes;
        uint64_t *store_base, *slot_base;
        uint32_t *counts;
        ScanScratch scan;
        auto carve_fixed = [&] {   // (again after the scratch has been regrown)
            sc = Carver{sc_entry->buf, 0, sc_entry->bytes};
            sizes = sc.take<AlignSizes>(1);
            store_base = sc.take<uint64_t>(count + 1); slot_base = sc.take<uint64_t>(count + 1);
            counts = sc.take<uint32_t>(count);
            offsets.place(sc, count + 1); distances.place(sc, count);
            scan.place(sc, count);
        };
        carve_fixed();

        const AlignSizes got = measure(scope, sizes, [&] {
            launch_align_sizes(scope, t, store_base, slot_base, sizes);
            // in place: count + 1 words each, the total in the last
            launch_offsets_scan(scope, store_base, count, 1, scan, nullptr, store_base);
            launch_offsets_scan(scope, slot_base, count, 1, scan, nullptr, slot_base);
        });
        if (got.first_oversize != ~0ull) {
            const size_t i = (size_t)got.first_oversize;
            const uint64_t la = string_symbols(t.a, t.a_off64, i, stream), lb = string_symbols(t.b, t.b_off64, i, stream);
            scope->stamps_used = 0;
            return fail(error, swh_unsupported_length_k, "pair %zu: %llu x %llu symbols exceeds SWH_ALIGN_MAX_CELLS (2^30 cells per pair)", i,
                        (unsigned long long)la, (unsigned long long)lb);
        }
        if (r.capacity < got.symbols) {
            scope->stamps_used = 0;
            return fail(error, swh_invalid_argument_k, "ops_capacity %zu is below the %llu symbols of the two tapes", r.capacity,
                        (unsigned long long)got.symbols);
        }

        // chunks of consecutive pairs; where they start in the storage space is read back (one strided copy) to size the largest
        const uint64_t per_chunk = align_chunk_pairs(scope, count, got.store_total);
        const uint64_t chunks = (count + per_chunk - 1) / per_chunk;
        std::vector<uint64_t> starts(chunks + 1, 0);
        if (chunks > 1) {
            SWH_HIP_CHECK(hipMemcpy2DAsync(starts.data(), 8, store_base, per_chunk * 8, 8, chunks, hipMemcpyDeviceToHost, stream));
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
        }
        starts[chunks] = got.store_total;
        uint64_t widest = 0;
        for (uint64_t q = 0; q < chunks; ++q) widest = std::max<uint64_t>(widest, starts[q + 1] - starts[q]);
        // variable part: the op slots (whole batch) | staged ops for host outputs | the widest chunk of stored delta vectors
        const size_t store_bytes = (size_t)widest;
        const size_t need = fixed + pad(got.symbols + 16) + ops.need(got.symbols + 16) + pad(store_bytes + 16);
        if (need > sc_entry->bytes) {
            // keep what the fixed part already holds: the measurements and scans live there
            char *grown = nullptr;
            const size_t want = need + need / 4 + (1 << 20);
            SWH_HIP_CHECK(hipMalloc((void **)&grown, want));
            SWH_HIP_CHECK(hipMemcpyAsync(grown, sc_entry->buf, fixed, hipMemcpyDeviceToDevice, stream));
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            SWH_HIP_CHECK(hipFree(sc_entry->buf));
            sc_entry->buf = grown;
            sc_entry->bytes = want;
            carve_fixed();
        }
        uint8_t *slots = sc.take<uint8_t>(got.symbols + 16);
        ops.place(sc, got.symbols + 16);
        char *store = sc.take<char>(store_bytes + 16);

        AlignChunk c{};
        c.store_base = store_base; c.slot_base = slot_base; c.store = store; c.slots = slots;
        c.counts = counts; c.distances = distances.dev; c.bound = bound;
        for (uint64_t q = 0; q < chunks; ++q) {
            c.pair_first = q * per_chunk;
            c.pair_end = std::min<uint64_t>(count, (q + 1) * per_chunk);
            c.store_first = starts[q];
            launch_align_chunk(scope, t, c);
        }
        launch_offsets_scan(scope, counts, count, 1, scan, nullptr, offsets.dev);
        launch_align_emit(scope, count, slot_base, counts, offsets.dev, slots, ops.dev);
        distances.copy_back(stream, count); offsets.copy_back(stream, count + 1);
        if (!ops.on_device) {   // only the ops there are, not the capacity: their number is read first
            const uint64_t total_ops = read_offset(offsets.dev, 1, count, true, stream);
            if (total_ops) ops.copy_back(stream, total_ops);
        }
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        close_call(scope, got.cells, (cp ? 4 : 1) * got.symbols + 2 * (count + 1) * 8 + count * 4 + got.symbols);
        return swh_success_k;
    });
}

static swh_status_t align_checks(swh_levenshtein_t e, swh_scope_t s, size_t a_count, size_t b_count, const uint32_t *distances,
                                 const uint64_t *offsets, const uint8_t *ops, const char **error) {
    if (!s || !e) return fail(error, swh_invalid_argument_k, "null scope or engine");
    const Engine *engine = (const Engine *)e;
    if (engine->kind != 0) return fail(error, swh_invalid_argument_k, "not a Levenshtein engine");
    if (!engine->unit_costs) return fail(error, swh_not_implemented_k, "alignments need unit costs (match 0, mismatch 1, open 1, extend 1)");
    if (a_count != b_count) return fail(error, swh_invalid_argument_k, "a and b must hold the same number of strings");
    if (!offsets || (a_count && (!distances || !ops))) return fail(error, swh_invalid_argument_k, "null output pointer");
    return swh_success_k;
}

static swh_status_t align_tapes(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b, bool utf8, uint32_t bound,
                                const AlignOutputs &outs, const char **error) {
    if (!a || !b) return fail(error, swh_invalid_argument_k, "null tape");
    swh_status_t status = align_checks(e, s, a->count, b->count, outs.distances, outs.offsets, outs.ops, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.begin(s, error)) != swh_success_k) return status;
    const bool pairs = a->count != 0;
    if ((status = call.prepare(a, b, utf8, pairs, pairs, error)) != swh_success_k) return status;
    return align_run(call.scope, call.pair, bound, outs, error);
}
swh_status_t swh_levenshtein_align_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b, uint32_t bound,
                                           uint32_t *distances, size_t *ops_offsets, char *ops, size_t ops_capacity, const char **error) {
    return align_tapes(e, s, a, b, false, bound, AlignOutputs{distances, (uint64_t *)ops_offsets, (uint8_t *)ops, ops_capacity}, error);
}
swh_status_t swh_levenshtein_utf8_align_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                uint32_t bound, uint32_t *distances, size_t *ops_offsets, char *ops, size_t ops_capacity,
                                                const char **error) {
    return align_tapes(e, s, a, b, true, bound, AlignOutputs{distances, (uint64_t *)ops_offsets, (uint8_t *)ops, ops_capacity}, error);
}
swh_status_t swh_levenshtein_align_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                            uint32_t bound, uint32_t *distances, size_t *ops_offsets, char *ops, size_t ops_capacity,
                                            const char **error) {
    const AlignOutputs outs{distances, (uint64_t *)ops_offsets, (uint8_t *)ops, ops_capacity};
    TwoTapeCall call;
    swh_status_t status = call.views(a, b, false, error);
    if (status != swh_success_k) return status;
    if ((status = align_checks(e, s, call.pair.a_count, call.pair.b_count, outs.distances, outs.offsets, outs.ops, error)) != swh_success_k) return status;
    if ((status = call.begin_on_views(s, error)) != swh_success_k) return status;
    return align_run(call.scope, call.pair, bound, outs, error);
}

// ---- infix search (infix.hip) ---------------------------------------------------------------------------------------------------------
// k_infix_sizes measures the batch (cells, the first pattern over SWH_INFIX_MAX_PATTERN) and cuts it into work items; one read-back of
// the measurements decides the errors before any output is written. Then the forward pass (distance and end of every pair) and the
// start pass (the starts, the bound) over the same items, and the copy-out of outputs that live on the host. The scratch -- the item
// list and, for host outputs, the three result arrays -- is the scope's alignment scratch: both calls are synchronous.
struct InfixOutputs { uint32_t *distances, *starts, *ends; };

static swh_status_t infix_run(Scope *scope, const TapePair &p, uint32_t bound, const InfixOutputs &r, const char **error) {
    return synchronous_run(scope, error, [&]() -> swh_status_t {
        const uint64_t count = p.a_count;
        if (count == 0) return swh_success_k;
        SWH_HIP_CHECK(hipSetDevice(scope->device));
        hipStream_t stream = scope->stream;
        Staged<uint32_t> distances(r.distances), starts(r.starts), ends(r.ends);
        const bool cp = p.pa->utf8;
        InfixTapes t{};
        t.patterns = tape_side(p.pa, cp, p.a_first, count, t.p_off64);
        t.texts = tape_side(p.pb, cp, p.b_first, count, t.t_off64);
        t.cp = cp ? 1 : 0;
        t.count = count;

        AlignScratch *sc_entry = call_scratch(scope);
        // sizes | items | distances | starts | ends (the last three only where the caller's array lives on the host)
        const size_t need = pad(sizeof(InfixSizes)) + pad(count * sizeof(LaneItem)) + distances.need(count) + starts.need(count) + ends.need(count);
        Carver sc = carve(sc_entry->buf, sc_entry->bytes, need);
        InfixSizes *sizes = sc.take<InfixSizes>(1);
        LaneItem *items = sc.take<LaneItem>(count);
        distances.place(sc, count); starts.place(sc, count); ends.place(sc, count);

        const InfixSizes got = measure(scope, sizes, [&] { launch_infix_sizes(scope, t, sizes, items); });
        if (got.first_oversize != ~0ull) {
            const size_t i = (size_t)got.first_oversize;
            const uint64_t m = string_symbols(t.patterns, t.p_off64, i, stream);
            scope->stamps_used = 0;
            return fail(error, swh_unsupported_length_k, "pair %zu: a pattern of %llu symbols exceeds SWH_INFIX_MAX_PATTERN (2048)", i,
                        (unsigned long long)m);
        }

        InfixRun run{};
        run.items = items; run.item_count = got.items;
        run.distances = distances.dev; run.starts = starts.dev; run.ends = ends.dev;
        run.bound = bound;
        run.wide_text = !cp && got.text_symbols >= 16;
        launch_infix_forward(scope, t, run);
        launch_infix_starts(scope, t, run);
        distances.copy_back(stream, count); starts.copy_back(stream, count); ends.copy_back(stream, count);
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        close_call(scope, got.cells, (cp ? 4 : 1) * got.symbols + 2 * (count + 1) * 8 + 3 * count * 4);
        return swh_success_k;
    });
}

// no scope or engine can exist without a device: a call that gets a null handle says so where there is none, as scope creation does
// (infix search and the scored families ask; top-k, within and align answer "null scope or engine" without the probe)
static swh_status_t probe_null_handles(swh_levenshtein_t e, swh_scope_t s, const char **error) {
    if (s && e) return swh_success_k;
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices == 0) {
        (void)hipGetLastError();
        return fail(error, swh_no_device_k, "no HIP device visible (this backend has no CPU path)");
    }
    return fail(error, swh_invalid_argument_k, "null scope or engine");
}
static swh_status_t infix_checks(swh_levenshtein_t e, swh_scope_t s, size_t p_count, size_t t_count, const uint32_t *distances,
                                 const uint32_t *starts, const uint32_t *ends, const char **error) {
    const Engine *engine = (const Engine *)e;
    if (engine->kind != 0) return fail(error, swh_invalid_argument_k, "not a Levenshtein engine");
    if (!engine->unit_costs) return fail(error, swh_not_implemented_k, "infix search needs unit costs (match 0, mismatch 1, open 1, extend 1)");
    if (p_count != t_count) return fail(error, swh_invalid_argument_k, "patterns and texts must hold the same number of strings");
    if (p_count && (!distances || !starts || !ends)) return fail(error, swh_invalid_argument_k, "null output pointer");
    return swh_success_k;
}

static swh_status_t infix_tapes(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *patterns, const swh_tape_u64_t *texts, bool utf8,
                                uint32_t bound, const InfixOutputs &outs, const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    if (!patterns || !texts) return fail(error, swh_invalid_argument_k, "null tape");
    status = infix_checks(e, s, patterns->count, texts->count, outs.distances, outs.starts, outs.ends, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.begin(s, error)) != swh_success_k) return status;
    const bool pairs = patterns->count != 0;
    if ((status = call.prepare(patterns, texts, utf8, pairs, pairs, error)) != swh_success_k) return status;
    return infix_run(call.scope, call.pair, bound, outs, error);
}
swh_status_t swh_levenshtein_infix_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *patterns, const swh_tape_u64_t *texts,
                                           uint32_t bound, uint32_t *distances, uint32_t *starts, uint32_t *ends, const char **error) {
    return infix_tapes(e, s, patterns, texts, false, bound, InfixOutputs{distances, starts, ends}, error);
}
swh_status_t swh_levenshtein_utf8_infix_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *patterns, const swh_tape_u64_t *texts,
                                                uint32_t bound, uint32_t *distances, uint32_t *starts, uint32_t *ends, const char **error) {
    return infix_tapes(e, s, patterns, texts, true, bound, InfixOutputs{distances, starts, ends}, error);
}
swh_status_t swh_levenshtein_infix_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *patterns,
                                            const swh_prepared_view_t *texts, uint32_t bound, uint32_t *distances, uint32_t *starts,
                                            uint32_t *ends, const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.views(patterns, texts, false, error)) != swh_success_k) return status;
    if ((status = infix_checks(e, s, call.pair.a_count, call.pair.b_count, distances, starts, ends, error)) != swh_success_k) return status;
    if ((status = call.begin_on_views(s, error)) != swh_success_k) return status;
    return infix_run(call.scope, call.pair, bound, InfixOutputs{distances, starts, ends}, error);
}

// ---- infix search for every occurrence within a bound (infix.hip's k_infix_hits / k_infix_hit_starts) -------------------------------------
// infix_run's measurement and items with within_run's protocol: the count walk leaves a count per pair, the scan turns the counts into
// cursors and the row offsets, the host reads the total (8 bytes), and only if the caller's arrays hold it the fill walk stores the
// hits; then, if starts are wanted, the hits are cut into items of their own and the start pass runs over them. The per-pair scratch
// (items, counts, best scores, cursors, the scan's block sums, staged offsets) is the scope's alignment scratch; the per-hit scratch
// (staged outputs, a row and at most an item per hit) is scope->within_out, sized once the total is known.
struct InfixAllOutputs {
    size_t *row_offsets;
    uint32_t *starts, *ends, *distances;
    size_t capacity;
};

static swh_status_t infix_all_run(Scope *scope, const TapePair &p, uint32_t bound, uint32_t select, const InfixAllOutputs &r, const char **error) {
    return synchronous_run(scope, error, [&]() -> swh_status_t {
        const uint64_t count = p.a_count;
        SWH_HIP_CHECK(hipSetDevice(scope->device));
        hipStream_t stream = scope->stream;
        CsrRows csr(r.row_offsets, count, r.capacity);
        Staged<uint32_t> starts(r.starts), ends(r.ends), distances(r.distances);   // (null in a counting call: nothing staged or filled)
        if (count == 0) {
            csr.fill_empty(stream);
            return swh_success_k;
        }
        const bool cp = p.pa->utf8;
        InfixTapes t{};
        t.patterns = tape_side(p.pa, cp, p.a_first, count, t.p_off64);
        t.texts = tape_side(p.pb, cp, p.b_first, count, t.t_off64);
        t.cp = cp ? 1 : 0;
        t.count = count;

        AlignScratch *sc_entry = call_scratch(scope);
        // sizes | items | a best score per pair | the rows' counts, cursors, scan scratch and offsets bound for the host
        Carver sc = carve(sc_entry->buf, sc_entry->bytes, pad(sizeof(InfixSizes)) + pad(count * sizeof(LaneItem)) + pad(count * 4) + csr.need());
        InfixSizes *sizes = sc.take<InfixSizes>(1);
        LaneItem *items = sc.take<LaneItem>(count);
        uint32_t *best = sc.take<uint32_t>(count);
        csr.place(sc);

        const InfixSizes got = measure(scope, sizes, [&] { launch_infix_sizes(scope, t, sizes, items); });
        if (got.first_oversize != ~0ull) {
            const size_t i = (size_t)got.first_oversize;
            const uint64_t m = string_symbols(t.patterns, t.p_off64, i, stream);
            scope->stamps_used = 0;
            return fail(error, swh_unsupported_length_k, "pair %zu: a pattern of %llu symbols exceeds SWH_INFIX_MAX_PATTERN (2048)", i,
                        (unsigned long long)m);
        }

        InfixHitsRun run{};
        run.items = items; run.item_count = got.items;
        run.bound = bound; run.select = select;
        run.counts = csr.counts; run.best = best; run.cursors = csr.cursors;
        run.wide_text = !cp && got.text_symbols >= 16;
        launch_infix_hits(scope, t, run, false);
        csr.scan_counts(scope);
        const bool filled = csr.publish(stream);
        if (filled) {
            // after the outputs, what the start pass needs: its measurement, and a row and at most an item per hit
            const size_t per_hit = r.starts ? pad(sizeof(InfixSizes)) + pad(csr.total * 8) + pad(csr.total * sizeof(LaneItem)) : 0;
            Carver oc = carve_hits(scope, csr.total, per_hit, ends, distances, starts);
            run.ends = ends.dev; run.distances = distances.dev; run.total = csr.total;
            launch_infix_hits(scope, t, run, true);
            if (r.starts) {
                InfixSizes *hit_sizes = oc.take<InfixSizes>(1);
                uint64_t *rows = oc.take<uint64_t>(csr.total);
                LaneItem *hit_items = oc.take<LaneItem>(csr.total);
                const InfixSizes cut = measure(scope, hit_sizes, [&] { launch_infix_hit_items(scope, t, csr.offs.dev, csr.total, hit_sizes, rows, hit_items); });
                InfixHitStartsRun pass{};
                pass.items = hit_items; pass.item_count = cut.items;
                pass.rows = rows; pass.ends = run.ends; pass.distances = run.distances; pass.starts = starts.dev;
                launch_infix_hit_starts(scope, t, pass);
                starts.copy_back(stream, csr.total);
            }
            ends.copy_back(stream, csr.total); distances.copy_back(stream, csr.total);
        }
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        // the tapes (twice if filled), the offsets of both, the row offsets and 8 or 12 bytes per stored hit
        close_call(scope, got.cells, (filled ? 2 : 1) * (cp ? 4 : 1) * got.symbols + 2 * (count + 1) * 8 + (count + 1) * 8 +
                                         (filled ? csr.total * (r.starts ? 12 : 8) : 0));
        return swh_success_k;
    });
}

static swh_status_t infix_all_checks(swh_levenshtein_t e, size_t p_count, size_t t_count, uint32_t select, const InfixAllOutputs &r,
                                     const char **error) {
    const Engine *engine = (const Engine *)e;
    if (engine->kind != 0) return fail(error, swh_invalid_argument_k, "not a Levenshtein engine");
    if (!engine->unit_costs) return fail(error, swh_not_implemented_k, "infix search needs unit costs (match 0, mismatch 1, open 1, extend 1)");
    if (p_count != t_count) return fail(error, swh_invalid_argument_k, "patterns and texts must hold the same number of strings");
    if (select > SWH_INFIX_SELECT_MINIMA) return fail(error, swh_invalid_argument_k, "select must be one of SWH_INFIX_SELECT_ALL, _BEST, _MINIMA");
    // (infix_all's own rule, where it has always stood: after the row offsets and "both or neither", before the capacity)
    if (r.row_offsets && !r.ends && !r.distances && r.starts) return fail(error, swh_invalid_argument_k, "starts without ends and distances");
    return csr_output_checks(r.row_offsets, r.ends, r.distances, "ends and distances", true, r.capacity, error);
}

static swh_status_t infix_all_tapes(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *patterns, const swh_tape_u64_t *texts, bool utf8,
                                    uint32_t bound, uint32_t select, const InfixAllOutputs &outs, const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    if (!patterns || !texts) return fail(error, swh_invalid_argument_k, "null tape");
    if ((status = infix_all_checks(e, patterns->count, texts->count, select, outs, error)) != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.begin(s, error)) != swh_success_k) return status;
    const bool pairs = patterns->count != 0;
    if ((status = call.prepare(patterns, texts, utf8, pairs, pairs, error)) != swh_success_k) return status;
    return infix_all_run(call.scope, call.pair, bound, select, outs, error);
}
swh_status_t swh_levenshtein_infix_all_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *patterns, const swh_tape_u64_t *texts,
                                               uint32_t bound, uint32_t select, size_t *row_offsets, uint32_t *starts, uint32_t *ends,
                                               uint32_t *distances, size_t capacity, const char **error) {
    return infix_all_tapes(e, s, patterns, texts, false, bound, select, InfixAllOutputs{row_offsets, starts, ends, distances, capacity}, error);
}
swh_status_t swh_levenshtein_utf8_infix_all_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *patterns,
                                                    const swh_tape_u64_t *texts, uint32_t bound, uint32_t select, size_t *row_offsets,
                                                    uint32_t *starts, uint32_t *ends, uint32_t *distances, size_t capacity, const char **error) {
    return infix_all_tapes(e, s, patterns, texts, true, bound, select, InfixAllOutputs{row_offsets, starts, ends, distances, capacity}, error);
}
swh_status_t swh_levenshtein_infix_all_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *patterns,
                                                const swh_prepared_view_t *texts, uint32_t bound, uint32_t select, size_t *row_offsets,
                                                uint32_t *starts, uint32_t *ends, uint32_t *distances, size_t capacity, const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.views(patterns, texts, false, error)) != swh_success_k) return status;
    const InfixAllOutputs outs{row_offsets, starts, ends, distances, capacity};
    if ((status = infix_all_checks(e, call.pair.a_count, call.pair.b_count, select, outs, error)) != swh_success_k) return status;
    if ((status = call.begin_on_views(s, error)) != swh_success_k) return status;
    return infix_all_run(call.scope, call.pair, bound, select, outs, error);
}

// ---- OSA distances, LCS lengths / Indel distances, partial ratios, Jaro counts (osa.hip, lcs.hip, partial.hip, jaro.hip): one planner ------
// The four families score pairs on the same phases. A sizes kernel measures the pairs (cells, symbols, the first pair over the
// family's length limit) and cuts them into work items; one read-back of the measurements decides the errors before any output is
// written; the family's kernel scores the items and writes whichever of its outputs the caller asked for. A pairwise call is one such
// round. A cross-product maps pair p to (p / nb, p % nb) and runs in slices of whole rows of about kScoredChunkPairs pairs -- the item
// list and, per output that lives on the host, the staged slice are all the scratch there is, whatever the matrix size; with more
// than one slice the whole matrix is measured first (no items), so that a refusal still comes before the first row is written. The
// family's test hook (test library) lowers the slice, to put many of them in a small test. The scratch is the scope's alignment
// scratch: the calls are synchronous, and they learn nothing into the scope.
// What a family brings is its ScoredFamily: the two launchers, its words, and the few argument rules that differ.
//  - OSA: k_osa_sizes cuts the items by the blocks of a pair's shorter string, which holds at most SWH_OSA_MAX_SHORTER symbols; one output.
//  - LCS / Indel: OSA's sizes kernel and limit as they stand (SWH_LCS_MAX_SHORTER); two outputs, indel and lcs.
//  - Jaro: k_jaro_sizes cuts the items by the blocks of b, and neither string holds more than SWH_JARO_MAX_LENGTH symbols; three
//    outputs, matches, transpositions and prefix, and the only family that holds strides to multiples of the element.
//  - Partial ratio: k_partial_sizes gives a pair an item per run of its windows, so a slice's items are counted, the item part of the
//    scratch sized by the count, and the items placed by a second measurement (`item_bytes`); they are scored once per slice (`score`)
//    and the launch merges each pair's records into its four outputs, lcs, starts, ends and sides. SWH_PARTIAL_MAX_NEEDLE on the shorter string.
constexpr uint64_t kScoredChunkPairs = (uint64_t)1 << 21;
constexpr int kScoredOutputs = 4;

struct ScoredFamily {
    int outputs;   // of kScoredOutputs
    // measures the pairs and, with `items`, cuts them (`counted`: the items an earlier measurement found, where item_bytes asks for one)
    void (*sizes)(Scope *scope, const OsaTapes &t, OsaSizes *sizes, void *items, uint64_t counted);
    // scores the items into where[0 .. outputs), null where an output is not written by this launch, all at `stride`
    void (*launch)(Scope *scope, const OsaTapes &t, const void *items, uint64_t item_count, char *const where[kScoredOutputs], uint64_t stride,
                   uint32_t bound, bool wide);
    const char *chunk_hook;      // the test hook that lowers the slice
    const char *oversize;        // how the refusal of a pair over the length limit ends
    const char *unit_costs;      // the refusal of a general-cost engine
    const char *null_outputs;    // the refusal of a call that wants no output ...
    bool null_outputs_on_empty;  // ... which a call without pairs meets too
    bool element_strides;        // strides are multiples of the element (4 bytes pairwise, 8 cross), not merely large enough
    // Null: a pair is at most one LaneItem, and the first measurement of a slice cuts it. Otherwise the family's items follow from the
    // pairs' lengths: every slice is measured once to count them, the item scratch is sized by item_bytes(pairs, items), and a second
    // measurement cuts.
    size_t (*item_bytes)(uint64_t pairs, uint64_t items) = nullptr;
    // Null: `launch` does the scoring. Otherwise the items are scored once per slice here, and `launch` only writes outputs from
    // what this left in the item scratch (a slice with outputs in host and in device memory launches twice).
    void (*score)(Scope *scope, const OsaTapes &t, void *items, uint64_t item_count, bool wide) = nullptr;
};

static const ScoredFamily kOsaFamily = {
    1, [](Scope *scope, const OsaTapes &t, OsaSizes *sizes, void *items, uint64_t) { launch_osa_sizes(scope, t, sizes, (LaneItem *)items); },
    [](Scope *scope, const OsaTapes &t, const void *items, uint64_t item_count, char *const where[kScoredOutputs], uint64_t stride, uint32_t bound,
       bool wide) {
        OsaRun run{};
        run.items = (const LaneItem *)items; run.item_count = item_count;
        run.out = where[0];
        run.stride = stride; run.bound = bound; run.wide = wide;
        launch_osa(scope, t, run);
    },
    "STRINGWARS_AMD_OSA_CHUNK_PAIRS", "the shorter string exceeds SWH_OSA_MAX_SHORTER (2048)",
    "OSA distances need unit costs (match 0, mismatch 1, open 1, extend 1)", "null output pointer", false, false};
static const ScoredFamily kLcsFamily = {
    2, [](Scope *scope, const OsaTapes &t, OsaSizes *sizes, void *items, uint64_t) { launch_osa_sizes(scope, t, sizes, (LaneItem *)items); },
    [](Scope *scope, const OsaTapes &t, const void *items, uint64_t item_count, char *const where[kScoredOutputs], uint64_t stride, uint32_t bound,
       bool wide) {
        LcsRun run{};
        run.items = (const LaneItem *)items; run.item_count = item_count;
        run.indel = where[0]; run.lcs = where[1];
        run.stride = stride; run.bound = bound; run.wide = wide;
        launch_lcs(scope, t, run);
    },
    "STRINGWARS_AMD_LCS_CHUNK_PAIRS", "the shorter string exceeds SWH_LCS_MAX_SHORTER (2048)",
    "LCS lengths and Indel distances are called on a unit-cost engine (match 0, mismatch 1, open 1, extend 1)",
    "null output pointers: one of indel and lcs is needed", true, false};
static const ScoredFamily kJaroFamily = {
    3, [](Scope *scope, const OsaTapes &t, OsaSizes *sizes, void *items, uint64_t) { launch_jaro_sizes(scope, t, sizes, (LaneItem *)items); },
    [](Scope *scope, const OsaTapes &t, const void *items, uint64_t item_count, char *const where[kScoredOutputs], uint64_t stride, uint32_t,
       bool wide) {
        JaroRun run{};
        run.items = (const LaneItem *)items; run.item_count = item_count;
        run.matches = where[0]; run.transpositions = where[1]; run.prefix = where[2];
        run.stride = stride; run.wide = wide;
        launch_jaro(scope, t, run);
    },
    "STRINGWARS_AMD_JARO_CHUNK_PAIRS", "a string exceeds SWH_JARO_MAX_LENGTH (2048)",
    "Jaro and Jaro-Winkler counts are called on a unit-cost engine (match 0, mismatch 1, open 1, extend 1)",
    "null output pointers: one of matches, transpositions and prefix is needed", true, true};
// Partial ratio: k_partial_sizes gives a pair an item per run of its n + m - 1 windows (per direction), so the items are counted before
// they are placed; k_partial scores them into records once per slice, and the launch merges each pair's records into its outputs.
static const ScoredFamily kPartialFamily = {
    4, [](Scope *scope, const OsaTapes &t, OsaSizes *sizes, void *items, uint64_t counted) { launch_partial_sizes(scope, t, sizes, items, counted); },
    [](Scope *scope, const OsaTapes &t, const void *items, uint64_t item_count, char *const where[kScoredOutputs], uint64_t stride, uint32_t, bool) {
        launch_partial_merge(scope, t, PartialMerge{items, where[0], where[1], where[2], where[3], stride}, item_count);
    },
    "STRINGWARS_AMD_PARTIAL_CHUNK_PAIRS", "the shorter string exceeds SWH_PARTIAL_MAX_NEEDLE (2048)",
    "partial ratios are called on a unit-cost engine (match 0, mismatch 1, open 1, extend 1)",
    "null output pointers: one of lcs, starts, ends and sides is needed", true, false,
    partial_scratch_bytes, launch_partial_items};

static uint64_t scored_chunk_pairs(const char *chunk_hook) {
    const char *hook = test_hook(chunk_hook);
    const uint64_t pairs = hook ? (uint64_t)atoll(hook) : kScoredChunkPairs;
    return std::max<uint64_t>(1, std::min<uint64_t>(pairs, kScoredChunkPairs));
}

struct ScoredRequest {
    bool cross;
    uint32_t bound;
    void *outs[kScoredOutputs];   // the family's outputs in the order of its exports: any may be null, those past its count are
    size_t stride;                // bytes between consecutive results (pairs) or rows (cross), of every output
};

// The pieces of a scored launch, which the score search (extract_run) scores its slices on too.
// Strings [a_first, a_first + na) x [b_first, b_first + nb) of the call's two views: pair p is (p / nb, p % nb) of a cross-product,
// (p, p) of a pairwise call.
static OsaTapes scored_view(const TapePair &p, size_t a_first, size_t na, size_t b_first, size_t nb, bool cross) {
    const bool cp = p.pa->utf8;
    OsaTapes t{};
    t.a = tape_side(p.pa, cp, p.a_first + a_first, na, t.a_off64);
    t.b = tape_side(p.pb, cp, p.b_first + b_first, nb, t.b_off64);
    t.cp = cp ? 1 : 0;
    t.nb = cross ? nb : 0;
    return t;
}
// makes `pairs` pairs from row `row0` on the view's launch, measures them and, with `items`, cuts them into items
static OsaSizes scored_measure(Scope *scope, const ScoredFamily &f, OsaTapes &t, uint64_t row0, uint64_t pairs, OsaSizes *sizes, void *items,
                               uint64_t counted = 0) {
    t.row0 = row0; t.count = pairs;
    return measure(scope, sizes, [&] { f.sizes(scope, t, sizes, items, counted); });
}
// both byte tapes hold at least 16 bytes: the kernels read the columns' string with 128-bit loads
static bool scored_wide(const OsaTapes &t, const OsaSizes &got) { return !t.cp && got.a_total >= 16 && got.b_total >= 16; }
// the refusal of pair (i, j) of the view, whose strings are over the family's length limit
static swh_status_t scored_oversize(const ScoredFamily &f, const OsaTapes &t, size_t i, size_t j, bool cross, hipStream_t stream, const char **error) {
    const uint64_t la = string_symbols(t.a, t.a_off64, i, stream), lb = string_symbols(t.b, t.b_off64, j, stream);
    if (cross)
        return fail(error, swh_unsupported_length_k, "pair (%zu, %zu): %llu x %llu symbols, %s", i, j, (unsigned long long)la,
                    (unsigned long long)lb, f.oversize);
    return fail(error, swh_unsupported_length_k, "pair %zu: %llu x %llu symbols, %s", i, (unsigned long long)la, (unsigned long long)lb, f.oversize);
}

static swh_status_t scored_run(Scope *scope, const ScoredFamily &f, const TapePair &p, const ScoredRequest &r, const char **error) {
    return synchronous_run(scope, error, [&]() -> swh_status_t {
        const uint64_t na = p.a_count, nb = p.b_count;
        if (na == 0 || nb == 0) return swh_success_k;
        if (r.cross && na > ((uint64_t)1 << 40) / nb) return fail(error, swh_unsupported_length_k, "more than 2^40 pairs in one call");
        const uint64_t total = r.cross ? na * nb : na;
        SWH_HIP_CHECK(hipSetDevice(scope->device));
        hipStream_t stream = scope->stream;
        // (an output the caller does not want is null, as are those past the family's count: not staged, not written)
        Staged<char> outs[kScoredOutputs] = {Staged<char>((char *)r.outs[0]), Staged<char>((char *)r.outs[1]), Staged<char>((char *)r.outs[2]),
                                             Staged<char>((char *)r.outs[3])};
        size_t staged_count = 0, wanted = 0;
        for (int k = 0; k < f.outputs; ++k) { staged_count += outs[k].on_device ? 0 : 1; wanted += r.outs[k] ? 1 : 0; }
        OsaTapes t = scored_view(p, 0, na, 0, nb, r.cross);

        // slices: all pairs of a pairwise call; whole rows of a cross-product
        const uint64_t rows_per_slice = r.cross ? std::max<uint64_t>(1, scored_chunk_pairs(f.chunk_hook) / nb) : na;
        const uint64_t slices = (na + rows_per_slice - 1) / rows_per_slice;
        const uint64_t slice_pairs = r.cross ? std::min<uint64_t>(rows_per_slice, na) * nb : na;
        const size_t width = r.cross ? 8 : 4;

        AlignScratch *sc_entry = call_scratch(scope);
        // sizes | the slice's results (one array per output that lives on the host) | items. A family that counts its items sizes
        // the last part slice by slice: the scratch is laid out again -- nothing in it outlives a slice -- once the count is known.
        OsaSizes *sizes;
        char *items;
        auto lay_out = [&](size_t item_bytes) {
            const size_t need = pad(sizeof(OsaSizes)) + staged_count * pad(slice_pairs * width) + pad(item_bytes);
            Carver sc = carve(sc_entry->buf, sc_entry->bytes, need);
            sizes = sc.take<OsaSizes>(1);
            for (int k = 0; k < f.outputs; ++k) outs[k].place(sc, slice_pairs * width);
            items = sc.take<char>(item_bytes);
        };
        lay_out(f.item_bytes ? 0 : slice_pairs * sizeof(LaneItem));

        // with more than one slice the whole matrix is measured first (no items): a refusal comes before the first row is written
        const OsaSizes whole = scored_measure(scope, f, t, 0, total, sizes, slices == 1 && !f.item_bytes ? items : nullptr);
        if (whole.first_oversize != ~0ull) {
            scope->stamps_used = 0;
            const size_t first = (size_t)whole.first_oversize;
            return scored_oversize(f, t, r.cross ? first / nb : first, r.cross ? first % nb : first, r.cross, stream, error);
        }

        const bool wide = scored_wide(t, whole);
        // the kernel writes its outputs at one stride: the caller's for those written in place, the packed one for those that are
        // staged; a call with outputs of both kinds runs the slice once per kind
        for (uint64_t q = 0; q < slices; ++q) {
            const uint64_t row0 = q * rows_per_slice, rows = std::min<uint64_t>(rows_per_slice, na - row0);
            const uint64_t pairs = r.cross ? rows * nb : na;
            uint64_t item_count;
            if (f.item_bytes) {
                item_count = slices == 1 ? whole.items : scored_measure(scope, f, t, row0, pairs, sizes, nullptr).items;
                lay_out(f.item_bytes(pairs, item_count));
                scored_measure(scope, f, t, row0, pairs, sizes, items, item_count);
            } else {
                item_count = slices == 1 ? whole.items : scored_measure(scope, f, t, row0, pairs, sizes, items).items;
            }
            if (f.score) f.score(scope, t, items, item_count, wide);
            for (int packed = 0; packed < 2; ++packed) {
                char *where[kScoredOutputs] = {};
                bool any = false;
                for (int k = 0; k < f.outputs; ++k) {
                    if (!r.outs[k] || outs[k].on_device == (packed == 1)) continue;
                    where[k] = packed ? outs[k].dev : outs[k].out + (r.cross ? row0 * r.stride : 0);
                    any = true;
                }
                if (any) f.launch(scope, t, items, item_count, where, packed ? (r.cross ? nb * 8 : 4) : r.stride, r.bound, wide);
            }
            for (int k = 0; k < f.outputs; ++k) {   // at the caller's stride: Staged::copy_back is for contiguous outputs
                if (outs[k].on_device) continue;
                if (r.cross)
                    SWH_HIP_CHECK(hipMemcpy2DAsync(outs[k].out + row0 * r.stride, r.stride, outs[k].dev, nb * 8, nb * 8, rows, hipMemcpyDeviceToHost, stream));
                else if (r.stride == 4)
                    outs[k].copy_back(stream, pairs * 4);
                else
                    SWH_HIP_CHECK(hipMemcpy2DAsync(outs[k].out, r.stride, outs[k].dev, 4, 4, pairs, hipMemcpyDeviceToHost, stream));
            }
            if (staged_count) SWH_HIP_CHECK(hipStreamSynchronize(stream));   // the next slice reuses the staging
        }
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        close_call(scope, whole.cells, (t.cp ? 4 : 1) * whole.symbols + (na + nb + 2) * 8 + total * width * wanted);
        return swh_success_k;
    });
}

// the argument rules; a stride of 0 becomes the packed one
static swh_status_t scored_checks(const ScoredFamily &f, swh_levenshtein_t e, size_t a_count, size_t b_count, bool cross,
                                  void *const (&outs)[kScoredOutputs], size_t &stride, const char **error) {
    const Engine *engine = (const Engine *)e;
    if (engine->kind != 0) return fail(error, swh_invalid_argument_k, "not a Levenshtein engine");
    if (!engine->unit_costs) return fail(error, swh_not_implemented_k, "%s", f.unit_costs);
    if (!cross && a_count != b_count) return fail(error, swh_invalid_argument_k, "a and b must hold the same number of strings");
    bool wanted = false;
    for (int k = 0; k < f.outputs; ++k) wanted = wanted || outs[k];
    if (!wanted && (f.null_outputs_on_empty || (a_count && b_count))) return fail(error, swh_invalid_argument_k, "%s", f.null_outputs);
    if (cross) {
        if (!stride) stride = b_count * 8;
        if (f.element_strides && stride % 8) return fail(error, swh_invalid_argument_k, "row_stride_bytes must be 0 or a multiple of 8");
        if (stride < b_count * 8) return fail(error, swh_invalid_argument_k, "row_stride_bytes too small");
    } else {
        if (!stride) stride = 4;
        if (f.element_strides && stride % 4) return fail(error, swh_invalid_argument_k, "out_stride_bytes must be 0 or a multiple of 4");
        if (stride < 4) return fail(error, swh_invalid_argument_k, "out_stride_bytes must be >= 4");
    }
    return swh_success_k;
}

static swh_status_t scored_tapes(const ScoredFamily &f, swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                 bool utf8, bool cross, uint32_t bound, void *const (&outs)[kScoredOutputs], size_t stride, const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    if (!a || (!b && !cross)) return fail(error, swh_invalid_argument_k, "null tape");
    const size_t b_count = (b ? b : a)->count;   // a cross-product without b: the self-product
    status = scored_checks(f, e, a->count, b_count, cross, outs, stride, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.begin(s, error)) != swh_success_k) return status;
    const bool pairs = a->count && b_count;
    if ((status = call.prepare(a, b, utf8, pairs, pairs, error)) != swh_success_k) return status;
    return scored_run(call.scope, f, call.pair, ScoredRequest{cross, bound, {outs[0], outs[1], outs[2], outs[3]}, stride}, error);
}
static swh_status_t scored_prepared(const ScoredFamily &f, swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a,
                                    const swh_prepared_view_t *b, bool cross, uint32_t bound, void *const (&outs)[kScoredOutputs], size_t stride,
                                    const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.views(a, b, cross, error)) != swh_success_k) return status;
    if ((status = scored_checks(f, e, call.pair.a_count, call.pair.b_count, cross, outs, stride, error)) != swh_success_k) return status;
    if ((status = call.begin_on_views(s, error)) != swh_success_k) return status;
    return scored_run(call.scope, f, call.pair, ScoredRequest{cross, bound, {outs[0], outs[1], outs[2], outs[3]}, stride}, error);
}

swh_status_t swh_levenshtein_osa_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b, uint32_t bound,
                                               uint32_t *out, size_t stride, const char **error) {
    return scored_tapes(kOsaFamily, e, s, a, b, false, false, bound, {out}, stride, error);
}
swh_status_t swh_levenshtein_utf8_osa_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                    uint32_t bound, uint32_t *out, size_t stride, const char **error) {
    return scored_tapes(kOsaFamily, e, s, a, b, true, false, bound, {out}, stride, error);
}
swh_status_t swh_levenshtein_osa_pairs_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                                uint32_t bound, uint32_t *out, size_t stride, const char **error) {
    return scored_prepared(kOsaFamily, e, s, a, b, false, bound, {out}, stride, error);
}
swh_status_t swh_levenshtein_osa_cross_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b, size_t *out,
                                               size_t row_stride, const char **error) {
    return scored_tapes(kOsaFamily, e, s, a, b, false, true, SWH_UNBOUNDED, {out}, row_stride, error);
}
swh_status_t swh_levenshtein_utf8_osa_cross_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                    size_t *out, size_t row_stride, const char **error) {
    return scored_tapes(kOsaFamily, e, s, a, b, true, true, SWH_UNBOUNDED, {out}, row_stride, error);
}
swh_status_t swh_levenshtein_osa_cross_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                                size_t *out, size_t row_stride, const char **error) {
    return scored_prepared(kOsaFamily, e, s, a, b, true, SWH_UNBOUNDED, {out}, row_stride, error);
}

swh_status_t swh_levenshtein_lcs_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b, uint32_t bound,
                                               uint32_t *indel, uint32_t *lcs, size_t stride, const char **error) {
    return scored_tapes(kLcsFamily, e, s, a, b, false, false, bound, {indel, lcs}, stride, error);
}
swh_status_t swh_levenshtein_utf8_lcs_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                    uint32_t bound, uint32_t *indel, uint32_t *lcs, size_t stride, const char **error) {
    return scored_tapes(kLcsFamily, e, s, a, b, true, false, bound, {indel, lcs}, stride, error);
}
swh_status_t swh_levenshtein_lcs_pairs_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                                uint32_t bound, uint32_t *indel, uint32_t *lcs, size_t stride, const char **error) {
    return scored_prepared(kLcsFamily, e, s, a, b, false, bound, {indel, lcs}, stride, error);
}
swh_status_t swh_levenshtein_lcs_cross_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b, size_t *indel,
                                               size_t *lcs, size_t row_stride, const char **error) {
    return scored_tapes(kLcsFamily, e, s, a, b, false, true, SWH_UNBOUNDED, {indel, lcs}, row_stride, error);
}
swh_status_t swh_levenshtein_utf8_lcs_cross_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                    size_t *indel, size_t *lcs, size_t row_stride, const char **error) {
    return scored_tapes(kLcsFamily, e, s, a, b, true, true, SWH_UNBOUNDED, {indel, lcs}, row_stride, error);
}
swh_status_t swh_levenshtein_lcs_cross_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                                size_t *indel, size_t *lcs, size_t row_stride, const char **error) {
    return scored_prepared(kLcsFamily, e, s, a, b, true, SWH_UNBOUNDED, {indel, lcs}, row_stride, error);
}

// (no bound: there is no score cutoff)
swh_status_t swh_levenshtein_partial_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                   uint32_t *lcs, uint32_t *starts, uint32_t *ends, uint32_t *sides, size_t stride, const char **error) {
    return scored_tapes(kPartialFamily, e, s, a, b, false, false, SWH_UNBOUNDED, {lcs, starts, ends, sides}, stride, error);
}
swh_status_t swh_levenshtein_utf8_partial_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                        uint32_t *lcs, uint32_t *starts, uint32_t *ends, uint32_t *sides, size_t stride,
                                                        const char **error) {
    return scored_tapes(kPartialFamily, e, s, a, b, true, false, SWH_UNBOUNDED, {lcs, starts, ends, sides}, stride, error);
}
swh_status_t swh_levenshtein_partial_pairs_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                                    uint32_t *lcs, uint32_t *starts, uint32_t *ends, uint32_t *sides, size_t stride,
                                                    const char **error) {
    return scored_prepared(kPartialFamily, e, s, a, b, false, SWH_UNBOUNDED, {lcs, starts, ends, sides}, stride, error);
}
swh_status_t swh_levenshtein_partial_cross_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                   size_t *lcs, size_t *starts, size_t *ends, size_t *sides, size_t row_stride, const char **error) {
    return scored_tapes(kPartialFamily, e, s, a, b, false, true, SWH_UNBOUNDED, {lcs, starts, ends, sides}, row_stride, error);
}
swh_status_t swh_levenshtein_utf8_partial_cross_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                        size_t *lcs, size_t *starts, size_t *ends, size_t *sides, size_t row_stride,
                                                        const char **error) {
    return scored_tapes(kPartialFamily, e, s, a, b, true, true, SWH_UNBOUNDED, {lcs, starts, ends, sides}, row_stride, error);
}
swh_status_t swh_levenshtein_partial_cross_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                                    size_t *lcs, size_t *starts, size_t *ends, size_t *sides, size_t row_stride,
                                                    const char **error) {
    return scored_prepared(kPartialFamily, e, s, a, b, true, SWH_UNBOUNDED, {lcs, starts, ends, sides}, row_stride, error);
}

// (the Jaro kernel takes no bound)
swh_status_t swh_levenshtein_jaro_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                uint32_t *matches, uint32_t *transpositions, uint32_t *prefix, size_t stride, const char **error) {
    return scored_tapes(kJaroFamily, e, s, a, b, false, false, SWH_UNBOUNDED, {matches, transpositions, prefix}, stride, error);
}
swh_status_t swh_levenshtein_utf8_jaro_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                     uint32_t *matches, uint32_t *transpositions, uint32_t *prefix, size_t stride, const char **error) {
    return scored_tapes(kJaroFamily, e, s, a, b, true, false, SWH_UNBOUNDED, {matches, transpositions, prefix}, stride, error);
}
swh_status_t swh_levenshtein_jaro_pairs_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                                 uint32_t *matches, uint32_t *transpositions, uint32_t *prefix, size_t stride, const char **error) {
    return scored_prepared(kJaroFamily, e, s, a, b, false, SWH_UNBOUNDED, {matches, transpositions, prefix}, stride, error);
}
swh_status_t swh_levenshtein_jaro_cross_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                size_t *matches, size_t *transpositions, size_t *prefix, size_t row_stride, const char **error) {
    return scored_tapes(kJaroFamily, e, s, a, b, false, true, SWH_UNBOUNDED, {matches, transpositions, prefix}, row_stride, error);
}
swh_status_t swh_levenshtein_utf8_jaro_cross_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                     size_t *matches, size_t *transpositions, size_t *prefix, size_t row_stride, const char **error) {
    return scored_tapes(kJaroFamily, e, s, a, b, true, true, SWH_UNBOUNDED, {matches, transpositions, prefix}, row_stride, error);
}
swh_status_t swh_levenshtein_jaro_cross_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                                 size_t *matches, size_t *transpositions, size_t *prefix, size_t row_stride, const char **error) {
    return scored_prepared(kJaroFamily, e, s, a, b, true, SWH_UNBOUNDED, {matches, transpositions, prefix}, row_stride, error);
}

// ---- token-sorted tapes and token_set_ratio (tokens.hip) ---------------------------------------------------------------------------------
// A normal form is never longer than its string, and neither are the two differences of a pair's token sets. So the kernels write
// into staging laid out like their source and leave the lengths beside it; the lengths become offsets through the offsets scan
// (scan.hpp), k_token_compact moves the results into buffers of their own, and prepare_tape measures those in place like
// any device tape (and decodes them, in UTF-8 mode): the handle that comes out owns them and is a prepared tape like every other.
// token_set_ratio derives the SWH_TOKENS_UNIQUE forms of both sides (or takes a tape that already is one), asks the LCS family's sizes
// kernel for the first pair it would refuse -- x <= len(a'), y <= len(b'), so the rule of ratio on the normal forms covers the
// differences -- splits every pair (k_token_set_split: s, x, y and the bytes of X and Y) and runs the LCS pairs route on the two
// difference tapes for L.
struct DeviceBuffer {
    void *p = nullptr;
    ~DeviceBuffer() { if (p) (void)hipFree(p); }
    void *alloc(size_t bytes) { SWH_HIP_CHECK(hipMalloc(&p, bytes ? bytes : 16)); return p; }
    void *release() { void *q = p; p = nullptr; return q; }
};

// strings [first, first + count) of a prepared tape as the token kernels read them (up to two reads and waits)
static TokenSide token_side(const Prepared *p, size_t first, size_t count, hipStream_t stream) {
    TokenSide s{};
    s.view = prepared_view(p, false, first, count);
    s.off64 = p->off64;
    s.total = p->total_bytes;
    s.base = first == 0 ? p->first_byte : std::min(read_offset(s.view.offsets, (int)p->off64, 0, true, stream), s.total);
    const uint64_t end = first + count == p->bytes.count ? s.total : std::min(read_offset(s.view.offsets, (int)p->off64, count, true, stream), s.total);
    s.span = end > s.base ? end - s.base : 0;
    return s;
}

// What a scan of `count` lengths needs beside them, and the tape it leads to.
struct TokenScan {
    ScanScratch scratch;
    uint64_t *offsets;
    static size_t need(uint64_t count) { return ScanScratch::need(count) + pad((count + 1) * 8); }
    void place(Carver &sc, uint64_t count) {
        scratch.place(sc, count);
        offsets = sc.take<uint64_t>(count + 1);
    }
};
struct TokenTape {
    DeviceBuffer data, offsets;
    uint32_t off64 = 0;
};
// the results of `like`'s strings, `lengths` bytes each in `staging`, as a tape of its own with `off64`-wide offsets (one read and wait)
static void token_pack(Scope *scope, const TokenSide &like, const uint8_t *staging, const uint32_t *lengths, const TokenScan &scan, uint32_t off64,
                       TokenTape &tape) {
    const uint64_t count = like.view.count;
    launch_offsets_scan(scope, lengths, count, 1, scan.scratch, nullptr, scan.offsets);
    const uint64_t total = read_offset(scan.offsets, 1, count, true, scope->stream);
    TokenCompact c{};
    c.like = like; c.staging = staging; c.lengths = lengths; c.starts = scan.offsets;
    c.out = (uint8_t *)tape.data.alloc(total + 16);
    c.out_offsets = tape.offsets.alloc((count + 1) * (off64 ? 8 : 4) + 16);
    c.out_off64 = tape.off64 = off64;
    launch_token_compact(scope, c);
}
// measures a packed tape in place and hands its buffers to the handle
static swh_status_t token_adopt(Scope *scope, TokenTape &tape, uint64_t count, bool utf8, int form, Prepared **out, const char **error) {
    swh_prepared_t handle = nullptr;
    const HostTape host{(const uint8_t *)tape.data.p, tape.offsets.p, (size_t)count, (int)tape.off64};
    const swh_status_t status = prepare_tape(scope, host, utf8, &handle, error);
    if (status != swh_success_k) return status;
    Prepared *p = (Prepared *)handle;
    p->owned.push_back(tape.data.release());
    p->owned.push_back(tape.offsets.release());
    p->token_form = form;
    *out = p;
    return swh_success_k;
}

// The tape of normal forms of strings [first, first + count) of `src`, on a scope held synchronous. HIP failures are thrown.
static swh_status_t token_derive(Scope *scope, const Prepared *src, size_t first, size_t count, int form, Prepared **out, const char **error) {
    *out = nullptr;
    SWH_HIP_CHECK(hipSetDevice(scope->device));
    hipStream_t stream = scope->stream;
    TokenTape tape;
    if (count == 0) {   // a valid empty tape: offsets[0] = 0
        tape.off64 = src->off64;
        tape.data.alloc(16);
        SWH_HIP_CHECK(hipMemsetAsync(tape.offsets.alloc(16), 0, 16, stream));
        return token_adopt(scope, tape, 0, src->utf8, form, out, error);
    }
    const TokenSide side = token_side(src, first, count, stream);
    DeviceBuffer work;
    Carver sc{(char *)work.alloc(pad(8) + pad(side.span) + pad(count * 4) + TokenScan::need(count)), 0, 0};
    TokenDerive d{};
    d.src = side; d.utf8 = src->utf8 ? 1 : 0; d.form = (uint32_t)form;
    d.first_oversize = sc.take<unsigned long long>(1);
    d.staging = sc.take<uint8_t>(side.span);
    d.lengths = sc.take<uint32_t>(count);
    TokenScan scan;
    scan.place(sc, count);
    // the launch for short strings where the tape's longest is one; it runs again for long ones if the tape's memory has changed since
    bool small = src->longest_bytes <= kTokenSmallBytes;
    unsigned long long oversize = ~0ull;
    for (;;) {
        SWH_HIP_CHECK(hipMemsetAsync(d.first_oversize, 0xFF, 8, stream));
        launch_token_derive(scope, d, small);
        SWH_HIP_CHECK(hipMemcpyAsync(&oversize, d.first_oversize, 8, hipMemcpyDeviceToHost, stream));
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        if (oversize == ~0ull || !small) break;
        small = false;
    }
    if (oversize != ~0ull) {
        const uint64_t bytes = string_symbols(side.view, side.off64, (size_t)oversize, stream);
        scope->stamps_used = 0;
        return fail(error, swh_unsupported_length_k, "string %llu: %llu bytes exceed SWH_TOKEN_MAX_BYTES (4096)", oversize, (unsigned long long)bytes);
    }
    token_pack(scope, side, d.staging, d.lengths, scan, src->off64, tape);
    SWH_HIP_CHECK(hipStreamSynchronize(stream));   // (before the staging goes)
    return token_adopt(scope, tape, count, src->utf8, form, out, error);
}

swh_status_t swh_tape_token_sort(swh_scope_t s, const swh_prepared_view_t *view, int form, swh_prepared_t *out, const char **error) {
    if (out) *out = nullptr;
    if (!s) return probe_null_handles(nullptr, nullptr, error);   // (no device, where none is visible)
    if (!out) return fail(error, swh_invalid_argument_k, "null output");
    if (!view || !view->tape) return fail(error, swh_invalid_argument_k, "null prepared view");
    if (form != SWH_TOKENS_SORTED && form != SWH_TOKENS_UNIQUE)
        return fail(error, swh_invalid_argument_k, "form must be SWH_TOKENS_SORTED or SWH_TOKENS_UNIQUE");
    if (!view_fits(view)) return fail(error, swh_invalid_argument_k, "view exceeds the prepared tape");
    const Prepared *src = (const Prepared *)view->tape;
    if (src->device != ((Scope *)s)->device) return fail(error, swh_invalid_argument_k, "a prepared tape lives on another device than the scope");
    TwoTapeCall call;
    const swh_status_t status = call.begin(s, error);
    if (status != swh_success_k) return status;
    return synchronous_run(call.scope, error, [&]() -> swh_status_t {
        Prepared *derived = nullptr;
        const swh_status_t made = token_derive(call.scope, src, view->first, view->count, form, &derived, error);
        if (made != swh_success_k) return made;
        *out = (swh_prepared_t)derived;
        close_call(call.scope, 0, src->total_bytes + derived->total_bytes);
        return swh_success_k;
    });
}

swh_status_t swh_prepared_read(swh_scope_t s, swh_prepared_t prepared, void *data, size_t *offsets, const char **error) {
    static_assert(sizeof(size_t) == sizeof(uint64_t), "the offsets are read as 64-bit words");
    if (!s) return probe_null_handles(nullptr, nullptr, error);   // (no device, where none is visible)
    if (!prepared || !offsets) return fail(error, swh_invalid_argument_k, "null tape or offsets");
    const Prepared *p = (const Prepared *)prepared;
    if (p->device != ((Scope *)s)->device) return fail(error, swh_invalid_argument_k, "a prepared tape lives on another device than the scope");
    TwoTapeCall call;
    const swh_status_t status = call.begin(s, error);
    if (status != swh_success_k) return status;
    return synchronous_run(call.scope, error, [&]() -> swh_status_t {
        SWH_HIP_CHECK(hipSetDevice(call.scope->device));
        hipStream_t stream = call.scope->stream;
        const size_t count = (size_t)p->bytes.count;
        if (p->off64) {
            SWH_HIP_CHECK(hipMemcpyAsync(offsets, p->bytes.offsets, (count + 1) * 8, hipMemcpyDeviceToHost, stream));
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
        } else {
            std::vector<uint32_t> narrow(count + 1);
            SWH_HIP_CHECK(hipMemcpyAsync(narrow.data(), p->bytes.offsets, (count + 1) * 4, hipMemcpyDeviceToHost, stream));
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            for (size_t i = 0; i <= count; ++i) offsets[i] = narrow[i];
        }
        const uint64_t base = std::min<uint64_t>(offsets[0], p->total_bytes);
        for (size_t i = 0; i <= count; ++i) offsets[i] = std::min<uint64_t>(std::max<uint64_t>(offsets[i], base), p->total_bytes) - base;
        if (data && offsets[count]) {
            SWH_HIP_CHECK(hipMemcpyAsync(data, (const uint8_t *)p->bytes.data + base, offsets[count], hipMemcpyDeviceToHost, stream));
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
        }
        return swh_success_k;
    });
}

struct TokenSetOutputs {
    uint32_t *sect, *ab, *ba, *lcs;
    size_t stride;
};
// `n` packed device words to an output of the caller's, in host or device memory, at its stride
static void token_set_copy(uint32_t *out, size_t stride, const uint32_t *dev, uint64_t n, hipStream_t stream) {
    if (!out) return;
    const hipMemcpyKind kind = is_device_pointer(out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (stride == 4) SWH_HIP_CHECK(hipMemcpyAsync(out, dev, n * 4, kind, stream));
    else SWH_HIP_CHECK(hipMemcpy2DAsync(out, stride, dev, 4, 4, n, kind, stream));
}

static swh_status_t token_set_run(Scope *scope, const TapePair &p, const TokenSetOutputs &r, const char **error) {
    const uint64_t n = p.a_count;
    if (n == 0) return swh_success_k;
    PreparedOwner unique_a, unique_b, x, y;
    const swh_status_t status = synchronous_run(scope, error, [&]() -> swh_status_t {
        SWH_HIP_CHECK(hipSetDevice(scope->device));
        hipStream_t stream = scope->stream;
        TapePair u = p;
        swh_status_t made = swh_success_k;
        if (p.pa->token_form != SWH_TOKENS_UNIQUE) {
            if ((made = token_derive(scope, p.pa, p.a_first, n, SWH_TOKENS_UNIQUE, &unique_a.p, error)) != swh_success_k) return made;
            u.pa = unique_a.p; u.a_first = 0;
        }
        if (p.pb->token_form != SWH_TOKENS_UNIQUE) {
            if ((made = token_derive(scope, p.pb, p.b_first, n, SWH_TOKENS_UNIQUE, &unique_b.p, error)) != swh_success_k) return made;
            u.pb = unique_b.p; u.b_first = 0;
        }
        // the first pair the LCS route would refuse on the normal forms, before anything is written
        AlignScratch *sc_entry = call_scratch(scope);
        Carver measuring = carve(sc_entry->buf, sc_entry->bytes, pad(sizeof(OsaSizes)));
        OsaTapes t = scored_view(u, 0, n, 0, n, false);
        const OsaSizes whole = scored_measure(scope, kLcsFamily, t, 0, n, measuring.take<OsaSizes>(1), nullptr);
        if (whole.first_oversize != ~0ull) {
            scope->stamps_used = 0;
            const size_t first = (size_t)whole.first_oversize;
            return scored_oversize(kLcsFamily, t, first, first, false, stream, error);
        }

        TokenSplit split{};
        split.a = token_side(u.pa, u.a_first, n, stream);
        split.b = token_side(u.pb, u.b_first, n, stream);
        split.utf8 = u.pa->utf8 ? 1 : 0;
        DeviceBuffer work;
        Carver sc{(char *)work.alloc(pad(split.a.span) + pad(split.b.span) + 5 * pad(n * 4) + TokenScan::need(n)), 0, 0};
        split.x_staging = sc.take<uint8_t>(split.a.span); split.y_staging = sc.take<uint8_t>(split.b.span);
        split.x_lengths = sc.take<uint32_t>(n); split.y_lengths = sc.take<uint32_t>(n);
        split.sect = sc.take<uint32_t>(n); split.ab = sc.take<uint32_t>(n); split.ba = sc.take<uint32_t>(n);
        TokenScan scan;
        scan.place(sc, n);
        launch_token_set_split(scope, split, u.pa->longest_bytes <= kTokenSmallBytes && u.pb->longest_bytes <= kTokenSmallBytes);
        token_set_copy(r.sect, r.stride, split.sect, n, stream);
        token_set_copy(r.ab, r.stride, split.ab, n, stream);
        token_set_copy(r.ba, r.stride, split.ba, n, stream);
        TokenTape tape_x, tape_y;
        if (r.lcs) {
            token_pack(scope, split.a, split.x_staging, split.x_lengths, scan, u.pa->off64, tape_x);
            token_pack(scope, split.b, split.y_staging, split.y_lengths, scan, u.pb->off64, tape_y);
        }
        SWH_HIP_CHECK(hipStreamSynchronize(stream));   // (before the staging goes)
        if (r.lcs) {
            if ((made = token_adopt(scope, tape_x, n, u.pa->utf8, -1, &x.p, error)) != swh_success_k) return made;
            if ((made = token_adopt(scope, tape_y, n, u.pb->utf8, -1, &y.p, error)) != swh_success_k) return made;
        }
        close_call(scope, 0, u.pa->total_bytes + u.pb->total_bytes + 3 * n * 4);
        return swh_success_k;
    });
    if (status != swh_success_k || !r.lcs) return status;
    TapePair differences;
    differences.pa = x.p; differences.pb = y.p; differences.a_count = differences.b_count = (size_t)n;
    return scored_run(scope, kLcsFamily, differences, ScoredRequest{false, SWH_UNBOUNDED, {nullptr, r.lcs, nullptr, nullptr}, r.stride}, error);
}

// the argument rules are the scored families' (scored_checks): this row holds the words of this call
static const ScoredFamily kTokenSetRules = {
    4, nullptr, nullptr, nullptr, "", "token set counts are called on a unit-cost engine (match 0, mismatch 1, open 1, extend 1)",
    "null output pointers: one of sect, ab, ba and lcs is needed", true, false};

static swh_status_t token_set_tapes(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b, bool utf8,
                                    void *const (&outs)[kScoredOutputs], size_t stride, const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    if (!a || !b) return fail(error, swh_invalid_argument_k, "null tape");
    if ((status = scored_checks(kTokenSetRules, e, a->count, b->count, false, outs, stride, error)) != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.begin(s, error)) != swh_success_k) return status;
    const bool pairs = a->count != 0;
    if ((status = call.prepare(a, b, utf8, pairs, pairs, error)) != swh_success_k) return status;
    return token_set_run(call.scope, call.pair, TokenSetOutputs{(uint32_t *)outs[0], (uint32_t *)outs[1], (uint32_t *)outs[2], (uint32_t *)outs[3], stride}, error);
}
swh_status_t swh_levenshtein_token_set_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                     uint32_t *sect, uint32_t *ab, uint32_t *ba, uint32_t *lcs, size_t stride, const char **error) {
    return token_set_tapes(e, s, a, b, false, {sect, ab, ba, lcs}, stride, error);
}
swh_status_t swh_levenshtein_utf8_token_set_pairs_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *a, const swh_tape_u64_t *b,
                                                          uint32_t *sect, uint32_t *ab, uint32_t *ba, uint32_t *lcs, size_t stride,
                                                          const char **error) {
    return token_set_tapes(e, s, a, b, true, {sect, ab, ba, lcs}, stride, error);
}
swh_status_t swh_levenshtein_token_set_pairs_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *a, const swh_prepared_view_t *b,
                                                      uint32_t *sect, uint32_t *ab, uint32_t *ba, uint32_t *lcs, size_t stride,
                                                      const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    void *const outs[kScoredOutputs] = {sect, ab, ba, lcs};
    TwoTapeCall call;
    if ((status = call.views(a, b, false, error)) != swh_success_k) return status;
    if ((status = scored_checks(kTokenSetRules, e, call.pair.a_count, call.pair.b_count, false, outs, stride, error)) != swh_success_k) return status;
    if ((status = call.begin_on_views(s, error)) != swh_success_k) return status;
    return token_set_run(call.scope, call.pair, TokenSetOutputs{sect, ab, ba, lcs, stride}, error);
}

// ---- score search (extract.hip): the k best candidates by an OSA, Indel, LCS, ratio, Jaro or Jaro-Winkler score ------------------------
// topk_run's general path with the three families as the scorers: query blocks x candidate slices of at most kScoredChunkPairs
// pairs, each slice measured and cut into items (scored_measure) and scored by the family's launcher into dense u64 counts in scratch
// (the candidates' slice is a view of the prepared tape: pair p of the launch is (p / columns, p % columns)) and folded into the
// block's running lists by k_extract_select, which evaluates the float64 score. The scratch is the slice's items and counts, the
// block's lists and, for outputs in host memory, the rows: nothing grows with queries x candidates. Both length limits follow from
// the two tapes' own lengths, so one pass over their offsets refuses the call before anything is scored or written.
// STRINGWARS_AMD_EXTRACT_CHUNK_PAIRS (test library) lowers the slice, to put several blocks and slices into a small test.
struct ExtractRequest {
    int scorer;
    uint32_t k;
    double cutoff, prefix_weight;
    uint32_t *indices;
    void *scores;
};

// What the two score searches (extract_run, extract_within_run) do alike: the family and its counts, the blocks and slices, the
// length pre-pass, and the walk that measures and scores every slice before the search's own kernel gets it. The search as one call:
// with profiling on, the kernels of every slice go into `sum`, the family's kernel as the dominant one.
extern "C++" {   // (its walk is a template)
struct ExtractSweep {
    Scope *scope; const TapePair &p; int scorer; double cutoff, prefix_weight;
    bool jaro; const ScoredFamily &f; int counts;
    OsaTapes whole;   // its two sides: the queries, the candidates
    uint64_t q_step, c_step, slice_pairs;
    unsigned long long *first_over = nullptr;
    OsaSizes *sizes = nullptr;
    LaneItem *items = nullptr;
    uint64_t *slice[kScoredOutputs] = {};
    swh_timing_t sum{};
    char scoring_name[40] = "";
    uint64_t symbols = 0;

    ExtractSweep(Scope *s, const TapePair &pair, int scorer_, double cutoff_, double prefix_weight_)
        : scope(s), p(pair), scorer(scorer_), cutoff(cutoff_), prefix_weight(prefix_weight_), jaro(scorer_ >= SWH_SCORER_JARO),
          f(scorer_ == SWH_SCORER_OSA ? kOsaFamily : (scorer_ >= SWH_SCORER_JARO ? kJaroFamily : kLcsFamily)),
          counts(scorer_ == SWH_SCORER_JARO_WINKLER ? 3 : (scorer_ >= SWH_SCORER_JARO ? 2 : 1)),
          whole(scored_view(pair, 0, pair.a_count, 0, pair.b_count, true)) {
        // query blocks of at most 4096 rows x candidate slices, at least 64 columns wide where the slice allows it
        const uint64_t nq = pair.a_count, nc = pair.b_count;
        const uint64_t chunk = scored_chunk_pairs("STRINGWARS_AMD_EXTRACT_CHUNK_PAIRS");
        q_step = std::min<uint64_t>(nq, std::max<uint64_t>(1, std::min<uint64_t>(4096, chunk >> 6)));
        c_step = std::max<uint64_t>(1, std::min<uint64_t>(nc, chunk / q_step));
        slice_pairs = q_step * c_step;
    }
    // first over-long strings | sizes | items | the slice's counts
    size_t need() const {
        return pad(2 * sizeof(unsigned long long)) + pad(sizeof(OsaSizes)) + pad(slice_pairs * sizeof(LaneItem)) + counts * pad(slice_pairs * 8);
    }
    void take(Carver &sc) {
        first_over = sc.take<unsigned long long>(2);
        sizes = sc.take<OsaSizes>(1);
        items = sc.take<LaneItem>(slice_pairs);
        for (int o = 0; o < counts; ++o) slice[o] = sc.take<uint64_t>(slice_pairs);
    }
    // the kernels since the last absorb() go into the sum (`scoring`: the family's kernel)
    void absorb(bool scoring) {
        if (scope->profiling && scope->stamps_used) {
            SWH_HIP_CHECK(hipStreamSynchronize(scope->stream));
            collect_timing(scope);
            const swh_timing_t &t = scope->last_timing;
            sum.total_ms += t.total_ms; sum.compute_ms += t.compute_ms; sum.kernels += t.kernels;
            if (scoring) { sum.dominant_ms += t.dominant_ms; snprintf(scoring_name, sizeof scoring_name, "%s", t.dominant_name); }
        }
        scope->stamps_used = 0;
    }
    // The length limits: OSA and LCS refuse a pair whose SHORTER string is over theirs, Jaro one with either string over its own.
    // Both follow from the two tapes' own lengths, so one pass over their offsets refuses the call before anything is scored or written.
    swh_status_t lengths(const char **error) {
        hipStream_t stream = scope->stream;
        SWH_HIP_CHECK(hipMemsetAsync(first_over, 0xFF, 2 * sizeof(unsigned long long), stream));
        const uint32_t limit = jaro ? SWH_JARO_MAX_LENGTH : SWH_OSA_MAX_SHORTER;
        launch_extract_first_over(scope, whole.a, whole.a_off64, limit, first_over);
        launch_extract_first_over(scope, whole.b, whole.b_off64, limit, first_over + 1);
        unsigned long long over[2];
        SWH_HIP_CHECK(hipMemcpyAsync(over, first_over, sizeof over, hipMemcpyDeviceToHost, stream));
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        absorb(false);
        const bool a_over = over[0] != ~0ull, b_over = over[1] != ~0ull;
        if (jaro ? (a_over || b_over) : (a_over && b_over))
            return scored_oversize(f, whole, a_over ? (size_t)over[0] : 0, b_over ? (size_t)over[1] : 0, true, stream, error);
        return swh_success_k;
    }
    // One walk over the blocks and slices. rows_begin(rows) opens every block of queries; each slice is measured, cut into items and
    // scored into the count arrays, and each(slice, last_slice) launches the search's own kernel on it.
    // `counted`: the walk's cells and symbols go into the sums (a second walk of the same pairs: not again).
    template <typename Rows, typename Each> swh_status_t walk(bool counted, const char **error, Rows rows_begin, Each each) {
        const uint64_t nq = p.a_count, nc = p.b_count;
        // a finite cutoff of the OSA scorer is the scoring kernel's bound: what it clamps is over the cutoff anyway (the LCS kernel
        // runs unbounded: every scorer of its family reads the LCS length)
        const uint32_t bound = scorer == SWH_SCORER_OSA && cutoff < 4294967294.0 ? (uint32_t)cutoff : SWH_UNBOUNDED;
        ExtractSlice x{};
        for (int o = 0; o < counts; ++o) x.counts[o] = slice[o];
        x.a = whole.a; x.b = whole.b; x.a_off64 = whole.a_off64; x.b_off64 = whole.b_off64;
        x.scorer = scorer; x.prefix_weight = prefix_weight;
        memcpy(&x.cutoff_bits, &cutoff, sizeof x.cutoff_bits);
        for (uint64_t q0 = 0; q0 < nq; q0 += q_step) {
            const uint64_t rows = std::min<uint64_t>(q_step, nq - q0);
            rows_begin(rows);
            for (uint64_t c0 = 0; c0 < nc; c0 += c_step) {
                const uint64_t columns = std::min<uint64_t>(c_step, nc - c0);
                OsaTapes t = scored_view(p, q0, rows, c0, columns, true);
                const OsaSizes got = scored_measure(scope, f, t, 0, rows * columns, sizes, items);
                absorb(false);
                if (got.first_oversize != ~0ull)   // (the memory of a prepared tape changed since the lengths were read)
                    return fail(error, swh_unsupported_length_k, "a string of the slice at (%llu, %llu) grew over the limit: %s",
                                (unsigned long long)q0, (unsigned long long)c0, f.oversize);
                if (counted) { sum.cells += got.cells; symbols += got.symbols; }
                char *where[kScoredOutputs] = {};
                if (jaro) for (int o = 0; o < counts; ++o) where[o] = (char *)slice[o];
                else where[scorer == SWH_SCORER_OSA ? 0 : 1] = (char *)slice[0];   // the OSA distance; the LCS length
                f.launch(scope, t, items, got.items, where, columns * 8, bound, scored_wide(t, got));
                absorb(true);
                x.rows = rows; x.columns = columns; x.row_first = q0; x.col_first = c0;
                each(x, c0 + columns == nc);
                absorb(false);
            }
        }
        return swh_success_k;
    }
    // the search as one call, "<search>/<scoring kernel>", once in the scope's totals; `out_bytes`: what it wrote for the caller
    void close(const char *search, uint64_t out_bytes) {
        scope->summary_pending = false;
        scope->stamps_pending = false;
        sum.bytes = (whole.cp ? 4 : 1) * symbols + out_bytes;
        snprintf(sum.dominant_name, sizeof sum.dominant_name, "%s/%s", search, scoring_name);
        scope->last_timing = sum;
        if (scope->profiling) add_to_totals(scope->totals, sum);
    }
};
}  // extern "C++"

static swh_status_t extract_run(Scope *scope, const TapePair &p, const ExtractRequest &r, const char **error) {
    return synchronous_run(scope, error, [&]() -> swh_status_t {
        const uint64_t nq = p.a_count, nc = p.b_count, k = r.k;
        if (nq == 0) return swh_success_k;
        const size_t index_bytes = nq * k * sizeof(uint32_t), score_bytes = nq * k * sizeof(uint64_t);
        SWH_HIP_CHECK(hipSetDevice(scope->device));
        hipStream_t stream = scope->stream;
        Staged<uint32_t> ind(r.indices); Staged<uint64_t> sco((uint64_t *)r.scores);
        if (nc == 0) {   // every row is padding
            ind.fill_padding(stream, nq * k); sco.fill_padding(stream, nq * k);
            SWH_HIP_CHECK(hipStreamSynchronize(stream));
            return swh_success_k;
        }
        ExtractSweep sweep(scope, p, r.scorer, r.cutoff, r.prefix_weight);

        // the sweep's part | the block's lists | rows bound for the host
        const size_t need = sweep.need() + pad(sweep.q_step * k * 16) + ind.need(nq * k) + sco.need(nq * k);
        Carver sc = carve(scope->topk_scratch, scope->topk_scratch_bytes, need);
        sweep.take(sc);
        char *lists = sc.take<char>(sweep.q_step * k * 16);
        ind.place(sc, nq * k); sco.place(sc, nq * k);

        swh_status_t status = sweep.lengths(error);
        if (status != swh_success_k) return status;
        status = sweep.walk(true, error,
            [&](uint64_t rows) { SWH_HIP_CHECK(hipMemsetAsync(lists, 0xFF, rows * k * 16, stream)); },   // every row is padding
            [&](const ExtractSlice &slice, bool last_slice) {
                ExtractLaunch x{};
                static_cast<ExtractSlice &>(x) = slice;
                x.k = r.k; x.emit = last_slice ? 1u : 0u;
                x.lists = lists; x.indices = ind.dev; x.scores = sco.dev;
                launch_extract_select(scope, x);
            });
        if (status != swh_success_k) return status;
        ind.copy_back(stream, nq * k); sco.copy_back(stream, nq * k);
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        sweep.close("extract_select", index_bytes + score_bytes);
        return swh_success_k;
    });
}

// the checks both score searches make, in extract's order: the handles, the engine's kind and the scorer ...
static swh_status_t extract_scorer_checks(swh_levenshtein_t e, swh_scope_t s, int scorer, const char **error) {
    const swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    if (((const Engine *)e)->kind != 0) return fail(error, swh_invalid_argument_k, "not a Levenshtein engine");
    if (scorer < SWH_SCORER_OSA || scorer > SWH_SCORER_JARO_WINKLER) return fail(error, swh_invalid_argument_k, "scorer must be one of SWH_SCORER_*");
    return swh_success_k;
}
// ... and the cutoff (which comes back with -0.0 made +0.0), the prefix weight, the costs and the number of candidates
static swh_status_t extract_value_checks(swh_levenshtein_t e, int scorer, uint64_t cutoff_bits, uint64_t prefix_weight_bits, size_t candidates,
                                         double &cutoff, double &prefix_weight, const char **error) {
    memcpy(&cutoff, &cutoff_bits, sizeof cutoff);
    memcpy(&prefix_weight, &prefix_weight_bits, sizeof prefix_weight);
    if (!(cutoff >= 0.0)) return fail(error, swh_invalid_argument_k, "the cutoff must be a non-negative number (or +infinity), not NaN");
    if (scorer == SWH_SCORER_JARO_WINKLER && !(prefix_weight >= 0.0 && prefix_weight <= 0.25))
        return fail(error, swh_invalid_argument_k, "the prefix weight must lie in [0, 0.25]");
    if (!((const Engine *)e)->unit_costs)
        return fail(error, swh_not_implemented_k, "the score search is called on a unit-cost engine (match 0, mismatch 1, open 1, extend 1)");
    if (candidates >= 0xFFFFFFFFull) return fail(error, swh_unsupported_length_k, "2^32 - 1 candidates or more");
    if (cutoff == 0.0) cutoff = 0.0;   // (-0.0: +0.0)
    return swh_success_k;
}

static swh_status_t extract_checks(swh_levenshtein_t e, swh_scope_t s, int scorer, size_t k, uint64_t cutoff_bits, uint64_t prefix_weight_bits,
                                   size_t queries, size_t candidates, const uint32_t *indices, const void *scores, ExtractRequest &request,
                                   const char **error) {
    swh_status_t status = extract_scorer_checks(e, s, scorer, error);
    if (status != swh_success_k) return status;
    if (k < 1 || k > SWH_TOPK_MAX) return fail(error, swh_invalid_argument_k, "k must lie in [1, SWH_TOPK_MAX]");
    double cutoff, prefix_weight;
    if ((status = extract_value_checks(e, scorer, cutoff_bits, prefix_weight_bits, candidates, cutoff, prefix_weight, error)) != swh_success_k) return status;
    if (queries && (!indices || !scores)) return fail(error, swh_invalid_argument_k, "null output pointer");
    request = ExtractRequest{scorer, (uint32_t)k, cutoff, prefix_weight, (uint32_t *)indices, (void *)scores};
    return swh_success_k;
}

static swh_status_t extract_tapes(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *q, const swh_tape_u64_t *c, bool utf8, int scorer,
                                  size_t k, uint64_t cutoff_bits, uint64_t prefix_weight_bits, uint32_t *indices, void *scores, const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    if (!q) return fail(error, swh_invalid_argument_k, "null tape");
    ExtractRequest request{};
    status = extract_checks(e, s, scorer, k, cutoff_bits, prefix_weight_bits, q->count, (c ? c : q)->count, indices, scores, request, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.begin(s, error)) != swh_success_k) return status;
    if (q->count == 0) return swh_success_k;
    if ((status = call.prepare(q, c, utf8, true, true, error)) != swh_success_k) return status;
    return extract_run(call.scope, call.pair, request, error);
}
swh_status_t swh_levenshtein_extract_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *queries, const swh_tape_u64_t *candidates,
                                             int scorer, size_t k, uint64_t cutoff_bits, uint64_t prefix_weight_bits, uint32_t *indices,
                                             void *scores, const char **error) {
    return extract_tapes(e, s, queries, candidates, false, scorer, k, cutoff_bits, prefix_weight_bits, indices, scores, error);
}
swh_status_t swh_levenshtein_utf8_extract_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *queries,
                                                  const swh_tape_u64_t *candidates, int scorer, size_t k, uint64_t cutoff_bits,
                                                  uint64_t prefix_weight_bits, uint32_t *indices, void *scores, const char **error) {
    return extract_tapes(e, s, queries, candidates, true, scorer, k, cutoff_bits, prefix_weight_bits, indices, scores, error);
}
swh_status_t swh_levenshtein_extract_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *queries,
                                              const swh_prepared_view_t *candidates, int scorer, size_t k, uint64_t cutoff_bits,
                                              uint64_t prefix_weight_bits, uint32_t *indices, void *scores, const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.views(queries, candidates, true, error)) != swh_success_k) return status;
    ExtractRequest request{};
    status = extract_checks(e, s, scorer, k, cutoff_bits, prefix_weight_bits, call.pair.a_count, call.pair.b_count, indices, scores, request, error);
    if (status != swh_success_k) return status;
    if ((status = call.begin_on_views(s, error)) != swh_success_k) return status;
    return extract_run(call.scope, call.pair, request, error);
}

// ---- score range search (extract_within.hip): every candidate whose score passes the cutoff, as CSR ---------------------------------------
// extract_run's sweep with within_run's protocol. Both walks score the pairs -- as the range search's general path does: nothing is
// kept between them but a count per query (4 bytes) that the scan turns into a cursor (8) and the row offsets. The count walk adds
// every slice's hits to the counts, the host reads the total (8 bytes), and only if the caller's arrays hold it the fill walk stores
// the hits at the cursors. The scratch is the sweep's, the counts and cursors, the scan's block sums and staging for host outputs
// (the hits' in scope->within_out, sized once the total is known): nothing grows with queries x candidates.
struct ExtractWithinRequest {
    int scorer;
    double cutoff, prefix_weight;
    size_t *row_offsets;
    uint32_t *indices;
    void *scores;
    size_t capacity;
};

static swh_status_t extract_within_run(Scope *scope, const TapePair &p, const ExtractWithinRequest &r, const char **error) {
    return synchronous_run(scope, error, [&]() -> swh_status_t {
        const uint64_t nq = p.a_count, nc = p.b_count;
        SWH_HIP_CHECK(hipSetDevice(scope->device));
        hipStream_t stream = scope->stream;
        CsrRows csr(r.row_offsets, nq, r.capacity);
        Staged<uint32_t> ind(r.indices); Staged<uint64_t> sco((uint64_t *)r.scores);   // (both null in a counting call: nothing is staged, nothing filled)
        if (nq == 0 || nc == 0) {
            csr.fill_empty(stream);
            return swh_success_k;
        }
        ExtractSweep sweep(scope, p, r.scorer, r.cutoff, r.prefix_weight);
        // the sweep's part | the rows' counts, cursors, scan scratch and offsets bound for the host
        Carver sc = carve(scope->topk_scratch, scope->topk_scratch_bytes, sweep.need() + csr.need());
        sweep.take(sc);
        csr.place(sc);

        swh_status_t status = sweep.lengths(error);
        if (status != swh_success_k) return status;
        ExtractWithinLaunch x{};
        x.hits = csr.counts; x.cursors = csr.cursors;
        auto no_rows_begin = [](uint64_t) {};   // (counts and cursors span all queries: nothing to open per block)
        auto launch = [&](bool fill) {
            return [&x, scope, fill](const ExtractSlice &slice, bool) {
                static_cast<ExtractSlice &>(x) = slice;
                launch_extract_within(scope, x, fill);
            };
        };
        SWH_HIP_CHECK(hipMemsetAsync(csr.counts, 0, nq * 4, stream));
        if ((status = sweep.walk(true, error, no_rows_begin, launch(false))) != swh_success_k) return status;
        csr.scan_counts(scope);
        sweep.absorb(false);
        const bool filled = csr.publish(stream);
        if (filled) {
            carve_hits(scope, csr.total, 0, ind, sco);
            x.indices = ind.dev; x.scores = sco.dev; x.total = csr.total;
            if ((status = sweep.walk(false, error, no_rows_begin, launch(true))) != swh_success_k) return status;
            ind.copy_back(stream, csr.total); sco.copy_back(stream, csr.total);
        }
        SWH_HIP_CHECK(hipStreamSynchronize(stream));
        sweep.close("extract_within", (nq + 1) * 8 + (filled ? csr.total * 12 : 0));
        return swh_success_k;
    });
}

static swh_status_t extract_within_checks(swh_levenshtein_t e, swh_scope_t s, int scorer, uint64_t cutoff_bits, uint64_t prefix_weight_bits,
                                          size_t candidates, size_t *row_offsets, uint32_t *indices, void *scores, size_t capacity,
                                          ExtractWithinRequest &request, const char **error) {
    swh_status_t status = extract_scorer_checks(e, s, scorer, error);
    if (status != swh_success_k) return status;
    double cutoff, prefix_weight;
    if ((status = extract_value_checks(e, scorer, cutoff_bits, prefix_weight_bits, candidates, cutoff, prefix_weight, error)) != swh_success_k) return status;
    if (scorer < SWH_SCORER_LCS && std::isinf(cutoff))
        return fail(error, swh_invalid_argument_k, "a range search by a distance needs a finite cutoff: without one it is the dense cross-product");
    if ((status = csr_output_checks(row_offsets, indices, scores, "indices and scores", false, capacity, error)) != swh_success_k) return status;
    request = ExtractWithinRequest{scorer, cutoff, prefix_weight, row_offsets, indices, scores, capacity};
    return swh_success_k;
}

static swh_status_t extract_within_tapes(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *q, const swh_tape_u64_t *c, bool utf8, int scorer,
                                         uint64_t cutoff_bits, uint64_t prefix_weight_bits, size_t *row_offsets, uint32_t *indices, void *scores,
                                         size_t capacity, const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    if (!q) return fail(error, swh_invalid_argument_k, "null tape");
    const size_t candidates = (c ? c : q)->count;
    ExtractWithinRequest request{};
    status = extract_within_checks(e, s, scorer, cutoff_bits, prefix_weight_bits, candidates, row_offsets, indices, scores, capacity, request, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.begin(s, error)) != swh_success_k) return status;
    // (a search without queries prepares nothing, one without candidates the queries alone: the offsets are still written)
    if ((status = call.prepare(q, c, utf8, q->count != 0, q->count && candidates, error)) != swh_success_k) return status;
    return extract_within_run(call.scope, call.pair, request, error);
}
swh_status_t swh_levenshtein_extract_within_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *queries,
                                                    const swh_tape_u64_t *candidates, int scorer, uint64_t cutoff_bits, uint64_t prefix_weight_bits,
                                                    size_t *row_offsets, uint32_t *indices, void *scores, size_t capacity, const char **error) {
    return extract_within_tapes(e, s, queries, candidates, false, scorer, cutoff_bits, prefix_weight_bits, row_offsets, indices, scores, capacity, error);
}
swh_status_t swh_levenshtein_utf8_extract_within_u64tape(swh_levenshtein_t e, swh_scope_t s, const swh_tape_u64_t *queries,
                                                         const swh_tape_u64_t *candidates, int scorer, uint64_t cutoff_bits,
                                                         uint64_t prefix_weight_bits, size_t *row_offsets, uint32_t *indices, void *scores,
                                                         size_t capacity, const char **error) {
    return extract_within_tapes(e, s, queries, candidates, true, scorer, cutoff_bits, prefix_weight_bits, row_offsets, indices, scores, capacity, error);
}
swh_status_t swh_levenshtein_extract_within_prepared(swh_levenshtein_t e, swh_scope_t s, const swh_prepared_view_t *queries,
                                                     const swh_prepared_view_t *candidates, int scorer, uint64_t cutoff_bits,
                                                     uint64_t prefix_weight_bits, size_t *row_offsets, uint32_t *indices, void *scores,
                                                     size_t capacity, const char **error) {
    swh_status_t status = probe_null_handles(e, s, error);
    if (status != swh_success_k) return status;
    TwoTapeCall call;
    if ((status = call.views(queries, candidates, true, error)) != swh_success_k) return status;
    ExtractWithinRequest request{};
    status = extract_within_checks(e, s, scorer, cutoff_bits, prefix_weight_bits, call.pair.b_count, row_offsets, indices, scores, capacity, request, error);
    if (status != swh_success_k) return status;
    if ((status = call.begin_on_views(s, error)) != swh_success_k) return status;
    return extract_within_run(call.scope, call.pair, request, error);
}

}  // extern "C"
