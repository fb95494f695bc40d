// within.hip -- Levenshtein range search: for every query EVERY candidate with d <= bound, as CSR rows of unknown length
// (swh_levenshtein_within_*, include/stringwars_amd.h). Top-k (topk.hip) folds a walk's distances into a list of k; a range search
// compacts them: rows in candidate order, no sort, no atomics on the output, the same bits on every run.
//
// Every path walks the pairs twice. The count pass leaves hit counts, the offsets scan (scan.hip) turns them into starts and row
// offsets, the host reads the total (8 bytes) and -- only if the caller's arrays hold it -- the fill pass repeats the walk and stores
// each hit at its row's cursor: a wave's 64 distances give one ballot, a hit's place is the cursor plus the hits in the lanes below it.
//
// Kernels:
//   k_cross_within<Off, Fill>  word-sized byte strings (<= 32 bytes, unit costs: the calls top-k serves with k_cross_topk), on the same item
//                              (cross_words.hpp). A chunk with no lane at |m - n| <= bound is skipped in both passes (d >= |m - n|).
//                              Lane q keeps query q's count (Fill = false) or cursor (true).
//   k_within_count,            the general path: one wave per row of a slice of a dense u32 matrix (scored by the ordinary
//   k_within_fill              cross-product routes into scratch). Slices run in stream order, so a row's cursor meets its candidates
//                              in ascending order.
#include "within.hpp"
#include "cross_words.hpp"

#include <algorithm>

namespace swh {

constexpr int kWithinWaves = kWordWaves;   // (also the general path's sweeps: one wave per row)

struct WithinArgs {
    WordSearchArgs search;     // prune: skip a query's chunk when no lane has |m - n| <= bound
    uint32_t bound;            // hits have d <= bound
    uint32_t *counts;          // Fill = false: [query][slice], out
    const uint64_t *starts;    // Fill = true: [query][slice], where the item's hits of that query begin
    uint64_t total;            // Fill = true: entries the outputs hold
    uint32_t *indices, *distances;
};

template <typename Off, bool Fill>
__global__ __launch_bounds__(kWithinWaves * 64, 4) void k_cross_within(WithinArgs args) {
    __shared__ WordSearchLds lds;
    const uint32_t lane = threadIdx.x & 63, bound = args.bound, slices = args.search.slices;
    const uint64_t lanes_below = (1ull << lane) - 1ull;
    // lane q: query q's hits so far in this item (count pass), or where its next hit goes (fill pass)
    uint32_t running = 0;
    uint64_t cursor = 0;
    // (the count pass sums the call's cells and lengths: they are counted once)
    word_search_items<Off, !Fill>(args.search, lds,
        [&](const WordItem &item) {
            running = 0;
            if constexpr (Fill) cursor = lane < item.q_count ? args.starts[(item.q_first + (uint64_t)lane) * slices + item.slice] : 0;
        },
        [&](uint32_t, uint32_t gap) { return gap <= bound; },   // (the bound is fixed: the test never loosens the way top-k's does)
        [&](uint32_t q, const WordCandidate &c, uint32_t d) {
            const bool hit = c.fits && d <= bound;
            const uint64_t hits = __ballot(hit);
            if (!hits) return;
            const uint32_t fresh = (uint32_t)__popcll(hits);
            if constexpr (Fill) {
                const uint64_t at = readlane64(cursor, (int)q) + (uint64_t)__popcll(hits & lanes_below);
                if (hit && at < args.total) {   // (a total the walk outgrows: the tapes changed between the passes -- never past the arrays)
                    args.indices[at] = (uint32_t)c.cand;
                    args.distances[at] = d;
                }
                if (lane == q) cursor += fresh;
            } else {
                if (lane == q) running += fresh;
            }
        },
        [&](const WordItem &item) {
            if constexpr (!Fill) {
                if (lane < item.q_count) args.counts[(item.q_first + (uint64_t)lane) * slices + item.slice] = running;
            }
            lds_order();   // the next item's tables are not cleared under this item's last reads
        });
}

// ---- the general path's sweeps -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWithinWaves * 64) void k_within_count(const uint32_t *scores, uint64_t rows, uint64_t columns, uint32_t bound,
                                                                     uint32_t *counts) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t r = (uint64_t)blockIdx.x * kWithinWaves + wave; r < rows; r += (uint64_t)gridDim.x * kWithinWaves) {
        const uint32_t *row = scores + r * columns;
        uint32_t hits = 0;
        for (uint64_t c0 = 0; c0 < columns; c0 += 64) {
            const uint64_t c = c0 + lane;
            hits += (uint32_t)__popcll(__ballot(c < columns && row[c] <= bound));
        }
        if (lane == 0) counts[r] += hits;   // (one wave per row, slices in stream order: no other writer)
    }
}

__global__ __launch_bounds__(kWithinWaves * 64) void k_within_fill(const uint32_t *scores, uint64_t rows, uint64_t columns, uint64_t col_first,
                                                                    uint32_t bound, uint64_t *cursors, uint64_t total, uint32_t *indices,
                                                                    uint32_t *distances) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t lanes_below = (1ull << lane) - 1ull;
    for (uint64_t r = (uint64_t)blockIdx.x * kWithinWaves + wave; r < rows; r += (uint64_t)gridDim.x * kWithinWaves) {
        const uint32_t *row = scores + r * columns;
        uint64_t cursor = cursors[r];
        for (uint64_t c0 = 0; c0 < columns; c0 += 64) {
            const uint64_t c = c0 + lane;
            const uint32_t score = c < columns ? row[c] : 0u;
            const bool hit = c < columns && score <= bound;
            const uint64_t hits = __ballot(hit);
            const uint64_t at = cursor + (uint64_t)__popcll(hits & lanes_below);
            if (hit && at < total) {
                indices[at] = (uint32_t)(col_first + c);
                distances[at] = score;
            }
            cursor += (uint64_t)__popcll(hits);
        }
        if (lane == 0) cursors[r] = cursor;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
void launch_cross_within(Scope *scope, const WithinLaunch &w, bool fill) {
    WithinArgs args{};
    args.search = {w.a, w.b, w.slices, w.prune, w.slice_chunks, scope->plan_partials, scope->done_counter, scope->summary_target()};
    args.bound = w.bound; args.counts = w.counts; args.starts = w.starts; args.total = w.total; args.indices = w.indices; args.distances = w.distances;
    StampGuard guard(scope, "cross_within");
    const dim3 grid(word_item_blocks(scope, ((w.a.count + kWordQueries - 1) / kWordQueries) * w.slices)), block(kWithinWaves * 64);
    if (w.off64) {
        if (fill) hipLaunchKernelGGL((k_cross_within<uint64_t, true>), grid, block, 0, scope->stream, args);
        else hipLaunchKernelGGL((k_cross_within<uint64_t, false>), grid, block, 0, scope->stream, args);
    } else {
        if (fill) hipLaunchKernelGGL((k_cross_within<uint32_t, true>), grid, block, 0, scope->stream, args);
        else hipLaunchKernelGGL((k_cross_within<uint32_t, false>), grid, block, 0, scope->stream, args);
    }
    SWH_HIP_CHECK(hipGetLastError());
}

static uint32_t within_row_blocks(const Scope *scope, uint64_t rows) {
    const uint64_t blocks = std::min<uint64_t>((rows + kWithinWaves - 1) / kWithinWaves, (uint64_t)scope->compute_units * 16);
    return (uint32_t)(blocks ? blocks : 1);
}

void launch_within_count(Scope *scope, const uint32_t *scores, uint64_t rows, uint64_t columns, uint32_t bound, uint32_t *counts) {
    StampGuard guard(scope, "within_count");
    hipLaunchKernelGGL(k_within_count, dim3(within_row_blocks(scope, rows)), dim3(kWithinWaves * 64), 0, scope->stream, scores, rows, columns, bound,
                       counts);
    SWH_HIP_CHECK(hipGetLastError());
}

void launch_within_fill(Scope *scope, const uint32_t *scores, uint64_t rows, uint64_t columns, uint64_t col_first, uint32_t bound,
                        uint64_t *cursors, uint64_t total, uint32_t *indices, uint32_t *distances) {
    StampGuard guard(scope, "within_fill");
    hipLaunchKernelGGL(k_within_fill, dim3(within_row_blocks(scope, rows)), dim3(kWithinWaves * 64), 0, scope->stream, scores, rows, columns,
                       col_first, bound, cursors, total, indices, distances);
    SWH_HIP_CHECK(hipGetLastError());
}

}  // namespace swh
