// within.hpp -- launchers of the Levenshtein range search (within.hip), called from two_tape.hip.
#pragma once
#include "common.hpp"

namespace swh {

// The fused word-sized search: one walk of k_cross_within. `fill` false: the count pass -- counts[row][slice] and the call's summary;
// `fill` true: the same walk stores every hit at starts[row][slice] onwards (positions at or beyond `total` are never written).
struct WithinLaunch {
    TapeRef a, b;                     // queries, candidates: device byte tapes with `off64`-wide offsets
    uint32_t off64, slices, bound, prune;
    uint64_t slice_chunks;            // chunks of 64 candidates per slice
    uint32_t *counts;                 // [query][slice]
    const uint64_t *starts;           // [query][slice]: the offsets scan (scan.hpp) of counts
    uint64_t total;                   // hits of the call = entries of indices / distances that may be written
    uint32_t *indices, *distances;
};
void launch_cross_within(Scope *scope, const WithinLaunch &w, bool fill);
// The general path's two sweeps over a slice of a dense u32 matrix (`columns` wide, row r = query row_first + r, column c = candidate
// col_first + c): hits (score <= bound) added to counts[row_first + r], or stored at cursors[row_first + r] onwards, which advances.
void launch_within_count(Scope *scope, const uint32_t *scores, uint64_t rows, uint64_t columns, uint32_t bound, uint32_t *counts);
void launch_within_fill(Scope *scope, const uint32_t *scores, uint64_t rows, uint64_t columns, uint64_t col_first, uint32_t bound,
                        uint64_t *cursors, uint64_t total, uint32_t *indices, uint32_t *distances);

}  // namespace swh
