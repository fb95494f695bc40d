// scan.hpp -- the library's one offsets scan (scan.hip): counts into exclusive prefix sums, row offsets and a total. Every call whose
// rows have unknown lengths goes through it: the range searches, infix_all, the token tapes and the alignments.
#pragma once
#include "api.hpp"   // Carver, pad

namespace swh {

constexpr uint64_t kScanTile = 4096;   // values per workgroup

// The scratch a scan of n values needs beside them: a sum per tile.
struct ScanScratch {
    uint64_t *block_sums = nullptr;
    static uint64_t tiles(uint64_t n) { return (n + kScanTile - 1) / kScanTile; }
    static size_t need(uint64_t n) { return pad(tiles(n) * 8); }
    void place(Carver &sc, uint64_t n) { block_sums = sc.take<uint64_t>(tiles(n)); }
};

// Exclusive scan of counts[0, n), n = rows * slices, row-major: starts[i] for every count (`starts` may be null: nobody wants a copy),
// row_offsets[r] = the start of count r * slices, row_offsets[rows] = the total. Two launches, "offsets_sums" and "offsets_scan".
// In place is legal with In = uint64_t and slices == 1: row_offsets == (uint64_t *)counts, rows + 1 words. A thread loads all of its
// counts before it stores any, threads own disjoint elements, and a tile sees the others only through block_sums, which the first
// launch completes -- so none of these pointers is __restrict__. No rows: row_offsets[0] = 0, nothing is launched.
template <typename In>
void launch_offsets_scan(Scope *scope, const In *counts, uint64_t rows, uint32_t slices, const ScanScratch &scratch, uint64_t *starts,
                         uint64_t *row_offsets);

}  // namespace swh
