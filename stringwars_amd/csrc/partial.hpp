// partial.hpp -- launchers of the partial-ratio kernels (partial.hip), called by two_tape.hip. The pairs of a launch and their
// measurements are osa.hpp's (OsaTapes, OsaSizes); the work items are this family's own: a pair has n + m - 1 windows, and a haystack
// of megabytes must not be chained on one wave.
#pragma once
#include "osa.hpp"

namespace swh {

// The windows of one (pair, direction) are cut into items of at most partial_item_windows(m) consecutive windows: whole passes of
// floor(64 / G) windows (G the needle's 32-row blocks), as many as keep an item near kPartialItemSteps column steps of one wave.
// m = 8: 256 passes of 64 windows; m = 64: 51 of 32; m = 2048: one window.
constexpr uint32_t kPartialItemSteps = 4096;
__host__ __device__ inline uint32_t partial_item_windows(uint32_t m) {
    const uint32_t G = m ? (m + 31) >> 5 : 1u, slots = 64u / G;
    const uint32_t steps = (m + G - 1 + 15) & ~15u;   // of one pass: the super-steps of 16 columns it runs
    const uint32_t passes = kPartialItemSteps / steps;
    return (passes ? passes : 1u) * slots;
}

// `windows` consecutive windows from window `first` on of pair `pair` (of the launch); window w has the offset o = w - (m - 1).
// Bit 31 of `windows_dir` is the direction: 0 -- the needle is a, the windows lie in b; 1 -- the needle is b.
struct PartialItem {
    uint64_t pair;
    uint32_t first, windows_dir;
};
// What an item found: the best of its windows -- L > 0, the window [start, end) of the haystack -- or L = 0: no window of the item
// shares a symbol with the needle.
struct PartialRecord {
    uint32_t lcs, start, end;
};
// The scratch of a launch of `pairs` pairs that `items` items were counted for, as partial_scratch_bytes lays it out:
// where each pair's items begin (u64) | the items | their records. Every part starts on a multiple of 256 bytes.
inline size_t partial_pad(size_t n) { return (n + 255) & ~(size_t)255; }
inline size_t partial_scratch_bytes(uint64_t pairs, uint64_t items) {
    return partial_pad(pairs * 8) + partial_pad(items * sizeof(PartialItem)) + partial_pad(items * sizeof(PartialRecord));
}

// Measures the launch's pairs into `sizes` as launch_osa_sizes does (zeroed by the caller, first_oversize set to ~0; the limit is
// SWH_PARTIAL_MAX_NEEDLE on the shorter string) and counts their items into sizes->items. With `scratch` (laid out as above for
// `capacity` items, what a counting launch found) it also places every pair's items.
void launch_partial_sizes(Scope *scope, const OsaTapes &t, OsaSizes *sizes, void *scratch, uint64_t capacity);

// Scores the `item_count` items of `scratch` into their records. `wide`: both byte tapes hold at least 16 bytes, the windows are read
// with 128-bit loads.
void launch_partial_items(Scope *scope, const OsaTapes &t, void *scratch, uint64_t item_count, bool wide);

// Merges every pair's records into the four outputs -- any may be null -- at + p * stride as a u32 (pairwise), or at
// + (p / nb) * stride + (p % nb) * 8 as a u64 (cross: the pointers are where row `row0` begins). May run again on the same records
// with other outputs.
struct PartialMerge {
    const void *scratch;
    char *lcs, *starts, *ends, *sides;
    uint64_t stride;
};
void launch_partial_merge(Scope *scope, const OsaTapes &t, const PartialMerge &r, uint64_t item_count);

}  // namespace swh
