// osa.hpp -- launchers of the optimal-string-alignment (restricted Damerau-Levenshtein) kernels (osa.hip), called by two_tape.hip.
// Kept apart from common.hpp, which every kernel family's profile stamp hashes (tools/kernel_sources.py).
#pragma once
#include "common.hpp"

namespace swh {

// One launch's pairs on prepared (device-resident, measured, decoded) tapes. Symbols are bytes (`cp` = 0, each tape's offsets u32
// or u64 by its `off64`) or code points (`cp` = 1: u32 symbols, u64 offsets). Pair p of the launch, 0 <= p < count, is
//  - pairwise (`nb` = 0): a[p] against b[p];
//  - a slice of whole rows of a cross-product (`nb` = strings of b): a[row0 + p / nb] against b[p % nb].
struct OsaTapes {
    TapeRef a, b;
    uint32_t a_off64, b_off64, cp;
    uint64_t count, nb, row0;
};

// What k_osa_sizes measures over a launch's pairs, read back by the host before anything is written.
struct OsaSizes {
    unsigned long long cells;            // sum len(a) * len(b)
    unsigned long long symbols;          // sum len(a) + len(b)
    unsigned long long first_oversize;   // the first pair whose SHORTER string has more than SWH_OSA_MAX_SHORTER symbols, or ~0
    unsigned long long items;            // work items written to the item list
    unsigned long long a_total, b_total; // symbols the two tapes (the views of them the call sees) hold
};

// A work item of every lane-per-block family (bp_lanes.hpp): `pairs` consecutive pairs from `first` on, `blocks` lanes (32-row blocks of
// the rows' string) each; pairs * blocks <= 64.
struct LaneItem {
    uint64_t first;
    uint32_t pairs, blocks;
};

// Measures the launch's pairs into `sizes` (zeroed by the caller, first_oversize set to ~0) and, unless `items` is null, cuts them
// into items (`items`: room for `count`).
void launch_osa_sizes(Scope *scope, const OsaTapes &t, OsaSizes *sizes, LaneItem *items);

// Scores the items' pairs: min(d, bound + 1) of pair p goes to `out` + p * stride as a u32 (pairwise), or to
// `out` + (p / nb) * stride + (p % nb) * 8 as a u64 (cross: `out` is where row `row0` begins, `stride` the bytes between rows).
struct OsaRun {
    const LaneItem *items;
    uint64_t item_count;
    char *out;
    uint64_t stride;
    uint32_t bound;
    bool wide;   // both byte tapes hold at least 16 bytes: the columns' string is read with 128-bit loads
};
void launch_osa(Scope *scope, const OsaTapes &t, const OsaRun &r);

}  // namespace swh
