// lcs.hpp -- launcher of the longest-common-subsequence / Indel kernel (lcs.hip), called by two_tape.hip. The pairs of a launch, their
// measurements and their work items are osa.hpp's (OsaTapes, OsaSizes, LaneItem, launch_osa_sizes), as they stand.
#pragma once
#include "osa.hpp"

namespace swh {

// Scores the items' pairs. With L the LCS length of pair p (m and n the two lengths), L goes to `lcs` and min(m + n - 2 L, bound + 1)
// to `indel` -- either may be null -- at + p * stride as a u32 (pairwise), or at + (p / nb) * stride + (p % nb) * 8 as a u64
// (cross: the pointers are where row `row0` begins, `stride` the bytes between rows).
struct LcsRun {
    const LaneItem *items;
    uint64_t item_count;
    char *indel, *lcs;
    uint64_t stride;
    uint32_t bound;
    bool wide;   // both byte tapes hold at least 16 bytes: the columns' string is read with 128-bit loads
};
void launch_lcs(Scope *scope, const OsaTapes &t, const LcsRun &r);

}  // namespace swh
