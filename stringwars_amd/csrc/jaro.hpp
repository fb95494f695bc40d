// jaro.hpp -- launchers of the Jaro / Jaro-Winkler kernels (jaro.hip), called by two_tape.hip. The pairs of a launch and the shapes of
// their measurements and work items are osa.hpp's (OsaTapes, OsaSizes, LaneItem), as they stand; the items are cut by jaro.hip's own
// k_jaro_sizes, because here the blocks follow b (never the shorter string) and both lengths are limited.
#pragma once
#include "osa.hpp"

namespace swh {

// Measures the launch's pairs into `sizes` (zeroed by the caller, first_oversize set to ~0: here the first pair with EITHER string
// over SWH_JARO_MAX_LENGTH symbols) and, unless `items` is null, cuts them into items (`items`: room for `count`) whose `blocks` is
// the largest number of 32-row blocks of a b among the item's pairs.
void launch_jaro_sizes(Scope *scope, const OsaTapes &t, OsaSizes *sizes, LaneItem *items);

// Counts the items' pairs: M matches, t = h / 2 transpositions, the common prefix of at most four symbols. Each goes to its output
// -- any may be null -- at + p * stride as a u32 (pairwise), or at + (p / nb) * stride + (p % nb) * 8 as a u64 (cross: the pointers
// are where row `row0` begins, `stride` the bytes between rows).
struct JaroRun {
    const LaneItem *items;
    uint64_t item_count;
    char *matches, *transpositions, *prefix;
    uint64_t stride;
    bool wide;   // both byte tapes hold at least 16 bytes: the columns' string is read with 128-bit loads
};
void launch_jaro(Scope *scope, const OsaTapes &t, const JaroRun &r);

}  // namespace swh
