// infix.hpp -- launchers of the Levenshtein infix-search kernels (infix.hip), called by two_tape.hip.
// Kept apart from common.hpp, which every kernel family's profile stamp hashes (tools/kernel_sources.py).
#pragma once
#include "osa.hpp"   // LaneItem: the work items of the two passes

namespace swh {

// One pairwise batch on prepared (device-resident, measured, decoded) tapes: pattern i is searched in text i. Symbols are bytes
// (`cp` = 0, each tape's offsets u32 or u64 by its `off64`) or code points (`cp` = 1: u32 symbols, u64 offsets).
struct InfixTapes {
    TapeRef patterns, texts;
    uint32_t p_off64, t_off64, cp;
    uint64_t count;
};

// What k_infix_sizes measures over the whole batch, read back by the host before anything is written.
struct InfixSizes {
    unsigned long long cells;            // sum m_i * n_i
    unsigned long long symbols;          // sum m_i + n_i
    unsigned long long first_oversize;   // the first pair whose pattern has more than SWH_INFIX_MAX_PATTERN symbols, or ~0
    unsigned long long items;            // work items written to the item list
    unsigned long long text_symbols;     // symbols the text tape (the view of it the call sees) holds
};

// Measures the batch into `sizes` (zeroed by the caller, first_oversize set to ~0) and cuts it into items (`items`: room for `count`).
void launch_infix_sizes(Scope *scope, const InfixTapes &t, InfixSizes *sizes, LaneItem *items);

// The forward pass writes every pair's distance and end (unclamped) to `distances` / `ends`; the start pass reads them, finds the
// starts of the pairs within the bound and writes all three arrays in their final form (the bound applied).
struct InfixRun {
    const LaneItem *items;
    uint64_t item_count;
    uint32_t *distances, *starts, *ends;
    uint32_t bound;
    bool wide_text;   // the text tape holds at least 16 bytes: the forward pass reads it with 128-bit loads
};
void launch_infix_forward(Scope *scope, const InfixTapes &t, const InfixRun &r);
void launch_infix_starts(Scope *scope, const InfixTapes &t, const InfixRun &r);

// ---- every occurrence within a bound (swh_levenshtein_infix_all_*) ----
// A hit of pair p is an end e, 0 <= e <= n, whose bottom-row score D(e) is within `bound` and passes `select` (SWH_INFIX_SELECT_*).
// The forward walk runs twice over the pairs' items: the count walk leaves counts[p] (and, for SELECT_BEST, best[p] = the pair's
// smallest score, or ~0 if that is over the bound); the fill walk stores (end, distance) of pair p's hits at cursors[p] onwards, in
// column order, and never at or beyond `total`.
struct InfixHitsRun {
    const LaneItem *items;
    uint64_t item_count;
    uint32_t bound, select;
    uint32_t *counts, *best;    // [pair]
    const uint64_t *cursors;    // [pair]: exclusive scan of counts (fill walk)
    uint64_t total;             // hits of the call = entries of ends / distances that may be written (fill walk)
    uint32_t *ends, *distances;
    bool wide_text;             // the text tape holds at least 16 bytes: it is read with 128-bit loads
};
void launch_infix_hits(Scope *scope, const InfixTapes &t, const InfixHitsRun &r, bool fill);

// The start pass over hits: hit h belongs to pair rows[h]; starts[h] = the largest s <= ends[h] with d(p, t[s..ends[h])) = distances[h].
// launch_infix_hit_items finds every hit's pair in the row offsets (`count` + 1 entries), writes it to `rows` and cuts the hits into
// items of consecutive hits (`items`: room for `total`; sizes->items counts them; `sizes` zeroed by the caller).
struct InfixHitStartsRun {
    const LaneItem *items;
    uint64_t item_count;
    const uint64_t *rows;
    const uint32_t *ends, *distances;
    uint32_t *starts;
};
void launch_infix_hit_items(Scope *scope, const InfixTapes &t, const uint64_t *row_offsets, uint64_t total, InfixSizes *sizes, uint64_t *rows,
                            LaneItem *items);
void launch_infix_hit_starts(Scope *scope, const InfixTapes &t, const InfixHitStartsRun &r);

}  // namespace swh
