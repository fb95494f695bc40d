// align.hpp -- launchers of the Levenshtein alignment kernels (align.hip), called by two_tape.hip.
// Kept apart from common.hpp, which every kernel family's profile stamp hashes (tools/kernel_sources.py).
#pragma once
#include "common.hpp"

namespace swh {

// One batch of pairs on prepared (device-resident, measured, decoded) tapes. Symbols are bytes (`cp` = 0, each tape's
// offsets u32 or u64 by its `off64`) or code points (`cp` = 1: u32 symbols, u64 offsets).
struct AlignTapes {
    TapeRef a, b;
    uint32_t a_off64, b_off64, cp;
    uint64_t count;
};

// What k_align_sizes measures over the whole batch, read back by the host before anything is written.
struct AlignSizes {
    unsigned long long store_total;   // bytes of stored delta vectors over all pairs
    unsigned long long symbols;       // sum len(a_i) + len(b_i): the ops capacity the call needs
    unsigned long long cells;         // sum len(a_i) * len(b_i)
    unsigned long long max_store;     // the largest single pair's stored bytes
    unsigned long long first_oversize;   // the first pair with len(a) * len(b) > SWH_ALIGN_MAX_CELLS, or ~0
};

// Per pair: stored bytes -> store_base[i], len(a) + len(b) -> slot_base[i] (both then scanned in place: scan.hpp), and `sizes`
// (zeroed by the caller, first_oversize set to ~0).
void launch_align_sizes(Scope *scope, const AlignTapes &t, uint64_t *store_base, uint64_t *slot_base, AlignSizes *sizes);

// The forward pass and the walk of pairs [pair_first, pair_end); `store` holds their part of the batch's storage space, which
// starts at store_first = store_base[pair_first]. The walk writes pair i's ops, in forward order, to the END of its slot
// [slot_base[i], slot_base[i] + len(a_i) + len(b_i)) of `slots`, their number to counts[i] and min(d, bound + 1) to distances[i].
struct AlignChunk {
    const uint64_t *store_base, *slot_base;
    uint64_t pair_first, pair_end, store_first;
    char *store;
    uint8_t *slots;
    uint32_t *counts, *distances;
    uint32_t bound;
};
void launch_align_chunk(Scope *scope, const AlignTapes &t, const AlignChunk &c);
// ops[offsets[i] ..] = the last counts[i] bytes of pair i's slot
void launch_align_emit(Scope *scope, uint64_t count, const uint64_t *slot_base, const uint32_t *counts, const uint64_t *offsets,
                       const uint8_t *slots, uint8_t *ops);

}  // namespace swh
