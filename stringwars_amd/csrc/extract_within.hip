// extract_within.hip -- the score range search (swh_levenshtein_extract_within_*, include/stringwars_amd.h): for every query EVERY
// candidate whose OSA, Indel, LCS, ratio, Jaro or Jaro-Winkler score passes the cutoff, as CSR rows of unknown length.
//
// It is extract.hip's walk with within.hip's compaction in place of the fold. The pairs are scored by the families' own kernels into
// a slice of integer counts in scratch; the kernel here evaluates the float64 score with extract_score (extract.hpp: the function
// k_extract_select calls, so a pair has the same 64 bits in both searches) and tests it as k_extract_select's `cap` does: on the bit
// pattern, complemented where the larger score is the better one, so any cutoff admits the same pairs in both calls and a score at
// the cutoff is admitted.
//
// The pairs are walked twice. The count pass adds popcount(ballot) to the row's count; the offsets scan (scan.hip) turns the counts
// into cursors and row offsets; the fill pass repeats the walk and stores a hit at the row's cursor plus the hits in the lanes below it.
// One wave per query row and slices in stream order: a row meets its candidates in ascending order, no atomics touch the output,
// nothing is sorted, and every run writes the same bytes.
#include "extract.hpp"
#include "topk_fold.hpp"

#include <algorithm>

namespace swh {

template <int Scorer, bool Fill>
__global__ __launch_bounds__(kExtractWaves * 64) void k_extract_within(ExtractWithinLaunch x) {
    using Ops = KeyOps<WideKey>;
    constexpr bool kMax = kLargerIsBetter<Scorer>;
    constexpr int kCounts = Scorer == SWH_SCORER_JARO_WINKLER ? 3 : (Scorer == SWH_SCORER_JARO ? 2 : 1);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t lanes_below = (1ull << lane) - 1ull;
    // (cutoff pattern, 0xFFFFFFFF) is above every key with that score and below every key with a worse one
    const WideKey cap{kMax ? ~x.cutoff_bits : x.cutoff_bits, 0xFFFFFFFFu};
    for (uint64_t r = (uint64_t)blockIdx.x * kExtractWaves + wave; r < x.rows; r += (uint64_t)gridDim.x * kExtractWaves) {
        uint64_t q_start;
        uint32_t m;
        tape_extent(x.a, x.a_off64, x.row_first + r, q_start, m);
        uint32_t found = 0;
        uint64_t cursor = 0;
        if constexpr (Fill) cursor = x.cursors[x.row_first + r];
        for (uint64_t c0 = 0; c0 < x.columns; c0 += 64 * kExtractBatch) {
            uint64_t counts[kExtractBatch][3] = {};
            uint32_t n[kExtractBatch] = {};
#pragma unroll
            for (int u = 0; u < kExtractBatch; ++u) {
                const uint64_t c = c0 + (uint64_t)u * 64 + lane;
                if (c < x.columns) {
                    uint64_t c_start;
#pragma unroll
                    for (int o = 0; o < kCounts; ++o) counts[u][o] = x.counts[o][r * x.columns + c];
                    tape_extent(x.b, x.b_off64, x.col_first + c, c_start, n[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < kExtractBatch; ++u) {
                const uint64_t c = c0 + (uint64_t)u * 64 + lane;
                if (c0 + (uint64_t)u * 64 >= x.columns) break;   // wave-uniform
                uint64_t bits = 0;
                bool hit = false;
                if (c < x.columns) {
                    const double score = extract_score<Scorer>(counts[u][0], counts[u][1], counts[u][2], m, n[u], x.prefix_weight);
                    bits = (uint64_t)__double_as_longlong(score);
                    hit = Ops::less(WideKey{kMax ? ~bits : bits, (uint32_t)(x.col_first + c)}, cap);
                }
                const uint64_t hits = __ballot(hit);
                if constexpr (Fill) {
                    const uint64_t at = cursor + (uint64_t)__popcll(hits & lanes_below);
                    if (hit && at < x.total) {   // (a total the walk outgrows: the tapes changed between the passes -- never past the arrays)
                        x.indices[at] = (uint32_t)(x.col_first + c);
                        x.scores[at] = bits;
                    }
                    cursor += (uint64_t)__popcll(hits);
                } else {
                    found += (uint32_t)__popcll(hits);
                }
            }
        }
        // (one wave per row, slices in stream order: no other writer)
        if (lane == 0) {
            if constexpr (Fill) x.cursors[x.row_first + r] = cursor;
            else x.hits[x.row_first + r] += found;
        }
    }
}

template <int Scorer>
static void launch_scorer(const ExtractWithinLaunch &x, bool fill, dim3 grid, dim3 block, hipStream_t stream) {
    if (fill) hipLaunchKernelGGL((k_extract_within<Scorer, true>), grid, block, 0, stream, x);
    else hipLaunchKernelGGL((k_extract_within<Scorer, false>), grid, block, 0, stream, x);
}

void launch_extract_within(Scope *scope, const ExtractWithinLaunch &x, bool fill) {
    const uint64_t blocks = std::min<uint64_t>((x.rows + kExtractWaves - 1) / kExtractWaves, (uint64_t)scope->compute_units * 16);
    const dim3 grid((uint32_t)(blocks ? blocks : 1)), block(kExtractWaves * 64);
    StampGuard guard(scope, "extract_within");
    switch (x.scorer) {
        case SWH_SCORER_OSA: launch_scorer<SWH_SCORER_OSA>(x, fill, grid, block, scope->stream); break;
        case SWH_SCORER_INDEL: launch_scorer<SWH_SCORER_INDEL>(x, fill, grid, block, scope->stream); break;
        case SWH_SCORER_LCS: launch_scorer<SWH_SCORER_LCS>(x, fill, grid, block, scope->stream); break;
        case SWH_SCORER_RATIO: launch_scorer<SWH_SCORER_RATIO>(x, fill, grid, block, scope->stream); break;
        case SWH_SCORER_JARO: launch_scorer<SWH_SCORER_JARO>(x, fill, grid, block, scope->stream); break;
        default: launch_scorer<SWH_SCORER_JARO_WINKLER>(x, fill, grid, block, scope->stream); break;
    }
    SWH_HIP_CHECK(hipGetLastError());
}

}  // namespace swh
