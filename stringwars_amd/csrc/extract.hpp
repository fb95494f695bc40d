// extract.hpp -- launchers of the score searches' own kernels (extract.hip, extract_within.hip), called by two_tape.hip:
// swh_levenshtein_extract_* keeps the k best candidates of every query under an OSA, Indel, LCS, ratio, Jaro or Jaro-Winkler score,
// swh_levenshtein_extract_within_* every candidate that passes the cutoff, as CSR rows. The pairs are scored by the families' own
// launchers (osa.hpp, lcs.hpp, jaro.hpp) into a slice of counts; what lives here ranks or compacts them -- on one score function.
#pragma once
#include "common.hpp"

namespace swh {

constexpr int kExtractWaves = 4;
constexpr int kExtractBatch = 4;   // chunks of 64 columns whose loads are in flight together

template <int Scorer> constexpr bool kLargerIsBetter = Scorer >= SWH_SCORER_LCS;

// The score of one pair from its counts (ExtractSlice::counts) and the symbol lengths m (query) and n (candidate), operation by
// operation as the host writes it. Both searches call this one function: their scores agree bit for bit by construction.
template <int Scorer>
__device__ __forceinline__ double extract_score(uint64_t c0, uint64_t c1, uint64_t c2, uint32_t m, uint32_t n, double prefix_weight) {
#pragma clang fp contract(off)
    if constexpr (Scorer == SWH_SCORER_OSA) {
        return (double)c0;
    } else if constexpr (Scorer == SWH_SCORER_INDEL) {
        return (double)((uint64_t)m + n - 2 * c0);
    } else if constexpr (Scorer == SWH_SCORER_LCS) {
        return (double)c0;
    } else if constexpr (Scorer == SWH_SCORER_RATIO) {
        const double twice = 2.0 * (double)c0;
        const double total = (double)((uint64_t)m + n - 2 * c0) + twice;
        return total > 0 ? 100.0 * twice / total : 100.0;
    } else {
        double jaro;
        if (c0 > 0) {
            const double M = (double)c0, t = (double)c1;
            jaro = (M / (double)m + M / (double)n + (M - t) / M) / 3.0;
        } else {
            jaro = (m == 0 && n == 0) ? 1.0 : 0.0;
        }
        if constexpr (Scorer == SWH_SCORER_JARO_WINKLER) {
            if (jaro > 0.7) jaro = jaro + (double)c2 * prefix_weight * (1.0 - jaro);
        }
        return jaro;
    }
}

// Strings [0, count) of `tape` (device; `off64`-wide offsets): the first one with more than `limit` symbols goes to *first_over by
// atomic minimum (the caller sets it to ~0).
void launch_extract_first_over(Scope *scope, const TapeRef &tape, uint32_t off64, uint32_t limit, unsigned long long *first_over);

// One slice of one query block: rows [0, rows) of the count matrices (`columns` u64 entries per row, dense) are queries
// row_first + r of `a`, column c is candidate col_first + c of `b`. `counts`: OSA -- the distance; Indel, LCS, ratio -- the LCS
// length; Jaro -- matches, transpositions; Jaro-Winkler -- and the prefix.
struct ExtractSlice {
    const uint64_t *counts[3];
    TapeRef a, b;                 // the call's queries and candidates, whole: the symbol lengths come from their offsets
    uint32_t a_off64, b_off64;
    uint64_t rows, columns, row_first, col_first;
    int scorer;                   // SWH_SCORER_*
    uint64_t cutoff_bits;         // the float64 cutoff: distances admit d <= cutoff, similarities s >= cutoff
    double prefix_weight;
};

// The k best: the rows' running lists (k keys of 16 bytes per row, all bytes 0xFF where nothing was kept yet) are read from and
// written back to `lists`; with `emit` the rows leave instead: the index and the float64 score of every kept candidate, 0xFFFFFFFF
// and a pattern of ones where fewer than k were admitted.
struct ExtractLaunch : ExtractSlice {
    uint32_t k, emit;
    void *lists;                  // [rows][k] keys
    uint32_t *indices;            // [row_first + r][k]
    uint64_t *scores;             // [row_first + r][k]: float64 patterns
};
void launch_extract_select(Scope *scope, const ExtractLaunch &x);

// Every candidate that passes the cutoff (extract_within.hip). The count pass adds a row's hits of the slice to hits[row_first + r]
// (zeroed once per call; slices run in stream order). The fill pass stores them from cursors[row_first + r] onwards -- the candidate
// index and the score's 64 bits, in ascending candidate order, never at or beyond `total` -- and advances the cursor.
struct ExtractWithinLaunch : ExtractSlice {
    uint32_t *hits;               // count pass: [query]
    uint64_t *cursors;            // fill pass: [query], where the row's next hit goes (from the offsets scan of hits: scan.hpp)
    uint64_t total;               // fill pass: entries that `indices` and `scores` hold
    uint32_t *indices;
    uint64_t *scores;             // float64 patterns
};
void launch_extract_within(Scope *scope, const ExtractWithinLaunch &x, bool fill);

}  // namespace swh
