// extract.hpp -- launchers of the score search's own kernels (extract.hip), called by two_tape.hip: swh_levenshtein_extract_* keeps the k
// best candidates of every query under an OSA, Indel, LCS, ratio, Jaro or Jaro-Winkler score. The pairs are scored by the families'
// own launchers (osa.hpp, lcs.hpp, jaro.hpp) into a slice of counts; what lives here ranks them.
#pragma once
#include "common.hpp"

namespace swh {

// Strings [0, count) of `tape` (device; `off64`-wide offsets): the first one with more than `limit` symbols goes to *first_over by
// atomic minimum (the caller sets it to ~0).
void launch_extract_first_over(Scope *scope, const TapeRef &tape, uint32_t off64, uint32_t limit, unsigned long long *first_over);

// One slice of one query block: rows [0, rows) of the count matrices (`columns` u64 entries per row, dense) are queries
// row_first + r of `a`, column c is candidate col_first + c of `b`. `counts`: OSA -- the distance; Indel, LCS, ratio -- the LCS
// length; Jaro -- matches, transpositions; Jaro-Winkler -- and the prefix. The rows' running lists (k keys of 16 bytes per row, all
// bytes 0xFF where nothing was kept yet) are read from and written back to `lists`; with `emit` the rows leave instead: the index
// and the float64 score of every kept candidate, 0xFFFFFFFF and a pattern of ones where fewer than k were admitted.
struct ExtractLaunch {
    const uint64_t *counts[3];
    TapeRef a, b;                 // the call's queries and candidates, whole: the symbol lengths come from their offsets
    uint32_t a_off64, b_off64;
    uint64_t rows, columns, row_first, col_first;
    int scorer;                   // SWH_SCORER_*
    uint32_t k, emit;
    uint64_t cutoff_bits;         // the float64 cutoff: distances admit d <= cutoff, similarities s >= cutoff
    double prefix_weight;
    void *lists;                  // [rows][k] keys
    uint32_t *indices;            // [row_first + r][k]
    uint64_t *scores;             // [row_first + r][k]: float64 patterns
};
void launch_extract_select(Scope *scope, const ExtractLaunch &x);

}  // namespace swh
