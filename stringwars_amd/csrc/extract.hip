// extract.hip -- the score search (swh_levenshtein_extract_*, include/stringwars_amd.h): for every query the k candidates with the
// best key (score, j) under an OSA, Indel, LCS, ratio, Jaro or Jaro-Winkler score, among those that pass the cutoff.
//
// The pairs are scored by the families' own kernels (osa.hip, lcs.hip, jaro.hip) into a slice of integer counts in scratch; the
// kernel here is the fold, topk.hip's k_topk_select with two differences.
//  - The score is a float64 that the host expressions (engines.py's _ratio, _jaro and _winkler, the header's formulas) define as a
//    chain of single IEEE operations on the counts and the two symbol lengths. extract_score (extract.hpp: the one function this
//    search and extract_within.hip's both call) performs the same chain: f64 division
//    is expanded to the correctly rounded v_div_scale / v_div_fmas / v_div_fixup sequence, and contraction is switched off for the
//    whole evaluation -- contracted, `jaro + l * p * (1.0 - jaro)` becomes a fused multiply-add that drops the product's rounding
//    and differs from the host in the last bit. So a score leaves with the 64 bits the host computes from the dense calls' counts.
//  - The key is wide (topk_fold.hpp's WideKey): the score's 64-bit pattern -- all scores are non-negative, so patterns order as the
//    values do; complemented for the scorers where larger is better -- and the 32-bit candidate index, compared lexicographically.
//    Ties are ties of float64 values, broken by the smaller index. The cutoff is the cap of the threshold: (cutoff pattern,
//    0xFFFFFFFF) is above every key with that score and below every key with a worse one, so a score at the cutoff is admitted.
//
// One wave per query row; lane c works on one candidate of a chunk of 64 columns, four chunks' counts and lengths requested
// together. Lists travel through scratch between the slices of a query block; the last slice writes indices and doubles.
#include "extract.hpp"
#include "topk_fold.hpp"

#include <algorithm>

namespace swh {

template <int Scorer>
__global__ __launch_bounds__(kExtractWaves * 64) void k_extract_select(ExtractLaunch x) {
    using Ops = KeyOps<WideKey>;
    constexpr bool kMax = kLargerIsBetter<Scorer>;
    constexpr int kCounts = Scorer == SWH_SCORER_JARO_WINKLER ? 3 : (Scorer == SWH_SCORER_JARO ? 2 : 1);
    __shared__ WideKey wave_list[kExtractWaves][64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t k = x.k;
    WideKey *list = wave_list[wave];
    WideKey *lists = (WideKey *)x.lists;
    const WideKey cap{kMax ? ~x.cutoff_bits : x.cutoff_bits, 0xFFFFFFFFu};
    for (uint64_t r = (uint64_t)blockIdx.x * kExtractWaves + wave; r < x.rows; r += (uint64_t)gridDim.x * kExtractWaves) {
        lds_order();
        if (lane < k) list[lane] = lists[r * k + lane];
        lds_order();
        WideKey threshold = list[k - 1];
        if (!Ops::less(threshold, cap)) threshold = cap;
        uint64_t q_start;
        uint32_t m;
        tape_extent(x.a, x.a_off64, x.row_first + r, q_start, m);
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
                WideKey key = Ops::pad();
                if (c < x.columns) {
                    const double score = extract_score<Scorer>(counts[u][0], counts[u][1], counts[u][2], m, n[u], x.prefix_weight);
                    const uint64_t bits = (uint64_t)__double_as_longlong(score);
                    key = WideKey{kMax ? ~bits : bits, (uint32_t)(x.col_first + c)};
                }
                const uint64_t admitted = __ballot(Ops::less(key, threshold));
                if (admitted) threshold = topk_fold(list, k, key, admitted, cap);
            }
        }
        if (lane < k) {
            const WideKey key = list[lane];
            if (x.emit) {
                const uint64_t out = (x.row_first + r) * k + lane;
                const bool kept = key.index != 0xFFFFFFFFu;
                x.indices[out] = key.index;
                x.scores[out] = kept ? (kMax ? ~key.score : key.score) : ~0ull;
            } else {
                lists[r * k + lane] = key;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_extract_first_over(TapeRef tape, uint32_t off64, uint32_t limit, unsigned long long *first_over) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= tape.count) return;
    uint64_t start;
    uint32_t len;
    tape_extent(tape, off64, i, start, len);
    if (len > limit) atomicMin(first_over, (unsigned long long)i);
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
void launch_extract_first_over(Scope *scope, const TapeRef &tape, uint32_t off64, uint32_t limit, unsigned long long *first_over) {
    if (!tape.count) return;
    StampGuard guard(scope, "extract_lengths");
    hipLaunchKernelGGL(k_extract_first_over, dim3((uint32_t)((tape.count + 255) / 256)), dim3(256), 0, scope->stream, tape, off64, limit, first_over);
    SWH_HIP_CHECK(hipGetLastError());
}

void launch_extract_select(Scope *scope, const ExtractLaunch &x) {
    const uint64_t blocks = std::min<uint64_t>((x.rows + kExtractWaves - 1) / kExtractWaves, (uint64_t)scope->compute_units * 16);
    const dim3 grid((uint32_t)(blocks ? blocks : 1)), block(kExtractWaves * 64);
    StampGuard guard(scope, "extract_select");
    switch (x.scorer) {
        case SWH_SCORER_OSA: hipLaunchKernelGGL(k_extract_select<SWH_SCORER_OSA>, grid, block, 0, scope->stream, x); break;
        case SWH_SCORER_INDEL: hipLaunchKernelGGL(k_extract_select<SWH_SCORER_INDEL>, grid, block, 0, scope->stream, x); break;
        case SWH_SCORER_LCS: hipLaunchKernelGGL(k_extract_select<SWH_SCORER_LCS>, grid, block, 0, scope->stream, x); break;
        case SWH_SCORER_RATIO: hipLaunchKernelGGL(k_extract_select<SWH_SCORER_RATIO>, grid, block, 0, scope->stream, x); break;
        case SWH_SCORER_JARO: hipLaunchKernelGGL(k_extract_select<SWH_SCORER_JARO>, grid, block, 0, scope->stream, x); break;
        default: hipLaunchKernelGGL(k_extract_select<SWH_SCORER_JARO_WINKLER>, grid, block, 0, scope->stream, x); break;
    }
    SWH_HIP_CHECK(hipGetLastError());
}

}  // namespace swh
