// topk.hip -- Levenshtein top-k search: for every query the k candidates with the smallest key (d, j) among those with d <= bound
// (swh_levenshtein_topk_*, include/stringwars_amd.h). The dense cross-product writes queries x candidates results; a search keeps only
// k per query, so the matrix is never written and the pair count is not limited by what a matrix (or a 32-bit pair index) can hold.
//
// A candidate j of query i is ranked by the 64-bit key (d << 32) | j: ascending keys are ascending distances with ties broken by the
// smaller candidate index, and every key is distinct. A row's running list is its k smallest keys so far, sorted, padded with
// kTopkPad (index and distance 0xFFFFFFFF); its threshold T = min(list[k - 1], cap), cap = (bound + 1) << 32, is wave-uniform.
// A wave's 64 fresh keys are admitted with one compare and one ballot (key < T): once a list is warm nearly every ballot is empty
// and that is all the selection costs. Admitted keys are merged by rank (topk_fold): a key's place in the new list is the number of
// list entries below it plus the number of admitted keys below it, every list entry moves down by the admitted keys below it, and
// whatever lands at k or beyond drops out.
//
// Kernels:
//   k_cross_topk<Off>   word-sized byte strings (<= 32 bytes, unit costs: the route the dense call takes to k_cross_short). The item is
//                       cross_words.hpp's -- 16 queries x one slice of the candidates -- with the distances folded into 16 lists
//                       instead of stored. Chunks whose every lane has |m - n| >= T are skipped: d >= |m - n| (on 2048 x 2048 random
//                       words this measured neither faster nor slower than walking them). Each item leaves its 16 lists in the
//                       outputs (one slice) or in scratch (several).
//   k_topk_merge        one wave per query: the slices' partial lists folded into the final row.
//   k_topk_select<Max>  the general path: one wave per query row folds a slice of a dense u32 distance matrix (scored by the
//                       ordinary cross-product routes into scratch) into the row's running list. `Max` ranks by the largest score
//                       (key (~s << 32) | j); only the distance form is built. (The search by a float64 score -- OSA, Indel, LCS,
//                       ratio, Jaro, Jaro-Winkler -- is extract.hip's, with a wider key on the same fold.)
#include "cross_words.hpp"
#include "topk_fold.hpp"

#include <algorithm>

namespace swh {

constexpr int kTopkWaves = kWordWaves;   // (also the merge and select kernels': one wave per row)
constexpr uint64_t kTopkPad = ~0ull;

// (topk_fold, the merge by rank of the admitted keys into a row's sorted list, is topk_fold.hpp's: the key is its type parameter, and the
// keys here are its uint64_t instantiation.)

// The same fold for the fused kernel, where the fresh keys come from ONE chunk (candidate = chunk * 64 + lane: the key order among them
// is (d, lane)) and every list entry from an earlier chunk of the item (a smaller candidate index than any fresh key): ranks are
// counted per distance level with two ballots -- one step per distance up to the largest admitted one (word-sized strings: <= 32),
// instead of one broadcast per admitted lane (64 when a list is empty) and a binary search of the list.
__device__ __forceinline__ uint64_t topk_fold_chunk(uint64_t *list, uint32_t k, uint64_t key, uint64_t admitted, uint64_t cap) {
    const uint32_t lane = __lane_id();
    const uint64_t own = lane < k ? list[lane] : kTopkPad;
    const bool mine = (admitted >> lane) & 1ull;
    const uint32_t d = (uint32_t)(key >> 32), od = (uint32_t)(own >> 32);   // (a pad's 0xFFFFFFFF is above every level)
    const uint64_t lanes_below = (1ull << lane) - 1ull;
    uint32_t below_key = 0, below_own = 0, list_upto_key = 0;
    uint64_t rest = admitted;
    for (uint32_t v = 0; rest; ++v) {
        const uint64_t level = __ballot(mine && d == v), list_level = __ballot(lane < k && od == v);
        rest &= ~level;
        const uint32_t count = (uint32_t)__popcll(level);
        below_key += v < d ? count : (v == d ? (uint32_t)__popcll(level & lanes_below) : 0u);
        below_own += v < od ? count : 0u;
        list_upto_key += v <= d ? (uint32_t)__popcll(list_level) : 0u;
    }
    lds_order();
    if (mine) {
        const uint32_t rank = list_upto_key + below_key;
        if (rank < k) list[rank] = key;
    }
    if (lane < k) {
        const uint32_t rank = lane + below_own;
        if (rank < k) list[rank] = own;
    }
    lds_order();
    const uint64_t last = list[k - 1];
    return last < cap ? last : cap;
}

__device__ __forceinline__ void topk_emit(uint64_t key, uint32_t *index, uint32_t *distance) {
    *index = (uint32_t)key;
    *distance = (uint32_t)(key >> 32);
}

struct TopkArgs {
    WordSearchArgs search;     // prune: skip a query's chunk when every lane's |m - n| bound is >= T
    uint32_t k;                // list length
    uint64_t cap;              // admitted keys are below it: (bound + 1) << 32, or kTopkPad
    uint64_t *partial;         // slices > 1: [query][slice][k] keys
    uint32_t *indices, *distances;   // slices == 1: the rows themselves
};

template <typename Off>
__global__ __launch_bounds__(kTopkWaves * 64, 3) void k_cross_topk(TopkArgs args) {
    __shared__ WordSearchLds lds;
    extern __shared__ uint64_t topk_lists[];   // [wave][query][k]
    const uint32_t lane = threadIdx.x & 63, k = args.k, slices = args.search.slices;
    uint64_t *lists = topk_lists + (size_t)(threadIdx.x >> 6) * kWordQueries * k;
    uint64_t thresholds = args.cap, threshold = 0;   // lane q: T of query q; T of the query at hand
    word_search_items<Off, true>(args.search, lds,
        [&](const WordItem &item) {
            for (uint32_t q = 0; q < item.q_count; ++q)
                if (lane < k) lists[q * k + lane] = kTopkPad;
            thresholds = args.cap;
        },
        [&](uint32_t q, uint32_t gap) { threshold = readlane64(thresholds, (int)q); return ((uint64_t)gap << 32) < threshold; },
        [&](uint32_t q, const WordCandidate &c, uint32_t d) {
            const uint64_t key = c.fits ? ((uint64_t)d << 32 | c.cand) : kTopkPad;
            const uint64_t admitted = __ballot(key < threshold);
            if (admitted) {
                threshold = topk_fold_chunk(lists + q * k, k, key, admitted, args.cap);
                if (lane == q) thresholds = threshold;
            }
        },
        // the item's lists leave: the rows themselves, or this slice's partial lists
        [&](const WordItem &item) {
            lds_order();
            for (uint32_t q = 0; q < item.q_count; ++q) {
                if (lane >= k) continue;
                const uint64_t key = lists[q * k + lane];
                const uint64_t row = item.q_first + q;
                if (slices == 1) topk_emit(key, args.indices + row * k + lane, args.distances + row * k + lane);
                else args.partial[(row * slices + item.slice) * k + lane] = key;
            }
            lds_order();
        });
}

// One wave per query: the query's `slices` partial lists (each sorted, k keys) folded into its final row.
__global__ __launch_bounds__(kTopkWaves * 64) void k_topk_merge(const uint64_t *partial, uint64_t rows, uint32_t slices, uint32_t k,
                                                                uint32_t *indices, uint32_t *distances) {
    __shared__ uint64_t wave_list[kTopkWaves][64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t *list = wave_list[wave];
    for (uint64_t row = (uint64_t)blockIdx.x * kTopkWaves + wave; row < rows; row += (uint64_t)gridDim.x * kTopkWaves) {
        const uint64_t *mine = partial + row * slices * k;
        lds_order();
        if (lane < k) list[lane] = mine[lane];
        lds_order();
        uint64_t threshold = list[k - 1];
        for (uint32_t s0 = 1; s0 < slices; s0 += 8) {
            uint64_t keys[8];   // eight slices' lists requested together: one memory latency per eight folds, not per fold
#pragma unroll
            for (uint32_t u = 0; u < 8; ++u) keys[u] = (s0 + u < slices && lane < k) ? mine[(uint64_t)(s0 + u) * k + lane] : kTopkPad;
#pragma unroll
            for (uint32_t u = 0; u < 8; ++u) {
                const uint64_t admitted = __ballot(keys[u] < threshold);
                if (admitted) threshold = topk_fold(list, k, keys[u], admitted, kTopkPad);
            }
        }
        if (lane < k) topk_emit(list[lane], indices + row * k + lane, distances + row * k + lane);
    }
}

// The general path's fold: rows [0, rows) of a dense u32 matrix (`columns` wide) are queries row_first + r, column c is candidate
// col_first + c. Lists (k keys per row, from the previous slice or kTopkPad) are read from and written back to `lists`; with `emit`
// the rows leave as indices / distances instead.
struct TopkSelectArgs {
    const uint32_t *scores;
    uint64_t rows, columns, row_first, col_first;
    uint32_t k, emit;
    uint64_t cap;
    uint64_t *lists;                  // [rows][k]: this query block's running lists
    uint32_t *indices, *distances;    // [row_first + r][k]
};

template <bool Max>
__device__ __forceinline__ uint64_t topk_key(uint32_t score, uint64_t j) {
    return (uint64_t)(Max ? ~score : score) << 32 | j;
}

template <bool Max>
__global__ __launch_bounds__(kTopkWaves * 64) void k_topk_select(TopkSelectArgs args) {
    __shared__ uint64_t wave_list[kTopkWaves][64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t k = args.k;
    uint64_t *list = wave_list[wave];
    for (uint64_t r = (uint64_t)blockIdx.x * kTopkWaves + wave; r < args.rows; r += (uint64_t)gridDim.x * kTopkWaves) {
        lds_order();
        if (lane < k) list[lane] = args.lists[r * k + lane];
        lds_order();
        uint64_t threshold = list[k - 1] < args.cap ? list[k - 1] : args.cap;
        const uint32_t *row = args.scores + r * args.columns;
        for (uint64_t c0 = 0; c0 < args.columns; c0 += 64) {
            const uint64_t c = c0 + lane;
            const uint64_t key = c < args.columns ? topk_key<Max>(row[c], args.col_first + c) : kTopkPad;
            const uint64_t admitted = __ballot(key < threshold);
            if (admitted) threshold = topk_fold(list, k, key, admitted, args.cap);
        }
        if (lane < k) {
            const uint64_t key = list[lane];
            if (args.emit) {
                const uint64_t out = (args.row_first + r) * k + lane;
                // (Max: the score is stored back as it came; pads stay 0xFFFFFFFF)
                topk_emit(Max && key != kTopkPad ? (key ^ 0xFFFFFFFF00000000ull) : key, args.indices + out, args.distances + out);
            } else {
                args.lists[r * k + lane] = key;
            }
        }
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
size_t topk_fused_lds(uint32_t k) { return (size_t)kWordWaves * kWordQueries * k * sizeof(uint64_t); }

void launch_cross_topk(Scope *scope, const TopkLaunch &t) {
    TopkArgs args{};
    args.search = {t.a, t.b, t.slices, t.prune, t.slice_chunks, scope->plan_partials, scope->done_counter, scope->summary_target()};
    args.k = t.k; args.cap = t.cap; args.partial = t.partial; args.indices = t.indices; args.distances = t.distances;
    const uint32_t blocks = word_item_blocks(scope, ((t.a.count + kWordQueries - 1) / kWordQueries) * t.slices);
    const size_t lds = topk_fused_lds(t.k);
    {
        StampGuard guard(scope, "cross_topk");
        if (t.off64) hipLaunchKernelGGL(k_cross_topk<uint64_t>, dim3(blocks), dim3(kTopkWaves * 64), lds, scope->stream, args);
        else hipLaunchKernelGGL(k_cross_topk<uint32_t>, dim3(blocks), dim3(kTopkWaves * 64), lds, scope->stream, args);
        SWH_HIP_CHECK(hipGetLastError());
    }
    if (t.slices > 1) {
        const uint64_t merge_blocks = std::min<uint64_t>((t.a.count + kTopkWaves - 1) / kTopkWaves, (uint64_t)scope->compute_units * 16);
        StampGuard guard(scope, "topk_merge");
        hipLaunchKernelGGL(k_topk_merge, dim3((uint32_t)merge_blocks), dim3(kTopkWaves * 64), 0, scope->stream, (const uint64_t *)t.partial,
                           (uint64_t)t.a.count, t.slices, t.k, t.indices, t.distances);
        SWH_HIP_CHECK(hipGetLastError());
    }
}

void launch_topk_select(Scope *scope, const uint32_t *scores, uint64_t rows, uint64_t columns, uint64_t row_first, uint64_t col_first, uint32_t k,
                        uint64_t cap, uint64_t *lists, bool emit, uint32_t *indices, uint32_t *distances) {
    TopkSelectArgs args{};
    args.scores = scores; args.rows = rows; args.columns = columns; args.row_first = row_first; args.col_first = col_first;
    args.k = k; args.emit = emit ? 1u : 0u; args.cap = cap; args.lists = lists; args.indices = indices; args.distances = distances;
    const uint64_t blocks = std::min<uint64_t>((rows + kTopkWaves - 1) / kTopkWaves, (uint64_t)scope->compute_units * 16);
    StampGuard guard(scope, "topk_select");
    hipLaunchKernelGGL(k_topk_select<false>, dim3((uint32_t)(blocks ? blocks : 1)), dim3(kTopkWaves * 64), 0, scope->stream, args);
    SWH_HIP_CHECK(hipGetLastError());
}

}  // namespace swh
