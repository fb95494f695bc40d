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
//   k_cross_topk<Off>   word-sized byte strings (<= 32 bytes, unit costs: the route the dense call takes to k_cross_short). The
//                       column walk is k_cross_short's -- candidates in lanes, the query's match table once per wave in LDS -- and the
//                       store is replaced by the selection. A work item is 16 queries x one slice of the candidates: the 16 tables
//                       are built once per item and reused for every chunk of 64 candidates of the slice (the dense kernel's item
//                       is one chunk, so it builds each table once per chunk). Chunks whose every lane has |m - n| >= T are skipped:
//                       d >= |m - n| (on 2048 x 2048 random words this measured neither faster nor slower than walking them).
//                       Each item leaves its 16 lists in the outputs (one slice) or in scratch (several).
//   k_topk_merge        one wave per query: the slices' partial lists folded into the final row.
//   k_topk_select<Max>  the general path: one wave per query row folds a slice of a dense u32 distance matrix (scored by the
//                       ordinary cross-product routes into scratch) into the row's running list. `Max` ranks by the largest score
//                       (key (~s << 32) | j) -- the same code for a later score-maximising search; only the distance form is built.
#include "common.hpp"
#include "bp_lanes.hpp"   // the offset reader, lds_order, readlane64

#include <algorithm>

namespace swh {

constexpr uint32_t kTopkLongest = 32;   // longest query / candidate of the fused kernel, bytes
constexpr int kTopkQueries = 16;        // queries per work item
constexpr int kTopkWaves = 4;
constexpr uint64_t kTopkPad = ~0ull;

// Merges the keys of the `admitted` lanes into the wave's sorted list of k keys (LDS, k <= 64) and returns the new threshold.
// Keys are distinct (candidate indices are), and no admitted key is a pad: ranks in the union are a permutation.
__device__ __forceinline__ uint64_t topk_fold(uint64_t *list, uint32_t k, uint64_t key, uint64_t admitted, uint64_t cap) {
    const uint32_t lane = __lane_id();
    const uint64_t own = lane < k ? list[lane] : kTopkPad;
    uint32_t below_key = 0, below_own = 0;
    for (uint64_t rest = admitted; rest; rest &= rest - 1) {
        const uint64_t other = readlane64(key, __builtin_ctzll(rest));
        below_key += other < key ? 1u : 0u;
        below_own += other < own ? 1u : 0u;
    }
    uint32_t at = 0;   // list entries below my key
#pragma unroll
    for (uint32_t step = 64; step; step >>= 1)
        if (at + step <= k && list[at + step - 1] < key) at += step;
    lds_order();
    if ((admitted >> lane) & 1ull) {
        const uint32_t rank = at + below_key;
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
    TapeRef a, b;              // queries, candidates: device byte tapes
    uint32_t k, slices;        // list length; candidate slices per query block
    uint64_t slice_chunks;     // chunks of 64 candidates per slice
    uint64_t cap;              // admitted keys are below it: (bound + 1) << 32, or kTopkPad
    uint32_t prune;            // skip a query's chunk when every lane's |m - n| bound is >= T
    uint64_t *partial;         // slices > 1: [query][slice][k] keys
    uint32_t *indices, *distances;   // slices == 1: the rows themselves
    PlanPartial *partials;
    uint32_t *done_counter;
    CallSummary *summary;
};

struct TopkWaveLds {
    uint32_t table[kTopkQueries][32];   // Lo[16] | Hi[16] of each query of the item
    uint32_t qlen[kTopkQueries];
};

template <typename Off>
__global__ __launch_bounds__(kTopkWaves * 64, 3) void k_cross_topk(TopkArgs args) {
    __shared__ TopkWaveLds wave_lds[kTopkWaves];
    extern __shared__ uint64_t topk_lists[];   // [wave][query][k]
    __shared__ SummaryLds summary_lds;
    __shared__ unsigned long long lcells, lsyms;
    __shared__ uint32_t lmaxa, lmaxb, lshorts, lmisfit;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    TopkWaveLds &wl = wave_lds[wave];
    const uint32_t k = args.k;
    uint64_t *lists = topk_lists + (size_t)wave * kTopkQueries * k;
    if (threadIdx.x == 0) { lcells = 0; lsyms = 0; lmaxa = 0; lmaxb = 0; lshorts = 0; lmisfit = 0; }
    __syncthreads();
    const uint64_t na = args.a.count, nb = args.b.count;
    const uint8_t *a_data = (const uint8_t *)args.a.data, *b_data = (const uint8_t *)args.b.data;
    const uint64_t b_total = (uint64_t)((const Off *)args.b.offsets)[nb];
    const uint64_t chunks = (nb + 63) / 64, qblocks = (na + kTopkQueries - 1) / kTopkQueries;
    const uint64_t items = qblocks * args.slices;
    const uint64_t waves_total = (uint64_t)gridDim.x * kTopkWaves, wave_id = (uint64_t)blockIdx.x * kTopkWaves + wave;
    unsigned long long cells = 0, syms = 0;
    uint32_t maxa = 0, maxb = 0, shorts = 0, misfit = 0;

    for (uint64_t item = wave_id; item < items; item += waves_total) {
        // neighbouring waves take neighbouring query blocks of one slice: the slice's candidates stay warm in the cache
        const uint64_t slice = item / qblocks, qb = item - slice * qblocks;
        const uint64_t q_first = qb * kTopkQueries, q_last = q_first + kTopkQueries < na ? q_first + kTopkQueries : na;
        const uint32_t q_count = (uint32_t)(q_last - q_first);
        // ---- the item's 16 match tables: lane l takes bytes 8 (l % 4) .. 8 (l % 4) + 7 of query l / 4 -------------------------
        const uint32_t ql = (uint32_t)lane >> 2, part = (uint32_t)lane & 3u;
        uint64_t qa0 = 0;
        uint32_t qm = 0;
        if (ql < q_count) tape_extent<Off>(args.a.offsets, q_first + ql, qa0, qm);
        uint32_t staged[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t at = part * 8 + (uint32_t)t;
            staged[t] = (at < qm && qm <= kTopkLongest) ? a_data[qa0 + at] : 0u;
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) (&wl.table[0][0])[lane * 8 + t] = 0;
        for (uint32_t q = 0; q < q_count; ++q)
            if ((uint32_t)lane < k) lists[q * k + lane] = kTopkPad;
        lds_order();
        if (part == 0) wl.qlen[ql] = ql < q_count ? qm : 0u;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t at = part * 8 + (uint32_t)t;
            if (at < qm && qm <= kTopkLongest) {
                atomicOr(&wl.table[ql][staged[t] & 15u], 1u << at);
                atomicOr(&wl.table[ql][16 + (staged[t] >> 4)], 1u << at);
            }
        }
        if (ql < q_count && qm > kTopkLongest) misfit = 1;
        lds_order();
        unsigned long long sum_m = 0;
        uint32_t item_maxa = 0;
        for (uint32_t q = 0; q < q_count; ++q) {
            const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)wl.qlen[q]);
            sum_m += m;
            item_maxa = m > item_maxa ? m : item_maxa;
        }
        uint64_t thresholds = args.cap;   // lane q: T of query q
        // ---- the slice's chunks of 64 candidates --------------------------------------------------------------------------------
        const uint64_t c_first = slice * args.slice_chunks;
        const uint64_t c_last = c_first + args.slice_chunks < chunks ? c_first + args.slice_chunks : chunks;
        for (uint64_t chunk = c_first; chunk < c_last; ++chunk) {
            const uint64_t cand = chunk * 64 + (uint64_t)lane;
            const bool have = cand < nb;
            uint64_t b0 = 0;
            uint32_t n = 0;
            if (have) tape_extent<Off>(args.b.offsets, cand, b0, n);
            const bool fits = have && n <= kTopkLongest;
            if (have && !fits) misfit = 1;
            uint32_t tw[8];
            {
                ByteWindow txt;
                txt.init(b_data, b0, b_total);
                if (b_total >= 16) {
                    uint32_t half[4];
                    int moved = txt.fetch16_raw(0, half);
                    txt.fix16(0, moved, half);
#pragma unroll
                    for (int w = 0; w < 4; ++w) tw[w] = half[w];
                    moved = txt.fetch16_raw(16, half);
                    txt.fix16(16, moved, half);
#pragma unroll
                    for (int w = 0; w < 4; ++w) tw[4 + w] = half[w];
                } else {
#pragma unroll
                    for (int w = 0; w < 8; ++w) tw[w] = txt.fetch4(w * 4);
                }
            }
            const uint32_t n_live = fits ? n : 0;
            const uint32_t n_max = wave_max_u32(n_live);
            for (uint32_t q = 0; q < q_count; ++q) {
                const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)wl.qlen[q]);
                if (m > kTopkLongest) continue;
                uint64_t threshold = readlane64(thresholds, (int)q);
                if (args.prune) {
                    const uint32_t gap = m > n ? m - n : n - m;
                    if (!__ballot(fits && ((uint64_t)gap << 32) < threshold)) continue;
                }
                const uint32_t *table = wl.table[q];
                uint32_t pv = 0xFFFFFFFFu, mv = 0;
#pragma unroll
                for (int w4 = 0; w4 < 8; ++w4) {
                    if ((uint32_t)w4 * 4 >= n_max) break;
                    const uint32_t w = tw[w4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const uint32_t lo_at = (u == 0 ? (w << 2) : (w >> (8 * u - 2))) & 0x3Cu;
                        const uint32_t hi_at = (w >> (8 * u + 2)) & 0x3Cu;
                        const uint32_t eq = *(const uint32_t *)((const char *)table + lo_at) & *(const uint32_t *)((const char *)table + 64 + hi_at);
                        if ((uint32_t)(w4 * 4 + u) < n_live) {
                            const uint32_t xv = eq | mv;
                            const uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
                            uint32_t ph = mv | ~(xh | pv);
                            const uint32_t mh = pv & xh;
                            ph = (ph << 1) | 1u;
                            pv = (mh << 1) | ~(xv | ph);
                            mv = ph & xv;
                        }
                    }
                }
                const uint32_t mask = m >= 32 ? 0xFFFFFFFFu : ((1u << m) - 1u);
                const uint32_t d = n + __popc(pv & mask) - __popc(mv & mask);
                const uint64_t key = fits ? ((uint64_t)d << 32 | cand) : kTopkPad;
                const uint64_t admitted = __ballot(key < threshold);
                if (admitted) {
                    threshold = topk_fold_chunk(lists + q * k, k, key, admitted, args.cap);
                    if ((uint32_t)lane == q) thresholds = threshold;
                }
            }
            if (have) {
                cells += sum_m * (unsigned long long)n;
                maxb = n > maxb ? n : maxb;
                if (qb == 0) syms += n;                                // every candidate once ...
                if (fits) shorts += q_count;
            }
        }
        if (lane == 0) {
            maxa = item_maxa > maxa ? item_maxa : maxa;
            if (slice == 0) syms += sum_m;                             // ... and every query once
        }
        // ---- the item's lists leave: the rows themselves, or this slice's partial lists -------------------------------------------
        lds_order();
        for (uint32_t q = 0; q < q_count; ++q) {
            if ((uint32_t)lane >= k) continue;
            const uint64_t key = lists[q * k + lane];
            const uint64_t row = q_first + q;
            if (args.slices == 1) topk_emit(key, args.indices + row * k + lane, args.distances + row * k + lane);
            else args.partial[(row * args.slices + slice) * k + lane] = key;
        }
        lds_order();
    }
    // ---- summary ---------------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        cells += __shfl_xor(cells, off);
        syms += __shfl_xor(syms, off);
        shorts += __shfl_xor(shorts, off);
        misfit |= __shfl_xor(misfit, off);
        const uint32_t oa = __shfl_xor(maxa, off), ob = __shfl_xor(maxb, off);
        maxa = oa > maxa ? oa : maxa;
        maxb = ob > maxb ? ob : maxb;
    }
    if (lane == 0) {
        atomicAdd(&lcells, cells);
        atomicAdd(&lsyms, syms);
        atomicAdd(&lshorts, shorts);
        atomicMax(&lmaxa, maxa);
        atomicMax(&lmaxb, maxb);
        atomicOr(&lmisfit, misfit);
    }
    __syncthreads();
    report_call_summary(PlanPartial{lcells, lsyms, lmaxa, lmaxb, lshorts, lmisfit}, args.partials, args.done_counter, args.summary, summary_lds);
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
size_t topk_fused_lds(uint32_t k) { return (size_t)kTopkWaves * kTopkQueries * k * sizeof(uint64_t); }

void launch_cross_topk(Scope *scope, const TopkLaunch &t) {
    TopkArgs args{};
    args.a = t.a; args.b = t.b; args.k = t.k; args.slices = t.slices; args.slice_chunks = t.slice_chunks; args.cap = t.cap;
    args.prune = t.prune; args.partial = t.partial; args.indices = t.indices; args.distances = t.distances;
    args.partials = scope->plan_partials; args.done_counter = scope->done_counter; args.summary = scope->summary_target();
    const uint64_t items = ((t.a.count + kTopkQueries - 1) / kTopkQueries) * t.slices;
    const uint64_t blocks64 = (items + kTopkWaves - 1) / kTopkWaves;
    uint32_t max_blocks = (uint32_t)scope->compute_units * 8;
    if (max_blocks > (uint32_t)kMaxPartials) max_blocks = kMaxPartials;
    const uint32_t blocks = blocks64 > max_blocks ? max_blocks : (uint32_t)(blocks64 ? blocks64 : 1);
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
