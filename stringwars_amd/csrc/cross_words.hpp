// cross_words.hpp -- what the kernels share that score word-sized byte strings (at most 32 bytes, unit costs) as a cross-product:
// k_cross_short (the dense matrix; cross.hip explains the layout: 64 candidates in a wave's lanes, the query's match table once per
// wave in LDS), k_cross_topk (topk.hip) and k_cross_within (within.hip).
//
// Shared here: the constants, the offset reader, lds_order and readlane64 (also bp_lanes.hpp's and align.hip's), the grid of an item
// kernel (word_item_blocks), the summary tail (WordSummary), the staging of an item's queries (StagedQueries), the candidate window
// load (WordCandidate), the column walk with its distance (word_distance) and the item skeleton of the two fused searches
// (word_search_items). k_cross_short keeps its own item: one chunk, each table built while the query before it is walked.
#pragma once
#include "common.hpp"
#include "bp_window.hpp"

namespace swh {

constexpr uint32_t kWordLongest = 32;   // longest query / candidate, bytes
constexpr int kWordQueries = 16;        // queries per work item
constexpr int kWordWaves = 4;

// String i of a tape: where it starts and its (saturated, common.hpp) length.
template <typename Off>
__device__ __forceinline__ void tape_extent(const TapeRef &t, uint64_t i, uint64_t &start, uint32_t &len) {
    const Off *o = (const Off *)t.offsets;
    const Off x0 = o[i], x1 = o[i + 1];
    start = (uint64_t)x0;
    len = extent_length<Off>(x0, x1);
}
__device__ __forceinline__ void tape_extent(const TapeRef &t, uint32_t off64, uint64_t i, uint64_t &start, uint32_t &len) {
    if (off64) tape_extent<uint64_t>(t, i, start, len);
    else tape_extent<uint32_t>(t, i, start, len);
}

// Between LDS operations of ONE wave only program order has to be kept: a wave's DS instructions are queued and executed in issue
// order, so a table update (ds_or) followed by a look-up (ds_read) of another lane's word needs no wait in between -- the compiler
// just must not move the accesses across each other (it reasons per thread).
__device__ __forceinline__ void lds_order() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return (uint64_t)hi << 32 | lo;
}

// Workgroups of kWordWaves waves for `items` work items, one per wave and round: at most eight per compute unit and one per partial.
static inline uint32_t word_item_blocks(const Scope *scope, uint64_t items) {
    const uint64_t blocks = (items + kWordWaves - 1) / kWordWaves;
    uint32_t max_blocks = (uint32_t)scope->compute_units * 8;
    if (max_blocks > (uint32_t)kMaxPartials) max_blocks = kMaxPartials;
    return blocks > max_blocks ? max_blocks : (uint32_t)(blocks ? blocks : 1);
}

// ---- the summary tail: a call's work units (cells, symbols, short pairs), longest strings and the misfit bit, summed per lane, then
// per workgroup in LDS, then handed to report_call_summary. (tiled.hip and alignshort.hip keep copies of their own: their text is
// hashed into the committed counter constants, tools/kernel_sources.py.)
struct WordSummary {
    struct Lds {
        SummaryLds report;
        unsigned long long cells, syms;
        uint32_t maxa, maxb, shorts, misfit;
    };
    unsigned long long cells = 0, syms = 0;
    uint32_t maxa = 0, maxb = 0, shorts = 0, misfit = 0;   // misfit: a string longer than kWordLongest (the host redoes the call)

    __device__ __forceinline__ void init(Lds &lds) {
        if (threadIdx.x == 0) { lds.cells = 0; lds.syms = 0; lds.maxa = 0; lds.maxb = 0; lds.shorts = 0; lds.misfit = 0; }
        __syncthreads();
    }
    // my candidate (n symbols) against the item's q_count queries of sum_m symbols
    __device__ __forceinline__ void add_chunk(bool have, bool fits, uint32_t n, unsigned long long sum_m, uint32_t q_count, bool first_queries) {
        if (have) {
            cells += sum_m * (unsigned long long)n;
            maxb = n > maxb ? n : maxb;
            if (first_queries) syms += n;                              // every candidate once ...
            if (fits) shorts += q_count;
        }
    }
    __device__ __forceinline__ void add_item(int lane, uint32_t item_maxa, unsigned long long sum_m, bool first_candidates) {
        if (lane == 0) {
            maxa = item_maxa > maxa ? item_maxa : maxa;
            if (first_candidates) syms += sum_m;                       // ... and every query once (bench.rs:216-224)
        }
    }
    __device__ __forceinline__ void finish(int lane, Lds &lds, PlanPartial *partials, uint32_t *done_counter, CallSummary *summary) {
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
            atomicAdd(&lds.cells, cells);
            atomicAdd(&lds.syms, syms);
            atomicAdd(&lds.shorts, shorts);
            atomicMax(&lds.maxa, maxa);
            atomicMax(&lds.maxb, maxb);
            atomicOr(&lds.misfit, misfit);
        }
        __syncthreads();
        report_call_summary(PlanPartial{lds.cells, lds.syms, lds.maxa, lds.maxb, lds.shorts, lds.misfit}, partials, done_counter, summary, lds.report);
    }
};

// ---- my lane's share of an item's 16 queries, requested in one batch: symbols 8 (l % 4) .. 8 (l % 4) + 7 of query l / 4 (16 queries
// x 32 symbols = 64 lanes x 8; zeros past the query's end and for a query that does not fit). qm: that query's length.
template <typename Off, typename Sym>
struct StagedQueries {
    uint32_t ql, part, qm = 0, staged[8];
    __device__ __forceinline__ void load(const TapeRef &a, uint64_t q_first, uint32_t q_count, int lane) {
        ql = (uint32_t)lane >> 2, part = (uint32_t)lane & 3u;
        uint64_t qa0 = 0;
        if (ql < q_count) tape_extent<Off>(a, q_first + ql, qa0, qm);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t at = part * 8 + (uint32_t)t;
            staged[t] = (at < qm && qm <= kWordLongest) ? ((const Sym *)a.data)[qa0 + at] : 0u;
        }
    }
};

// ---- my lane's candidate of a chunk of 64: `locate` requests its extent, `fetch` its 32 bytes (tw[8], zero past the string: the
// 128-bit path, or the dword path on a tape too short for it). The two are apart so that a kernel can send other loads in between.
struct WordCandidate {
    uint64_t cand, b0 = 0;       // which, and where its bytes start
    uint32_t n = 0, n_live;      // its length; 0 for a lane whose columns are not walked
    bool have, fits;             // a candidate in this lane; of at most kWordLongest bytes
    uint32_t tw[8];

    template <typename Off>
    __device__ __forceinline__ void locate(const TapeRef &b, uint64_t slot) {
        cand = slot;   // (unconditional: a select here costs k_cross_topk, which has no register to spare, 2 % on 65 536 x 1 M words)
        have = slot < b.count;
        if (have) tape_extent<Off>(b, cand, b0, n);
    }
    __device__ __forceinline__ void fetch(const uint8_t *b_data, uint64_t b_total, uint32_t &misfit) {
        fits = have && n <= kWordLongest;
        if (have && !fits) misfit = 1;
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
        n_live = fits ? n : 0;
    }
};

// One column of Myers' recurrence on a 32-row word: eq = the rows that match the column's symbol, pv / mv = the vertical +1 / -1 deltas.
__device__ __forceinline__ void myers_column(uint32_t eq, uint32_t &pv, uint32_t &mv) {
    const uint32_t xv = eq | mv;
    const uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
    uint32_t ph = mv | ~(xh | pv);
    const uint32_t mh = pv & xh;
    ph = (ph << 1) | 1u;
    pv = (mh << 1) | ~(xv | ph);
    mv = ph & xv;
}

// ---- the column walk: the query of m <= 32 rows (`table`: its Lo[16] | Hi[16]) against my candidate's n columns, n_live of them
// walked (n_max: the wave's largest n_live). Returns the distance.
__device__ __forceinline__ uint32_t word_distance(const uint32_t *table, uint32_t m, const uint32_t (&tw)[8], uint32_t n_live, uint32_t n_max, uint32_t n) {
    uint32_t pv = 0xFFFFFFFFu, mv = 0;
#pragma unroll
    for (int w4 = 0; w4 < 8; ++w4) {
        if ((uint32_t)w4 * 4 >= n_max) break;
        const uint32_t w = tw[w4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            // Lo[c & 15] and Hi[c >> 4] as byte offsets: ((w >> 8u) & 15) << 2 and ((w >> (8u + 4)) & 15) << 2
            const uint32_t lo_at = (u == 0 ? (w << 2) : (w >> (8 * u - 2))) & 0x3Cu;
            const uint32_t hi_at = (w >> (8 * u + 2)) & 0x3Cu;
            const uint32_t eq = *(const uint32_t *)((const char *)table + lo_at) & *(const uint32_t *)((const char *)table + 64 + hi_at);
            if ((uint32_t)(w4 * 4 + u) < n_live) myers_column(eq, pv, mv);
        }
    }
    const uint32_t mask = m >= 32 ? 0xFFFFFFFFu : ((1u << m) - 1u);
    return n + __popc(pv & mask) - __popc(mv & mask);
}

// ---- the fused searches' item: 16 queries x one slice of the candidates. The 16 tables are built once per item and reused for every
// chunk of 64 candidates of the slice; neighbouring waves take neighbouring query blocks of one slice, so the slice's candidates
// stay warm in the cache.
struct WordSearchArgs {
    TapeRef a, b;              // queries, candidates: device byte tapes
    uint32_t slices, prune;    // candidate slices per query block; skip a query's chunk when the prune test fails in every lane
    uint64_t slice_chunks;     // chunks of 64 candidates per slice
    PlanPartial *partials;
    uint32_t *done_counter;
    CallSummary *summary;
};

struct WordSearchLds {
    struct Wave {
        uint32_t table[kWordQueries][32];   // Lo[16] | Hi[16] of each query of the item
        uint32_t qlen[kWordQueries];
    } wave[kWordWaves];
    WordSummary::Lds summary;
};

struct WordItem { uint64_t slice, q_first; uint32_t q_count; };   // its candidate slice, its first query and how many (<= 16)

// begin(item)           before the item's tables are built (its LDS writes are ordered with the table's clear)
// near(q, gap) -> bool  once per query and chunk, before the walk: can a lane with |m - n| = gap still matter to query q? (d >= |m - n|;
//                       with args.prune the walk is skipped when no lane can)
// score(q, c, d)        candidate c (WordCandidate) is at distance d from query q; c.fits says whether that counts
// end(item)             after the slice's last chunk; it ends with an lds_order(): the next item's clear stays behind its reads
// kCounts: the pass sums the call's work units and reports them (a second pass over the same pairs does not).
template <typename Off, bool kCounts, typename Begin, typename Near, typename Score, typename End>
__device__ __forceinline__ void word_search_items(const WordSearchArgs &args, WordSearchLds &lds, Begin &&begin, Near &&near, Score &&score, End &&end) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    WordSearchLds::Wave &wl = lds.wave[wave];
    WordSummary sum;
    sum.init(lds.summary);
    const uint64_t na = args.a.count, nb = args.b.count;
    const uint8_t *b_data = (const uint8_t *)args.b.data;
    const uint64_t b_total = (uint64_t)((const Off *)args.b.offsets)[nb];
    const uint64_t chunks = (nb + 63) / 64, qblocks = (na + kWordQueries - 1) / kWordQueries;
    const uint64_t items = qblocks * args.slices;
    const uint64_t waves_total = (uint64_t)gridDim.x * kWordWaves, wave_id = (uint64_t)blockIdx.x * kWordWaves + wave;
    for (uint64_t at = wave_id; at < items; at += waves_total) {
        const uint64_t slice = at / qblocks, qb = at - slice * qblocks, q_first = qb * kWordQueries;
        const uint32_t q_count = (uint32_t)((q_first + kWordQueries < na ? q_first + kWordQueries : na) - q_first);
        const WordItem item{slice, q_first, q_count};
        // ---- the item's 16 match tables ------------------------------------------------------------------------------------------
        StagedQueries<Off, uint8_t> sq;
        sq.load(args.a, q_first, q_count, lane);
        const uint32_t ql = sq.ql, part = sq.part, qm = sq.qm;
#pragma unroll
        for (int t = 0; t < 8; ++t) (&wl.table[0][0])[lane * 8 + t] = 0;
        begin(item);
        lds_order();
        if (part == 0) wl.qlen[ql] = ql < q_count ? qm : 0u;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t byte_at = part * 8 + (uint32_t)t;
            if (byte_at < qm && qm <= kWordLongest) {
                atomicOr(&wl.table[ql][sq.staged[t] & 15u], 1u << byte_at);
                atomicOr(&wl.table[ql][16 + (sq.staged[t] >> 4)], 1u << byte_at);
            }
        }
        if (ql < q_count && qm > kWordLongest) sum.misfit = 1;
        lds_order();
        unsigned long long sum_m = 0;
        uint32_t item_maxa = 0;
        for (uint32_t q = 0; q < q_count; ++q) {
            const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)wl.qlen[q]);
            sum_m += m;
            item_maxa = m > item_maxa ? m : item_maxa;
        }
        // ---- the slice's chunks of 64 candidates --------------------------------------------------------------------------------
        const uint64_t c_first = slice * args.slice_chunks;
        const uint64_t c_last = c_first + args.slice_chunks < chunks ? c_first + args.slice_chunks : chunks;
        for (uint64_t chunk = c_first; chunk < c_last; ++chunk) {
            WordCandidate c;
            c.locate<Off>(args.b, chunk * 64 + (uint64_t)lane);
            c.fetch(b_data, b_total, sum.misfit);
            const uint32_t n_max = wave_max_u32(c.n_live);
            for (uint32_t q = 0; q < q_count; ++q) {
                const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)wl.qlen[q]);
                if (m > kWordLongest) continue;
                const uint32_t gap = m > c.n ? m - c.n : c.n - m;
                const bool close = near(q, gap);
                if (args.prune && !__ballot(c.fits && close)) continue;
                score(q, c, word_distance(wl.table[q], m, c.tw, c.n_live, n_max, c.n));
            }
            if constexpr (kCounts) sum.add_chunk(c.have, c.fits, c.n, sum_m, q_count, qb == 0);
        }
        if constexpr (kCounts) sum.add_item(lane, item_maxa, sum_m, slice == 0);
        end(item);
    }
    if constexpr (kCounts) sum.finish(lane, lds.summary, args.partials, args.done_counter, args.summary);
}

}  // namespace swh
