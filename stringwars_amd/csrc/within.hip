// within.hip -- Levenshtein range search: for every query EVERY candidate with d <= bound, as CSR rows of unknown length
// (swh_levenshtein_within_*, include/stringwars_amd.h). Top-k (topk.hip) folds a walk's distances into a list of k; a range search
// compacts them: rows in candidate order, no sort, no atomics on the output, the same bits on every run.
//
// Every path walks the pairs twice. The count pass leaves hit counts, an exclusive scan turns them into starts and row offsets, the
// host reads the total (8 bytes) and -- only if the caller's arrays hold it -- the fill pass repeats the walk and stores each hit at
// its row's cursor: a wave's 64 distances give one ballot, a hit's place is the cursor plus the hits in the lanes below it.
//
// Kernels:
//   k_cross_within<Off, Fill>  word-sized byte strings (<= 32 bytes, unit costs: the calls top-k serves with k_cross_topk). The work item,
//                              the 16 match tables in LDS and the column walk are k_cross_topk's; the lists are gone. A chunk with no
//                              lane at |m - n| <= bound is skipped in both passes (d >= |m - n|; the bound is fixed, so the test never
//                              loosens the way top-k's threshold does). Lane q keeps query q's count (Fill = false) or cursor (true).
//   k_within_sums,             the scan of counts[row][slice], row-major: per-tile sums, then every tile adds up the sums before it
//   k_within_offsets           and scans itself. Two plain launches: no workgroup waits for another.
//   k_within_count,            the general path: one wave per row of a slice of a dense u32 matrix (scored by the ordinary
//   k_within_fill              cross-product routes into scratch). Slices run in stream order, so a row's cursor meets its candidates
//                              in ascending order.
#include "within.hpp"
#include "bp_lanes.hpp"   // the offset reader, lds_order, readlane64

#include <algorithm>

namespace swh {

constexpr uint32_t kWithinLongest = 32;   // longest query / candidate of the fused kernel, bytes
constexpr int kWithinQueries = 16;        // queries per work item
constexpr int kWithinWaves = 4;

struct WithinArgs {
    TapeRef a, b;              // queries, candidates: device byte tapes
    uint32_t slices, bound;    // candidate slices per query block; hits have d <= bound
    uint64_t slice_chunks;     // chunks of 64 candidates per slice
    uint32_t prune;            // skip a query's chunk when no lane has |m - n| <= bound
    uint32_t *counts;          // Fill = false: [query][slice], out
    const uint64_t *starts;    // Fill = true: [query][slice], where the item's hits of that query begin
    uint64_t total;            // Fill = true: entries the outputs hold
    uint32_t *indices, *distances;
    PlanPartial *partials;
    uint32_t *done_counter;
    CallSummary *summary;
};

struct WithinWaveLds {
    uint32_t table[kWithinQueries][32];   // Lo[16] | Hi[16] of each query of the item
    uint32_t qlen[kWithinQueries];
};

template <typename Off, bool Fill>
__global__ __launch_bounds__(kWithinWaves * 64, 4) void k_cross_within(WithinArgs args) {
    __shared__ WithinWaveLds wave_lds[kWithinWaves];
    __shared__ SummaryLds summary_lds;
    __shared__ unsigned long long lcells, lsyms;
    __shared__ uint32_t lmaxa, lmaxb, lshorts, lmisfit;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    WithinWaveLds &wl = wave_lds[wave];
    if (threadIdx.x == 0) { lcells = 0; lsyms = 0; lmaxa = 0; lmaxb = 0; lshorts = 0; lmisfit = 0; }
    __syncthreads();
    const uint64_t na = args.a.count, nb = args.b.count;
    const uint8_t *a_data = (const uint8_t *)args.a.data, *b_data = (const uint8_t *)args.b.data;
    const uint64_t b_total = (uint64_t)((const Off *)args.b.offsets)[nb];
    const uint64_t chunks = (nb + 63) / 64, qblocks = (na + kWithinQueries - 1) / kWithinQueries;
    const uint64_t items = qblocks * args.slices;
    const uint64_t waves_total = (uint64_t)gridDim.x * kWithinWaves, wave_id = (uint64_t)blockIdx.x * kWithinWaves + wave;
    const uint64_t lanes_below = (1ull << lane) - 1ull;
    const uint32_t bound = args.bound;
    unsigned long long cells = 0, syms = 0;
    uint32_t maxa = 0, maxb = 0, shorts = 0, misfit = 0;

    for (uint64_t item = wave_id; item < items; item += waves_total) {
        // neighbouring waves take neighbouring query blocks of one slice: the slice's candidates stay warm in the cache
        const uint64_t slice = item / qblocks, qb = item - slice * qblocks;
        const uint64_t q_first = qb * kWithinQueries, q_last = q_first + kWithinQueries < na ? q_first + kWithinQueries : na;
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
            staged[t] = (at < qm && qm <= kWithinLongest) ? a_data[qa0 + at] : 0u;
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) (&wl.table[0][0])[lane * 8 + t] = 0;
        lds_order();
        if (part == 0) wl.qlen[ql] = ql < q_count ? qm : 0u;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t at = part * 8 + (uint32_t)t;
            if (at < qm && qm <= kWithinLongest) {
                atomicOr(&wl.table[ql][staged[t] & 15u], 1u << at);
                atomicOr(&wl.table[ql][16 + (staged[t] >> 4)], 1u << at);
            }
        }
        if (ql < q_count && qm > kWithinLongest) misfit = 1;
        lds_order();
        unsigned long long sum_m = 0;
        uint32_t item_maxa = 0;
        for (uint32_t q = 0; q < q_count; ++q) {
            const uint32_t m = (uint32_t)__builtin_amdgcn_readfirstlane((int)wl.qlen[q]);
            sum_m += m;
            item_maxa = m > item_maxa ? m : item_maxa;
        }
        // lane q: query q's hits so far in this item (count pass), or where its next hit goes (fill pass)
        uint32_t running = 0;
        uint64_t cursor = 0;
        if constexpr (Fill) {
            if ((uint32_t)lane < q_count) cursor = args.starts[(q_first + (uint64_t)lane) * args.slices + slice];
        }
        // ---- the slice's chunks of 64 candidates --------------------------------------------------------------------------------
        const uint64_t c_first = slice * args.slice_chunks;
        const uint64_t c_last = c_first + args.slice_chunks < chunks ? c_first + args.slice_chunks : chunks;
        for (uint64_t chunk = c_first; chunk < c_last; ++chunk) {
            const uint64_t cand = chunk * 64 + (uint64_t)lane;
            const bool have = cand < nb;
            uint64_t b0 = 0;
            uint32_t n = 0;
            if (have) tape_extent<Off>(args.b.offsets, cand, b0, n);
            const bool fits = have && n <= kWithinLongest;
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
                if (m > kWithinLongest) continue;
                if (args.prune) {
                    const uint32_t gap = m > n ? m - n : n - m;
                    if (!__ballot(fits && gap <= bound)) continue;
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
                const bool hit = fits && d <= bound;
                const uint64_t hits = __ballot(hit);
                if (!hits) continue;
                const uint32_t fresh = (uint32_t)__popcll(hits);
                if constexpr (Fill) {
                    const uint64_t at = readlane64(cursor, (int)q) + (uint64_t)__popcll(hits & lanes_below);
                    if (hit && at < args.total) {   // (a total the walk outgrows: the tapes changed between the passes -- never past the arrays)
                        args.indices[at] = (uint32_t)cand;
                        args.distances[at] = d;
                    }
                    if ((uint32_t)lane == q) cursor += fresh;
                } else {
                    if ((uint32_t)lane == q) running += fresh;
                }
            }
            if constexpr (!Fill) {
                if (have) {
                    cells += sum_m * (unsigned long long)n;
                    maxb = n > maxb ? n : maxb;
                    if (qb == 0) syms += n;                            // every candidate once ...
                    if (fits) shorts += q_count;
                }
            }
        }
        if constexpr (!Fill) {
            if (lane == 0) {
                maxa = item_maxa > maxa ? item_maxa : maxa;
                if (slice == 0) syms += sum_m;                         // ... and every query once
            }
            if ((uint32_t)lane < q_count) args.counts[(q_first + (uint64_t)lane) * args.slices + slice] = running;
        }
        lds_order();   // the next item's tables are not cleared under this item's last reads
    }
    if constexpr (Fill) return;
    // ---- summary (count pass: the call's cells and lengths are counted once) ----------------------------------------------------
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

// ---- the scan of the counts --------------------------------------------------------------------------------------------------------
constexpr int kWithinScanThreads = 256;
constexpr int kWithinScanPerThread = (int)(kWithinScanTile / kWithinScanThreads);   // 16 consecutive counts per thread

__device__ __forceinline__ uint64_t within_block_sum(unsigned long long v, uint64_t *wave_sums) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
    __syncthreads();
    return wave_sums[0] + wave_sums[1] + wave_sums[2] + wave_sums[3];
}

__global__ __launch_bounds__(kWithinScanThreads) void k_within_sums(const uint32_t *counts, uint64_t n, uint64_t *block_sums) {
    __shared__ uint64_t wave_sums[4];
    const uint64_t first = (uint64_t)blockIdx.x * kWithinScanTile + (uint64_t)threadIdx.x * kWithinScanPerThread;
    uint64_t mine = 0;
#pragma unroll
    for (int j = 0; j < kWithinScanPerThread; ++j) mine += first + j < n ? counts[first + j] : 0u;
    const uint64_t sum = within_block_sum(mine, wave_sums);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = sum;
}

// Tile t: the sums of the tiles before it, then its own exclusive scan. starts[i] for every count; row_offsets[r] = starts[r * slices]
// and row_offsets[rows] = the total, written by whoever holds count n - 1.
__global__ __launch_bounds__(kWithinScanThreads) void k_within_offsets(const uint32_t *counts, uint64_t n, uint32_t slices, const uint64_t *block_sums,
                                                                         uint64_t *starts, uint64_t *row_offsets) {
    __shared__ uint64_t wave_sums[4];
    __shared__ uint64_t wave_scan[4];
    uint64_t before = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += kWithinScanThreads) before += block_sums[b];
    const uint64_t base = within_block_sum(before, wave_sums);
    const uint64_t first = (uint64_t)blockIdx.x * kWithinScanTile + (uint64_t)threadIdx.x * kWithinScanPerThread;
    uint32_t c[kWithinScanPerThread];
    uint64_t mine = 0;
#pragma unroll
    for (int j = 0; j < kWithinScanPerThread; ++j) {
        c[j] = first + j < n ? counts[first + j] : 0u;
        mine += c[j];
    }
    // exclusive scan of the threads' sums: within the wave by shuffles, across the four waves through LDS
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long other = __shfl_up(incl, off);
        if (lane >= (uint32_t)off) incl += other;
    }
    if (lane == 63) wave_scan[wave] = incl;
    __syncthreads();
    uint64_t at = base + incl - mine;
    for (uint32_t w = 0; w < wave; ++w) at += wave_scan[w];
#pragma unroll
    for (int j = 0; j < kWithinScanPerThread; ++j) {
        const uint64_t i = first + j;
        if (i < n) {
            starts[i] = at;
            if (slices == 1) row_offsets[i] = at;
            else if (i % slices == 0) row_offsets[i / slices] = at;
            if (i == n - 1) row_offsets[n / slices] = at + c[j];
        }
        at += c[j];
    }
}

// ---- the general path's sweeps -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWithinWaves * 64) void k_within_count(const uint32_t *scores, uint64_t rows, uint64_t columns, uint32_t bound,
                                                                     uint32_t *counts) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t r = (uint64_t)blockIdx.x * kWithinWaves + wave; r < rows; r += (uint64_t)gridDim.x * kWithinWaves) {
        const uint32_t *row = scores + r * columns;
        uint32_t hits = 0;
        for (uint64_t c0 = 0; c0 < columns; c0 += 64) {
            const uint64_t c = c0 + lane;
            hits += (uint32_t)__popcll(__ballot(c < columns && row[c] <= bound));
        }
        if (lane == 0) counts[r] += hits;   // (one wave per row, slices in stream order: no other writer)
    }
}

__global__ __launch_bounds__(kWithinWaves * 64) void k_within_fill(const uint32_t *scores, uint64_t rows, uint64_t columns, uint64_t col_first,
                                                                    uint32_t bound, uint64_t *cursors, uint64_t total, uint32_t *indices,
                                                                    uint32_t *distances) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t lanes_below = (1ull << lane) - 1ull;
    for (uint64_t r = (uint64_t)blockIdx.x * kWithinWaves + wave; r < rows; r += (uint64_t)gridDim.x * kWithinWaves) {
        const uint32_t *row = scores + r * columns;
        uint64_t cursor = cursors[r];
        for (uint64_t c0 = 0; c0 < columns; c0 += 64) {
            const uint64_t c = c0 + lane;
            const uint32_t score = c < columns ? row[c] : 0u;
            const bool hit = c < columns && score <= bound;
            const uint64_t hits = __ballot(hit);
            const uint64_t at = cursor + (uint64_t)__popcll(hits & lanes_below);
            if (hit && at < total) {
                indices[at] = (uint32_t)(col_first + c);
                distances[at] = score;
            }
            cursor += (uint64_t)__popcll(hits);
        }
        if (lane == 0) cursors[r] = cursor;
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
void launch_cross_within(Scope *scope, const WithinLaunch &w, bool fill) {
    WithinArgs args{};
    args.a = w.a; args.b = w.b; args.slices = w.slices; args.bound = w.bound; args.slice_chunks = w.slice_chunks; args.prune = w.prune;
    args.counts = w.counts; args.starts = w.starts; args.total = w.total; args.indices = w.indices; args.distances = w.distances;
    args.partials = scope->plan_partials; args.done_counter = scope->done_counter; args.summary = scope->summary_target();
    const uint64_t items = ((w.a.count + kWithinQueries - 1) / kWithinQueries) * w.slices;
    const uint64_t blocks64 = (items + kWithinWaves - 1) / kWithinWaves;
    uint32_t max_blocks = (uint32_t)scope->compute_units * 8;
    if (max_blocks > (uint32_t)kMaxPartials) max_blocks = kMaxPartials;
    const uint32_t blocks = blocks64 > max_blocks ? max_blocks : (uint32_t)(blocks64 ? blocks64 : 1);
    StampGuard guard(scope, "cross_within");
    const dim3 grid(blocks), block(kWithinWaves * 64);
    if (w.off64) {
        if (fill) hipLaunchKernelGGL((k_cross_within<uint64_t, true>), grid, block, 0, scope->stream, args);
        else hipLaunchKernelGGL((k_cross_within<uint64_t, false>), grid, block, 0, scope->stream, args);
    } else {
        if (fill) hipLaunchKernelGGL((k_cross_within<uint32_t, true>), grid, block, 0, scope->stream, args);
        else hipLaunchKernelGGL((k_cross_within<uint32_t, false>), grid, block, 0, scope->stream, args);
    }
    SWH_HIP_CHECK(hipGetLastError());
}

void launch_within_offsets(Scope *scope, const uint32_t *counts, uint64_t rows, uint32_t slices, uint64_t *block_sums, uint64_t *starts,
                           uint64_t *row_offsets) {
    const uint64_t n = rows * slices;
    const uint32_t blocks = (uint32_t)((n + kWithinScanTile - 1) / kWithinScanTile);
    {
        StampGuard guard(scope, "within_sums");
        hipLaunchKernelGGL(k_within_sums, dim3(blocks), dim3(kWithinScanThreads), 0, scope->stream, counts, n, block_sums);
        SWH_HIP_CHECK(hipGetLastError());
    }
    StampGuard guard(scope, "within_offsets");
    hipLaunchKernelGGL(k_within_offsets, dim3(blocks), dim3(kWithinScanThreads), 0, scope->stream, counts, n, slices, (const uint64_t *)block_sums,
                       starts, row_offsets);
    SWH_HIP_CHECK(hipGetLastError());
}

static uint32_t within_row_blocks(const Scope *scope, uint64_t rows) {
    const uint64_t blocks = std::min<uint64_t>((rows + kWithinWaves - 1) / kWithinWaves, (uint64_t)scope->compute_units * 16);
    return (uint32_t)(blocks ? blocks : 1);
}

void launch_within_count(Scope *scope, const uint32_t *scores, uint64_t rows, uint64_t columns, uint32_t bound, uint32_t *counts) {
    StampGuard guard(scope, "within_count");
    hipLaunchKernelGGL(k_within_count, dim3(within_row_blocks(scope, rows)), dim3(kWithinWaves * 64), 0, scope->stream, scores, rows, columns, bound,
                       counts);
    SWH_HIP_CHECK(hipGetLastError());
}

void launch_within_fill(Scope *scope, const uint32_t *scores, uint64_t rows, uint64_t columns, uint64_t col_first, uint32_t bound,
                        uint64_t *cursors, uint64_t total, uint32_t *indices, uint32_t *distances) {
    StampGuard guard(scope, "within_fill");
    hipLaunchKernelGGL(k_within_fill, dim3(within_row_blocks(scope, rows)), dim3(kWithinWaves * 64), 0, scope->stream, scores, rows, columns,
                       col_first, bound, cursors, total, indices, distances);
    SWH_HIP_CHECK(hipGetLastError());
}

}  // namespace swh
