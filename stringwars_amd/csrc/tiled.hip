// tiled.hip -- unit-cost Levenshtein without a planning pre-pass: every workgroup plans its own tile.
//
// The globally planned path (prepass.hip -> bitparallel.hip) spends three launches (histogram, scan, scatter), a
// permutation array and a round trip of the plan to the host before the first DP column is computed -- a third of a
// synchronous call on a 1 M-pair batch of tokens, nine tenths of it on 10 K words. Here a workgroup takes a TILE of
// consecutive pairs (<= 1024), and in LDS
//   B. classifies them: pattern side, G = blocks of 32 rows, text length n; finishes the trivial ones;
//   C. moves a class's few left-over pairs up into the next class when that saves a mostly empty work item;
//   D-F. counting-sorts the tile by (G, n bucket) into a u16 index list;
//   G. runs the work items of bp_item.hpp on it, longest first, waves taking items from an LDS ticket -- for a tile away from both ends
//      of both tapes (step B finds out) the item that reads its strings without clamping its windows into the tape.
// Pairs of one item are consecutive in the sorted tile, so the lanes of a wave finish together just as with the global
// sort; what is lost is one partly filled item per class and tile. What is gained: one launch per call, no host
// round trip, no permutation / key arrays in HBM, and results that land in a 4 KB window per tile instead of being
// scattered over the whole output.
//
// The kernel is exact for every pair whose pattern fits 64 blocks (2048 symbols). A longer pair raises the
// `violation` flag (host-mapped memory) and is left alone: the host only picks this kernel when tape statistics or the
// previous call say no such pair exists, checks the flag after the call and falls back to the planned path if it is
// set (api.hip).
#include <atomic>
#include <cstdio>
#include <cstdlib>

#include "api.hpp"   // launch_bitparallel_tiled_side
#include "bp_item.hpp"

namespace swh {

// Pairs per tile: 2048, and 4096 for the sixteen-wave workgroup that has a compute unit to itself (kIndexBits of an index-list
// entry, then 6 + 6 bits: common prefix / suffix). ONE tile per workgroup is what the sizes are for: a second round of tiles cost
// C2 12 % (tiles of 652 pairs in three rounds against 977 in two: 25.2 against 28.7 TCUPS), one round of 1954 gave 29.6.
constexpr int tile_index_bits(int waves) { return waves >= 16 ? 12 : 11; }
constexpr int tile_max(int waves) { return 1 << tile_index_bits(waves); }
constexpr uint32_t kAffixCap = 16; // symbols cut off at either end: what one 16-byte window shows
constexpr int kTileBuckets = 32;   // text-length buckets per class
constexpr int kTileClasses = 64;
constexpr int kTileBins = kTileClasses * kTileBuckets;

// Waves per workgroup. The hardware favours a compute unit's oldest workgroups, so the youngest run the last part of
// their tile alone: with four-wave workgroups that is ONE wave per SIMD, and a wave of this serial recurrence issues at
// half rate on its own (C2: the four workgroups of a CU finish at 105 / 150 / 190 / 235 us of a 260 us profiled launch,
// tools/tile_spans.py). Eight-wave workgroups (two per CU, two tiles each) leave two waves per SIMD in that tail: -6 % for
// a launch on its own (C2 synchronous: 22.95 -> 24.1-24.6 TCUPS); overlapping launches of two pipeline lanes, where the
// other launch fills the tail anyway, measure the same with either (27.7-28.2 TCUPS). Round 4 took the step after that: ONE
// sixteen-wave workgroup per compute unit with one tile of up to 4096 pairs (160 KB of LDS: sixteen 8.25 KB tables, the tile's
// 16 KB index list, 8 KB of counters / staged distances) -- sixteen waves on one ticket finish together: 29.6 -> 31.1 TCUPS.
template <int kTileMax>
struct TileLds {
    uint32_t sorted[kTileMax];            // tile-local pair indices (| prefix << kIndexBits | suffix << (kIndexBits + 6) | "a is the pattern" << (kIndexBits + 12)), sorted by (class, text-length bucket)
    uint32_t bins[kTileBins / 2 > kTileMax / 2 ? kTileBins / 2 : kTileMax / 2];   // two u16 counters per word: counts, then exclusive prefixes; later a tile's distances, 16 bits each
    uint32_t class_count[kTileClasses];   // pairs per natural class; after step C: per final class
    uint16_t class_thr[kTileClasses];     // ranks >= thr move up to class_tgt
    uint16_t class_tgt[kTileClasses];     // after step F: floor(65535 / G) of class G - 1 (lane_over())
    uint32_t item_prefix[kTileClasses + 1];
    union {
        uint32_t wave_sums[16];           // step E
        struct { unsigned long long lo_a, hi_a, lo_b, hi_b; } span;   // steps A - B: the bytes of either tape this tile's strings lie in
    };
    uint32_t ticket;
};
static_assert(sizeof(TileLds<4096>::span) <= sizeof(TileLds<4096>::wave_sums), "the tile's span borrows the scan's wave sums");

// x / G for x <= 64 and a wave-uniform G in 1 .. 64 without a division: ceil(2^16 / G) = floor(65535 / G) + 1 as a 16-bit magic (the
// table entry is the floor: G = 1 would not fit otherwise), exact because x (magic - 2^16 / G) < 65 < 2^16 / G.
__host__ __device__ constexpr uint32_t lane_over(uint32_t x, uint32_t floor_magic) { return (x * floor_magic + x) >> 16; }
constexpr bool lane_over_is_exact() {
    for (uint32_t g = 1; g <= 64; ++g)
        for (uint32_t x = 0; x <= 64; ++x)
            if (lane_over(x, 65535u / g) != x / g) return false;
    return true;
}
static_assert(lane_over_is_exact(), "lane / G and 64 / G by multiplication");

struct TileTail {   // after the last tile the counters' space serves the call summary
    unsigned long long cells, syms;
    uint32_t maxa, maxb, shorts, misfit;
    SummaryLds summary;
};
static_assert(sizeof(TileTail) <= sizeof(uint32_t) * kTileBins / 2, "the tail reuses TileLds::bins");

template <typename Sym, int kWaves> constexpr size_t tiled_lds_bytes() {
    return (size_t)kWaves * (bp_table_words<Sym>() + 64) * 4 + sizeof(TileLds<tile_max(kWaves)>);
}

#if defined(SWH_TILE_PROFILE) || defined(SWH_TILE_SPANS)
// Diagnostic builds only. make EXTRA=-DSWH_TILE_SPANS: four time stamps per workgroup of k_bitparallel_tiled, taken by its first thread
// (tools/tile_spans.py) -- close to the shipped kernel's time. EXTRA=-DSWH_TILE_PROFILE: those, and wave cycles per phase summed over
// the waves (tools/tile_phases.py), which make the kernel several times slower.
__device__ unsigned long long g_tile_span[2048][4];   // per workgroup: start, end of planning, end of items, end (100 MHz clock)
extern "C" void swh_debug_tile_spans(unsigned long long *out) {
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tile_span), sizeof(unsigned long long) * 2048 * 4);
}
#define TILE_SPAN(slot) do { if (threadIdx.x == 0) g_tile_span[blockIdx.x][slot] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define TILE_SPAN(slot) do {} while (0)
#endif
#ifdef SWH_TILE_PROFILE
__device__ unsigned long long g_tile_phase[8];
extern "C" void swh_debug_tile_phases(unsigned long long *out) {
    unsigned long long zero[8] = {};
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tile_phase), sizeof(zero));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_tile_phase), zero, sizeof(zero));
}
#define TILE_STAMP(slot) do { const unsigned long long now__ = __builtin_readcyclecounter(); phase_acc[slot] += now__ - phase_t; phase_t = now__; } while (0)
#else
#define TILE_STAMP(slot) do {} while (0)
#endif

#ifdef SWH_TEST_HOOKS
// Test library only: how often this process chose k_bitparallel_tiled_side, so that a test sees which kernel its call ran on.
static std::atomic<unsigned long long> g_tiled_side_launches{0};
extern "C" unsigned long long swh_debug_tiled_side_launches() { return g_tiled_side_launches.load(); }
#endif

struct TiledArgs {
    KernelArgs k;
    uint32_t tile;          // pairs per tile
    uint32_t tiles;
    uint32_t shift;         // text-length bucket = min(n >> shift, kTileBuckets - 1)
    uint32_t cut_affixes;   // byte strings: cut what a pair shares at both ends before classifying it
    uint32_t no_interior;   // comparison knob: every tile runs the clamped item
    PlanPartial *partials;  // per-workgroup work-unit sums (cells, symbols, maxima, "met a pair that does not fit")
    uint32_t *done_counter;
    CallSummary *summary;   // host-mapped: the last workgroup reports (common.hpp: report_call_summary)
    const uint4 *side_a, *side_b;   // kSide: per string its first and its last sixteen bytes (api.hip: k_tape_side), already moved to the views' first strings
};

// kPlain: the launch's shape is known when the kernel is compiled -- 32-bit offsets, pairwise, unbounded (what launch_tiled_sym sends
// there) -- so the per-pair tests of offset width, cross-product split and bound fold away.
// kSide (only with kPlain, on wide byte tapes): both tapes are prepared ones that carry side arrays, and step B takes a pair's windows from
// them -- entries 2 p and 2 p + 1 of either array, addressed by the pair's index like its offsets, so that nothing step B loads depends
// on anything it loaded before: everything a thread needs is requested at the very top of the tile, above the table clear and step A's
// barrier. Positions of a window that lie outside the tape read as zero there; only positions inside BOTH strings count (the clamps
// to min(la, lb)), so no pair needs the `inside` exception.
template <typename Sym, int kWaves, bool kWide, bool kPlain = false, bool kSide = false>
__device__ __forceinline__ void tiled_run(const TiledArgs &targs, char *smem, const uint64_t a_total, const uint64_t b_total) {
    constexpr int kThreads = kWaves * 64, kTableWords = bp_table_words<Sym>();
    // pairs per thread and tile, rounded UP: ten-wave workgroups (code points) have 640 threads, and 1024 / 640 = 1 left the
    // pairs 640 .. 1023 of a full tile unclassified (every use below is guarded by idx < count)
    constexpr int kTileMax = tile_max(kWaves), kTileIndexBits = tile_index_bits(kWaves);
    constexpr int kPer = (kTileMax + kThreads - 1) / kThreads;
    // tiles away from the tapes' ends run the unclamped item (not the four-wave workgroup, a test shape that holds eight pairs per
    // thread while it classifies: the extents' four registers would make it spill)
    constexpr bool kInteriorTiles = sizeof(Sym) == 1 && kWide && kWaves >= 8;
    [[maybe_unused]] KernelArgs shaped;
    const KernelArgs *shaped_or_sent = &targs.k;
    if constexpr (kPlain) {
        shaped = targs.k;
        shaped.off64 = 0; shaped.job.cross = 0; shaped.job.bound = 0xFFFFFFFFu;
        shaped_or_sent = &shaped;
    }
    const KernelArgs &args = *shaped_or_sent;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    static_assert(!kSide || (kPlain && kWide && sizeof(Sym) == 1), "side arrays: the headline shape only");
    BpWave<Sym> wv;
    const auto init_tables = [&] {
        wv.init((uint32_t *)smem + (size_t)wave * kTableWords, (uint32_t *)smem + (size_t)kWaves * kTableWords + wave * 64, lane,
                a_total, b_total);
    };
    if constexpr (!kSide) init_tables();   // (kSide: under the first tile's loads)
    TileLds<kTileMax> &tl = *(TileLds<kTileMax> *)(smem + (size_t)kWaves * (kTableWords + 64) * 4);
    unsigned long long cells = 0, syms = 0;
    uint32_t maxa = 0, maxb = 0, shorts = 0, misfit = 0;
#ifdef SWH_TILE_PROFILE
    unsigned long long phase_acc[4] = {0, 0, 0, 0}, phase_t = __builtin_readcyclecounter(), items_done = 0;
#endif
    TILE_SPAN(0);

    for (uint32_t tile = blockIdx.x; tile < targs.tiles; tile += gridDim.x) {
        const uint64_t base = (uint64_t)tile * targs.tile;
        const uint32_t count = (uint32_t)(args.job.pairs - base < targs.tile ? args.job.pairs - base : targs.tile);
        // (two pairs per thread at a time: a pair's four 16-byte windows are 16 registers while they are in flight)
#ifndef SWH_TILE_BATCH
#define SWH_TILE_BATCH 2
#endif
        constexpr int kBatch = kPer < SWH_TILE_BATCH ? kPer : SWH_TILE_BATCH;
        static_assert(kPer % kBatch == 0, "pairs per thread come in whole batches");
        // (kSide) what step B reads of a batch -- four offsets and four windows per pair, all of them addressed by the pair's index -- is
        // requested here, before anything else, for the first batch, and for the next one as soon as a batch's windows have been used
        // (all four pairs' windows at once made the kernel spill, as they did on the other path)
        constexpr int kBatchSide = kSide ? kBatch : 1;
        [[maybe_unused]] uint32_t side_off[kBatchSide][4];
        [[maybe_unused]] uint4 side_win[kBatchSide][4];
        [[maybe_unused]] const auto request_side = [&](int kb) {
            // (the tile's own bases, wave-uniform, and 32-bit indices into the tile: no address takes a register pair)
            const uint32_t *oa = (const uint32_t *)args.job.a.offsets + base, *ob = (const uint32_t *)args.job.b.offsets + base;
            const uint4 *sa = targs.side_a + 2 * base, *sb = targs.side_b + 2 * base;
#pragma unroll
            for (int j = 0; j < kBatchSide; ++j) {
                const uint32_t idx = (uint32_t)(kb + j) * kThreads + threadIdx.x, at = idx < count ? idx : count - 1;
                const uint32_t *xa = (const uint32_t *)((const char *)oa + at * 4u), *xb = (const uint32_t *)((const char *)ob + at * 4u);
                const uint4 *wa = (const uint4 *)((const char *)sa + at * 32u), *wb = (const uint4 *)((const char *)sb + at * 32u);
                side_off[j][0] = xa[0]; side_off[j][1] = xa[1]; side_off[j][2] = xb[0]; side_off[j][3] = xb[1];
                side_win[j][0] = wa[0]; side_win[j][1] = wa[1]; side_win[j][2] = wb[0]; side_win[j][3] = wb[1];
            }
        };
        if constexpr (kSide) {
            request_side(0);
            if (tile == blockIdx.x) init_tables();
        }
        // ---- A: clear the counters ------------------------------------------------------------------------------
        __builtin_amdgcn_s_setprio(3);   // planning is a chain of round trips and barriers: it goes first, the work items of other workgroups fill the gaps
        for (int i = threadIdx.x; i < kTileBins / 2; i += kThreads) tl.bins[i] = 0;
        if (threadIdx.x < kTileClasses) tl.class_count[threadIdx.x] = 0;
        if (threadIdx.x == 0) { tl.ticket = 0; tl.span.lo_a = tl.span.lo_b = ~0ull; tl.span.hi_a = tl.span.hi_b = 0; }
        __syncthreads();
        // ---- B: classify my pairs ---------------------------------------------------------------------------------
        // Every load a thread needs here is requested in two batches (indices clamped into the batch, no branch between the
        // loads): the extents of its pairs, then -- byte strings -- the first and last sixteen bytes of both strings of every
        // pair. What a pair shares at both ends is cut off before it is classified (the first thing rapidfuzz's Levenshtein
        // does, too): up to kAffixCap symbols each, kept in the upper bits of the pair's entry in the tile's index list.
        uint32_t cls[kPer], txt[kPer], rank[kPer], affix[kPer];
        using Ext = std::conditional_t<kSide, uint32_t, unsigned long long>;   // (kSide's offsets are 32-bit ones: half the registers)
        [[maybe_unused]] Ext lo_a = (Ext)~0ull, hi_a = 0, lo_b = (Ext)~0ull, hi_b = 0;   // where my pairs' strings lie (whole strings, affixes included)
#pragma unroll
        for (int kb = 0; kb < kPer; kb += kBatch) {
        std::conditional_t<kSide, uint32_t, uint64_t> a0s[kBatch], b0s[kBatch];
        uint32_t las[kBatch], lbs[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const int k = kb + j;
            const uint64_t p = base + (uint32_t)k * kThreads + threadIdx.x;
            const uint64_t pc = p < args.job.pairs ? p : args.job.pairs - 1;
            if constexpr (kSide) {
                a0s[j] = side_off[j][0]; las[j] = side_off[j][1] - side_off[j][0];
                b0s[j] = side_off[j][2]; lbs[j] = side_off[j][3] - side_off[j][2];
            }
            else if (args.off64) pair_extent<uint64_t, true>(args.job, pc, a0s[j], las[j], b0s[j], lbs[j]);
            else pair_extent<uint32_t, true>(args.job, pc, a0s[j], las[j], b0s[j], lbs[j]);
            affix[k] = 0;
        }
        if constexpr (sizeof(Sym) == 1 && kWide) {
            if (targs.cut_affixes) {
                uint4 ha[kBatch], hb[kBatch], ta[kBatch], tb[kBatch];
                bool inside[kBatch];
#pragma unroll
                for (int j = 0; j < kBatch; ++j) {
                    if constexpr (kSide) {
                        inside[j] = true;
                        ha[j] = side_win[j][0]; ta[j] = side_win[j][1]; hb[j] = side_win[j][2]; tb[j] = side_win[j][3];
                        continue;
                    }
                    // windows that would leave the tapes (the first / last strings) are read at the tapes' start and not used
                    const uint64_t ea = a0s[j] + las[j], eb = b0s[j] + lbs[j];
                    inside[j] = a0s[j] + 16 <= a_total && b0s[j] + 16 <= b_total && ea >= 16 && eb >= 16;
                    const uint8_t *ad = (const uint8_t *)args.job.a.data, *bd = (const uint8_t *)args.job.b.data;
                    __builtin_memcpy(&ha[j], ad + (inside[j] ? a0s[j] : 0), 16);
                    __builtin_memcpy(&hb[j], bd + (inside[j] ? b0s[j] : 0), 16);
                    __builtin_memcpy(&ta[j], ad + (inside[j] ? ea - 16 : 0), 16);
                    __builtin_memcpy(&tb[j], bd + (inside[j] ? eb - 16 : 0), 16);
                }
#pragma unroll
                for (int j = 0; j < kBatch; ++j) {
                    const uint32_t mn = las[j] < lbs[j] ? las[j] : lbs[j];
                    const unsigned long long h_lo = (unsigned long long)(ha[j].x ^ hb[j].x) | ((unsigned long long)(ha[j].y ^ hb[j].y) << 32);
                    const unsigned long long h_hi = (unsigned long long)(ha[j].z ^ hb[j].z) | ((unsigned long long)(ha[j].w ^ hb[j].w) << 32);
                    const unsigned long long t_lo = (unsigned long long)(ta[j].x ^ tb[j].x) | ((unsigned long long)(ta[j].y ^ tb[j].y) << 32);
                    const unsigned long long t_hi = (unsigned long long)(ta[j].z ^ tb[j].z) | ((unsigned long long)(ta[j].w ^ tb[j].w) << 32);
                    uint32_t pre = h_lo ? (uint32_t)__builtin_ctzll(h_lo) >> 3 : (h_hi ? 8u + ((uint32_t)__builtin_ctzll(h_hi) >> 3) : kAffixCap);
                    pre = pre < mn ? pre : mn;
                    uint32_t suf = t_hi ? (uint32_t)__builtin_clzll(t_hi) >> 3 : (t_lo ? 8u + ((uint32_t)__builtin_clzll(t_lo) >> 3) : kAffixCap);
                    suf = suf < mn - pre ? suf : mn - pre;
                    affix[kb + j] = inside[j] ? pre | (suf << 6) : 0u;
                }
            }
        }
        if constexpr (kSide) {
            if (kb + kBatch < kPer) request_side(kb + kBatch);   // under this batch's class counters
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const int k = kb + j;
            const uint32_t idx = (uint32_t)k * kThreads + threadIdx.x;
            cls[k] = 0xFFu; txt[k] = 0; rank[k] = 0;
            if (idx < count) {
                const uint64_t p = base + idx;
                uint32_t la = las[j], lb = lbs[j];
                if constexpr (kInteriorTiles) {
                    lo_a = a0s[j] < lo_a ? a0s[j] : lo_a; hi_a = a0s[j] + la > hi_a ? a0s[j] + la : hi_a;
                    lo_b = b0s[j] < lo_b ? b0s[j] : lo_b; hi_b = b0s[j] + lb > hi_b ? b0s[j] + lb : hi_b;
                }
                cells += (unsigned long long)la * lb;
                syms += (unsigned long long)la + lb;
                maxa = la > maxa ? la : maxa;
                maxb = lb > maxb ? lb : maxb;
                shorts += (la <= 32 && lb <= 32) ? 1u : 0u;
                // (a string the windows cannot index, common.hpp: a short pattern would otherwise walk it as its text. The redo plans the
                // call, and the planned path refuses it)
                if ((la | lb) >= kStringLimit) { misfit = 1; continue; }
                const uint32_t diff = la > lb ? la - lb : lb - la;
                const uint32_t shared = (affix[k] & 63u) + (affix[k] >> 6);
                la -= shared; lb -= shared;
                if (la == 0 || lb == 0) {
                    store_result(args.job, p, (int64_t)clamp_bound(la + lb, args.job.bound));
                } else if (args.job.bound != 0xFFFFFFFFu && diff > args.job.bound) {
                    store_result(args.job, p, (int64_t)args.job.bound + 1);
                } else {
                    const bool pattern_is_a = bp_pattern_is_a(la, lb);
                    const uint32_t m = pattern_is_a ? la : lb, n = pattern_is_a ? lb : la;
                    const uint32_t g = (m + 31) >> 5;
                    if (g > (uint32_t)kTileClasses) {
                        misfit = 1;   // both strings beyond 2048 symbols: not for this kernel (the host redoes the call)
                    } else {
                        cls[k] = g - 1;
                        txt[k] = n;
                        affix[k] |= pattern_is_a ? 1u << 12 : 0u;
                        rank[k] = atomicAdd(&tl.class_count[g - 1], 1u);
                    }
                }
            }
        }
        }
        if constexpr (kInteriorTiles) {
            if (!args.off64) {   // 32-bit offsets: four DPP reductions (the minima as maxima of the complements)
                lo_a = (uint32_t)~wave_max_u32(~(uint32_t)lo_a); hi_a = wave_max_u32((uint32_t)hi_a);
                lo_b = (uint32_t)~wave_max_u32(~(uint32_t)lo_b); hi_b = wave_max_u32((uint32_t)hi_b);
            } else {
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    const unsigned long long la_ = __shfl_xor(lo_a, off), ha_ = __shfl_xor(hi_a, off), lb_ = __shfl_xor(lo_b, off), hb_ = __shfl_xor(hi_b, off);
                    lo_a = la_ < lo_a ? la_ : lo_a; hi_a = ha_ > hi_a ? ha_ : hi_a;
                    lo_b = lb_ < lo_b ? lb_ : lo_b; hi_b = hb_ > hi_b ? hb_ : hi_b;
                }
            }
            if (lane == 0) {
                atomicMin(&tl.span.lo_a, (unsigned long long)lo_a); atomicMax(&tl.span.hi_a, (unsigned long long)hi_a);
                atomicMin(&tl.span.lo_b, (unsigned long long)lo_b); atomicMax(&tl.span.hi_b, (unsigned long long)hi_b);
            }
        }
        __syncthreads();
        // Is this an INTERIOR tile -- may its items read both tapes without clamping their windows (bp_item.hpp: kBpInterior)? On both
        // tapes the lowest start of the tile's strings lies kBpMarginLo bytes or more behind the tape's start and their highest end
        // kBpMarginHi or more before its end (the ACTUAL extents: a cross-product tile's candidates are scattered over their tape),
        // and the two windows, margins included, lie within 2^31 bytes of address space, so that one base and a 32-bit offset reach
        // both. Only the tiles that hold a tape's first or last strings fail the first test; a tile that fails either runs the
        // clamped item, as do tapes shorter than the margins. Workgroup-uniform, read once per tile (wave_sums is next written in step E).
        [[maybe_unused]] bool interior = false;
        [[maybe_unused]] BpTileItem ti;
        if constexpr (kInteriorTiles) {
            const unsigned long long s_lo_a = tl.span.lo_a, s_hi_a = tl.span.hi_a, s_lo_b = tl.span.lo_b, s_hi_b = tl.span.hi_b;
            const bool inside = !targs.no_interior && s_lo_a <= s_hi_a && s_lo_b <= s_hi_b && s_lo_a >= kBpMarginLo && s_lo_b >= kBpMarginLo &&
                                s_hi_a <= a_total && s_hi_b <= b_total && a_total - s_hi_a >= kBpMarginHi && b_total - s_hi_b >= kBpMarginHi;
            const unsigned long long da = (unsigned long long)(uintptr_t)args.job.a.data, db = (unsigned long long)(uintptr_t)args.job.b.data;
            const unsigned long long low = (da + s_lo_a < db + s_lo_b ? da + s_lo_a : db + s_lo_b) - kBpMarginLo;
            const unsigned long long top = (da + s_hi_a > db + s_hi_b ? da + s_hi_a : db + s_hi_b) + kBpMarginHi;
            interior = __builtin_amdgcn_readfirstlane((int)(inside && top - low <= (1ull << 31))) != 0;
            if (interior) {
                const uint32_t base_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)low), base_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(low >> 32));
                ti.base = (bp_global_bytes)(uintptr_t)(((unsigned long long)base_hi << 32) | base_lo);
                ti.a_off = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(da - low));
                ti.b_off = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(db - low));
                ti.a_last = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(da + s_hi_a + kBpMarginHi - 16 - low));
                ti.b_last = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(db + s_hi_b + kBpMarginHi - 16 - low));
            }
        }
        // ---- C: left-overs move up; work items per class (wave 0) -------------------------------------------------
        if (wave == 0) {
            const uint32_t mine = tl.class_count[lane];
            tl.class_thr[lane] = (uint16_t)mine;
            tl.class_tgt[lane] = (uint16_t)lane;
            unsigned long long present = __ballot(mine != 0);
            wave_lds_fence();
            if (lane == 0) {
                uint32_t incoming = 0;
                while (present) {
                    const int c = __builtin_ctzll(present);
                    present &= present - 1;
                    const uint32_t native = tl.class_count[c];
                    uint32_t total = native + incoming;
                    incoming = 0;
                    const uint32_t per = 64u / (uint32_t)(c + 1), rest = total % per;
                    if (rest && present) {
                        const int up = __builtin_ctzll(present);
                        const uint32_t per_up = 64u / (uint32_t)(up + 1);
                        // at most half an item of the class above, instead of a mostly idle item of this one
                        if (rest <= native && 2 * rest <= per_up) {
                            tl.class_thr[c] = (uint16_t)(native - rest);
                            tl.class_tgt[c] = (uint16_t)up;
                            incoming = rest;
                            total -= rest;
                        }
                    }
                    tl.class_count[c] = total;
                }
            }
            wave_lds_fence();
            const uint32_t final_count = tl.class_count[lane], per = 64u / (uint32_t)(lane + 1);
            const uint32_t items = (final_count + per - 1) / per;
            const uint32_t incl = wave_inclusive_sum_u32(items);
            tl.item_prefix[lane] = incl - items;
            if (lane == 63) tl.item_prefix[64] = incl;
        }
        __syncthreads();
        // ---- D: final keys, ranks inside a key ---------------------------------------------------------------------
        uint32_t key[kPer];
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            key[k] = 0xFFFFFFFFu;
            if (cls[k] != 0xFFu) {
                uint32_t c = cls[k];
                if (rank[k] >= tl.class_thr[c]) c = tl.class_tgt[c];
                const uint32_t bucket = txt[k] >> targs.shift;
                key[k] = c * kTileBuckets + (bucket < (uint32_t)kTileBuckets - 1 ? bucket : (uint32_t)kTileBuckets - 1);
                const uint32_t old = atomicAdd(&tl.bins[key[k] >> 1], (key[k] & 1u) ? 0x10000u : 1u);
                rank[k] = (key[k] & 1u) ? old >> 16 : old & 0xFFFFu;
            }
        }
        __syncthreads();
        // ---- E: exclusive scan of the key counters (two u16 per word, in place) -------------------------------------
        {
            // consecutive words per thread, rounded UP (640 threads: 1024 / 640 = 1 left the keys of classes >= 40 -- patterns of more
            // than 1280 symbols -- out of the scan: wrong distances for code-point strings that long, found by the soak test)
            constexpr int kWords = (kTileBins / 2 + kThreads - 1) / kThreads;
            uint32_t words[kWords], sum = 0;
#pragma unroll
            for (int q = 0; q < kWords; ++q) {
                const int at = threadIdx.x * kWords + q;
                words[q] = at < kTileBins / 2 ? tl.bins[at] : 0u;
                sum += (words[q] & 0xFFFFu) + (words[q] >> 16);
            }
            const uint32_t incl = wave_inclusive_sum_u32(sum);
            if (lane == 63) tl.wave_sums[wave] = incl;
            __syncthreads();
            uint32_t run = incl - sum;
            for (int w = 0; w < wave; ++w) run += tl.wave_sums[w];
#pragma unroll
            for (int q = 0; q < kWords; ++q) {
                const uint32_t lo = words[q] & 0xFFFFu, hi = words[q] >> 16;
                const int at = threadIdx.x * kWords + q;
                if (at < kTileBins / 2) tl.bins[at] = run | ((run + lo) << 16);
                run += lo + hi;
            }
        }
        __syncthreads();
        // ---- F: scatter the tile-local indices ------------------------------------------------------------------------
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            if (key[k] != 0xFFFFFFFFu) {
                const uint32_t word = tl.bins[key[k] >> 1];
                const uint32_t start = (key[k] & 1u) ? word >> 16 : word & 0xFFFFu;
                tl.sorted[start + rank[k]] = ((uint32_t)k * kThreads + threadIdx.x) | (affix[k] << kTileIndexBits);   // index | prefix << 11 | suffix << 17 | pattern side << 23
            }
        }
        __syncthreads();
        TILE_STAMP(0);   // planning the tile
        TILE_SPAN(1);
        // The key counters have done their work: keep the 64 class starts (class_thr is free since step D), then the
        // 4 KB they occupied stage the tile's distances -- one coalesced sweep at the end instead of 4-byte stores
        // scattered over the tile's window (which reached HBM as one 32-byte sector each: 6x the result bytes).
        // (class_tgt has been free since step D too: the multiplier that stands for a division by the class's G, lane_over())
        if (threadIdx.x < kTileClasses) {
            tl.class_thr[threadIdx.x] = (uint16_t)(tl.bins[(threadIdx.x * kTileBuckets) >> 1] & 0xFFFFu);
            tl.class_tgt[threadIdx.x] = (uint16_t)(65535u / (threadIdx.x + 1u));
        }
        __syncthreads();
        static_assert(sizeof(tl.bins) >= (size_t)kTileMax * 2, "the key counters' space holds a tile's distances as 16-bit slots");
        uint16_t *const staged = (uint16_t *)tl.bins;
        for (int i = threadIdx.x; i < kTileMax / 2; i += kThreads) tl.bins[i] = 0xFFFFFFFFu;   // "no distance here" (trivial pairs are stored directly)
        __syncthreads();
        // ---- G: work items, heaviest first (high class, long text), dealt by an LDS ticket --------------------------------
        __builtin_amdgcn_s_setprio(0);
        // The item loop exists once per item mode, chosen per tile OUTSIDE the loop for kWide's reason (bp_item.hpp): the interior
        // tiles' unclamped item, the clamped one for the tiles at a tape's edges; code points keep the item that derives everything itself.
        auto run_items = [&](auto mode_tag) {
            constexpr int kMode = decltype(mode_tag)::value;
            const uint32_t items_total = tl.item_prefix[64];
            const uint32_t my_prefix = tl.item_prefix[lane];
            for (;;) {
                uint32_t t = 0;
                if (lane == 0) t = __hip_atomic_fetch_add(&tl.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
                if (t >= items_total) break;
                const uint32_t item = items_total - 1 - t;
                const uint32_t G = (uint32_t)__popcll(__ballot(my_prefix <= item));   // class = prefix entries <= item
                const uint32_t over_g = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)tl.class_tgt[G - 1]);
                const uint32_t per = lane_over(64, over_g);
                const uint32_t chunk = item - tl.item_prefix[G - 1];
                const uint32_t cstart = tl.class_thr[G - 1], ccount = tl.class_count[G - 1];
                const uint32_t slot = lane_over((uint32_t)lane, over_g);
                const uint32_t pidx = chunk * per + slot;
                const bool have = slot < per && pidx < ccount;
                uint64_t p = 0, a0 = 0, b0 = 0;
                uint32_t la = 0, lb = 0;
                BpTileItem mine = ti;
                mine.slot = slot; mine.blk = (uint32_t)lane - slot * G;
                if (have) {
                    const uint32_t entry = tl.sorted[cstart + pidx];
                    p = base + (entry & (uint32_t)(kTileMax - 1));
                    if (args.off64) pair_extent<uint64_t, true>(args.job, p, a0, la, b0, lb);
                    else pair_extent<uint32_t, true>(args.job, p, a0, la, b0, lb);
                    const uint32_t pre = (entry >> kTileIndexBits) & 63u, both = pre + ((entry >> (kTileIndexBits + 6)) & 63u);   // what the pair shares at both ends (step B)
                    a0 += pre; b0 += pre; la -= both; lb -= both;
                    mine.a_is_pattern = (entry >> (kTileIndexBits + 12)) & 1u;   // step B's bp_pattern_is_a of the same cut lengths
                }
                bp_item<Sym, kWide, kMode>(args, wv, G, have, p, a0, la, b0, lb, staged, base, mine);
#ifdef SWH_TILE_PROFILE
                ++items_done;
#endif
            }
        };
        if constexpr (kInteriorTiles) {
            if (interior) run_items(std::integral_constant<int, kBpInterior>{});
            else run_items(std::integral_constant<int, kBpFromTile>{});
        } else if constexpr (sizeof(Sym) == 1) {
            run_items(std::integral_constant<int, kBpFromTile>{});
        } else {
            run_items(std::integral_constant<int, kBpAlone>{});
        }
        TILE_STAMP(1);   // work items
        __syncthreads();
        TILE_STAMP(2);   // waiting for the workgroup's other waves
        TILE_SPAN(2);
        for (uint32_t i = threadIdx.x; i < count; i += kThreads) {
            const uint32_t d = staged[i];
            if (d != 0xFFFFu) store_result(args.job, base + i, (int64_t)d);
        }
        __syncthreads();   // the next tile rewrites the lists
    }
    TILE_SPAN(3);
#ifdef SWH_TILE_PROFILE
    if (lane == 0) {
        for (int q = 0; q < 3; ++q) atomicAdd(&g_tile_phase[q], phase_acc[q]);
        atomicAdd(&g_tile_phase[3], 1ull);
        atomicAdd(&g_tile_phase[4], items_done);
    }
#endif
    {
        TileTail &tail = *(TileTail *)tl.bins;   // the tile loop ended with a barrier
        unsigned long long &lcells = tail.cells, &lsyms = tail.syms;
        uint32_t &lmaxa = tail.maxa, &lmaxb = tail.maxb, &lshorts = tail.shorts, &lmisfit = tail.misfit;
        if (threadIdx.x == 0) { lcells = 0; lsyms = 0; lmaxa = 0; lmaxb = 0; lshorts = 0; lmisfit = 0; }
        __syncthreads();
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
            atomicMax(&lmaxa, maxa);
            atomicMax(&lmaxb, maxb);
            atomicAdd(&lshorts, shorts);
            atomicOr(&lmisfit, misfit);
        }
        __syncthreads();
        report_call_summary(PlanPartial{lcells, lsyms, lmaxa, lmaxb, lshorts, lmisfit}, targs.partials, targs.done_counter, targs.summary, tail.summary);
    }
}

template <typename Sym, int kWaves, bool kPlain = false>
__global__ __launch_bounds__(kWaves * 64, BpTraits<Sym>::kMinWavesPerSimd) void k_bitparallel_tiled(TiledArgs targs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const KernelArgs &args = targs.k;
    const uint64_t a_total = tape_total(args.job.a, args.off64);
    const uint64_t b_total = tape_total(args.job.b, args.off64);
    if constexpr (sizeof(Sym) == 1) {
        if (a_total >= 16 && b_total >= 16) tiled_run<Sym, kWaves, true, kPlain>(targs, smem, a_total, b_total);
        else tiled_run<Sym, kWaves, false, kPlain>(targs, smem, a_total, b_total);
    } else {
        tiled_run<Sym, kWaves, false, kPlain>(targs, smem, a_total, b_total);
    }
}

// The plain-shape kernel on two prepared tapes with side arrays (tiled_run: kSide). A kernel of its own name rather than one more
// parameter of the template above, which would rename every instantiation in the profiles and the resource table. Tapes shorter than a
// window cut no affixes and so read no side arrays.
template <int kWaves>
__global__ __launch_bounds__(kWaves * 64, BpTraits<uint8_t>::kMinWavesPerSimd) void k_bitparallel_tiled_side(TiledArgs targs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const KernelArgs &args = targs.k;
    const uint64_t a_total = tape_total<uint32_t>(args.job.a), b_total = tape_total<uint32_t>(args.job.b);
    if (a_total >= 16 && b_total >= 16) tiled_run<uint8_t, kWaves, true, true, true>(targs, smem, a_total, b_total);
    else tiled_run<uint8_t, kWaves, false, true>(targs, smem, a_total, b_total);
}

// Tile size: every workgroup slot should get the same number of tiles (1, 2, ...), tiles stay <= kTileMax pairs, and a
// batch too small to give every slot a useful tile uses fewer workgroups instead of smaller tiles.
TilePlan plan_tiles(uint64_t pairs, uint32_t slots, uint32_t longest_text, uint32_t kTileMax) {
    TilePlan tp{};
    constexpr uint32_t kTileMin = 256;
    const uint64_t rounds = (pairs + (uint64_t)slots * kTileMax - 1) / ((uint64_t)slots * kTileMax);
    uint64_t tile = (pairs + slots * rounds - 1) / (slots * rounds);
    static const uint32_t forced = [] { const char *e = test_hook("STRINGWARS_AMD_TILE"); return e ? (uint32_t)atoi(e) : 0u; }();   // tuning knob
    if (forced) tile = forced;
    if (tile < kTileMin) tile = kTileMin;
    if (tile > (uint64_t)kTileMax) tile = kTileMax;
    tp.tile = (uint32_t)tile;
    tp.tiles = (uint32_t)((pairs + tile - 1) / tile);
    tp.blocks = tp.tiles < slots ? tp.tiles : slots;
    uint32_t shift = 0;
    while (((uint64_t)longest_text >> shift) >= (uint64_t)kTileBuckets) ++shift;
    tp.shift = shift;
    return tp;
}

template <typename Sym, int kWaves>
static void launch_tiled_sym(Scope *scope, const KernelArgs &args, uint64_t pairs, uint32_t longest_text, const uint4 *side_a, const uint4 *side_b) {
    constexpr size_t lds = tiled_lds_bytes<Sym, kWaves>();
    uint32_t slots = (uint32_t)scope->compute_units * (uint32_t)((160 * 1024) / lds);
    if (slots > (uint32_t)kMaxPartials) slots = kMaxPartials;
    const TilePlan tp = plan_tiles(pairs, slots, longest_text, (uint32_t)tile_max(kWaves));
    TiledArgs t{};
    t.k = args;
    t.k.boundary = nullptr;
    t.tile = tp.tile; t.tiles = tp.tiles; t.shift = tp.shift;
    static const bool no_affix = [] { const char *e = test_hook("STRINGWARS_AMD_AFFIX"); return e && atoi(e) == 0; }();   // comparison knob
    t.cut_affixes = sizeof(Sym) == 1 && !no_affix ? 1u : 0u;
    static const bool no_interior = [] { const char *e = test_hook("STRINGWARS_AMD_INTERIOR"); return e && atoi(e) == 0; }();   // comparison knob
    t.no_interior = no_interior ? 1u : 0u;
    t.partials = scope->plan_partials;
    t.done_counter = scope->done_counter;
    t.summary = scope->summary_target();
    // the headline shape (bytes, sixteen waves, 32-bit offsets, pairwise, unbounded) has a kernel of its own
    void (*kernel)(TiledArgs) = k_bitparallel_tiled<Sym, kWaves>;
    if constexpr (sizeof(Sym) == 1 && kWaves == 16) {
        if (!args.off64 && !args.job.cross && args.job.bound == 0xFFFFFFFFu) {
            kernel = k_bitparallel_tiled<Sym, kWaves, true>;
            // ... which plans its tiles from the side arrays of two prepared tapes (not where the affixes stay uncut: they are all it reads there)
            if (side_a && side_b && t.cut_affixes) {
                kernel = k_bitparallel_tiled_side<kWaves>;
                t.side_a = side_a; t.side_b = side_b;
#ifdef SWH_TEST_HOOKS
                ++g_tiled_side_launches;
#endif
            }
        }
    }
    opt_in_dynamic_lds(scope, (const void *)kernel, lds);
    static const bool debug = test_hook("STRINGWARS_AMD_DEBUG") != nullptr;
    if (debug) {
        int per_cu = 0;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kWaves * 64, lds);
        fprintf(stderr, "[swh] tiled: pairs %llu tile %u tiles %u blocks %u shift %u lds %zu -> %d workgroups per CU\n",
                (unsigned long long)pairs, tp.tile, tp.tiles, tp.blocks, tp.shift, lds, per_cu);
    }
    StampGuard guard(scope, sizeof(Sym) == 1 ? "bitparallel_tiled" : "bitparallel_tiled_u32");
    hipLaunchKernelGGL(kernel, dim3(tp.blocks), dim3(kWaves * 64), lds, scope->stream, t);
    SWH_HIP_CHECK(hipGetLastError());
}

void launch_bitparallel_tiled(Scope *scope, const KernelArgs &args, uint64_t pairs, uint32_t longest_text) {
    launch_bitparallel_tiled_side(scope, args, pairs, longest_text, nullptr, nullptr);
}

// side_a / side_b: the side arrays of two prepared byte tapes (api.hpp: Prepared::side) at the views' first strings, or null. Only the
// headline shape's kernel reads them; every other launch goes as if they were not there.
void launch_bitparallel_tiled_side(Scope *scope, const KernelArgs &args, uint64_t pairs, uint32_t longest_text, const uint4 *side_a, const uint4 *side_b) {
    static const int forced = [] { const char *e = test_hook("STRINGWARS_AMD_TILED_WAVES"); return e ? atoi(e) : 0; }();   // comparison knob: 4; code points also 8
    if (args.sym_bytes == 4) {   // code points: 14.25 KB of tables per wave -- one workgroup of ten waves fills a CU next to the tile's lists
                                 // (latency-bound like the planned kernel: 8 -> 10 waves is 8 % on token-sized strings; STRINGWARS_AMD_TILED_WAVES=8 / =4:
                                 // eight waves; two-wave workgroups, five per CU)
        if (forced == 4) launch_tiled_sym<uint32_t, BpTraits<uint32_t>::kWaves>(scope, args, pairs, longest_text, side_a, side_b);
        else if (forced == 8) launch_tiled_sym<uint32_t, 8>(scope, args, pairs, longest_text, side_a, side_b);
        else launch_tiled_sym<uint32_t, 10>(scope, args, pairs, longest_text, side_a, side_b);
    }
    else if (forced == 4) launch_tiled_sym<uint8_t, 4>(scope, args, pairs, longest_text, side_a, side_b);
    else if (forced == 8) launch_tiled_sym<uint8_t, 8>(scope, args, pairs, longest_text, side_a, side_b);
    // a batch that fills the device: ONE sixteen-wave workgroup per compute unit, one tile of up to 4096 pairs each. Two eight-wave
    // workgroups share a CU unevenly -- the arbiter favours the older one, it finishes at ~half time and the younger runs the rest
    // of its tile at two waves per SIMD (tools/tile_spans.py) --; sixteen waves on one ticket finish together.
    // (Not in asynchronous scopes: two pipelined launches share the device best as eight-wave workgroups side by side on a CU -- 32.8
    // TCUPS over pipelined steps against 31.2 -- where a 160 KB workgroup keeps the other launch off its CU.)
    else if (forced == 16 || (!forced && !scope->async && pairs >= (uint64_t)scope->compute_units * 2048)) launch_tiled_sym<uint8_t, 16>(scope, args, pairs, longest_text, side_a, side_b);
    else launch_tiled_sym<uint8_t, 8>(scope, args, pairs, longest_text, side_a, side_b);
}

}  // namespace swh
