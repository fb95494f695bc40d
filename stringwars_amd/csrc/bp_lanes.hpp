// bp_lanes.hpp -- what the lane-per-block kernel families share (infix.hip, osa.hip, lcs.hip, jaro.hip): one string's symbols are the
// rows, cut into blocks of 32, the other string's are the columns; G lanes per pair, one per block, floor(64 / G) pairs per wave; the
// lane of block k works on column s - k in step s and takes what crosses the block edge from the lane below it by DPP. The match
// words come from the wave's LDS tables (nibble tables for bytes, 3-bit group tables for code points, bp_window.hpp / bp_item.hpp),
// the columns' string is prefetched one super-step of 16 symbols ahead. The layout is bp_item.hpp's; these families are plan-free
// (they cut their own items) and differ from each other in their recurrence and in what the keeper lane writes.
//
// Shared here: lane_blocks, the pair split of OsaTapes, the two parts of a sizes kernel (the workgroup's sums, the cut of a wave's
// run of pairs into LaneItems), the item skeleton BpLanes (tables, prefetch, super-step loop) and the launch of an item kernel. A
// family writes: which string supplies the rows, `columns`, its boundary masks, its `column` recurrence, its reductions after the
// loop and the keeper's stores.
//
// The offset reader (tape_extent), lds_order and readlane64 come from cross_words.hpp, which the word-sized cross-product kernels
// (cross.hip, topk.hip, within.hip) include without this header's bp_item.hpp and osa.hpp.
#pragma once
#include <algorithm>
#include <type_traits>

#include "bp_item.hpp"
#include "cross_words.hpp"
#include "osa.hpp"

namespace swh {

// 32-row blocks (lanes) of a string of m rows; an empty string still takes a lane
__device__ __forceinline__ uint32_t lane_blocks(uint32_t m) { return m ? (m + 31) >> 5 : 1u; }

// the strings of the launch's pair p
__device__ __forceinline__ void lane_pair(const OsaTapes &t, uint64_t p, uint64_t &ia, uint64_t &ib) {
    if (t.nb) { const uint64_t row = p / t.nb; ia = t.row0 + row; ib = p - row * t.nb; }
    else { ia = p; ib = p; }
}

// ---- the sizes kernels: one thread per pair, 256 threads, one wave per run of 64 consecutive pairs ----
struct LaneSizesLds {
    unsigned long long part[4][2];
    uint32_t blocks_of[4][64];   // the lanes' block counts; 0: no pair there
};

// The launch's sums of cells and symbols: one atomic per workgroup and quantity. Returns true on the thread that added them.
template <typename Sizes>
__device__ __forceinline__ bool lane_sizes_sum(LaneSizesLds &lds, Sizes *sizes, unsigned long long cells, unsigned long long symbols) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = 32; s > 0; s >>= 1) {
        cells += __shfl_xor(cells, s);
        symbols += __shfl_xor(symbols, s);
    }
    if (lane == 0) { lds.part[wave][0] = cells; lds.part[wave][1] = symbols; }
    __syncthreads();
    if (threadIdx.x != 0) return false;
    for (int w = 1; w < 4; ++w) { cells += lds.part[w][0]; symbols += lds.part[w][1]; }
    atomicAdd(&sizes->cells, cells);
    atomicAdd(&sizes->symbols, symbols);
    return true;
}

// The item that starts at pair `first` of a run: it takes pairs while pairs x G <= 64, G the largest block count among them
// (lanes past a shorter string idle). Returns its pairs.
__device__ __forceinline__ uint32_t lane_item_at(const uint32_t *blocks_of, uint32_t first, uint32_t in_run, uint32_t &G) {
    uint32_t k = 1;
    G = blocks_of[first];
    while (first + k < in_run) {
        const uint32_t g2 = blocks_of[first + k], widest = g2 > G ? g2 : G;
        if ((k + 1) * widest > 64) break;
        G = widest; ++k;
    }
    return k;
}

// Cuts my wave's run greedily into items of consecutive pairs, on the wave's first lane, from the block counts the lanes left in
// LDS (after lane_sizes_sum's barrier). The run's items are counted first, then placed with one atomic.
template <typename Sizes>
__device__ __forceinline__ void lane_cut_run(const LaneSizesLds &lds, Sizes *sizes, LaneItem *items) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t *blocks_of = lds.blocks_of[wave];
    if (!items || lane != 0 || !blocks_of[0]) return;
    const uint64_t run_first = (uint64_t)blockIdx.x * blockDim.x + (uint64_t)wave * 64;
    uint32_t in_run = 0, count = 0, G;
    while (in_run < 64 && blocks_of[in_run]) ++in_run;
    for (uint32_t first = 0; first < in_run; ++count) first += lane_item_at(blocks_of, first, in_run, G);
    LaneItem *out = items + atomicAdd(&sizes->items, (unsigned long long)count);
    for (uint32_t first = 0; first < in_run;) {
        LaneItem it;
        it.pairs = lane_item_at(blocks_of, first, in_run, G);
        it.first = run_first + first; it.blocks = G;
        *out++ = it;
        first += it.pairs;
    }
}

// ---- the item skeleton ----
// kWide: byte tapes of at least 16 bytes each, the columns' string read with 128-bit loads (a compile-time switch, bp_item.hpp).
// kMirror (infix.hip's start pass): both strings are read backwards from an `end` -- symbols idx .. idx + 3 are the window at
// end - 4 - idx with its symbols swapped. The flag is the only way those reads differ.
template <typename Sym, bool kWide, bool kMirror = false>
struct BpLanes {
    static constexpr bool kBytes = sizeof(Sym) == 1;
    static_assert(kBytes || !kWide, "128-bit reads of the columns' string are a byte-tape variant");
    static_assert(!(kMirror && kWide), "mirrored windows are short: they are read word by word");
    static constexpr int kEntries = BpTraits<Sym>::kEntries;
    static constexpr int kTextRegs = kBytes ? 4 : 16;   // 16 symbols: 4 dwords of bytes, or 16 code points
    using Window = typename std::conditional<kBytes, ByteWindow, SymWindow32>::type;

    uint32_t *table;   // the wave's tables, [kEntries][64 lanes]
    int lane;
    typename std::conditional<kBytes, NibbleTables, GroupTables3>::type tab;
    uint32_t tnxt[kTextRegs];   // the next super-step's symbols as they were loaded
    int tshift[kBytes ? 4 : 1];

    static __device__ __forceinline__ uint32_t raw4(const ByteWindow &w, int idx, int end, int &shift) {
        return w.fetch4_raw(kMirror ? end - 4 - idx : idx, shift);
    }
    static __device__ __forceinline__ uint32_t word4(uint32_t raw, int shift) {
        const uint32_t dw = ByteWindow::realign(raw, shift);
        return kMirror ? __builtin_bswap32(dw) : dw;
    }
    static __device__ __forceinline__ void sym4(const SymWindow32 &w, int idx, int end, uint32_t *out) {
        uint32_t four[4];
        w.fetch4(kMirror ? end - 4 - idx : idx, four);
#pragma unroll
        for (int r = 0; r < 4; ++r) out[r] = four[kMirror ? 3 - r : r];
    }

    // once per wave; `table`: 8 KB (bytes) or 14 KB (code points) per wave, from LDS address 0 -- what NibbleTables / GroupTables3 need
    __device__ __forceinline__ void init(uint32_t *table_, int lane_) {
        table = table_; lane = lane_;
        tab.init(table, lane);
    }

    // requests the columns' symbols first .. first + 15 (unconditional: clamped addresses are always readable, bp_item.hpp)
    __device__ __forceinline__ void fetch_text(const Window &txt, int first, [[maybe_unused]] int end = 0) {
        if constexpr (kBytes) {
            if constexpr (kWide) {
                tshift[0] = txt.fetch16_raw(first, tnxt);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) tnxt[q] = raw4(txt, first + q * 4, end, tshift[q]);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 16; q += 4) sym4(txt, first + q, end, tnxt + q);
        }
    }

    // ---- the match tables of my block: rows row0 .. min(row0 + 32, m) - 1 of `pat` ----
    // The block's 32 symbols are requested at once: one memory latency per item. Byte words arrive unaligned-corrected only where
    // they are consumed (`word4`).
    // (`m`: the rows of this lane's string, 0 for a lane with nothing to do. The row count is worked out next to the insert loop's
    // tests: handed down as a finished number, the 32 tests of the code-point loop compile to 32 separate regions instead of one nest.)
    static __device__ __forceinline__ uint32_t block_rows(uint32_t row0, uint32_t m) { return m > row0 ? (m - row0 < 32 ? m - row0 : 32) : 0; }
    static constexpr int kRowRegs = kBytes ? 8 : 32, kRowShifts = kBytes ? 8 : 1;
    static __device__ __forceinline__ void fetch_rows(const Window &pat, uint32_t row0, uint32_t (&raw)[kRowRegs], [[maybe_unused]] int (&shift)[kRowShifts],
                                                      [[maybe_unused]] int end = 0) {
        if constexpr (kBytes) {
#pragma unroll
            for (int q = 0; q < 8; ++q) raw[q] = raw4(pat, (int)row0 + q * 4, end, shift[q]);
        } else {
#pragma unroll
            for (int q = 0; q < 32; q += 4) sym4(pat, (int)row0 + q, end, raw + q);
        }
    }
    // row q of a fetched block, 0 <= q < 32
    static __device__ __forceinline__ uint32_t row_symbol(const uint32_t (&raw)[kRowRegs], [[maybe_unused]] const int (&shift)[kRowShifts], int q) {
        if constexpr (kBytes) return (word4(raw[q >> 2], shift[q >> 2]) >> (8 * (q & 3))) & 0xFFu;
        else return raw[q];
    }
    __device__ __forceinline__ void clear_tables() const {
#pragma unroll
        for (int k = 0; k < kEntries; ++k) table[k * 64 + lane] = 0;
        wave_lds_fence();
    }
    // (follow with a wave_lds_fence() before the first look-up)
    __device__ __forceinline__ void insert_rows(const uint32_t (&raw)[kRowRegs], [[maybe_unused]] const int (&shift)[kRowShifts], uint32_t row0, uint32_t m) const {
        const uint32_t brows = block_rows(row0, m);
        if constexpr (kBytes) {
            // rows past the block's end OR in a zero (one predicated branch per word instead of one per byte)
            const uint32_t row_mask = brows >= 32 ? 0xFFFFFFFFu : ((1u << brows) - 1u);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (brows > (uint32_t)q * 4) {
                    const uint32_t dw = word4(raw[q], shift[q]);
                    tab.template insert<0>(dw, row_mask & (1u << (q * 4 + 0)));
                    tab.template insert<1>(dw, row_mask & (1u << (q * 4 + 1)));
                    tab.template insert<2>(dw, row_mask & (1u << (q * 4 + 2)));
                    tab.template insert<3>(dw, row_mask & (1u << (q * 4 + 3)));
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < 32; ++q)
                if ((uint32_t)q < brows) tab.insert(raw[q], 1u << q);
        }
    }
    // (jaro.hip, which has reads of its own to send out between the block's reads and their inserts, calls the parts itself)
    __device__ __forceinline__ void build_tables(const Window &pat, uint32_t row0, uint32_t m, int end = 0) const {
        uint32_t raw[kRowRegs];
        int shift[kRowShifts];
        clear_tables();
        fetch_rows(pat, row0, raw, shift, end);
        insert_rows(raw, shift, row0, m);
        wave_lds_fence();
    }

    // The super-steps of 16 columns, after fetch_text(txt, 0 - blk): `column(eq, s)` -- or `column(eq, s, symbol)` -- is called for
    // steps s = 0, 1, ... in order with the match word (and the symbol) of this lane's column s - blk; it tests s - blk against its
    // own `columns`. steps = n_eff rounded up to 16, n_eff the wave's step count.
    template <typename Column>
    __device__ __forceinline__ void run(const Window &txt, uint32_t steps, uint32_t n_eff, uint32_t blk, Column &&column, int end = 0) {
        constexpr bool kWithSymbol = std::is_invocable<Column, uint32_t, uint32_t, uint32_t>::value;
        for (uint32_t s0 = 0; s0 < steps; s0 += 16) {
            uint32_t tcur[kTextRegs];
            if constexpr (kBytes) {
                if constexpr (kWide) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) tcur[q] = tnxt[q];
                    txt.fix16((int)s0 - (int)blk, tshift[0], tcur);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) tcur[q] = word4(tnxt[q], tshift[q]);
                }
            } else {
#pragma unroll
                for (int q = 0; q < kTextRegs; ++q) tcur[q] = tnxt[q];
            }
            fetch_text(txt, (int)s0 + 16 - (int)blk, end);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t gs = s0 + q * 4;
                if (gs >= n_eff) break;  // wave-uniform: no lane has a symbol left in this group
                uint32_t eqs[4];
                [[maybe_unused]] uint32_t syms[4];
                if constexpr (kBytes) {
                    eqs[0] = tab.template lookup<0>(tcur[q]);
                    eqs[1] = tab.template lookup<1>(tcur[q]);
                    eqs[2] = tab.template lookup<2>(tcur[q]);
                    eqs[3] = tab.template lookup<3>(tcur[q]);
#pragma unroll
                    for (int u = 0; u < 4; ++u) syms[u] = tcur[q] >> (8 * u);   // (the symbol is the low byte)
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u) { eqs[u] = tab.lookup(tcur[q * 4 + u]); syms[u] = tcur[q * 4 + u]; }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if constexpr (kWithSymbol) column(eqs[u], gs + u, syms[u]);
                    else column(eqs[u], gs + u);
                }
            }
        }
    }
};

// Launches an item kernel over r.item_count items, kWaves of them per workgroup.
template <typename Sym, typename Tapes, typename Run>
static void lane_launch(Scope *scope, void (*kernel)(Tapes, Run), const Tapes &t, const Run &r) {
    constexpr int kWaves = BpTraits<Sym>::kWaves;
    const uint64_t blocks = std::min<uint64_t>((r.item_count + kWaves - 1) / kWaves, 1u << 22);
    hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(kWaves * 64), 0, scope->stream, t, r);
    SWH_HIP_CHECK(hipGetLastError());
}

}  // namespace swh
