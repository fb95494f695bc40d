// jaro.hip -- the counts behind the Jaro and Jaro-Winkler similarities of every pair (swh_levenshtein_jaro_*; rapidfuzz
// distance.Jaro / distance.JaroWinkler, jellyfish jaro_similarity / jaro_winkler_similarity).
//
// The definition (stringwars_amd.h has it in full): with a of m symbols and b of n, R = max(0, max(m, n) / 2 - 1); a's symbols are
// taken in order, and a[i] matches the smallest j in [i - R, i + R] with b[j] == a[i] that no earlier symbol of a has flagged. M is
// the number of matches, h the number of k < M at which the k-th matched symbol of a differs from the k-th flagged symbol of b,
// t = h / 2, and the prefix is the common prefix of at most four symbols. The definition is one-sided -- a drives, b is flagged --
// and the kernel never swaps the sides of a pair: b's n symbols are the rows, cut into blocks of 32, a's m symbols are the columns.
//
// lcs.hip's layout, whose shared text (tables, prefetch, super-step loop, the sizes kernel's sums and cut) is bp_lanes.hpp's: G lanes per pair, one per block of b, floor(64 / G) pairs per wave; the lane of block k works on column
// s - k in step s. n <= 32 is one lane per pair with everything in registers.
//
// Pass 1, the flags. A lane keeps F, the flagged rows of its block (0 at first). In column i, with Eq the match word of a[i]:
//     w = Eq & window(i) & ~F        window(i): the block's bits j with i - R <= j <= i + R
//     cin = the "found" bit of the block below in the SAME column (0 for block 0)
//     cin == 0 and w != 0:  F |= w & -w, cout = 1        otherwise:  cout = cin
// The found bit is all that crosses a block edge, and it travels like lcs.hip's carry: the lane above runs the column one step later
// and reads by DPP (wave_shr:1) what its neighbour left in the step before. A lane whose column is not active advances nothing.
// Columns i >= n + R cannot match, so min(m, n + R) columns run. The lane of the LAST block sees the column's final found bit; when
// it is set, the lane appends a[i] -- it holds the symbol in its text registers at that step -- to the pair's slice of the wave's
// LDS buffer at a running rank. A wave's pairs hold at most 64 x 32 rows, so 2048 symbols per wave suffice whatever m is.
//
// Pass 2, the transpositions. A lane's base rank is the number of flagged rows in the pair's lower blocks (G - 1 DPP steps). It
// walks its flagged rows from the lowest and compares b[row] -- the block's symbols, read once more -- with the buffered symbol at
// base + local rank. h is the sum over the pair's lanes, M the sum of the popcounts; the lane of the last block writes M, h / 2
// and the prefix.
//
// Work items: k_jaro_sizes measures the pairs (cells, the first pair with a string over SWH_JARO_MAX_LENGTH -- errors come before
// any output) and cuts every run of 64 consecutive pairs into items as k_osa_sizes does, with the blocks of b. The same kernels
// serve the pairwise calls and, in slices of whole rows, the cross-products (OsaTapes).
#include "jaro.hpp"
#include "bp_lanes.hpp"

namespace swh {

static_assert(SWH_JARO_MAX_LENGTH == 2048u, "one wave's 64 blocks of 32 rows; the wave's buffer of matched symbols");
constexpr uint32_t kJaroBuffer = 2048;   // matched symbols of a per wave: its pairs flag at most 64 x 32 rows

// One thread per pair: the sums, the first pair with an oversize string, and (with `items`) the items of each run of 64 pairs, by
// the blocks of b (bp_lanes.hpp).
__global__ void __launch_bounds__(256) k_jaro_sizes(OsaTapes t, OsaSizes *sizes, LaneItem *items) {
    __shared__ LaneSizesLds lds;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long cells = 0, symbols = 0;
    uint32_t g = 0;   // 0: no pair here
    if (i < t.count) {
        uint64_t ia, ib, a0, b0;
        uint32_t la, lb;
        lane_pair(t, i, ia, ib);
        tape_extent(t.a, t.a_off64, ia, a0, la);
        tape_extent(t.b, t.b_off64, ib, b0, lb);
        cells = (unsigned long long)la * lb;
        symbols = (unsigned long long)la + lb;
        if (la > SWH_JARO_MAX_LENGTH || lb > SWH_JARO_MAX_LENGTH) {
            atomicMin(&sizes->first_oversize, (unsigned long long)i);
            if (lb > SWH_JARO_MAX_LENGTH) lb = SWH_JARO_MAX_LENGTH;   // (the call fails; the items only have to stay well-formed)
        }
        g = lane_blocks(lb);
    }
    lds.blocks_of[threadIdx.x >> 6][threadIdx.x & 63] = g;
    if (lane_sizes_sum(lds, sizes, cells, symbols) && blockIdx.x == 0) {
        sizes->a_total = tape_total(t.a, t.a_off64);
        sizes->b_total = tape_total(t.b, t.b_off64);
    }
    lane_cut_run(lds, sizes, items);
}

template <typename Sym, bool kWide>
__global__ void __launch_bounds__(BpTraits<Sym>::kWaves * 64, BpTraits<Sym>::kMinWavesPerSimd) k_jaro(OsaTapes t, JaroRun run) {
    using Lanes = BpLanes<Sym, kWide>;
    constexpr bool kBytes = Lanes::kBytes;
    constexpr int kWaves = BpTraits<Sym>::kWaves, kEntries = BpTraits<Sym>::kEntries;
    // the wave's tables: 8 KB (bytes) or 14 KB (code points) apart, from LDS address 0 -- the layout NibbleTables / GroupTables3 need
    __shared__ __attribute__((aligned(8192))) uint32_t tables[kWaves * kEntries * 64];
    // the matched symbols of a, pair by pair in a's order: 2 KB (bytes) or 8 KB (code points) per wave
    __shared__ Sym matched_of[kWaves * kJaroBuffer];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Sym *const matched = matched_of + wave * kJaroBuffer;
    Lanes lanes;
    lanes.init(tables + wave * kEntries * 64, lane);
    const uint64_t a_total = tape_total(t.a, t.a_off64), b_total = tape_total(t.b, t.b_off64);
    using Window = typename Lanes::Window;

    for (uint64_t item = (uint64_t)blockIdx.x * kWaves + wave; item < run.item_count; item += (uint64_t)gridDim.x * kWaves) {
        const LaneItem it = run.items[item];
        const uint32_t G = it.blocks;
        const uint32_t slot = (uint32_t)lane / G, blk = (uint32_t)lane - slot * G;
        const bool have = slot < it.pairs;
        const uint64_t p = it.first + (have ? slot : 0);
        uint64_t ia, ib, a0, b0;
        uint32_t m, n;
        lane_pair(t, p, ia, ib);
        tape_extent(t.a, t.a_off64, ia, a0, m);
        tape_extent(t.b, t.b_off64, ib, b0, n);
        // rows / bits / lanes: b, whichever is longer; columns / steps: a
        const uint32_t longer = m > n ? m : n;
        const int R = longer >= 4 ? (int)(longer / 2 - 1) : 0;
        const uint32_t last = lane_blocks(n) - 1;   // the block whose lane sees a column's final found bit
        const bool keeper = have && blk == last;
        const uint32_t columns = (have && m && n) ? (m < n + (uint32_t)R ? m : n + (uint32_t)R) : 0;
        // lanes that start a pair take no found bit
        const bool first_blk = blk == 0;
        uint32_t keep_mask = first_blk ? 0u : 0xFFFFFFFFu;
        asm volatile("" : "+v"(keep_mask));   // opaque, so that the splice stays one v_and (bp_item)
        // the pair's slice of the wave's buffer: its G blocks flag at most 32 G rows, and slot * 32 G + 32 G <= 2048
        const uint32_t slice = slot * G * 32;
        const uint32_t row0 = blk * 32;
        const uint32_t rows = columns ? n : 0, brows = Lanes::block_rows(row0, rows);

        uint32_t flags = 0, rank = 0, prefix = 0;
        // wave-uniform step count (lane `blk` of a pair works in steps blk .. columns + blk - 1)
        const uint32_t n_eff = wave_max_u32(columns ? columns + last : 0);
        if (n_eff) {   // (so both tapes hold symbols: the clamped windows below have something to read)
            const uint32_t steps = (n_eff + 15) & ~15u;
            Window pat, txt;
            pat.init((const Sym *)t.b.data, b0, b_total);
            txt.init((const Sym *)t.a.data, a0, a_total);
            lanes.fetch_text(txt, 0 - (int)blk);

            // ---- the match tables of my block, and the common prefix of the pair's first four symbols (its reads go out between the
            // block's reads and their inserts) ----
            const uint32_t shorter = m < n ? m : n, prefix_max = shorter < 4 ? shorter : 4;
            uint32_t braw[Lanes::kRowRegs];
            int bshifts[Lanes::kRowShifts];
            lanes.clear_tables();
            Lanes::fetch_rows(pat, row0, braw, bshifts);
            if constexpr (kBytes) {
                int ashift, bshift;
                const uint32_t a4 = txt.fetch4_raw(0, ashift), b4 = pat.fetch4_raw(0, bshift);
                lanes.insert_rows(braw, bshifts, row0, rows);
                // (bytes past a string's end are whatever follows it: prefix_max cuts them off)
                const uint32_t differ = ByteWindow::realign(a4, ashift) ^ ByteWindow::realign(b4, bshift);
                prefix = differ ? (uint32_t)(__ffs((int)differ) - 1) >> 3 : 4u;
            } else {
                uint32_t a4[4], b4[4];
                txt.fetch4(0, a4);
                pat.fetch4(0, b4);
                lanes.insert_rows(braw, bshifts, row0, rows);
                prefix = a4[0] != b4[0] ? 0u : (a4[1] != b4[1] ? 1u : (a4[2] != b4[2] ? 2u : (a4[3] != b4[3] ? 3u : 4u)));
            }
            prefix = prefix < prefix_max ? prefix : prefix_max;
            wave_lds_fence();

            // ---- pass 1: the flags of my block, the matched symbols of a ----
            uint32_t found = 0;   // of my last column: 1 if my block or one below it took the column's symbol
            auto column = [&](uint32_t eq, uint32_t s, uint32_t sym) {
                const uint32_t cin = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)found, 0x138, 0xf, 0xf, true) & keep_mask;
                if (s - blk < columns) {
                    // the window's bits of my block: rows i - R .. i + R, i - row0 = d
                    const int d = (int)(s - blk) - (int)row0;
                    const uint32_t lo = (uint32_t)bp_med3i(d - R, 0, 32), hi = (uint32_t)bp_med3i(d + R + 1, 0, 32);
                    const uint32_t window = (uint32_t)(0xFFFFFFFFull << lo) & (uint32_t)((1ull << hi) - 1ull);
                    const uint32_t w = eq & window & ~flags;
                    flags |= (w & (0u - w)) & (cin - 1u);   // the lowest free match, unless a lower block has taken the column
                    found = cin | (w ? 1u : 0u);
                    if (keeper && found) {
                        matched[(slice + rank) & (kJaroBuffer - 1)] = (Sym)sym;
                        ++rank;
                    }
                }
            };
            lanes.run(txt, steps, n_eff, blk, column);
        }
        wave_lds_fence();   // the matched symbols were written by the lanes of the last blocks, and are read by every lane

        // the flagged rows below my block: the blocks' counts, summed upwards (G is no power of two: G - 1 wave_shr:1 steps)
        const uint32_t mine = (uint32_t)__popc(flags);
        uint32_t upto = mine;
        for (uint32_t k = 1; k < G; ++k)   // wave-uniform
            upto = mine + ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)upto, 0x138, 0xf, 0xf, true) & keep_mask);

        // ---- pass 2: my flagged rows against the matched symbols of a at the same ranks ----
        uint32_t differ = 0;
        const uint32_t rows_eff = wave_max_u32(mine ? brows : 0);
        if (rows_eff) {   // (so n_eff was not 0 either: b's tape holds symbols)
            Window pat;
            pat.init((const Sym *)t.b.data, b0, b_total);
            uint32_t braw[Lanes::kRowRegs];
            int bshifts[Lanes::kRowShifts];
            Lanes::fetch_rows(pat, row0, braw, bshifts);
            uint32_t at = slice + upto - mine;   // where my lowest flagged row's partner lies
#pragma unroll
            for (int q = 0; q < 32; ++q) {
                if ((q & 3) == 0 && (uint32_t)q >= rows_eff) break;   // wave-uniform
                const uint32_t flagged = (flags >> q) & 1u;
                const uint32_t theirs = (uint32_t)matched[at & (kJaroBuffer - 1)];
                const uint32_t ours = Lanes::row_symbol(braw, bshifts, q);
                differ += flagged & (ours != theirs ? 1u : 0u);
                at += flagged;
            }
        }
        uint32_t h = differ;
        for (uint32_t k = 1; k < G; ++k)   // wave-uniform
            h = differ + ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)h, 0x138, 0xf, 0xf, true) & keep_mask);

        if (keeper) {   // upto: the pair's matches (lanes past the last block hold none)
            const uint32_t M = upto, T = h >> 1;
            if (t.nb) {
                const uint64_t row = p / t.nb, at = row * run.stride + (p - row * t.nb) * 8;
                if (run.matches) *(uint64_t *)(run.matches + at) = M;
                if (run.transpositions) *(uint64_t *)(run.transpositions + at) = T;
                if (run.prefix) *(uint64_t *)(run.prefix + at) = prefix;
            } else {
                if (run.matches) *(uint32_t *)(run.matches + p * run.stride) = M;
                if (run.transpositions) *(uint32_t *)(run.transpositions + p * run.stride) = T;
                if (run.prefix) *(uint32_t *)(run.prefix + p * run.stride) = prefix;
            }
        }
        wave_lds_fence();   // the next item writes the buffer
    }
}

void launch_jaro_sizes(Scope *scope, const OsaTapes &t, OsaSizes *sizes, LaneItem *items) {
    StampGuard guard(scope, "jaro_sizes");
    hipLaunchKernelGGL(k_jaro_sizes, dim3((uint32_t)((t.count + 255) / 256)), dim3(256), 0, scope->stream, t, sizes, items);
    SWH_HIP_CHECK(hipGetLastError());
}

void launch_jaro(Scope *scope, const OsaTapes &t, const JaroRun &r) {
    if (!r.item_count) return;
    StampGuard guard(scope, t.cp ? "jaro_u32" : "jaro");
    if (t.cp) lane_launch<uint32_t>(scope, k_jaro<uint32_t, false>, t, r);
    else if (r.wide) lane_launch<uint8_t>(scope, k_jaro<uint8_t, true>, t, r);
    else lane_launch<uint8_t>(scope, k_jaro<uint8_t, false>, t, r);
}

}  // namespace swh
