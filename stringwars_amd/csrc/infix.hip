// infix.hip -- Levenshtein infix search: the best approximate occurrence of every pattern in its text (swh_levenshtein_infix_*).
//
// Myers' bit-vector algorithm in the form it was published for: the pattern's m symbols are the rows, cut into blocks of 32, the text's
// n symbols are the columns, and the horizontal delta fed into the top block is 0 instead of +1 -- an occurrence may start at any
// text position. The layout is bp_lanes.hpp's, which holds its shared text (BpLanes, the sizes kernel's sums and its cut): G lanes
// per pair, one per block, floor(64 / G) pairs per wave; the lane of block k works on text
// column s - k in step s and hands bit 31 of its horizontal deltas to the lane above it by DPP (wave_shr:1); the match words come
// from the wave's LDS tables (nibble tables for bytes, 3-bit group tables for code points), the text is prefetched one super-step of
// 16 symbols ahead. What differs from bp_item: the pattern is always the rows (no bp_pattern_is_a), there is no popcount epilogue,
// and the lane of the pattern's LAST block follows the score of the bottom row column by column -- it starts at m, every column
// adds bit (m - 1) & 31 of the +1 deltas and subtracts that bit of the -1 deltas -- and keeps its first minimum and where it ends.
//
// Two passes run the same column code (k_infix<Sym, kMirror, kWide>):
//  - forward (kMirror = false): the whole text, top delta 0; leaves d_i and the smallest end e_i that reaches it.
//  - start (kMirror = true), only for pairs with d_i <= bound and e_i > 0: an occurrence that ends at e has at most m + d symbols, so
//    the reversed pattern is aligned GLOBALLY (top delta +1) against the reversed t[e - w .. e), w = min(e, m + d), and the first
//    column j whose bottom score is d gives start = e - j: the shortest occurrence that ends at e. Both strings are read mirrored
//    from the tapes themselves (BpLanes' kMirror: a 4-symbol window read at the mirrored place, its symbols swapped), nothing is
//    staged. The same pass
//    applies the bound and writes the three outputs in their final form. At most 2 m^2 cells per pair against the forward pass's m n.
//
// Work items: k_infix_sizes measures the batch (cells, the first pattern over SWH_INFIX_MAX_PATTERN -- errors come before any output)
// and cuts every run of 64 consecutive pairs greedily into items of consecutive pairs: an item takes pairs while pairs x G <= 64,
// G the largest block count among them (lanes past a shorter pattern idle, as bp_item tolerates). Sorting the pairs by block count
// first, as the distance kernels' planner does, is a later optimisation. The bound only clamps the result: a block-level cutoff
// (Ukkonen's, in its semi-global form) is a later optimisation too.
#include "infix.hpp"
#include "bp_lanes.hpp"

namespace swh {

// One thread per pair: the batch's sums, the first oversize pattern, and the items of each run of 64 pairs (bp_lanes.hpp).
__global__ void __launch_bounds__(256) k_infix_sizes(InfixTapes t, InfixSizes *sizes, LaneItem *items) {
    __shared__ LaneSizesLds lds;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long cells = 0, symbols = 0;
    uint32_t g = 0;   // 0: no pair here
    if (i < t.count) {
        uint64_t p0, t0;
        uint32_t m, n;
        tape_extent(t.patterns, t.p_off64, i, p0, m);
        tape_extent(t.texts, t.t_off64, i, t0, n);
        cells = (unsigned long long)m * n;
        symbols = (unsigned long long)m + n;
        if (m > SWH_INFIX_MAX_PATTERN) {
            atomicMin(&sizes->first_oversize, (unsigned long long)i);
            m = SWH_INFIX_MAX_PATTERN;   // (the call fails; the items only have to stay well-formed)
        }
        g = lane_blocks(m);
    }
    lds.blocks_of[threadIdx.x >> 6][threadIdx.x & 63] = g;
    if (lane_sizes_sum(lds, sizes, cells, symbols) && blockIdx.x == 0) sizes->text_symbols = tape_total(t.texts, t.t_off64);
    lane_cut_run(lds, sizes, items);
}

template <typename Sym, bool kMirror, bool kWide>
__global__ void __launch_bounds__(BpTraits<Sym>::kWaves * 64, BpTraits<Sym>::kMinWavesPerSimd) k_infix(InfixTapes t, InfixRun run) {
    using Lanes = BpLanes<Sym, kWide, kMirror>;
    constexpr int kWaves = BpTraits<Sym>::kWaves, kEntries = BpTraits<Sym>::kEntries;
    // the wave's tables: 8 KB (bytes) or 14 KB (code points) apart, from LDS address 0 -- the layout NibbleTables / GroupTables3 need
    __shared__ __attribute__((aligned(8192))) uint32_t tables[kWaves * kEntries * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Lanes lanes;
    lanes.init(tables + wave * kEntries * 64, lane);
    const uint64_t p_total = tape_total(t.patterns, t.p_off64), t_total = tape_total(t.texts, t.t_off64);

    for (uint64_t item = (uint64_t)blockIdx.x * kWaves + wave; item < run.item_count; item += (uint64_t)gridDim.x * kWaves) {
        const LaneItem it = run.items[item];
        const uint32_t G = it.blocks;
        const uint32_t slot = (uint32_t)lane / G, blk = (uint32_t)lane - slot * G;
        const bool have = slot < it.pairs;
        const uint64_t p = it.first + (have ? slot : 0);
        uint64_t p0, t0;
        uint32_t m, n;
        tape_extent(t.patterns, t.p_off64, p, p0, m);
        tape_extent(t.texts, t.t_off64, p, t0, n);
        const uint32_t last = lane_blocks(m) - 1;   // the block whose lane keeps the score
        const bool keeper = have && blk == last;

        // columns this pair runs: the text (forward), or the w symbols in front of its end (start pass, pairs within the bound)
        uint32_t columns = m ? n : 0, d = 0, end = 0;
        bool over = false;
        if constexpr (kMirror) {
            d = run.distances[p];
            end = run.ends[p];
            over = run.bound != SWH_UNBOUNDED && d > run.bound;
            columns = (!over && end > 0) ? (end < m + d ? end : m + d) : 0;
        }
        if (!have) columns = 0;

        uint32_t score = m, best = kMirror ? d + 1 : m, best_end = 0;
        // wave-uniform step count (lane `blk` of a pair works in steps blk .. columns + blk - 1)
        const uint32_t n_eff = wave_max_u32(columns ? columns + last : 0);
        if (n_eff) {   // (so both tapes hold symbols: the clamped windows below have something to read)
            const uint32_t steps = (n_eff + 15) & ~15u;
            typename Lanes::Window pat, txt;
            pat.init((const Sym *)t.patterns.data, p0, p_total);
            txt.init((const Sym *)t.texts.data, t0, t_total);
            lanes.fetch_text(txt, 0 - (int)blk, (int)end);
            lanes.build_tables(pat, blk * 32, columns ? m : 0, (int)m);

            // Lanes that start a pair take the boundary's horizontal delta instead of a neighbour's: 0 when the occurrence may start
            // anywhere, +1 in the anchored start pass. The masks are made opaque so that the splice stays two plain bitwise ops (bp_item).
            const bool first_blk = blk == 0;
            uint32_t keep_mask = first_blk ? 0u : 0xFFFFFFFFu, first_ph = (kMirror && first_blk) ? 0x80000000u : 0u;
            asm volatile("" : "+v"(keep_mask), "+v"(first_ph));
            const uint32_t score_bit = (m - 1) & 31;
            uint32_t pv = 0xFFFFFFFFu, mv = 0, ph = 0, mh = 0;
            auto column = [&](uint32_t eq, uint32_t s) {
                uint32_t ph_in = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ph, 0x138, 0xf, 0xf, true);
                uint32_t mh_in = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mh, 0x138, 0xf, 0xf, true);
                ph_in = (uint32_t)__builtin_amdgcn_bitop3_b32((int)ph_in, (int)keep_mask, (int)first_ph, 0xEA);  // (a & b) | c
                mh_in = mh_in & keep_mask;
                if (s - blk < columns) {
                    uint32_t xv = eq | mv;
                    eq |= mh_in >> 31;
                    uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
                    ph = mv | ~(xh | pv);
                    mh = pv & xh;
                    // the bottom row's score in this column (meaningful on the lane of the pattern's last block), its first minimum and
                    // the end that goes with it: this lane's column index + 1
                    score += (ph >> score_bit) & 1u;
                    score -= (mh >> score_bit) & 1u;
                    if (score < best) { best = score; best_end = s - blk + 1; }
                    uint32_t ph_s = __builtin_amdgcn_alignbit(ph, ph_in, 31);  // (ph << 1) | hin(+1)
                    uint32_t mh_s = __builtin_amdgcn_alignbit(mh, mh_in, 31);  // (mh << 1) | hin(-1)
                    pv = mh_s | ~(xv | ph_s);
                    mv = ph_s & xv;
                }
            };
            lanes.run(txt, steps, n_eff, blk, column, (int)end);
        }

        if (keeper) {
            if constexpr (!kMirror) {
                run.distances[p] = best;
                run.ends[p] = best_end;
            } else if (over) {
                run.distances[p] = run.bound + 1;
                run.starts[p] = SWH_INFIX_NONE;
                run.ends[p] = SWH_INFIX_NONE;
            } else {
                run.starts[p] = columns ? end - best_end : 0u;
            }
        }
    }
}

void launch_infix_sizes(Scope *scope, const InfixTapes &t, InfixSizes *sizes, LaneItem *items) {
    StampGuard guard(scope, "infix_sizes");
    hipLaunchKernelGGL(k_infix_sizes, dim3((uint32_t)((t.count + 255) / 256)), dim3(256), 0, scope->stream, t, sizes, items);
    SWH_HIP_CHECK(hipGetLastError());
}

void launch_infix_forward(Scope *scope, const InfixTapes &t, const InfixRun &r) {
    if (!r.item_count) return;
    StampGuard guard(scope, t.cp ? "infix_u32" : "infix");
    if (t.cp) lane_launch<uint32_t>(scope, k_infix<uint32_t, false, false>, t, r);
    else if (r.wide_text) lane_launch<uint8_t>(scope, k_infix<uint8_t, false, true>, t, r);
    else lane_launch<uint8_t>(scope, k_infix<uint8_t, false, false>, t, r);
}

void launch_infix_starts(Scope *scope, const InfixTapes &t, const InfixRun &r) {
    if (!r.item_count) return;
    StampGuard guard(scope, t.cp ? "infix_starts_u32" : "infix_starts");
    if (t.cp) lane_launch<uint32_t>(scope, k_infix<uint32_t, true, false>, t, r);
    else lane_launch<uint8_t>(scope, k_infix<uint8_t, true, false>, t, r);
}

}  // namespace swh
