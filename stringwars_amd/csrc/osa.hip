// osa.hip -- optimal-string-alignment distances (restricted Damerau-Levenshtein: a swap of two neighbouring symbols costs one edit, no
// substring is edited twice) of every pair (swh_levenshtein_osa_*).
//
// Hyyro's 2003 transposition form of Myers' bit-vector algorithm on infix.hip's layout: the SHORTER string's m symbols are the rows
// (OSA is symmetric; ties go to a), cut into blocks of 32, the longer string's n symbols are the columns. G lanes per pair, one per
// block, floor(64 / G) pairs per wave; the lane of block k works on column s - k in step s and hands bit 31 of its horizontal
// deltas to the lane above it by DPP (wave_shr:1). The alignment is global: the horizontal delta fed into the top block is +1, and
// the lane of the LAST block follows the score of the bottom row column by column -- it starts at m, every column adds bit
// (m - 1) & 31 of the +1 deltas and subtracts that bit of the -1 deltas -- and writes it after the last column.
//
// The transposition term: row i of column j may also take D[i-2][j-2] + 1 when a[i-1] = b[j-2] and a[i-2] = b[j-1]. With Eq the
// column's match word, Eq' the previous column's and D0' the previous column's diagonal-zero word (bit i: D[i][j-1] = D[i-1][j-2]),
//     t0 = ~D0' & Eq      tr = (t0 << 1 | bit 31 of the block below's t0) & Eq'
// and tr is OR-ed into both the vertical and the horizontal term. So a lane keeps two more words (D0', Eq') and takes one more
// bit from its neighbour: t0's bit 31 belongs to the SAME column, which the lane above runs one step later -- the timing of the
// horizontal deltas' bit 31. A lane whose column is not active in a step advances none of them.
//
// The layout's shared text (tables, prefetch, super-step loop, the sizes kernel's sums and cut) is bp_lanes.hpp's.
// Work items: k_osa_sizes measures the pairs (cells, the first pair whose shorter string is over SWH_OSA_MAX_SHORTER -- errors come
// before any output) and cuts every run of 64 consecutive pairs greedily into items of consecutive pairs: an item takes pairs while
// pairs x G <= 64, G the largest block count among them (lanes past a shorter string idle). The same kernels serve the pairwise
// calls and, in slices of whole rows, the cross-products (OsaTapes). The bound only clamps the result.
#include "osa.hpp"
#include "bp_lanes.hpp"

namespace swh {

// One thread per pair: the sums, the first oversize pair, and (with `items`) the items of each run of 64 pairs (bp_lanes.hpp).
__global__ void __launch_bounds__(256) k_osa_sizes(OsaTapes t, OsaSizes *sizes, LaneItem *items) {
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
        uint32_t m = la <= lb ? la : lb;
        if (m > SWH_OSA_MAX_SHORTER) {
            atomicMin(&sizes->first_oversize, (unsigned long long)i);
            m = SWH_OSA_MAX_SHORTER;   // (the call fails; the items only have to stay well-formed)
        }
        g = lane_blocks(m);
    }
    lds.blocks_of[threadIdx.x >> 6][threadIdx.x & 63] = g;
    if (lane_sizes_sum(lds, sizes, cells, symbols) && blockIdx.x == 0) {
        sizes->a_total = tape_total(t.a, t.a_off64);
        sizes->b_total = tape_total(t.b, t.b_off64);
    }
    lane_cut_run(lds, sizes, items);
}

template <typename Sym, bool kWide>
__global__ void __launch_bounds__(BpTraits<Sym>::kWaves * 64, BpTraits<Sym>::kMinWavesPerSimd) k_osa(OsaTapes t, OsaRun run) {
    using Lanes = BpLanes<Sym, kWide>;
    constexpr int kWaves = BpTraits<Sym>::kWaves, kEntries = BpTraits<Sym>::kEntries;
    // the wave's tables: 8 KB (bytes) or 14 KB (code points) apart, from LDS address 0 -- the layout NibbleTables / GroupTables3 need
    __shared__ __attribute__((aligned(8192))) uint32_t tables[kWaves * kEntries * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Lanes lanes;
    lanes.init(tables + wave * kEntries * 64, lane);
    const uint64_t a_total = tape_total(t.a, t.a_off64), b_total = tape_total(t.b, t.b_off64);

    for (uint64_t item = (uint64_t)blockIdx.x * kWaves + wave; item < run.item_count; item += (uint64_t)gridDim.x * kWaves) {
        const LaneItem it = run.items[item];
        const uint32_t G = it.blocks;
        const uint32_t slot = (uint32_t)lane / G, blk = (uint32_t)lane - slot * G;
        const bool have = slot < it.pairs;
        const uint64_t p = it.first + (have ? slot : 0);
        uint64_t ia, ib, a0, b0;
        uint32_t la, lb;
        lane_pair(t, p, ia, ib);
        tape_extent(t.a, t.a_off64, ia, a0, la);
        tape_extent(t.b, t.b_off64, ib, b0, lb);
        // rows / bits / lanes: the shorter string; columns / steps: the longer one
        const bool a_is_rows = la <= lb;
        const uint32_t m = a_is_rows ? la : lb, n = a_is_rows ? lb : la;
        const uint32_t last = lane_blocks(m) - 1;   // the block whose lane keeps the score
        const bool keeper = have && blk == last;
        const uint32_t columns = (have && m) ? n : 0;

        uint32_t score = m;
        // wave-uniform step count (lane `blk` of a pair works in steps blk .. columns + blk - 1)
        const uint32_t n_eff = wave_max_u32(columns ? columns + last : 0);
        if (n_eff) {   // (so both tapes hold symbols: the clamped windows below have something to read)
            const uint32_t steps = (n_eff + 15) & ~15u;
            typename Lanes::Window pat, txt;
            pat.init((const Sym *)(a_is_rows ? t.a.data : t.b.data), a_is_rows ? a0 : b0, a_is_rows ? a_total : b_total);
            txt.init((const Sym *)(a_is_rows ? t.b.data : t.a.data), a_is_rows ? b0 : a0, a_is_rows ? b_total : a_total);
            lanes.fetch_text(txt, 0 - (int)blk);
            lanes.build_tables(pat, blk * 32, columns ? m : 0);

            // Lanes that start a pair take the boundary instead of a neighbour: a horizontal delta of +1 (the alignment is global) and
            // no transposition bit. The masks are made opaque so that the splice stays plain bitwise ops (bp_item).
            const bool first_blk = blk == 0;
            uint32_t keep_mask = first_blk ? 0u : 0xFFFFFFFFu, first_ph = first_blk ? 0x80000000u : 0u;
            asm volatile("" : "+v"(keep_mask), "+v"(first_ph));
            const uint32_t score_bit = (m - 1) & 31;
            uint32_t pv = 0xFFFFFFFFu, mv = 0, ph = 0, mh = 0;
            uint32_t t0 = 0, d0_prev = 0xFFFFFFFFu, eq_prev = 0;   // the transposition state: this column's t0, the previous column's D0 and Eq
            auto column = [&](uint32_t eq, uint32_t s) {
                uint32_t ph_in = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ph, 0x138, 0xf, 0xf, true);
                uint32_t mh_in = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mh, 0x138, 0xf, 0xf, true);
                uint32_t tr_in = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)t0, 0x138, 0xf, 0xf, true);
                ph_in = (uint32_t)__builtin_amdgcn_bitop3_b32((int)ph_in, (int)keep_mask, (int)first_ph, 0xEA);  // (a & b) | c
                mh_in = mh_in & keep_mask;
                tr_in = tr_in & keep_mask;
                if (s - blk < columns) {
                    t0 = eq & ~d0_prev;   // the raw eq: before the -1 delta from above is OR-ed in
                    const uint32_t tr = __builtin_amdgcn_alignbit(t0, tr_in, 31) & eq_prev;  // (t0 << 1) | the block below's bit 31
                    eq_prev = eq;
                    uint32_t xv = eq | mv | tr;
                    eq |= mh_in >> 31;
                    uint32_t xh = ((((eq & pv) + pv) ^ pv) | eq) | tr;
                    d0_prev = xh | mv;
                    ph = mv | ~(xh | pv);
                    mh = pv & xh;
                    // the bottom row's score in this column (meaningful on the lane of the last block)
                    score += (ph >> score_bit) & 1u;
                    score -= (mh >> score_bit) & 1u;
                    uint32_t ph_s = __builtin_amdgcn_alignbit(ph, ph_in, 31);  // (ph << 1) | hin(+1)
                    uint32_t mh_s = __builtin_amdgcn_alignbit(mh, mh_in, 31);  // (mh << 1) | hin(-1)
                    pv = mh_s | ~(xv | ph_s);
                    mv = ph_s & xv;
                }
            };
            lanes.run(txt, steps, n_eff, blk, column);
        }

        if (keeper) {
            const uint32_t d = clamp_bound(m ? score : n, run.bound);   // an empty string: the other one's length, no columns run
            if (t.nb) {
                const uint64_t row = p / t.nb;
                *(uint64_t *)(run.out + row * run.stride + (p - row * t.nb) * 8) = d;
            } else {
                *(uint32_t *)(run.out + p * run.stride) = d;
            }
        }
    }
}

void launch_osa_sizes(Scope *scope, const OsaTapes &t, OsaSizes *sizes, LaneItem *items) {
    StampGuard guard(scope, "osa_sizes");
    hipLaunchKernelGGL(k_osa_sizes, dim3((uint32_t)((t.count + 255) / 256)), dim3(256), 0, scope->stream, t, sizes, items);
    SWH_HIP_CHECK(hipGetLastError());
}

void launch_osa(Scope *scope, const OsaTapes &t, const OsaRun &r) {
    if (!r.item_count) return;
    StampGuard guard(scope, t.cp ? "osa_u32" : "osa");
    if (t.cp) lane_launch<uint32_t>(scope, k_osa<uint32_t, false>, t, r);
    else if (r.wide) lane_launch<uint8_t>(scope, k_osa<uint8_t, true>, t, r);
    else lane_launch<uint8_t>(scope, k_osa<uint8_t, false>, t, r);
}

}  // namespace swh
