// lcs.hip -- the length of the longest common subsequence of every pair and its Indel distance m + n - 2 LCS, the edit distance
// with insertions and deletions only (swh_levenshtein_lcs_*; rapidfuzz distance.LCSseq, distance.Indel, fuzz.ratio).
//
// The bit-vector LCS of Allison-Dix / Crochemore et al. / Hyyro 2004 on osa.hip's layout: the SHORTER string's m symbols are the
// rows (LCS is symmetric; ties go to a), cut into blocks of 32, the longer string's n symbols are the columns. G lanes per pair, one
// per block, floor(64 / G) pairs per wave; the lane of block k works on column s - k in step s. A lane keeps one word V, all ones
// at first; bit i of V is 0 where the LCS length grows from row i to row i + 1 of the column. With Eq the column's match word and
// cin the carry of the block below (0 for block 0):
//     U = V & Eq        S = V + U + cin  (33 bits; cout = bit 32, and U is a subset of V, so cout <= 1)        V' = S | (V & ~Eq)
// The carry is all that crosses a block edge: cout of block k in column j is cin of block k + 1 in the SAME column, which the lane
// above runs one step later, so a lane reads by DPP (wave_shr:1) the carry its neighbour left in the step before. A lane whose
// column is not active in a step advances neither V nor its carry. Rows past m have Eq = 0 and stay 1, so LCS = sum over the pair's
// blocks of popcount(~V) with no mask at the end; the lane of the last block collects the sum in G - 1 more wave_shr:1 steps (G is
// no power of two) and writes the results.
//
// The layout's shared text is bp_lanes.hpp's BpLanes. Work items: osa.hip's k_osa_sizes measures the pairs and cuts them
// (launch_osa_sizes, OsaTapes / LaneItem / OsaSizes), the shorter
// string at most SWH_LCS_MAX_SHORTER = SWH_OSA_MAX_SHORTER symbols. The same kernel serves the pairwise calls and, in slices of
// whole rows, the cross-products. The bound only clamps the Indel distance.
#include "lcs.hpp"
#include "bp_lanes.hpp"

namespace swh {

static_assert(SWH_LCS_MAX_SHORTER == SWH_OSA_MAX_SHORTER, "the work items are cut by k_osa_sizes");

template <typename Sym, bool kWide>
__global__ void __launch_bounds__(BpTraits<Sym>::kWaves * 64, BpTraits<Sym>::kMinWavesPerSimd) k_lcs(OsaTapes t, LcsRun run) {
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
        const uint32_t last = lane_blocks(m) - 1;   // the block whose lane collects the pair's count
        const bool keeper = have && blk == last;
        const uint32_t columns = (have && m) ? n : 0;
        // lanes that start a pair take no carry
        const bool first_blk = blk == 0;
        uint32_t keep_mask = first_blk ? 0u : 0xFFFFFFFFu;
        asm volatile("" : "+v"(keep_mask));   // opaque, so that the splice stays one v_and (bp_item)

        uint32_t v = 0xFFFFFFFFu;
        // wave-uniform step count (lane `blk` of a pair works in steps blk .. columns + blk - 1)
        const uint32_t n_eff = wave_max_u32(columns ? columns + last : 0);
        if (n_eff) {   // (so both tapes hold symbols: the clamped windows below have something to read)
            const uint32_t steps = (n_eff + 15) & ~15u;
            typename Lanes::Window pat, txt;
            pat.init((const Sym *)(a_is_rows ? t.a.data : t.b.data), a_is_rows ? a0 : b0, a_is_rows ? a_total : b_total);
            txt.init((const Sym *)(a_is_rows ? t.b.data : t.a.data), a_is_rows ? b0 : a0, a_is_rows ? b_total : a_total);
            lanes.fetch_text(txt, 0 - (int)blk);
            lanes.build_tables(pat, blk * 32, columns ? m : 0);

            uint32_t carry = 0;   // of my block's addition in my last column: 0 or 1
            auto column = [&](uint32_t eq, uint32_t s) {
                const uint32_t cin = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)carry, 0x138, 0xf, 0xf, true) & keep_mask;
                if (s - blk < columns) {
                    const uint64_t sum = (uint64_t)v + (v & eq) + cin;
                    carry = (uint32_t)(sum >> 32);
                    v = (uint32_t)__builtin_amdgcn_bitop3_b32((int)(uint32_t)sum, (int)v, (int)eq, 0xF4);  // a | (b & ~c)
                }
            };
            lanes.run(txt, steps, n_eff, blk, column);
        }

        // the pair's LCS length: the blocks' counts, summed towards the lane of the last block (lanes past it hold 0)
        const uint32_t mine = (uint32_t)__popc(~v);
        uint32_t L = mine;
        for (uint32_t k = 1; k < G; ++k)   // wave-uniform
            L = mine + ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)L, 0x138, 0xf, 0xf, true) & keep_mask);
        if (keeper) {
            const uint32_t d = clamp_bound(m + n - 2 * L, run.bound);   // an empty string: L = 0, no columns run
            if (t.nb) {
                const uint64_t row = p / t.nb, at = row * run.stride + (p - row * t.nb) * 8;
                if (run.indel) *(uint64_t *)(run.indel + at) = d;
                if (run.lcs) *(uint64_t *)(run.lcs + at) = L;
            } else {
                if (run.indel) *(uint32_t *)(run.indel + p * run.stride) = d;
                if (run.lcs) *(uint32_t *)(run.lcs + p * run.stride) = L;
            }
        }
    }
}

void launch_lcs(Scope *scope, const OsaTapes &t, const LcsRun &r) {
    if (!r.item_count) return;
    StampGuard guard(scope, t.cp ? "lcs_u32" : "lcs");
    if (t.cp) lane_launch<uint32_t>(scope, k_lcs<uint32_t, false>, t, r);
    else if (r.wide) lane_launch<uint8_t>(scope, k_lcs<uint8_t, true>, t, r);
    else lane_launch<uint8_t>(scope, k_lcs<uint8_t, false>, t, r);
}

}  // namespace swh
