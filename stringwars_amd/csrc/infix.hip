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
//
// The search for EVERY occurrence within a bound (swh_levenshtein_infix_all_*) stands below k_infix: the same items and the same
// walk, run around the offsets scan (scan.hip), with kernels of its own (k_infix_hits, k_infix_hit_items, k_infix_hit_starts).
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

// ---- every occurrence within a bound (swh_levenshtein_infix_all_*) ---------------------------------------------------------------------
// The forward walk again, with the keeper lane applying `select` to the score it follows instead of keeping the first minimum:
// k_infix_hits<Sym, kFill, kWide> counts the hits of every pair (kFill = false) or stores them at the pair's cursor in column order
// (kFill = true); one lane owns a pair, so nothing is atomic and the bytes are the same on every run. k_infix_hit_items cuts the
// stored hits into items of consecutive hits (hits x G <= 64, lane_cut_run's rule) and k_infix_hit_starts<Sym> runs k_infix's
// mirrored anchored pass once per hit. k_infix itself is left as it is: these kernels share InfixBlock among themselves.

// One 32-row block of Myers' column on its lane. `receive` runs on every lane in every step (DPP reads the lane below), `advance`
// only where the lane has a column; afterwards ph / mh are the column's horizontal deltas (bit r: row r of the block).
struct InfixBlock {
    uint32_t keep_mask, first_ph, pv = 0xFFFFFFFFu, mv = 0, ph = 0, mh = 0;
    // The lane that starts a pair takes the boundary's horizontal delta instead of a neighbour's: 0 (an occurrence may start
    // anywhere) or +1 (`anchored`). The masks are made opaque so that the splice stays two plain bitwise ops (bp_item).
    __device__ __forceinline__ void init(bool first_blk, bool anchored) {
        keep_mask = first_blk ? 0u : 0xFFFFFFFFu;
        first_ph = (anchored && first_blk) ? 0x80000000u : 0u;
        asm volatile("" : "+v"(keep_mask), "+v"(first_ph));
    }
    __device__ __forceinline__ void receive(uint32_t &ph_in, uint32_t &mh_in) const {
        ph_in = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ph, 0x138, 0xf, 0xf, true);
        mh_in = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mh, 0x138, 0xf, 0xf, true);
        ph_in = (uint32_t)__builtin_amdgcn_bitop3_b32((int)ph_in, (int)keep_mask, (int)first_ph, 0xEA);  // (a & b) | c
        mh_in = mh_in & keep_mask;
    }
    __device__ __forceinline__ void advance(uint32_t eq, uint32_t ph_in, uint32_t mh_in) {
        const uint32_t xv = eq | mv;
        eq |= mh_in >> 31;
        const uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
        ph = mv | ~(xh | pv);
        mh = pv & xh;
        const uint32_t ph_s = __builtin_amdgcn_alignbit(ph, ph_in, 31);  // (ph << 1) | hin(+1)
        const uint32_t mh_s = __builtin_amdgcn_alignbit(mh, mh_in, 31);  // (mh << 1) | hin(-1)
        pv = mh_s | ~(xv | ph_s);
        mv = ph_s & xv;
    }
};

template <typename Sym, bool kFill, bool kWide>
__global__ void __launch_bounds__(BpTraits<Sym>::kWaves * 64, BpTraits<Sym>::kMinWavesPerSimd) k_infix_hits(InfixTapes t, InfixHitsRun run) {
    using Lanes = BpLanes<Sym, kWide, false>;
    constexpr int kWaves = BpTraits<Sym>::kWaves, kEntries = BpTraits<Sym>::kEntries;
    __shared__ __attribute__((aligned(8192))) uint32_t tables[kWaves * kEntries * 64];   // (k_infix's layout)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Lanes lanes;
    lanes.init(tables + wave * kEntries * 64, lane);
    const uint64_t p_total = tape_total(t.patterns, t.p_off64), t_total = tape_total(t.texts, t.t_off64);
    const uint32_t bound = run.bound, select = run.select;

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
        const uint32_t columns = (have && m) ? n : 0;

        // The keeper's hits so far, and where the fill walk puts them. Only the keeper's numbers mean anything: the other lanes follow
        // a bit of some inner row, count what they like and store nothing.
        uint32_t score = m, hits = 0;
        uint64_t base = 0;
        uint32_t wanted = 0;   // SELECT_BEST, fill walk: the score a hit has
        if constexpr (kFill) {
            if (keeper) {
                base = run.cursors[p];
                if (select == SWH_INFIX_SELECT_BEST) wanted = run.best[p];
            }
        }
        auto emit = [&](uint32_t e, uint32_t v) {
            if constexpr (kFill) {
                const uint64_t at = base + hits;
                if (keeper && at < run.total) { run.ends[at] = e; run.distances[at] = v; }
            }
            ++hits;
        };
        // column 0 of the bottom row: D(0) = m
        uint32_t best = m, at_best = 1;          // SELECT_BEST, count walk: the smallest score so far and the columns that have it
        bool pending = m <= bound;                // SELECT_MINIMA: a descent (from +inf in front of column 0) waits for its ascent
        uint32_t cand_e = 0, cand_v = m;          //   ... the first column of its plateau
        if (select == SWH_INFIX_SELECT_ALL ? m <= bound : (kFill && select == SWH_INFIX_SELECT_BEST && m == wanted)) emit(0, m);

        // wave-uniform step count (lane `blk` of a pair works in steps blk .. columns + blk - 1)
        const uint32_t n_eff = wave_max_u32(columns ? columns + last : 0);
        if (n_eff) {   // (so both tapes hold symbols: the clamped windows below have something to read)
            const uint32_t steps = (n_eff + 15) & ~15u;
            typename Lanes::Window pat, txt;
            pat.init((const Sym *)t.patterns.data, p0, p_total);
            txt.init((const Sym *)t.texts.data, t0, t_total);
            lanes.fetch_text(txt, 0 - (int)blk);
            lanes.build_tables(pat, blk * 32, columns ? m : 0);

            InfixBlock b;
            b.init(blk == 0, false);
            const uint32_t score_bit = (m - 1) & 31;
            // `keep(e, up, down)`: the keeper's rule for end e = column + 1, whose score moved up, down or neither
            auto walk = [&](auto keep) {
                lanes.run(txt, steps, n_eff, blk, [&](uint32_t eq, uint32_t s) {
                    uint32_t ph_in, mh_in;
                    b.receive(ph_in, mh_in);
                    if (s - blk < columns) {
                        b.advance(eq, ph_in, mh_in);
                        const uint32_t up = (b.ph >> score_bit) & 1u, down = (b.mh >> score_bit) & 1u;
                        score += up;
                        score -= down;
                        keep(s - blk + 1, up, down);
                    }
                });
            };
            if (select == SWH_INFIX_SELECT_ALL) {
                walk([&](uint32_t e, uint32_t, uint32_t) { if (score <= bound) emit(e, score); });
            } else if (select == SWH_INFIX_SELECT_BEST) {
                if constexpr (kFill) {
                    walk([&](uint32_t e, uint32_t, uint32_t) { if (score == wanted) emit(e, score); });
                } else {
                    walk([&](uint32_t, uint32_t, uint32_t) {
                        at_best = score < best ? 1u : at_best + (score == best ? 1u : 0u);
                        best = score < best ? score : best;
                    });
                }
            } else {
                // an ascent closes the dip that the last descent opened; a descent opens one (a step moves the score by at most one)
                walk([&](uint32_t e, uint32_t up, uint32_t down) {
                    if (up) {
                        if (pending) emit(cand_e, cand_v);
                        pending = false;
                    }
                    if (down) { pending = score <= bound; cand_e = e; cand_v = score; }
                });
            }
        }

        if (select == SWH_INFIX_SELECT_MINIMA) {
            if (pending) emit(cand_e, cand_v);   // the end of the text closes a dip too
        } else if (have && m == 0) {
            // an empty pattern occurs at every end with distance 0 (no walk: there is no row to follow)
            if constexpr (kFill) {
                if (keeper) for (uint32_t e = 1; e <= n; ++e) emit(e, 0);
            } else {
                hits += n; at_best += n;
            }
        }
        if constexpr (!kFill) {
            if (keeper) {
                if (select == SWH_INFIX_SELECT_BEST) {
                    hits = best <= bound ? at_best : 0u;
                    run.best[p] = best <= bound ? best : 0xFFFFFFFFu;
                }
                run.counts[p] = hits;
            }
        }
    }
}

// One thread per hit: its pair, by bisection of the row offsets, and the items of each run of 64 consecutive hits (bp_lanes.hpp).
__global__ void __launch_bounds__(256) k_infix_hit_items(InfixTapes t, const uint64_t *row_offsets, uint64_t total, InfixSizes *sizes,
                                                         uint64_t *rows, LaneItem *items) {
    __shared__ LaneSizesLds lds;
    const uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t g = 0;   // 0: no hit here
    if (h < total) {
        // the last row that begins at or before h: empty rows in front of it begin there too, and row_offsets[count] = total > h
        uint64_t lo = 0, hi = t.count;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (row_offsets[mid] <= h) lo = mid; else hi = mid - 1;
        }
        rows[h] = lo;
        uint64_t p0;
        uint32_t m;
        tape_extent(t.patterns, t.p_off64, lo, p0, m);
        g = lane_blocks(m);
    }
    lds.blocks_of[threadIdx.x >> 6][threadIdx.x & 63] = g;
    __syncthreads();
    lane_cut_run(lds, sizes, items);
}

template <typename Sym>
__global__ void __launch_bounds__(BpTraits<Sym>::kWaves * 64, BpTraits<Sym>::kMinWavesPerSimd) k_infix_hit_starts(InfixTapes t, InfixHitStartsRun run) {
    using Lanes = BpLanes<Sym, false, true>;
    constexpr int kWaves = BpTraits<Sym>::kWaves, kEntries = BpTraits<Sym>::kEntries;
    __shared__ __attribute__((aligned(8192))) uint32_t tables[kWaves * kEntries * 64];   // (k_infix's layout)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Lanes lanes;
    lanes.init(tables + wave * kEntries * 64, lane);
    const uint64_t p_total = tape_total(t.patterns, t.p_off64), t_total = tape_total(t.texts, t.t_off64);

    for (uint64_t item = (uint64_t)blockIdx.x * kWaves + wave; item < run.item_count; item += (uint64_t)gridDim.x * kWaves) {
        const LaneItem it = run.items[item];   // `first`, `pairs`: hits
        const uint32_t G = it.blocks;
        const uint32_t slot = (uint32_t)lane / G, blk = (uint32_t)lane - slot * G;
        const bool have = slot < it.pairs;
        const uint64_t h = it.first + (have ? slot : 0);
        const uint64_t p = run.rows[h];
        uint64_t p0, t0;
        uint32_t m, n;
        tape_extent(t.patterns, t.p_off64, p, p0, m);
        tape_extent(t.texts, t.t_off64, p, t0, n);
        const uint32_t last = lane_blocks(m) - 1;
        const bool keeper = have && blk == last;
        // An occurrence that ends at `end` has at most m + d symbols. With d = m the empty one at `end` is the shortest: no column.
        const uint32_t d = run.distances[h], end = run.ends[h];
        uint32_t columns = d < m ? (end < m + d ? end : m + d) : 0;
        if (!have) columns = 0;

        uint32_t score = m, best = d + 1, best_end = 0;
        const uint32_t n_eff = wave_max_u32(columns ? columns + last : 0);
        if (n_eff) {
            const uint32_t steps = (n_eff + 15) & ~15u;
            typename Lanes::Window pat, txt;
            pat.init((const Sym *)t.patterns.data, p0, p_total);
            txt.init((const Sym *)t.texts.data, t0, t_total);
            lanes.fetch_text(txt, 0 - (int)blk, (int)end);
            lanes.build_tables(pat, blk * 32, columns ? m : 0, (int)m);

            InfixBlock b;
            b.init(blk == 0, true);
            const uint32_t score_bit = (m - 1) & 31;
            lanes.run(txt, steps, n_eff, blk, [&](uint32_t eq, uint32_t s) {
                uint32_t ph_in, mh_in;
                b.receive(ph_in, mh_in);
                if (s - blk < columns) {
                    b.advance(eq, ph_in, mh_in);
                    score += (b.ph >> score_bit) & 1u;
                    score -= (b.mh >> score_bit) & 1u;
                    if (score < best) { best = score; best_end = s - blk + 1; }   // the first column that reaches d
                }
            }, (int)end);
        }
        if (keeper) run.starts[h] = end - best_end;
    }
}

void launch_infix_hits(Scope *scope, const InfixTapes &t, const InfixHitsRun &r, bool fill) {
    if (!r.item_count) return;
    StampGuard guard(scope, t.cp ? "infix_hits_u32" : "infix_hits");
    if (t.cp) lane_launch<uint32_t>(scope, fill ? k_infix_hits<uint32_t, true, false> : k_infix_hits<uint32_t, false, false>, t, r);
    else if (r.wide_text) lane_launch<uint8_t>(scope, fill ? k_infix_hits<uint8_t, true, true> : k_infix_hits<uint8_t, false, true>, t, r);
    else lane_launch<uint8_t>(scope, fill ? k_infix_hits<uint8_t, true, false> : k_infix_hits<uint8_t, false, false>, t, r);
}

void launch_infix_hit_items(Scope *scope, const InfixTapes &t, const uint64_t *row_offsets, uint64_t total, InfixSizes *sizes, uint64_t *rows,
                            LaneItem *items) {
    StampGuard guard(scope, "infix_hit_items");
    hipLaunchKernelGGL(k_infix_hit_items, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, scope->stream, t, row_offsets, total, sizes, rows, items);
    SWH_HIP_CHECK(hipGetLastError());
}

void launch_infix_hit_starts(Scope *scope, const InfixTapes &t, const InfixHitStartsRun &r) {
    if (!r.item_count) return;
    StampGuard guard(scope, t.cp ? "infix_hit_starts_u32" : "infix_hit_starts");
    if (t.cp) lane_launch<uint32_t>(scope, k_infix_hit_starts<uint32_t>, t, r);
    else lane_launch<uint8_t>(scope, k_infix_hit_starts<uint8_t>, t, r);
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
