// infix.hip -- Levenshtein infix search: the best approximate occurrence of every pattern in its text (swh_levenshtein_infix_*).
//
// Myers' bit-vector algorithm in the form it was published for: the pattern's m symbols are the rows, cut into blocks of 32, the text's
// n symbols are the columns, and the horizontal delta fed into the top block is 0 instead of +1 -- an occurrence may start at any
// text position. The layout is bp_item.hpp's: G lanes per pair, one per block, floor(64 / G) pairs per wave; the lane of block k works on text
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
//    from the tapes themselves (a 4-symbol window read at the mirrored place, its symbols swapped), nothing is staged. The same pass
//    applies the bound and writes the three outputs in their final form. At most 2 m^2 cells per pair against the forward pass's m n.
//
// Work items: k_infix_sizes measures the batch (cells, the first pattern over SWH_INFIX_MAX_PATTERN -- errors come before any output)
// and cuts every run of 64 consecutive pairs greedily into items of consecutive pairs: an item takes pairs while pairs x G <= 64,
// G the largest block count among them (lanes past a shorter pattern idle, as bp_item tolerates). Sorting the pairs by block count
// first, as the distance kernels' planner does, is a later optimisation. The bound only clamps the result: a block-level cutoff
// (Ukkonen's, in its semi-global form) is a later optimisation too.
#include "infix.hpp"
#include "bp_item.hpp"

namespace swh {

template <typename Off>
__device__ __forceinline__ void infix_extent(const TapeRef &t, uint64_t i, uint64_t &start, uint32_t &len) {
    const Off *o = (const Off *)t.offsets;
    const Off x0 = o[i], x1 = o[i + 1];
    start = (uint64_t)x0;
    len = extent_length<Off>(x0, x1);
}
__device__ __forceinline__ void infix_extent(const TapeRef &t, uint32_t off64, uint64_t i, uint64_t &start, uint32_t &len) {
    if (off64) infix_extent<uint64_t>(t, i, start, len);
    else infix_extent<uint32_t>(t, i, start, len);
}
__device__ __forceinline__ uint32_t infix_blocks(uint32_t m) { return m ? (m + 31) >> 5 : 1u; }

// One thread per pair, one wave per run of 64 consecutive pairs: the batch's sums (one atomic per workgroup and quantity), the first
// oversize pattern, and the run's items -- cut by the wave's first lane from the block counts the lanes left in LDS.
__global__ void __launch_bounds__(256) k_infix_sizes(InfixTapes t, InfixSizes *sizes, InfixItem *items) {
    __shared__ unsigned long long part[4][2];
    __shared__ uint32_t blocks_of[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long cells = 0, symbols = 0;
    uint32_t g = 0;   // 0: no pair here
    if (i < t.count) {
        uint64_t p0, t0;
        uint32_t m, n;
        infix_extent(t.patterns, t.p_off64, i, p0, m);
        infix_extent(t.texts, t.t_off64, i, t0, n);
        cells = (unsigned long long)m * n;
        symbols = (unsigned long long)m + n;
        if (m > SWH_INFIX_MAX_PATTERN) {
            atomicMin(&sizes->first_oversize, (unsigned long long)i);
            m = SWH_INFIX_MAX_PATTERN;   // (the call fails; the items only have to stay well-formed)
        }
        g = infix_blocks(m);
    }
    blocks_of[wave][lane] = g;
    for (int s = 32; s > 0; s >>= 1) {
        cells += __shfl_xor(cells, s);
        symbols += __shfl_xor(symbols, s);
    }
    if (lane == 0) { part[wave][0] = cells; part[wave][1] = symbols; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) { cells += part[w][0]; symbols += part[w][1]; }
        atomicAdd(&sizes->cells, cells);
        atomicAdd(&sizes->symbols, symbols);
        if (blockIdx.x == 0) sizes->text_symbols = tape_total(t.texts, t.t_off64);
    }
    if (lane == 0 && blocks_of[wave][0]) {
        const uint64_t run_first = (uint64_t)blockIdx.x * blockDim.x + (uint64_t)wave * 64;
        uint32_t in_run = 0;
        while (in_run < 64 && blocks_of[wave][in_run]) ++in_run;
        // the run's items are counted first, then placed with one atomic
        uint32_t count = 0;
        for (uint32_t first = 0; first < in_run; ++count) {
            uint32_t G = blocks_of[wave][first], k = 1;
            while (first + k < in_run) {
                const uint32_t g2 = blocks_of[wave][first + k], widest = g2 > G ? g2 : G;
                if ((k + 1) * widest > 64) break;
                G = widest; ++k;
            }
            first += k;
        }
        InfixItem *out = items + atomicAdd(&sizes->items, (unsigned long long)count);
        for (uint32_t first = 0; first < in_run;) {
            uint32_t G = blocks_of[wave][first], k = 1;
            while (first + k < in_run) {
                const uint32_t g2 = blocks_of[wave][first + k], widest = g2 > G ? g2 : G;
                if ((k + 1) * widest > 64) break;
                G = widest; ++k;
            }
            InfixItem it;
            it.first = run_first + first; it.pairs = k; it.blocks = G;
            *out++ = it;
            first += k;
        }
    }
}

// Four consecutive symbols of a string, in column (or row) order: forward from `idx`; mirrored, the symbols `idx` .. `idx + 3` of the
// string read backwards from `end`, i.e. the window at end - 4 - idx with its symbols swapped.
template <bool kMirror>
__device__ __forceinline__ uint32_t infix_raw4(const ByteWindow &w, int idx, int end, int &shift) {
    return w.fetch4_raw(kMirror ? end - 4 - idx : idx, shift);
}
template <bool kMirror>
__device__ __forceinline__ uint32_t infix_word4(uint32_t raw, int shift) {
    const uint32_t dw = ByteWindow::realign(raw, shift);
    return kMirror ? __builtin_bswap32(dw) : dw;
}
template <bool kMirror>
__device__ __forceinline__ void infix_sym4(const SymWindow32 &w, int idx, int end, uint32_t *out) {
    uint32_t four[4];
    w.fetch4(kMirror ? end - 4 - idx : idx, four);
#pragma unroll
    for (int r = 0; r < 4; ++r) out[r] = four[kMirror ? 3 - r : r];
}

template <typename Sym, bool kMirror, bool kWide>
__global__ void __launch_bounds__(BpTraits<Sym>::kWaves * 64, BpTraits<Sym>::kMinWavesPerSimd) k_infix(InfixTapes t, InfixRun run) {
    static_assert(!(kMirror && kWide), "the start pass reads its short windows word by word");
    constexpr bool kBytes = sizeof(Sym) == 1;
    constexpr int kWaves = BpTraits<Sym>::kWaves, kEntries = BpTraits<Sym>::kEntries;
    // the wave's tables: 8 KB (bytes) or 14 KB (code points) apart, from LDS address 0 -- the layout NibbleTables / GroupTables3 need
    __shared__ __attribute__((aligned(8192))) uint32_t tables[kWaves * kEntries * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *const table = tables + wave * kEntries * 64;
    [[maybe_unused]] NibbleTables nib;
    [[maybe_unused]] GroupTables3 grp;
    if constexpr (kBytes) nib.init(table, lane);
    else grp.init(table, lane);
    const uint64_t p_total = tape_total(t.patterns, t.p_off64), t_total = tape_total(t.texts, t.t_off64);
    using Window = typename std::conditional<kBytes, ByteWindow, SymWindow32>::type;

    for (uint64_t item = (uint64_t)blockIdx.x * kWaves + wave; item < run.item_count; item += (uint64_t)gridDim.x * kWaves) {
        const InfixItem it = run.items[item];
        const uint32_t G = it.blocks;
        const uint32_t slot = (uint32_t)lane / G, blk = (uint32_t)lane - slot * G;
        const bool have = slot < it.pairs;
        const uint64_t p = it.first + (have ? slot : 0);
        uint64_t p0, t0;
        uint32_t m, n;
        infix_extent(t.patterns, t.p_off64, p, p0, m);
        infix_extent(t.texts, t.t_off64, p, t0, n);
        const uint32_t last = infix_blocks(m) - 1;   // the block whose lane keeps the score
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
            Window pat, txt;
            pat.init((const Sym *)t.patterns.data, p0, p_total);
            txt.init((const Sym *)t.texts.data, t0, t_total);

            // text prefetch: 16 symbols per super-step, one super-step ahead (bytes: 4 dwords; code points: 16)
            constexpr int kTextRegs = kBytes ? 4 : 16;
            uint32_t tnxt[kTextRegs];
            int tshift[kBytes ? 4 : 1];
            auto fetch_text = [&](int first) {
                if constexpr (kBytes) {
                    if constexpr (kWide) {
                        tshift[0] = txt.fetch16_raw(first, tnxt);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) tnxt[q] = infix_raw4<kMirror>(txt, first + q * 4, (int)end, tshift[q]);
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 16; q += 4) infix_sym4<kMirror>(txt, first + q, (int)end, tnxt + q);
                }
            };
            fetch_text(0 - (int)blk);

            // ---- the match tables of my block ----
            const uint32_t row0 = blk * 32;
            const uint32_t brows = columns ? (m > row0 ? (m - row0 < 32 ? m - row0 : 32) : 0) : 0;
            const uint32_t row_mask = brows >= 32 ? 0xFFFFFFFFu : ((1u << brows) - 1u);
#pragma unroll
            for (int k = 0; k < kEntries; ++k) table[k * 64 + lane] = 0;
            wave_lds_fence();
            if constexpr (kBytes) {
                uint32_t praw[8];
                int pshift[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) praw[q] = infix_raw4<kMirror>(pat, (int)row0 + q * 4, (int)m, pshift[q]);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    if (brows > (uint32_t)q * 4) {
                        const uint32_t dw = infix_word4<kMirror>(praw[q], pshift[q]);
                        nib.template insert<0>(dw, row_mask & (1u << (q * 4 + 0)));
                        nib.template insert<1>(dw, row_mask & (1u << (q * 4 + 1)));
                        nib.template insert<2>(dw, row_mask & (1u << (q * 4 + 2)));
                        nib.template insert<3>(dw, row_mask & (1u << (q * 4 + 3)));
                    }
                }
            } else {
                uint32_t psym[32];
#pragma unroll
                for (int q = 0; q < 32; q += 4) infix_sym4<kMirror>(pat, (int)row0 + q, (int)m, psym + q);
#pragma unroll
                for (int q = 0; q < 32; ++q)
                    if ((uint32_t)q < brows) grp.insert(psym[q], 1u << q);
            }
            wave_lds_fence();

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
            for (uint32_t s0 = 0; s0 < steps; s0 += 16) {
                uint32_t tcur[kTextRegs];
                if constexpr (kBytes) {
                    if constexpr (kWide) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) tcur[q] = tnxt[q];
                        txt.fix16((int)s0 - (int)blk, tshift[0], tcur);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) tcur[q] = infix_word4<kMirror>(tnxt[q], tshift[q]);
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < kTextRegs; ++q) tcur[q] = tnxt[q];
                }
                // unconditional: clamped addresses are always readable (bp_item)
                fetch_text((int)s0 + 16 - (int)blk);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t gs = s0 + q * 4;
                    if (gs >= n_eff) break;  // wave-uniform: no lane has a symbol left in this group
                    uint32_t eqs[4];
                    if constexpr (kBytes) {
                        eqs[0] = nib.template lookup<0>(tcur[q]);
                        eqs[1] = nib.template lookup<1>(tcur[q]);
                        eqs[2] = nib.template lookup<2>(tcur[q]);
                        eqs[3] = nib.template lookup<3>(tcur[q]);
                    } else {
#pragma unroll
                        for (int u = 0; u < 4; ++u) eqs[u] = grp.lookup(tcur[q * 4 + u]);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) column(eqs[u], gs + u);
                }
            }
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

void launch_infix_sizes(Scope *scope, const InfixTapes &t, InfixSizes *sizes, InfixItem *items) {
    StampGuard guard(scope, "infix_sizes");
    hipLaunchKernelGGL(k_infix_sizes, dim3((uint32_t)((t.count + 255) / 256)), dim3(256), 0, scope->stream, t, sizes, items);
    SWH_HIP_CHECK(hipGetLastError());
}

template <typename Sym, bool kMirror, bool kWide>
static void infix_launch(Scope *scope, const InfixTapes &t, const InfixRun &r) {
    constexpr int kWaves = BpTraits<Sym>::kWaves;
    const uint64_t blocks = std::min<uint64_t>((r.item_count + kWaves - 1) / kWaves, 1u << 22);
    hipLaunchKernelGGL((k_infix<Sym, kMirror, kWide>), dim3((uint32_t)blocks), dim3(kWaves * 64), 0, scope->stream, t, r);
    SWH_HIP_CHECK(hipGetLastError());
}

void launch_infix_forward(Scope *scope, const InfixTapes &t, const InfixRun &r) {
    if (!r.item_count) return;
    StampGuard guard(scope, t.cp ? "infix_u32" : "infix");
    if (t.cp) infix_launch<uint32_t, false, false>(scope, t, r);
    else if (r.wide_text) infix_launch<uint8_t, false, true>(scope, t, r);
    else infix_launch<uint8_t, false, false>(scope, t, r);
}

void launch_infix_starts(Scope *scope, const InfixTapes &t, const InfixRun &r) {
    if (!r.item_count) return;
    StampGuard guard(scope, t.cp ? "infix_starts_u32" : "infix_starts");
    if (t.cp) infix_launch<uint32_t, true, false>(scope, t, r);
    else infix_launch<uint8_t, true, false>(scope, t, r);
}

}  // namespace swh
