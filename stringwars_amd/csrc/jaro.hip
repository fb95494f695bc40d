// jaro.hip -- the counts behind the Jaro and Jaro-Winkler similarities of every pair (swh_levenshtein_jaro_*; rapidfuzz
// distance.Jaro / distance.JaroWinkler, jellyfish jaro_similarity / jaro_winkler_similarity).
//
// The definition (stringwars_amd.h has it in full): with a of m symbols and b of n, R = max(0, max(m, n) / 2 - 1); a's symbols are
// taken in order, and a[i] matches the smallest j in [i - R, i + R] with b[j] == a[i] that no earlier symbol of a has flagged. M is
// the number of matches, h the number of k < M at which the k-th matched symbol of a differs from the k-th flagged symbol of b,
// t = h / 2, and the prefix is the common prefix of at most four symbols. The definition is one-sided -- a drives, b is flagged --
// and the kernel never swaps the sides of a pair: b's n symbols are the rows, cut into blocks of 32, a's m symbols are the columns.
//
// lcs.hip's layout: G lanes per pair, one per block of b, floor(64 / G) pairs per wave; the lane of block k works on column
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
#include "bp_item.hpp"

namespace swh {

static_assert(SWH_JARO_MAX_LENGTH == 2048u, "one wave's 64 blocks of 32 rows; the wave's buffer of matched symbols");
constexpr uint32_t kJaroBuffer = 2048;   // matched symbols of a per wave: its pairs flag at most 64 x 32 rows

template <typename Off>
__device__ __forceinline__ void jaro_extent(const TapeRef &t, uint64_t i, uint64_t &start, uint32_t &len) {
    const Off *o = (const Off *)t.offsets;
    const Off x0 = o[i], x1 = o[i + 1];
    start = (uint64_t)x0;
    len = extent_length<Off>(x0, x1);
}
__device__ __forceinline__ void jaro_extent(const TapeRef &t, uint32_t off64, uint64_t i, uint64_t &start, uint32_t &len) {
    if (off64) jaro_extent<uint64_t>(t, i, start, len);
    else jaro_extent<uint32_t>(t, i, start, len);
}
__device__ __forceinline__ uint32_t jaro_blocks(uint32_t n) { return n ? (n + 31) >> 5 : 1u; }
// the strings of the launch's pair p
__device__ __forceinline__ void jaro_pair(const OsaTapes &t, uint64_t p, uint64_t &ia, uint64_t &ib) {
    if (t.nb) { const uint64_t row = p / t.nb; ia = t.row0 + row; ib = p - row * t.nb; }
    else { ia = p; ib = p; }
}

// One thread per pair, one wave per run of 64 consecutive pairs: the sums (one atomic per workgroup and quantity), the first pair
// with an oversize string, and (with `items`) the run's items -- cut by the wave's first lane from the block counts the lanes left
// in LDS.
__global__ void __launch_bounds__(256) k_jaro_sizes(OsaTapes t, OsaSizes *sizes, OsaItem *items) {
    __shared__ unsigned long long part[4][2];
    __shared__ uint32_t blocks_of[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long cells = 0, symbols = 0;
    uint32_t g = 0;   // 0: no pair here
    if (i < t.count) {
        uint64_t ia, ib, a0, b0;
        uint32_t la, lb;
        jaro_pair(t, i, ia, ib);
        jaro_extent(t.a, t.a_off64, ia, a0, la);
        jaro_extent(t.b, t.b_off64, ib, b0, lb);
        cells = (unsigned long long)la * lb;
        symbols = (unsigned long long)la + lb;
        if (la > SWH_JARO_MAX_LENGTH || lb > SWH_JARO_MAX_LENGTH) {
            atomicMin(&sizes->first_oversize, (unsigned long long)i);
            if (lb > SWH_JARO_MAX_LENGTH) lb = SWH_JARO_MAX_LENGTH;   // (the call fails; the items only have to stay well-formed)
        }
        g = jaro_blocks(lb);
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
        if (blockIdx.x == 0) { sizes->a_total = tape_total(t.a, t.a_off64); sizes->b_total = tape_total(t.b, t.b_off64); }
    }
    if (items && lane == 0 && blocks_of[wave][0]) {
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
        OsaItem *out = items + atomicAdd(&sizes->items, (unsigned long long)count);
        for (uint32_t first = 0; first < in_run;) {
            uint32_t G = blocks_of[wave][first], k = 1;
            while (first + k < in_run) {
                const uint32_t g2 = blocks_of[wave][first + k], widest = g2 > G ? g2 : G;
                if ((k + 1) * widest > 64) break;
                G = widest; ++k;
            }
            OsaItem it;
            it.first = run_first + first; it.pairs = k; it.blocks = G;
            *out++ = it;
            first += k;
        }
    }
}

template <typename Sym, bool kWide>
__global__ void __launch_bounds__(BpTraits<Sym>::kWaves * 64, BpTraits<Sym>::kMinWavesPerSimd) k_jaro(OsaTapes t, JaroRun run) {
    constexpr bool kBytes = sizeof(Sym) == 1;
    static_assert(kBytes || !kWide, "128-bit reads of the columns' string are a byte-tape variant");
    constexpr int kWaves = BpTraits<Sym>::kWaves, kEntries = BpTraits<Sym>::kEntries;
    // the wave's tables: 8 KB (bytes) or 14 KB (code points) apart, from LDS address 0 -- the layout NibbleTables / GroupTables3 need
    __shared__ __attribute__((aligned(8192))) uint32_t tables[kWaves * kEntries * 64];
    // the matched symbols of a, pair by pair in a's order: 2 KB (bytes) or 8 KB (code points) per wave
    __shared__ Sym matched_of[kWaves * kJaroBuffer];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *const table = tables + wave * kEntries * 64;
    Sym *const matched = matched_of + wave * kJaroBuffer;
    [[maybe_unused]] NibbleTables nib;
    [[maybe_unused]] GroupTables3 grp;
    if constexpr (kBytes) nib.init(table, lane);
    else grp.init(table, lane);
    const uint64_t a_total = tape_total(t.a, t.a_off64), b_total = tape_total(t.b, t.b_off64);
    using Window = typename std::conditional<kBytes, ByteWindow, SymWindow32>::type;

    for (uint64_t item = (uint64_t)blockIdx.x * kWaves + wave; item < run.item_count; item += (uint64_t)gridDim.x * kWaves) {
        const OsaItem it = run.items[item];
        const uint32_t G = it.blocks;
        const uint32_t slot = (uint32_t)lane / G, blk = (uint32_t)lane - slot * G;
        const bool have = slot < it.pairs;
        const uint64_t p = it.first + (have ? slot : 0);
        uint64_t ia, ib, a0, b0;
        uint32_t m, n;
        jaro_pair(t, p, ia, ib);
        jaro_extent(t.a, t.a_off64, ia, a0, m);
        jaro_extent(t.b, t.b_off64, ib, b0, n);
        // rows / bits / lanes: b, whichever is longer; columns / steps: a
        const uint32_t longer = m > n ? m : n;
        const int R = longer >= 4 ? (int)(longer / 2 - 1) : 0;
        const uint32_t last = jaro_blocks(n) - 1;   // the block whose lane sees a column's final found bit
        const bool keeper = have && blk == last;
        const uint32_t columns = (have && m && n) ? (m < n + (uint32_t)R ? m : n + (uint32_t)R) : 0;
        // lanes that start a pair take no found bit
        const bool first_blk = blk == 0;
        uint32_t keep_mask = first_blk ? 0u : 0xFFFFFFFFu;
        asm volatile("" : "+v"(keep_mask));   // opaque, so that the splice stays one v_and (bp_item)
        // the pair's slice of the wave's buffer: its G blocks flag at most 32 G rows, and slot * 32 G + 32 G <= 2048
        const uint32_t slice = slot * G * 32;
        const uint32_t row0 = blk * 32;
        const uint32_t brows = columns ? (n > row0 ? (n - row0 < 32 ? n - row0 : 32) : 0) : 0;

        uint32_t flags = 0, rank = 0, prefix = 0;
        // wave-uniform step count (lane `blk` of a pair works in steps blk .. columns + blk - 1)
        const uint32_t n_eff = wave_max_u32(columns ? columns + last : 0);
        if (n_eff) {   // (so both tapes hold symbols: the clamped windows below have something to read)
            const uint32_t steps = (n_eff + 15) & ~15u;
            Window pat, txt;
            pat.init((const Sym *)t.b.data, b0, b_total);
            txt.init((const Sym *)t.a.data, a0, a_total);

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
                        for (int q = 0; q < 4; ++q) tnxt[q] = txt.fetch4_raw(first + q * 4, tshift[q]);
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 16; q += 4) {
                        uint32_t four[4];
                        txt.fetch4(first + q, four);
#pragma unroll
                        for (int r = 0; r < 4; ++r) tnxt[q + r] = four[r];
                    }
                }
            };
            fetch_text(0 - (int)blk);

            // ---- the match tables of my block, and the common prefix of the pair's first four symbols ----
            const uint32_t row_mask = brows >= 32 ? 0xFFFFFFFFu : ((1u << brows) - 1u);
            const uint32_t shorter = m < n ? m : n, prefix_max = shorter < 4 ? shorter : 4;
#pragma unroll
            for (int k = 0; k < kEntries; ++k) table[k * 64 + lane] = 0;
            wave_lds_fence();
            if constexpr (kBytes) {
                uint32_t praw[8];
                int pshift[8], ashift, bshift;
#pragma unroll
                for (int q = 0; q < 8; ++q) praw[q] = pat.fetch4_raw((int)row0 + q * 4, pshift[q]);
                const uint32_t a4 = txt.fetch4_raw(0, ashift), b4 = pat.fetch4_raw(0, bshift);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    if (brows > (uint32_t)q * 4) {
                        const uint32_t dw = ByteWindow::realign(praw[q], pshift[q]);
                        nib.template insert<0>(dw, row_mask & (1u << (q * 4 + 0)));
                        nib.template insert<1>(dw, row_mask & (1u << (q * 4 + 1)));
                        nib.template insert<2>(dw, row_mask & (1u << (q * 4 + 2)));
                        nib.template insert<3>(dw, row_mask & (1u << (q * 4 + 3)));
                    }
                }
                // (bytes past a string's end are whatever follows it: prefix_max cuts them off)
                const uint32_t differ = ByteWindow::realign(a4, ashift) ^ ByteWindow::realign(b4, bshift);
                prefix = differ ? (uint32_t)(__ffs((int)differ) - 1) >> 3 : 4u;
            } else {
                uint32_t psym[32];
#pragma unroll
                for (int q = 0; q < 32; q += 4) {
                    uint32_t four[4];
                    pat.fetch4((int)row0 + q, four);
#pragma unroll
                    for (int r = 0; r < 4; ++r) psym[q + r] = four[r];
                }
                uint32_t a4[4], b4[4];
                txt.fetch4(0, a4);
                pat.fetch4(0, b4);
#pragma unroll
                for (int q = 0; q < 32; ++q)
                    if ((uint32_t)q < brows) grp.insert(psym[q], 1u << q);
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
            for (uint32_t s0 = 0; s0 < steps; s0 += 16) {
                uint32_t tcur[kTextRegs];
                if constexpr (kBytes) {
                    if constexpr (kWide) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) tcur[q] = tnxt[q];
                        txt.fix16((int)s0 - (int)blk, tshift[0], tcur);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) tcur[q] = ByteWindow::realign(tnxt[q], tshift[q]);
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
                    uint32_t eqs[4], syms[4];
                    if constexpr (kBytes) {
                        eqs[0] = nib.template lookup<0>(tcur[q]);
                        eqs[1] = nib.template lookup<1>(tcur[q]);
                        eqs[2] = nib.template lookup<2>(tcur[q]);
                        eqs[3] = nib.template lookup<3>(tcur[q]);
#pragma unroll
                        for (int u = 0; u < 4; ++u) syms[u] = tcur[q] >> (8 * u);   // (the store keeps the low byte)
                    } else {
#pragma unroll
                        for (int u = 0; u < 4; ++u) { eqs[u] = grp.lookup(tcur[q * 4 + u]); syms[u] = tcur[q * 4 + u]; }
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) column(eqs[u], gs + u, syms[u]);
                }
            }
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
            uint32_t bsym[kBytes ? 8 : 32];
            if constexpr (kBytes) {
                int pshift[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) bsym[q] = pat.fetch4_raw((int)row0 + q * 4, pshift[q]);
#pragma unroll
                for (int q = 0; q < 8; ++q) bsym[q] = ByteWindow::realign(bsym[q], pshift[q]);
            } else {
#pragma unroll
                for (int q = 0; q < 32; q += 4) {
                    uint32_t four[4];
                    pat.fetch4((int)row0 + q, four);
#pragma unroll
                    for (int r = 0; r < 4; ++r) bsym[q + r] = four[r];
                }
            }
            uint32_t at = slice + upto - mine;   // where my lowest flagged row's partner lies
#pragma unroll
            for (int q = 0; q < 32; ++q) {
                if ((q & 3) == 0 && (uint32_t)q >= rows_eff) break;   // wave-uniform
                const uint32_t flagged = (flags >> q) & 1u;
                const uint32_t theirs = (uint32_t)matched[at & (kJaroBuffer - 1)];
                uint32_t ours;
                if constexpr (kBytes) ours = (bsym[q >> 2] >> (8 * (q & 3))) & 0xFFu;
                else ours = bsym[q];
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

void launch_jaro_sizes(Scope *scope, const OsaTapes &t, OsaSizes *sizes, OsaItem *items) {
    StampGuard guard(scope, "jaro_sizes");
    hipLaunchKernelGGL(k_jaro_sizes, dim3((uint32_t)((t.count + 255) / 256)), dim3(256), 0, scope->stream, t, sizes, items);
    SWH_HIP_CHECK(hipGetLastError());
}

template <typename Sym, bool kWide>
static void jaro_launch(Scope *scope, const OsaTapes &t, const JaroRun &r) {
    constexpr int kWaves = BpTraits<Sym>::kWaves;
    const uint64_t blocks = std::min<uint64_t>((r.item_count + kWaves - 1) / kWaves, 1u << 22);
    hipLaunchKernelGGL((k_jaro<Sym, kWide>), dim3((uint32_t)blocks), dim3(kWaves * 64), 0, scope->stream, t, r);
    SWH_HIP_CHECK(hipGetLastError());
}

void launch_jaro(Scope *scope, const OsaTapes &t, const JaroRun &r) {
    if (!r.item_count) return;
    StampGuard guard(scope, t.cp ? "jaro_u32" : "jaro");
    if (t.cp) jaro_launch<uint32_t, false>(scope, t, r);
    else if (r.wide) jaro_launch<uint8_t, true>(scope, t, r);
    else jaro_launch<uint8_t, false>(scope, t, r);
}

}  // namespace swh
