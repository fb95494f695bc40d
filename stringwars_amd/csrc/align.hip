// align.hip -- Levenshtein alignments: the canonical edit script of every pair (swh_levenshtein_align_*).
//
// One lane per pair. The pattern -- the longer of the two strings, so that the stored bits stay near two per cell -- is cut
// into blocks of 32 rows; the lane sweeps the text, the shorter string, once per block with the
// Myers / Hyyro step (the block's match table in the wave's LDS: nibble tables for bytes, 3-bit group tables for code
// points, as in the distance kernels), feeding each block the horizontal deltas of the block above from that block's
// stored bottom scores. Per block and column it stores the vertical delta vectors Pv / Mv (8 bytes per 32 cells) and,
// for every block but the last, the score of the block's bottom row (4 bytes). Any D(i, j) the walk needs is then
//     D(i, j) = score at the top of i's block + popcount(Pv_j & mask_i) - popcount(Mv_j & mask_i)
// The same lane walks back from (m, n) over its own stores (no hand-off) with the canonical rule of the C ABI:
// '=' on equal symbols, else 'X' if the diagonal gives D, else 'D' if the cell above does, else 'I' -- in (a, b) terms,
// reading D(i, j) of a transposed pair as D^T(j, i) (the matrix is symmetric under swapping the strings).
// The ops come out back to front and are written from the end of the pair's slot, so they sit there in forward order;
// k_align_emit moves them to their compact place once the counts are scanned (scan.hip).
#include "align.hpp"
#include "bp_lanes.hpp"   // the offset reader

namespace swh {

constexpr int kAlignWaves = 4;
constexpr uint32_t kAlignRun = 16;   // columns of the forward pass whose inputs are loaded together

// stored bytes of one pair: Pv / Mv per (pattern block, text column), then the bottom scores of all blocks but the last;
// the pattern is the longer string
__device__ __forceinline__ uint64_t align_store_bytes(uint32_t m, uint32_t n) {
    if (m == 0 || n == 0) return 0;
    const uint32_t rows = m > n ? m : n, columns = m > n ? n : m;
    const uint64_t blocks = (rows + 31) / 32;
    return 8 * blocks * columns + (((4 * (blocks - 1) * columns) + 7) & ~7ull);
}

__global__ void __launch_bounds__(256) k_align_sizes(AlignTapes t, uint64_t *store_base, uint64_t *slot_base, AlignSizes *sizes) {
    // grid-stride, then one atomic per workgroup and quantity (an atomic per wave on four shared words serialised at 1 M pairs)
    __shared__ unsigned long long part[4][4];
    unsigned long long store = 0, symbols = 0, cells = 0, biggest = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < t.count; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t a0, b0;
        uint32_t m, n;
        tape_extent(t.a, t.a_off64, i, a0, m);
        tape_extent(t.b, t.b_off64, i, b0, n);
        const uint64_t bytes = align_store_bytes(m, n), c = (uint64_t)m * n;
        store += bytes;
        symbols += (uint64_t)m + n;
        cells += c;
        biggest = bytes > biggest ? bytes : biggest;
        store_base[i] = bytes;
        slot_base[i] = (uint64_t)m + n;
        if (c > SWH_ALIGN_MAX_CELLS) atomicMin(&sizes->first_oversize, (unsigned long long)i);
    }
    for (int s = 32; s > 0; s >>= 1) {
        store += __shfl_xor(store, s);
        symbols += __shfl_xor(symbols, s);
        cells += __shfl_xor(cells, s);
        const unsigned long long o = __shfl_xor(biggest, s);
        biggest = o > biggest ? o : biggest;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = store; part[wave][1] = symbols; part[wave][2] = cells; part[wave][3] = biggest;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            store += part[w][0]; symbols += part[w][1]; cells += part[w][2];
            biggest = part[w][3] > biggest ? part[w][3] : biggest;
        }
        atomicAdd(&sizes->store_total, store);
        atomicAdd(&sizes->symbols, symbols);
        atomicAdd(&sizes->cells, cells);
        atomicMax(&sizes->max_store, biggest);
    }
}

// ---- the forward pass and the walk ------------------------------------------------------------------------------------------------
template <typename Sym> struct AlignTable;
template <> struct AlignTable<uint8_t> {
    static constexpr int kWords = 32 * 64;   // 16 low-nibble + 16 high-nibble entries x 64 lanes
    NibbleTables t;
    __device__ __forceinline__ void init(uint32_t *table, int lane) { t.init(table, lane); }
    __device__ __forceinline__ void insert(uint32_t c, uint32_t bit) const { t.insert<0>(c, bit); }
    __device__ __forceinline__ uint32_t lookup(uint32_t c) const { return t.lookup<0>(c); }
};
template <> struct AlignTable<uint32_t> {
    static constexpr int kWords = 56 * 64;   // seven groups of eight entries x 64 lanes
    GroupTables3 t;
    __device__ __forceinline__ void init(uint32_t *table, int lane) { t.init(table, lane); }
    __device__ __forceinline__ void insert(uint32_t c, uint32_t bit) const { t.insert(c, bit); }
    __device__ __forceinline__ uint32_t lookup(uint32_t c) const { return t.lookup(c); }
};

template <typename Sym, typename OffA, typename OffB>
__global__ void __launch_bounds__(kAlignWaves * 64) k_align(AlignTapes t, AlignChunk c) {
    // the wave's table: 8 KB (bytes) or 14 KB (code points) apart, from LDS address 0 -- the layout NibbleTables / GroupTables3 need
    __shared__ __attribute__((aligned(8192))) uint32_t tables[kAlignWaves * AlignTable<Sym>::kWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *table = tables + wave * AlignTable<Sym>::kWords;
    AlignTable<Sym> eq;
    eq.init(table, lane);

    const uint64_t p = c.pair_first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= c.pair_end) return;
    uint64_t a0, b0;
    uint32_t m, n;
    tape_extent<OffA>(t.a, p, a0, m);
    tape_extent<OffB>(t.b, p, b0, n);
    const Sym *a = (const Sym *)t.a.data + a0, *b = (const Sym *)t.b.data + b0;
    uint8_t *slot_end = c.slots + c.slot_base[p] + m + n;

    if (m == 0 || n == 0) {   // all insertions or all deletions
        const uint32_t d = m + n;
        c.distances[p] = d <= c.bound ? d : c.bound + 1;
        const uint32_t ops = d <= c.bound ? d : 0;
        for (uint32_t q = 1; q <= ops; ++q) slot_end[-(int64_t)q] = m ? (uint8_t)SWH_OP_DEL : (uint8_t)SWH_OP_INS;
        c.counts[p] = ops;
        return;
    }
    if ((m > n ? m - n : n - m) > c.bound) {   // the length difference alone exceeds the bound
        c.distances[p] = c.bound + 1;
        c.counts[p] = 0;
        return;
    }

    // the pattern (rows) is the longer string, the text (columns) the shorter one
    const bool swapped = m < n;
    const Sym *pat = swapped ? b : a, *txt = swapped ? a : b;
    const uint32_t rows = swapped ? n : m, columns = swapped ? m : n;
    const uint32_t blocks = (rows + 31) / 32;
    uint2 *pm = (uint2 *)(c.store + (c.store_base[p] - c.store_first));   // [block][column - 1]: (Pv, Mv)
    int32_t *bottom = (int32_t *)(pm + (uint64_t)blocks * columns);      // [block][column - 1], blocks 0 .. blocks - 2: D(32 (k + 1), j)

    // ---- forward: one sweep of the text per block of 32 pattern rows ----
    int32_t score = 0;
    for (uint32_t k = 0; k < blocks; ++k) {
        const uint32_t r0 = 32 * k, h = rows - r0 < 32 ? rows - r0 : 32;
        const uint32_t mask = h == 32 ? 0xFFFFFFFFu : (1u << h) - 1;
        for (int e = 0; e < AlignTable<Sym>::kWords / 64; ++e) table[e * 64 + lane] = 0;
        for (uint32_t r = 0; r < h; ++r) eq.insert((uint32_t)pat[r0 + r], 1u << r);
        uint32_t pv = mask, mv = 0;
        score = (int32_t)(r0 + h);
        int32_t above_prev = (int32_t)r0;   // D(r0, j - 1)
        const int32_t *above = k ? bottom + (uint64_t)(k - 1) * columns : nullptr;
        int32_t *below = k + 1 < blocks ? bottom + (uint64_t)k * columns : nullptr;
        uint2 *out = pm + (uint64_t)k * columns;
        const uint32_t high = 1u << (h - 1);
        // the text symbols and the block above's scores in runs of kAlignRun, loaded together: one memory latency per run, not per column
        for (uint32_t j0 = 0; j0 < columns; j0 += kAlignRun) {
            Sym sym[kAlignRun];
            int32_t up[kAlignRun];
#pragma unroll
            for (uint32_t q = 0; q < kAlignRun; ++q) {
                const uint32_t j = j0 + q < columns ? j0 + q : columns - 1;
                sym[q] = txt[j];
                up[q] = above ? above[j] : 0;
            }
#pragma unroll
            for (uint32_t q = 0; q < kAlignRun; ++q) {
                const uint32_t j = j0 + q;
                if (j >= columns) break;
                int32_t hin = 1;
                if (above) {
                    hin = up[q] - above_prev;
                    above_prev = up[q];
                }
                uint32_t e = eq.lookup((uint32_t)sym[q]);
                const uint32_t xv = e | mv;
                if (hin < 0) e |= 1u;
                const uint32_t xh = (((e & pv) + pv) ^ pv) | e;
                uint32_t ph = mv | ~(xh | pv);
                uint32_t mh = pv & xh;
                score += (ph & high) ? 1 : ((mh & high) ? -1 : 0);
                ph <<= 1;
                mh <<= 1;
                if (hin < 0) mh |= 1u;
                else if (hin > 0) ph |= 1u;
                pv = mh | ~(xv | ph);
                mv = ph & xv;
                out[j] = make_uint2(pv & mask, mv & mask);
                if (below) below[j] = score;
            }
        }
    }
    const uint32_t d = (uint32_t)score;
    c.distances[p] = d <= c.bound ? d : c.bound + 1;
    if (d > c.bound) {
        c.counts[p] = 0;
        return;
    }

    // ---- walk back from (m, n) ----
    // D(i, j) in (a, b) terms: row i, column j of the stored matrix, or column i, row j of a transposed pair
    auto cell = [&](uint32_t i, uint32_t j) -> int32_t {
        const uint32_t row = swapped ? j : i, col = swapped ? i : j;
        if (row == 0) return (int32_t)col;
        if (col == 0) return (int32_t)row;
        const uint32_t k = (row - 1) >> 5, r = row - (k << 5);
        const uint32_t mask = r == 32 ? 0xFFFFFFFFu : (1u << r) - 1;
        const int32_t top = k ? bottom[(uint64_t)(k - 1) * columns + (col - 1)] : (int32_t)col;
        const uint2 v = pm[(uint64_t)k * columns + (col - 1)];
        return top + __popc(v.x & mask) - __popc(v.y & mask);
    };
    uint32_t i = m, j = n;
    int32_t cur = (int32_t)d;
    uint8_t *w = slot_end;
    while (i > 0 && j > 0) {
        // every value the step may need is loaded up front: one memory latency per step
        const Sym x = a[i - 1], y = b[j - 1];
        const int32_t diag = cell(i - 1, j - 1), up = cell(i - 1, j);
        uint8_t op;
        if (x == y) {
            op = SWH_OP_MATCH;
            --i; --j;
        } else if (diag + 1 == cur) {
            op = SWH_OP_SUBST;
            --i; --j; cur = diag;
        } else if (up + 1 == cur) {
            op = SWH_OP_DEL;
            --i; cur = up;
        } else {
            op = SWH_OP_INS;
            --j; cur -= 1;
        }
        *--w = op;
    }
    for (; i > 0; --i) *--w = SWH_OP_DEL;
    for (; j > 0; --j) *--w = SWH_OP_INS;
    c.counts[p] = (uint32_t)(slot_end - w);
}

void launch_align_sizes(Scope *scope, const AlignTapes &t, uint64_t *store_base, uint64_t *slot_base, AlignSizes *sizes) {
    StampGuard guard(scope, "align_sizes");
    const uint64_t blocks = std::min<uint64_t>((t.count + 255) / 256, (uint64_t)scope->compute_units * 4);
    hipLaunchKernelGGL(k_align_sizes, dim3((uint32_t)(blocks ? blocks : 1)), dim3(256), 0, scope->stream, t, store_base, slot_base, sizes);
    SWH_HIP_CHECK(hipGetLastError());
}

void launch_align_chunk(Scope *scope, const AlignTapes &t, const AlignChunk &c) {
    const uint64_t pairs = c.pair_end - c.pair_first;
    if (!pairs) return;
    const dim3 grid((uint32_t)((pairs + kAlignWaves * 64 - 1) / (kAlignWaves * 64))), block(kAlignWaves * 64);
    if (t.cp) {
        StampGuard guard(scope, "align_u32");
        hipLaunchKernelGGL((k_align<uint32_t, uint64_t, uint64_t>), grid, block, 0, scope->stream, t, c);
    } else {
        StampGuard guard(scope, "align");
        if (t.a_off64 && t.b_off64) hipLaunchKernelGGL((k_align<uint8_t, uint64_t, uint64_t>), grid, block, 0, scope->stream, t, c);
        else if (t.a_off64) hipLaunchKernelGGL((k_align<uint8_t, uint64_t, uint32_t>), grid, block, 0, scope->stream, t, c);
        else if (t.b_off64) hipLaunchKernelGGL((k_align<uint8_t, uint32_t, uint64_t>), grid, block, 0, scope->stream, t, c);
        else hipLaunchKernelGGL((k_align<uint8_t, uint32_t, uint32_t>), grid, block, 0, scope->stream, t, c);
    }
    SWH_HIP_CHECK(hipGetLastError());
}

// sixteen lanes per pair copy its ops to their compact place
__global__ void __launch_bounds__(256) k_align_emit(uint64_t count, const uint64_t *slot_base, const uint32_t *counts, const uint64_t *offsets,
                                                    const uint8_t *slots, uint8_t *ops) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t p = g >> 4;
    if (p >= count) return;
    const uint32_t q = (uint32_t)(g & 15), len = counts[p];
    const uint8_t *src = slots + slot_base[p + 1] - len;   // the end of pair p's slot is where pair p + 1's begins
    uint8_t *dst = ops + offsets[p];
    for (uint32_t x = q; x < len; x += 16) dst[x] = src[x];
}

void launch_align_emit(Scope *scope, uint64_t count, const uint64_t *slot_base, const uint32_t *counts, const uint64_t *offsets,
                       const uint8_t *slots, uint8_t *ops) {
    StampGuard guard(scope, "align_emit");
    hipLaunchKernelGGL(k_align_emit, dim3((uint32_t)((count * 16 + 255) / 256)), dim3(256), 0, scope->stream, count, slot_base, counts, offsets,
                       slots, ops);
    SWH_HIP_CHECK(hipGetLastError());
}

}  // namespace swh
