// partial.hip -- the partial ratio of every pair: the best Indel ratio of the shorter string (the needle p, m symbols) against the
// windows of the longer one (the haystack t, n symbols) (swh_levenshtein_partial_*; rapidfuzz fuzz.partial_ratio,
// fuzz.partial_ratio_alignment). include/stringwars_amd.h states the contract: window w, 0 <= w < n + m - 1, has the offset
// o = w - (m - 1) and is t[max(0, o) .. min(n, o + m)), l symbols; it scores L / (m + l), L = LCS(p, window), compared exactly by
// cross-multiplication; among equals the smallest offset wins; with m == n both directions are run and the second wins only on a
// strictly larger rational.
//
// The kernel is lcs.hip's on bp_lanes.hpp's layout with the slots of a wave given to windows of ONE pair: the needle's rows are cut
// into G = lane_blocks(m) blocks of 32, a slot of G lanes runs one window, floor(64 / G) windows run per pass. Every slot builds the
// needle's tables once per item; per pass a slot points its text window at its own window of the haystack (`columns` = l), V restarts
// at all ones, and the recurrence, the carry hand-off by DPP and the popcount reduction are k_lcs's. After a pass the slot's keeper
// lane compares (L, l, w) with the best it holds in registers; after the last pass the slots' bests are folded in slot order and
// lane 0 writes the item's record.
//
// Work items (partial.hpp): k_partial_sizes measures the pairs as k_osa_sizes does (cells, symbols, the first pair whose shorter
// string is over SWH_PARTIAL_MAX_NEEDLE) and gives every (pair, direction) ceil((n + m - 1) / partial_item_windows(m)) items of
// consecutive windows -- counted in a first launch, which sizes the scratch, placed in a second. A pair's items are consecutive, first
// direction first, windows ascending; where the pairs' runs lie in the list depends on the order of the waves' atomics, which nothing
// reads: k_partial_merge walks each pair's records in their own order with the strict rule, so the same bytes come out of every run.
#include "partial.hpp"
#include "bp_lanes.hpp"

namespace swh {

// What the sizes, item and merge kernels agree on about a pair of la x lb symbols.
struct PartialPlan {
    uint32_t m, n;        // needle, haystack
    uint32_t side;        // of the first direction: 0 -- the needle is a; 1 -- the needle is b (la > lb)
    uint32_t dirs;        // directions run: 0 (an empty or oversize needle), 1, or 2 (la == lb)
    uint32_t per_dir;     // items of a direction
    uint32_t per_item;    // windows of every item but a direction's last
};
__device__ __forceinline__ PartialPlan partial_plan(uint32_t la, uint32_t lb) {
    PartialPlan p;
    p.side = la > lb ? 1u : 0u;
    p.m = p.side ? lb : la; p.n = p.side ? la : lb;
    p.dirs = (p.m == 0 || p.m > SWH_PARTIAL_MAX_NEEDLE) ? 0u : (la == lb ? 2u : 1u);
    p.per_item = partial_item_windows(p.m);
    p.per_dir = p.dirs ? (p.n + p.m - 1 + p.per_item - 1) / p.per_item : 0u;   // (strings hold fewer than 2^30 symbols, kStringLimit)
    return p;
}
// a better window: a larger L / (m + l)
__device__ __forceinline__ bool partial_better(uint32_t m, uint32_t L, uint32_t len, uint32_t best_L, uint32_t best_len) {
    return (uint64_t)L * (m + best_len) > (uint64_t)best_L * (m + len);
}

// the parts of the launch's scratch (partial_scratch_bytes)
struct PartialScratch {
    uint64_t *pair_first;
    PartialItem *items;
    PartialRecord *records;
};
static PartialScratch partial_scratch(void *scratch, uint64_t pairs, uint64_t items) {
    char *at = (char *)scratch;
    PartialScratch s;
    s.pair_first = (uint64_t *)at; at += partial_pad(pairs * 8);
    s.items = (PartialItem *)at; at += partial_pad(items * sizeof(PartialItem));
    s.records = (PartialRecord *)at;
    return s;
}

// One thread per pair: the sums, the first oversize pair, the pair's item count; with `items` (room for `capacity`) also its items.
__global__ void __launch_bounds__(256) k_partial_sizes(OsaTapes t, OsaSizes *sizes, uint64_t *pair_first, PartialItem *items, uint64_t capacity) {
    __shared__ LaneSizesLds lds;
    const int lane = threadIdx.x & 63;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long cells = 0, symbols = 0, count = 0;
    PartialPlan plan = partial_plan(0, 0);
    if (i < t.count) {
        uint64_t ia, ib, a0, b0;
        uint32_t la, lb;
        lane_pair(t, i, ia, ib);
        tape_extent(t.a, t.a_off64, ia, a0, la);
        tape_extent(t.b, t.b_off64, ib, b0, lb);
        cells = (unsigned long long)la * lb;
        symbols = (unsigned long long)la + lb;
        plan = partial_plan(la, lb);
        if (plan.m > SWH_PARTIAL_MAX_NEEDLE) atomicMin(&sizes->first_oversize, (unsigned long long)i);   // (the call fails: no items)
        count = (unsigned long long)plan.dirs * plan.per_dir;
    }
    if (lane_sizes_sum(lds, sizes, cells, symbols) && blockIdx.x == 0) {
        sizes->a_total = tape_total(t.a, t.a_off64);
        sizes->b_total = tape_total(t.b, t.b_off64);
    }
    // my wave's items: one atomic, the pairs' runs in pair order behind it
    unsigned long long upto = count;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long below = __shfl_up(upto, d);
        if (lane >= d) upto += below;
    }
    unsigned long long base = 0;
    if (lane == 63 && upto) base = atomicAdd(&sizes->items, upto);
    base = __shfl(base, 63);
    if (!items || i >= t.count) return;
    const uint64_t first = base + upto - count;
    pair_first[i] = first;
    if (first + count > capacity) return;   // (the tapes changed since they were counted: the merge finds no record either)
    PartialItem *out = items + first;
    const uint32_t windows = plan.n + plan.m - 1;
    for (uint32_t d = 0; d < plan.dirs; ++d) {
        const uint32_t dir = plan.dirs == 2 ? d : plan.side;
        for (uint32_t k = 0; k < plan.per_dir; ++k) {
            PartialItem it;
            it.pair = i; it.first = k * plan.per_item;
            const uint32_t left = windows - it.first;
            it.windows_dir = (left < plan.per_item ? left : plan.per_item) | dir << 31;
            *out++ = it;
        }
    }
}

template <typename Sym, bool kWide>
__global__ void __launch_bounds__(BpTraits<Sym>::kWaves * 64, BpTraits<Sym>::kMinWavesPerSimd)
k_partial(OsaTapes t, const PartialItem *items, PartialRecord *records, uint64_t item_count) {
    using Lanes = BpLanes<Sym, kWide>;
    constexpr int kWaves = BpTraits<Sym>::kWaves, kEntries = BpTraits<Sym>::kEntries;
    // the wave's tables: 8 KB (bytes) or 14 KB (code points) apart, from LDS address 0 -- the layout NibbleTables / GroupTables3 need
    __shared__ __attribute__((aligned(8192))) uint32_t tables[kWaves * kEntries * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Lanes lanes;
    lanes.init(tables + wave * kEntries * 64, lane);
    const uint64_t a_total = tape_total(t.a, t.a_off64), b_total = tape_total(t.b, t.b_off64);

    for (uint64_t item = (uint64_t)blockIdx.x * kWaves + wave; item < item_count; item += (uint64_t)gridDim.x * kWaves) {
        const PartialItem it = items[item];
        const bool a_is_rows = (it.windows_dir >> 31) == 0;
        uint64_t ia, ib, a0, b0;
        uint32_t la, lb;
        lane_pair(t, it.pair, ia, ib);
        tape_extent(t.a, t.a_off64, ia, a0, la);
        tape_extent(t.b, t.b_off64, ib, b0, lb);
        // rows / bits / lanes: the needle; columns / steps: a window of the haystack
        const uint32_t m = a_is_rows ? la : lb, n = a_is_rows ? lb : la;
        uint32_t best_L = 0, best_len = m, best_w = 0;   // (no window of L = 0 replaces it)
        if (m >= 1 && m <= SWH_PARTIAL_MAX_NEEDLE && n >= m) {   // (as they were counted: anything else has changed since)
            const uint32_t G = lane_blocks(m), slots = 64u / G, last = G - 1;
            const uint32_t slot = (uint32_t)lane / G, blk = (uint32_t)lane - slot * G;
            const bool active = slot < slots, keeper = active && blk == last;
            // lanes that start a window take no carry
            uint32_t keep_mask = blk == 0 ? 0u : 0xFFFFFFFFu;
            asm volatile("" : "+v"(keep_mask));   // opaque, so that the splice stays one v_and (bp_item)
            typename Lanes::Window pat, txt;
            pat.init((const Sym *)(a_is_rows ? t.a.data : t.b.data), a_is_rows ? a0 : b0, a_is_rows ? a_total : b_total);
            lanes.build_tables(pat, blk * 32, active ? m : 0);

            const uint32_t all_windows = n + m - 1, upto = it.first + (it.windows_dir & 0x7FFFFFFFu);
            const uint32_t w_end = upto < all_windows ? upto : all_windows;
            for (uint32_t w0 = it.first; w0 < w_end; w0 += slots) {   // a pass: wave-uniform
                const uint32_t w = w0 + slot;
                const bool have = active && w < w_end;
                // window w = [ws, we) of the haystack: offset o = w - (m - 1), o + m = w + 1
                const uint32_t ws = (have && w >= m - 1) ? w - (m - 1) : 0, we = w + 1 < n ? w + 1 : n;
                const uint32_t columns = have ? we - ws : 0;
                txt.init((const Sym *)(a_is_rows ? t.b.data : t.a.data), (a_is_rows ? b0 : a0) + ws, a_is_rows ? b_total : a_total);
                // wave-uniform step count (lane `blk` of a window works in steps blk .. columns + blk - 1); slot 0 has a window
                const uint32_t n_eff = wave_max_u32(columns ? columns + last : 0);
                const uint32_t steps = (n_eff + 15) & ~15u;
                uint32_t v = 0xFFFFFFFFu, carry = 0;   // carry: of my block's addition in my last column, 0 or 1
                auto column = [&](uint32_t eq, uint32_t s) {
                    const uint32_t cin = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)carry, 0x138, 0xf, 0xf, true) & keep_mask;
                    if (s - blk < columns) {
                        const uint64_t sum = (uint64_t)v + (v & eq) + cin;
                        carry = (uint32_t)(sum >> 32);
                        v = (uint32_t)__builtin_amdgcn_bitop3_b32((int)(uint32_t)sum, (int)v, (int)eq, 0xF4);  // a | (b & ~c)
                    }
                };
                lanes.fetch_text(txt, 0 - (int)blk);
                lanes.run(txt, steps, n_eff, blk, column);

                // the window's LCS length: the blocks' counts, summed towards the lane of the last block
                const uint32_t mine = (uint32_t)__popc(~v);
                uint32_t L = mine;
                for (uint32_t k = 1; k < G; ++k)   // wave-uniform
                    L = mine + ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)L, 0x138, 0xf, 0xf, true) & keep_mask);
                // (a slot's windows ascend from pass to pass: strict improvement keeps the smallest offset)
                if (keeper && have && partial_better(m, L, columns, best_L, best_len)) { best_L = L; best_len = columns; best_w = w; }
            }
            // the slots' bests, folded in slot order on every lane alike: the larger rational, among equals the smaller window
            uint32_t item_L = 0, item_len = m, item_w = 0;
            for (uint32_t s = 0; s < slots; ++s) {
                const int from = (int)(s * G + last);
                const uint32_t L = (uint32_t)__shfl((int)best_L, from), len = (uint32_t)__shfl((int)best_len, from), w = (uint32_t)__shfl((int)best_w, from);
                const uint64_t mine = (uint64_t)L * (m + item_len), held = (uint64_t)item_L * (m + len);
                if (mine > held || (mine == held && L && w < item_w)) { item_L = L; item_len = len; item_w = w; }
            }
            best_L = item_L; best_w = item_w;
        }
        if (lane == 0) {
            PartialRecord rec{0, 0, 0};
            if (best_L) {
                rec.lcs = best_L;
                rec.start = best_w >= m - 1 ? best_w - (m - 1) : 0;
                rec.end = best_w + 1 < n ? best_w + 1 : n;
            }
            records[item] = rec;
        }
    }
}

// One thread per pair: its records in their order (first direction first, windows ascending), a later one only on a strictly
// larger rational.
__global__ void __launch_bounds__(256) k_partial_merge(OsaTapes t, const uint64_t *pair_first, const PartialRecord *records, uint64_t record_count,
                                                       PartialMerge out) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= t.count) return;
    uint64_t ia, ib, a0, b0;
    uint32_t la, lb;
    lane_pair(t, p, ia, ib);
    tape_extent(t.a, t.a_off64, ia, a0, la);
    tape_extent(t.b, t.b_off64, ib, b0, lb);
    const PartialPlan plan = partial_plan(la, lb);
    uint32_t L = 0, start = 0, end = plan.m, side = plan.side;   // no common symbol: window (0, m); an empty needle: (0, 0)
    uint64_t at = plan.dirs ? pair_first[p] : 0;
    if (at + (uint64_t)plan.dirs * plan.per_dir > record_count) at = record_count;   // (the tapes changed since they were counted)
    for (uint32_t d = 0; d < plan.dirs && at < record_count; ++d) {
        for (uint32_t k = 0; k < plan.per_dir; ++k, ++at) {
            const PartialRecord r = records[at];
            if (r.lcs && partial_better(plan.m, r.lcs, r.end - r.start, L, end - start)) {
                L = r.lcs; start = r.start; end = r.end;
                side = plan.dirs == 2 ? d : plan.side;
            }
        }
    }
    char *const where[4] = {out.lcs, out.starts, out.ends, out.sides};
    const uint32_t value[4] = {L, start, end, side};
    uint64_t offset = p * out.stride;
    if (t.nb) {
        const uint64_t row = p / t.nb;
        offset = row * out.stride + (p - row * t.nb) * 8;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!where[k]) continue;
        if (t.nb) *(uint64_t *)(where[k] + offset) = value[k];
        else *(uint32_t *)(where[k] + offset) = value[k];
    }
}

void launch_partial_sizes(Scope *scope, const OsaTapes &t, OsaSizes *sizes, void *scratch, uint64_t capacity) {
    StampGuard guard(scope, "partial_sizes");
    PartialScratch s{};
    if (scratch) s = partial_scratch(scratch, t.count, capacity);
    hipLaunchKernelGGL(k_partial_sizes, dim3((uint32_t)((t.count + 255) / 256)), dim3(256), 0, scope->stream, t, sizes, s.pair_first, s.items, capacity);
    SWH_HIP_CHECK(hipGetLastError());
}

void launch_partial_items(Scope *scope, const OsaTapes &t, void *scratch, uint64_t item_count, bool wide) {
    if (!item_count) return;
    StampGuard guard(scope, t.cp ? "partial_u32" : "partial");
    const PartialScratch s = partial_scratch(scratch, t.count, item_count);
    constexpr uint64_t kMostBlocks = 1u << 22;
    auto launch = [&](auto kernel, int waves) {
        const uint64_t blocks = std::min<uint64_t>((item_count + waves - 1) / waves, kMostBlocks);
        hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(waves * 64), 0, scope->stream, t, (const PartialItem *)s.items, s.records, item_count);
    };
    if (t.cp) launch(k_partial<uint32_t, false>, BpTraits<uint32_t>::kWaves);
    else if (wide) launch(k_partial<uint8_t, true>, BpTraits<uint8_t>::kWaves);
    else launch(k_partial<uint8_t, false>, BpTraits<uint8_t>::kWaves);
    SWH_HIP_CHECK(hipGetLastError());
}

void launch_partial_merge(Scope *scope, const OsaTapes &t, const PartialMerge &r, uint64_t item_count) {
    StampGuard guard(scope, "partial_merge");
    const PartialScratch s = partial_scratch((void *)r.scratch, t.count, item_count);
    hipLaunchKernelGGL(k_partial_merge, dim3((uint32_t)((t.count + 255) / 256)), dim3(256), 0, scope->stream, t, (const uint64_t *)s.pair_first,
                       (const PartialRecord *)s.records, item_count, r);
    SWH_HIP_CHECK(hipGetLastError());
}

}  // namespace swh
