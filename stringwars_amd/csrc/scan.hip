// scan.hip -- the offsets scan (scan.hpp). k_offsets_sums leaves a sum per tile of 4096 values; in k_offsets_scan every tile adds up
// the sums before it and scans itself: within the wave by shuffles, across the four waves through LDS. Two plain launches: no
// workgroup waits for another.
#include "scan.hpp"

namespace swh {

constexpr int kScanThreads = 256;
constexpr int kScanPerThread = (int)(kScanTile / kScanThreads);   // 16 consecutive values per thread

__device__ __forceinline__ uint64_t scan_block_sum(unsigned long long v, uint64_t *wave_sums) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
    __syncthreads();
    return wave_sums[0] + wave_sums[1] + wave_sums[2] + wave_sums[3];
}

template <typename In>
__global__ __launch_bounds__(kScanThreads) void k_offsets_sums(const In *counts, uint64_t n, uint64_t *block_sums) {
    __shared__ uint64_t wave_sums[4];
    const uint64_t first = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPerThread;
    uint64_t mine = 0;
#pragma unroll
    for (int j = 0; j < kScanPerThread; ++j) mine += first + j < n ? counts[first + j] : In(0);
    const uint64_t sum = scan_block_sum(mine, wave_sums);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = sum;
}

// Tile t: the sums of the tiles before it, then its own exclusive scan. starts[i] for every count (if wanted); row_offsets[r] =
// the start of count r * slices and row_offsets[rows] = the total, written by whoever holds count n - 1. Every count of the thread is
// in registers before its first store: `row_offsets` may be `counts`. (kStarts is a template flag: as a test of the pointer it cost the
// kernel 19 VGPRs and a wave per SIMD.)
template <typename In, bool kStarts>
__global__ __launch_bounds__(kScanThreads) void k_offsets_scan(const In *counts, uint64_t n, uint32_t slices, const uint64_t *block_sums, uint64_t *starts,
                                                                uint64_t *row_offsets) {
    __shared__ uint64_t wave_sums[4];
    __shared__ uint64_t wave_scan[4];
    uint64_t before = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += kScanThreads) before += block_sums[b];
    const uint64_t base = scan_block_sum(before, wave_sums);
    const uint64_t first = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPerThread;
    In c[kScanPerThread];
    uint64_t mine = 0;
#pragma unroll
    for (int j = 0; j < kScanPerThread; ++j) {
        c[j] = first + j < n ? counts[first + j] : In(0);
        mine += c[j];
    }
    // exclusive scan of the threads' sums: within the wave by shuffles, across the four waves through LDS
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long other = __shfl_up(incl, off);
        if (lane >= (uint32_t)off) incl += other;
    }
    if (lane == 63) wave_scan[wave] = incl;
    __syncthreads();
    uint64_t at = base + incl - mine;
    for (uint32_t w = 0; w < wave; ++w) at += wave_scan[w];
#pragma unroll
    for (int j = 0; j < kScanPerThread; ++j) {
        const uint64_t i = first + j;
        if (i < n) {
            if constexpr (kStarts) starts[i] = at;
            if (slices == 1) row_offsets[i] = at;
            else if (i % slices == 0) row_offsets[i / slices] = at;
            if (i == n - 1) row_offsets[n / slices] = at + c[j];
        }
        at += c[j];
    }
}

template <typename In>
void launch_offsets_scan(Scope *scope, const In *counts, uint64_t rows, uint32_t slices, const ScanScratch &scratch, uint64_t *starts,
                         uint64_t *row_offsets) {
    const uint64_t n = rows * slices;
    // No caller comes here: within_run (both paths), extract_within_run and infix_all_run answer a call without rows first, token_derive
    // and token_set_run return before token_pack, and align_run returns before its three scans.
    if (n == 0) {
        SWH_HIP_CHECK(hipMemsetAsync(row_offsets, 0, 8, scope->stream));
        return;
    }
    const dim3 grid((uint32_t)ScanScratch::tiles(n)), block(kScanThreads);
    {
        StampGuard guard(scope, "offsets_sums");
        hipLaunchKernelGGL(k_offsets_sums<In>, grid, block, 0, scope->stream, counts, n, scratch.block_sums);
        SWH_HIP_CHECK(hipGetLastError());
    }
    StampGuard guard(scope, "offsets_scan");
    const auto kernel = starts ? k_offsets_scan<In, true> : k_offsets_scan<In, false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, scope->stream, counts, n, slices, (const uint64_t *)scratch.block_sums, starts, row_offsets);
    SWH_HIP_CHECK(hipGetLastError());
}
template void launch_offsets_scan<uint32_t>(Scope *, const uint32_t *, uint64_t, uint32_t, const ScanScratch &, uint64_t *, uint64_t *);
template void launch_offsets_scan<uint64_t>(Scope *, const uint64_t *, uint64_t, uint32_t, const ScanScratch &, uint64_t *, uint64_t *);

}  // namespace swh
