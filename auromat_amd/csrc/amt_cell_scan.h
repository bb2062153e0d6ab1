// Pixels sorted into cells: what the counting sorts of amt_median.hip (keys per cell) and amt_nearest.hip (pixel indices per
// cell) share.  Both count with one atomic per run of equal cells in a wave (run_of), scan the counts (cell_scan) and fill
// through a cursor; the count and fill bodies stay with their files (pixels per lane, payload, cell rule and member view differ).
#pragma once

#include "amt_common.h"

namespace {

using namespace amt;

// Runs of consecutive lanes with the same cell: for every lane the first lane of its run, and the number of
// pixels of the run before this lane (excl) and in all of it (total); cnt: this lane's pixels.  Called by the whole wave.
struct lane_run {
    int head;
    unsigned excl, total;
};

__device__ __forceinline__ lane_run run_of(int cell, unsigned cnt, int lane) {
    unsigned incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    const int prev = __shfl_up(cell, 1);
    const bool is_head = lane == 0 || prev != cell;
    const unsigned long long heads = __ballot(is_head);
    const unsigned long long upto = heads & (~0ull >> (63 - lane));
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    lane_run r;
    r.head = 63 - __clzll(upto);
    const int last = above ? lane + __ffsll((long long)above) - 1 : 63;
    const unsigned before_run = __shfl(incl, r.head) - __shfl(cnt, r.head);
    r.excl = incl - cnt - before_run;
    r.total = __shfl(incl, last) - before_run;
    return r;
}

// ---- exclusive scan of the counts: offset[0..cells], offset[cells] = number of binned pixels ----
constexpr int kScanItems = 8;           // cells per thread of the scan
constexpr int kScanTile = kBlock * kScanItems;

// workgroups of the scan, and the block sums it needs: cell_scan_blocks(cells) + 1 words
inline int cell_scan_blocks(int64_t cells) { return (int)((cells + kScanTile - 1) / kScanTile); }

__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned* sWave, unsigned& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    if (lane == 63) sWave[wave] = incl;
    __syncthreads();
    unsigned before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
        before += w < wave ? sWave[w] : 0u;
        total += sWave[w];
    }
    __syncthreads();
    return before + incl - v;
}

__global__ __launch_bounds__(kBlock) void k_cell_scan_sums(const unsigned* __restrict__ count, int64_t cells,
                                                          unsigned* __restrict__ bsum) {
    __shared__ unsigned sWave[kBlock / 64];
    const int64_t b0 = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    unsigned s = 0;
#pragma unroll
    for (int q = 0; q < kScanItems; ++q) s += b0 + q < cells ? count[b0 + q] : 0u;
    unsigned total;
    (void)block_excl_scan(s, sWave, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the nb block sums in place, bsum[nb] = the grand total
__global__ __launch_bounds__(kBlock) void k_cell_scan_blocks(unsigned* __restrict__ bsum, int nb) {
    __shared__ unsigned sWave[kBlock / 64];
    unsigned carry = 0;
    for (int base = 0; base < nb; base += kBlock) {
        const int i = base + threadIdx.x;
        const unsigned v = i < nb ? bsum[i] : 0u;
        unsigned total;
        const unsigned e = block_excl_scan(v, sWave, total);
        if (i < nb) bsum[i] = carry + e;
        carry += total;
    }
    if (threadIdx.x == 0) bsum[nb] = carry;
}

__global__ __launch_bounds__(kBlock) void k_cell_scan_apply(const unsigned* __restrict__ count, int64_t cells,
                                                           const unsigned* __restrict__ bsum, int nb,
                                                           unsigned* __restrict__ offset) {
    __shared__ unsigned sWave[kBlock / 64];
    const int64_t b0 = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    unsigned v[kScanItems], s = 0;
#pragma unroll
    for (int q = 0; q < kScanItems; ++q) {
        v[q] = b0 + q < cells ? count[b0 + q] : 0u;
        s += v[q];
    }
    unsigned total;
    unsigned run = bsum[blockIdx.x] + block_excl_scan(s, sWave, total);
#pragma unroll
    for (int q = 0; q < kScanItems; ++q) {
        if (b0 + q < cells) offset[b0 + q] = run;
        run += v[q];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) offset[cells] = bsum[nb];
}

// offset[0 .. cells] from count[0 .. cells) on the context's stream; bsum: cell_scan_blocks(cells) + 1 words of scratch
inline void cell_scan(amt_ctx* ctx, const unsigned* count, int64_t cells, unsigned* bsum, unsigned* offset) {
    const int nb = cell_scan_blocks(cells);
    hipLaunchKernelGGL(k_cell_scan_sums, dim3(nb), dim3(kBlock), 0, ctx->stream, count, cells, bsum);
    hipLaunchKernelGGL(k_cell_scan_blocks, dim3(1), dim3(kBlock), 0, ctx->stream, bsum, nb);
    hipLaunchKernelGGL(k_cell_scan_apply, dim3(nb), dim3(kBlock), 0, ctx->stream, count, cells, bsum, nb, offset);
}

}  // namespace
