// Median binning (auromat_amd.resample.resampleMedian): np.median of every channel over the pixels that
// resample(method='mean') bins into a cell (reference auromat/resample.py:353-357 names the statistic and leaves it
// unbuilt).  Exact and independent of scatter order: every result is an order statistic of the cell's keys.
//
//   k_med_count    cell of every pixel by the membership rule of k_bin_frame (amt_frame_src.h), counts per cell;
//                  a lane takes 4 consecutive pixels and a run of lanes with one cell issues one atomic
//   k_cell_scan_*  exclusive scan of the counts (amt_cell_scan.h: block sums, one workgroup over the sums, block rescan)
//   k_med_fill     scatter of the KEYS into contiguous per-cell segments, one plane per channel: u16 channel values,
//                  elevation as an order-preserving u64 of its float64 bits; positions reserved per run of lanes
//   k_med_small    one wave per cell: outputs of every cell (count, mask, empty cells) and, for cells of <= 64 pixels,
//                  a 64-lane bitonic sort per plane; larger cells are listed for the two tiers below (a large cell's
//                  histograms and tickets are zeroed as it is listed)
//   k_med_medium   one workgroup per cell of <= kLargeMin keys: radix select in LDS (8-bit digits: one pass for u8,
//                  two for u16, eight for the elevation key)
//   k_med_large_*  cells above kLargeMin: the same radix select over many workgroups per cell, digit histograms in
//                  global memory (one launch pair per digit and plane)
// amt_median_frame_async enqueues the same passes without reading anything back: one launch of k_med_medium_walk, whose
// fixed grid walks the device-side list of medium cells, and the large tier as k_med_large_step (one launch per digit
// position, all planes and large cells in it; the last workgroup to finish a cell's histogram picks the digit) and
// k_med_large_last.  Each of them reads the tier sizes from device memory and returns at once when its tier is empty.
// Same bits from both forms of the upper tiers, but neither replaces the other (profiles/REJECTED.md): every workgroup
// of the ticket form visits the large cells one after the other (7 x the time of the launch pairs with 51 large cells),
// and a workgroup of the walk waits for one more load than one of k_med_medium.
// Both tiers select k_lo = (n-1)/2 and get k_hi = n/2 from the same pass: it is k_lo's value when the keys <= that
// value are more than k_hi, else the smallest key above it (one more pass).  Even counts average the two in float64.
// Quantile binning (amt_quantile_frame[_async], auromat_amd.resample.resampleQuantile) is the same code under another rank
// rule (rank_rule below): np.quantile's pair (k, k + 1) of method 'linear' and its lerp (put_quantile) in place of the
// middle pair and its mean.  The count, scan and fill passes run once per call; the small tier sorts a plane once and
// reads every quantile's pair from the sorted lanes, the two upper tiers select once per quantile of the call.
// Median and quantile mosaics (amt_mosaic_median_frames, amt_mosaic_quantile_frames; resampleMosaic(statistic=...)) put another
// front before the same tiers: k_med_count_members and k_med_fill_members run the bodies of the count and fill passes
// (count_wave, fill_wave) over the concatenated pixels of a mosaic's members, one launch each whatever the member count; a
// pixel counts inside its member's window and, under rule 1, where amt_mosaic_frames' election (k_mosaic_select) chose its member.
#include "amt_common.h"
#include "amt_cell_scan.h"
#include "amt_frame_src.h"
#include "amt_mosaic_plan.h"

#include <algorithm>
#include <cmath>

namespace {

using namespace amt;

constexpr int kPPT = 4;                 // consecutive pixels per lane in the count and fill passes
constexpr int kSmallMax = 64;           // cells up to one wave's lanes are sorted in registers
constexpr int kLargeMin = 16384;        // cells above this many keys are spread over several workgroups
constexpr int kChunk = 4096;            // keys per workgroup of the large tier
constexpr int kQuantilesMax = AMT_QUANTILES_MAX;

// The rank rule: which two order statistics of a cell's n >= 1 sorted keys a result is made of (k2 is k or k + 1), and the
// weight g that put_quantile gives them.
//   median:  np.median's middle pair (n-1)/2 and n/2, combined as (a + b) / 2 (put_median; g is not used)
//   else:    np.quantile(..., q) by method 'linear', operation by operation (numpy/lib/_function_base_impl.py: _quantile,
//            _get_indexes, _get_gamma): vi = (n-1) * q in float64, k = floor(vi), g = vi - k; where vi >= n-1 (q = 1,
//            n = 1) both ranks are n-1 and g = vi + 1, NumPy's index -1 for the last value taken literally: the lerp of
//            the equal pair then leaves -0.0 as it is for n = 1 and gives +0.0 otherwise, as np.quantile does
// One function for the device and for the host entry point amt_quantile_rank.
struct rank_pair {
    int64_t k, k2;
    double g;
};

__host__ __device__ inline rank_pair rank_rule(int64_t n, double q, bool median) {
#pragma clang fp contract(off)
    rank_pair r;
    __builtin_assume(n >= 1);
    if (median) {
        // (unsigned shifts: for the 32-bit counts of the kernels these stay 32-bit operations, as they were before this rule)
        r.k = (int64_t)((uint64_t)(n - 1) >> 1);
        r.k2 = (int64_t)((uint64_t)n >> 1);
        r.g = 0.5;
        return r;
    }
    const double top = (double)(n - 1);
    const double vi = top * q;
    const double fl = floor(vi);
    if (vi >= top) {
        r.k = r.k2 = n - 1;
        r.g = vi + 1.0;
    } else {
        r.k = (int64_t)fl;
        r.k2 = r.k + 1;
        r.g = vi - fl;
    }
    return r;
}

struct med_args {
    frame_src S;
    const void* img;
    int nx, ny, nch, img_dtype;
};

__device__ __forceinline__ int64_t pixels_of(const med_args& A) { return (int64_t)A.S.height * A.S.width; }

// Flat cell (iy * nx + ix) of pixel i or -1: the membership of k_bin_frame (pixel_cell, amt_frame_src.h).
__device__ __forceinline__ int flat_cell(const med_args& A, int64_t i) {
    int bx, by;
    return pixel_cell(A.S, i, bx, by) ? (by - 1) * A.nx + (bx - 1) : -1;
}

// order-preserving integer key of a float64 (NaN with the sign bit clear sorts above +inf)
__device__ __forceinline__ unsigned long long elev_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double elev_of_key(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// One lane's 4 pixels as seen by the wave: the cell they share (-1: none valid, or `mixed` when they fall into
// more than one cell) and how many are valid.
struct lane_cells {
    int c[kPPT];
    int cell;
    unsigned cnt;
    bool mixed;
};

__device__ __forceinline__ void summarise(lane_cells& L) {
    L.cell = -1;
    L.cnt = 0;
    L.mixed = false;
#pragma unroll
    for (int j = 0; j < kPPT; ++j) {
        if (L.c[j] < 0) continue;
        if (L.cell < 0) L.cell = L.c[j];
        else if (L.c[j] != L.cell) L.mixed = true;
        L.cnt += 1;
    }
    if (L.mixed) {
        L.cell = -1;
        L.cnt = 0;
    }
}

// ---- the member table of a mosaic (amt_mosaic_median_frames, amt_mosaic_quantile_frames) ----
// The pixel index space of the count and fill passes is the concatenation of the members that have a window: member m's
// pixel i is g0 + i.  Work is handed out in whole workgroups of kBlock * kPPT pixels of ONE member (block_start: the first
// workgroup of every member, n + 1 entries), so a wave only ever sees one member and the run rule below carries over.
struct med_member {
    frame_src S;                        // the member's frame on the common axes
    const void* img;
    int g0;                             // index of pixel 0 in the concatenated space
    cell_window W;                      // window in cells of the common grid (amt_mosaic_plan.h)
};
struct member_table {
    const med_member* __restrict__ members;
    const int* __restrict__ block_start;
    int n;
    const int32_t* source;              // rule 1: the elected member of every OUTPUT cell (k_mosaic_select), else NULL
    int* first;                         // rule 0: the lowest member index present per cell (atomicMin), or NULL
};

// What a wave of the count pass knows beside the frame: nothing (a frame alone), or its member of a mosaic.
struct no_member {};
struct member_view {
    int m;
    cell_window W;
    const int32_t* source;
    int* first;
};

// the cell a pixel counts in: for a member, only inside its window, and under rule 1 only where it was elected
__device__ __forceinline__ int keep_cell(const med_args&, const no_member&, int c) { return c; }
__device__ __forceinline__ int keep_cell(const med_args& A, const member_view& V, int c) {
    if (c < 0) return -1;
    const int iy = c / A.nx, ix = c - iy * A.nx;
    if ((unsigned)(ix - V.W.x0) >= (unsigned)V.W.nx || (unsigned)(iy - V.W.y0) >= (unsigned)V.W.ny) return -1;
    if (V.source && V.source[(int64_t)(A.ny - 1 - iy) * A.nx + ix] != V.m) return -1;
    return c;
}
__device__ __forceinline__ void note_member(const no_member&, int) {}
__device__ __forceinline__ void note_member(const member_view& V, int c) {
    if (V.first) atomicMin(&V.first[c], V.m);
}

// The frame of a member as the kernels' argument: the call's common part A0 with the member's arrays.
__device__ __forceinline__ med_args member_args(const med_args& A0, const med_member& D) {
    med_args A = A0;
    A.S = D.S;
    A.img = D.img;
    return A;
}

// One wave's kPPT * 64 pixels of frame A from pixel `base` on; the frame's pixel 0 is g0 in cell_of.  The body of the count
// pass, shared by the frame kernel and the member-table kernel.  Called by the whole wave.
template <typename VIEW>
__device__ __forceinline__ void count_wave(const med_args& A, const VIEW& V, int64_t base, int64_t g0, int lane, int* cell_of,
                                           unsigned* count) {
    const int64_t i0 = base + (int64_t)lane * kPPT, n = pixels_of(A);
    lane_cells L;
#pragma unroll
    for (int j = 0; j < kPPT; ++j) {
        const int64_t i = i0 + j;
        L.c[j] = i < n ? keep_cell(A, V, flat_cell(A, i)) : -1;
        if (i < n) cell_of[g0 + i] = L.c[j];
    }
    summarise(L);
    if (L.mixed) {
#pragma unroll
        for (int j = 0; j < kPPT; ++j)
            if (L.c[j] >= 0) {
                atomicAdd(&count[L.c[j]], 1u);
                note_member(V, L.c[j]);
            }
    }
    const lane_run r = run_of(L.cell, L.cnt, lane);
    if (r.head == lane && L.cell >= 0 && r.total) {
        atomicAdd(&count[L.cell], r.total);
        note_member(V, L.cell);
    }
}

__global__ __launch_bounds__(kBlock) void k_med_count(med_args A, int* __restrict__ cell_of,
                                                     unsigned* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kBlock * kPPT, n = pixels_of(A);
    // whole waves stay in the loop together (the shuffles need every lane)
    for (int64_t base = (blockIdx.x * (int64_t)kBlock + (threadIdx.x & ~63)) * kPPT; base < n; base += stride)
        count_wave(A, no_member{}, base, 0, lane, cell_of, count);
}

// The count pass over a member table: workgroup blockIdx.x takes kBlock * kPPT pixels of one member.  The member's
// descriptor is copied into registers once (the atomics below may alias the table for all the compiler knows).
__global__ __launch_bounds__(kBlock) void k_med_count_members(med_args A0, member_table T, int* __restrict__ cell_of,
                                                             unsigned* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int m = member_of(T.block_start, T.n, blockIdx.x);
    const med_member D = T.members[m];
    const med_args A = member_args(A0, D);
    const member_view V = {m, D.W, T.source, T.first};
    const int64_t base = ((int64_t)(blockIdx.x - (unsigned)T.block_start[m]) * kBlock + (threadIdx.x & ~63)) * kPPT;
    if (base >= pixels_of(A)) return;                               // (wave-uniform)
    count_wave(A, V, base, D.g0, lane, cell_of, count);
}

// rule 0 of a mosaic: out_source of every cell from the lowest member index the count pass has seen there
__global__ __launch_bounds__(kBlock) void k_med_source(const unsigned* __restrict__ count, const int* __restrict__ first, int nx,
                                                      int ny, int32_t* __restrict__ out_source) {
    const int64_t cells = (int64_t)nx * ny;
    for (int64_t c = blockIdx.x * (int64_t)kBlock + threadIdx.x; c < cells; c += (int64_t)gridDim.x * kBlock) {
        const int iy = (int)(c / nx), ix = (int)(c - (int64_t)iy * nx);
        out_source[(int64_t)(ny - 1 - iy) * nx + ix] = count[c] ? first[c] : -1;
    }
}

// ---- scatter of the keys ----
// One wave's kPPT * 64 pixels of frame A from pixel `base` on (pixel 0 is g0 in cell_of; the key planes are `stride` keys
// apart): the body of the fill pass, shared like count_wave.  Called by the whole wave.
template <typename IMG_T>
__device__ __forceinline__ void fill_wave(const med_args& A, int64_t base, int64_t g0, int64_t stride, int lane,
                                          const int* cell_of, const unsigned* offset, unsigned* cursor, uint16_t* keys16,
                                          unsigned long long* keys64) {
    const IMG_T* img = static_cast<const IMG_T*>(A.img);
    const int64_t i0 = base + (int64_t)lane * kPPT, n = pixels_of(A);
    lane_cells L;
#pragma unroll
    for (int j = 0; j < kPPT; ++j) L.c[j] = i0 + j < n ? cell_of[g0 + i0 + j] : -1;
    summarise(L);
    const lane_run r = run_of(L.cell, L.cnt, lane);
    unsigned first = 0;
    if (r.head == lane && L.cell >= 0 && r.total) first = offset[L.cell] + atomicAdd(&cursor[L.cell], r.total);
    first = __shfl(first, r.head) + r.excl;
#pragma unroll
    for (int j = 0; j < kPPT; ++j) {
        const int c = L.c[j];
        if (c < 0) continue;
        unsigned pos;
        if (L.mixed) pos = offset[c] + atomicAdd(&cursor[c], 1u);
        else pos = first++;
        const int64_t i = i0 + j;
        for (int ch = 0; ch < A.nch; ++ch) keys16[(int64_t)ch * stride + pos] = (uint16_t)img[i * A.nch + ch];
        if (keys64) keys64[pos] = elev_key(A.S.elev[i]);
    }
}

template <typename IMG_T>
__global__ __launch_bounds__(kBlock) void k_med_fill(med_args A, const int* __restrict__ cell_of,
                                                    const unsigned* __restrict__ offset, unsigned* __restrict__ cursor,
                                                    uint16_t* __restrict__ keys16, unsigned long long* __restrict__ keys64) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kBlock * kPPT, n = pixels_of(A);
    for (int64_t base = (blockIdx.x * (int64_t)kBlock + (threadIdx.x & ~63)) * kPPT; base < n; base += stride)
        fill_wave<IMG_T>(A, base, 0, n, lane, cell_of, offset, cursor, keys16, keys64);
}

// The fill pass over a member table (the workgroups of k_med_count_members); total: the pixels of the concatenated space.
template <typename IMG_T>
__global__ __launch_bounds__(kBlock) void k_med_fill_members(med_args A0, member_table T, int64_t total,
                                                            const int* __restrict__ cell_of,
                                                            const unsigned* __restrict__ offset, unsigned* __restrict__ cursor,
                                                            uint16_t* __restrict__ keys16,
                                                            unsigned long long* __restrict__ keys64) {
    const int lane = threadIdx.x & 63;
    const int m = member_of(T.block_start, T.n, blockIdx.x);
    const med_member D = T.members[m];
    const med_args A = member_args(A0, D);
    const int64_t base = ((int64_t)(blockIdx.x - (unsigned)T.block_start[m]) * kBlock + (threadIdx.x & ~63)) * kPPT;
    if (base >= pixels_of(A)) return;                               // (wave-uniform)
    fill_wave<IMG_T>(A, base, D.g0, total, lane, cell_of, offset, cursor, keys16, keys64);
}

// ---- outputs ----
struct out_args {
    int nx, ny, nch, img_dtype, has_elev;
    int64_t n;                          // pixels: stride of the key planes
    const unsigned* count;
    const unsigned* offset;
    const uint16_t* keys16;
    const unsigned long long* keys64;
    double* median;                     // median (ny, nx, nch+1), or quantile (nq, ny, nx, nch+1)
    void* out_img;                      // (ny, nx, nch), or (nq, ny, nx, nch)
    uint8_t* out_mask;
    double* out_count;
    int nq;                             // 0: the median; else the quantiles q[0 .. nq)
    double q[kQuantilesMax];
};

// The kernels below that depend on the statistic are instantiated once per rank rule (QUANT false: the median, which then
// compiles to what it was before the quantiles came: one result, constant ranks, no look at q).
// results per cell and plane, and the ranks of result j for a cell of cnt keys
template <bool QUANT>
__device__ __forceinline__ int stat_count(const out_args& O) { return QUANT ? O.nq : 1; }

template <bool QUANT>
__device__ __forceinline__ rank_pair stat_rank(const out_args& O, int j, unsigned cnt) {
    return rank_rule((int64_t)cnt, QUANT ? O.q[j] : 0.5, !QUANT);
}

__device__ __forceinline__ int64_t out_index(const out_args& O, int cell) {
    const int iy = cell / O.nx, ix = cell - iy * O.nx;
    return (int64_t)(O.ny - 1 - iy) * O.nx + ix;      // rows north to south (resample.py:339-349)
}

// plane p < nch: channel p; p == nch: elevation.  lo / hi: the keys of ranks (n-1)/2 and n/2.
__device__ __forceinline__ void put_median(const out_args& O, int cell, int p, unsigned long long lo, unsigned long long hi) {
    const int64_t o = out_index(O, cell);
    if (p == O.nch) {
        // np.median is np.mean of the middle pair, whose sum starts from +0.0: a pair of -0.0 gives +0.0 (every other pair is
        // untouched: 0.0 + a is a)
        O.median[o * (O.nch + 1) + p] = ((0.0 + elev_of_key(lo)) + elev_of_key(hi)) / 2.0;
        return;
    }
    const double v = ((double)lo + (double)hi) / 2.0;       // np.median: mean of the middle pair in float64
    O.median[o * (O.nch + 1) + p] = v;
    if (O.out_img) {
        if (O.img_dtype == 1) static_cast<uint8_t*>(O.out_img)[o * O.nch + p] = (uint8_t)rint(v);     // half to even
        else static_cast<uint16_t*>(O.out_img)[o * O.nch + p] = (uint16_t)rint(v);
    }
}

// np.quantile's lerp of the keys of ranks k and k2 into result j (numpy/lib/_function_base_impl.py: _lerp), every operation
// rounded on its own.  Always evaluated: a + d * 0 turns -0.0 into +0.0, as NumPy does.  The image: round half to even.
__device__ __forceinline__ void put_quantile(const out_args& O, int cell, int p, int j, unsigned long long lo,
                                             unsigned long long hi, double g) {
#pragma clang fp contract(off)
    const int64_t o = (int64_t)j * O.nx * O.ny + out_index(O, cell);
    const double a = p == O.nch ? elev_of_key(lo) : (double)lo;
    const double b = p == O.nch ? elev_of_key(hi) : (double)hi;
    const double d = b - a;
    double v;
    if (g >= 0.5) {
        const double t = d * (1.0 - g);
        v = b - t;
    } else {
        const double t = d * g;
        v = a + t;
    }
    O.median[o * (O.nch + 1) + p] = v;
    if (p < O.nch && O.out_img) {
        if (O.img_dtype == 1) static_cast<uint8_t*>(O.out_img)[o * O.nch + p] = (uint8_t)rint(v);
        else static_cast<uint16_t*>(O.out_img)[o * O.nch + p] = (uint16_t)rint(v);
    }
}

// result j of plane p from the keys of its two ranks, by the call's statistic
template <bool QUANT>
__device__ __forceinline__ void put_stat(const out_args& O, int cell, int p, int j, unsigned long long lo,
                                         unsigned long long hi, double g) {
    if (!QUANT) put_median(O, cell, p, lo, hi);
    else put_quantile(O, cell, p, j, lo, hi, g);
}

__device__ __forceinline__ int plane_bits(const out_args& O, int p) {
    return p == O.nch ? 64 : (O.img_dtype == 1 ? 8 : 16);
}

__device__ __forceinline__ unsigned long long load_key(const out_args& O, int p, unsigned pos) {
    return p == O.nch ? O.keys64[pos] : (unsigned long long)O.keys16[(int64_t)p * O.n + pos];
}

// ascending bitonic sort of one key per lane over the 64 lanes of a wave
template <typename K>
__device__ __forceinline__ K wave_sort(K key, int lane) {
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const K other = __shfl_xor(key, j);
            const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
            key = keep_min ? (other < key ? other : key) : (other > key ? other : key);
        }
    }
    return key;
}

struct tier_counters {
    unsigned n_medium, n_large, max_large, pad;
};

// One wave per cell: every cell's count and mask, NaN / 0 for empty ones, the median of cells of <= 64 keys; the
// others are appended to the medium or large list.  The wave that lists a large cell also zeroes that cell's digit
// histograms and tickets (nplane * 256 + nplane words from `lclear` on).
template <bool QUANT>
__global__ __launch_bounds__(kBlock) void k_med_small(out_args O, int* __restrict__ medium, int* __restrict__ large,
                                                     tier_counters* __restrict__ tiers, unsigned* __restrict__ lclear) {
    const int lane = threadIdx.x & 63;
    const int64_t cells = (int64_t)O.nx * O.ny;
    const int64_t waves = (int64_t)gridDim.x * (kBlock / 64);
    const int nplane = O.nch + (O.has_elev ? 1 : 0);
    const int nstat = stat_count<QUANT>(O);
    for (int64_t w = blockIdx.x * (int64_t)(kBlock / 64) + (threadIdx.x >> 6); w < cells; w += waves) {
        const int cell = (int)w;
        const unsigned cnt = O.count[cell];
        const int64_t o = out_index(O, cell);
        int listed = -1;
        if (lane == 0) {
            if (O.out_count) O.out_count[o] = (double)cnt;
            if (O.out_mask) O.out_mask[o] = cnt == 0;
            for (int j = 0; j < nstat; ++j) {
                const int64_t oj = j * cells + o;
                if (cnt == 0 || !O.has_elev) O.median[oj * (O.nch + 1) + O.nch] = NAN;
                if (cnt != 0) continue;
                for (int p = 0; p < O.nch; ++p) {
                    O.median[oj * (O.nch + 1) + p] = NAN;
                    if (O.out_img) {
                        if (O.img_dtype == 1) static_cast<uint8_t*>(O.out_img)[oj * O.nch + p] = 0;
                        else static_cast<uint16_t*>(O.out_img)[oj * O.nch + p] = 0;
                    }
                }
            }
            if (cnt > (unsigned)kSmallMax) {
                if (cnt > (unsigned)kLargeMin) {
                    listed = (int)atomicAdd(&tiers->n_large, 1u);
                    large[listed] = cell;
                    atomicMax(&tiers->max_large, cnt);
                } else {
                    medium[atomicAdd(&tiers->n_medium, 1u)] = cell;
                }
            }
        }
        if (cnt > (unsigned)kLargeMin) {                           // (wave-uniform)
            listed = __shfl(listed, 0);
            const int words = nplane * 257;
            for (int q = lane; q < words; q += 64) lclear[(int64_t)listed * words + q] = 0u;
        }
        if (cnt == 0 || cnt > (unsigned)kSmallMax) continue;       // (wave-uniform)
        const unsigned off = O.offset[cell];
        // a plane is sorted once; every result of the call reads its pair from the sorted lanes
        for (int p = 0; p < nplane; ++p) {
            if (p == O.nch) {
                const unsigned long long key = wave_sort(lane < (int)cnt ? O.keys64[off + lane] : ~0ull, lane);
                for (int j = 0; j < nstat; ++j) {
                    const rank_pair r = stat_rank<QUANT>(O, j, cnt);
                    const unsigned long long lo = __shfl(key, (int)r.k), hi = __shfl(key, (int)r.k2);
                    if (lane == 0) put_stat<QUANT>(O, cell, p, j, lo, hi, r.g);
                }
            } else {
                const unsigned key = wave_sort(lane < (int)cnt ? (unsigned)O.keys16[(int64_t)p * O.n + off + lane] : ~0u, lane);
                for (int j = 0; j < nstat; ++j) {
                    const rank_pair r = stat_rank<QUANT>(O, j, cnt);
                    const unsigned lo = __shfl(key, (int)r.k), hi = __shfl(key, (int)r.k2);
                    if (lane == 0) put_stat<QUANT>(O, cell, p, j, lo, hi, r.g);
                }
            }
        }
    }
}

// Adds 1 to h[d] for every active lane; lanes that agree on d (the common case: the high digits of a cell's
// keys are mostly equal) share one LDS / global atomic.  Called by the whole wave.
__device__ __forceinline__ void hist_add(unsigned* h, int d, bool act, int lane) {
    const unsigned long long m = __ballot(act);
    if (!m) return;
    const int first = __builtin_ctzll(m);
    const int d0 = __shfl(d, first);
    if (__ballot(act && d == d0) == m) {
        if (lane == first) atomicAdd(&h[d0], (unsigned)__popcll(m));
    } else if (act) {
        atomicAdd(&h[d], 1u);
    }
}

// The digit of the k-th smallest key (0-based) from a 256-bin histogram; run by one wave.
// below: keys in lower bins; in_bin: keys in the digit's bin.
struct digit_pick {
    int d;
    unsigned below, in_bin;
};

__device__ __forceinline__ digit_pick find_digit(const unsigned* h, unsigned k, int lane) {
    unsigned b[4], s = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        b[q] = h[4 * lane + q];
        s += b[q];
    }
    unsigned incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    const unsigned excl = incl - s;
    const unsigned long long hit = __ballot(excl <= k && k < incl);
    const int src = hit ? __builtin_ctzll(hit) : 63;
    digit_pick r = {0, 0, 0};
    unsigned acc = excl;
    bool found = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (!found && k < acc + b[q]) {
            r.d = 4 * lane + q;
            r.below = acc;
            r.in_bin = b[q];
            found = true;
        }
        acc += b[q];
    }
    r.d = __shfl(r.d, src);
    r.below = __shfl(r.below, src);
    r.in_bin = __shfl(r.in_bin, src);
    return r;
}

// does `key` share the digits above bit `shift + 8` with `prefix`?
__device__ __forceinline__ bool prefix_match(unsigned long long key, unsigned long long prefix, int shift) {
    return shift + 8 >= 64 || (key >> (shift + 8)) == (prefix >> (shift + 8));
}

// Radix select of the first rank per plane and result in LDS for one cell, by the whole workgroup.
template <bool QUANT>
__device__ __forceinline__ void medium_cell(const out_args& O, int cell, unsigned* sHist, digit_pick& sPick,
                                            unsigned long long& sMin) {
    const int lane = threadIdx.x & 63;
    const unsigned cnt = O.count[cell], off = O.offset[cell];
    const int nplane = O.nch + (O.has_elev ? 1 : 0);
    const int nstat = stat_count<QUANT>(O);
    for (int p = 0; p < nplane; ++p)
    for (int j = 0; j < nstat; ++j) {
        const rank_pair rk = stat_rank<QUANT>(O, j, cnt);
        const unsigned khi = (unsigned)rk.k2;
        unsigned long long prefix = 0;
        unsigned k = (unsigned)rk.k, less = 0, eq = 0;
        for (int shift = plane_bits(O, p) - 8; shift >= 0; shift -= 8) {
            sHist[threadIdx.x] = 0;
            __syncthreads();
            for (unsigned b = 0; b < cnt; b += kBlock) {
                const unsigned i = b + threadIdx.x;
                const unsigned long long key = i < cnt ? load_key(O, p, off + i) : 0ull;
                hist_add(sHist, (int)((key >> shift) & 255), i < cnt && prefix_match(key, prefix, shift), lane);
            }
            __syncthreads();
            if (threadIdx.x < 64) {
                const digit_pick r = find_digit(sHist, k, lane);
                if (lane == 0) sPick = r;
            }
            __syncthreads();
            const digit_pick r = sPick;
            prefix |= (unsigned long long)r.d << shift;
            k -= r.below;
            less += r.below;
            eq = r.in_bin;
            __syncthreads();
        }
        unsigned long long hi = prefix;
        if (khi >= less + eq) {
            // the key of the second rank is the smallest key above the first one
            if (threadIdx.x == 0) sMin = ~0ull;
            __syncthreads();
            unsigned long long m = ~0ull;
            for (unsigned i = threadIdx.x; i < cnt; i += kBlock) {
                const unsigned long long key = load_key(O, p, off + i);
                if (key > prefix && key < m) m = key;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long t = __shfl_xor(m, o);
                m = t < m ? t : m;
            }
            if (lane == 0) atomicMin(&sMin, m);
            __syncthreads();
            hi = sMin;
        }
        if (threadIdx.x == 0) put_stat<QUANT>(O, cell, p, j, prefix, hi, rk.g);
        __syncthreads();
    }
}

// One workgroup per cell of 65 .. kLargeMin keys.
template <bool QUANT>
__global__ __launch_bounds__(kBlock) void k_med_medium(out_args O, const int* __restrict__ medium) {
    __shared__ unsigned sHist[256];
    __shared__ digit_pick sPick;
    __shared__ unsigned long long sMin;
    medium_cell<QUANT>(O, medium[blockIdx.x], sHist, sPick, sMin);
}

// The same over a fixed grid: the workgroups walk the list of medium cells, whose length they read from device memory.
template <bool QUANT>
__global__ __launch_bounds__(kBlock) void k_med_medium_walk(out_args O, const int* __restrict__ medium,
                                                           const tier_counters* __restrict__ tiers) {
    __shared__ unsigned sHist[256];
    __shared__ digit_pick sPick;
    __shared__ unsigned long long sMin;
    const unsigned n_medium = tiers->n_medium;
    for (unsigned i = blockIdx.x; i < n_medium; i += gridDim.x) medium_cell<QUANT>(O, medium[i], sHist, sPick, sMin);
}

// ---- large tier: one plane at a time, one launch pair per digit ----
// (ghist: 256 words per large cell from the start of `lh`, zero on entry and after every k_med_large_digit)
struct large_state {
    unsigned long long prefix, min_above;
    unsigned k, less, eq, k2;           // k2: the second rank of the result being selected
};

template <bool QUANT>
__global__ void k_med_large_init(const out_args O, const int* __restrict__ large, int n_large, int j,
                                 large_state* __restrict__ st) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_large) return;
    const unsigned cnt = O.count[large[l]];
    large_state s;
    s.prefix = 0;
    s.min_above = ~0ull;
    const rank_pair r = stat_rank<QUANT>(O, j, cnt);
    s.k = (unsigned)r.k;
    s.k2 = (unsigned)r.k2;
    s.less = s.eq = 0;
    st[l] = s;
}

// blockIdx.y: large cell, blockIdx.x: chunk of kChunk keys of its segment.  Digit histogram of the keys that match
// the prefix so far, added into ghist[cell][256].
__global__ __launch_bounds__(kBlock) void k_med_large_hist(const out_args O, const int* __restrict__ large, int p, int shift,
                                                          const large_state* __restrict__ st, unsigned* __restrict__ ghist) {
    __shared__ unsigned sHist[256];
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.y;
    const int cell = large[l];
    const unsigned cnt = O.count[cell], off = O.offset[cell];
    const unsigned b0 = blockIdx.x * (unsigned)kChunk;
    if (b0 >= cnt) return;                                          // (block-uniform)
    const unsigned b1 = min(cnt, b0 + (unsigned)kChunk);
    const unsigned long long prefix = st[l].prefix;
    sHist[threadIdx.x] = 0;
    __syncthreads();
    for (unsigned b = b0; b < b1; b += kBlock) {
        const unsigned i = b + threadIdx.x;
        const unsigned long long key = i < b1 ? load_key(O, p, off + i) : 0ull;
        hist_add(sHist, (int)((key >> shift) & 255), i < b1 && prefix_match(key, prefix, shift), lane);
    }
    __syncthreads();
    const unsigned v = sHist[threadIdx.x];
    if (v) atomicAdd(&ghist[(int64_t)l * 256 + threadIdx.x], v);
}

// one wave per large cell: pick the digit, advance the state, clear the histogram for the next pass
__global__ __launch_bounds__(64) void k_med_large_digit(int shift, large_state* __restrict__ st, unsigned* __restrict__ ghist) {
    const int lane = threadIdx.x;
    const int l = blockIdx.x;
    unsigned* h = ghist + (int64_t)l * 256;
    const digit_pick r = find_digit(h, st[l].k, lane);
#pragma unroll
    for (int q = 0; q < 4; ++q) h[4 * lane + q] = 0;
    if (lane == 0) {
        st[l].prefix |= (unsigned long long)r.d << shift;
        st[l].k -= r.below;
        st[l].less += r.below;
        st[l].eq = r.in_bin;
    }
}

// the smallest key above the selected one, where the second rank needs it
__global__ __launch_bounds__(kBlock) void k_med_large_above(const out_args O, const int* __restrict__ large, int p,
                                                           large_state* __restrict__ st) {
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.y;
    const unsigned cnt = O.count[large[l]], off = O.offset[large[l]];
    const unsigned b0 = blockIdx.x * (unsigned)kChunk;
    if (b0 >= cnt || st[l].k2 < st[l].less + st[l].eq) return;     // (block-uniform)
    const unsigned b1 = min(cnt, b0 + (unsigned)kChunk);
    const unsigned long long lo = st[l].prefix;
    unsigned long long m = ~0ull;
    for (unsigned i = b0 + threadIdx.x; i < b1; i += kBlock) {
        const unsigned long long key = load_key(O, p, off + i);
        if (key > lo && key < m) m = key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(m, o);
        m = t < m ? t : m;
    }
    if (lane == 0 && m != ~0ull) atomicMin(&st[l].min_above, m);
}

template <bool QUANT>
__global__ void k_med_large_put(const out_args O, const int* __restrict__ large, int n_large, int p, int j,
                                const large_state* __restrict__ st) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_large) return;
    const int cell = large[l];
    const unsigned cnt = O.count[cell];
    const large_state s = st[l];
    put_stat<QUANT>(O, cell, p, j, s.prefix, s.k2 < s.less + s.eq ? s.prefix : s.min_above, stat_rank<QUANT>(O, j, cnt).g);
}

// ---- large tier without a read-back (amt_median_frame_async) ----
// Per large cell l and plane p: a large_state, a 256-bin histogram and a ticket, in `lh` as l * nplane * 257 words:
// the histograms of its planes, then their tickets (zeroed by k_med_small when it lists the cell).  A fixed grid
// of workgroups; each one takes chunks blockIdx.x, blockIdx.x + gridDim.x, ... of every large cell.  After adding its
// share to a histogram a workgroup takes a ticket; the one that draws the last ticket reads the histogram, advances the
// state and clears both for the next launch.  Nothing waits for another workgroup.

// adds the LDS histogram to the global one, then: is this the last workgroup to do so? (block-uniform result)
__device__ __forceinline__ bool flush_and_ticket(const unsigned* sHist, unsigned* h, unsigned* tick, bool* sLast) {
    if (h != nullptr) {
        const unsigned v = sHist[threadIdx.x];
        if (v) atomicAdd(&h[threadIdx.x], v);
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) *sLast = atomicAdd(tick, 1u) == gridDim.x - 1;
    __syncthreads();
    const bool last = *sLast;
    if (last) __threadfence();
    return last;
}

// one launch per digit position `shift` (56, 48, ..., 0) and result j: the digit of every plane whose keys have one there
template <bool QUANT>
__global__ __launch_bounds__(kBlock) void k_med_large_step(const out_args O, const int* __restrict__ large,
                                                          const tier_counters* __restrict__ tiers, int shift, int j,
                                                          large_state* __restrict__ st, unsigned* __restrict__ lh) {
    __shared__ unsigned sHist[256];
    __shared__ digit_pick sPick;
    __shared__ bool sLast;
    const int lane = threadIdx.x & 63;
    const unsigned n_large = tiers->n_large;
    const int nplane = O.nch + (O.has_elev ? 1 : 0);
    for (unsigned l = 0; l < n_large; ++l) {
        const int cell = large[l];
        const unsigned cnt = O.count[cell], off = O.offset[cell];
        for (int p = 0; p < nplane; ++p) {
            const int bits = plane_bits(O, p);
            if (shift >= bits) continue;                                    // (uniform)
            const bool first = shift == bits - 8;
            large_state* s = st + (int64_t)l * nplane + p;
            const unsigned long long prefix = first ? 0ull : s->prefix;
            sHist[threadIdx.x] = 0;
            __syncthreads();
            for (unsigned b0 = blockIdx.x * (unsigned)kChunk; b0 < cnt; b0 += gridDim.x * (unsigned)kChunk) {
                const unsigned b1 = min(cnt, b0 + (unsigned)kChunk);
                for (unsigned b = b0; b < b1; b += kBlock) {
                    const unsigned i = b + threadIdx.x;
                    const unsigned long long key = i < b1 ? load_key(O, p, off + i) : 0ull;
                    hist_add(sHist, (int)((key >> shift) & 255), i < b1 && prefix_match(key, prefix, shift), lane);
                }
            }
            __syncthreads();
            unsigned* h = lh + (int64_t)l * nplane * 257 + p * 256;
            unsigned* tick = lh + (int64_t)l * nplane * 257 + nplane * 256 + p;
            if (!flush_and_ticket(sHist, h, tick, &sLast)) continue;
            // the last workgroup: the whole histogram, the digit, the state for the next position
            sHist[threadIdx.x] = __hip_atomic_load(&h[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            h[threadIdx.x] = 0;
            __syncthreads();
            if (threadIdx.x < 64) {
                const rank_pair rk = stat_rank<QUANT>(O, j, cnt);
                const unsigned k = first ? (unsigned)rk.k : s->k;
                const digit_pick r = find_digit(sHist, k, lane);
                if (lane == 0) {
                    large_state n;
                    n.prefix = prefix | ((unsigned long long)r.d << shift);
                    n.min_above = ~0ull;
                    n.k = k - r.below;
                    n.less = (first ? 0u : s->less) + r.below;
                    n.eq = r.in_bin;
                    n.k2 = (unsigned)rk.k2;
                    *s = n;
                    *tick = 0;
                }
            }
            __syncthreads();
        }
    }
}

// after the last digit: the smallest key above the selected one where the second rank needs it, then result j
template <bool QUANT>
__global__ __launch_bounds__(kBlock) void k_med_large_last(const out_args O, const int* __restrict__ large,
                                                          const tier_counters* __restrict__ tiers, int j,
                                                          large_state* __restrict__ st, unsigned* __restrict__ lh) {
    __shared__ bool sLast;
    __shared__ unsigned long long sMin;
    const int lane = threadIdx.x & 63;
    const unsigned n_large = tiers->n_large;
    const int nplane = O.nch + (O.has_elev ? 1 : 0);
    for (unsigned l = 0; l < n_large; ++l) {
        const int cell = large[l];
        const unsigned cnt = O.count[cell], off = O.offset[cell];
        for (int p = 0; p < nplane; ++p) {
            large_state* s = st + (int64_t)l * nplane + p;
            const unsigned long long lo = s->prefix;
            const bool need = s->k2 >= s->less + s->eq;
            if (threadIdx.x == 0) sMin = ~0ull;
            __syncthreads();
            if (need) {
                unsigned long long m = ~0ull;
                for (unsigned b0 = blockIdx.x * (unsigned)kChunk; b0 < cnt; b0 += gridDim.x * (unsigned)kChunk) {
                    const unsigned b1 = min(cnt, b0 + (unsigned)kChunk);
                    for (unsigned i = b0 + threadIdx.x; i < b1; i += kBlock) {
                        const unsigned long long key = load_key(O, p, off + i);
                        if (key > lo && key < m) m = key;
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const unsigned long long t = __shfl_xor(m, o);
                    m = t < m ? t : m;
                }
                if (lane == 0 && m != ~0ull) atomicMin(&sMin, m);
                __syncthreads();
                if (threadIdx.x == 0 && sMin != ~0ull) atomicMin(&s->min_above, sMin);
            }
            unsigned* tick = lh + (int64_t)l * nplane * 257 + nplane * 256 + p;
            if (!flush_and_ticket(nullptr, nullptr, tick, &sLast)) continue;
            if (threadIdx.x == 0) {
                const unsigned long long hi =
                    need ? __hip_atomic_load(&s->min_above, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : lo;
                put_stat<QUANT>(O, cell, p, j, lo, hi, stat_rank<QUANT>(O, j, cnt).g);
                *tick = 0;
            }
            __syncthreads();
        }
    }
}

// launch of a kernel that is instantiated per rank rule
#define MED_LAUNCH(kernel, quant, grid, block, ...)                                                  \
    do {                                                                                             \
        if (quant) hipLaunchKernelGGL((kernel<true>), grid, block, 0, ctx->stream, __VA_ARGS__);     \
        else hipLaunchKernelGGL((kernel<false>), grid, block, 0, ctx->stream, __VA_ARGS__);          \
    } while (0)

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }


// compute units of the context's device (queried once per device)
int64_t amt_cu_count(amt_ctx* ctx) {
    static int cus[64];
    const int d = ctx->device;
    if (d < 0 || d >= 64) return 256;
    if (cus[d] <= 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || v <= 0) {
            (void)hipGetLastError();
            v = 256;
        }
        cus[d] = v;
    }
    return cus[d];
}

// What both entry points share: the arguments, the workspace and every pass up to the small tier (k_med_small); the
// two upper tiers are enqueued by the callers.
struct median_pass {
    out_args O;
    int64_t n, cells, large_cap;
    int nplane;
    tier_counters* tiers;
    int* medium;
    int* large;
    large_state* state;
    unsigned* lh;                       // per large cell: the histograms of its planes, then their tickets
};

// The workspace of a pass over n pixels and `cells` cells: count, cursor [cells] | tier counters | offset [cells + 1] | block
// sums [nb + 1] | medium, large lists [cells] | cell_of [n] | u16 keys [nchan * n] | u64 elevation keys [n] | large-tier state
// [large_cap * nplane] and histograms with their tickets [large_cap * nplane * 257]: every plane of every large cell, as
// amt_median_frame_async has them in flight (733 cells x 4 planes x 1060 bytes = 3.1 MB at 12 Mpixel, beside ~18 bytes per
// pixel); amt_median_frame, one plane at a time, uses the first large_cap states and large_cap * 256 words.
struct med_layout {
    size_t count, tiers, offset, bsum, medium, large, cellof, keys16, keys64, state, ghist, bytes;
    int nb;
    int64_t large_cap;
};

med_layout median_layout(int64_t n, int64_t cells, int nchan, bool has_elev) {
    med_layout L;
    L.nb = cell_scan_blocks(cells);
    L.large_cap = n / (kLargeMin + 1) + 1;
    const int nplane = nchan + (has_elev ? 1 : 0);
    size_t at = 0;
    L.count = at;   at = align256(at + (size_t)2 * cells * sizeof(unsigned));
    L.tiers = at;   at = align256(at + sizeof(tier_counters));
    L.offset = at;  at = align256(at + (size_t)(cells + 1) * sizeof(unsigned));
    L.bsum = at;    at = align256(at + (size_t)(L.nb + 1) * sizeof(unsigned));
    L.medium = at;  at = align256(at + (size_t)cells * sizeof(int));
    L.large = at;   at = align256(at + (size_t)cells * sizeof(int));
    L.cellof = at;  at = align256(at + (size_t)n * sizeof(int));
    L.keys16 = at;  at = align256(at + (size_t)nchan * n * sizeof(uint16_t));
    L.keys64 = at;  at = align256(at + (has_elev ? (size_t)n * sizeof(unsigned long long) : 0));
    L.state = at;   at = align256(at + (size_t)(L.large_cap * nplane) * sizeof(large_state));
    L.ghist = at;   at = align256(at + (size_t)(L.large_cap * nplane * 257) * sizeof(unsigned));
    L.bytes = at;
    return L;
}

// the arrays of the count, scan and fill passes in a workspace laid out by median_layout
struct med_buffers {
    unsigned* count;
    unsigned* cursor;
    unsigned* offset;
    unsigned* bsum;
    int* cell_of;
    uint16_t* keys16;
    unsigned long long* keys64;
};

med_buffers median_bind(char* ws, const med_layout& L, int64_t n, int64_t cells, int nchan, bool has_elev, median_pass* M) {
    med_buffers B;
    B.count = reinterpret_cast<unsigned*>(ws + L.count);
    B.cursor = B.count + cells;
    B.offset = reinterpret_cast<unsigned*>(ws + L.offset);
    B.bsum = reinterpret_cast<unsigned*>(ws + L.bsum);
    B.cell_of = reinterpret_cast<int*>(ws + L.cellof);
    B.keys16 = reinterpret_cast<uint16_t*>(ws + L.keys16);
    B.keys64 = has_elev ? reinterpret_cast<unsigned long long*>(ws + L.keys64) : nullptr;
    M->tiers = reinterpret_cast<tier_counters*>(ws + L.tiers);
    M->medium = reinterpret_cast<int*>(ws + L.medium);
    M->large = reinterpret_cast<int*>(ws + L.large);
    M->state = reinterpret_cast<large_state*>(ws + L.state);
    M->lh = reinterpret_cast<unsigned*>(ws + L.ghist);
    M->n = n, M->cells = cells, M->large_cap = L.large_cap, M->nplane = nchan + (has_elev ? 1 : 0);
    return B;
}

// the output arguments and the small tier (k_med_small), after the fill pass
int median_small(amt_ctx* ctx, const med_buffers& B, const med_args& A, bool has_elev, const double* q, int nq, double* median,
                 void* out_img, uint8_t* out_mask, double* out_count, median_pass* M) {
    out_args& O = M->O;
    O.nx = A.nx;
    O.ny = A.ny;
    O.nch = A.nch;
    O.img_dtype = A.img_dtype;
    O.has_elev = has_elev;
    O.n = M->n;
    O.count = B.count;
    O.offset = B.offset;
    O.keys16 = B.keys16;
    O.keys64 = B.keys64;
    O.median = median;
    O.out_img = A.nch ? out_img : nullptr;
    O.out_mask = out_mask;
    O.out_count = out_count;
    O.nq = nq;
    for (int j = 0; j < kQuantilesMax; ++j) O.q[j] = j < nq ? q[j] : 0.0;
    MED_LAUNCH(k_med_small, nq != 0, grid_for(M->cells * 64), dim3(kBlock), O, M->medium, M->large, M->tiers, M->lh);
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

int median_front(amt_ctx* ctx, const double* lat_c, const double* lon_c, const double* elev, const void* img,
                 int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height, int32_t width,
                 double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap, int lon_from_mlt,
                 const double* q, int nq, double* median, void* out_img, uint8_t* out_mask, double* out_count,
                 median_pass* M) {
    // (nq == 0: the median; the callers have checked the quantiles)
    AMT_REQUIRE(ctx, median != nullptr, "NULL argument");
    med_args A;
    const char* bad = make_frame_src(&A.S, lat_c, lon_c, elev, center_mask, height, width, min_elevation, xaxis, yaxis, lon_wrap,
                                     lon_from_mlt);
    AMT_REQUIRE(ctx, bad == nullptr, bad);
    AMT_REQUIRE(ctx, (int64_t)height * width < 2147483647LL, "frame too large for 32-bit pixel indices");
    AMT_REQUIRE(ctx, nchan >= 0 && nchan <= 4, "nchan must be 0..4");
    AMT_REQUIRE(ctx, nchan == 0 || (img && (img_dtype == 1 || img_dtype == 2)), "img must be uint8 (1) or uint16 (2)");
    AMT_REQUIRE(ctx, (int64_t)xaxis->nbin * yaxis->nbin < 2147483647LL, "grid too large");
    A.img = img;
    A.nx = xaxis->nbin;
    A.ny = yaxis->nbin;
    A.nch = nchan;
    A.img_dtype = img_dtype;
    const int64_t n = (int64_t)height * width, cells = (int64_t)A.nx * A.ny;
    const med_layout L = median_layout(n, cells, nchan, elev != nullptr);
    char* ws = static_cast<char*>(amt_workspace(ctx, L.bytes));
    if (ws == nullptr) {
        ctx->last_error = "amt_median_frame: workspace allocation failed";
        return AMT_ENOMEM;
    }
    const med_buffers B = median_bind(ws, L, n, cells, nchan, elev != nullptr, M);

    // count, cursor and the tier counters are adjacent: one clear
    AMT_HIP(ctx, hipMemsetAsync(ws, 0, L.offset, ctx->stream));
    hipLaunchKernelGGL(k_med_count, grid_for((n + kPPT - 1) / kPPT), dim3(kBlock), 0, ctx->stream, A, B.cell_of, B.count);
    cell_scan(ctx, B.count, cells, B.bsum, B.offset);
    if (nchan == 0 || img_dtype == 1)
        hipLaunchKernelGGL(k_med_fill<uint8_t>, grid_for((n + kPPT - 1) / kPPT), dim3(kBlock), 0, ctx->stream, A, B.cell_of,
                           B.offset, B.cursor, B.keys16, B.keys64);
    else
        hipLaunchKernelGGL(k_med_fill<uint16_t>, grid_for((n + kPPT - 1) / kPPT), dim3(kBlock), 0, ctx->stream, A, B.cell_of,
                           B.offset, B.cursor, B.keys16, B.keys64);
    return median_small(ctx, B, A, elev != nullptr, q, nq, median, out_img, out_mask, out_count, M);
}

// The front of a mosaic (amt_mosaic_median_frames, amt_mosaic_quantile_frames): the cells, windows and overlap rule of
// amt_mosaic_frames, the segments of the passes above.  Rule 1 first runs amt_mosaic_frames' own binning and election for
// `source` alone; the count pass then keeps a member's pixel only where that member was elected, and from there both rules are
// the frame's problem over the concatenated pixels of the members.  One count and one fill launch whatever n_members is.
// Workspace (one allocation): rule 1's member tables and accumulators | source or first-member plane [cells] | member table |
// block prefix | the median workspace for the concatenated pixels.
int mosaic_median_front(amt_ctx* ctx, const amt_mosaic_member* members, int32_t n_members, int32_t img_dtype, int32_t nchan,
                        double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap, int32_t rule,
                        const double* q, int nq, double* median, void* out_img, uint8_t* out_mask, double* out_count,
                        int32_t* out_source, median_pass* M) {
    AMT_REQUIRE(ctx, members && xaxis && yaxis && median, "NULL argument");
    AMT_REQUIRE(ctx, nchan == 0 || img_dtype == 1 || img_dtype == 2, "img must be uint8 (1) or uint16 (2)");
    const int nx = xaxis->nbin, ny = yaxis->nbin;
    const int64_t cells = (int64_t)nx * ny;
    int64_t all_pixels = 0;
    const char* bad = mosaic_members_bad(members, n_members, rule, nchan, axis_ok(xaxis) && axis_ok(yaxis), nx, ny,
                                         [&](const amt_mosaic_member& m) -> const char* {
        if (!m.lon_c) return "member without centres";
        if (m.height > 0 && m.width > 0) all_pixels += (int64_t)m.height * m.width;
        return all_pixels < 2147483647LL ? nullptr : "the members' pixels together exceed 32-bit pixel indices";
    });
    AMT_REQUIRE(ctx, bad == nullptr, bad);
    mosaic_plan P;
    const bool fits = plan_members(P, members, n_members, nx, ny, nchan, [](const amt_mosaic_member& m) {
        return ((int64_t)m.height * m.width + kBlock * kPPT - 1) / (kBlock * kPPT);
    });
    AMT_REQUIRE(ctx, fits, "too many workgroups");          // (fewer than the pixels, which fit)
    std::vector<med_member> table((size_t)n_members);
    int64_t total = 0;
    bool has_elev = true;
    for (int32_t i = 0; i < n_members; ++i) {
        const amt_mosaic_member& m = members[i];
        has_elev = has_elev && m.elev != nullptr;           // (the elevation plane: of every member, or NaN)
        med_member& d = table[(size_t)i];
        bad = make_frame_src(&d.S, m.lat_c, m.lon_c, m.elev, m.center_mask, m.height, m.width, min_elevation, xaxis, yaxis, lon_wrap,
                             0);
        AMT_REQUIRE(ctx, bad == nullptr, bad);              // (mosaic_members_bad has looked at every member)
        d.img = m.img;
        d.g0 = (int)total;
        d.W = P.win[(size_t)i];
        if (d.W.nx != 0) total += (int64_t)m.height * m.width;
    }
    const int64_t blocks = P.units;
    if (amt_set_device(ctx)) return AMT_EHIP;

    const med_layout L = median_layout(total, cells, nchan, has_elev);
    workspace_packer K;
    const size_t o_plane = K.add((size_t)cells * sizeof(int32_t));
    const size_t o_table = K.upload(table.data(), table.size() * sizeof(med_member));
    const size_t o_bstart = K.upload(P.unit_start.data(), P.unit_start.size() * sizeof(int));
    const size_t o_med = K.add(L.bytes);
    const size_t bytes = K.total();
    char* ws = nullptr;
    if (rule == 1) {
        // the windowed binning and the election; with no out_source of its own the elected member of every output cell goes
        // to the head of the tail, where it stays until the count pass has read it
        if (int rc = amt_mosaic_run(ctx, members, n_members, img_dtype, nchan, min_elevation, xaxis, yaxis, lon_wrap, 1, nullptr,
                                    nullptr, nullptr, nullptr, nullptr, bytes, &ws))
            return rc;
    } else {
        ws = static_cast<char*>(amt_workspace(ctx, bytes));
    }
    if (ws == nullptr) {
        ctx->last_error = "amt_mosaic_median_frames: workspace allocation failed";
        return AMT_ENOMEM;
    }
    int32_t* plane = reinterpret_cast<int32_t*>(ws + o_plane);
    const med_buffers B = median_bind(ws + o_med, L, total, cells, nchan, has_elev, M);

    med_args A = {};                    // the call's common part; the kernels put a member's frame in (member_args)
    A.nx = nx;
    A.ny = ny;
    A.nch = nchan;
    A.img_dtype = img_dtype;
    member_table T;
    T.members = reinterpret_cast<const med_member*>(ws + o_table);
    T.block_start = reinterpret_cast<const int*>(ws + o_bstart);
    T.n = n_members;
    T.source = rule == 1 ? plane : nullptr;
    T.first = rule == 0 && out_source ? plane : nullptr;

    // member table and block prefix: one upload (pageable source: the copy has consumed the staging buffer when the call returns)
    const std::vector<char> host = K.host();
    AMT_HIP(ctx, hipMemcpyAsync(ws + o_table, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream));
    if (T.first) AMT_HIP(ctx, hipMemsetAsync(plane, 0x7f, (size_t)cells * sizeof(int32_t), ctx->stream));
    AMT_HIP(ctx, hipMemsetAsync(ws + o_med, 0, L.offset, ctx->stream));
    if (blocks > 0)
        hipLaunchKernelGGL(k_med_count_members, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, A, T, B.cell_of, B.count);
    if (out_source) {
        if (rule == 1)
            AMT_HIP(ctx, hipMemcpyAsync(out_source, plane, (size_t)cells * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
        else
            hipLaunchKernelGGL(k_med_source, grid_for(cells), dim3(kBlock), 0, ctx->stream, B.count, plane, nx, ny, out_source);
    }
    cell_scan(ctx, B.count, cells, B.bsum, B.offset);
    if (blocks > 0) {
        if (nchan == 0 || img_dtype == 1)
            hipLaunchKernelGGL(k_med_fill_members<uint8_t>, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, A, T, total,
                               B.cell_of, B.offset, B.cursor, B.keys16, B.keys64);
        else
            hipLaunchKernelGGL(k_med_fill_members<uint16_t>, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, A, T, total,
                               B.cell_of, B.offset, B.cursor, B.keys16, B.keys64);
    }
    return median_small(ctx, B, A, has_elev, q, nq, median, out_img, out_mask, out_count, M);
}

// The quantiles of a call, checked before anything else looks at its arguments or touches the device: 1 .. AMT_QUANTILES_MAX
// finite values in [0, 1].
bool quantiles_ok(amt_ctx* ctx, const double* q, int nq) {
    bool ok = q != nullptr && nq >= 1 && nq <= kQuantilesMax;
    for (int j = 0; ok && j < nq; ++j) ok = q[j] >= 0.0 && q[j] <= 1.0;      // (false for NaN)
    if (!ok && ctx != nullptr) ctx->last_error = "quantiles: 1..AMT_QUANTILES_MAX values in [0, 1]";
    return ok;
}

// The two upper tiers with one read-back (amt_median_frame, amt_quantile_frame): one launch per medium cell, and launch
// pairs per digit, plane and result for the large cells.
int upper_tiers_sync(amt_ctx* ctx, const median_pass& M) {
    const out_args& O = M.O;
    int* medium = M.medium;
    int* large = M.large;
    large_state* state = M.state;
    unsigned* ghist = M.lh;
    // the one device -> host read: how many cells the two upper tiers have
    tier_counters t;
    AMT_HIP(ctx, hipMemcpyAsync(&t, M.tiers, sizeof(t), hipMemcpyDeviceToHost, ctx->stream));
    AMT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int nplane = M.nplane, nstat = O.nq ? O.nq : 1;
    const bool quant = O.nq != 0;
    if (t.n_medium > 0)
        MED_LAUNCH(k_med_medium, quant, dim3(t.n_medium), dim3(kBlock), O, medium);
    if (t.n_large > 0) {
        AMT_REQUIRE(ctx, (int64_t)t.n_large <= M.large_cap, "internal: large-cell count out of range");
        const int nl = (int)t.n_large;
        const dim3 chunks((t.max_large + kChunk - 1) / kChunk, (unsigned)nl);
        const dim3 per_cell((nl + kBlock - 1) / kBlock);
        // (k_med_small has zeroed nplane * 257 >= 256 words of ghist for each of the nl cells it listed)
        for (int p = 0; p < nplane; ++p)
            for (int j = 0; j < nstat; ++j) {
                MED_LAUNCH(k_med_large_init, quant, per_cell, dim3(kBlock), O, large, nl, j, state);
                const int bits = p == O.nch ? 64 : (O.img_dtype == 1 ? 8 : 16);
                for (int shift = bits - 8; shift >= 0; shift -= 8) {
                    hipLaunchKernelGGL(k_med_large_hist, chunks, dim3(kBlock), 0, ctx->stream, O, large, p, shift, state, ghist);
                    hipLaunchKernelGGL(k_med_large_digit, dim3(nl), dim3(64), 0, ctx->stream, shift, state, ghist);
                }
                hipLaunchKernelGGL(k_med_large_above, chunks, dim3(kBlock), 0, ctx->stream, O, large, p, state);
                MED_LAUNCH(k_med_large_put, quant, per_cell, dim3(kBlock), O, large, nl, p, j, state);
            }
    }
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

// The two upper tiers without a read-back (amt_median_frame_async, amt_quantile_frame_async).
int upper_tiers_async(amt_ctx* ctx, const median_pass& M) {
    // fixed grids from what the host knows: a medium cell has more than kSmallMax pixels, a large one more than kLargeMin;
    // the workgroups read the tier sizes from device memory
    const out_args& O = M.O;
    const int64_t cu = amt_cu_count(ctx);
    const int64_t medium_bound = std::min(M.cells, M.n / (kSmallMax + 1));
    const int64_t medium_grid = std::max<int64_t>(1, std::min(medium_bound, 8 * cu));
    const bool quant = O.nq != 0;
    MED_LAUNCH(k_med_medium_walk, quant, dim3((unsigned)medium_grid), dim3(kBlock), O, M.medium, M.tiers);
    const int64_t large_grid = std::max<int64_t>(1, std::min(M.n / kChunk + 1, cu));
    if (M.n > kLargeMin && M.nplane > 0) {
        int top = 0;
        for (int p = 0; p < M.nplane; ++p) top = std::max(top, p == O.nch ? 64 : (O.img_dtype == 1 ? 8 : 16));
        // (every result starts from the first digit again: the states, histograms and tickets are left clean by the last one)
        const int nstat = O.nq ? O.nq : 1;
        for (int j = 0; j < nstat; ++j) {
            for (int shift = top - 8; shift >= 0; shift -= 8)
                MED_LAUNCH(k_med_large_step, quant, dim3((unsigned)large_grid), dim3(kBlock), O, M.large, M.tiers, shift, j,
                           M.state, M.lh);
            MED_LAUNCH(k_med_large_last, quant, dim3((unsigned)large_grid), dim3(kBlock), O, M.large, M.tiers, j, M.state, M.lh);
        }
    }
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

}  // namespace

extern "C" {

int amt_median_frame(amt_ctx* ctx, const double* lat_c, const double* lon_c, const double* elev, const void* img,
                     int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height, int32_t width,
                     double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap, double* median,
                     void* out_img, uint8_t* out_mask, double* out_count) {
    AMT_CHECK_CTX(ctx);
    median_pass M;
    if (int rc = median_front(ctx, lat_c, lon_c, elev, img, img_dtype, nchan, center_mask, height, width, min_elevation, xaxis,
                              yaxis, lon_wrap, 0, nullptr, 0, median, out_img, out_mask, out_count, &M))
        return rc;
    return upper_tiers_sync(ctx, M);
}

int amt_median_frame_async(amt_ctx* ctx, const double* lat_c, const double* lon_c, const double* elev, const void* img,
                           int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height, int32_t width,
                           double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap,
                           int lon_from_mlt, double* median, void* out_img, uint8_t* out_mask, double* out_count) {
    AMT_CHECK_CTX(ctx);
    median_pass M;
    if (int rc = median_front(ctx, lat_c, lon_c, elev, img, img_dtype, nchan, center_mask, height, width, min_elevation, xaxis,
                              yaxis, lon_wrap, lon_from_mlt, nullptr, 0, median, out_img, out_mask, out_count, &M))
        return rc;
    return upper_tiers_async(ctx, M);
}

int amt_quantile_frame(amt_ctx* ctx, const double* lat_c, const double* lon_c, const double* elev, const void* img,
                       int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height, int32_t width,
                       double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap, const double* q,
                       int nq, double* quantile, void* out_img, uint8_t* out_mask, double* out_count) {
    if (!quantiles_ok(ctx, q, nq)) return AMT_EINVAL;
    AMT_CHECK_CTX(ctx);
    median_pass M;
    if (int rc = median_front(ctx, lat_c, lon_c, elev, img, img_dtype, nchan, center_mask, height, width, min_elevation, xaxis,
                              yaxis, lon_wrap, 0, q, nq, quantile, out_img, out_mask, out_count, &M))
        return rc;
    return upper_tiers_sync(ctx, M);
}

int amt_quantile_frame_async(amt_ctx* ctx, const double* lat_c, const double* lon_c, const double* elev, const void* img,
                             int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height, int32_t width,
                             double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap,
                             int lon_from_mlt, const double* q, int nq, double* quantile, void* out_img, uint8_t* out_mask,
                             double* out_count) {
    if (!quantiles_ok(ctx, q, nq)) return AMT_EINVAL;
    AMT_CHECK_CTX(ctx);
    median_pass M;
    if (int rc = median_front(ctx, lat_c, lon_c, elev, img, img_dtype, nchan, center_mask, height, width, min_elevation, xaxis,
                              yaxis, lon_wrap, lon_from_mlt, q, nq, quantile, out_img, out_mask, out_count, &M))
        return rc;
    return upper_tiers_async(ctx, M);
}

int amt_mosaic_median_frames(amt_ctx* ctx, const amt_mosaic_member* members, int32_t n_members, int32_t img_dtype,
                             int32_t nchan, double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap,
                             int32_t rule, double* median, void* out_img, uint8_t* out_mask, double* out_count,
                             int32_t* out_source) {
    AMT_CHECK_CTX(ctx);
    median_pass M;
    if (int rc = mosaic_median_front(ctx, members, n_members, img_dtype, nchan, min_elevation, xaxis, yaxis, lon_wrap, rule,
                                     nullptr, 0, median, out_img, out_mask, out_count, out_source, &M))
        return rc;
    return upper_tiers_sync(ctx, M);
}

int amt_mosaic_quantile_frames(amt_ctx* ctx, const amt_mosaic_member* members, int32_t n_members, int32_t img_dtype,
                               int32_t nchan, double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap,
                               int32_t rule, const double* q, int nq, double* quantile, void* out_img, uint8_t* out_mask,
                               double* out_count, int32_t* out_source) {
    if (!quantiles_ok(ctx, q, nq)) return AMT_EINVAL;
    AMT_CHECK_CTX(ctx);
    median_pass M;
    if (int rc = mosaic_median_front(ctx, members, n_members, img_dtype, nchan, min_elevation, xaxis, yaxis, lon_wrap, rule, q,
                                     nq, quantile, out_img, out_mask, out_count, out_source, &M))
        return rc;
    return upper_tiers_sync(ctx, M);
}

int amt_quantile_rank(int64_t n, double q, int64_t* k, int64_t* k2, double* g) {
    if (n < 1 || !(q >= 0.0 && q <= 1.0) || k == nullptr || k2 == nullptr || g == nullptr) return AMT_EINVAL;
    const rank_pair r = rank_rule(n, q, false);
    *k = r.k, *k2 = r.k2, *g = r.g;
    return AMT_OK;
}

}  // extern "C"
