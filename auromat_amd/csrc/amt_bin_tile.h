// The tile body of the histogram binning (k_bin_frame, amt_binning.hip; k_mosaic_bin, amt_mosaic.hip) and the
// finalise arithmetic of a cell (k_bin_finalize; k_mosaic_select): one definition, so that a frame binned alone and
// the same frame binned as a member of a mosaic give the same integer sums and the same bits.
//
// One workgroup bins a BW x BH tile of the image.  Neighbouring pixels fall into neighbouring cells, so the tile's
// cells form a small window of the output grid: the window is privatised in LDS (u32 count / channel sums, i64
// fixed-point elevation), filled with LDS atomics and flushed with one 64-bit global integer atomic per touched cell
// and plane.  Integer accumulation is exact and order independent, so the result is bit-reproducible.
#pragma once

#include <type_traits>

#include "amt_common.h"
#include "amt_frame_src.h"
#include "amt_mosaic_plan.h"

namespace {

using namespace amt;

constexpr int kBinBlock = 256;

struct bin_args {
    frame_src S;
    const void* img;
    unsigned long long* acc;
};

constexpr int kPPT = 4;                      // consecutive pixels (along x) per thread and row, loaded as two pairs
constexpr int kBW = 64 * kPPT, kBH = kBinBlock / 64, kWCap = 1024;   // tile: 256 x 4 pixels, one image row per wave
// Column of pixel j of lane l inside the tile row.  (A layout with the two pairs 128 pixels apart, which makes
// every 16-byte wave load one contiguous 1 KiB segment, measured 25 % slower: 146 vs 118 us per frame.)
__device__ __forceinline__ int tile_col(int lane, int j) { return kPPT * lane + j; }

// Loads the thread's two pixel pairs of one row; `row` points at the tile's first pixel of that row, `n_row`
// is the number of pixels of the tile row inside the image.  VEC promises 16-byte alignment of `row`.
template <bool VEC>
__device__ __forceinline__ void load_run(const double* __restrict__ row, int lane, int n_row, double (&v)[kPPT]) {
#pragma unroll
    for (int k = 0; k < kPPT / 2; ++k) {
        const int c = tile_col(lane, 2 * k);
        if (VEC && c + 1 < n_row) {
            const double2 a = *reinterpret_cast<const double2*>(row + c);
            v[2 * k] = a.x;
            v[2 * k + 1] = a.y;
        } else {
            v[2 * k] = c < n_row ? row[c] : NAN;
            v[2 * k + 1] = c + 1 < n_row ? row[c + 1] : NAN;
        }
    }
}

constexpr int kWX = 32, kWY = 32;            // LDS window of kWX x kWY cells centred on the tile's anchor cell
constexpr int kRowIters = 4;                 // a workgroup walks kRowIters x kBH image rows (16) with one window
static_assert(kWX * kWY == kWCap, "window size");

// The members of a mosaic (amt_mosaic.hip): one descriptor per member in device memory, and the first global tile of
// every member (a prefix over the members' tiles, n + 1 entries).
struct mosaic_dev {
    bin_args A;             // the member's frame; A.acc = its window planes ((nchan + 2) x W.nx * W.ny cells)
    cell_window W;          // a tile body with WIN keeps the cells of W only (amt_mosaic_plan.h)
};
struct mosaic_args {
    const mosaic_dev* __restrict__ members;
    const int* __restrict__ tile_start;
    int n;
};

template <bool WIN> struct bin_kernel_args { using type = bin_args; };
template <> struct bin_kernel_args<true> { using type = mosaic_args; };

__device__ __forceinline__ const bin_args& frame_args(const bin_args& A, int) { return A; }
__device__ __forceinline__ const bin_args& frame_args(const mosaic_args& M, int m) { return M.members[m].A; }

// k_bin_frame: workgroup blockIdx.x bins one BW x (BH * kRowIters) tile of a frame.
// WIN = false: the argument is the frame (bin_args); the whole grid is kept (ax.nbin x ay.nbin cells per plane).
// WIN = true (the mosaic binning of amt_mosaic_frames, "k_mosaic_bin"): the argument is the member table (mosaic_args); the
// workgroup finds its member by the tile prefix and keeps only the cells of the member's window W.
template <typename IMG_T, int NCH, bool VEC, bool WIN>
__global__ __launch_bounds__(kBinBlock) void k_bin_frame(typename bin_kernel_args<WIN>::type P) {
    __shared__ unsigned int sCnt[kWCap];
    __shared__ unsigned int sCh[NCH > 0 ? NCH : 1][kWCap];
    __shared__ unsigned long long sEl[kWCap];
    __shared__ int sCand[kBinBlock / 64];

    int member = 0;
    if constexpr (WIN) member = member_of(P.tile_start, P.n, blockIdx.x);
    // (the frame: the kernel argument itself; a member: its descriptor copied into registers once, so that the global
    //  atomics below, which may alias the table for all the compiler knows, do not make every use reload it)
    typename std::conditional<WIN, const bin_args, const bin_args&>::type A = frame_args(P, member);
    const frame_src& S = A.S;
    cell_window W{0, 0, 0, 0};
    if constexpr (WIN) W = P.members[member].W;
    const int tiles_x = (S.width + kBW - 1) / kBW;
    unsigned t = blockIdx.x;                    // the tile's number within the frame
    if constexpr (WIN) t -= (unsigned)P.tile_start[member];
    const int tile_y = t / tiles_x, tile_x = t - tile_y * tiles_x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gx0 = tile_x * kBW;
    const int64_t ncell = WIN ? (int64_t)W.nx * W.ny : (int64_t)S.ax.nbin * S.ay.nbin;
    const IMG_T* img = static_cast<const IMG_T*>(A.img);

    for (int i = threadIdx.x; i < kWCap; i += kBinBlock) {
        sCnt[i] = 0;
        sEl[i] = 0;
#pragma unroll
        for (int c = 0; c < NCH; ++c) sCh[c][i] = 0;
    }
    // anchor cell (block-uniform): the window covers cells [ax0, ax0 + kWX) x [ay0, ay0 + kWY)
    int ax0 = 0, ay0 = 0;
    bool have_anchor = false;
    __syncthreads();

    for (int it = 0; it < kRowIters; ++it) {
        const int gy = (tile_y * kRowIters + it) * kBH + wave;
        const int n_row = (gy < S.height) ? min(kBW, S.width - gx0) : 0;   // pixels of this tile row inside the image

        // ---- all loads first (one memory latency per row group), then arithmetic ---------------------
        double la[kPPT], lo[kPPT], ev[kPPT];
        unsigned int ch[kPPT][NCH > 0 ? NCH : 1];
        unsigned char mk[kPPT];
#pragma unroll
        for (int j = 0; j < kPPT; ++j) {
            la[j] = NAN; lo[j] = NAN; ev[j] = 0.0; mk[j] = 0;
#pragma unroll
            for (int c = 0; c < NCH; ++c) ch[j][c] = 0;
        }
        if (n_row > 0) {
            const int64_t g0 = (int64_t)gy * S.width + gx0;
            load_run<VEC>(S.lat_c + g0, lane, n_row, la);
        }
        // a pixel without a latitude is not binned (resample.py:315-321): where a wave's whole tile row has none — the sky
        // above the limb, 30-40 % of an ISS frame — its longitudes, elevations and image bytes (22 of the 30 B per pixel)
        // are not read at all
        bool any_lat = false;
#pragma unroll
        for (int j = 0; j < kPPT; ++j) any_lat = any_lat || la[j] == la[j];
        if (n_row > 0 && __any(any_lat)) {
            const int64_t g0 = (int64_t)gy * S.width + gx0;
            load_run<VEC>(S.lon_c + g0, lane, n_row, lo);
            if (S.elev) load_run<VEC>(S.elev + g0, lane, n_row, ev);
            if (S.mask) {
#pragma unroll
                for (int j = 0; j < kPPT; ++j) mk[j] = tile_col(lane, j) < n_row ? S.mask[g0 + tile_col(lane, j)] : 1;
            }
            if (NCH > 0) {
                constexpr int kPairBytes = 2 * NCH * (int)sizeof(IMG_T);
#pragma unroll
                for (int k = 0; k < kPPT / 2; ++k) {
                    const int c0 = tile_col(lane, 2 * k);
                    const IMG_T* q = img + (g0 + c0) * NCH;
                    if (VEC && kPairBytes % 4 == 0 && c0 + 1 < n_row) {
                        // a pixel pair is kPairBytes contiguous, 4-byte aligned bytes (even column, even width)
                        constexpr int kWords = kPairBytes / 4;
                        const uint32_t* w = reinterpret_cast<const uint32_t*>(q);
                        uint32_t buf[kWords > 0 ? kWords : 1];
#pragma unroll
                        for (int i = 0; i < kWords; ++i) buf[i] = w[i];
#pragma unroll
                        for (int e = 0; e < 2 * NCH; ++e) {
                            const unsigned int val = sizeof(IMG_T) == 2 ? (buf[e >> 1] >> ((e & 1) * 16)) & 0xffffu
                                                                        : (buf[e >> 2] >> ((e & 3) * 8)) & 0xffu;
                            ch[2 * k + e / NCH][e % NCH] = val;
                        }
                    } else {
#pragma unroll
                        for (int e = 0; e < 2; ++e)
#pragma unroll
                            for (int c = 0; c < NCH; ++c) ch[2 * k + e][c] = c0 + e < n_row ? q[e * NCH + c] : 0;
                    }
                }
            }
        }

        int cellx[kPPT], celly[kPPT];
        int first = 0;                                  // first valid cell of this thread, packed (x << 16 | y) + 1
#pragma unroll
        for (int j = kPPT - 1; j >= 0; --j) {
            cellx[j] = 0;
            celly[j] = 0;
            if (src_keeps(S, la[j], ev[j], mk[j])) {
                int bx, by;
                if (src_cell(S, la[j], src_x(S, lo[j]), bx, by) &&
                    (!WIN || ((unsigned)(bx - 1 - W.x0) < (unsigned)W.nx && (unsigned)(by - 1 - W.y0) < (unsigned)W.ny))) {
                    cellx[j] = bx;
                    celly[j] = by;
                    first = -1 - j;   // the loop runs downwards: the smallest valid j wins
                }
            }
        }
        if (!have_anchor) {
            // elect the anchor: cell of the first valid pixel of the lowest wave that has one
            const unsigned long long m = __ballot(first < 0);
            int cand = 0;
            if (m) {
                const int src = __builtin_ctzll(m);
                const int j = -1 - __shfl(first, src);
                int cx = 0, cy = 0;
#pragma unroll
                for (int k = 0; k < kPPT; ++k) {
                    cx = (k == j) ? cellx[k] : cx;
                    cy = (k == j) ? celly[k] : cy;
                }
                cx = __shfl(cx, src);
                cy = __shfl(cy, src);
                cand = ((cx & 0xffff) << 16 | (cy & 0xffff)) + 1;     // grids have < 65535 bins per axis here
            }
            if (lane == 0) sCand[wave] = cand;
            __syncthreads();
            int chosen = 0;
#pragma unroll
            for (int w = kBinBlock / 64 - 1; w >= 0; --w) chosen = sCand[w] ? sCand[w] : chosen;
            __syncthreads();
            if (chosen) {
                have_anchor = true;
                ax0 = (((chosen - 1) >> 16) & 0xffff) - kWX / 2;
                ay0 = ((chosen - 1) & 0xffff) - kWY / 2;
            }
        }

        // consecutive pixels of a thread mostly share a cell: sum runs in registers, one atomic set per run.
        // (a NaN elevation of a kept pixel contributes 0; the reference would poison the cell — the mask
        //  invariants of mapping.py:299-316 make that unreachable)
        int run_x = 0, run_y = 0;
        unsigned int rcnt = 0, rch[NCH > 0 ? NCH : 1];
        long long rel = 0;
#pragma unroll
        for (int c = 0; c < NCH; ++c) rch[c] = 0;
        auto flush = [&]() {
            const int dx = run_x - ax0, dy = run_y - ay0;
            if (dx >= 0 && dx < kWX && dy >= 0 && dy < kWY) {
                const int wi = dx * kWY + dy;
                atomicAdd(&sCnt[wi], rcnt);
#pragma unroll
                for (int c = 0; c < NCH; ++c) atomicAdd(&sCh[c][wi], rch[c]);
                atomicAdd(&sEl[wi], (unsigned long long)rel);
            } else {
                // outside the LDS window (very fine grids or strongly stretched tiles): global atomics
                const int64_t cell = WIN ? (int64_t)(run_x - 1 - W.x0) * W.ny + (run_y - 1 - W.y0)
                                         : (int64_t)(run_x - 1) * S.ay.nbin + (run_y - 1);
                atomicAdd(&A.acc[cell], (unsigned long long)rcnt);
#pragma unroll
                for (int c = 0; c < NCH; ++c) atomicAdd(&A.acc[(int64_t)(1 + c) * ncell + cell], (unsigned long long)rch[c]);
                atomicAdd(&A.acc[(int64_t)(1 + NCH) * ncell + cell], (unsigned long long)rel);
            }
        };
#pragma unroll
        for (int j = 0; j < kPPT; ++j) {
            if (cellx[j] == 0) continue;
            if (cellx[j] != run_x || celly[j] != run_y) {
                if (run_x > 0) flush();
                run_x = cellx[j];
                run_y = celly[j];
                rcnt = 0;
                rel = 0;
#pragma unroll
                for (int c = 0; c < NCH; ++c) rch[c] = 0;
            }
            rcnt += 1;
#pragma unroll
            for (int c = 0; c < NCH; ++c) rch[c] += ch[j][c];
            rel += (ev[j] == ev[j]) ? __double2ll_rn(ev[j] * kFix) : 0;
        }
        if (run_x > 0) flush();
    }

    if (!have_anchor) return;      // nothing of this tile landed on the grid (block-uniform)
    __syncthreads();
    for (int i = threadIdx.x; i < kWCap; i += kBinBlock) {
        const unsigned int cnt = sCnt[i];
        if (cnt == 0) continue;
        const int dx = i / kWY, dy = i - dx * kWY;
        const int64_t cell = WIN ? (int64_t)(ax0 + dx - 1 - W.x0) * W.ny + (ay0 + dy - 1 - W.y0)
                                 : (int64_t)(ax0 + dx - 1) * S.ay.nbin + (ay0 + dy - 1);
        atomicAdd(&A.acc[cell], (unsigned long long)cnt);
#pragma unroll
        for (int c = 0; c < NCH; ++c) atomicAdd(&A.acc[(int64_t)(1 + c) * ncell + cell], (unsigned long long)sCh[c][i]);
        atomicAdd(&A.acc[(int64_t)(1 + NCH) * ncell + cell], sEl[i]);
    }
}

// Which outputs a finalise step writes: the kernel tests its own pointer arguments (global pointers) for NULL.
struct cell_wants {
    bool mean, img, mask, count;
};

// Mean, image, mask and count of output cell i from its integer accumulators (resample.py:339-351 and :128-136):
// sum(k) is channel k's sum, fix() the elevation sum in 31.32 fixed point (read only when `mean` is wanted).
template <typename IMG_T, typename SUM, typename FIX>
__device__ __forceinline__ void finalize_cell(unsigned long long cnt, SUM sum, FIX fix, int nch, int64_t i, double* mean,
                                              IMG_T* out_img, uint8_t* out_mask, double* out_count, cell_wants want) {
    const double dc = (double)cnt;
    for (int k = 0; k < nch; ++k) {
        const double m = cnt ? (double)sum(k) / dc : NAN;
        if (want.mean) mean[i * (nch + 1) + k] = m;
        if (want.img) out_img[i * nch + k] = cnt ? (IMG_T)rint(m) : (IMG_T)0;   // np.round: half to even
    }
    if (want.mean) {
        const long long fx = fix();
        mean[i * (nch + 1) + nch] = cnt ? ((double)fx / kFix) / dc : NAN;
    }
    if (want.mask) out_mask[i] = cnt ? 0 : 1;
    if (want.count) out_count[i] = dc;
}

}  // namespace
