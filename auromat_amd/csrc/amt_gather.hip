// Gather mosaic (include/auromat_hip.h: amt_gather_mosaic): the members of a collection gathered onto ONE grid in one kernel.
//
// k_remap's tiling: a block of 256 threads makes a 32 x 32 tile of cells, every thread four cells a quarter tile apart.  A thread
// projects its cells' centres through every member's camera model (w2p_point, amt_w2p.h: the arithmetic of amt_grid_to_pixel) and
// keeps only the running best of the overlap rule per cell: member, x, y, elevation.  No coordinate leaves the registers unless
// out_xy asks for the winner's.  Then the block looks at its winners.  One winner whose taps fit the LDS window — the interior of a
// footprint, the common case: that member's window is staged as k_remap stages it and every cell samples from LDS.  Several
// winners, or a window that does not fit: every cell takes its own winner's taps from global memory.  No winner: the empty values.
// Both ways go through tap_weights / sample / to_sample (amt_remap.h) with the same operands in the same order, so they give the
// same bits, and those of amt_grid_to_pixel + amt_remap_coords for the winning member alone.
//
// The member table (w2p_consts + w2p_sip + pointers per member) lies in the context's workspace; the member loop is uniform over
// the block, so the table is read through scalar loads.
//
// A member with a lens (the _lens entry points) is a raw frame that still carries its lens distortion: in elect() its (x, y) of
// the corrected frame goes on through step 9 (w2p_lens_step, amt_w2p.h: the arithmetic of amt_grid_to_pixel_lens) into the raw
// frame before the support test, and everything downstream works on the raw coordinates and the raw image.  The lenses (w2p_lens)
// are a table of their own behind the member table, and a launch without any lens has no such table.  Every kernel is compiled
// with and without step 9 (the template argument LENS of the one source: 72 instantiations of the 36); the host takes the one with
// it only where the launch has a lens table, so a launch without lenses runs the code it ran before step 9 existed.  With a table,
// "this member has a lens" is the same for the whole block; the lens constants are read, through scalar loads, inside that branch
// alone.
//
// The supersampled form (amt_gather_mosaic_supersampled) runs the same steps — load_points, elect, survey, stage_window,
// sample_point below are the one code of both kernels — on the n x n sub-sample points of T x T cells, T = 32 / n, laid over the
// same 32 x 32 threads' points, and then reduces the points to cells through LDS (k_gather_mosaic_ss).
//
// A batch of frames (amt_gather_frames): up to 64 jobs, each one member with its own grid and outputs, in ONE launch over the sum
// of their tiles.  The two kernels' bodies are device functions that take the tile's position (gather_tile_body, gather_ss_body);
// k_gather_frames looks its block's job up in a prefix table of tile counts and calls the same bodies.
#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "amt_common.h"
#include "amt_remap.h"
#include "amt_w2p.h"      // (fp contract off from here on)

namespace {

using namespace amt;

struct gather_dev {
    w2p_consts K;
    w2p_sip S;
    const void* img;
    const uint8_t* center_mask;
    double min_elevation;       // NaN: none
};

struct gather_args {
    const gather_dev* __restrict__ members;
    const double* __restrict__ lat;         // axes form (NULL: point form)
    const double* __restrict__ lon;
    const double* __restrict__ cell_lat;    // point form
    const double* __restrict__ cell_lon;
    int n, ny, nx, C;
    int rule, same_ellipsoid, force, pad_;
    void* img;
    uint8_t* mask;
    double* elev;
    int32_t* source;
    double* xy;
    uint8_t* tile_path;
    // (last: the arguments before it lie where they lay without it)  One per member, or NULL: no member has a lens; a member's
    // img and center_mask are the raw frame's, K.width x K.height, where its lens is not of kind AMT_LENS_NONE
    const w2p_lens* __restrict__ lenses;
};

// the supersampled call: G.ny, G.nx count cells, the coordinate arrays of G hold the factor x factor sub-sample points of each
struct gather_ss_args {
    gather_args G;
    int factor, min_count;
    int head, pad_;             // bytes of the dynamic LDS ahead of the points' samples: the window, later the winners and elevations
    uint8_t* count;
};

// a thread's four points (8 rows apart), the running best of the overlap rule at each, and the winner's taps
struct gather_points {
    bool in[kRowsPerThread];
    double lat[kRowsPerThread];
    lon_terms L[kRowsPerThread];
    lat_terms T[kRowsPerThread];
};
struct gather_best {
    int m[kRowsPerThread];
    double x[kRowsPerThread], y[kRowsPerThread], e[kRowsPerThread];
};
struct gather_taps {
    int ix[kRowsPerThread], iy[kRowsPerThread];
    double fx[kRowsPerThread], fy[kRowsPerThread];
};
// what the block's points hold: the one winner and the box of its taps where the window serves (staged)
struct gather_tile {
    int m, x_lo, y_lo, nwx, nwy, pitch;
    bool any, staged;
};

// N: taps per axis (2 linear, 8 Lanczos-4); 0: the nearest pixel, which needs no window
template <int N>
struct tap_range {
    static constexpr int lo = N == 8 ? -3 : 0, hi = lo + (N ? N : 1) - 1;
};

// the nearest pixel of a seen point (half to even), kept inside the frame: x in [-0.5, n - 0.5] rounds to -0 or n at the ends
__device__ __forceinline__ int nearest_index(double v, int n) { return (int)fmin(fmax(rint(v), 0.0), (double)(n - 1)); }

// the coordinates of a thread's points: column X and rows Y[k] of a point grid `pitch` points wide (the point form's rows)
__device__ __forceinline__ void load_points(const gather_args& A, int X, bool x_in, const int (&Y)[kRowsPerThread],
                                            const bool (&y_in)[kRowsPerThread], int64_t pitch, gather_points& P) {
    const bool points = A.cell_lat != nullptr;
    // a thread's points share their column: its longitude terms are computed once (the point form has a longitude per point)
    const lon_terms L0 = w2p_lon_terms(!points && x_in ? A.lon[X] : 0.0);
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        P.in[k] = x_in && y_in[k];
        const int64_t i = (int64_t)Y[k] * pitch + X;
        P.lat[k] = !P.in[k] ? 0.0 : (points ? A.cell_lat[i] : A.lat[Y[k]]);
        P.L[k] = points ? w2p_lon_terms(P.in[k] ? A.cell_lon[i] : 0.0) : L0;
        // the latitude terms depend on the member through the WGS84 constants alone: one evaluation where all members agree
        if (A.same_ellipsoid) P.T[k] = w2p_lat_terms(A.members[0].K, P.lat[k]);
    }
}

// ---- election: the running best per point ----------------------------------------------------------------------------
// LENS: some member of the launch has a lens (A.lenses is not NULL); without, step 9 is not part of the kernel
template <int N, bool LENS>
__device__ __forceinline__ void elect(const gather_args& A, const gather_points& P, gather_best& B) {
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) B.m[k] = -1, B.x[k] = B.y[k] = B.e[k] = NAN;
    for (int m = 0; m < A.n; ++m) {
        const gather_dev& M = A.members[m];
        const int w = M.K.width, h = M.K.height;
        const double least = M.min_elevation;
#pragma unroll
        for (int k = 0; k < kRowsPerThread; ++k) {
            if (!P.in[k]) continue;
            if (A.rule == 0 && B.m[k] >= 0) continue;       // the first member that sees the point keeps it
            const lat_terms Tm = A.same_ellipsoid ? P.T[k] : w2p_lat_terms(M.K, P.lat[k]);
            double x, y, e;
            unsigned fl = w2p_point(M.K, M.S, Tm, P.L[k], x, y, e);
            // a raw frame with its lens: (x, y) goes on through the lens into the raw frame (wave-uniform: M is the block's)
            if (LENS && A.lenses[m].m.kind != AMT_LENS_NONE) fl = w2p_lens_step(A.lenses[m], w, h, fl, x, y);
            bool seen = fl == 0;
            if (N != 0) {
                // support, as k_remap evaluates it on the float32 coordinates it is given
                const double xs = (double)(float)x, ys = (double)(float)y;
                seen = seen && xs >= 0.0 && xs <= (double)(w - 1) && ys >= 0.0 && ys <= (double)(h - 1);
            }
            if (seen && M.center_mask) seen = M.center_mask[(int64_t)nearest_index(y, h) * w + nearest_index(x, w)] == 0;
            if (least == least) seen = seen && e >= least;
            seen = seen && e == e;                          // a NaN elevation never wins
            if (seen && (B.m[k] < 0 || e > B.e[k])) B.m[k] = m, B.x[k] = x, B.y[k] = y, B.e[k] = e;   // (ties: the lower index)
        }
    }
}

// ---- what the tile holds: the range of its winners and the box of their taps, as (min, -max) so that one fold serves all ----
// (a barrier inside: every thread of the block calls it; `fold` is the block's, `tile` its tile's row-major index in the grid)
template <int N>
__device__ __forceinline__ gather_tile survey(const gather_args& A, const gather_best& B, gather_taps& t, int (&fold)[4][6], int tile) {
    constexpr int lo = tap_range<N>::lo, hi = tap_range<N>::hi;
    int r0 = INT32_MAX, r1 = INT32_MAX, b0 = INT32_MAX, b1 = INT32_MAX, b2 = INT32_MAX, b3 = INT32_MAX;
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        t.ix[k] = t.iy[k] = 0, t.fx[k] = t.fy[k] = 0.0;
        if (B.m[k] < 0) continue;
        r0 = min(r0, B.m[k]), r1 = min(r1, -B.m[k]);
        if (N == 0) {
            const w2p_consts& K = A.members[B.m[k]].K;
            t.ix[k] = nearest_index(B.x[k], K.width), t.iy[k] = nearest_index(B.y[k], K.height);
        } else {
            // (a seen point has support: k_remap's clamp of far-away coordinates would change nothing)
            const double xs = (double)(float)B.x[k], ys = (double)(float)B.y[k];
            const double flx = floor(xs), fly = floor(ys);
            t.ix[k] = (int)flx, t.iy[k] = (int)fly;
            t.fx[k] = xs - flx, t.fy[k] = ys - fly;
        }
        b0 = min(b0, t.ix[k] + lo), b1 = min(b1, -(t.ix[k] + hi));
        b2 = min(b2, t.iy[k] + lo), b3 = min(b3, -(t.iy[k] + hi));
    }
    r0 = wave_min(r0), r1 = wave_min(r1), b0 = wave_min(b0), b1 = wave_min(b1), b2 = wave_min(b2), b3 = wave_min(b3);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) fold[wave][0] = r0, fold[wave][1] = r1, fold[wave][2] = b0, fold[wave][3] = b1, fold[wave][4] = b2, fold[wave][5] = b3;
    __syncthreads();
    auto folded = [&](int j) { return min(min(fold[0][j], fold[1][j]), min(fold[2][j], fold[3][j])); };
    const int m_lo = folded(0), m_hi = -folded(1);
    const int x_lo = folded(2), x_hi = -folded(3), y_lo = folded(4), y_hi = -folded(5);
    gather_tile W;
    W.any = m_lo != INT32_MAX;
    W.m = m_lo, W.x_lo = x_lo, W.y_lo = y_lo;
    W.nwx = W.any ? x_hi - x_lo + 1 : 0, W.nwy = W.any ? y_hi - y_lo + 1 : 0;
    // the same for the whole block
    W.staged = N != 0 && W.any && m_lo == m_hi && W.nwx <= kWin && W.nwy <= kWin && A.force != AMT_GATHER_PATH_CELL;
    W.pitch = W.nwx * A.C;
    if (A.tile_path && threadIdx.x == 0)
        A.tile_path[tile] = !W.any ? 0 : (W.staged ? AMT_GATHER_PATH_STAGED : AMT_GATHER_PATH_CELL);
    return W;
}

// the one winner's window into LDS (a barrier inside; W.staged is the same for the whole block)
template <typename T>
__device__ __forceinline__ void stage_window(const gather_args& A, const gather_tile& W, T* win) {
    const int C = A.C, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const gather_dev& M = A.members[__builtin_amdgcn_readfirstlane(W.m)];
    const T* src = static_cast<const T*>(M.img);
    const int sw = M.K.width, sh = M.K.height;
    // a wave per window row, lanes along the row's samples: consecutive lanes read consecutive samples of the source row
    for (int r = wave; r < W.nwy; r += 4) {
        const int gy = W.y_lo + r;
        const bool row_in = gy >= 0 && gy < sh;
        const T* srow = src + ((int64_t)(row_in ? gy : 0) * sw) * C;
        for (int e = lane; e < W.pitch; e += 64) {
            const int gx = W.x_lo + e / C;
            const bool in = row_in && gx >= 0 && gx < sw;
            win[r * W.pitch + e] = in ? srow[(int64_t)W.x_lo * C + e] : (T)0;
        }
    }
    __syncthreads();
}

// the C samples of a won point: member m's image at the taps (ix, iy) + (fx, fy)
template <typename T, int N>
__device__ __forceinline__ void sample_point(const gather_args& A, const gather_tile& W, const T* win, int m, int ix, int iy, double fx,
                                             double fy, T* out) {
    constexpr int lo = tap_range<N>::lo;
    const int C = A.C;
    const gather_dev& M = A.members[m];
    const T* src = static_cast<const T*>(M.img);
    const int sw = M.K.width, sh = M.K.height;
    if (N == 0) {
        const T* px = src + ((int64_t)iy * sw + ix) * C;
        for (int c = 0; c < C; ++c) out[c] = px[c];
    } else {
        constexpr int NT = N ? N : 2;
        double wx[NT], wy[NT];
        tap_weights<NT>(fx, wx);
        tap_weights<NT>(fy, wy);
        if (W.staged) {
            const window_fetch<T> f = {win, W.x_lo, W.y_lo, W.pitch, C};
            for (int c = 0; c < C; ++c) out[c] = to_sample<T>(sample<NT>(f, ix + lo, iy + lo, c, wx, wy));
        } else {
            const global_fetch<T> f = {src, sw, sh, C};
            for (int c = 0; c < C; ++c) out[c] = to_sample<T>(sample<NT>(f, ix + lo, iy + lo, c, wx, wy));
        }
    }
}

// A block's work on the tile (bx, by) of A's grid; `tile` = by * tiles_x + bx.  k_gather_mosaic runs it on its own block index,
// k_gather_frames (below) on the tile of the job that the block has looked up.
template <typename T, int N, bool LENS>
__device__ __forceinline__ void gather_tile_body(const gather_args& A, int bx, int by, int tile, T* win, int (&fold)[4][6]) {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int X = bx * kTile + tx;
    const int C = A.C;
    int Y[kRowsPerThread];
    bool y_in[kRowsPerThread];
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) Y[k] = by * kTile + ty + 8 * k, y_in[k] = Y[k] < A.ny;

    gather_points P;
    gather_best B;
    gather_taps t;
    load_points(A, X, X < A.nx, Y, y_in, A.nx, P);
    elect<N, LENS>(A, P, B);
    const gather_tile W = survey<N>(A, B, t, fold, tile);
    if (W.staged) stage_window<T>(A, W, win);

#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        if (!P.in[k]) continue;
        const int64_t i = (int64_t)Y[k] * A.nx + X;
        T* out = static_cast<T*>(A.img) + i * C;
        const bool won = B.m[k] >= 0;
        A.mask[i] = won ? 0 : 1;
        if (A.source) A.source[i] = B.m[k];
        A.elev[i] = B.e[k];
        if (A.xy) A.xy[2 * i + 0] = B.x[k], A.xy[2 * i + 1] = B.y[k];
        if (!won) {
            for (int c = 0; c < C; ++c) out[c] = (T)0;
            continue;
        }
        sample_point<T, N>(A, W, win, B.m[k], t.ix[k], t.iy[k], t.fx[k], t.fy[k], out);
    }
}

template <typename T, int N, bool LENS>
__global__ __launch_bounds__(256) void k_gather_mosaic(gather_args A) {
    extern __shared__ __align__(16) unsigned char gather_smem[];
    __shared__ int fold[4][6];
    gather_tile_body<T, N, LENS>(A, (int)blockIdx.x, (int)blockIdx.y, (int)(blockIdx.y * gridDim.x + blockIdx.x),
                           reinterpret_cast<T*>(gather_smem), fold);
}

// ---- the supersampled form --------------------------------------------------------------------------------------------
// The block's 32 x 32 points are the factor x factor sub-samples of T x T cells, T = 32 / factor (threads whose point lies past
// T * factor idle).  Every point is elected and sampled as a cell of k_gather_mosaic is; its samples go to LDS behind the window,
// and once the block has sampled, the winners and elevations take the window's bytes.  Then one thread per (cell, quantity) —
// the C channels, the elevation with count and mask, the source — walks its cell's points in row-major order, which is the order
// the contract sums in.
constexpr int kPoints = kTile * kTile;
constexpr int kHeadMin = kPoints * (int)(sizeof(double) + sizeof(int));      // the elevations and winners of the block's points

template <typename T, int N, bool LENS>
__device__ __forceinline__ void gather_ss_body(const gather_ss_args& S, int bx, int by, int tile, unsigned char* gather_smem,
                                               int (&fold)[4][6]) {
    const gather_args& A = S.G;
    T* win = reinterpret_cast<T*>(gather_smem);
    double* p_elev = reinterpret_cast<double*>(gather_smem);
    int* p_win = reinterpret_cast<int*>(gather_smem + kPoints * sizeof(double));
    T* p_val = reinterpret_cast<T*>(gather_smem + S.head);

    const int n = S.factor, Tc = kTile / n, span = Tc * n;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int X = bx * span + tx;
    const int C = A.C;
    int Y[kRowsPerThread];
    bool y_in[kRowsPerThread];
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        Y[k] = by * span + ty + 8 * k;
        y_in[k] = ty + 8 * k < span && Y[k] < A.ny * n;
    }

    gather_points P;
    gather_best B;
    gather_taps t;
    load_points(A, X, tx < span && X < A.nx * n, Y, y_in, (int64_t)A.nx * n, P);
    elect<N, LENS>(A, P, B);
    const gather_tile W = survey<N>(A, B, t, fold, tile);
    if (W.staged) stage_window<T>(A, W, win);

#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        if (B.m[k] < 0) continue;
        const int p = (ty + 8 * k) * kTile + tx;
        sample_point<T, N>(A, W, win, B.m[k], t.ix[k], t.iy[k], t.fx[k], t.fy[k], p_val + p * C);
    }
    __syncthreads();            // the window has been read: its bytes now hold the points' winners and elevations
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        const int p = (ty + 8 * k) * kTile + tx;
        p_win[p] = B.m[k];      // (-1 also for the points outside the grid)
        p_elev[p] = B.e[k];
    }
    __syncthreads();

    const int cells = Tc * Tc, items = cells * (C + (A.source ? 2 : 1));       // (no source: nobody to count the winners for)
    for (int w = threadIdx.x; w < items; w += 256) {
        const int q = w / cells, cell = w - q * cells, cy = cell / Tc, cx = cell - cy * Tc;
        const int Yc = by * Tc + cy, Xc = bx * Tc + cx;
        if (Yc >= A.ny || Xc >= A.nx) continue;
        const int64_t i = (int64_t)Yc * A.nx + Xc;
        const int p0 = cy * n * kTile + cx * n;
        int count = 0;
        if (q < C) {
            // a channel: the exact integer sum, or the float64 sum in row-major order that the first seen value starts
            uint32_t isum = 0;
            double acc = 0.0;
            for (int s = 0; s < n; ++s)
                for (int u = 0; u < n; ++u) {
                    const int p = p0 + s * kTile + u;
                    if (p_win[p] < 0) continue;
                    const T v = p_val[p * C + q];
                    if (std::is_same<T, float>::value)
                        acc = count ? acc + (double)v : (double)v;
                    else
                        isum += (uint32_t)v;
                    ++count;
                }
            T out = (T)0;
            if (count >= S.min_count)
                out = std::is_same<T, float>::value ? (T)(float)(acc / (double)count) : (T)rint((double)isum / (double)count);
            static_cast<T*>(A.img)[i * C + q] = out;
        } else if (q == C) {
            double acc = 0.0;
            for (int s = 0; s < n; ++s)
                for (int u = 0; u < n; ++u) {
                    const int p = p0 + s * kTile + u;
                    if (p_win[p] < 0) continue;
                    acc = count ? acc + p_elev[p] : p_elev[p];
                    ++count;
                }
            const bool valid = count >= S.min_count;
            S.count[i] = (uint8_t)count;
            A.mask[i] = valid ? 0 : 1;
            A.elev[i] = valid ? acc / (double)count : (double)NAN;
        } else {
            // the member that won the most points, the lower index on a tie: the winners are counted in ascending order
            int cur = INT32_MAX;
            for (int s = 0; s < n; ++s)
                for (int u = 0; u < n; ++u) {
                    const int m = p_win[p0 + s * kTile + u];
                    if (m < 0) continue;
                    cur = min(cur, m);
                    ++count;
                }
            int best = -1, most = 0;
            while (cur != INT32_MAX) {
                int won = 0, next = INT32_MAX;
                for (int s = 0; s < n; ++s)
                    for (int u = 0; u < n; ++u) {
                        const int m = p_win[p0 + s * kTile + u];
                        won += m == cur ? 1 : 0;
                        if (m > cur) next = min(next, m);
                    }
                if (won > most) best = cur, most = won;
                cur = next;
            }
            A.source[i] = count >= S.min_count ? best : -1;
        }
    }
}

template <typename T, int N, bool LENS>
__global__ __launch_bounds__(256) void k_gather_mosaic_ss(gather_ss_args S) {
    extern __shared__ __align__(16) unsigned char gather_smem[];
    __shared__ int fold[4][6];
    gather_ss_body<T, N, LENS>(S, (int)blockIdx.x, (int)blockIdx.y, (int)(blockIdx.y * gridDim.x + blockIdx.x), gather_smem, fold);
}

// ---- a batch of frames (amt_gather_frames): one launch over the tiles of all jobs -----------------------------------------------
// A job is one member with a grid and outputs of its own.  The jobs' tile counts are summed into `first` (n_jobs + 1 entries,
// first[0] = 0); block b belongs to the job j with first[j] <= b < first[j + 1] and makes that job's tile b - first[j].  The
// look-up depends on the block index alone, so it runs on scalar loads; what it finds — the job's gather_args, with a member
// table of one — is uniform over the block as the kernel arguments of k_gather_mosaic are, and the block runs the same body.
struct gather_job_dev {
    gather_dev M;
    const double *lat, *lon, *cell_lat, *cell_lon;
    void* img;
    uint8_t* mask;
    double* elev;
    uint8_t* count;
    int ny, nx, tiles_x, pad_;
};

struct gather_frames_args {
    const int* __restrict__ first;
    const gather_job_dev* __restrict__ jobs;
    int n_jobs, C, force, factor;
    int min_count, head;
    uint8_t* tile_path;         // the jobs' tiles one job after the other
    const w2p_lens* __restrict__ lenses;    // (last, as in gather_args) one per job, or NULL
};

template <typename T, int N, bool SS, bool LENS>
__global__ __launch_bounds__(256) void k_gather_frames(gather_frames_args F) {
    extern __shared__ __align__(16) unsigned char gather_smem[];
    __shared__ int fold[4][6];

    const int b = (int)blockIdx.x;
    int lo = 0, hi = F.n_jobs;              // first[lo] <= b < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (F.first[mid] <= b)
            lo = mid;
        else
            hi = mid;
    }
    const gather_job_dev& J = F.jobs[lo];
    const int start = F.first[lo], tile = b - start;
    const int by = tile / J.tiles_x, bx = tile - by * J.tiles_x;

    gather_ss_args S;
    gather_args& A = S.G;
    A.members = &J.M;
    A.lenses = LENS ? F.lenses + lo : nullptr;
    A.lat = J.lat, A.lon = J.lon, A.cell_lat = J.cell_lat, A.cell_lon = J.cell_lon;
    A.n = 1, A.ny = J.ny, A.nx = J.nx, A.C = F.C;
    A.rule = 1, A.same_ellipsoid = 1, A.force = F.force, A.pad_ = 0;
    A.img = J.img, A.mask = J.mask, A.elev = J.elev, A.source = nullptr, A.xy = nullptr;
    A.tile_path = F.tile_path ? F.tile_path + start : nullptr;
    if (SS) {
        S.factor = F.factor, S.min_count = F.min_count, S.head = F.head, S.pad_ = 0;
        S.count = J.count;
        gather_ss_body<T, N, LENS>(S, bx, by, tile, gather_smem, fold);
    } else {
        gather_tile_body<T, N, LENS>(A, bx, by, tile, reinterpret_cast<T*>(gather_smem), fold);
    }
}

template <typename T>
size_t window_bytes(int C) {
    return (size_t)kWin * kWin * (size_t)C * sizeof(T);
}

// the dynamic LDS of a launch: the window (none for the nearest pixel); a supersampled launch holds the window or the winners and
// elevations, whichever is larger (`head`: its bytes, 16-byte rounded), then the points' samples: at most 36 KB + 16 KB
// (float32 x 4 channels)
template <typename T>
size_t gather_lds(int C, int interpolation, bool supersampled, int& head) {
    const size_t window = interpolation == AMT_INTERP_NEAREST ? 0 : window_bytes<T>(C);
    if (!supersampled) return window;
    const size_t h = (std::max(window, (size_t)kHeadMin) + 15) & ~(size_t)15;
    head = (int)h;
    return h + (size_t)kPoints * (size_t)C * sizeof(T);
}

// the one dispatch over (sample type, taps per axis): launch(T(), integral_constant<int, N>())
template <typename F>
void gather_dispatch(int sample_bytes, int interpolation, F launch) {
    const auto taps = [&](auto t) {
        if (interpolation == AMT_INTERP_LINEAR)
            launch(t, std::integral_constant<int, 2>());
        else if (interpolation == AMT_INTERP_LANCZOS4)
            launch(t, std::integral_constant<int, 8>());
        else
            launch(t, std::integral_constant<int, 0>());
    };
    switch (sample_bytes) {
        case 1: taps(uint8_t()); break;
        case 2: taps(uint16_t()); break;
        default: taps(float()); break;
    }
}

void launch_gather(amt_ctx* ctx, const gather_args& A, int sample_bytes, int interpolation) {
    const dim3 grid((unsigned)((A.nx + kTile - 1) / kTile), (unsigned)((A.ny + kTile - 1) / kTile));
    gather_dispatch(sample_bytes, interpolation, [&](auto t, auto taps) {
        using T = decltype(t);
        int head;
        const size_t lds = gather_lds<T>(A.C, interpolation, false, head);
        constexpr int N = decltype(taps)::value;
        if (A.lenses)
            hipLaunchKernelGGL((k_gather_mosaic<T, N, true>), grid, dim3(256), lds, ctx->stream, A);
        else
            hipLaunchKernelGGL((k_gather_mosaic<T, N, false>), grid, dim3(256), lds, ctx->stream, A);
    });
}

void launch_gather_ss(amt_ctx* ctx, gather_ss_args S, int sample_bytes, int interpolation) {
    const int Tc = kTile / S.factor;
    const dim3 grid((unsigned)((S.G.nx + Tc - 1) / Tc), (unsigned)((S.G.ny + Tc - 1) / Tc));
    gather_dispatch(sample_bytes, interpolation, [&](auto t, auto taps) {
        using T = decltype(t);
        const size_t lds = gather_lds<T>(S.G.C, interpolation, true, S.head);
        constexpr int N = decltype(taps)::value;
        if (S.G.lenses)
            hipLaunchKernelGGL((k_gather_mosaic_ss<T, N, true>), grid, dim3(256), lds, ctx->stream, S);
        else
            hipLaunchKernelGGL((k_gather_mosaic_ss<T, N, false>), grid, dim3(256), lds, ctx->stream, S);
    });
}

void launch_gather_frames(amt_ctx* ctx, gather_frames_args F, int tiles, int sample_bytes, int interpolation) {
    const dim3 grid((unsigned)tiles);
    gather_dispatch(sample_bytes, interpolation, [&](auto t, auto taps) {
        using T = decltype(t);
        constexpr int N = decltype(taps)::value;
        const bool ss = F.factor > 1;
        const size_t lds = gather_lds<T>(F.C, interpolation, ss, F.head);
        if (ss && F.lenses)
            hipLaunchKernelGGL((k_gather_frames<T, N, true, true>), grid, dim3(256), lds, ctx->stream, F);
        else if (ss)
            hipLaunchKernelGGL((k_gather_frames<T, N, true, false>), grid, dim3(256), lds, ctx->stream, F);
        else if (F.lenses)
            hipLaunchKernelGGL((k_gather_frames<T, N, false, true>), grid, dim3(256), lds, ctx->stream, F);
        else
            hipLaunchKernelGGL((k_gather_frames<T, N, false, false>), grid, dim3(256), lds, ctx->stream, F);
    });
}

#define GATHER_REQUIRE(cond, msg)                                     \
    do {                                                               \
        if (!(cond)) {                                                 \
            ctx->last_error = std::string(fn) + ": " + (msg);          \
            return AMT_EINVAL;                                         \
        }                                                              \
    } while (0)

// the arguments every entry point takes (`rule`: a batch of frames has one member per job and passes the kernel's 1)
int gather_check(amt_ctx* ctx, const char* fn, int32_t frame, int32_t interpolation, int32_t rule, int32_t sample_bytes, int32_t channels,
                 const amt_gather_debug* debug) {
    GATHER_REQUIRE(frame == AMT_W2P_GEODETIC || frame == AMT_W2P_SM, "unknown frame (AMT_W2P_GEODETIC or AMT_W2P_SM)");
    GATHER_REQUIRE(interpolation == AMT_INTERP_LINEAR || interpolation == AMT_INTERP_LANCZOS4 || interpolation == AMT_INTERP_NEAREST,
                   "unknown interpolation");
    GATHER_REQUIRE(rule == 0 || rule == 1, "unknown rule");
    GATHER_REQUIRE(sample_bytes == 1 || sample_bytes == 2 || sample_bytes == 4, "sample_bytes must be 1 (uint8), 2 (uint16) or 4 (float32)");
    GATHER_REQUIRE(channels == 1 || channels == 3 || channels == 4, "channels must be 1, 3 or 4");
    GATHER_REQUIRE(!debug || (debug->force_path >= AMT_GATHER_PATH_AUTO && debug->force_path <= AMT_GATHER_PATH_CELL), "unknown force_path");
    return AMT_OK;
}

// the supersampled calls' own: the factor and the least count, then (per grid; `job`: "job k: " or nothing) the sub-sample grid
int gather_check_factor(amt_ctx* ctx, const char* fn, int32_t factor, int32_t min_count) {
    GATHER_REQUIRE(factor >= 1 && factor <= 8, "factor must be 1 ... 8");
    GATHER_REQUIRE(min_count >= 1 && min_count <= factor * factor, "min_count must be 1 ... factor * factor");
    return AMT_OK;
}

int gather_check_subgrid(amt_ctx* ctx, const char* fn, const std::string& job, int32_t ny, int32_t nx, int32_t factor) {
    GATHER_REQUIRE(ny <= INT32_MAX / factor && nx <= INT32_MAX / factor, job + "the sub-sample grid does not fit 32-bit indices");
    return AMT_OK;
}

// "either the two axes or the two cell arrays": the pair that is given goes to `to` (gather_args, gather_job_dev), the other is NULL
template <typename To>
int gather_coordinates(amt_ctx* ctx, const char* fn, const std::string& job, const double* lat, const double* lon, const double* cell_lat,
                       const double* cell_lon, To& to) {
    const bool axes = lat && lon, cells = cell_lat && cell_lon;
    GATHER_REQUIRE((lat != nullptr) == (lon != nullptr) && (cell_lat != nullptr) == (cell_lon != nullptr) && axes != cells,
                   job + "give either the two axes or the two cell arrays");
    to.lat = axes ? lat : nullptr, to.lon = axes ? lon : nullptr;
    to.cell_lat = axes ? nullptr : cell_lat, to.cell_lon = axes ? nullptr : cell_lon;
    return AMT_OK;
}

// a member as the kernels read it: w2p_prepare's or w2p_lens_prepare's message, or "member without image", or NULL
// (Ln: NULL where the call has no lenses at all)
const char* gather_member(const amt_gather_member& m, const amt_lens_model* lens, int32_t frame, gather_dev& d, w2p_lens* Ln) {
    const char* err = m.img ? w2p_prepare(&m.params, m.zenithal, frame, &d.K, &d.S) : "member without image";
    if (err == nullptr && Ln) err = w2p_lens_prepare(lens, &m.params, m.zenithal, Ln);
    d.img = m.img;
    d.center_mask = m.center_mask;
    d.min_elevation = m.min_elevation > -INFINITY ? m.min_elevation : (double)NAN;      // (-inf and NaN: none)
    return err;
}

// what both mosaic entry points check and prepare: the arguments they share, the member table in the context's workspace, and the
// kernel's arguments for a grid of ny x nx cells (the supersampled call adds its own)
int gather_prepare(amt_ctx* ctx, const char* fn, const amt_gather_member* members, const amt_lens_model* const* lenses,
                   int32_t n_members, int32_t frame, const double* lat_axis,
                   int32_t ny, const double* lon_axis, int32_t nx, const double* cell_lat, const double* cell_lon, int32_t sample_bytes,
                   int32_t channels, int32_t interpolation, int32_t rule, void* out_img, uint8_t* out_mask, double* out_elev,
                   int32_t* out_source, const amt_gather_debug* debug, gather_args& A) {
    GATHER_REQUIRE(members && out_img && out_mask && out_elev && out_source, "NULL argument");
    GATHER_REQUIRE(n_members >= 1, "no members");
    GATHER_REQUIRE(ny > 0 && nx > 0, "empty axis");
    int rc = gather_coordinates(ctx, fn, "", lat_axis, lon_axis, cell_lat, cell_lon, A);
    if (rc == AMT_OK) rc = gather_check(ctx, fn, frame, interpolation, rule, sample_bytes, channels, debug);
    if (rc != AMT_OK) return rc;

    // the member table and, where a member has a lens, the lens table behind it, in one staging buffer: one copy
    const size_t lens_at = (size_t)n_members * sizeof(gather_dev);
    std::vector<unsigned char> staged(lens_at + (lenses ? (size_t)n_members * sizeof(w2p_lens) : 0));
    gather_dev* dev = reinterpret_cast<gather_dev*>(staged.data());
    w2p_lens* lens = reinterpret_cast<w2p_lens*>(staged.data() + lens_at);
    bool same = true, any_lens = false;
    for (int32_t i = 0; i < n_members; ++i) {
        gather_dev& d = dev[i];
        const char* err = gather_member(members[i], lenses ? lenses[i] : nullptr, frame, d, lenses ? &lens[i] : nullptr);
        GATHER_REQUIRE(err == nullptr, "member " + std::to_string(i) + ": " + err);
        same = same && d.K.a0 == dev[0].K.a0 && d.K.e2 == dev[0].K.e2;
        any_lens = any_lens || (lenses && lens[i].m.kind != AMT_LENS_NONE);
    }
    if (amt_set_device(ctx)) return AMT_EHIP;
    const size_t bytes = any_lens ? staged.size() : lens_at;
    char* ws = static_cast<char*>(amt_workspace(ctx, bytes));
    if (ws == nullptr) {
        ctx->last_error = std::string(fn) + ": workspace allocation failed";
        return AMT_ENOMEM;
    }
    // (pageable source: the copy has consumed the staging buffer when the call returns)
    const hipError_t err = hipMemcpyAsync(ws, staged.data(), bytes, hipMemcpyHostToDevice, ctx->stream);
    if (err != hipSuccess) {
        ctx->last_error = std::string(fn) + ": hipMemcpyAsync -> " + hipGetErrorString(err);
        return AMT_EHIP;
    }

    A.members = reinterpret_cast<const gather_dev*>(ws);
    A.lenses = any_lens ? reinterpret_cast<const w2p_lens*>(ws + lens_at) : nullptr;
    A.n = n_members, A.ny = ny, A.nx = nx, A.C = channels;
    A.rule = rule, A.same_ellipsoid = same ? 1 : 0, A.force = debug ? debug->force_path : AMT_GATHER_PATH_AUTO, A.pad_ = 0;
    A.img = out_img, A.mask = out_mask, A.elev = out_elev, A.source = out_source, A.xy = nullptr;
    A.tile_path = debug ? debug->tile_path : nullptr;
    return AMT_OK;
}

}  // namespace

// The three entry points with and without lenses: `fn` is the name the caller knows, for the error texts.
static int gather_mosaic_call(amt_ctx* ctx, const char* fn, const amt_gather_member* members, int32_t n_members, int32_t frame,
                              const double* lat_centres, int32_t ny, const double* lon_centres, int32_t nx, const double* cell_lat,
                              const double* cell_lon, int32_t sample_bytes, int32_t channels, int32_t interpolation, int32_t rule,
                              void* out_img, uint8_t* out_mask, double* out_elev, int32_t* out_source, double* out_xy,
                              const amt_gather_debug* debug, const amt_lens_model* const* lenses) {
    AMT_CHECK_CTX(ctx);
    gather_args A;
    const int rc = gather_prepare(ctx, fn, members, lenses, n_members, frame, lat_centres, ny, lon_centres, nx, cell_lat, cell_lon,
                                  sample_bytes, channels, interpolation, rule, out_img, out_mask, out_elev, out_source, debug, A);
    if (rc != AMT_OK) return rc;
    A.xy = out_xy;
    launch_gather(ctx, A, sample_bytes, interpolation);
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

extern "C" int amt_gather_mosaic(amt_ctx* ctx, const amt_gather_member* members, int32_t n_members, int32_t frame,
                                 const double* lat_centres, int32_t ny, const double* lon_centres, int32_t nx,
                                 const double* cell_lat, const double* cell_lon, int32_t sample_bytes, int32_t channels,
                                 int32_t interpolation, int32_t rule, void* out_img, uint8_t* out_mask, double* out_elev,
                                 int32_t* out_source, double* out_xy, const amt_gather_debug* debug) {
    return gather_mosaic_call(ctx, __func__, members, n_members, frame, lat_centres, ny, lon_centres, nx, cell_lat, cell_lon, sample_bytes,
                              channels, interpolation, rule, out_img, out_mask, out_elev, out_source, out_xy, debug, nullptr);
}

extern "C" int amt_gather_mosaic_lens(amt_ctx* ctx, const amt_gather_member* members, int32_t n_members, int32_t frame,
                                      const double* lat_centres, int32_t ny, const double* lon_centres, int32_t nx,
                                      const double* cell_lat, const double* cell_lon, int32_t sample_bytes, int32_t channels,
                                      int32_t interpolation, int32_t rule, void* out_img, uint8_t* out_mask, double* out_elev,
                                      int32_t* out_source, double* out_xy, const amt_gather_debug* debug,
                                      const amt_lens_model* const* lenses) {
    return gather_mosaic_call(ctx, __func__, members, n_members, frame, lat_centres, ny, lon_centres, nx, cell_lat, cell_lon, sample_bytes,
                              channels, interpolation, rule, out_img, out_mask, out_elev, out_source, out_xy, debug, lenses);
}

static int gather_supersampled_call(amt_ctx* ctx, const char* fn, const amt_gather_member* members, int32_t n_members, int32_t frame,
                                    const double* sub_lat, int32_t ny, const double* sub_lon, int32_t nx, const double* sub_cell_lat,
                                    const double* sub_cell_lon, int32_t factor, int32_t min_count, int32_t sample_bytes,
                                    int32_t channels, int32_t interpolation, int32_t rule, void* out_img, uint8_t* out_mask,
                                    double* out_elev, int32_t* out_source, uint8_t* out_count, const amt_gather_debug* debug,
                                    const amt_lens_model* const* lenses) {
    AMT_CHECK_CTX(ctx);
    GATHER_REQUIRE(out_count, "NULL argument");
    gather_ss_args S;
    int rc = gather_check_factor(ctx, fn, factor, min_count);
    if (rc == AMT_OK) rc = gather_check_subgrid(ctx, fn, "", ny, nx, factor);
    if (rc == AMT_OK)
        rc = gather_prepare(ctx, fn, members, lenses, n_members, frame, sub_lat, ny, sub_lon, nx, sub_cell_lat, sub_cell_lon, sample_bytes,
                            channels, interpolation, rule, out_img, out_mask, out_elev, out_source, debug, S.G);
    if (rc != AMT_OK) return rc;
    S.factor = factor, S.min_count = min_count, S.head = 0, S.pad_ = 0;
    S.count = out_count;
    launch_gather_ss(ctx, S, sample_bytes, interpolation);
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

extern "C" int amt_gather_mosaic_supersampled(amt_ctx* ctx, const amt_gather_member* members, int32_t n_members, int32_t frame,
                                              const double* sub_lat, int32_t ny, const double* sub_lon, int32_t nx,
                                              const double* sub_cell_lat, const double* sub_cell_lon, int32_t factor,
                                              int32_t min_count, int32_t sample_bytes, int32_t channels, int32_t interpolation,
                                              int32_t rule, void* out_img, uint8_t* out_mask, double* out_elev, int32_t* out_source,
                                              uint8_t* out_count, const amt_gather_debug* debug) {
    return gather_supersampled_call(ctx, __func__, members, n_members, frame, sub_lat, ny, sub_lon, nx, sub_cell_lat, sub_cell_lon, factor,
                                    min_count, sample_bytes, channels, interpolation, rule, out_img, out_mask, out_elev, out_source,
                                    out_count, debug, nullptr);
}

extern "C" int amt_gather_mosaic_supersampled_lens(amt_ctx* ctx, const amt_gather_member* members, int32_t n_members, int32_t frame,
                                                   const double* sub_lat, int32_t ny, const double* sub_lon, int32_t nx,
                                                   const double* sub_cell_lat, const double* sub_cell_lon, int32_t factor,
                                                   int32_t min_count, int32_t sample_bytes, int32_t channels, int32_t interpolation,
                                                   int32_t rule, void* out_img, uint8_t* out_mask, double* out_elev,
                                                   int32_t* out_source, uint8_t* out_count, const amt_gather_debug* debug,
                                                   const amt_lens_model* const* lenses) {
    return gather_supersampled_call(ctx, __func__, members, n_members, frame, sub_lat, ny, sub_lon, nx, sub_cell_lat, sub_cell_lon, factor,
                                    min_count, sample_bytes, channels, interpolation, rule, out_img, out_mask, out_elev, out_source,
                                    out_count, debug, lenses);
}

// The body of both entry points is an overload of the older one's name, not a gather_frames_call: the registry of scratch-memory
// users (tests/_scratch_cases.py, tests/test_scratch_cases_cpu.py) knows the call of amt_workspace below as amt_gather_frames'.
static int amt_gather_frames(amt_ctx* ctx, const char* fn, const amt_gather_job* jobs, int32_t n_jobs, int32_t frame, int32_t factor,
                             int32_t min_count, int32_t sample_bytes, int32_t channels, int32_t interpolation,
                             const amt_gather_debug* debug, const amt_lens_model* const* lenses) {
    AMT_CHECK_CTX(ctx);
    GATHER_REQUIRE(jobs, "NULL argument");
    GATHER_REQUIRE(n_jobs >= 1 && n_jobs <= AMT_GATHER_MAX_JOBS, "n_jobs must be 1 ... " + std::to_string(AMT_GATHER_MAX_JOBS));
    int rc = gather_check(ctx, fn, frame, interpolation, 1, sample_bytes, channels, debug);
    if (rc == AMT_OK) rc = gather_check_factor(ctx, fn, factor, min_count);
    if (rc != AMT_OK) return rc;

    // the prefix table of tile counts, then the jobs, in one staging buffer: one copy
    const size_t jobs_at = (((size_t)n_jobs + 1) * sizeof(int) + 15) & ~(size_t)15;
    const size_t lens_at = jobs_at + (size_t)n_jobs * sizeof(gather_job_dev);      // (a multiple of 8: the structs hold doubles)
    std::vector<unsigned char> staged(lens_at + (lenses ? (size_t)n_jobs * sizeof(w2p_lens) : 0));
    int* first = reinterpret_cast<int*>(staged.data());
    gather_job_dev* dev = reinterpret_cast<gather_job_dev*>(staged.data() + jobs_at);
    w2p_lens* lens = reinterpret_cast<w2p_lens*>(staged.data() + lens_at);
    bool any_lens = false;
    const int Tc = kTile / factor;          // cells per tile side
    int64_t tiles = 0;
    for (int32_t k = 0; k < n_jobs; ++k) {
        const amt_gather_job& j = jobs[k];
        const std::string job = "job " + std::to_string(k) + ": ";
        gather_job_dev& d = dev[k];
        GATHER_REQUIRE(j.out_img && j.out_mask && j.out_elev, job + "NULL argument");
        GATHER_REQUIRE(factor == 1 || j.out_count, job + "NULL out_count with factor > 1");
        GATHER_REQUIRE(j.ny > 0 && j.nx > 0, job + "empty axis");
        rc = gather_check_subgrid(ctx, fn, job, j.ny, j.nx, factor);
        if (rc == AMT_OK) rc = gather_coordinates(ctx, fn, job, j.lat, j.lon, j.cell_lat, j.cell_lon, d);
        if (rc != AMT_OK) return rc;
        const char* err = gather_member(j.member, lenses ? lenses[k] : nullptr, frame, d.M, lenses ? &lens[k] : nullptr);
        GATHER_REQUIRE(err == nullptr, job + err);
        any_lens = any_lens || (lenses && lens[k].m.kind != AMT_LENS_NONE);
        d.img = j.out_img, d.mask = j.out_mask, d.elev = j.out_elev, d.count = factor > 1 ? j.out_count : nullptr;
        d.ny = j.ny, d.nx = j.nx, d.tiles_x = (j.nx + Tc - 1) / Tc, d.pad_ = 0;
        first[k] = (int)tiles;
        tiles += (int64_t)d.tiles_x * (int64_t)((j.ny + Tc - 1) / Tc);
        GATHER_REQUIRE(tiles <= INT32_MAX, "the jobs' tiles (up to " + job + std::to_string(tiles) + ") do not fit one launch");
    }
    first[n_jobs] = (int)tiles;

    if (amt_set_device(ctx)) return AMT_EHIP;
    const size_t bytes = any_lens ? staged.size() : lens_at;      // (without a lens: the parent's buffer)
    char* ws = static_cast<char*>(amt_workspace(ctx, bytes));
    if (ws == nullptr) {
        ctx->last_error = std::string(fn) + ": workspace allocation failed";
        return AMT_ENOMEM;
    }
    // (pageable source: the copy has consumed the staging buffer when the call returns)
    AMT_HIP(ctx, hipMemcpyAsync(ws, staged.data(), bytes, hipMemcpyHostToDevice, ctx->stream));

    gather_frames_args F;
    F.first = reinterpret_cast<const int*>(ws);
    F.jobs = reinterpret_cast<const gather_job_dev*>(ws + jobs_at);
    F.lenses = any_lens ? reinterpret_cast<const w2p_lens*>(ws + lens_at) : nullptr;
    F.n_jobs = n_jobs, F.C = channels, F.force = debug ? debug->force_path : AMT_GATHER_PATH_AUTO, F.factor = factor;
    F.min_count = min_count, F.head = 0;
    F.tile_path = debug ? debug->tile_path : nullptr;
    launch_gather_frames(ctx, F, (int)tiles, sample_bytes, interpolation);
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

extern "C" int amt_gather_frames(amt_ctx* ctx, const amt_gather_job* jobs, int32_t n_jobs, int32_t frame, int32_t factor,
                                 int32_t min_count, int32_t sample_bytes, int32_t channels, int32_t interpolation,
                                 const amt_gather_debug* debug) {
    return amt_gather_frames(ctx, __func__, jobs, n_jobs, frame, factor, min_count, sample_bytes, channels, interpolation, debug, nullptr);
}

extern "C" int amt_gather_frames_lens(amt_ctx* ctx, const amt_gather_job* jobs, int32_t n_jobs, int32_t frame, int32_t factor,
                                      int32_t min_count, int32_t sample_bytes, int32_t channels, int32_t interpolation,
                                      const amt_gather_debug* debug, const amt_lens_model* const* lenses) {
    return amt_gather_frames(ctx, __func__, jobs, n_jobs, frame, factor, min_count, sample_bytes, channels, interpolation, debug, lenses);
}
