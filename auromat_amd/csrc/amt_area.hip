// Area-weighted (conservative) binning: a pixel is the quadrilateral of its four corners, and every cell of the output
// grid that the quadrilateral overlaps receives the pixel's values with the integer weight
//     W = rint(|area(quadrilateral ∩ cell)| / area(cell) * 2^32).
// No counterpart in the reference: resample(method='mean') puts a pixel into the one cell that holds its centre and
// leaves holes where the cells are smaller than the pixels.
//
// k_area_frame: one pixel per lane.  The accumulators have the layout of amt_bin_frame (int64, (nch + 2) planes of
// nx * ny cells, cell ix * ny + iy): plane 0 sum(W), plane 1 + k sum(W * v_k), the last plane sum(W * E) with
// E = rint(elev * 2^16).  Every accumulation is a 64-bit integer atomic, so the result is exact, independent of the
// order and bit-reproducible; tests/_area_oracle.py restates cell_weight() operation for operation in NumPy.
//
// Three regimes by the number of candidate cells of a pixel (the cells its bounding box meets):
//   * one cell (cells much larger than pixels) and a few cells (cells about as large as pixels): the lane walks its
//     own cells, at most kLaneCells of them, through the same cell_weight() — one code path, the same bits;
//   * many cells (a pixel near the limb on a fine grid covers thousands): such pixels are collected by ballot, their
//     quadrilaterals broadcast one at a time, and the wave's 64 lanes stride over the cells of each.
//
// No LDS privatisation.  Where it would find sharing — cells much larger than pixels, every pixel one cell — the mean
// binning does not leave holes and the area weights add little; the regime this pass exists for is the fine grid,
// where a (pixel, cell) pair is nearly unique (a cell meets about as many quadrilaterals as a quadrilateral meets
// cells), a window of u64 LDS counters (W has 33 bits, so the u32 window of amt_bin_tile.h does not do) would be
// filled and flushed with one global atomic per LDS atomic, and the large quadrilaterals fall outside any window.
// The global atomics of a wave go to neighbouring cells of one or two grid columns (iy runs fastest).
//
// Area-weighted mosaics (amt_area_mosaic_frames, auromat_amd.resample.resampleMosaic(statistic='area')): the members of a
// collection on ONE grid in a fixed number of launches whatever the member count, as amt_mosaic.hip does for the mean.  The
// member table is uploaded, the members' window accumulators and the overflow flag are zeroed by one memset, one launch of
// k_area_frame<..., WIN = true> bins every member (a workgroup finds its member through a prefix of workgroups per member; a
// pixel's candidate cells are cut to the member's window BEFORE the choice between the lane and the wave path, and the window
// planes are column-major with iy fastest like the grid's, so a wave's atomics keep their layout), and k_area_select gives every
// cell its value by the overlap rule with the finalise arithmetic of k_area_finalize (area_finalize_cell, shared by both).
//
// On a map plane (amt_area_plane_frame, auromat_amd.resample.resampleStereographic and its kin): k_area_frame<..., PLANE = true>
// takes the corners' projected x and y (amt_project.hip) on uniform axes in the plane's unit.  x is no longitude there: no wrap,
// and no rule on a quadrilateral's x extent; everything else is the frame's, bit for bit.
#include <algorithm>
#include <type_traits>

#include "amt_common.h"
#include "amt_frame_src.h"
#include "amt_mosaic_plan.h"

namespace {

using namespace amt;

constexpr int kAreaBlock = 256;
static_assert(kAreaBlock == kBlock, "grid_for counts workgroups of kBlock threads");
constexpr int kLaneCells = 16;                   // a pixel with more candidate cells is walked by the whole wave
constexpr double kWeightOne = 4294967296.0;      // 2^32: the weight of a cell that a pixel covers whole
constexpr double kElevFix = 65536.0;             // 2^16: E = rint(elev * 2^16)
constexpr unsigned long long kWeightLimit = 1ull << 40;   // a cell covered more than 256 times over: AMT_EDOMAIN

struct area_args {
    frame_src S;             // (of the centres, the latitude decides whether a pixel counts; lon_c is not read)
    const double* lat;       // corners, (height + 1) x (width + 1)
    const double* lon;
    const void* img;
    int nch;
    unsigned long long* acc;
};

// The members of an area-weighted mosaic: one descriptor per member in device memory, and the first workgroup of every
// member (a prefix over the members' workgroups, n + 1 entries).
struct area_member {
    area_args A;            // the member's frame on the common axes; A.acc = its window planes
    cell_window W;          // the cells of the common grid the member keeps (amt_mosaic_plan.h)
};
struct area_mosaic_args {
    const area_member* __restrict__ members;
    const int* __restrict__ block_start;
    int n;
};

// The frame of a sequence (amt_area_frame_async): only the pixels of the rows [row_begin, row_end) are visited.
struct area_seq_args : area_args {
    int row_begin, row_end;
};

template <bool WIN, bool SEQ, bool PLANE = false> struct area_kernel_args { using type = area_args; };
template <> struct area_kernel_args<true, false, false> { using type = area_mosaic_args; };
template <> struct area_kernel_args<false, true, false> { using type = area_seq_args; };

__device__ __forceinline__ const area_args& frame_args(const area_args& A, int) { return A; }
__device__ __forceinline__ const area_args& frame_args(const area_mosaic_args& M, int m) { return M.members[m].A; }
// SEQ: the band of pixels the sweep covers
__device__ __forceinline__ int64_t first_pixel(const area_seq_args& K) { return (int64_t)K.row_begin * K.S.width; }
__device__ __forceinline__ int64_t end_pixel(const area_seq_args& K) { return (int64_t)K.row_end * K.S.width; }

// Edge i of an axis: the double bin_index compares against.
__device__ __forceinline__ double axis_edge(const axis_dev& ax, int i) {
    return ax.uniform ? linspace_edge(ax, i) : ax.edges[i];
}

__device__ __forceinline__ double clamp_to(double v, double hi) { return fmin(fmax(v, 0.0), hi); }

// W of the quadrilateral (X[i], Y[i]), i = 0..3 in order, and the cell [x0, x1] x [y0, y1].
//
// The signed area of quadrilateral ∩ cell is the boundary integral of clamp(y, 0, b) d clamp(x, 0, a) over the
// quadrilateral's edges in cell-relative coordinates (the change of variables (x, y) -> (clamp x, clamp y) maps the
// polygon onto its clipped self, winding included, so concave and self-intersecting quadrilaterals need no case).
// Every edge is split at its at most four crossings with the lines x = 0, x = a, y = 0, y = b; on each piece both
// clamped coordinates are linear, and the piece contributes one trapezoid.  Only + - * /, min, max, |.| and rint, each
// rounded on its own (no contraction): NumPy computes the same bits.
__device__ __forceinline__ unsigned long long cell_weight(const double (&X)[4], const double (&Y)[4], double x0, double x1,
                                                          double y0, double y1) {
#pragma clang fp contract(off)
    const double a = x1 - x0, b = y1 - y0;
    double px[4], py[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        px[i] = X[i] - x0;
        py[i] = Y[i] - y0;
    }
    double S = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double ax_ = px[i], ay_ = py[i], bx_ = px[(i + 1) & 3], by_ = py[(i + 1) & 3];
        const double dx = bx_ - ax_, dy = by_ - ay_;
        // parameters of the crossings, 0 where the edge is parallel to the line (that piece then adds nothing new)
        double t0 = dx != 0.0 ? (0.0 - ax_) / dx : 0.0;
        double t1 = dx != 0.0 ? (a - ax_) / dx : 0.0;
        double t2 = dy != 0.0 ? (0.0 - ay_) / dy : 0.0;
        double t3 = dy != 0.0 ? (b - ay_) / dy : 0.0;
        t0 = clamp_to(t0, 1.0);
        t1 = clamp_to(t1, 1.0);
        t2 = clamp_to(t2, 1.0);
        t3 = clamp_to(t3, 1.0);
        // sorting network of four: (0,1) (2,3) (0,2) (1,3) (1,2)
        double lo, hi;
        lo = fmin(t0, t1); hi = fmax(t0, t1); t0 = lo; t1 = hi;
        lo = fmin(t2, t3); hi = fmax(t2, t3); t2 = lo; t3 = hi;
        lo = fmin(t0, t2); hi = fmax(t0, t2); t0 = lo; t2 = hi;
        lo = fmin(t1, t3); hi = fmax(t1, t3); t1 = lo; t3 = hi;
        lo = fmin(t1, t2); hi = fmax(t1, t2); t1 = lo; t2 = hi;
        const double ts[4] = {t0, t1, t2, t3};
        double ux = clamp_to(ax_, a), uy = clamp_to(ay_, b);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            double x, y;
            if (k < 4) {
                const double mx = ts[k] * dx, my = ts[k] * dy;
                x = ax_ + mx;
                y = ay_ + my;
            } else {
                x = bx_;        // the edge ends at its end point exactly: the boundary closes
                y = by_;
            }
            const double vx = clamp_to(x, a), vy = clamp_to(y, b);
            const double w = vx - ux, h = uy + vy;
            const double piece = w * h;
            S = S + piece;
            ux = vx;
            uy = vy;
        }
    }
    const double A = fabs(S) * 0.5;
    const double cell = a * b;
    const double f = A / cell;
    const double scaled = f * kWeightOne;
    return (unsigned long long)rint(scaled);
}

struct area_pixel {
    double X[4], Y[4];
    int ix0, iy0, nxr, nyr;          // candidate cells [ix0, ix0 + nxr) x [iy0, iy0 + nyr); nxr = 0: the pixel takes no part
    unsigned int ch[4];
    long long E;
};

// Adds the pixel's share of candidate cell (jx, jy) of its range to the accumulators (WIN: of the member's window Wn, which
// holds the whole range).
template <bool WIN>
__device__ __forceinline__ void add_cell(const area_args& A, const cell_window& Wn, const area_pixel& P, int jx, int jy,
                                         int64_t plane) {
    const int ix = P.ix0 + jx, iy = P.iy0 + jy;
    const unsigned long long W = cell_weight(P.X, P.Y, axis_edge(A.S.ax, ix), axis_edge(A.S.ax, ix + 1), axis_edge(A.S.ay, iy),
                                             axis_edge(A.S.ay, iy + 1));
    if (W == 0) return;
    const int64_t cell = WIN ? (int64_t)(ix - Wn.x0) * Wn.ny + (iy - Wn.y0) : (int64_t)ix * A.S.ay.nbin + iy;
    atomicAdd(&A.acc[cell], W);
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < A.nch) atomicAdd(&A.acc[(int64_t)(1 + c) * plane + cell], W * (unsigned long long)P.ch[c]);
    atomicAdd(&A.acc[(int64_t)(1 + A.nch) * plane + cell], (unsigned long long)((long long)W * P.E));
}

// WIN = false: the argument is the frame (area_args); the whole grid is kept (ax.nbin x ay.nbin cells per plane).
// WIN = true (the binning of amt_area_mosaic_frames): the argument is the member table (area_mosaic_args); the workgroup finds
// its member by the workgroup prefix, sweeps that member's pixels with the member's other workgroups and keeps only the cells of
// the member's window.  The weights and the sums are the same integers either way.
// SEQ = true (amt_area_frame_async; not with WIN): the argument is the frame with a row band and the MLT switch (area_seq_args);
// the sweep covers the pixels of the band only, whole waves from its first pixel on.
// PLANE = true (amt_area_plane_frame; not with WIN or SEQ): the corner arrays hold the x and y of a map plane.  x is no
// longitude: no wrap, and no limit on a quadrilateral's x extent.  Everything else is the frame's.
template <typename IMG_T, bool WIN, bool SEQ = false, bool PLANE = false>
__global__ __launch_bounds__(kAreaBlock) void k_area_frame(typename area_kernel_args<WIN, SEQ, PLANE>::type K) {
    static_assert(!(WIN && SEQ), "a mosaic member has no row band");
    static_assert(!(PLANE && (WIN || SEQ)), "the plane form is the plain frame's");
    int member = 0;
    if constexpr (WIN) member = member_of(K.block_start, K.n, blockIdx.x);
    // (the frame: the kernel argument itself; a member: its descriptor copied into registers once, so that the global
    //  atomics below, which may alias the table for all the compiler knows, do not make every use reload it)
    typename std::conditional<WIN, const area_args, const area_args&>::type A = frame_args(K, member);
    const frame_src& S = A.S;
    cell_window Wn{0, 0, 0, 0};
    unsigned block0 = 0, nblocks = gridDim.x;
    if constexpr (WIN) {
        Wn = K.members[member].W;
        block0 = (unsigned)K.block_start[member];
        nblocks = (unsigned)K.block_start[member + 1] - block0;
    }
    int64_t pix0 = 0, npix = (int64_t)S.height * S.width;
    if constexpr (SEQ) pix0 = first_pixel(K), npix = end_pixel(K);
    const int64_t plane = WIN ? (int64_t)Wn.nx * Wn.ny : (int64_t)S.ax.nbin * S.ay.nbin;
    const int lane = threadIdx.x & 63;
    const IMG_T* img = static_cast<const IMG_T*>(A.img);
    // (whole waves run every iteration: the cooperative part below needs all 64 lanes)
    const int64_t per_sweep = (int64_t)nblocks * kAreaBlock;
    for (int64_t base = pix0 + (int64_t)(blockIdx.x - block0) * kAreaBlock + (threadIdx.x & ~63); base < npix; base += per_sweep) {
        const int64_t p = base + lane;
        area_pixel P;
        P.nxr = P.nyr = 0;
        P.ix0 = P.iy0 = 0;
        P.E = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            P.X[i] = P.Y[i] = 0.0;
            P.ch[i] = 0;
        }
        if (p < npix) {
            const int r = (int)(p / S.width), c = (int)(p - (int64_t)r * S.width);
            const double ev = S.elev ? S.elev[p] : 0.0;
            if (src_keeps(S, S.lat_c[p], ev, S.mask ? S.mask[p] : 0u)) {
                // corners (r, c), (r, c + 1), (r + 1, c + 1), (r + 1, c)
                const int64_t q = (int64_t)r * (S.width + 1) + c;
                const int64_t at[4] = {q, q + 1, q + S.width + 2, q + S.width + 1};
                double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
                bool fin = true;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double lo = A.lon[at[i]], la = A.lat[at[i]];
                    fin = fin && finite(lo) && finite(la);
                    const double x = PLANE ? lo : src_x(S, lo);        // (a plane's x is no longitude)
                    P.X[i] = x;
                    P.Y[i] = la;
                    xmin = fmin(xmin, x); xmax = fmax(xmax, x);
                    ymin = fmin(ymin, la); ymax = fmax(ymax, la);
                }
                // (a quadrilateral as wide as half the globe straddles the seam of the longitudes; a plane has no seam)
                if (fin && (PLANE || xmax - xmin < 180.0) && xmax > S.ax.e0 && xmin < S.ax.e_last && ymax > S.ay.e0 &&
                    ymin < S.ay.e_last) {
                    // edges[g] <= v < edges[g + 1] for the bin g + 1 of bin_index: no cell below that of the minimum or
                    // above that of the maximum meets the quadrilateral
                    const int nbx = S.ax.nbin, nby = S.ay.nbin;
                    int ix0 = min(max(bin_index(S.ax, xmin) - 1, 0), nbx - 1);
                    int ix1 = min(max(bin_index(S.ax, xmax) - 1, 0), nbx - 1);
                    int iy0 = min(max(bin_index(S.ay, ymin) - 1, 0), nby - 1);
                    int iy1 = min(max(bin_index(S.ay, ymax) - 1, 0), nby - 1);
                    if (WIN) {
                        // the range is cut to the window before the path is chosen: what is left decides lane or wave
                        ix0 = max(ix0, Wn.x0);
                        ix1 = min(ix1, Wn.x0 + Wn.nx - 1);
                        iy0 = max(iy0, Wn.y0);
                        iy1 = min(iy1, Wn.y0 + Wn.ny - 1);
                    }
                    if (!WIN || (ix1 >= ix0 && iy1 >= iy0)) {
                        P.ix0 = ix0;
                        P.iy0 = iy0;
                        P.nxr = ix1 - ix0 + 1;
                        P.nyr = iy1 - iy0 + 1;
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (k < A.nch) P.ch[k] = img[p * A.nch + k];
                        // (a NaN elevation of an admitted pixel contributes 0, as in amt_bin_tile.h)
                        P.E = (ev == ev) ? (long long)rint(ev * kElevFix) : 0;
                    }
                }
            }
        }
        const long long ncells = (long long)P.nxr * P.nyr;
        const bool wide = ncells > kLaneCells;
        if (!wide)
            for (int jx = 0; jx < P.nxr; ++jx)
                for (int jy = 0; jy < P.nyr; ++jy) add_cell<WIN>(A, Wn, P, jx, jy, plane);
        // the wide quadrilaterals of this wave, one at a time over all 64 lanes
        unsigned long long todo = __ballot(wide);
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            area_pixel Q;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                Q.X[i] = __shfl(P.X[i], src);
                Q.Y[i] = __shfl(P.Y[i], src);
                Q.ch[i] = __shfl(P.ch[i], src);
            }
            Q.ix0 = __shfl(P.ix0, src);
            Q.iy0 = __shfl(P.iy0, src);
            Q.nxr = __shfl(P.nxr, src);
            Q.nyr = __shfl(P.nyr, src);
            Q.E = __shfl(P.E, src);
            // lane l takes cells l, l + 64, ... of the range in the order jx * nyr + jy; the step of 64 cells is split into
            // whole columns and a rest once per quadrilateral, so that no cell costs a division
            const int step_x = 64 / Q.nyr, step_y = 64 - step_x * Q.nyr;
            int jx = lane / Q.nyr, jy = lane - jx * Q.nyr;
            while (jx < Q.nxr) {
                add_cell<WIN>(A, Wn, Q, jx, jy, plane);
                jx += step_x;
                jy += step_y;
                if (jy >= Q.nyr) {
                    jy -= Q.nyr;
                    jx += 1;
                }
            }
        }
    }
}

// The finalise arithmetic of one cell, for k_area_finalize and k_area_select alike: w = sum(W), sum(k) the cell's plane 1 + k
// (k = nch: sum(W * E)), read only where it is needed; output cell i.  A cell is valid when w reaches min_weight.
template <typename IMG_T, typename SUM>
__device__ __forceinline__ void area_finalize_cell(unsigned long long w, unsigned long long min_weight, SUM sum, int nch, int64_t i,
                                                   double* __restrict__ area, IMG_T* __restrict__ out_img,
                                                   uint8_t* __restrict__ out_mask, double* __restrict__ out_coverage) {
#pragma clang fp contract(off)
    const bool valid = w >= min_weight;
    const double dw = (double)w;
    for (int k = 0; k < nch; ++k) {
        const double m = valid ? (double)sum(k) / dw : NAN;
        if (area) area[i * (nch + 1) + k] = m;
        if (out_img) out_img[i * nch + k] = valid ? (IMG_T)rint(m) : (IMG_T)0;
    }
    if (area) {
        const double e = (double)(long long)sum(nch) / dw;
        area[i * (nch + 1) + nch] = valid ? e / kElevFix : NAN;
    }
    if (out_mask) out_mask[i] = valid ? 0 : 1;
    if (out_coverage) out_coverage[i] = dw / kWeightOne;
}

// Transpose + flipud as k_bin_finalize; a cell is valid when its total weight reaches min_weight.
template <typename IMG_T>
__global__ void k_area_finalize(const unsigned long long* __restrict__ acc, int nx, int ny, int nch,
                                unsigned long long min_weight, double* __restrict__ area, IMG_T* __restrict__ out_img,
                                uint8_t* __restrict__ out_mask, double* __restrict__ out_coverage,
                                unsigned int* __restrict__ over) {
    const int64_t n = (int64_t)nx * ny;
    bool too_much = false;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / nx), c = (int)(i - (int64_t)r * nx);
        const int64_t cell = (int64_t)c * ny + (ny - 1 - r);
        const unsigned long long w = acc[cell];
        too_much = too_much || w > kWeightLimit;
        area_finalize_cell(w, min_weight, [&](int k) { return acc[(int64_t)(1 + k) * n + cell]; }, nch, i, area, out_img,
                           out_mask, out_coverage);
    }
    if (too_much) atomicOr(over, 1u);
}

struct area_select_args {
    const area_member* __restrict__ members;
    const int* __restrict__ list_start;     // CSR per 16 x 16 tile of cells: members whose window meets the tile,
    const int* __restrict__ list;           // ascending
    int tiles_y;                            // tiles along the (ascending) latitude bins
    int nx, ny, nch, rule;
    unsigned long long min_weight;          // >= 1
    double* area;
    void* img;
    uint8_t* mask;
    double* coverage;
    int32_t* source;
    unsigned int* over;
};

// One thread per output cell: the cell's tile's members, in ascending order.
// rule 0: the accumulators of every member added (source: the first member with weight there, where the total is valid);
// rule 1: of the members whose OWN weight in the cell reaches min_weight, the one with the largest (double)(int64)sum(W * E) /
// (double)sum(W) — the quotient area_finalize_cell forms — the first on a tie; without such a member the cell is masked and
// its coverage is the largest single weight.  Then area_finalize_cell.  The flag: a member's weight in a cell, or under rule 0
// a cell's total, above 2^40 (below it no sum can wrap: the members' weights are checked one by one, so the total of n members
// stays below n * 2^40 < 2^64 while it is compared).
template <typename IMG_T>
__global__ __launch_bounds__(kSelTile * kSelTile) void k_area_select(area_select_args S) {
#pragma clang fp contract(off)
    int cx, cy;
    const int64_t i = select_cell(S.tiles_y, S.nx, S.ny, cx, cy);
    if (i < 0) return;
    const int nch = S.nch;
    // the cell's sum(W), channel sums and sum(W * E): the total (rule 0) or the elected member's (rule 1; before a member is
    // elected w is the largest weight seen)
    unsigned long long w = 0, s0 = 0, s1 = 0, s2 = 0, s3 = 0, se = 0;
    int src = -1;
    double best = 0.0;
    bool too_much = false;
    walk_tile_members(S.members, S.list_start, S.list, cx, cy,
                      [&](int m, const unsigned long long* acc, int64_t plane, int64_t cell) {
        const unsigned long long c = acc[cell];
        if (c == 0) return;
        too_much = too_much || c > kWeightLimit;
        if (S.rule == 0) {
            w += c;
            if (0 < nch) s0 += acc[1 * plane + cell];
            if (1 < nch) s1 += acc[2 * plane + cell];
            if (2 < nch) s2 += acc[3 * plane + cell];
            if (3 < nch) s3 += acc[4 * plane + cell];
            se += acc[(int64_t)(1 + nch) * plane + cell];
            if (src < 0) src = m;
        } else if (c >= S.min_weight) {
            const unsigned long long f = acc[(int64_t)(1 + nch) * plane + cell];
            const double el = (double)(long long)f / (double)c;
            if (src < 0 || el > best) {
                src = m;
                best = el;
                w = c;
                if (0 < nch) s0 = acc[1 * plane + cell];
                if (1 < nch) s1 = acc[2 * plane + cell];
                if (2 < nch) s2 = acc[3 * plane + cell];
                if (3 < nch) s3 = acc[4 * plane + cell];
                se = f;
            }
        } else if (src < 0 && c > w) {
            w = c;
        }
    });
    if (S.rule == 0) {
        too_much = too_much || w > kWeightLimit;
        if (w < S.min_weight) src = -1;
    }
    area_finalize_cell(w, S.min_weight,
                       [&](int k) { return k == nch ? se : (k == 0 ? s0 : (k == 1 ? s1 : (k == 2 ? s2 : s3))); }, nch, i, S.area,
                       static_cast<IMG_T*>(S.img), S.mask, S.coverage);
    if (S.source) S.source[i] = src;
    if (too_much) atomicOr(S.over, 1u);
}

// The frame of amt_area_frame, amt_area_plane_frame, amt_area_frame_async and of a mosaic's member as the kernel takes it, with
// the checks they share beside make_frame_src's.  The centres' longitudes are not among an entry point's arguments and are not
// read (the corners' are): S.lon_c stands on lat_c.  Returns what is wrong, or NULL.
const char* make_area_frame(area_args* A, const double* lat, const double* lon, const double* lat_c, const double* elev,
                            const void* img, int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height,
                            int32_t width, double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap,
                            int lon_from_mlt, unsigned long long* acc) {
    if (!(lat && lon)) return "NULL argument";
    if (const char* bad = make_frame_src(&A->S, lat_c, lat_c, elev, center_mask, height, width, min_elevation, xaxis, yaxis,
                                         lon_wrap, lon_from_mlt))
        return bad;
    if (!((int64_t)(height + 1) * (width + 1) < ((int64_t)1 << 31))) return "frames below 2^31 pixels";
    if (!(nchan >= 0 && nchan <= 4)) return "nchan must be 0..4";
    if (!(nchan == 0 || (img && (img_dtype == 1 || img_dtype == 2)))) return "img must be uint8 (1) or uint16 (2)";
    if (!(xaxis->nbin < 65535 && yaxis->nbin < 65535)) return "at most 65534 bins per axis";
    A->lat = lat;
    A->lon = lon;
    A->img = img;
    A->nch = nchan;
    A->acc = acc;
    return nullptr;
}

// Reads the overflow word of a finalise or select launch back (waits for the stream): AMT_EDOMAIN when it is set, with
// "<entry>: <what> exceeds 2^40 ..." as the error.
int area_overflow_status(amt_ctx* ctx, const unsigned int* over, const char* entry, const char* what) {
    unsigned int flag = 0;
    AMT_HIP(ctx, hipMemcpyAsync(&flag, over, sizeof(flag), hipMemcpyDeviceToHost, ctx->stream));
    AMT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (flag) {
        ctx->last_error = std::string(entry) + ": " + what + " exceeds 2^40 (covered more than 256 times over)";
        return AMT_EDOMAIN;
    }
    return AMT_OK;
}

}  // namespace

extern "C" {

int amt_area_frame(amt_ctx* ctx, const double* lat, const double* lon, const double* lat_c, const double* elev, const void* img,
                   int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height, int32_t width,
                   double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap, uint64_t* acc) {
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, acc != nullptr, "NULL argument");
    area_args A;
    const char* bad = make_area_frame(&A, lat, lon, lat_c, elev, img, img_dtype, nchan, center_mask, height, width, min_elevation,
                                      xaxis, yaxis, lon_wrap, 0, reinterpret_cast<unsigned long long*>(acc));
    AMT_REQUIRE(ctx, bad == nullptr, bad);
    const dim3 grid = grid_for((int64_t)height * width), block(kAreaBlock);
    if (img_dtype == 2)
        hipLaunchKernelGGL((k_area_frame<uint16_t, false>), grid, block, 0, ctx->stream, A);
    else
        hipLaunchKernelGGL((k_area_frame<uint8_t, false>), grid, block, 0, ctx->stream, A);
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

int amt_area_plane_frame(amt_ctx* ctx, const double* x, const double* y, const double* lat_c, const double* elev,
                         const void* img, int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height,
                         int32_t width, double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, uint64_t* acc) {
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, acc != nullptr, "NULL argument");
    area_args A;
    const char* bad = make_area_frame(&A, y, x, lat_c, elev, img, img_dtype, nchan, center_mask, height, width, min_elevation,
                                      xaxis, yaxis, 0, 0, reinterpret_cast<unsigned long long*>(acc));
    AMT_REQUIRE(ctx, bad == nullptr, bad);
    AMT_REQUIRE(ctx, xaxis->uniform && yaxis->uniform, "the axes of a map plane are uniform");
    const dim3 grid = grid_for((int64_t)height * width), block(kAreaBlock);
    if (img_dtype == 2)
        hipLaunchKernelGGL((k_area_frame<uint16_t, false, false, true>), grid, block, 0, ctx->stream, A);
    else
        hipLaunchKernelGGL((k_area_frame<uint8_t, false, false, true>), grid, block, 0, ctx->stream, A);
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

int amt_area_frame_finalize(amt_ctx* ctx, const uint64_t* acc, int32_t nx, int32_t ny, int32_t nchan, int32_t img_dtype,
                            uint64_t min_weight, double* area, void* out_img, uint8_t* out_mask, double* out_coverage) {
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, acc != nullptr, "NULL argument");
    AMT_REQUIRE(ctx, nx > 0 && ny > 0 && nchan >= 0 && nchan <= 4, "bad shape");
    AMT_REQUIRE(ctx, out_img == nullptr || img_dtype == 1 || img_dtype == 2, "img must be uint8 (1) or uint16 (2)");
    unsigned int* over = static_cast<unsigned int*>(amt_workspace(ctx, sizeof(unsigned int)));
    if (over == nullptr) {
        ctx->last_error = "amt_area_frame_finalize: no device memory for the workspace";
        return AMT_ENOMEM;
    }
    AMT_HIP(ctx, hipMemsetAsync(over, 0, sizeof(unsigned int), ctx->stream));
    const unsigned long long least = min_weight < 1 ? 1ull : (unsigned long long)min_weight;
    const dim3 grid = grid_for((int64_t)nx * ny), block(kAreaBlock);
    const unsigned long long* a = reinterpret_cast<const unsigned long long*>(acc);
    if (img_dtype == 2)
        hipLaunchKernelGGL((k_area_finalize<uint16_t>), grid, block, 0, ctx->stream, a, nx, ny, nchan, least, area,
                           static_cast<uint16_t*>(out_img), out_mask, out_coverage, over);
    else
        hipLaunchKernelGGL((k_area_finalize<uint8_t>), grid, block, 0, ctx->stream, a, nx, ny, nchan, least, area,
                           static_cast<uint8_t*>(out_img), out_mask, out_coverage, over);
    AMT_LAUNCH_CHECK(ctx);
    return area_overflow_status(ctx, over, "amt_area_frame_finalize", "a cell's total weight");
}

int amt_area_frame_async(amt_ctx* ctx, const double* lat, const double* lon, const double* lat_c, const double* elev,
                         const void* img, int32_t img_dtype, int32_t nchan, const uint8_t* center_mask, int32_t height,
                         int32_t width, double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap,
                         int lon_from_mlt, int32_t row_begin, int32_t row_end, uint64_t min_weight, double* area, void* out_img,
                         uint8_t* out_mask, double* out_coverage, uint32_t* over) {
    AMT_CHECK_CTX(ctx);
    area_seq_args S;
    const char* bad = make_area_frame(&S, lat, lon, lat_c, elev, img, img_dtype, nchan, center_mask, height, width, min_elevation,
                                      xaxis, yaxis, lon_wrap, lon_from_mlt, nullptr);
    AMT_REQUIRE(ctx, bad == nullptr, bad);
    AMT_REQUIRE(ctx, out_img == nullptr || img_dtype == 1 || img_dtype == 2, "img must be uint8 (1) or uint16 (2)");
    AMT_REQUIRE(ctx, 0 <= row_begin && row_begin <= row_end && row_end <= height, "0 <= row_begin <= row_end <= height");
    if (amt_set_device(ctx)) return AMT_EHIP;
    // the workspace: the accumulator planes, then a word for the flag of a caller that passes none; zeroed together
    const int nx = xaxis->nbin, ny = yaxis->nbin;
    const size_t acc_bytes = (size_t)(nchan + 2) * (size_t)nx * (size_t)ny * sizeof(unsigned long long);
    char* ws = static_cast<char*>(amt_workspace(ctx, acc_bytes + 256));
    if (ws == nullptr) {
        ctx->last_error = "amt_area_frame_async: no device memory for the workspace";
        return AMT_ENOMEM;
    }
    AMT_HIP(ctx, hipMemsetAsync(ws, 0, acc_bytes + 256, ctx->stream));
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(ws);
    unsigned int* flag = over ? over : reinterpret_cast<unsigned int*>(ws + acc_bytes);
    S.acc = acc;
    S.row_begin = row_begin;
    S.row_end = row_end;
    const dim3 block(kAreaBlock);
    const dim3 grid = grid_for((int64_t)(row_end - row_begin) * width);
    if (img_dtype == 2)
        hipLaunchKernelGGL((k_area_frame<uint16_t, false, true>), grid, block, 0, ctx->stream, S);
    else
        hipLaunchKernelGGL((k_area_frame<uint8_t, false, true>), grid, block, 0, ctx->stream, S);
    AMT_LAUNCH_CHECK(ctx);
    const unsigned long long least = min_weight < 1 ? 1ull : (unsigned long long)min_weight;
    const dim3 fgrid = grid_for((int64_t)nx * ny);
    if (img_dtype == 2)
        hipLaunchKernelGGL((k_area_finalize<uint16_t>), fgrid, block, 0, ctx->stream, acc, nx, ny, nchan, least, area,
                           static_cast<uint16_t*>(out_img), out_mask, out_coverage, flag);
    else
        hipLaunchKernelGGL((k_area_finalize<uint8_t>), fgrid, block, 0, ctx->stream, acc, nx, ny, nchan, least, area,
                           static_cast<uint8_t*>(out_img), out_mask, out_coverage, flag);
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

int amt_area_mosaic_frames(amt_ctx* ctx, const amt_area_mosaic_member* members, int32_t n_members, int32_t img_dtype,
                           int32_t nchan, double min_elevation, const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap,
                           int32_t rule, uint64_t min_weight, double* area, void* out_img, uint8_t* out_mask,
                           double* out_coverage, int32_t* out_source) {
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, members && xaxis && yaxis, "NULL argument");
    AMT_REQUIRE(ctx, out_img == nullptr || img_dtype == 1 || img_dtype == 2, "img must be uint8 (1) or uint16 (2)");
    const int nx = xaxis->nbin, ny = yaxis->nbin;
    const char* bad = mosaic_members_bad(members, n_members, rule, nchan, axis_ok(xaxis) && axis_ok(yaxis), nx, ny,
                                         [](const amt_area_mosaic_member& m) -> const char* {
        if (!(m.lat && m.lon && m.lat_c)) return "member without corners or centres";
        if (!(m.height > 0 && m.width > 0)) return "empty member";
        if (!((int64_t)(m.height + 1) * (m.width + 1) < ((int64_t)1 << 31))) return "members below 2^31 pixels";
        return nullptr;
    });
    AMT_REQUIRE(ctx, bad == nullptr, bad);
    AMT_REQUIRE(ctx, nchan == 0 || img_dtype == 1 || img_dtype == 2, "member image missing");
    if (amt_set_device(ctx)) return AMT_EHIP;

    mosaic_plan P;
    const bool fits = plan_members(P, members, n_members, nx, ny, nchan, [](const amt_area_mosaic_member& m) {
        return grid_for((int64_t)m.height * m.width).x;
    });
    AMT_REQUIRE(ctx, fits, "too many workgroups");
    plan_select_lists(P);

    // the workspace: member descriptors | workgroup prefix [n + 1] | CSR of the select tiles (one upload); then the flag and
    // the accumulators, zeroed together
    std::vector<area_member> dev((size_t)n_members);
    workspace_packer K;
    const size_t o_dev = K.upload(dev.data(), dev.size() * sizeof(area_member));     // (filled below, copied by K.host())
    const size_t o_bstart = K.upload(P.unit_start.data(), P.unit_start.size() * sizeof(int));
    const size_t o_lstart = K.upload(P.list_start.data(), P.list_start.size() * sizeof(int));
    const size_t o_list = K.upload(P.list.data(), P.list.size() * sizeof(int));
    const size_t o_flag = K.add(256);
    const size_t o_acc = K.add(P.acc_words * sizeof(unsigned long long));
    char* ws = static_cast<char*>(amt_workspace(ctx, K.total()));
    if (ws == nullptr) {
        ctx->last_error = "amt_area_mosaic_frames: no device memory for the workspace";
        return AMT_ENOMEM;
    }
    unsigned int* over = reinterpret_cast<unsigned int*>(ws + o_flag);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(ws + o_acc);

    for (int32_t i = 0; i < n_members; ++i) {
        const amt_area_mosaic_member& m = members[i];
        bad = make_area_frame(&dev[(size_t)i].A, m.lat, m.lon, m.lat_c, m.elev, m.img, img_dtype, nchan, m.center_mask, m.height,
                              m.width, min_elevation, xaxis, yaxis, lon_wrap, 0, acc + P.acc_off[(size_t)i]);
        AMT_REQUIRE(ctx, bad == nullptr, bad);          // (mosaic_members_bad has looked at every member)
        dev[(size_t)i].W = P.win[(size_t)i];
    }
    // (pageable source: the copy has consumed the staging buffer when the call returns)
    const std::vector<char> host = K.host();
    AMT_HIP(ctx, hipMemcpyAsync(ws + o_dev, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream));
    AMT_HIP(ctx, hipMemsetAsync(over, 0, K.total() - o_flag, ctx->stream));

    if (P.units > 0) {
        area_mosaic_args M;
        M.members = reinterpret_cast<const area_member*>(ws + o_dev);
        M.block_start = reinterpret_cast<const int*>(ws + o_bstart);
        M.n = n_members;
        const dim3 grid((unsigned)P.units), block(kAreaBlock);
        if (img_dtype == 2)
            hipLaunchKernelGGL((k_area_frame<uint16_t, true>), grid, block, 0, ctx->stream, M);
        else
            hipLaunchKernelGGL((k_area_frame<uint8_t, true>), grid, block, 0, ctx->stream, M);
        AMT_LAUNCH_CHECK(ctx);
    }

    area_select_args S;
    S.members = reinterpret_cast<const area_member*>(ws + o_dev);
    S.list_start = reinterpret_cast<const int*>(ws + o_lstart);
    S.list = reinterpret_cast<const int*>(ws + o_list);
    S.tiles_y = P.sty;
    S.nx = nx;
    S.ny = ny;
    S.nch = nchan;
    S.rule = rule;
    S.min_weight = min_weight < 1 ? 1ull : (unsigned long long)min_weight;
    S.area = area;
    S.img = out_img;
    S.mask = out_mask;
    S.coverage = out_coverage;
    S.source = out_source;
    S.over = over;
    const dim3 sgrid((unsigned)(P.stx * P.sty)), sblock(kSelTile * kSelTile);
    if (img_dtype == 2)
        hipLaunchKernelGGL(k_area_select<uint16_t>, sgrid, sblock, 0, ctx->stream, S);
    else
        hipLaunchKernelGGL(k_area_select<uint8_t>, sgrid, sblock, 0, ctx->stream, S);
    AMT_LAUNCH_CHECK(ctx);
    return area_overflow_status(ctx, over, "amt_area_mosaic_frames",
                                rule == 0 ? "a cell's total weight" : "a member's weight in a cell");
}

}  // extern "C"
