// The scan-line map of a sequence (reference auromat/draw.py:589-879, drawScanLinesCo): every frame contributes the strip of
// its resampled cells that lie inside a narrow polygon through its centroid, and the strips of all frames lie side by side on
// one raster, later frames over earlier ones.
//
//   k_scanline_select  which cells of ONE resampled (plate carree) frame lie in its strip: a cell is kept iff it is unmasked and
//                      all four of its corners are inside the polygon — the rule of BaseMapping.maskedByPolygon, with the
//                      corner test of k_points_in_polygon (amt_polygon.h: the same expression, the same bits).  A resampled
//                      frame's corners are the outer product of two 1-D axes, so the kernel reads the axes and never the 2-D
//                      corner arrays; a workgroup tests the 16 x 16 corners of a tile of 15 x 15 cells once each, keeps the
//                      results in LDS, and every cell ANDs its four.  Polygon edges are staged through LDS in chunks of 256;
//                      an edge whose longitude range misses the tile's columns cannot flip any of its corners and is dropped.
//   k_scanline_pack    one record per kept cell (global row, global column, the planes, the image), structure of arrays.
//   k_scanline_*       the union raster: the strip with the largest frame index wins a cell (an integer max per cell first,
//   (compose)          then every record writes where its strip is the winner: no order of launches or lanes shows).
#include "amt_common.h"
#include "amt_polygon.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace {

using namespace amt;

constexpr int kSide = 16;             // corners per tile side: kSide * kSide == kBlock, one corner per thread
constexpr int kTile = kSide - 1;       // cells per tile side
constexpr long long kNoMin = 0x7fffffffffffffffLL, kNoMax = -kNoMin - 1;

inline unsigned blocks_for(int64_t n) {
    int64_t blocks = (n + kBlock - 1) / kBlock;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    return static_cast<unsigned>(blocks);
}

// number of set bits of `ballot` below this lane
__device__ __forceinline__ unsigned lanes_below(unsigned long long ballot) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

__global__ void k_scanline_stats_init(long long* stats) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        stats[0] = 0;
        stats[1] = kNoMin, stats[2] = kNoMax, stats[3] = kNoMin, stats[4] = kNoMax;
    }
}

struct select_args {
    const double* lat_axis;     // [ny + 1] latitudes of the corner rows
    const double* lon_axis;     // [nx + 1] longitudes of the corner columns
    const double* poly;         // [m][2] (lat, lon)
    const uint8_t* mask;        // [ny][nx], non-zero: the cell is masked
    uint8_t* keep;              // [rows][cols]
    long long* stats;           // count, min row, max row, min col, max col (rows and columns of the frame)
    int m, nx, row0, col0, rows, cols;
};

// grid: (ceil(cols / kTile), ceil(rows / kTile)); thread (r, c) = (threadIdx.x / 16, threadIdx.x % 16) owns corner
// (blockIdx.y * kTile + r, blockIdx.x * kTile + c) of the window and, for r, c < kTile, the cell of that index.
__global__ __launch_bounds__(kBlock) void k_scanline_select(select_args A) {
    __shared__ double sx0[kBlock], sy0[kBlock], sx1[kBlock], sy1[kBlock];
    __shared__ double sLon[kSide];
    __shared__ int sCount;
    __shared__ uint8_t sIn[kSide][kSide + 1];
    const int r = threadIdx.x / kSide, c = threadIdx.x % kSide;
    const int wr = blockIdx.y * kTile + r, wc = blockIdx.x * kTile + c;
    const bool live = wr <= A.rows && wc <= A.cols;                 // (a window of rows x cols cells has one more of each)
    // as maskedByPolygon calls the test: x is the latitude, y the longitude
    const double tx = live ? A.lat_axis[A.row0 + wr] : 0.0, ty = live ? A.lon_axis[A.col0 + wc] : 0.0;
    if (r == 0) sLon[c] = live ? ty : NAN;                          // (row 0 of a tile is always inside the window)
    __syncthreads();
    // longitude range of the tile's corners (a NaN never compares: it takes no part, as in k_points_in_polygon)
    double lo = __builtin_huge_val(), hi = -__builtin_huge_val();
    for (int j = 0; j < kSide; ++j) {
        const double v = sLon[j];
        if (v == v) {
            lo = fmin(lo, v);
            hi = fmax(hi, v);
        }
    }
    bool in = false;
    for (int base = 0; base < A.m; base += kBlock) {
        __syncthreads();
        if (threadIdx.x == 0) sCount = 0;
        __syncthreads();
        const int k = base + (int)threadIdx.x;
        if (k < A.m) {
            const int k1 = k + 1 == A.m ? 0 : k + 1;
            const double x0 = A.poly[2 * (int64_t)k], y0 = A.poly[2 * (int64_t)k + 1];
            const double x1 = A.poly[2 * (int64_t)k1], y1 = A.poly[2 * (int64_t)k1 + 1];
            if (polygon_edge_meets(y0, y1, lo, hi)) {
                const int slot = atomicAdd(&sCount, 1);             // (< kBlock: at most one edge per thread and chunk)
                sx0[slot] = x0;
                sy0[slot] = y0;
                sx1[slot] = x1;
                sy1[slot] = y1;
            }
        }
        __syncthreads();
        const int cnt = sCount;
        // (the order of the staged edges varies from run to run; flips commute)
        for (int e = 0; e < cnt; ++e)
            if (polygon_edge_flips(sx0[e], sy0[e], sx1[e], sy1[e], tx, ty)) in = !in;
    }
    sIn[r][c] = (live && in && isfinite(tx) && isfinite(ty)) ? 1 : 0;
    __syncthreads();
    const bool cell = r < kTile && c < kTile && wr < A.rows && wc < A.cols;
    bool kept = false;
    const int fr = A.row0 + wr, fc = A.col0 + wc;
    if (cell) {
        kept = sIn[r][c] && sIn[r + 1][c] && sIn[r][c + 1] && sIn[r + 1][c + 1] && A.mask[(int64_t)fr * A.nx + fc] == 0;
        A.keep[(int64_t)wr * A.cols + wc] = kept ? 1 : 0;
    }
    // count and extents: reduced over the wave, then one integer atomic each from the waves that kept anything
    const unsigned long long ballot = __ballot(kept);
    if (ballot == 0) return;                                        // (wave-uniform; no barrier follows)
    int rmin = kept ? fr : 0x7fffffff, rmax = kept ? fr : -1, cmin = kept ? fc : 0x7fffffff, cmax = kept ? fc : -1;
    for (int o = 32; o > 0; o >>= 1) {
        rmin = min(rmin, __shfl_xor(rmin, o));
        rmax = max(rmax, __shfl_xor(rmax, o));
        cmin = min(cmin, __shfl_xor(cmin, o));
        cmax = max(cmax, __shfl_xor(cmax, o));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(reinterpret_cast<unsigned long long*>(A.stats), (unsigned long long)__popcll(ballot));
        atomicMin(A.stats + 1, (long long)rmin);
        atomicMax(A.stats + 2, (long long)rmax);
        atomicMin(A.stats + 3, (long long)cmin);
        atomicMax(A.stats + 4, (long long)cmax);
    }
}

struct pack_args {
    const uint8_t* keep;        // [rows][cols]
    const double* planes;       // [ny][nx][nplane]
    const void* img;            // [ny][nx][nchan]
    int nx, row0, col0, rows, cols, nplane, nchan, row_offset, col_offset;
    unsigned int count;
    unsigned int* cursor;       // zeroed; ends at the number of keep bytes set
    int32_t* out_row;           // [count]
    int32_t* out_col;           // [count]
    double* out_planes;         // [nplane][count]
    void* out_img;              // [nchan][count]
};

// Every kept cell takes the next free record: one atomic per wave (the ballot's population), the lanes' places from the bits
// below them.  A place beyond `count` is not written (the host compares the cursor with `count` afterwards).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_scanline_pack(pack_args A) {
    const int64_t n = (int64_t)A.rows * A.cols;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = blockIdx.x * (int64_t)blockDim.x; base < n; base += stride) {     // (uniform over the workgroup)
        const int64_t i = base + threadIdx.x;
        const bool kept = i < n && A.keep[i] != 0;
        const unsigned long long ballot = __ballot(kept);
        if (ballot == 0) continue;
        unsigned int first = 0;
        if ((threadIdx.x & 63) == 0) first = atomicAdd(A.cursor, (unsigned int)__popcll(ballot));
        first = __shfl(first, 0);
        const unsigned int at = first + lanes_below(ballot);
        if (!kept || at >= A.count) continue;
        const int fr = A.row0 + (int)(i / A.cols), fc = A.col0 + (int)(i % A.cols);
        const int64_t cell = (int64_t)fr * A.nx + fc;
        A.out_row[at] = A.row_offset + fr;
        A.out_col[at] = A.col_offset + fc;
        for (int p = 0; p < A.nplane; ++p) A.out_planes[(int64_t)p * A.count + at] = A.planes[cell * A.nplane + p];
        for (int ch = 0; ch < A.nchan; ++ch)
            static_cast<T*>(A.out_img)[(int64_t)ch * A.count + at] = static_cast<const T*>(A.img)[cell * A.nchan + ch];
    }
}

struct strip_dev {
    const int32_t* row;
    const int32_t* col;
    const double* planes;
    const void* img;
    long long count;
    int k, pad_;
};

struct compose_args {
    const strip_dev* strips;
    int row_base, col_base, NY, NX, nplane, nchan;
    double* planes;             // [NY][NX][nplane]
    void* img;                  // [NY][NX][nchan]
    uint8_t* mask;              // [NY][NX]
    int32_t* frame_index;       // [NY][NX]
    unsigned int* outside;      // set when a record lies outside the raster
};

template <typename T>
__global__ __launch_bounds__(kBlock) void k_scanline_clear(compose_args A) {
    const int64_t n = (int64_t)A.NY * A.NX;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        A.frame_index[i] = -1;
        A.mask[i] = 1;
        for (int p = 0; p < A.nplane; ++p) A.planes[i * A.nplane + p] = NAN;
        for (int ch = 0; ch < A.nchan; ++ch) static_cast<T*>(A.img)[i * A.nchan + ch] = 0;
    }
}

// the raster cell of record j of strip S, -1 when it lies outside
__device__ __forceinline__ int64_t compose_cell(const compose_args& A, const strip_dev& S, int64_t j) {
    const int64_t y = (int64_t)S.row[j] - A.row_base, x = (int64_t)S.col[j] - A.col_base;
    return (y < 0 || y >= A.NY || x < 0 || x >= A.NX) ? -1 : y * A.NX + x;
}

// grid: (workgroups over a strip's records, strips).  Pass 1: the largest frame index per cell.
__global__ __launch_bounds__(kBlock) void k_scanline_claim(compose_args A) {
    const strip_dev S = A.strips[blockIdx.y];
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < S.count; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t cell = compose_cell(A, S, j);
        if (cell < 0)
            atomicOr(A.outside, 1u);
        else
            atomicMax(A.frame_index + cell, S.k);
    }
}

// Pass 2: a record writes its cell where its strip holds it (the records of a strip are unique and the frame indices of the
// strips differ: one writer per cell).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_scanline_write(compose_args A) {
    const strip_dev S = A.strips[blockIdx.y];
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < S.count; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t cell = compose_cell(A, S, j);
        if (cell < 0 || A.frame_index[cell] != S.k) continue;
        A.mask[cell] = 0;
        for (int p = 0; p < A.nplane; ++p) A.planes[cell * A.nplane + p] = S.planes[(int64_t)p * S.count + j];
        for (int ch = 0; ch < A.nchan; ++ch)
            static_cast<T*>(A.img)[cell * A.nchan + ch] = static_cast<const T*>(S.img)[(int64_t)ch * S.count + j];
    }
}

}  // namespace

extern "C" {

int amt_scanline_select(amt_ctx* ctx, const double* lat_axis, const double* lon_axis, int32_t ny, int32_t nx,
                        const double* polygon, int32_t n_vertices, const uint8_t* cell_mask, int32_t row0, int32_t col0,
                        int32_t rows, int32_t cols, uint8_t* out_keep, int64_t* out_stats) {
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, lat_axis && lon_axis && cell_mask && out_stats, "NULL argument");
    AMT_REQUIRE(ctx, n_vertices >= 0 && (n_vertices == 0 || polygon), "bad size or NULL polygon");
    AMT_REQUIRE(ctx, ny > 0 && nx > 0, "empty grid");
    AMT_REQUIRE(ctx, row0 >= 0 && col0 >= 0 && rows >= 0 && cols >= 0 && (int64_t)row0 + rows <= ny && (int64_t)col0 + cols <= nx,
                "the window does not lie in the grid");
    const int64_t cells = (int64_t)rows * cols;
    AMT_REQUIRE(ctx, cells == 0 || out_keep, "NULL argument");
    AMT_REQUIRE(ctx, (rows + kTile - 1) / kTile <= 65535, "window too tall");
    if (amt_set_device(ctx)) return AMT_EHIP;
    long long* stats = reinterpret_cast<long long*>(out_stats);
    hipLaunchKernelGGL(k_scanline_stats_init, dim3(1), dim3(64), 0, ctx->stream, stats);
    AMT_LAUNCH_CHECK(ctx);
    if (cells == 0) return AMT_OK;
    if (n_vertices < 3) {                               // no area: nothing is inside
        AMT_HIP(ctx, hipMemsetAsync(out_keep, 0, (size_t)cells, ctx->stream));
        return AMT_OK;
    }
    select_args A;
    A.lat_axis = lat_axis, A.lon_axis = lon_axis, A.poly = polygon, A.mask = cell_mask, A.keep = out_keep, A.stats = stats;
    A.m = n_vertices, A.nx = nx, A.row0 = row0, A.col0 = col0, A.rows = rows, A.cols = cols;
    const dim3 grid((unsigned)((cols + kTile - 1) / kTile), (unsigned)((rows + kTile - 1) / kTile));
    hipLaunchKernelGGL(k_scanline_select, grid, dim3(kBlock), 0, ctx->stream, A);
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

int amt_scanline_pack(amt_ctx* ctx, const uint8_t* keep, int32_t row0, int32_t col0, int32_t rows, int32_t cols,
                      const double* planes, int32_t nplane, const void* img, int32_t img_dtype, int32_t nchan, int32_t ny,
                      int32_t nx, int32_t row_offset, int32_t col_offset, int64_t count, int32_t* out_row, int32_t* out_col,
                      double* out_planes, void* out_img) {
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, ny > 0 && nx > 0, "empty grid");
    AMT_REQUIRE(ctx, row0 >= 0 && col0 >= 0 && rows >= 0 && cols >= 0 && (int64_t)row0 + rows <= ny && (int64_t)col0 + cols <= nx,
                "the window does not lie in the grid");
    const int64_t cells = (int64_t)rows * cols;
    AMT_REQUIRE(ctx, count >= 0 && count <= cells && count < 2147483647LL, "count outside the window's size");
    AMT_REQUIRE(ctx, nchan >= 0 && nchan <= 4, "nchan must be 0..4");
    AMT_REQUIRE(ctx, nplane >= 0 && nplane <= 5, "nplane must be 0..5");
    AMT_REQUIRE(ctx, nchan == 0 || img_dtype == 1 || img_dtype == 2, "img must be uint8 (1) or uint16 (2)");
    AMT_REQUIRE(ctx, cells == 0 || keep, "NULL argument");
    AMT_REQUIRE(ctx, (nplane == 0 || planes) && (nchan == 0 || img), "NULL argument");
    AMT_REQUIRE(ctx, count == 0 || (out_row && out_col && (nplane == 0 || out_planes) && (nchan == 0 || out_img)), "NULL argument");
    if (amt_set_device(ctx)) return AMT_EHIP;
    if (cells == 0) return AMT_OK;
    unsigned int* cursor = static_cast<unsigned int*>(amt_workspace(ctx, 256));
    if (cursor == nullptr) {
        ctx->last_error = "amt_scanline_pack: no device memory for the workspace";
        return AMT_ENOMEM;
    }
    AMT_HIP(ctx, hipMemsetAsync(cursor, 0, sizeof(unsigned int), ctx->stream));
    pack_args A;
    A.keep = keep, A.planes = planes, A.img = img;
    A.nx = nx, A.row0 = row0, A.col0 = col0, A.rows = rows, A.cols = cols, A.nplane = nplane, A.nchan = nchan;
    A.row_offset = row_offset, A.col_offset = col_offset, A.count = (unsigned int)count, A.cursor = cursor;
    A.out_row = out_row, A.out_col = out_col, A.out_planes = out_planes, A.out_img = out_img;
    if (nchan && img_dtype == 2)
        hipLaunchKernelGGL(k_scanline_pack<uint16_t>, dim3(blocks_for(cells)), dim3(kBlock), 0, ctx->stream, A);
    else
        hipLaunchKernelGGL(k_scanline_pack<uint8_t>, dim3(blocks_for(cells)), dim3(kBlock), 0, ctx->stream, A);
    AMT_LAUNCH_CHECK(ctx);
    unsigned int found = 0;
    AMT_HIP(ctx, hipMemcpyAsync(&found, cursor, sizeof(found), hipMemcpyDeviceToHost, ctx->stream));
    AMT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    AMT_REQUIRE(ctx, (int64_t)found == count, "count differs from the number of keep bytes set (records beyond it were not written)");
    return AMT_OK;
}

int amt_scanline_compose(amt_ctx* ctx, const amt_scanline_strip* strips, int32_t n_strips, int32_t img_dtype, int32_t nchan,
                         int32_t nplane, int32_t row_base, int32_t col_base, int32_t NY, int32_t NX, double* planes, void* img,
                         uint8_t* mask, int32_t* frame_index) {
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, n_strips >= 0 && n_strips <= 65535 && (n_strips == 0 || strips), "bad strip table");
    AMT_REQUIRE(ctx, NY > 0 && NX > 0, "empty raster");
    AMT_REQUIRE(ctx, nchan >= 0 && nchan <= 4, "nchan must be 0..4");
    AMT_REQUIRE(ctx, nplane >= 0 && nplane <= 5, "nplane must be 0..5");
    AMT_REQUIRE(ctx, nchan == 0 || img_dtype == 1 || img_dtype == 2, "img must be uint8 (1) or uint16 (2)");
    AMT_REQUIRE(ctx, mask && frame_index && (nplane == 0 || planes) && (nchan == 0 || img), "NULL argument");
    int64_t longest = 0;
    for (int32_t i = 0; i < n_strips; ++i) {
        const amt_scanline_strip& s = strips[i];
        AMT_REQUIRE(ctx, s.count >= 0 && s.count < 2147483647LL, "bad record count");
        AMT_REQUIRE(ctx, s.frame >= 0 && (i == 0 || s.frame > strips[i - 1].frame), "frame indices must be >= 0 and ascend");
        AMT_REQUIRE(ctx, s.count == 0 || (s.row && s.col && (nplane == 0 || s.planes) && (nchan == 0 || s.img)), "strip without records");
        if (s.count > longest) longest = s.count;
    }
    if (amt_set_device(ctx)) return AMT_EHIP;
    const size_t table_bytes = ((size_t)n_strips * sizeof(strip_dev) + 255) & ~(size_t)255;
    char* ws = static_cast<char*>(amt_workspace(ctx, table_bytes + 256));
    if (ws == nullptr) {
        ctx->last_error = "amt_scanline_compose: no device memory for the workspace";
        return AMT_ENOMEM;
    }
    unsigned int* outside = reinterpret_cast<unsigned int*>(ws + table_bytes);
    std::vector<strip_dev> host((size_t)n_strips);
    for (int32_t i = 0; i < n_strips; ++i) {
        const amt_scanline_strip& s = strips[i];
        host[(size_t)i] = strip_dev{s.row, s.col, s.planes, s.img, (long long)s.count, s.frame, 0};
    }
    // (pageable source: the copy has consumed the staging buffer when the call returns)
    if (n_strips)
        AMT_HIP(ctx, hipMemcpyAsync(ws, host.data(), host.size() * sizeof(strip_dev), hipMemcpyHostToDevice, ctx->stream));
    AMT_HIP(ctx, hipMemsetAsync(outside, 0, sizeof(unsigned int), ctx->stream));
    compose_args A;
    A.strips = reinterpret_cast<const strip_dev*>(ws);
    A.row_base = row_base, A.col_base = col_base, A.NY = NY, A.NX = NX, A.nplane = nplane, A.nchan = nchan;
    A.planes = planes, A.img = img, A.mask = mask, A.frame_index = frame_index, A.outside = outside;
    const bool wide = nchan && img_dtype == 2;
    const dim3 all(blocks_for((int64_t)NY * NX));
    if (wide)
        hipLaunchKernelGGL(k_scanline_clear<uint16_t>, all, dim3(kBlock), 0, ctx->stream, A);
    else
        hipLaunchKernelGGL(k_scanline_clear<uint8_t>, all, dim3(kBlock), 0, ctx->stream, A);
    if (n_strips && longest) {
        const dim3 grid(blocks_for(longest), (unsigned)n_strips);
        hipLaunchKernelGGL(k_scanline_claim, grid, dim3(kBlock), 0, ctx->stream, A);
        if (wide)
            hipLaunchKernelGGL(k_scanline_write<uint16_t>, grid, dim3(kBlock), 0, ctx->stream, A);
        else
            hipLaunchKernelGGL(k_scanline_write<uint8_t>, grid, dim3(kBlock), 0, ctx->stream, A);
    }
    AMT_LAUNCH_CHECK(ctx);
    unsigned int flag = 0;
    AMT_HIP(ctx, hipMemcpyAsync(&flag, outside, sizeof(flag), hipMemcpyDeviceToHost, ctx->stream));
    AMT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (flag) {
        ctx->last_error = "amt_scanline_compose: a record lies outside the raster (the cells inside it are composed)";
        return AMT_EDOMAIN;
    }
    return AMT_OK;
}

}  // extern "C"
