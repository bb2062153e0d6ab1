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
#include <cmath>
#include <string>
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
};

// the nearest pixel of a seen point (half to even), kept inside the frame: x in [-0.5, n - 0.5] rounds to -0 or n at the ends
__device__ __forceinline__ int nearest_index(double v, int n) { return (int)fmin(fmax(rint(v), 0.0), (double)(n - 1)); }

// N: taps per axis (2 linear, 8 Lanczos-4); 0: the nearest pixel, which needs no window
template <typename T, int N>
__global__ __launch_bounds__(256) void k_gather_mosaic(gather_args A) {
    extern __shared__ __align__(16) unsigned char gather_smem[];
    T* win = reinterpret_cast<T*>(gather_smem);
    __shared__ int fold[4][6];
    constexpr int lo = N == 8 ? -3 : 0, hi = lo + (N ? N : 1) - 1;

    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int X = blockIdx.x * kTile + tx;
    const bool points = A.cell_lat != nullptr;
    const int C = A.C;

    bool in_grid[kRowsPerThread];
    double latv[kRowsPerThread];
    lon_terms Lk[kRowsPerThread];
    lat_terms Tk[kRowsPerThread];
    // a thread's cells share their column: its longitude terms are computed once (the point form has a longitude per cell)
    const lon_terms L0 = w2p_lon_terms(!points && X < A.nx ? A.lon[X] : 0.0);
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        const int Y = blockIdx.y * kTile + ty + 8 * k;
        in_grid[k] = X < A.nx && Y < A.ny;
        const int64_t i = (int64_t)Y * A.nx + X;
        latv[k] = !in_grid[k] ? 0.0 : (points ? A.cell_lat[i] : A.lat[Y]);
        Lk[k] = points ? w2p_lon_terms(in_grid[k] ? A.cell_lon[i] : 0.0) : L0;
        // the latitude terms depend on the member through the WGS84 constants alone: one evaluation where all members agree
        if (A.same_ellipsoid) Tk[k] = w2p_lat_terms(A.members[0].K, latv[k]);
    }

    // ---- election: the running best per cell -------------------------------------------------------------------------
    int bm[kRowsPerThread];
    double bx[kRowsPerThread], by[kRowsPerThread], be[kRowsPerThread];
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) bm[k] = -1, bx[k] = by[k] = be[k] = NAN;
    for (int m = 0; m < A.n; ++m) {
        const gather_dev& M = A.members[m];
        const int w = M.K.width, h = M.K.height;
        const double least = M.min_elevation;
#pragma unroll
        for (int k = 0; k < kRowsPerThread; ++k) {
            if (!in_grid[k]) continue;
            if (A.rule == 0 && bm[k] >= 0) continue;        // the first member that sees the cell keeps it
            const lat_terms Tm = A.same_ellipsoid ? Tk[k] : w2p_lat_terms(M.K, latv[k]);
            double x, y, e;
            bool seen = w2p_point(M.K, M.S, Tm, Lk[k], x, y, e) == 0;
            if (N != 0) {
                // support, as k_remap evaluates it on the float32 coordinates it is given
                const double xs = (double)(float)x, ys = (double)(float)y;
                seen = seen && xs >= 0.0 && xs <= (double)(w - 1) && ys >= 0.0 && ys <= (double)(h - 1);
            }
            if (seen && M.center_mask) seen = M.center_mask[(int64_t)nearest_index(y, h) * w + nearest_index(x, w)] == 0;
            if (least == least) seen = seen && e >= least;
            seen = seen && e == e;                          // a NaN elevation never wins
            if (seen && (bm[k] < 0 || e > be[k])) bm[k] = m, bx[k] = x, by[k] = y, be[k] = e;       // (ties: the lower index)
        }
    }

    // ---- what the tile holds: the range of its winners and the box of their taps, as (min, -max) so that one fold serves all ----
    int ix[kRowsPerThread], iy[kRowsPerThread];
    double fx[kRowsPerThread], fy[kRowsPerThread];
    int r0 = INT32_MAX, r1 = INT32_MAX, b0 = INT32_MAX, b1 = INT32_MAX, b2 = INT32_MAX, b3 = INT32_MAX;
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        ix[k] = iy[k] = 0, fx[k] = fy[k] = 0.0;
        if (bm[k] < 0) continue;
        r0 = min(r0, bm[k]), r1 = min(r1, -bm[k]);
        if (N == 0) {
            const w2p_consts& K = A.members[bm[k]].K;
            ix[k] = nearest_index(bx[k], K.width), iy[k] = nearest_index(by[k], K.height);
        } else {
            // (a seen cell has support: k_remap's clamp of far-away coordinates would change nothing)
            const double xs = (double)(float)bx[k], ys = (double)(float)by[k];
            const double flx = floor(xs), fly = floor(ys);
            ix[k] = (int)flx, iy[k] = (int)fly;
            fx[k] = xs - flx, fy[k] = ys - fly;
        }
        b0 = min(b0, ix[k] + lo), b1 = min(b1, -(ix[k] + hi));
        b2 = min(b2, iy[k] + lo), b3 = min(b3, -(iy[k] + hi));
    }
    r0 = wave_min(r0), r1 = wave_min(r1), b0 = wave_min(b0), b1 = wave_min(b1), b2 = wave_min(b2), b3 = wave_min(b3);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) fold[wave][0] = r0, fold[wave][1] = r1, fold[wave][2] = b0, fold[wave][3] = b1, fold[wave][4] = b2, fold[wave][5] = b3;
    __syncthreads();
    auto folded = [&](int j) { return min(min(fold[0][j], fold[1][j]), min(fold[2][j], fold[3][j])); };
    const int m_lo = folded(0), m_hi = -folded(1);
    const int x_lo = folded(2), x_hi = -folded(3), y_lo = folded(4), y_hi = -folded(5);
    const bool any = m_lo != INT32_MAX;
    const int nwx = any ? x_hi - x_lo + 1 : 0, nwy = any ? y_hi - y_lo + 1 : 0;
    // the same for the whole block
    const bool staged = N != 0 && any && m_lo == m_hi && nwx <= kWin && nwy <= kWin && A.force != AMT_GATHER_PATH_CELL;
    if (A.tile_path && threadIdx.x == 0)
        A.tile_path[blockIdx.y * gridDim.x + blockIdx.x] = !any ? 0 : (staged ? AMT_GATHER_PATH_STAGED : AMT_GATHER_PATH_CELL);

    const int pitch = nwx * C;
    if (staged) {
        const gather_dev& M = A.members[__builtin_amdgcn_readfirstlane(m_lo)];
        const T* src = static_cast<const T*>(M.img);
        const int sw = M.K.width, sh = M.K.height;
        // a wave per window row, lanes along the row's samples: consecutive lanes read consecutive samples of the source row
        for (int r = wave; r < nwy; r += 4) {
            const int gy = y_lo + r;
            const bool row_in = gy >= 0 && gy < sh;
            const T* srow = src + ((int64_t)(row_in ? gy : 0) * sw) * C;
            for (int e = lane; e < pitch; e += 64) {
                const int gx = x_lo + e / C;
                const bool in = row_in && gx >= 0 && gx < sw;
                win[r * pitch + e] = in ? srow[(int64_t)x_lo * C + e] : (T)0;
            }
        }
        __syncthreads();
    }

#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        const int Y = blockIdx.y * kTile + ty + 8 * k;
        if (!in_grid[k]) continue;
        const int64_t i = (int64_t)Y * A.nx + X;
        T* out = static_cast<T*>(A.img) + i * C;
        const bool won = bm[k] >= 0;
        A.mask[i] = won ? 0 : 1;
        A.source[i] = bm[k];
        A.elev[i] = be[k];
        if (A.xy) A.xy[2 * i + 0] = bx[k], A.xy[2 * i + 1] = by[k];
        if (!won) {
            for (int c = 0; c < C; ++c) out[c] = (T)0;
            continue;
        }
        const gather_dev& M = A.members[bm[k]];
        const T* src = static_cast<const T*>(M.img);
        const int sw = M.K.width, sh = M.K.height;
        if (N == 0) {
            const T* px = src + ((int64_t)iy[k] * sw + ix[k]) * C;
            for (int c = 0; c < C; ++c) out[c] = px[c];
        } else {
            constexpr int NT = N ? N : 2;
            double wx[NT], wy[NT];
            tap_weights<NT>(fx[k], wx);
            tap_weights<NT>(fy[k], wy);
            if (staged) {
                const window_fetch<T> f = {win, x_lo, y_lo, pitch, C};
                for (int c = 0; c < C; ++c) out[c] = to_sample<T>(sample<NT>(f, ix[k] + lo, iy[k] + lo, c, wx, wy));
            } else {
                const global_fetch<T> f = {src, sw, sh, C};
                for (int c = 0; c < C; ++c) out[c] = to_sample<T>(sample<NT>(f, ix[k] + lo, iy[k] + lo, c, wx, wy));
            }
        }
    }
}

template <typename T>
void launch_gather(amt_ctx* ctx, const gather_args& A, int interpolation) {
    const dim3 grid((unsigned)((A.nx + kTile - 1) / kTile), (unsigned)((A.ny + kTile - 1) / kTile));
    const size_t lds = (size_t)kWin * kWin * (size_t)A.C * sizeof(T);
    if (interpolation == AMT_INTERP_LINEAR)
        hipLaunchKernelGGL((k_gather_mosaic<T, 2>), grid, dim3(256), lds, ctx->stream, A);
    else if (interpolation == AMT_INTERP_LANCZOS4)
        hipLaunchKernelGGL((k_gather_mosaic<T, 8>), grid, dim3(256), lds, ctx->stream, A);
    else
        hipLaunchKernelGGL((k_gather_mosaic<T, 0>), grid, dim3(256), 0, ctx->stream, A);
}

}  // namespace

extern "C" int amt_gather_mosaic(amt_ctx* ctx, const amt_gather_member* members, int32_t n_members, int32_t frame,
                                 const double* lat_centres, int32_t ny, const double* lon_centres, int32_t nx,
                                 const double* cell_lat, const double* cell_lon, int32_t sample_bytes, int32_t channels,
                                 int32_t interpolation, int32_t rule, void* out_img, uint8_t* out_mask, double* out_elev,
                                 int32_t* out_source, double* out_xy, const amt_gather_debug* debug) {
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, members && out_img && out_mask && out_elev && out_source, "NULL argument");
    AMT_REQUIRE(ctx, n_members >= 1, "no members");
    AMT_REQUIRE(ctx, ny > 0 && nx > 0, "empty axis");
    const bool axes = lat_centres && lon_centres, cells = cell_lat && cell_lon;
    AMT_REQUIRE(ctx, (lat_centres != nullptr) == (lon_centres != nullptr) && (cell_lat != nullptr) == (cell_lon != nullptr) && axes != cells,
                "give either the two axes or the two cell arrays");
    AMT_REQUIRE(ctx, frame == AMT_W2P_GEODETIC || frame == AMT_W2P_SM, "unknown frame (AMT_W2P_GEODETIC or AMT_W2P_SM)");
    AMT_REQUIRE(ctx, interpolation == AMT_INTERP_LINEAR || interpolation == AMT_INTERP_LANCZOS4 || interpolation == AMT_INTERP_NEAREST,
                "unknown interpolation");
    AMT_REQUIRE(ctx, rule == 0 || rule == 1, "unknown rule");
    AMT_REQUIRE(ctx, sample_bytes == 1 || sample_bytes == 2 || sample_bytes == 4, "sample_bytes must be 1 (uint8), 2 (uint16) or 4 (float32)");
    AMT_REQUIRE(ctx, channels == 1 || channels == 3 || channels == 4, "channels must be 1, 3 or 4");
    AMT_REQUIRE(ctx, !debug || (debug->force_path >= AMT_GATHER_PATH_AUTO && debug->force_path <= AMT_GATHER_PATH_CELL), "unknown force_path");

    std::vector<gather_dev> dev((size_t)n_members);
    bool same = true;
    for (int32_t i = 0; i < n_members; ++i) {
        const amt_gather_member& m = members[i];
        gather_dev& d = dev[(size_t)i];
        const char* err = m.img ? w2p_prepare(&m.params, m.zenithal, frame, &d.K, &d.S) : "member without image";
        AMT_REQUIRE(ctx, err == nullptr, "member " + std::to_string(i) + ": " + err);
        d.img = m.img;
        d.center_mask = m.center_mask;
        d.min_elevation = m.min_elevation > -INFINITY ? m.min_elevation : (double)NAN;      // (-inf and NaN: none)
        same = same && d.K.a0 == dev[0].K.a0 && d.K.e2 == dev[0].K.e2;
    }
    if (amt_set_device(ctx)) return AMT_EHIP;
    const size_t bytes = dev.size() * sizeof(gather_dev);
    char* ws = static_cast<char*>(amt_workspace(ctx, bytes));
    if (ws == nullptr) {
        ctx->last_error = "amt_gather_mosaic: workspace allocation failed";
        return AMT_ENOMEM;
    }
    // (pageable source: the copy has consumed the staging buffer when the call returns)
    AMT_HIP(ctx, hipMemcpyAsync(ws, dev.data(), bytes, hipMemcpyHostToDevice, ctx->stream));

    gather_args A;
    A.members = reinterpret_cast<const gather_dev*>(ws);
    A.lat = axes ? lat_centres : nullptr, A.lon = axes ? lon_centres : nullptr;
    A.cell_lat = axes ? nullptr : cell_lat, A.cell_lon = axes ? nullptr : cell_lon;
    A.n = n_members, A.ny = ny, A.nx = nx, A.C = channels;
    A.rule = rule, A.same_ellipsoid = same ? 1 : 0, A.force = debug ? debug->force_path : AMT_GATHER_PATH_AUTO, A.pad_ = 0;
    A.img = out_img, A.mask = out_mask, A.elev = out_elev, A.source = out_source, A.xy = out_xy;
    A.tile_path = debug ? debug->tile_path : nullptr;
    switch (sample_bytes) {
        case 1: launch_gather<uint8_t>(ctx, A, interpolation); break;
        case 2: launch_gather<uint16_t>(ctx, A, interpolation); break;
        default: launch_gather<float>(ctx, A, interpolation); break;
    }
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}
