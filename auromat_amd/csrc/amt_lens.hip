// Lens distortion (include/auromat_hip.h: amt_lens_coords, amt_lens_undistort, amt_lens_remap, amt_remap_coords): the step the
// reference takes through lensfunpy and cv2 before an image matches its .wcs (auromat/mapping/iss.py:232-243,
// util/lensdistortion.py).  The radial models and their radius convention are those the reference documents in draw.py:1104-1148;
// lensfun itself is not here to compare against, so what these kernels compute is pinned by the NumPy / mpmath statement in
// tests/_lens_oracle.py, not by lensfun's output.
//
// The remap is one fused kernel: a block of 256 threads makes a 32 x 32 tile of the corrected image, every thread four pixels a
// quarter tile apart.  Source coordinates are evaluated in float64 in registers and never stored.  A lens displacement is smooth, so
// the taps of a tile lie in the tile's own rectangle moved and stretched a little: the block folds the tap range of its pixels into
// one box, copies that box of the source (zeros outside the image: the constant border) into LDS with coalesced row reads, and every
// pixel takes its 2 x 2 or 8 x 8 taps per channel from there.  A tile whose box does not fit the window (strong magnification,
// extreme coefficients, an arbitrary coordinate array) takes its taps from global memory with a bounds test each.  Both ways go
// through the same sampling function with the same operands in the same order, so they give the same bits.
#include "amt_common.h"
#include "amt_lens.h"       // the models' constants and per-coordinate functions: shared with amt_w2p.h
#include "amt_remap.h"      // the tiling, tap_weights, the two fetches and sample: shared with amt_gather.hip

namespace {

using namespace amt;

template <bool INVERSE>
__global__ __launch_bounds__(256) void k_lens_coords(lens_dev m, double x0, double y0, int cols, double* __restrict__ out,
                                                      float* __restrict__ out32) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= cols) return;
    const double px = x0 + i, py = y0 + (double)blockIdx.y;
    double ax, ay;
    if (INVERSE) {
        lens_inverse(m, px, py, ax, ay);
        ax -= m.crop_x, ay -= m.crop_y;
    } else {
        lens_forward(m, px + m.crop_x, py + m.crop_y, ax, ay);
    }
    const int64_t o = 2 * ((int64_t)blockIdx.y * cols + i);
    out[o] = ax, out[o + 1] = ay;
    if (out32) out32[o] = (float)ax, out32[o + 1] = (float)ay;
}

struct model_coord {
    lens_dev m;
    __device__ __forceinline__ void operator()(int X, int Y, double& xs, double& ys) const {
        lens_forward(m, (double)(X + m.crop_x), (double)(Y + m.crop_y), xs, ys);
    }
};

struct array_coord {
    const float* xy;
    int dw;
    __device__ __forceinline__ void operator()(int X, int Y, double& xs, double& ys) const {
        const int64_t o = 2 * ((int64_t)Y * dw + X);
        xs = (double)xy[o], ys = (double)xy[o + 1];
    }
};

template <typename T, int N, typename Coord>
__global__ __launch_bounds__(256) void k_remap(Coord coord, const T* __restrict__ src, int sw, int sh, int C, T* __restrict__ dst, int dw,
                                                int dh, uint8_t* __restrict__ support, int force, uint8_t* __restrict__ tile_path) {
    extern __shared__ __align__(16) unsigned char lens_smem[];
    T* win = reinterpret_cast<T*>(lens_smem);
    __shared__ int fold[4][4];
    constexpr int lo = N == 8 ? -3 : 0, hi = lo + N - 1;

    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int X = blockIdx.x * kTile + tx;
    int ix[kRowsPerThread], iy[kRowsPerThread];
    double fx[kRowsPerThread], fy[kRowsPerThread];
    bool live[kRowsPerThread];
    // box of the taps of this block's pixels, as (min x, -max x, min y, -max y) so that one fold serves all four
    int b0 = INT32_MAX, b1 = INT32_MAX, b2 = INT32_MAX, b3 = INT32_MAX;
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        const int Y = blockIdx.y * kTile + ty + 8 * k;
        const bool in_dst = X < dw && Y < dh;
        double xs = NAN, ys = NAN;
        if (in_dst) coord(X, Y, xs, ys);
        const bool finite = in_dst && fabs(xs) <= 1.7976931348623157e308 && fabs(ys) <= 1.7976931348623157e308;
        if (in_dst && support) support[(int64_t)Y * dw + X] = finite && xs >= 0.0 && xs <= (double)(sw - 1) && ys >= 0.0 && ys <= (double)(sh - 1);
        // far outside: no tap in the image wherever exactly, so the clamp changes nothing
        const double xc = finite ? fmin(fmax(xs, -16.0), (double)sw + 16.0) : -16.0;
        const double yc = finite ? fmin(fmax(ys, -16.0), (double)sh + 16.0) : -16.0;
        const double flx = floor(xc), fly = floor(yc);
        ix[k] = (int)flx, iy[k] = (int)fly;
        fx[k] = xc - flx, fy[k] = yc - fly;
        live[k] = finite && ix[k] + hi >= 0 && ix[k] + lo <= sw - 1 && iy[k] + hi >= 0 && iy[k] + lo <= sh - 1;
        if (live[k]) {
            b0 = min(b0, ix[k] + lo), b1 = min(b1, -(ix[k] + hi));
            b2 = min(b2, iy[k] + lo), b3 = min(b3, -(iy[k] + hi));
        }
    }
    b0 = wave_min(b0), b1 = wave_min(b1), b2 = wave_min(b2), b3 = wave_min(b3);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) fold[wave][0] = b0, fold[wave][1] = b1, fold[wave][2] = b2, fold[wave][3] = b3;
    __syncthreads();
    const int x_lo = min(min(fold[0][0], fold[1][0]), min(fold[2][0], fold[3][0]));
    const int x_hi = -min(min(fold[0][1], fold[1][1]), min(fold[2][1], fold[3][1]));
    const int y_lo = min(min(fold[0][2], fold[1][2]), min(fold[2][2], fold[3][2]));
    const int y_hi = -min(min(fold[0][3], fold[1][3]), min(fold[2][3], fold[3][3]));
    const bool any = x_lo != INT32_MAX;
    const int nwx = any ? x_hi - x_lo + 1 : 0, nwy = any ? y_hi - y_lo + 1 : 0;
    const bool staged = any && nwx <= kWin && nwy <= kWin && force != AMT_LENS_PATH_GATHER;      // the same for the whole block
    if (tile_path && threadIdx.x == 0) tile_path[blockIdx.y * gridDim.x + blockIdx.x] = !any ? 0 : (staged ? AMT_LENS_PATH_STAGED : AMT_LENS_PATH_GATHER);

    const int pitch = nwx * C;
    if (staged) {
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
        if (!(X < dw && Y < dh)) continue;
        T* out = dst + ((int64_t)Y * dw + X) * C;
        if (!live[k]) {
            for (int c = 0; c < C; ++c) out[c] = (T)0;
            continue;
        }
        double wx[N], wy[N];
        tap_weights<N>(fx[k], wx);
        tap_weights<N>(fy[k], wy);
        if (staged) {
            const window_fetch<T> f = {win, x_lo, y_lo, pitch, C};
            for (int c = 0; c < C; ++c) out[c] = to_sample<T>(sample<N>(f, ix[k] + lo, iy[k] + lo, c, wx, wy));
        } else {
            const global_fetch<T> f = {src, sw, sh, C};
            for (int c = 0; c < C; ++c) out[c] = to_sample<T>(sample<N>(f, ix[k] + lo, iy[k] + lo, c, wx, wy));
        }
    }
}

template <typename T, typename Coord>
int launch_remap_t(amt_ctx* ctx, const Coord& coord, const void* src, int sw, int sh, int C, int interpolation, void* dst, int dw, int dh,
                   uint8_t* support, const amt_lens_debug* dbg) {
    const dim3 grid((unsigned)((dw + kTile - 1) / kTile), (unsigned)((dh + kTile - 1) / kTile));
    const size_t lds = (size_t)kWin * kWin * (size_t)C * sizeof(T);
    const int force = dbg ? dbg->force_path : AMT_LENS_PATH_AUTO;
    uint8_t* tiles = dbg ? dbg->tile_path : nullptr;
    if (interpolation == AMT_INTERP_LINEAR)
        hipLaunchKernelGGL((k_remap<T, 2, Coord>), grid, dim3(256), lds, ctx->stream, coord, static_cast<const T*>(src), sw, sh, C,
                           static_cast<T*>(dst), dw, dh, support, force, tiles);
    else
        hipLaunchKernelGGL((k_remap<T, 8, Coord>), grid, dim3(256), lds, ctx->stream, coord, static_cast<const T*>(src), sw, sh, C,
                           static_cast<T*>(dst), dw, dh, support, force, tiles);
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

template <typename Coord>
int launch_remap(amt_ctx* ctx, const Coord& coord, const void* src, int sw, int sh, int sample_bytes, int C, int interpolation, void* dst,
                 int dw, int dh, uint8_t* support, const amt_lens_debug* dbg) {
    AMT_REQUIRE(ctx, src && dst, "NULL argument");
    AMT_REQUIRE(ctx, sample_bytes == 1 || sample_bytes == 2 || sample_bytes == 4, "sample_bytes must be 1 (uint8), 2 (uint16) or 4 (float32)");
    AMT_REQUIRE(ctx, C == 1 || C == 3 || C == 4, "channels must be 1, 3 or 4");
    AMT_REQUIRE(ctx, interpolation == AMT_INTERP_LINEAR || interpolation == AMT_INTERP_LANCZOS4, "unknown interpolation");
    AMT_REQUIRE(ctx, sw > 0 && sh > 0 && dw > 0 && dh > 0, "empty image");
    AMT_REQUIRE(ctx, !dbg || (dbg->force_path >= AMT_LENS_PATH_AUTO && dbg->force_path <= AMT_LENS_PATH_GATHER), "unknown force_path");
    if (amt_set_device(ctx)) return AMT_EHIP;
    switch (sample_bytes) {
        case 1: return launch_remap_t<uint8_t>(ctx, coord, src, sw, sh, C, interpolation, dst, dw, dh, support, dbg);
        case 2: return launch_remap_t<uint16_t>(ctx, coord, src, sw, sh, C, interpolation, dst, dw, dh, support, dbg);
        default: return launch_remap_t<float>(ctx, coord, src, sw, sh, C, interpolation, dst, dw, dh, support, dbg);
    }
}

int coords_call(amt_ctx* ctx, const amt_lens_model* model, int inverse, int32_t x0, int32_t y0, int32_t cols, int32_t rows, int corner,
                double* out_xy, float* out_xy32) {
    AMT_REQUIRE(ctx, lens_model_ok(model), "bad lens model (kind, size or crop)");
    AMT_REQUIRE(ctx, out_xy != nullptr, "NULL argument");
    AMT_REQUIRE(ctx, cols >= 0 && rows >= 0, "negative size");
    const int c = corner ? 1 : 0;
    if (cols + c == 0 || rows + c == 0 || (!c && (cols == 0 || rows == 0))) return AMT_OK;
    if (amt_set_device(ctx)) return AMT_EHIP;
    const double off = c ? -0.5 : 0.0;
    const dim3 grid((unsigned)((cols + c + 255) / 256), (unsigned)(rows + c));
    if (inverse)
        hipLaunchKernelGGL(k_lens_coords<true>, grid, dim3(256), 0, ctx->stream, make_lens(model), x0 + off, y0 + off, cols + c, out_xy, out_xy32);
    else
        hipLaunchKernelGGL(k_lens_coords<false>, grid, dim3(256), 0, ctx->stream, make_lens(model), x0 + off, y0 + off, cols + c, out_xy, out_xy32);
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

}  // namespace

extern "C" {

int amt_lens_coords(amt_ctx* ctx, const amt_lens_model* model, int32_t x0, int32_t y0, int32_t cols, int32_t rows, int corner, double* out_xy,
                    float* out_xy32) {
    AMT_CHECK_CTX(ctx);
    return coords_call(ctx, model, 0, x0, y0, cols, rows, corner, out_xy, out_xy32);
}

int amt_lens_undistort(amt_ctx* ctx, const amt_lens_model* model, int32_t x0, int32_t y0, int32_t cols, int32_t rows, int corner,
                       double* out_xy) {
    AMT_CHECK_CTX(ctx);
    return coords_call(ctx, model, 1, x0, y0, cols, rows, corner, out_xy, nullptr);
}

int amt_lens_remap(amt_ctx* ctx, const amt_lens_model* model, const void* src, int32_t sample_bytes, int32_t channels, int32_t interpolation,
                   void* dst, uint8_t* support, const amt_lens_debug* debug) {
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, lens_model_ok(model), "bad lens model (kind, size or crop)");
    const model_coord coord = {make_lens(model)};
    const int dw = model->crop_width ? model->crop_width : model->width, dh = model->crop_height ? model->crop_height : model->height;
    return launch_remap(ctx, coord, src, model->width, model->height, sample_bytes, channels, interpolation, dst, dw, dh, support, debug);
}

int amt_remap_coords(amt_ctx* ctx, const void* src, int32_t src_width, int32_t src_height, int32_t sample_bytes, int32_t channels,
                     const float* coords, int32_t dst_width, int32_t dst_height, int32_t interpolation, void* dst, uint8_t* support,
                     const amt_lens_debug* debug) {
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, coords != nullptr, "NULL argument");
    const array_coord coord = {coords, dst_width};
    return launch_remap(ctx, coord, src, src_width, src_height, sample_bytes, channels, interpolation, dst, dst_width, dst_height, support,
                        debug);
}

int amt_lens_fold_radius(const amt_lens_model* model, double* out_r) {
    if (model == nullptr || out_r == nullptr || model->kind < AMT_LENS_NONE || model->kind > AMT_LENS_PTLENS) return AMT_EINVAL;
    *out_r = lens_fold_radius(*model);
    return AMT_OK;
}

}  // extern "C"
