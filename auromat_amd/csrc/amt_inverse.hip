// Inverse georeferencing: world -> pixel (include/auromat_hip.h, "inverse georeferencing", is the statement).
// Two kernels, one thread per point, that share one __device__ function per step: k_world_to_pixel takes n points in SoA,
// k_grid_to_pixel the outer product of a latitude-like and a longitude-like axis (the cell centres of a plate carree grid are
// never materialised).  Everything that depends on the frame alone is prepared on the host (w2p_consts); the two SIP tables
// travel by value in the kernel arguments and are indexed with wave-uniform indices only, so they stay in scalar loads.
// A frame with a lens (the _lens entry points; w2p_lens, kernel arguments too) takes step 9 behind the camera model in the same
// kernels: one kernel family, and without a lens the bits of before.
#include "amt_common.h"
#include "amt_w2p.h"      // the per-point arithmetic and w2p_prepare (fp contract off from here on)

namespace {

using namespace amt;

constexpr int kGridCols = 4;                  // columns per thread of a work item of the grid kernel
constexpr int kGridRows = 8;                  // rows of a work item

__global__ void __launch_bounds__(kBlock)
k_world_to_pixel(w2p_consts K, w2p_sip S, w2p_lens Ln, const double* __restrict__ c0, const double* __restrict__ c1, int64_t n,
                 double* __restrict__ out_xy, double* __restrict__ out_elev, uint8_t* __restrict__ out_flags) {
    AMT_GRID_STRIDE(i, n) {
        const lat_terms T = w2p_lat_terms(K, c0[i]);
        double x, y, e;
        const unsigned fl = w2p_point_lens(K, S, Ln, T, w2p_lon_terms(c1[i]), x, y, e);
        out_xy[2 * i + 0] = x;
        out_xy[2 * i + 1] = y;
        if (out_elev) out_elev[i] = e;
        out_flags[i] = (uint8_t)fl;
    }
}

// A work item is kGridRows rows of kBlock * kGridCols consecutive columns: a thread keeps the longitude terms of its columns for
// the rows of the item and computes a row's latitude terms once, and each wave reads and writes 64 consecutive cells at a time.
__global__ void __launch_bounds__(kBlock)
k_grid_to_pixel(w2p_consts K, w2p_sip S, w2p_lens Ln, const double* __restrict__ lat, int ny, const double* __restrict__ lon, int nx,
                int items_per_row, float* __restrict__ out_xy32, double* __restrict__ out_xy, double* __restrict__ out_elev,
                uint8_t* __restrict__ out_flags) {
    const int row_groups = (ny + kGridRows - 1) / kGridRows;
    const int64_t items = (int64_t)row_groups * items_per_row;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int group = (int)(item / items_per_row), seg = (int)(item - (int64_t)group * items_per_row);
        const int col0 = seg * kGridCols * kBlock + (int)threadIdx.x;
        lon_terms L[kGridCols];
#pragma unroll
        for (int k = 0; k < kGridCols; ++k) {
            const int col = col0 + k * kBlock;
            L[k] = w2p_lon_terms(col < nx ? lon[col] : 0.0);
        }
        const int row_end = min(ny, (group + 1) * kGridRows);
        for (int row = group * kGridRows; row < row_end; ++row) {
            const lat_terms T = w2p_lat_terms(K, lat[row]);
#pragma unroll
            for (int k = 0; k < kGridCols; ++k) {
                const int col = col0 + k * kBlock;
                if (col >= nx) continue;
                double x, y, e;
                const unsigned fl = w2p_point_lens(K, S, Ln, T, L[k], x, y, e);
                const int64_t i = (int64_t)row * nx + col;
                if (out_xy32) {
                    out_xy32[2 * i + 0] = (float)x;
                    out_xy32[2 * i + 1] = (float)y;
                }
                if (out_xy) {
                    out_xy[2 * i + 0] = x;
                    out_xy[2 * i + 1] = y;
                }
                if (out_elev) out_elev[i] = e;
                out_flags[i] = (uint8_t)fl;
            }
        }
    }
}

// The entry points with and without a lens are one call each: `fn` is the name the caller knows, for the error texts.
#define W2P_REQUIRE(cond, msg)                                    \
    do {                                                           \
        if (!(cond)) {                                             \
            ctx->last_error = std::string(fn) + ": " + (msg);      \
            return AMT_EINVAL;                                     \
        }                                                          \
    } while (0)

int world_to_pixel_call(amt_ctx* ctx, const char* fn, const amt_frame_params* params, const amt_zenithal_wcs* zenithal, int32_t frame,
                        const double* c0, const double* c1, int64_t n, double* out_xy, double* out_elev, uint8_t* out_flags,
                        const amt_lens_model* lens) {
    AMT_CHECK_CTX(ctx);
    W2P_REQUIRE(params != nullptr, "NULL argument");
    W2P_REQUIRE(n >= 0, "negative size");
    W2P_REQUIRE(n == 0 || (c0 && c1 && out_xy && out_flags), "NULL argument");
    w2p_consts K;
    w2p_sip S;
    const char* err = w2p_prepare(params, zenithal, frame, &K, &S);
    W2P_REQUIRE(err == nullptr, err);
    w2p_lens Ln;
    err = w2p_lens_prepare(lens, params, zenithal, &Ln);
    W2P_REQUIRE(err == nullptr, err);
    if (n == 0) return AMT_OK;
    hipLaunchKernelGGL(k_world_to_pixel, grid_for(n), dim3(kBlock), 0, ctx->stream, K, S, Ln, c0, c1, n, out_xy, out_elev, out_flags);
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

int grid_to_pixel_call(amt_ctx* ctx, const char* fn, const amt_frame_params* params, const amt_zenithal_wcs* zenithal, int32_t frame,
                       const double* lat_centres, int32_t ny, const double* lon_centres, int32_t nx, float* out_xy32, double* out_xy,
                       double* out_elev, uint8_t* out_flags, const amt_lens_model* lens) {
    AMT_CHECK_CTX(ctx);
    W2P_REQUIRE(params && lat_centres && lon_centres && out_flags && (out_xy32 || out_xy), "NULL argument");
    W2P_REQUIRE(ny > 0 && nx > 0, "empty axis");
    w2p_consts K;
    w2p_sip S;
    const char* err = w2p_prepare(params, zenithal, frame, &K, &S);
    W2P_REQUIRE(err == nullptr, err);
    w2p_lens Ln;
    err = w2p_lens_prepare(lens, params, zenithal, &Ln);
    W2P_REQUIRE(err == nullptr, err);
    const int per_item = kBlock * kGridCols;
    const int items_per_row = (nx + per_item - 1) / per_item;
    int64_t blocks = (int64_t)((ny + kGridRows - 1) / kGridRows) * items_per_row;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(k_grid_to_pixel, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, K, S, Ln, lat_centres, ny, lon_centres,
                       nx, items_per_row, out_xy32, out_xy, out_elev, out_flags);
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

}  // namespace

extern "C" {

int amt_world_to_pixel(amt_ctx* ctx, const amt_frame_params* params, const amt_zenithal_wcs* zenithal, int32_t frame,
                       const double* c0, const double* c1, int64_t n, double* out_xy, double* out_elev, uint8_t* out_flags) {
    return world_to_pixel_call(ctx, __func__, params, zenithal, frame, c0, c1, n, out_xy, out_elev, out_flags, nullptr);
}

int amt_world_to_pixel_lens(amt_ctx* ctx, const amt_frame_params* params, const amt_zenithal_wcs* zenithal, int32_t frame,
                            const double* c0, const double* c1, int64_t n, double* out_xy, double* out_elev, uint8_t* out_flags,
                            const amt_lens_model* lens) {
    return world_to_pixel_call(ctx, __func__, params, zenithal, frame, c0, c1, n, out_xy, out_elev, out_flags, lens);
}

int amt_grid_to_pixel(amt_ctx* ctx, const amt_frame_params* params, const amt_zenithal_wcs* zenithal, int32_t frame,
                      const double* lat_centres, int32_t ny, const double* lon_centres, int32_t nx, float* out_xy32, double* out_xy,
                      double* out_elev, uint8_t* out_flags) {
    return grid_to_pixel_call(ctx, __func__, params, zenithal, frame, lat_centres, ny, lon_centres, nx, out_xy32, out_xy, out_elev,
                              out_flags, nullptr);
}

int amt_grid_to_pixel_lens(amt_ctx* ctx, const amt_frame_params* params, const amt_zenithal_wcs* zenithal, int32_t frame,
                           const double* lat_centres, int32_t ny, const double* lon_centres, int32_t nx, float* out_xy32,
                           double* out_xy, double* out_elev, uint8_t* out_flags, const amt_lens_model* lens) {
    return grid_to_pixel_call(ctx, __func__, params, zenithal, frame, lat_centres, ny, lon_centres, nx, out_xy32, out_xy, out_elev,
                              out_flags, lens);
}

}  // extern "C"
