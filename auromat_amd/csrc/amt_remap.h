// Sampling an image at fractional positions (include/auromat_hip.h, "Sampling (both remap calls)", is the statement): the tap
// weights, the two ways to fetch a tap and the one sampling function.  Shared by k_remap (amt_lens.hip) and the fused gather mosaic
// (amt_gather.hip), which must give identical bits for identical positions; so is the tiling both use.
#pragma once

#include "amt_common.h"

namespace amt {

constexpr int kTile = 32;            // output tile, pixels per side
constexpr int kRowsPerThread = 4;    // rows of the tile a thread makes (8 rows apart)
constexpr int kWin = 48;             // staging window, source pixels per side: the tile, 7 for the taps, 9 for the displacement

// ---- sampling -------------------------------------------------------------------------------------------------------

// tap weights of one axis for the fractional position f in [0, 1): N = 2 linear (taps 0, 1), N = 8 Lanczos-4 (taps o = -3 ... 4 at
// t = o - f), L(t) = sinc(t) sinc(t / 4) with L = 1 at 0 and 0 at the other integers exactly, the eight normalised to sum 1.
// Sixteen sines per axis cost more than the 64 taps of three channels (1.1 of 1.9 ms on a 12 Mpx frame), so the eight of each kind
// come from three evaluations: sin(pi (o - f)) = -(-1)^o sin(pi f) exactly, and sin(pi t / 4) by the addition theorem from the sine and
// cosine of pi f / 4 (taps o <= 0) and of pi (1 - f) / 4 (taps o >= 1, t = (o - 1) + (1 - f)) with the constants sin / cos(k pi / 4) —
// split that way no difference of nearly equal terms meets a weight that is not itself vanishing (only o = -3 and o = 4 subtract,
// where t -> -4, 4 and L -> 0).
template <int N>
__device__ __forceinline__ void tap_weights(double f, double (&w)[N]) {
#pragma clang fp contract(off)
    if (N == 2) {
        w[0] = 1.0 - f, w[1] = f;
        return;
    }
    if (f == 0.0) {
#pragma unroll
        for (int i = 0; i < N; ++i) w[i] = i == 3 ? 1.0 : 0.0;
        return;
    }
    const double s1 = sinpi(f);
    double sa, ca, sb, cb;
    sincospi(f * 0.25, &sa, &ca);
    sincospi((1.0 - f) * 0.25, &sb, &cb);
    constexpr double h = 0.70710678118654752440;
    // sin(pi t / 4) for o = -3 ... 4
    const double q[8] = {-(h * (ca - sa)), -ca, -(h * (ca + sa)), -sa, sb, h * (cb + sb), cb, h * (cb - sb)};
    constexpr double k = 4.0 / (M_PI * M_PI);
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double t = (double)(i - 3) - f;           // 0 < |t| < 4, never an integer
        const double n1 = (i & 1) ? -s1 : s1;           // sin(pi t): o = i - 3 is even where i is odd
        const double rt = 1.0 / t;                      // (not 1 / t^2: t^2 underflows for a tiny f while sin(pi t) / t does not)
        w[i] = ((n1 * rt) * (q[i] * rt)) * k;
        sum = sum + w[i];
    }
    const double inv = 1.0 / sum;
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = w[i] * inv;
}

template <typename T>
__device__ __forceinline__ T to_sample(double v);
template <>
__device__ __forceinline__ uint8_t to_sample<uint8_t>(double v) {
    return (uint8_t)fmin(fmax(rint(v), 0.0), 255.0);
}
template <>
__device__ __forceinline__ uint16_t to_sample<uint16_t>(double v) {
    return (uint16_t)fmin(fmax(rint(v), 0.0), 65535.0);
}
template <>
__device__ __forceinline__ float to_sample<float>(double v) {
    return (float)v;
}

// taps from the staged window (zeros outside the image are in it)
template <typename T>
struct window_fetch {
    const T* win;
    int x0, y0, pitch, C;       // pitch: samples per window row
    __device__ __forceinline__ double operator()(int x, int y, int c) const { return (double)win[(y - y0) * pitch + (x - x0) * C + c]; }
};

// taps from global memory, zero outside the image
template <typename T>
struct global_fetch {
    const T* src;
    int w, h, C;
    __device__ __forceinline__ double operator()(int x, int y, int c) const {
        const bool in = x >= 0 && x < w && y >= 0 && y < h;
        return in ? (double)src[((int64_t)y * w + x) * C + c] : 0.0;
    }
};

// the one sampling function: rows of taps first, then the column, accumulated in float64 in a fixed order
template <int N, typename Fetch>
__device__ __forceinline__ double sample(const Fetch& fetch, int tx0, int ty0, int c, const double (&wx)[N], const double (&wy)[N]) {
#pragma clang fp contract(off)
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double row = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i) row = __builtin_fma(wx[i], fetch(tx0 + i, ty0 + j, c), row);
        acc = __builtin_fma(wy[j], row, acc);
    }
    return acc;
}

__device__ __forceinline__ int wave_min(int v) {
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}

}  // namespace amt
