// The radial lens models (include/auromat_hip.h, "lens distortion", is the statement): the constants of a model prepared on the
// host (make_lens), one __device__ function per step, and the host-only radius at which a model folds over.  Shared by the lens
// kernels (amt_lens.hip) and by step 9 of world -> pixel (amt_w2p.h: the point and grid kernels of amt_inverse.hip and elect() of
// amt_gather.hip), which must give identical
// bits for identical coordinates.  Every function switches fp contraction off for itself, so that it computes the same bits
// whatever the including file's setting is.
#pragma once

#include <cmath>
#include <utility>

#include "amt_common.h"

namespace amt {

struct lens_dev {
    int kind, crop_x, crop_y, pad_;
    double k0, k1, k2;
    double cx, cy, norm;
};

inline lens_dev make_lens(const amt_lens_model* m) {
    lens_dev d;
    d.kind = m->kind;
    d.crop_x = m->crop_x, d.crop_y = m->crop_y, d.pad_ = 0;
    d.k0 = m->k[0], d.k1 = m->k[1], d.k2 = m->k[2];
    d.cx = (m->width - 1) / 2.0;
    d.cy = (m->height - 1) / 2.0;
    const int side = (m->width < m->height ? m->width : m->height) - 1;
    d.norm = 2.0 / (side < 1 ? 1 : side);      // (a frame one pixel wide has no half side: radius in pixels)
    return d;
}

// kind, size and crop window of a model as every entry point requires them
inline bool lens_model_ok(const amt_lens_model* m) {
    if (m == nullptr || m->kind < AMT_LENS_NONE || m->kind > AMT_LENS_PTLENS || m->width <= 0 || m->height <= 0) return false;
    if (m->crop_width == 0 && m->crop_height == 0) return m->crop_x == 0 && m->crop_y == 0;
    return m->crop_width > 0 && m->crop_height > 0 && m->crop_x >= 0 && m->crop_y >= 0 && m->crop_x + m->crop_width <= m->width &&
           m->crop_y + m->crop_height <= m->height;
}

// g(r) of the model, from r^2; every operation spelled out so that the NumPy statement can follow it step by step
__device__ __forceinline__ double lens_g(const lens_dev& m, double r2) {
#pragma clang fp contract(off)
    switch (m.kind) {
        case AMT_LENS_POLY3: return (1.0 - m.k0) + m.k0 * r2;
        case AMT_LENS_POLY5: return (1.0 + m.k0 * r2) + m.k1 * (r2 * r2);
        case AMT_LENS_PTLENS: {
            const double r = sqrt(r2);
            return ((m.k0 * (r2 * r) + m.k1 * r2) + m.k2 * r) + (((1.0 - m.k0) - m.k1) - m.k2);
        }
        default: return 1.0;
    }
}

// d(r g(r)) / dr
__device__ __forceinline__ double lens_slope(const lens_dev& m, double r) {
#pragma clang fp contract(off)
    const double r2 = r * r;
    switch (m.kind) {
        case AMT_LENS_POLY3: return (1.0 - m.k0) + (3.0 * m.k0) * r2;
        case AMT_LENS_POLY5: return (1.0 + (3.0 * m.k0) * r2) + (5.0 * m.k1) * (r2 * r2);
        case AMT_LENS_PTLENS:
            return (((4.0 * m.k0) * (r2 * r) + (3.0 * m.k1) * r2) + (2.0 * m.k2) * r) + (((1.0 - m.k0) - m.k1) - m.k2);
        default: return 1.0;
    }
}

// r^2 of the corrected full-frame coordinate (X, Y), as lens_forward forms it
__device__ __forceinline__ double lens_r2(const lens_dev& m, double X, double Y) {
#pragma clang fp contract(off)
    const double u = (X - m.cx) * m.norm, v = (Y - m.cy) * m.norm;
    return u * u + v * v;
}

// corrected full-frame coordinate (X, Y) -> where to sample the raw frame
__device__ __forceinline__ void lens_forward(const lens_dev& m, double X, double Y, double& xs, double& ys) {
#pragma clang fp contract(off)
    const double u = (X - m.cx) * m.norm, v = (Y - m.cy) * m.norm;
    const double g = lens_g(m, u * u + v * v);
    // (a n) / n need not round back to a: a factor of exactly 1 returns the pixel's own coordinate
    const bool same = g == 1.0;
    xs = same ? X : m.cx + (u * g) / m.norm;
    ys = same ? Y : m.cy + (v * g) / m.norm;
}

constexpr int kNewtonCap = 24;

// raw coordinate -> corrected full-frame coordinate: ru with ru g(ru) = rd by Newton's method from ru = rd.  NaN where the
// slope d(ru g)/dru is not positive on the way (the model folds over), where kNewtonCap steps do not converge, and for NaN input
__device__ __forceinline__ void lens_inverse(const lens_dev& m, double x, double y, double& X, double& Y) {
#pragma clang fp contract(off)
    const double u = (x - m.cx) * m.norm, v = (y - m.cy) * m.norm;
    const double rd = sqrt(u * u + v * v);
    if (rd == 0.0) {
        // the centre maps to itself whatever the model, unless a coefficient is NaN
        const bool bad = lens_g(m, 0.0) != lens_g(m, 0.0);
        X = bad ? NAN : m.cx, Y = bad ? NAN : m.cy;
        return;
    }
    double ru = rd;
    bool ok = false;
    for (int it = 0; it < kNewtonCap; ++it) {
        const double slope = lens_slope(m, ru);
        if (!(slope > 0.0)) break;
        const double step = (ru * lens_g(m, ru * ru) - rd) / slope;
        ru = ru - step;
        if (!(ru > 0.0)) break;
        if (fabs(step) <= 1e-13 * ru) {
            ok = lens_slope(m, ru) > 0.0;
            break;
        }
    }
    const double s = ok ? ru / rd : NAN;
    const bool same = s == 1.0;             // as in lens_forward
    X = same ? x : m.cx + (u * s) / m.norm;
    Y = same ? y : m.cy + (v * s) / m.norm;
}

// ---- host only: where the model folds over ------------------------------------------------------------------------------
// r_fold: the smallest r > 0 with d(r g)/dr = 0 (lens_slope, whose coefficients 3 k0, 5 k1, 4 a, 3 b, 2 c and 1 - a - b - c are
// float64 roundings: the root is that of the polynomial the kernels evaluate), +inf where there is none, 0 where the slope is
// not positive at the centre already, NaN for a NaN coefficient.  Beyond it the forward polynomial maps far-off corrected points
// back into the raw frame, and the inverse (lens_inverse) has no value.
inline double lens_fold_radius(const amt_lens_model& m) {
    const double k0 = m.k[0], k1 = m.k[1], k2 = m.k[2];
    switch (m.kind) {
        case AMT_LENS_POLY3: {
            // (1 - k0) + 3 k0 r^2
            if (k0 != k0) return NAN;
            const double c0 = 1.0 - k0, c2 = 3.0 * k0;
            if (!(c0 > 0.0)) return 0.0;
            return c2 < 0.0 ? std::sqrt(c0 / -c2) : INFINITY;
        }
        case AMT_LENS_POLY5: {
            // 1 + b s + a s^2 in s = r^2: the smaller positive root, by the formula that does not cancel
            if (k0 != k0 || k1 != k1) return NAN;
            const double b = 3.0 * k0, a = 5.0 * k1;
            double s = INFINITY;
            if (a == 0.0) {
                if (b < 0.0) s = -1.0 / b;
            } else {
                const double disc = std::fma(b, b, -4.0 * a);
                if (disc >= 0.0) {
                    const double q = -0.5 * (b + std::copysign(std::sqrt(disc), b));      // s1 = q / a, s2 = 1 / q
                    const double s1 = q / a, s2 = 1.0 / q;
                    if (s1 > 0.0) s = s1;
                    if (s2 > 0.0 && s2 < s) s = s2;
                }
            }
            return std::sqrt(s);
        }
        case AMT_LENS_PTLENS: {
            // c3 r^3 + c2 r^2 + c1 r + c0: its monotonic pieces lie between the positive roots of the derivative; the first piece
            // at whose end the slope is not positive any more holds the root, found by bisection to the last bit
            if (k0 != k0 || k1 != k1 || k2 != k2) return NAN;
            const long double c3 = 4.0 * k0, c2 = 3.0 * k1, c1 = 2.0 * k2, c0 = ((1.0 - k0) - k1) - k2;
            if (!(c0 > 0.0L)) return 0.0;
            const auto f = [&](long double r) { return ((c3 * r + c2) * r + c1) * r + c0; };
            // positive roots of 3 c3 r^2 + 2 c2 r + c1, ascending
            long double t[2];
            int nt = 0;
            const long double qa = 3.0L * c3, qb = 2.0L * c2, qc = c1;
            if (qa == 0.0L) {
                if (qb != 0.0L && -qc / qb > 0.0L) t[nt++] = -qc / qb;
            } else {
                const long double disc = qb * qb - 4.0L * qa * qc;
                if (disc >= 0.0L) {
                    const long double q = -0.5L * (qb + std::copysign(std::sqrt(disc), qb));
                    long double r1 = q / qa, r2 = q != 0.0L ? qc / q : 0.0L;
                    if (r1 > r2) std::swap(r1, r2);
                    if (r1 > 0.0L && std::isfinite(r1)) t[nt++] = r1;
                    if (r2 > 0.0L && std::isfinite(r2) && r2 != r1) t[nt++] = r2;
                }
            }
            long double lo = 0.0L, hi = -1.0L;       // f(lo) > 0; hi: the end of the piece that holds the root, once found
            for (int i = 0; i < nt && hi < 0.0L; ++i) {
                if (f(t[i]) <= 0.0L)
                    hi = t[i];
                else
                    lo = t[i];
            }
            if (hi < 0.0L) {
                // the last piece runs to infinity: a root iff the leading coefficient is negative
                const long double lead = c3 != 0.0L ? c3 : (c2 != 0.0L ? c2 : c1);
                if (!(lead < 0.0L)) return INFINITY;
                hi = lo > 1.0L ? 2.0L * lo : 1.0L;
                while (f(hi) > 0.0L) {
                    lo = hi, hi *= 2.0L;
                    if (!(hi < 1e300L)) return INFINITY;
                }
            }
            for (int it = 0; it < 256; ++it) {
                const long double mid = lo + (hi - lo) / 2.0L;
                if (!(mid > lo && mid < hi)) break;
                if (f(mid) > 0.0L)
                    lo = mid;
                else
                    hi = mid;
            }
            return (double)hi;
        }
        default: return INFINITY;
    }
}

}  // namespace amt
