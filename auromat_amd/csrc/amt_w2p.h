// World -> pixel, the per-point arithmetic (include/auromat_hip.h, "inverse georeferencing", is the statement): the constants of a
// frame prepared on the host (w2p_prepare) and one __device__ function per step.  Shared by the kernels of amt_inverse.hip (points
// and grids to coordinate arrays) and amt_gather.hip (the fused gather mosaic), which must give identical bits for identical points.
// Step 9, the lens of a raw frame applied after the camera model (w2p_lens, w2p_lens_step), is what its three callers add behind
// w2p_point when a frame has a lens: k_world_to_pixel and k_grid_to_pixel of amt_inverse.hip (through w2p_point_lens) and elect()
// of amt_gather.hip.
#pragma once

#include <cmath>
#include <cstring>

#include "amt_common.h"
#include "amt_lens.h"

// Every operation of the per-point arithmetic is rounded on its own (fused multiply-adds are written out where wanted): the
// kernels must give identical bits for identical points whatever code surrounds the shared functions.  (At file scope: it holds
// for the rest of the including file as well.)
#pragma clang fp contract(off)

namespace amt {

constexpr int kSipSteps = 20;                 // cap of the Newton iteration of the SIP inverse
constexpr double kSipTol = 0x1p-40;           // it stops after a step of at most kSipTol * max(1, |u|, |v|) pixels

struct w2p_consts {
    int32_t frame, projection, width, height;
    int32_t sip_order_a, sip_order_b, inside, pad_;
    double cam[3], cs[3];       // camera; camera / (a, a, b)
    double ia, ib;              // 1/a, 1/b
    double a0, e2;              // WGS84 semi-major axis, first eccentricity squared
    double m[9];                // J2000 -> GEO or J2000 -> SM (applied transposed)
    double rot[9];              // native -> celestial (applied transposed)
    double icd[4];              // CD^-1
    double off_x, off_y;        // CRPIX - 1 - start
    double os[3], oo;           // -cs and |cs|^2: the forward's ray constants (ellipsoid_ray)
};

struct w2p_sip {
    double a[AMT_SIP_MAX][AMT_SIP_MAX], b[AMT_SIP_MAX][AMT_SIP_MAX];
};

// what a point's first coordinate (latitude, MLat, declination) contributes
struct lat_terms {
    double c, s;        // cos, sin
    double r, z;        // GEODETIC: N cos(lat), N (1 - e^2) sin(lat) [km], the point of the WGS84 ellipsoid below P
    bool bad;           // non-finite or |lat| > 90
};

__device__ __forceinline__ lat_terms w2p_lat_terms(const w2p_consts& K, double lat) {
    lat_terms T;
    T.bad = !(fabs(lat) <= 90.0);
    sincos(lat * kDeg2Rad, &T.s, &T.c);
    const double n = K.a0 / sqrt(1.0 - K.e2 * T.s * T.s);
    T.r = n * T.c;
    T.z = n * (1.0 - K.e2) * T.s;
    return T;
}

// f = sum c[p][q] u^p v^q and its two partial derivatives (p + q <= order)
__device__ __forceinline__ void sip_eval_d(const double (&c)[AMT_SIP_MAX][AMT_SIP_MAX], int order, double u, double v, double& f,
                                           double& fu, double& fv) {
    f = fu = fv = 0;
    double up = 1, upm = 0;         // u^p, p u^(p-1)
    for (int p = 0; p <= order; ++p) {
        double g = 0, gv = 0, vq = 1, vqm = 0;      // v^q, q v^(q-1)
        for (int q = 0; q <= order - p; ++q) {
            g = __builtin_fma(c[p][q], vq, g);
            gv = __builtin_fma(c[p][q], vqm, gv);
            vqm = (double)(q + 1) * vq;
            vq *= v;
        }
        f = __builtin_fma(g, up, f);
        fu = __builtin_fma(g, upm, fu);
        fv = __builtin_fma(gv, up, fv);
        upm = (double)(p + 1) * up;
        up *= u;
    }
}

// what a point's second coordinate (longitude, SM longitude, right ascension) contributes
struct lon_terms {
    double s, c;
    bool bad;           // non-finite
};

__device__ __forceinline__ lon_terms w2p_lon_terms(double lon) {
    lon_terms L;
    L.bad = !finite(lon);
    const double lr = lon - 360.0 * floor((lon + 180.0) / 360.0);       // [-180, 180): 180, -180 and 540 are one number
    sincos(lr * kDeg2Rad, &L.s, &L.c);
    return L;
}

// Steps 1-8 of the statement for the point (T, L).  Returns the flag byte; x, y, elev as the statement defines them.
__device__ __forceinline__ unsigned w2p_point(const w2p_consts& K, const w2p_sip& S, const lat_terms& T, const lon_terms& L,
                                              double& x, double& y, double& elev) {
    x = y = elev = NAN;
    if (T.bad || L.bad) return AMT_W2P_INVALID;
    const double so = L.s, co = L.c;
    // the unit vector of the two angles (GEODETIC: the ellipsoid's normal), through m^T into J2000
    const double gx = T.c * co, gy = T.c * so, gz = T.s;
    double px = K.m[0] * gx + K.m[3] * gy + K.m[6] * gz;
    double py = K.m[1] * gx + K.m[4] * gy + K.m[7] * gz;
    double pz = K.m[2] * gx + K.m[5] * gy + K.m[8] * gz;
    if (K.frame == AMT_W2P_GEODETIC) {
        // P(h) = P0 + h nu on the shell, whose axes are J2000's as in the forward: A h^2 + 2 B h + C = 0 with B > 0, the
        // larger root h = -C / (B + sqrt(B^2 - A C)) (no cancellation whatever the sign of C)
        const double ex = T.r * co, ey = T.r * so, ez = T.z;
        const double p0x = K.m[0] * ex + K.m[3] * ey + K.m[6] * ez;
        const double p0y = K.m[1] * ex + K.m[4] * ey + K.m[7] * ez;
        const double p0z = K.m[2] * ex + K.m[5] * ey + K.m[8] * ez;
        const double sx = px * K.ia, sy = py * K.ia, sz = pz * K.ib;
        const double tx = p0x * K.ia, ty = p0y * K.ia, tz = p0z * K.ib;
        const double A = sx * sx + sy * sy + sz * sz, B = sx * tx + sy * ty + sz * tz;
        const double Cq = __builtin_fma(tx, tx, __builtin_fma(ty, ty, __builtin_fma(tz, tz, -1.0)));
        const double h = -Cq / (B + sqrt(B * B - A * Cq));
        px = __builtin_fma(h, px, p0x), py = __builtin_fma(h, py, p0y), pz = __builtin_fma(h, pz, p0z);
    }
    unsigned flags = 0;
    double dx, dy, dz;
    if (K.frame == AMT_W2P_J2000) {
        dx = px, dy = py, dz = pz;
        // hidden iff the ray hits the shell: the forward's rule (ray_param, directed)
        const double sx = dx * K.ia, sy = dy * K.ia, sz = dz * K.ib;
        const double d_o = sx * K.os[0] + sy * K.os[1] + sz * K.os[2];
        const double d_d = sx * sx + sy * sy + sz * sz;
        const double disc = d_o * d_o - K.oo * d_d + d_d;
        if (disc >= 0) {
            const double root = sqrt(disc);
            if ((K.inside ? d_o + root : d_o - root) >= 0) flags |= AMT_W2P_HIDDEN;
        }
    } else {
        if (K.frame == AMT_W2P_SM) {
            const double qx = px * K.ia, qy = py * K.ia, qz = pz * K.ib;
            const double sc = 1.0 / sqrt(qx * qx + qy * qy + qz * qz);
            px *= sc, py *= sc, pz *= sc;
        }
        const double wx = px - K.cam[0], wy = py - K.cam[1], wz = pz - K.cam[2];
        const double dist = sqrt(wx * wx + wy * wy + wz * wz);
        dx = wx / dist, dy = wy / dist, dz = wz / dist;
        // visible iff the camera is inside the shell or on the outer side of the tangent plane at P
        const double qc = (px * K.ia) * K.cs[0] + (py * K.ia) * K.cs[1] + (pz * K.ib) * K.cs[2];
        if (!(K.inside || qc > 1.0)) flags |= AMT_W2P_HIDDEN;
        // elevation = 90 deg - angle(-d, P / |P|), as the arctangent of sine over cosine: accurate at the zenith too
        const double cx = dy * pz - dz * py, cy = dz * px - dx * pz, cz = dx * py - dy * px;
        elev = atan2(-(dx * px + dy * py + dz * pz), sqrt(cx * cx + cy * cy + cz * cz)) * kRad2Deg;
    }
    // native direction rot^T d
    const double l = K.rot[0] * dx + K.rot[3] * dy + K.rot[6] * dz;
    const double m = K.rot[1] * dx + K.rot[4] * dy + K.rot[7] * dz;
    const double n = K.rot[2] * dx + K.rot[5] * dy + K.rot[8] * dz;
    const double rho = sqrt(l * l + m * m);
    double f;           // R / rho
    bool ok;
    switch (K.projection) {
        case 0: ok = n > 0, f = kRad2Deg / n; break;                                     // TAN
        case 1: ok = n >= 0, f = kRad2Deg; break;                                        // SIN
        case 2: ok = rho > 0 || n > 0, f = kRad2Deg * atan2(rho, n) / rho; break;        // ARC
        case 3: ok = n > -1, f = 2.0 * kRad2Deg / (1.0 + n); break;                      // STG
        default: ok = n > -1, f = kRad2Deg * sqrt(2.0 / (1.0 + n)); break;               // ZEA: 1 - n = rho^2 / (1 + n)
    }
    if (rho == 0 && !(n > 0)) ok = false;        // the antipode of the boresight has no position angle
    if (!ok || !finite(n) || !finite(rho)) return flags | AMT_W2P_UNPROJECTABLE;
    const double wx_ = rho == 0 ? 0.0 : f * m, wy_ = rho == 0 ? 0.0 : -(f * l);
    const double U = K.icd[0] * wx_ + K.icd[1] * wy_, V = K.icd[2] * wx_ + K.icd[3] * wy_;
    double u = U, v = V;
    if (K.sip_order_a > 0 || K.sip_order_b > 0) {
        bool done = false;
        for (int it = 0; it < kSipSteps; ++it) {
            double fa = 0, fau = 0, fav = 0, fb = 0, fbu = 0, fbv = 0;
            if (K.sip_order_a > 0) sip_eval_d(S.a, K.sip_order_a, u, v, fa, fau, fav);
            if (K.sip_order_b > 0) sip_eval_d(S.b, K.sip_order_b, u, v, fb, fbu, fbv);
            const double j00 = 1.0 + fau, j11 = 1.0 + fbv;
            const double det = j00 * j11 - fav * fbu;
            if (!(det > 0)) break;
            const double r0 = (u + fa) - U, r1 = (v + fb) - V;
            const double du = (j11 * r0 - fav * r1) / det, dv = (j00 * r1 - fbu * r0) / det;
            u -= du, v -= dv;
            if (!finite(u) || !finite(v)) break;
            if (fmax(fabs(du), fabs(dv)) <= kSipTol * fmax(1.0, fmax(fabs(u), fabs(v)))) {
                done = true;
                break;
            }
        }
        if (!done) return flags | AMT_W2P_NOT_CONVERGED;
    }
    x = u + K.off_x;
    y = v + K.off_y;
    if (!finite(x) || !finite(y)) {
        x = y = NAN;
        return flags | AMT_W2P_UNPROJECTABLE;
    }
    if (!(x >= -0.5 && x <= K.width - 0.5 && y >= -0.5 && y <= K.height - 0.5)) flags |= AMT_W2P_OUTSIDE;
    return flags;
}

// ---- step 9: through the lens ----------------------------------------------------------------------------------------------
// the constants of a frame's lens (kind AMT_LENS_NONE: the frame has none) and the square of the radius at which the model folds
struct w2p_lens {
    lens_dev m;
    double fold2;       // r_fold^2: +inf where the model never folds, NaN with a NaN coefficient (no point is kept then)
};

// Step 9 for a point that w2p_point has placed at (x, y) of the cropped corrected frame with the flags `flags`: (x, y) becomes the
// point of the raw frame, width x height, that lens_forward samples for it, and OUTSIDE is decided there.
__device__ __forceinline__ unsigned w2p_lens_step(const w2p_lens& Ln, int width, int height, unsigned flags, double& x, double& y) {
    if (!(x == x)) return flags;        // INVALID, UNPROJECTABLE, NOT_CONVERGED: no pixel to take through the lens
    flags &= ~(unsigned)AMT_W2P_OUTSIDE;
    const double Xf = x + (double)Ln.m.crop_x, Yf = y + (double)Ln.m.crop_y;
    const double r2 = lens_r2(Ln.m, Xf, Yf);
    const double g = lens_g(Ln.m, r2);
    // the principal branch alone: beyond the fold the polynomial maps far-off points back into the frame
    if (!(r2 < Ln.fold2) || !finite(g)) {
        x = y = NAN;
        return flags | AMT_W2P_LENS_FOLD;
    }
    lens_forward(Ln.m, Xf, Yf, x, y);
    if (!(x >= -0.5 && x <= width - 0.5 && y >= -0.5 && y <= height - 0.5)) flags |= AMT_W2P_OUTSIDE;
    return flags;
}

// Steps 1-9: w2p_point, then the lens where the frame has one (the same for every thread of a launch)
__device__ __forceinline__ unsigned w2p_point_lens(const w2p_consts& K, const w2p_sip& S, const w2p_lens& Ln, const lat_terms& T,
                                                   const lon_terms& L, double& x, double& y, double& elev) {
    const unsigned flags = w2p_point(K, S, T, L, x, y, elev);
    return Ln.m.kind == AMT_LENS_NONE ? flags : w2p_lens_step(Ln, K.width, K.height, flags, x, y);
}

// Host: a frame's lens as the kernels read it.  NULL or kind AMT_LENS_NONE: no lens.  `p`, `z`: the frame the lens belongs to, as
// w2p_prepare takes them.  NULL: all is well.
inline const char* w2p_lens_prepare(const amt_lens_model* lens, const amt_frame_params* p, const amt_zenithal_wcs* z, w2p_lens* L) {
    std::memset(L, 0, sizeof(*L));
    if (lens == nullptr || lens->kind == AMT_LENS_NONE) return nullptr;
    if (lens->kind < AMT_LENS_NONE || lens->kind > AMT_LENS_PTLENS) return "unknown lens kind";
    if (!(lens->width > 0 && lens->height > 0)) return "lens: empty raw frame";
    if (!lens_model_ok(lens)) return "lens: the crop window does not lie in the corrected frame";
    if (lens->width != p->width || lens->height != p->height) return "lens: the raw frame's size is not the params' width x height";
    const int cw = lens->crop_width ? lens->crop_width : lens->width, ch = lens->crop_height ? lens->crop_height : lens->height;
    if (z && (z->width != cw || z->height != ch)) return "lens: the corrected frame's size is not the camera model's (zenithal width x height)";
    L->m = make_lens(lens);
    const double r = lens_fold_radius(*lens);
    L->fold2 = r * r;
    return nullptr;
}

// Host: the argument checks shared by the entry points and the constants of the frame.  NULL: all is well.
inline const char* w2p_prepare(const amt_frame_params* p, const amt_zenithal_wcs* z, int32_t frame, w2p_consts* K, w2p_sip* S) {
    if (frame != AMT_W2P_GEODETIC && frame != AMT_W2P_SM && frame != AMT_W2P_J2000) return "unknown frame";
    if (!(p->width > 0 && p->height > 0)) return "empty frame";
    if (!(p->a > 0 && p->b > 0 && p->a0 > 0 && p->b0 > 0 && p->b0 <= p->a0)) return "bad axes";
    std::memset(K, 0, sizeof(*K));
    std::memset(S, 0, sizeof(*S));
    const double *cd = p->cd, *crpix = p->crpix, *rot = p->rot;
    double sx = 0, sy = 0;
    if (z) {
        if (z->projection < 0 || z->projection > 4) return "projection must be 0 TAN, 1 SIN, 2 ARC, 3 STG or 4 ZEA";
        if (z->sip_order_a < 0 || z->sip_order_a >= AMT_SIP_MAX || z->sip_order_b < 0 || z->sip_order_b >= AMT_SIP_MAX)
            return "SIP order out of range";
        cd = z->cd, crpix = z->crpix, rot = z->rot;
        sx = z->start_x, sy = z->start_y;
        K->projection = z->projection;
        K->sip_order_a = z->sip_order_a;
        K->sip_order_b = z->sip_order_b;
        std::memcpy(S->a, z->sip_a, sizeof(S->a));
        std::memcpy(S->b, z->sip_b, sizeof(S->b));
    }
    const double det = cd[0] * cd[3] - cd[1] * cd[2];
    if (!(std::fabs(det) > 0) || !std::isfinite(det)) return "singular CD matrix";
    K->icd[0] = cd[3] / det, K->icd[1] = -cd[1] / det, K->icd[2] = -cd[2] / det, K->icd[3] = cd[0] / det;
    K->off_x = crpix[0] - 1.0 - sx;
    K->off_y = crpix[1] - 1.0 - sy;
    K->frame = frame;
    K->width = p->width, K->height = p->height;
    K->ia = 1.0 / p->a, K->ib = 1.0 / p->b;
    K->a0 = p->a0;
    K->e2 = (p->a0 * p->a0 - p->b0 * p->b0) / (p->a0 * p->a0);
    const double sc[3] = {K->ia, K->ia, K->ib};
    for (int i = 0; i < 3; ++i) {
        K->cam[i] = p->cam[i];
        K->cs[i] = p->cam[i] * sc[i];
        K->os[i] = -K->cs[i];
        K->oo += K->cs[i] * K->cs[i];
    }
    K->inside = K->oo < 1;
    static const double identity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double* m = frame == AMT_W2P_GEODETIC ? p->m_geo : frame == AMT_W2P_SM ? p->m_sm : identity;
    for (int i = 0; i < 9; ++i) K->m[i] = m[i], K->rot[i] = rot[i];
    return nullptr;
}

}  // namespace amt
