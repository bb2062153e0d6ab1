// Map projections on the device: the stereographic projection of an ellipsoid and the polar azimuthal equidistant projection of a
// sphere, forward and inverse, elementwise over n points (include/auromat_hip.h, "map projections").  Snyder, Map Projections - A
// Working Manual, ch. 21 and 25; the constants come from the host (amt_params.h: projection_stereographic,
// projection_polar_aeqd), so that oblique, equatorial and polar centres are ONE expression here.
//
// A point moves 32 bytes (two doubles in, two out), so the forward kernel keeps its transcendentals few: one sincos for the
// latitude, one for the longitude difference, one log and one exp for w = ((1 - e s) / (1 + e s))^e, one sqrt — sin chi and
// cos chi follow from s = sin phi and w by + - * / alone (conformal_sin_cos of amt_params.h states the same expressions).
//
// The inverse recovers the point on the conformal sphere as three numbers proportional to (sin chi, cos chi cos dlon,
// cos chi sin dlon) — rational in x / k and y / k, no trigonometry —, the longitude by one atan2, and the geodetic latitude
// from tan chi by Newton's method on tan phi (Karney, Transverse Mercator with an accuracy of a few nanometers, 2011, eq. 7
// and 19-21: well conditioned from the equator to the poles, two or three steps for terrestrial eccentricities, none for a sphere).
#include "amt_common.h"
#include "amt_params.h"

namespace {

using namespace amt;

struct proj_dev {
    double lon0, e, sin_chi1, cos_chi1, k;
    int north;
};

// a longitude into [-180, 180) (the two corrections: l + 180 may round up to a multiple of 360 from just below it)
__device__ __forceinline__ double wrap_lon(double l) {
    double w = l - 360.0 * floor((l + 180.0) / 360.0);
    if (w < -180.0) w += 360.0;
    if (w >= 180.0) w -= 360.0;
    return w;
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void k_project_forward(proj_dev P, const double* __restrict__ lat, const double* __restrict__ lon,
                                                            int64_t n, double* __restrict__ x, double* __restrict__ y) {
    AMT_GRID_STRIDE(i, n) {
        const double la = lat[i], lo = lon[i];
        double ox = NAN, oy = NAN;
        if (finite(la) && finite(lo)) {
            double sl, cl;
            sincos((lo - P.lon0) * kDeg2Rad, &sl, &cl);
            if (KIND == AMT_PROJ_POLAR_AEQD) {
                const double colat = P.north ? 90.0 - la : 90.0 + la;        // degrees from the centre
                if (colat <= 90.0) {
                    const double rho = P.k * (colat * kDeg2Rad);
                    ox = rho * sl;
                    oy = P.north ? -(rho * cl) : rho * cl;
                }
            } else {
                double s, c;
                sincos(la * kDeg2Rad, &s, &c);
                const double es = P.e * s;
                const double w = exp(P.e * log((1.0 - es) / (1.0 + es)));
                const double plus = s >= 0 ? 1.0 + s : c * c / (1.0 - s);
                const double minus = s >= 0 ? c * c / (1.0 + s) : 1.0 - s;
                const double pw = plus * w, den = pw + minus;
                const double sin_chi = (pw - minus) / den;
                const double cos_chi = 2.0 * c * sqrt(w) / den;
                const double D = 1.0 + P.sin_chi1 * sin_chi + P.cos_chi1 * cos_chi * cl;
                if (D >= 1.0) {                 // at most 90 degrees from the centre on the conformal sphere
                    const double A = P.k / D;
                    ox = A * cos_chi * sl;
                    oy = A * (P.cos_chi1 * sin_chi - P.sin_chi1 * cos_chi * cl);
                }
            }
        }
        x[i] = ox;
        y[i] = oy;
    }
}

// tan chi of tan phi (Karney eq. 7)
__device__ __forceinline__ double taupf(double tau, double e) {
    const double tau1 = sqrt(1.0 + tau * tau);
    const double sig = sinh(e * atanh(e * tau / tau1));
    return sqrt(1.0 + sig * sig) * tau - sig * tau1;
}

// tan phi of tan chi: Newton's method (Karney eq. 19-21)
__device__ __forceinline__ double tauf(double taup, double e) {
    const double e2m = (1.0 - e) * (1.0 + e);
    double tau = fabs(taup) > 70.0 ? taup * exp(e * atanh(e)) : taup / e2m;
    for (int it = 0; it < 5; ++it) {
        const double taupa = taupf(tau, e);
        const double dtau = (taup - taupa) * (1.0 + e2m * tau * tau) / (e2m * sqrt(1.0 + tau * tau) * sqrt(1.0 + taupa * taupa));
        tau += dtau;
        if (!(fabs(dtau) >= 1.5e-9 * fmax(1.0, fabs(tau)))) break;       // (0.1 sqrt(eps): the next step is below eps)
    }
    return tau;
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void k_project_inverse(proj_dev P, const double* __restrict__ x, const double* __restrict__ y,
                                                            int64_t n, double* __restrict__ lat, double* __restrict__ lon) {
    AMT_GRID_STRIDE(i, n) {
        const double px = x[i], py = y[i];
        double ola = NAN, olo = NAN;
        if (finite(px) && finite(py)) {
            if (KIND == AMT_PROJ_POLAR_AEQD) {
                const double colat = sqrt(px * px + py * py) / P.k * kRad2Deg;
                if (colat <= 180.0) {
                    ola = P.north ? 90.0 - colat : colat - 90.0;
                    // (0.0 - py, py + 0.0: never -0, which would turn the centre's atan2(0, -0) into pi)
                    olo = wrap_lon(P.lon0 + atan2(px, P.north ? 0.0 - py : py + 0.0) * kRad2Deg);
                }
            } else {
                // (1 + u^2) (sin chi, cos chi cos dlon, cos chi sin dlon), u = rho / k = tan(c / 2)  (Snyder 21-15, 20-14, 20-15)
                const double ux = px / P.k, uy = py / P.k;
                const double q = 1.0 - (ux * ux + uy * uy);
                const double ns = q * P.sin_chi1 + 2.0 * uy * P.cos_chi1;
                const double nc = q * P.cos_chi1 - 2.0 * uy * P.sin_chi1;
                const double nx = 2.0 * ux;
                const double h = sqrt(nc * nc + nx * nx);
                if (finite(ns) && finite(h)) {
                    ola = h > 0 ? atan(tauf(ns / h, P.e)) * kRad2Deg : copysign(90.0, ns);
                    olo = wrap_lon(P.lon0 + atan2(nx, nc) * kRad2Deg);
                }
            }
        }
        lat[i] = ola;
        lon[i] = olo;
    }
}

bool projection_ok(const amt_projection* p) {
    if (p == nullptr) return false;
    if (p->kind != AMT_PROJ_STEREOGRAPHIC && p->kind != AMT_PROJ_POLAR_AEQD) return false;
    if (p->mode < -1 || p->mode > 1 || (p->kind == AMT_PROJ_POLAR_AEQD && p->mode == 0)) return false;
    return std::isfinite(p->lon0) && p->e >= 0 && p->e < 1 && p->k > 0 && std::isfinite(p->k) && std::isfinite(p->sin_chi1) &&
           std::isfinite(p->cos_chi1);
}

proj_dev make_proj(const amt_projection* p) {
    proj_dev d;
    d.lon0 = p->lon0;
    d.e = p->e;
    d.sin_chi1 = p->sin_chi1;
    d.cos_chi1 = p->cos_chi1;
    d.k = p->k;
    d.north = p->mode > 0 ? 1 : 0;
    return d;
}

}  // namespace

extern "C" {

int amt_projection_stereographic(double lat0, double lon0, double a, double b, amt_projection* out) {
    return amt_prm::projection_stereographic(lat0, lon0, a, b, out);
}

int amt_projection_polar_aeqd(int north, double lon0, double radius, amt_projection* out) {
    return amt_prm::projection_polar_aeqd(north, lon0, radius, out);
}

int amt_project_forward(amt_ctx* ctx, const amt_projection* p, const double* lat_deg, const double* lon_deg, int64_t n,
                        double* out_x, double* out_y) {
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, projection_ok(p), "not a projection that amt_projection_* filled");
    AMT_REQUIRE(ctx, n >= 0 && (n == 0 || (lat_deg && lon_deg && out_x && out_y)), "NULL argument or negative size");
    if (n == 0) return AMT_OK;
    if (p->kind == AMT_PROJ_POLAR_AEQD)
        hipLaunchKernelGGL(k_project_forward<AMT_PROJ_POLAR_AEQD>, grid_for(n), dim3(kBlock), 0, ctx->stream, make_proj(p), lat_deg,
                           lon_deg, n, out_x, out_y);
    else
        hipLaunchKernelGGL(k_project_forward<AMT_PROJ_STEREOGRAPHIC>, grid_for(n), dim3(kBlock), 0, ctx->stream, make_proj(p),
                           lat_deg, lon_deg, n, out_x, out_y);
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

int amt_project_inverse(amt_ctx* ctx, const amt_projection* p, const double* x, const double* y, int64_t n, double* out_lat_deg,
                        double* out_lon_deg) {
    AMT_CHECK_CTX(ctx);
    AMT_REQUIRE(ctx, projection_ok(p), "not a projection that amt_projection_* filled");
    AMT_REQUIRE(ctx, n >= 0 && (n == 0 || (x && y && out_lat_deg && out_lon_deg)), "NULL argument or negative size");
    if (n == 0) return AMT_OK;
    if (p->kind == AMT_PROJ_POLAR_AEQD)
        hipLaunchKernelGGL(k_project_inverse<AMT_PROJ_POLAR_AEQD>, grid_for(n), dim3(kBlock), 0, ctx->stream, make_proj(p), x, y, n,
                           out_lat_deg, out_lon_deg);
    else
        hipLaunchKernelGGL(k_project_inverse<AMT_PROJ_STEREOGRAPHIC>, grid_for(n), dim3(kBlock), 0, ctx->stream, make_proj(p), x, y,
                           n, out_lat_deg, out_lon_deg);
    AMT_LAUNCH_CHECK(ctx);
    return AMT_OK;
}

}  // extern "C"
