// Per-frame host scalars of the frame pipeline in C++: ephemeris seconds, the cxform rotation matrices J2000 -> GEO and
// J2000 -> SM (with the IGRF dipole), the WCS Euler matrix.  Ports of auromat_amd/coordinates/{transform,wcs,igrf}.py,
// which are pinned to the reference's doubles (tests/golden/host_scalars.npz; reference transform.py:491-696,
// wcs.py:133-139, igrf.py:25-58): the same operations in the same order; products of 3x3 matrices accumulate with fused
// multiply-adds in the order k = 0, 1, 2, which is what the BLAS behind NumPy's `dot` does for these sizes on the build
// host (tests/test_host_cpu.py compares the two: equal to the last bit on the dates tried, and in any case to 4e-16).
// And the host rules on those scalars, each implemented here once for the frame drivers, the sequence runner and (through
// amt_pole_in_view, amt_frames_close, amt_box_hint) Python: the pole test and the sequence coherence behind the box hints;
// tests/test_host_rules_cpu.py compares them with the NumPy restatements of tests/_host_rules.py.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/auromat_hip.h"

namespace amt_prm {

constexpr double kDeg2Rad = 0.017453292519943295;      // np.deg2rad(x) = x * (pi / 180)
constexpr double kPi = 3.141592653589793;
constexpr double kWgs84A = 6378.137, kWgs84B = 6356.752314245179;      // km, reference geodesic.py:20-21

struct m3 {
    double v[9];
};

inline m3 mul(const m3& a, const m3& b) {
    m3 c;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
#ifdef AMT_PRM_NOFMA
            c.v[3 * i + j] = a.v[3 * i] * b.v[j] + a.v[3 * i + 1] * b.v[3 + j] + a.v[3 * i + 2] * b.v[6 + j];
#else
            double acc = a.v[3 * i] * b.v[j];
            acc = std::fma(a.v[3 * i + 1], b.v[3 + j], acc);
            acc = std::fma(a.v[3 * i + 2], b.v[6 + j], acc);
            c.v[3 * i + j] = acc;
#endif
        }
    return c;
}

inline m3 transpose(const m3& a) {
    m3 t;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) t.v[3 * i + j] = a.v[3 * j + i];
    return t;
}

// rotation_matrix(angle, axis)[:3, :3] for the three axis directions that make it agree with cxform's hapgood_matrix
// (transform.py:491-494): X = [-1, 0, 0], Y = [0, 1, 0], Z = [0, 0, -1]
enum axis_id { AX = 0, AY = 1, AZ = 2 };
inline m3 rotation(double angle, axis_id ax) {
    const double s = std::sin(angle), c = std::cos(angle);
    const double d[3] = {ax == AX ? -1.0 : 0.0, ax == AY ? 1.0 : 0.0, ax == AZ ? -1.0 : 0.0};
    const double k = 1.0 - c;
    m3 r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.v[3 * i + j] = (i == j ? c : 0.0) + (d[i] * d[j]) * k;
    const double a0 = d[0] * s, a1 = d[1] * s, a2 = d[2] * s;
    r.v[0] += 0.0, r.v[1] += -a2, r.v[2] += a1;
    r.v[3] += a2, r.v[4] += 0.0, r.v[5] += -a0;
    r.v[6] += -a1, r.v[7] += a0, r.v[8] += 0.0;
    return r;
}

inline double T0(double et) { return (et / 86400.0) / 36525.0; }

inline double H(double et) {
    const double jd = (et / 86400.0) - 0.5;
    double hh = (jd - (double)(long long)jd) * 24.0;
    if (hh < 0.0) hh += 24.0;
    return hh;
}

inline double lambda0(double et) {
    const double M = 357.528 + 35999.050 * T0(et);
    const double lambd = 280.460 + 36000.772 * T0(et);
    return lambd + (1.915 - 0.0048 * T0(et)) * std::sin(M * kDeg2Rad) + 0.020 * std::sin((2 * M) * kDeg2Rad);
}

inline double epsilon(double et) { return 23.439 - 0.013 * T0(et); }

// IGRF g01, g11, h11 for 1900 ... 2020 (nT; igrf.py:25-58 of the reference; the last entry is extrapolated there)
constexpr int kIgrfYears = 25;
constexpr double kG01[kIgrfYears] = {-31543, -31464, -31354, -31212, -31060, -30926, -30805, -30715, -30654, -30594, -30554, -30500,
                                      -30421, -30334, -30220, -30100, -29992, -29873, -29775, -29692, -29619.4, -29554.63, -29496.5,
                                      -29442, -29390.5};
constexpr double kG11[kIgrfYears] = {-2298, -2298, -2297, -2306, -2317, -2318, -2316, -2306, -2292, -2285, -2250, -2215, -2169,
                                      -2119, -2068, -2013, -1956, -1905, -1848, -1784, -1728.2, -1669.05, -1585.9, -1501, -1410.5};
constexpr double kH11[kIgrfYears] = {5922, 5909, 5898, 5875, 5845, 5817, 5808, 5812, 5821, 5810, 5815, 5820, 5791, 5776, 5737,
                                      5675, 5604, 5500, 5406, 5306, 5186.1, 5077.99, 4944.26, 4797.1, 4664.1};

// false when the date is outside the table (the Python side raises ValueError)
inline bool igrf(double et, double* g01, double* g11, double* h11) {
    const double idx = (et + 3155803200.0) / 157788000.0;
    const double frac = std::fmod(idx, 1.0);
    if (!(idx >= 0) || idx >= kIgrfYears - 1) return false;
    const int lo = (int)std::floor(idx), hi = (int)std::ceil(idx);
    *g01 = kG01[lo] * (1.0 - frac) + kG01[hi] * frac;
    *g11 = kG11[lo] * (1.0 - frac) + kG11[hi] * frac;
    *h11 = kH11[lo] * (1.0 - frac) + kH11[hi] * frac;
    return true;
}

inline m3 mat_P(double et) {
    const double t0 = T0(et);
    m3 m = rotation((-1.0 * (0.64062 * t0 + 0.00030 * t0 * t0)) * kDeg2Rad, AZ);
    m = mul(m, rotation((0.55675 * t0 - 0.00012 * t0 * t0) * kDeg2Rad, AY));
    m = mul(m, rotation((-1.0 * (0.64062 * t0 + 0.00008 * t0 * t0)) * kDeg2Rad, AZ));
    return m;
}

inline m3 mat_T1(double et) {
    const double theta = 100.461 + 36000.770 * T0(et) + 360.0 * (H(et) / 24.0);
    return rotation(theta * kDeg2Rad, AZ);
}

inline m3 mat_T2(double et) { return mul(rotation(lambda0(et) * kDeg2Rad, AZ), rotation(epsilon(et) * kDeg2Rad, AX)); }

// J2000 -> GEO (transform.py:683-686)
inline m3 j2000_to_geo(double et) { return mul(mat_T1(et), mat_P(et)); }

// J2000 -> SM (transform.py:688-691); false when the date is outside the IGRF table
inline bool j2000_to_sm(double et, m3* out) {
    double g01, g11, h11;
    if (!igrf(et, &g01, &g11, &h11)) return false;
    const double lon = std::atan2(h11, g11) + kPi;
    const double lat = kPi / 2 - std::atan((g11 * std::cos(lon) + h11 * std::sin(lon)) / g01);
    const double qg[3] = {std::cos(lat) * std::cos(lon), std::cos(lat) * std::sin(lon), std::sin(lat)};
    const m3 t2 = mat_T2(et), t1 = mat_T1(et);
    const m3 a = mul(t2, transpose(t1));
    double qe[3];
    for (int i = 0; i < 3; ++i) {
        double acc = a.v[3 * i] * qg[0];
        acc = std::fma(a.v[3 * i + 1], qg[1], acc);
        acc = std::fma(a.v[3 * i + 2], qg[2], acc);
        qe[i] = acc;
    }
    const double psi = std::atan2(qe[1] * kDeg2Rad, qe[2] * kDeg2Rad);
    const m3 t3 = rotation(-psi, AX);
    const double mu = std::atan2(qe[0] * kDeg2Rad, std::sqrt(qe[1] * qe[1] + qe[2] * qe[2]) * kDeg2Rad);
    const m3 t4 = rotation(-mu, AY);
    *out = mul(mul(mul(t4, t3), t2), mat_P(et));
    return true;
}

// euler_matrix(ai, aj, ak, 'rzxz')[:3, :3] (wcs.py:133-139 -> the vendored transformations.py:1042-1102)
inline m3 euler_rzxz(double ai, double aj, double ak) {
    const double t = ai;
    ai = ak, ak = t;
    const double si = std::sin(ai), sj = std::sin(aj), sk = std::sin(ak);
    const double ci = std::cos(ai), cj = std::cos(aj), ck = std::cos(ak);
    const double cc = ci * ck, cs = ci * sk, sc = si * ck, ss = si * sk;
    m3 m;
    const int i = 2, j = 0, k = 1;
    m.v[3 * i + i] = cj;
    m.v[3 * i + j] = sj * si;
    m.v[3 * i + k] = sj * ci;
    m.v[3 * j + i] = sj * sk;
    m.v[3 * j + j] = -cj * ss + cc;
    m.v[3 * j + k] = -cj * cs - sc;
    m.v[3 * k + i] = -sj * ck;
    m.v[3 * k + j] = cj * sc + cs;
    m.v[3 * k + k] = cj * cc - ss;
    return m;
}

// The whole amt_frame_params block of a frame.  Returns AMT_OK, or AMT_EINVAL (date outside the IGRF table with want_sm).
inline int frame_params(const amt_run_frame* f, int32_t width, int32_t height, int32_t fast_center, double altitude,
                        int want_sm, amt_frame_params* p) {
    std::memset(p, 0, sizeof(*p));
    p->width = width;
    p->height = height;
    p->fast_center = fast_center ? 1 : 0;
    for (int i = 0; i < 4; ++i) p->cd[i] = f->cd[i];
    p->crpix[0] = f->crpix[0];
    p->crpix[1] = f->crpix[1];
    const m3 rot = euler_rzxz((f->crval[0] + 90) * kDeg2Rad, (90 - f->crval[1]) * kDeg2Rad, (-(f->lonpole - 90)) * kDeg2Rad);
    std::memcpy(p->rot, rot.v, sizeof(rot.v));
    for (int i = 0; i < 3; ++i) p->cam[i] = f->cam[i];
    p->a = kWgs84A + altitude;
    p->b = kWgs84B + altitude;
    p->a0 = kWgs84A;
    p->b0 = kWgs84B;
    const double et = (f->jd - 2451545) * 86400;
    const m3 geo = j2000_to_geo(et);
    std::memcpy(p->m_geo, geo.v, sizeof(geo.v));
    if (want_sm) {
        m3 sm;
        if (!j2000_to_sm(et, &sm)) return AMT_EINVAL;
        std::memcpy(p->m_sm, sm.v, sizeof(sm.v));
    }
    return AMT_OK;
}

// ---- host rules on amt_frame_params ---------------------------------------------------------------------------------------

// Is the north (+1) or south (-1) pole of the mapping shell imaged by a valid pixel (0: neither)?  The pole point is
// projected through the inverse TAN model; it counts when it falls inside the frame, is the first hit of its ray and
// lies above the elevation threshold (-inf: none).  Replaces the outline-based test of the reference, geodesic.py:183 /
// mapping.py:705-721, for known camera models.
inline int pole_in_view(const amt_frame_params* p, double min_elevation, int magnetic) {
    const double* m = magnetic ? p->m_sm : p->m_geo;
    const double* r = p->rot;
    const double sc[3] = {1 / p->a, 1 / p->a, 1 / p->b};
    for (int sign = 1; sign >= -1; sign -= 2) {
        double u[3], pole[3], los[3], d[3], n2 = 0;
        for (int i = 0; i < 3; ++i) u[i] = m[6 + i] * sign;              // m^T (0,0,sign): pole axis in J2000
        for (int i = 0; i < 3; ++i) n2 += u[i] * sc[i] * u[i] * sc[i];
        double dist2 = 0;
        for (int i = 0; i < 3; ++i) {
            pole[i] = u[i] / std::sqrt(n2);
            los[i] = pole[i] - p->cam[i];
            dist2 += los[i] * los[i];
        }
        const double dist = std::sqrt(dist2);
        double d_o = 0, d_d = 0, o_o = 0;
        for (int i = 0; i < 3; ++i) {
            d[i] = los[i] / dist;
            const double ds = d[i] * sc[i], os = -p->cam[i] * sc[i];
            d_o += ds * os;
            d_d += ds * ds;
            o_o += os * os;
        }
        const double disc = d_o * d_o - o_o * d_d + d_d;
        if (disc < 0) continue;
        const double t = (o_o < 1 ? d_o + std::sqrt(disc) : d_o - std::sqrt(disc)) / d_d;
        if (std::fabs(t - dist) > 1e-6 * dist) continue;                  // the pole is on the far side
        double v[3];
        for (int i = 0; i < 3; ++i) v[i] = r[i] * d[0] + r[3 + i] * d[1] + r[6 + i] * d[2];   // rot^T d
        if (v[2] <= 0) continue;
        const double k = 180.0 / M_PI, bx = k * v[1] / v[2], by = -k * v[0] / v[2];
        const double det = p->cd[0] * p->cd[3] - p->cd[1] * p->cd[2];
        const double px = (bx * p->cd[3] - p->cd[1] * by) / det, py = (p->cd[0] * by - p->cd[2] * bx) / det;
        const double x = px + p->crpix[0] - 1, y = py + p->crpix[1] - 1;
        if (!(x >= -0.5 && x <= p->width - 0.5 && y >= -0.5 && y <= p->height - 0.5)) continue;
        if (!std::isinf(min_elevation)) {
            double dp = 0, pp = 0;
            for (int i = 0; i < 3; ++i) {
                dp += d[i] * pole[i];
                pp += pole[i] * pole[i];
            }
            double sn = -dp / std::sqrt(pp);
            sn = sn < -1 ? -1 : (sn > 1 ? 1 : sn);
            if (!(std::asin(sn) * k >= min_elevation)) continue;
        }
        return sign;
    }
    return 0;
}

inline bool all_within(const double* a, const double* b, int n, double tol) {
    for (int i = 0; i < n; ++i)
        if (std::fabs(a[i] - b[i]) > tol) return false;
    return true;
}

// Neighbours in a sequence: same frame size, camera model within 1 % in scale (separately solved frames of one sequence
// differ in the sixth digit of their CD matrix) and 5 px in the reference pixel, camera within 100 km, boresight and Earth
// rotation within about half a degree, shell within 30 km — all of which move the box by far less than the superset's margin.
inline bool close_frames(const amt_frame_params& a, const amt_frame_params& b) {
    if (a.width != b.width || a.height != b.height || a.fast_center != b.fast_center) return false;
    if (std::fabs(a.a - b.a) > 30.0 || std::fabs(a.b - b.b) > 30.0) return false;
    double cd_max = 0;
    for (int i = 0; i < 4; ++i) cd_max = std::max(cd_max, std::fabs(a.cd[i]));
    return all_within(a.cam, b.cam, 3, 100.0) && all_within(a.rot, b.rot, 9, 0.01) && all_within(a.m_geo, b.m_geo, 9, 0.01) &&
           all_within(a.m_sm, b.m_sm, 9, 0.01) && all_within(a.cd, b.cd, 4, 0.01 * cd_max) && all_within(a.crpix, b.crpix, 2, 5.0);
}

// Frames a, b (n_ab frames apart) and c (n_bc frames after b) of a steady sequence: same frame size, shell and reference pixel
// as close_frames asks, c within 400 km of b, the same plate scale within 1 %, and CD matrix (it turns with the camera's
// roll: 5e-4 per element over 20 s of the real ISS029 sequence), camera and boresight of c where the pace of a -> b puts them.
inline bool steady_frames(const amt_frame_params& a, const amt_frame_params& b, const amt_frame_params& c, long long n_ab, long long n_bc) {
    if (n_ab <= 0 || n_bc <= 0 || n_bc > 16) return false;
    if (b.width != c.width || b.height != c.height || b.fast_center != c.fast_center) return false;
    if (std::fabs(b.a - c.a) > 30.0 || std::fabs(b.b - c.b) > 30.0) return false;
    if (!(all_within(b.cam, c.cam, 3, 400.0) && all_within(b.rot, c.rot, 9, 0.05) && all_within(b.m_geo, c.m_geo, 9, 0.05) &&
          all_within(b.m_sm, c.m_sm, 9, 0.05) && all_within(b.crpix, c.crpix, 2, 5.0)))
        return false;
    const double scale_b = std::sqrt(std::fabs(b.cd[0] * b.cd[3] - b.cd[1] * b.cd[2]));
    const double scale_c = std::sqrt(std::fabs(c.cd[0] * c.cd[3] - c.cd[1] * c.cd[2]));
    if (!(scale_b > 0 && std::fabs(scale_c - scale_b) <= 0.01 * scale_b)) return false;
    for (int i = 0; i < 4; ++i) {
        const double step = (b.cd[i] - a.cd[i]) / n_ab;
        if (std::fabs((c.cd[i] - b.cd[i]) - step * n_bc) > 0.3 * std::fabs(step * n_bc) + 0.01 * scale_b) return false;
    }
    for (int i = 0; i < 3; ++i) {
        const double step = (b.cam[i] - a.cam[i]) / n_ab;
        if (std::fabs((c.cam[i] - b.cam[i]) - step * n_bc) > 0.2 * std::fabs(step * n_bc) + 5.0) return false;
    }
    for (int i = 0; i < 9; ++i) {
        const double step = (b.rot[i] - a.rot[i]) / n_ab;
        if (std::fabs((c.rot[i] - b.rot[i]) - step * n_bc) > 0.3 * std::fabs(step * n_bc) + 2e-3) return false;
    }
    return true;
}

// Estimate of the box reduction of frame k (parameters p) from the latest frame the single-pass plan finished (its exact
// reduction, parameters and running index) and the one finished before it (prev_box == nullptr: there is none), or false
// (then the coarse pre-pass runs).  The latest frame's box as it is when that frame is a neighbour of this one; else, in a
// steady sequence, the two boxes extrapolated linearly to this frame: a frame is prepared two batches ahead of the latest
// finished one, 20 s of orbit at the ISS's 3 s cadence, which moves the box by more than the superset's margin, but
// smoothly.  A poor estimate costs time (the frame is handed back), never correctness.
inline bool box_hint(const double* last_box, const amt_frame_params& last_p, long long last_index, const double* prev_box,
                     const amt_frame_params* prev_p, long long prev_index, long long k, const amt_frame_params& p, double* est) {
    if (close_frames(last_p, p)) {
        std::memcpy(est, last_box, 8 * sizeof(double));
        return true;
    }
    if (prev_box == nullptr || prev_p == nullptr || !close_frames(*prev_p, last_p) ||
        !steady_frames(*prev_p, last_p, p, last_index - prev_index, k - last_index))
        return false;
    if ((prev_box[7] != 0) != (last_box[7] != 0) || (last_box[3] - last_box[2] > 180) != (prev_box[3] - prev_box[2] > 180))
        return false;                               // a pole or the date line came into view between the two
    const double f = (double)(k - last_index) / (double)(last_index - prev_index);
    for (int i = 0; i < 6; ++i) est[i] = last_box[i] + f * (last_box[i] - prev_box[i]);
    est[6] = last_box[6], est[7] = last_box[7];
    est[0] = std::max(est[0], -90.0), est[1] = std::min(est[1], 90.0);
    for (int i = 2; i < 6; ++i) est[i] = std::min(std::max(est[i], -180.0), 180.0);
    return true;
}

// ---- sky rows a frame's arrays already hold as NaN ----------------------------------------------------------------------------
// The big kernel writes NaN into the rows of work items ("bands", n of them) that cannot see the shell: the frame's sky,
// [0, t) and [b, n).  A slot of the sequence runner takes a new frame every n_slots frames, and what its arrays hold then is
// known: the sky of the frame before is NaN, everything else is data.  `known` says so as [0, top_end) and [bottom_begin, n); a
// bottom_begin beyond n counts as n, so that "nothing known" has one form whatever the number of bands: sky_known_empty().
struct sky_known {
    int top_end, bottom_begin;
};
constexpr int kSkyNoBottom = 0x7fffffff;
inline sky_known sky_known_empty() { return sky_known{0, kSkyNoBottom}; }

// The one rule: which sky bands of a frame still have to be written, [*fill_top_begin, t) and [b, *fill_bottom_end), when
// its arrays hold `known`; returns what they hold after the launch: the frame's own sky (every sky band NaN — written now or
// before —, every other band data).  The two ranges may hold more than is needed (known bottom bands inside a growing top
// range, say), never less: known plus filled covers the sky.  Nothing known gives the fill range (0, n): every sky band is written.
inline sky_known sky_fill(const sky_known& known, int n, int t, int b, int* fill_top_begin, int* fill_bottom_end) {
    const int kt = std::min(std::max(known.top_end, 0), n), kb = std::min(std::max(known.bottom_begin, 0), n);
    *fill_top_begin = std::min(kt, t);
    *fill_bottom_end = std::max(kb, b);
    return sky_known{t, b};
}

// ---- roles of the Earth bands ---------------------------------------------------------------------------------------------------
// The bands between the two sky ranges, [t, b), cast rays.  Most of them need none of the row step's guards, and some need none
// of its binning: a band is
//   inner    when every corner ray and every pixel centre of it hits the shell and every pixel of it lies at or above the
//            elevation threshold — no miss, nothing masked: the kernel's inner loop has no hit test, no threshold test and no
//            keep flags;
//   low      when none of its pixels can reach the threshold — nothing is binned and no corner enters the box: the kernel's low
//            loop reads no image and keeps no runs and no box;
//   generic  otherwise (the limb, the threshold line, and every band of a frame the rule does not decide).
// As ranges of bands: inner [inner_begin, inner_end), low [t, low_top_end) and [low_bottom_begin, b).  Both kinds of region are
// convex in the image of a TAN camera (cones about the nadir), so the inner bands are one range and the low ones lie at the two
// ends of the Earth bands.
struct band_role_ranges {
    int inner_begin, inner_end;
    int low_top_end, low_bottom_begin;
};
// no roles: every Earth band of a frame of n bands is generic
inline band_role_ranges band_roles_none(int n) { return band_role_ranges{0, 0, 0, n}; }

// The one rule, on what the geometry gives for a frame of n bands with Earth bands [t, b): [can_top, can_bottom), outside of
// which no pixel reaches the threshold (elevation_bands(); (0, n) when there is no threshold or no bound), and [in_begin,
// in_end), the bands that are wholly inside the cone of the threshold with a margin (inner_bands(); empty when undecided).
// Whatever the inputs, the ranges it returns are ordered and disjoint and lie inside [t, b): t <= low_top_end <= inner_begin
// <= inner_end <= low_bottom_begin <= b (inner_begin = inner_end = 0 when there is no inner band).
inline band_role_ranges band_roles(int n, int t, int b, int can_top, int can_bottom, int in_begin, int in_end) {
    band_role_ranges r = band_roles_none(n);
    t = std::min(std::max(t, 0), n), b = std::min(std::max(b, t), n);
    r.low_top_end = std::min(std::max(can_top, t), b);
    r.low_bottom_begin = std::min(std::max(can_bottom, r.low_top_end), b);
    const int i0 = std::max(in_begin, r.low_top_end), i1 = std::min(in_end, r.low_bottom_begin);
    if (i0 < i1) r.inner_begin = i0, r.inner_end = i1;
    return r;
}
// bands per role among the Earth bands [t, b): counts[0] generic, [1] inner, [2] low
inline void band_role_counts(const band_role_ranges& r, int t, int b, int* counts) {
    t = std::max(t, 0), b = std::max(b, t);
    counts[1] = r.inner_end - r.inner_begin;
    counts[2] = std::max(0, std::min(r.low_top_end, b) - t) + std::max(0, b - std::max(r.low_bottom_begin, t));
    counts[0] = (b - t) - counts[1] - counts[2];
}

// ---- core bands -------------------------------------------------------------------------------------------------------------------
// An inner band whose two neighbours are inner as well is a CORE band when the frame passes core_frame_ok().  The middle strips of a
// core band (all but the first and the last) are core items: the kernel's core loop leaves out the bounding box, the keep flags
// and the test that sends a corner or a centre to the full arctangents from the second row of an item on.  What has to hold
// for every corner of such an item, its eight neighbours on the pixel lattice included (they lie in inner bands and inside the frame):
//   (a) none of them is an extreme of the box: each has a strictly larger and a strictly smaller neighbour in latitude and in
//       longitude, and the longitudes have one sign (the box keeps the smallest positive and the largest non-positive one);
//   (b) every small-angle step passes: steps far below the 1.7 deg limit, longitudes inside +-178 deg.
// The rule is decided for the whole frame from the cone about the nadir that inner_bands() proves the inner bands to lie in:
// nadir angles up to eta_k = asin(k), k = r_min / |C| cos e0, whose rays hit within the ground angle g_k = 90 deg - e0 - eta_k
// of the sub-satellite point (law of sines on the sphere of radius r_min, which gives the largest angle).  With the
// sub-satellite point at geocentric latitude lat_s and longitude lon_s:
//   latitude    |lat| <= |lat_s| + g_k + 0.5 deg (geodetic against geocentric latitude: 0.2 deg; the shell's flattening) must stay
//               below kCoreMaxLat;
//   longitude   |lon - lon_s| <= dl, sin dl = sin g_k / cos(lat bound) (a cap on the sphere); that range, widened by 1 deg and by
//               one step, must hold neither 0 nor +-180 deg and lie inside +-178 deg;
//   steps       the ground moves by at most gamma'(eta_k) s_hi per pixel (s_lo, s_hi: the smallest and the largest angle a pixel
//               step spans anywhere in the frame, rad), a longitude by 1 / cos(lat bound) of that: below 0.01 rad, a third of the
//               limit of fx::small_angles;
//   (a)         f(x + h) - f(x) = grad f . h + h' H h / 2 on the lattice: among the eight neighbours one has grad f . h >=
//               |grad f| / sqrt 2, its opposite the negative of that, and |h|^2 <= 2, so |grad f| > sqrt 2 |H| is enough.  Along the
//               chain pixel -> ray (TAN plane) -> ground (nadir angle eta -> ground angle gamma(eta), sin(eta + gamma) = R sin eta,
//               R = |C| / r_min) -> angle, per unit of |grad f| on the ground: the gradient is at least s_lo sin gamma / sin eta, the
//               second derivative at most s_hi^2 (2 tan(lat bound) gamma'^2 + 2 gamma'' + 2 gamma') (the curvature of parallels and
//               meridians; the ground map; the TAN plane).  gamma', gamma'' and sin gamma / sin eta grow with eta, so the cone is cut into
//               kCoreRings rings, each with the gradient of its inner and the second derivative of its outer edge, and
//               the rule asks for a factor kCoreFactor (4, where sqrt 2 would do) in every ring.
constexpr double kCoreMaxLat = 75.0;       // degrees
constexpr double kCoreFactor = 4.0;
constexpr int kCoreRings = 8;

struct core_frame {
    double cam_r, r_min;        // |C| and the shell's smaller semi-axis (same unit)
    double e0_deg;              // the elevation the inner cone ends at (inner_bands: threshold + margin)
    double lat_s_deg, lon_s_deg;
    double s_lo, s_hi;          // rad per pixel step
};

inline bool core_frame_ok(const core_frame& f) {
    if (!(f.cam_r > f.r_min) || !(f.r_min > 0) || !(f.s_lo > 0) || !(f.s_hi >= f.s_lo) || !(f.e0_deg > 0 && f.e0_deg < 89.0)) return false;
    if (!std::isfinite(f.lat_s_deg) || !std::isfinite(f.lon_s_deg)) return false;
    const double big_r = f.cam_r / f.r_min;
    const double k = std::cos(f.e0_deg * kDeg2Rad) / big_r;
    if (!(k > 0.0 && k < 1.0)) return false;
    const double eta_k = std::asin(k);
    const double g_k = 90.0 - f.e0_deg - eta_k / kDeg2Rad;
    if (!(g_k > 0)) return false;
    const double lat_hi = std::fabs(f.lat_s_deg) + g_k + 0.5;
    if (!(lat_hi < kCoreMaxLat)) return false;
    const double cos_lat = std::cos(lat_hi * kDeg2Rad), tan_lat = std::tan(lat_hi * kDeg2Rad);
    const double sin_dl = std::sin((g_k + 0.5) * kDeg2Rad) / cos_lat;
    if (!(sin_dl < 1.0)) return false;
    auto slope = [&](double eta) { return big_r * std::cos(eta) / std::cos(std::asin(big_r * std::sin(eta))) - 1.0; };    // gamma'
    auto second = [&](double eta) {                                                                                         // gamma''
        const double a = std::asin(big_r * std::sin(eta)), ca = std::cos(a);
        return big_r * (std::cos(eta) * std::sin(a) * (1.0 + slope(eta)) - std::sin(eta) * ca) / (ca * ca);
    };
    auto across = [&](double eta) {                                                                                         // sin gamma / sin eta
        return eta > 0 ? std::sin(std::asin(big_r * std::sin(eta)) - eta) / std::sin(eta) : big_r - 1.0;
    };
    const double step = slope(eta_k) * f.s_hi / cos_lat;          // rad of longitude per pixel step, at most
    if (!(step < 0.01)) return false;
    // ... and at least 1e-9 rad of ground angle: the box also takes an item's last corner row as its own chain of small angles
    // gives it, some 1e-13 deg from the value the item below stores for the same corner, which must stay far below a lattice step
    if (!(f.s_lo * across(0.0) > 1e-9)) return false;
    const double dl = std::asin(sin_dl) / kDeg2Rad + 1.0 + step / kDeg2Rad;
    const double lo = f.lon_s_deg - dl, hi = f.lon_s_deg + dl;
    if (!(lo > -178.0 && hi < 178.0) || (lo <= 0.0 && hi >= 0.0)) return false;
    for (int i = 0; i < kCoreRings; ++i) {
        const double e_in = eta_k * i / kCoreRings, e_out = eta_k * (i + 1) / kCoreRings;
        const double g1 = slope(e_out), g2 = second(e_out);
        if (!(f.s_lo * across(e_in) > kCoreFactor * f.s_hi * f.s_hi * (2.0 * tan_lat * g1 * g1 + 2.0 * g2 + 2.0 * g1))) return false;
    }
    return true;
}

// the core bands among the inner bands [in_begin, in_end) of a frame that passes: those with an inner band on either side (so
// never the frame's first or last band); (0, 0) when there is none
inline void core_bands(int in_begin, int in_end, bool frame_ok, int* begin, int* end) {
    *begin = *end = 0;
    if (frame_ok && in_end - in_begin >= 3) *begin = in_begin + 1, *end = in_end - 1;
}

// ---- map projections ----------------------------------------------------------------------------------------------------------
// The constants of amt_project_forward / amt_project_inverse (csrc/amt_project.hip), computed once per projection.  Snyder, Map
// Projections - A Working Manual, ch. 21 (stereographic, ellipsoid) and 25 (azimuthal equidistant, polar, sphere).
//
// The conformal latitude chi of the geodetic latitude phi, as its sine and cosine and without tan / atan: with s = sin phi and
// w = ((1 - e s) / (1 + e s))^e
//     sin chi = ((1 + s) w - (1 - s)) / ((1 + s) w + (1 - s)),   cos chi = 2 cos phi sqrt(w) / ((1 + s) w + (1 - s)),
// 1 - s (s >= 0) or 1 + s (s < 0) taken as cos^2 phi / (1 +- s), which keeps its relative accuracy at the poles.  The kernel
// evaluates the same expressions.
inline void conformal_sin_cos(double e, double s, double c, double* sin_chi, double* cos_chi) {
    const double es = e * s;
    const double w = std::exp(e * std::log((1.0 - es) / (1.0 + es)));
    const double plus = s >= 0 ? 1.0 + s : c * c / (1.0 - s);
    const double minus = s >= 0 ? c * c / (1.0 + s) : 1.0 - s;
    const double pw = plus * w, den = pw + minus;
    *sin_chi = (pw - minus) / den;
    *cos_chi = 2.0 * c * std::sqrt(w) / den;
}

constexpr double kPolarLimit = 1e-8;        // degrees: a centre closer than this to a pole takes the polar form

// Stereographic projection of the ellipsoid (a, b) centred on (lat0, lon0), scale 1 at the centre.  With
//     D = 1 + sin chi1 sin chi + cos chi1 cos chi cos dlon
// the plane coordinates are x = k cos chi sin dlon / D, y = k (cos chi1 sin chi - sin chi1 cos chi cos dlon) / D, where
// k = 2 a m1 / cos chi1 (21-27, 21-24, 21-25 with k0 = 1).  The polar form (21-33, 21-30, 21-31) is the same expression with
// sin chi1 = +-1, cos chi1 = 0 and k = 2 a / sqrt((1 + e)^(1 + e) (1 - e)^(1 - e)): cos chi / (1 + sin chi) is Snyder's t.
inline int projection_stereographic(double lat0, double lon0, double a, double b, amt_projection* p) {
    if (p == nullptr) return AMT_EINVAL;
    std::memset(p, 0, sizeof(*p));
    if (!(std::isfinite(lat0) && std::isfinite(lon0) && std::isfinite(a) && std::isfinite(b))) return AMT_EINVAL;
    if (!(std::fabs(lat0) <= 90.0) || !(a > 0) || !(b > 0) || b > a) return AMT_EINVAL;
    const double e = std::sqrt((a - b) * (a + b)) / a;
    p->kind = AMT_PROJ_STEREOGRAPHIC;
    p->lat0 = lat0;
    p->lon0 = lon0;
    p->a = a;
    p->e = e;
    if (90.0 - std::fabs(lat0) < kPolarLimit) {
        p->mode = lat0 > 0 ? 1 : -1;
        p->sin_chi1 = p->mode;
        p->cos_chi1 = 0.0;
        p->m1 = 0.0;
        p->k = 2.0 * a / std::sqrt(std::pow(1.0 + e, 1.0 + e) * std::pow(1.0 - e, 1.0 - e));
        return AMT_OK;
    }
    // (beyond 45 degrees through the colatitude, which is exact in degrees: cos lat0 keeps its relative accuracy up to the pole)
    const double colat = (90.0 - std::fabs(lat0)) * kDeg2Rad;
    const double s1 = std::fabs(lat0) > 45.0 ? std::copysign(std::cos(colat), lat0) : std::sin(lat0 * kDeg2Rad);
    const double c1 = std::fabs(lat0) > 45.0 ? std::sin(colat) : std::cos(lat0 * kDeg2Rad);
    conformal_sin_cos(e, s1, c1, &p->sin_chi1, &p->cos_chi1);
    p->mode = 0;
    p->m1 = c1 / std::sqrt(1.0 - (e * s1) * (e * s1));
    p->k = 2.0 * a * p->m1 / p->cos_chi1;
    return AMT_OK;
}

// Polar azimuthal equidistant projection of a sphere: rho = radius (pi/2 -+ phi), x = rho sin dlon, y = -+rho cos dlon.
inline int projection_polar_aeqd(int north, double lon0, double radius, amt_projection* p) {
    if (p == nullptr) return AMT_EINVAL;
    std::memset(p, 0, sizeof(*p));
    if (!(std::isfinite(lon0) && std::isfinite(radius)) || !(radius > 0)) return AMT_EINVAL;
    p->kind = AMT_PROJ_POLAR_AEQD;
    p->mode = north ? 1 : -1;
    p->lat0 = north ? 90.0 : -90.0;
    p->lon0 = lon0;
    p->a = radius;
    p->e = 0.0;
    p->sin_chi1 = p->mode;
    p->cos_chi1 = 0.0;
    p->m1 = 0.0;
    p->k = radius;
    return AMT_OK;
}

}  // namespace amt_prm
