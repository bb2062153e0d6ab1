// The frame as a grid kernel reads it, and THE rule for which of its pixels count and in which cell: the pixel set that
// resample(method='mean') bins.  Mean, median, quantile and area-weighted binning and their mosaics promise that set; they keep
// it by calling the functions below (amt_bin_tile.h, amt_median.hip, amt_area.hip, and amt_binning.hip's k_hist2d for the
// longitude).  The nearest-neighbour search (amt_nearest.hip) takes the same pixels with a finite longitude and has a cell rule
// of its own.
#pragma once

#include "amt_common.h"

namespace {

using namespace amt;

struct frame_src {
    const double* lat_c;        // pixel centres, height x width
    const double* lon_c;
    const double* elev;         // or NULL
    const uint8_t* mask;        // centre mask (1 = masked), or NULL
    int height, width;
    double min_elev;
    int use_elev_threshold;
    int lon_from_mlt;           // lon_c (and an area frame's corner x) holds MLT hours
    axis_dev ax, ay;
    int lon_wrap;
};

// Fills S from an entry point's arguments and makes the checks every entry point shares.  Returns what is wrong, or NULL.
inline const char* make_frame_src(frame_src* S, const double* lat_c, const double* lon_c, const double* elev,
                                  const uint8_t* center_mask, int32_t height, int32_t width, double min_elevation,
                                  const amt_axis* xaxis, const amt_axis* yaxis, int lon_wrap, int lon_from_mlt) {
    if (!(lat_c && lon_c && xaxis && yaxis)) return "NULL argument";
    if (!(height > 0 && width > 0)) return "empty frame";
    if (!(axis_ok(xaxis) && axis_ok(yaxis))) return "bad axis";
    S->lat_c = lat_c;
    S->lon_c = lon_c;
    S->elev = elev;
    S->mask = center_mask;
    S->height = height;
    S->width = width;
    S->min_elev = min_elevation;
    // no elevations, or a threshold of -inf: every elevation passes, NaN included (mapping.py:856 is not applied)
    S->use_elev_threshold = (elev != nullptr) && !(std::isinf(min_elevation) && min_elevation < 0);
    S->lon_from_mlt = lon_from_mlt ? 1 : 0;
    make_axis(xaxis, &S->ax);
    make_axis(yaxis, &S->ay);
    S->lon_wrap = lon_wrap ? 1 : 0;
    return nullptr;
}

// The x a longitude is binned at: SM longitude from MLT hours as convertMappingToSM computes it (mltToSmLon), then the shift by
// 180 deg of a frame on the date line.  Every operation rounded on its own.
__device__ __forceinline__ double src_x(int lon_from_mlt, int lon_wrap, double lo) {
#pragma clang fp contract(off)
    if (lon_from_mlt) {
        const double d = lo - 12.0;
        lo = d / kMltPerDeg;
    }
    return lon_wrap ? wrap180_shifted(lo) : lo;
}
__device__ __forceinline__ double src_x(const frame_src& S, double lo) { return src_x(S.lon_from_mlt, S.lon_wrap, lo); }

// Does a pixel count?  A finite latitude (resample.py:315-321), an elevation at or above the threshold (mapping.py:856; NaN
// fails) and centre mask 0.  la, ev, mk: the pixel's latitude, elevation (any value without a threshold) and mask byte.
__device__ __forceinline__ bool src_keeps(const frame_src& S, double la, double ev, unsigned mk) {
    bool ok = finite(la);
    if (S.use_elev_threshold) ok = ok && (ev >= S.min_elev);
    return ok && mk == 0;
}

// The 1-based bins of a pixel that counts, at latitude la and x = src_x(longitude), by histogram2d's rules (bin_index); false
// outside the edges.
__device__ __forceinline__ bool src_cell(const frame_src& S, double la, double x, int& bx, int& by) {
    bx = bin_index(S.ax, x);
    by = bin_index(S.ay, la);
    return bx >= 1 && bx <= S.ax.nbin && by >= 1 && by <= S.ay.nbin;
}

// The same for pixel i of the frame's arrays: does it count, and its latitude and x.  (A pixel without a latitude — the sky
// above the limb — is left before anything else of it is read; src_keeps decides.)
__device__ __forceinline__ bool src_pixel(const frame_src& S, int64_t i, double& la, double& x) {
    la = S.lat_c[i];
    if (!(la == la)) return false;
    const double ev = S.use_elev_threshold ? S.elev[i] : 0.0;
    const unsigned mk = S.mask ? S.mask[i] : 0u;
    if (!src_keeps(S, la, ev, mk)) return false;
    x = src_x(S, S.lon_c[i]);
    return true;
}
__device__ __forceinline__ bool pixel_cell(const frame_src& S, int64_t i, int& bx, int& by) {
    double la, x;
    return src_pixel(S, i, la, x) && src_cell(S, la, x, bx, by);
}

}  // namespace
