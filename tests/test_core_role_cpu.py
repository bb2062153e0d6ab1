"""
The host rule of the core bands (amt_georef_core_bands: amt_prm::core_frame_ok / core_bands on top of amt_georef_band_roles; no GPU)
against oracle/ref_numpy.py on every pixel.  A core item — a middle strip of a core band — leaves out the bounding box, the keep
flags and the test that sends a small-angle step to the full arctangents (k_georef_rows, kRoleCore).  That is sound when, for
every corner of the item (rows r0 .. r1 of the band, the strip's 64 corner columns):

  * its four pixels are valid (they hit and lie at or above the threshold);
  * among its eight neighbours on the corner lattice one is strictly larger and one strictly smaller, in latitude and in longitude:
    it is no extreme of the box;
  * every small-angle step of its chain — corner to the corner below, corner to the centre above it — stays below 1 deg in both
    angles (the kernel's limit is atan(0.03) = 1.718 deg; the gap covers any rounding between the oracle and the kernel);
  * every longitude lies inside +-178 deg, with one sign throughout the band's core items.

The rule may name a band core only where all of that holds, and must name none where the date line, the prime meridian or 80 - 89
deg of latitude lie inside the frame or within a row of it.  What it gives away (bands the oracle would allow) is printed.

Cameras: the bench frames 0, 100 and 196 at three tenths of their size, every camera of tests/_band_role_sweep.py at its thresholds,
and nadir cameras of 200 x 96 pixels (6 bands, 4 strips) at 0.01 deg / px moved across the three lines.
"""
import ctypes

import numpy as np
import pytest

import _band_role_sweep as S
import _camera_cases as K
import _camera_oracle as Q

ROWS = S.ROWS
STEP_LIMIT = 1.0            # degrees


def core_bands(params, thr):
    from auromat_amd import _native
    c2 = (ctypes.c_int32 * 2)()
    assert _native.lib().amt_georef_core_bands(ctypes.byref(params), float(thr), c2) == 0
    return int(c2[0]), int(c2[1])


def roles_of(params, thr):
    from auromat_amd import _native
    rows = ctypes.c_int32(0)
    r = (ctypes.c_int32 * 8)()
    assert _native.lib().amt_georef_band_roles(ctypes.byref(params), float(thr), ctypes.byref(rows), r) == 0
    assert rows.value == ROWS
    return list(r)


def core_strips(w):
    """corner-column ranges [x0, x0 + 64) of the strips whose items may be core: s >= 1 with 63 (s + 1) < w"""
    return [(63 * s, 63 * s + 64) for s in range(1, max((w - 1) // 63, 1))]


class Frame(object):
    """what the checks need of a frame's oracle arrays, computed once"""

    def __init__(self, arrays, w, h):
        self.w, self.h = w, h
        lat, lon = np.asarray(arrays['lat'], np.float64), np.asarray(arrays['lon'], np.float64)
        self.lat, self.lon = lat, lon
        self.lat_c, self.lon_c = np.asarray(arrays['lat_c'], np.float64), np.asarray(arrays['lon_c'], np.float64)
        self.elev = np.asarray(arrays['elev'], np.float64)
        self.no_extreme = np.zeros(lat.shape, bool)
        with np.errstate(invalid='ignore'):
            ok = np.ones((h - 1, w - 1), bool)
            for a in (lat, lon):
                mid = a[1:-1, 1:-1]
                larger, smaller = np.zeros(mid.shape, bool), np.zeros(mid.shape, bool)
                for dy in (0, 1, 2):
                    for dx in (0, 1, 2):
                        if (dy, dx) != (1, 1):
                            nb = a[dy:dy + h - 1, dx:dx + w - 1]
                            larger |= nb > mid
                            smaller |= nb < mid
                ok &= larger & smaller
            self.no_extreme[1:-1, 1:-1] = ok
            # steps: corner (r, x) from corner (r - 1, x); centre (r - 1, x) from corner (r, x)
            self.step_down = np.full(lat.shape, np.inf)
            self.step_down[1:] = np.maximum(np.abs(lat[1:] - lat[:-1]), np.abs(lon[1:] - lon[:-1]))
            self.step_centre = np.full(lat.shape, np.inf)
            self.step_centre[1:, :-1] = np.maximum(np.abs(self.lat_c - lat[1:, :-1]), np.abs(self.lon_c - lon[1:, :-1]))
        self.step_down[np.isnan(self.step_down)] = np.inf
        self.step_centre[np.isnan(self.step_centre)] = np.inf

    def valid(self, thr):
        with np.errstate(invalid='ignore'):
            v = ~np.isnan(self.lat_c) & ~np.isnan(self.elev)
            return v & (self.elev >= thr) if thr == thr else np.zeros_like(v)

    def band_faults(self, k, thr):
        """the properties a core band k must have, as a list of what fails (empty: the oracle allows it)"""
        h, w = self.h, self.w
        r0, r1 = k * ROWS, min((k + 1) * ROWS, h)
        if r0 < 1 or r1 + 1 > h:
            return ['first or last band']
        # (a frame too narrow for a middle strip has no core item whatever the rule says: its bands are held to the same
        # properties on all the corner columns that have a pixel on either side)
        strips = core_strips(w) or [(1, w)]
        valid = self.valid(thr)
        faults = []
        signs = set()
        for x0, x1 in strips:
            rows, cols = slice(r0, r1 + 1), slice(x0, x1)
            four = valid[r0 - 1:r1, x0 - 1:x1 - 1] & valid[r0 - 1:r1, x0:x1] & valid[r0:r1 + 1, x0 - 1:x1 - 1] & valid[r0:r1 + 1, x0:x1]
            if not four.all():
                faults.append('a corner lacks a valid pixel')
            if not self.no_extreme[rows, cols].all():
                faults.append('a corner is an extreme of latitude or longitude among its neighbours')
            if not (self.step_down[r0 + 1:r1 + 1, cols] < STEP_LIMIT).all():
                faults.append('a corner step of %g deg or more' % STEP_LIMIT)
            if not (self.step_centre[r0 + 1:r1 + 1, x0:x1 - 1] < STEP_LIMIT).all():
                faults.append('a centre step of %g deg or more' % STEP_LIMIT)
            lo = np.concatenate([self.lon[rows, cols].ravel(), self.lon_c[r0:r1, x0:x1 - 1].ravel()])
            if not (np.abs(lo) < 178.0).all():
                faults.append('a longitude beyond 178 deg')
            signs.update(np.sign(lo).tolist())
        if len(signs) != 1 or 0.0 in signs:
            faults.append('longitudes of both signs')
        return sorted(set(faults))


def check_frame(tag, params, frame, thr, must_decline=False):
    """-> (core bands named, bands the oracle allows as core that the rule leaves inner)"""
    r = roles_of(params, thr)
    n, in0, in1 = r[0], r[6], r[7]
    cb, ce = core_bands(params, thr)
    assert (cb, ce) == (0, 0) or (in0 < cb < ce < in1), (tag, thr, 'core bands outside the inner ones', (cb, ce), (in0, in1))
    assert (cb, ce) == (0, 0) or (cb >= 1 and ce <= n - 1), (tag, thr, (cb, ce), n)
    if must_decline:
        assert (cb, ce) == (0, 0), (tag, thr, 'the rule must decline', (cb, ce))
    for k in range(cb, ce):
        faults = frame.band_faults(k, thr)
        assert not faults, (tag, thr, 'band', k, faults)
    lost = 0
    if thr == thr and np.isfinite(thr):
        for k in range(in0 + 1, in1 - 1):
            if not (cb <= k < ce) and not frame.band_faults(k, thr):
                lost += 1
    return ce - cb, lost


# ---- the bench frames ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [0, 100, 196])
def test_bench_frames(k):
    from auromat_amd.coordinates import transform as T
    from auromat_amd.mapping.astrometry import frame_params
    from auromat_amd.synthetic import sequence_frame
    from oracle import ref_numpy as O
    w, h = 1272, 850          # (three tenths of the size: at a quarter the rule's plate-scale gate declines)
    hdr, cam, t, _ = sequence_frame(k, w, h)
    et = T.date2es(t)
    ref = O.georef_frame(hdr, 110, cam, O.mat_j2000_to_geo(et), O.mat_j2000_to_sm(et), fast=True)
    frame = Frame(ref, w, h)
    p = frame_params(hdr, 110, cam, t, True)
    for thr in (10.0, 30.0, 0.0, float('-inf'), float('nan')):
        named, lost = check_frame('bench frame %d' % k, p, frame, thr, must_decline=not np.isfinite(thr))
        print('bench frame %d at %dx%d, threshold %r: %d core bands, %d more the oracle allows' % (k, w, h, thr, named, lost))
        if thr == 10.0:
            assert named > 0, 'the bench threshold names no core band'
    # the full-size frame takes the same decision for more bands (no oracle at that size: the rule is the one checked above)
    hdr, cam, t, _ = sequence_frame(k)
    cb, ce = core_bands(frame_params(hdr, 110, cam, t, True), 10.0)
    assert ce - cb >= 70, (cb, ce)


# ---- the cameras at the margins of the band roles -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', S.names())
def test_sweep_cameras(name):
    c = S.by_name(name)
    frame = Frame(S.f64(name), c['width'], c['height'])
    p = K.native_params(c)
    out = []
    for thr in S.tested_thresholds(c):
        named, lost = check_frame(name, p, frame, thr, must_decline=not np.isfinite(thr))
        out.append('%r: %d core, %d lost' % (thr, named, lost))
    print(name, '  '.join(out))


# ---- cameras aimed at the lines the rule must keep out ------------------------------------------------------------------------------
W, H, SCALE, THR = 200, 96, 0.01, 10.0
# one pixel on the ground: 290 km * 0.01 deg = 50 m, 0.0007 deg of longitude at 49 deg of latitude; the frame spans 0.14 x 0.04 deg.
# Offsets of the camera's longitude from the line: on it, inside a would-be core band, at the frame's edge, one row outside
# (0.5 px beyond the half height or half width), and well outside but within the rule's margin
LINE_OFFSETS = (0.0, 0.004, -0.004, 0.0168, -0.0168, 0.0345, -0.0345, 0.0705, -0.0705, 0.3, -0.3)
_AIMED = {}


def aimed(kind, off, roll):
    key = (kind, off, roll)
    if key not in _AIMED:
        if kind == 'meridian':
            lat, lon = 49.0, off
        elif kind == 'dateline':
            lat, lon = 49.0, (180.0 + off if off < 0 else -180.0 + off) if off != 0.0 else 180.0
        else:
            lat, lon = float(kind) + off, 60.0        # (far from both lines: the cone spans +-21 deg of longitude at 49 deg)
        c = K.finish(K.camera('core-%s%+g-roll%g' % key, 'core', W, H, lat=lat, lon=lon, height=400.0, nadir_angle=0.0,
                              scale=SCALE, roll=roll))
        _AIMED[key] = (c, Frame(Q.float64_oracle(c), W, H))
    return _AIMED[key]


def test_nadir_camera_has_core_items():
    c, frame = aimed('49', 0.0, 0.0)
    named, lost = check_frame(c['name'], K.native_params(c), frame, THR)
    assert core_bands(K.native_params(c), THR) == (1, 5), core_bands(K.native_params(c), THR)
    assert len(core_strips(W)) == 2 and lost == 0
    for thr in (float('nan'), float('-inf'), float('inf')):
        assert core_bands(K.native_params(c), thr) == (0, 0), thr


@pytest.mark.parametrize('roll', [0.0, 90.0])
@pytest.mark.parametrize('kind', ['meridian', 'dateline'])
def test_lines_of_longitude(kind, roll):
    allowed = 0
    for off in LINE_OFFSETS:
        c, frame = aimed(kind, off, roll)
        named, lost = check_frame(c['name'], K.native_params(c), frame, THR, must_decline=True)
        allowed += lost
    print('%s, roll %g: the oracle would allow %d bands in %d frames the rule declines' % (kind, roll, allowed, len(LINE_OFFSETS)))


@pytest.mark.parametrize('lat', [80, 83, 86, 88, 89])
def test_high_latitudes(lat):
    allowed = 0
    for sign in (1.0, -1.0):
        for off in (0.0, 0.0168, 0.3):
            c, frame = aimed(repr(sign * lat), sign * off, 0.0)
            named, lost = check_frame(c['name'], K.native_params(c), frame, THR, must_decline=True)
            allowed += lost
    print('latitude %d: the oracle would allow %d bands in 6 frames the rule declines' % (lat, allowed))


def test_latitude_bound_is_where_the_rule_says():
    """the frame-wide bound: sub-satellite latitude + the cone's ground angle (9.6 deg at 10 deg from 400 km) + 0.5 < 75 deg"""
    inside, _ = aimed('60', 0.0, 0.0)
    outside, _ = aimed('66', 0.0, 0.0)
    assert core_bands(K.native_params(inside), THR) != (0, 0)
    assert core_bands(K.native_params(outside), THR) == (0, 0)


# ---- oblique cameras the rule accepts, up to its own plate-scale gate ---------------------------------------------------------------
def oblique(lat, nadir_angle, azimuth, roll, scale, w=330, h=200):
    name = 'core-oblique-%g-%g-%g-%g-%g' % (lat, nadir_angle, azimuth, roll, scale)
    return K.finish(K.camera(name, 'core', w, h, lat=lat, lon=60.0, height=400.0, nadir_angle=nadir_angle, azimuth=azimuth,
                             scale=scale, roll=roll))


@pytest.mark.parametrize('lat', [49.0, -40.0, 62.0])
def test_oblique_cameras(lat):
    """from the nadir to the threshold line (10 deg of elevation lies 70.5 deg from the nadir): 6 strips, 13 bands"""
    named_total = lost_total = frames = 0
    for nadir_angle in (0.0, 35.0, 60.0, 68.0):
        for azimuth in (0.0, 90.0, 225.0):
            for roll in (0.0, 37.0):
                c = oblique(lat, nadir_angle, azimuth, roll, 0.02)
                named, lost = check_frame(c['name'], K.native_params(c), Frame(Q.float64_oracle(c), c['width'], c['height']), THR)
                named_total += named
                lost_total += lost
                frames += 1
    print('latitude %g: %d core bands in %d frames, %d more the oracle allows' % (lat, named_total, frames, lost_total))
    assert named_total >= 4 * frames, named_total


@pytest.mark.parametrize('nadir_angle', [0.0, 60.0, 68.0])
def test_at_the_plate_scale_gate(nadir_angle):
    """the coarsest pixels the rule accepts for this camera (bisection on the rule itself): the properties hold there too, and
    the scale at which the oracle first shows a lattice extreme is printed beside it"""
    def names(scale):
        c = oblique(49.0, nadir_angle, 90.0, 37.0, scale)
        return c, core_bands(K.native_params(c), THR) != (0, 0)
    lo, hi = 0.005, 1.0
    assert names(lo)[1] and not names(hi)[1]
    for _ in range(12):
        mid = np.sqrt(lo * hi)
        lo, hi = (mid, hi) if names(mid)[1] else (lo, mid)
    c, ok = names(lo)
    assert ok
    named, lost = check_frame(c['name'], K.native_params(c), Frame(Q.float64_oracle(c), c['width'], c['height']), THR)
    assert named > 0
    print('nadir angle %g: the rule accepts up to %.4f deg / px (%d core bands there)' % (nadir_angle, lo, named))
