"""
The library's host rules (no GPU): amt_pole_in_view, amt_frames_close and amt_box_hint (csrc/amt_params.h) against the
Python restatements of tests/_host_rules.py, and the box -> range -> grid helpers of csrc/amt_grid.h (amt_gl::range_of_box,
layout_of_box) against bounding_box_from_reduction + wrap_at_180 + _Grid.
"""
import copy
import ctypes as C
import glob
import os
import subprocess
from datetime import datetime

import numpy as np
import pytest

import _host_rules as R
from conftest import GOLDEN, ROOT, header_from, load_golden

NEG_INF = float('-inf')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from auromat_amd import _native
    return _native.lib()


def params_of(hdr, cam, t, altitude=110, fast=True):
    from auromat_amd.mapping.astrometry import frame_params
    return frame_params(hdr, altitude, cam, t, fast, magnetic=True)


def real_headers():
    from auromat_amd.fits import getSpacecraftPosition, readHeader
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, 'resources', 'seq', '*.wcs'))):
        hdr = readHeader(path)
        cam, t = getSpacecraftPosition(hdr)
        out.append((hdr, cam, t))
    assert len(out) == 10
    return out


def test_retry_threshold_has_the_headers_value():
    import re
    from auromat_amd import _native
    with open(os.path.join(ROOT, 'include', 'auromat_hip.h')) as fp:
        assert _native.PIPE_MAX_EDGE_PIXELS == int(re.search(r'#define AMT_PIPE_MAX_EDGE_PIXELS (\d+)', fp.read()).group(1))


# ---- the pole test -------------------------------------------------------------------------------------------------------

def pole_frames():
    import test_sky_rows
    from auromat_amd.synthetic import pole_frame, random_sequence
    frames = [tuple(c[1:4]) for c in test_sky_rows.cases()]
    assert len(frames) == 17
    frames += [pole_frame(400, 320, south=south) for south in (False, True)]
    frames += [f[:3] for f in random_sequence(np.random.RandomState(1), 400, 320, 40)]
    for name in ('north_fast', 'north_exact', 'south_fast', 'south_exact', 'magnetic_fast', 'magnetic_exact'):
        z = load_golden('pole_frame_%s.npz' % name)
        frames.append((header_from(z), z['cam'], datetime.strptime(str(z['time_iso']), '%Y-%m-%dT%H:%M:%S.%f')))
    return frames + real_headers()


def test_pole_in_view_equals_the_numpy_restatement(lib):
    """Equal return value, sign included, for every frame, shell, threshold and grid kind; and the set of cases is not
    one-sided: north, south and no pole on the geodetic side, a pole and none on the magnetic side, and the elevation
    threshold crossed in both directions."""
    from auromat_amd.mapping.astrometry import pole_in_view
    seen = {False: set(), True: set()}
    crossed = set()
    n = 0
    for hdr, cam, t in pole_frames():
        for altitude in (110, 300):
            p = params_of(hdr, cam, t, altitude)
            for magnetic in (False, True):
                by_threshold = []
                for min_elevation in (None, 0, 10, 45):
                    want = R.pole_in_view(p, min_elevation, magnetic)
                    got = lib.amt_pole_in_view(C.byref(p), NEG_INF if min_elevation is None else float(min_elevation), int(magnetic))
                    assert got == want, (hdr, altitude, min_elevation, magnetic, got, want)
                    assert pole_in_view(p, min_elevation, magnetic) == want
                    seen[magnetic].add(want)
                    by_threshold.append(want)
                    n += 1
                if by_threshold[0] != 0 and by_threshold[-1] == 0:
                    crossed.add(by_threshold[0])
    assert n >= 8 * 2 * 60
    assert seen[False] == {1, -1, 0}, seen
    assert 0 in seen[True] and seen[True] & {1, -1}, seen
    assert crossed == {1, -1}, crossed
    assert lib.amt_pole_in_view(None, NEG_INF, 0) == 0


# ---- sequence coherence: neighbours, steadiness, the extrapolated box -------------------------------------------------------

def lib_close(lib, a, b):
    return bool(lib.amt_frames_close(C.byref(a), C.byref(b)))


def lib_box_hint(lib, last, prev, k, p):
    d8 = C.c_double * 8
    est = d8()
    rc = lib.amt_box_hint(d8(*last[0]), C.byref(last[1]), last[2], d8(*prev[0]) if prev else None,
                          C.byref(prev[1]) if prev else None, prev[2] if prev else 0, k, C.byref(p), est)
    return list(est) if rc else None


def check_box_hint(lib, last, prev, k, p, expect):
    """Same yes / no as the restatement (and as `expect`), the estimate equal to 1e-9 deg."""
    want = R.box_hint(last, prev, k, p)
    got = lib_box_hint(lib, last, prev, k, p) if last is not None else None
    assert (want is not None) == expect, (want, expect)
    assert (got is not None) == expect, (got, expect)
    if expect:
        # (slots 4 / 5 of a box that does not straddle are +-inf: their extrapolation is NaN in both)
        g, w = np.array(got[:6]), np.array(want[:6])
        assert np.array_equal(got[6:], want[6:]) and np.array_equal(np.isnan(g), np.isnan(w)), (got, want)
        with np.errstate(invalid='ignore'):
            assert np.all((g == w) | np.isnan(w) | (np.abs(g - w) <= 1e-9)), (got, want)
    return got


def poke(p, field, index, delta):
    q = copy.deepcopy(p)
    if index is None:
        setattr(q, field, getattr(q, field) + delta)
    else:
        getattr(q, field)[index] += delta
    return q


def test_frames_close_equals_the_restatement(lib):
    from auromat_amd.synthetic import sequence_frame
    ps = [params_of(*f) for f in real_headers()]
    for a in ps:
        for b in ps:
            assert lib_close(lib, a, b) == R.close(a, b)
    # neighbouring real frames are neighbours for the box hints too, frames 20 s apart are not
    assert all(lib_close(lib, a, b) for a, b in zip(ps, ps[1:])) and lib_close(lib, ps[0], ps[3]) and not lib_close(lib, ps[0], ps[7])
    qs = [params_of(*sequence_frame(k, 424, 283)[:3]) for k in (0, 1, 2, 5, 12, 13, 14, 20, 40, 299)]
    answers = set()
    for a in qs:
        for b in qs:
            assert lib_close(lib, a, b) == R.close(a, b)
            answers.add(R.close(a, b))
    assert answers == {True, False}
    # every comparison, inside (0.9 x) and outside (1.1 x) its tolerance
    p = qs[0]
    cd_tol = 0.01 * max(abs(v) for v in p.cd)
    for field, index, tol in [('cam', 0, 100.0), ('cam', 2, 100.0), ('rot', 0, 0.01), ('rot', 8, 0.01), ('m_geo', 4, 0.01),
                              ('m_sm', 7, 0.01), ('cd', 1, cd_tol), ('cd', 3, cd_tol), ('crpix', 0, 5.0), ('crpix', 1, 5.0),
                              ('a', None, 30.0), ('b', None, 30.0)]:
        for sign in (1, -1):
            inside, outside = poke(p, field, index, sign * 0.9 * tol), poke(p, field, index, sign * 1.1 * tol)
            assert R.close(p, inside) and lib_close(lib, p, inside), (field, index)
            assert not R.close(p, outside) and not lib_close(lib, p, outside), (field, index)
            assert lib_close(lib, inside, p) == R.close(inside, p) and lib_close(lib, outside, p) == R.close(outside, p)
    for field in ('width', 'height', 'fast_center'):
        q = poke(p, field, None, 1)
        assert not R.close(p, q) and not lib_close(lib, p, q)
    assert not lib.amt_frames_close(None, C.byref(p))


def paced(a, b, n_ab, n_bc):
    """The frame n_bc frames after b when camera, pointing and CD matrix keep the pace of a -> b (n_ab frames)."""
    c = copy.deepcopy(b)
    for field in ('cam', 'rot', 'cd'):
        x, y, z = getattr(a, field), getattr(b, field), getattr(c, field)
        for i in range(len(z)):
            z[i] = y[i] + (y[i] - x[i]) / n_ab * n_bc
    return c


BOX_A = [40.0, 52.0, -101.0, -80.0, float('inf'), -80.0, 1000.0, 0.0]
BOX_B = [40.5, 52.25, -100.0, -79.5, float('inf'), -79.5, 1100.0, 0.0]


def test_box_hint_tolerances_of_the_steady_test(lib):
    """amt_box_hint where the latest frame is NOT a neighbour of the new one, so that the answer is the steadiness test's:
    one perturbation inside and one outside each of its tolerances."""
    from auromat_amd.synthetic import sequence_frame
    a = params_of(*sequence_frame(0, 424, 283)[:3])
    b = poke(a, 'cam', 0, 30.0)                     # 30 km per frame: neighbours
    assert R.close(a, b)

    def ask(c, n_bc, expect, n_ab=1, a_=a, b_=b):
        assert not R.close(b_, c) or not expect
        return check_box_hint(lib, (BOX_B, b_, n_ab), (BOX_A, a_, 0), n_ab + n_bc, c, expect)

    base = paced(a, b, 1, 5)                        # 150 km after b
    est = ask(base, 5, True)
    assert abs(est[0] - (40.5 + 5 * 0.5)) < 1e-9 and abs(est[2] - (-100.0 + 5 * 1.0)) < 1e-9 and est[6:] == BOX_B[6:]
    scale = abs(b.cd[0] * b.cd[3] - b.cd[1] * b.cd[2]) ** 0.5
    # (field, index, tolerance): the new frame against the pace of a -> b, and against b
    for field, index, tol in [('cam', 1, 5.0), ('cam', 0, 0.2 * 150 + 5.0), ('rot', 3, 2e-3), ('m_geo', 0, 0.05), ('m_sm', 5, 0.05),
                              ('crpix', 0, 5.0), ('crpix', 1, 5.0), ('a', None, 30.0), ('b', None, 30.0), ('cd', 1, 0.01 * scale)]:
        for sign in (1, -1):
            ask(poke(base, field, index, sign * 0.9 * tol), 5, True)
            ask(poke(base, field, index, sign * 1.1 * tol), 5, False)
    # the plate scale within 1 %
    for factor, expect in ((1.009, True), (1.011, False), (0.991, True), (0.989, False)):
        c = copy.deepcopy(base)
        for i in range(4):
            c.cd[i] *= factor
        ask(c, 5, expect)
    # the paced terms: 30 % of the step of rot and cd
    b_rot = poke(b, 'rot', 3, 0.002)
    c = paced(a, b_rot, 1, 5)
    for f, expect in ((0.9, True), (1.1, False)):
        ask(poke(c, 'rot', 3, f * (0.3 * 0.010 + 2e-3)), 5, expect, b_=b_rot)
    b_cd = poke(b, 'cd', 1, 0.004 * scale)
    c = paced(a, b_cd, 1, 5)
    for f, expect in ((0.9, True), (1.1, False)):
        ask(poke(c, 'cd', 1, f * (0.3 * 0.020 * scale + 0.01 * scale)), 5, expect, b_=b_cd)
    # the new frame within 400 km of b, pointing within 0.05
    for step, expect in ((22.5, True), (27.5, False)):
        b2 = poke(a, 'cam', 0, step)
        ask(paced(a, b2, 1, 16), 16, expect, b_=b2)
    b_rot = poke(b, 'rot', 0, 0.005)
    for n_bc, expect in ((9, True), (11, False)):
        ask(paced(a, b_rot, 1, n_bc), n_bc, expect, b_=b_rot)
    # at most 16 frames ahead; the two records must be different frames; the frame's size and centre rule
    b2 = poke(a, 'cam', 0, 20.0)
    ask(paced(a, b2, 1, 16), 16, True, b_=b2)
    ask(paced(a, b2, 1, 17), 17, False, b_=b2)
    ask(base, 5, False, n_ab=0)
    for field in ('width', 'height', 'fast_center'):
        ask(poke(base, field, None, 1), 5, False)
    # the two records must be neighbours of each other
    far = poke(a, 'cam', 0, 110.0)
    ask(paced(a, far, 1, 3), 3, False, b_=far)


def test_box_hint_scenarios(lib):
    from auromat_amd.synthetic import sequence_frame
    frame = lambda k: params_of(*sequence_frame(k, 424, 283)[:3])
    box = lambda k: [40.0 + 0.05 * k, 52.0 + 0.04 * k, -101.0 + 0.11 * k, -80.0 + 0.12 * k, float('inf'), -80.0 + 0.12 * k, 1000.0 + k, 0.0]
    # nothing finished yet
    check_box_hint(lib, None, None, 3, frame(3), False)
    # the latest finished frame only, and it is a neighbour: its box as it is
    got = check_box_hint(lib, (box(0), frame(0), 0), None, 7, frame(7), True)
    assert got == box(0)
    check_box_hint(lib, (box(0), frame(0), 0), None, 20, frame(20), False)          # 150 km away: not a neighbour, no second record
    # a neighbour wins over the extrapolation
    got = check_box_hint(lib, (box(1), frame(1), 1), (box(0), frame(0), 0), 8, frame(8), True)
    assert got == box(1)
    # two records, steady, at the 1 s cadence (7.66 km per frame: frames 14-16 ahead are no neighbours) ...
    for k in (15, 16, 17):
        got = check_box_hint(lib, (box(1), frame(1), 1), (box(0), frame(0), 0), k, frame(k), True)
        assert np.max(np.abs(np.array(got[:4]) - np.array(box(k)[:4]))) < 1e-9 and np.isnan(got[4]) and got[6:] == box(1)[6:]
    check_box_hint(lib, (box(1), frame(1), 1), (box(0), frame(0), 0), 18, frame(18), False)
    # ... and at the 3 s cadence of the real sequences: records three sequence frames apart, six to seven frames ahead
    for j in (8, 9, 10):
        got = check_box_hint(lib, (box(6), frame(6), 2), (box(3), frame(3), 1), j, frame(3 * j), True)
        assert np.max(np.abs(np.array(got[:4]) - np.array(box(3 * j)[:4]))) < 1e-9
    # records that are not consecutive frames: the pace per frame counts
    got = check_box_hint(lib, (box(4), frame(4), 4), (box(0), frame(0), 0), 19, frame(19), True)
    assert np.max(np.abs(np.array(got[:4]) - np.array(box(19)[:4]))) < 1e-9
    # a pole came into view between the two records; the date line did
    k = 16
    pole = box(1)[:7] + [1.0]
    check_box_hint(lib, (pole, frame(1), 1), (box(0), frame(0), 0), k, frame(k), False)
    check_box_hint(lib, (box(1), frame(1), 1), (box(0)[:7] + [1.0], frame(0), 0), k, frame(k), False)
    check_box_hint(lib, (pole, frame(1), 1), (box(0)[:7] + [1.0], frame(0), 0), k, frame(k), True)
    wide = [40.0, 52.0, -179.5, 179.0, 170.0, -172.0, 900.0, 0.0]
    wider = [40.1, 52.1, -179.6, 179.2, 170.5, -171.5, 900.0, 0.0]
    check_box_hint(lib, (wide, frame(1), 1), (box(0), frame(0), 0), k, frame(k), False)
    check_box_hint(lib, (box(1), frame(1), 1), (wide, frame(0), 0), k, frame(k), False)
    got = check_box_hint(lib, (wider, frame(1), 1), (wide, frame(0), 0), k, frame(k), True)
    assert abs(got[4] - (170.5 + 15 * 0.5)) < 1e-9 and abs(got[5] - (-171.5 + 15 * 0.5)) < 1e-9
    # the estimate is clamped to +-90 / +-180
    lo = [-88.0, 80.0, -170.0, 160.0, 150.0, -150.0, 10.0, 0.0]
    hi = [-89.0, 86.0, -175.0, 170.0, 165.0, -165.0, 10.0, 0.0]
    got = check_box_hint(lib, (hi, frame(1), 1), (lo, frame(0), 0), k, frame(k), True)
    assert got == [-90.0, 90.0, -180.0, 180.0, 180.0, -180.0, 10.0, 0.0]


# ---- box reduction -> range -> grid (csrc/amt_grid.h) ----------------------------------------------------------------------

RANGE_PROBE = r'''
#include <cstdio>
#include <cstdlib>
#include "amt_grid.h"
int main(int argc, char** argv) {
    for (int k = 1; k + 9 < argc; k += 10) {
        double v[10];
        for (int i = 0; i < 10; ++i) v[i] = std::strtod(argv[k + i], nullptr);
        amt_gl::box_range r;
        const bool ok = amt_gl::range_of_box(v, &r);
        amt_grid g;
        int32_t wrapped = -1;
        const bool laid = amt_gl::layout_of_box(v[8], v[9], v, &g, &wrapped);
        std::printf("%d %.17g %.17g %.17g %.17g %.17g %.17g %d %d %d %d %d %.17g %.17g\n", ok ? 1 : 0, r.lat_lo, r.lat_hi, r.west, r.east,
                    r.lon_lo, r.lon_hi, r.wrapped ? 1 : 0, laid ? 1 : 0, (int)wrapped, laid ? g.nx : 0, laid ? g.ny : 0,
                    laid ? g.lon_center_first : 0.0, laid ? g.lat_center_first : 0.0);
    }
    return 0;
}
'''


def test_box_range_and_layout_equal_the_python_rule(tmp_path):
    """amt_gl::range_of_box / layout_of_box against bounding_box_from_reduction + wrap_at_180 + _Grid on reductions that are
    plain, that straddle the date line, and that straddle without a finite west or east (refused)."""
    from auromat_amd.mapping.mapping import bounding_box_from_reduction, wrap_at_180
    from auromat_amd.resample import _Grid
    inf = float('inf')
    rng = np.random.RandomState(11)
    cases = [([10, 20, -30, 40, 5, -2, 100, 0], (10, 10)), ([10, 20, -179, 178, 170, -175, 100, 0], (10, 10)),
             ([-60.25, -41.5, -179.99, 179.99, 150.125, -160.5, 7, 0], (4, 7)),
             ([10, 20, -179, 178, inf, -175, 100, 0], (10, 10)), ([10, 20, -179, 178, 170, -inf, 100, 0], (10, 10)),
             ([10, 20, -90, 90, 1, -1, 5, 0], (10, 10)),                      # exactly 180 wide: not a straddling box
             ([10.2, 10.3, 20.2, 20.3, 20.2, -inf, 5, 0], (1, 1))]            # a box inside one cell: a range, no grid
    for i in range(60):
        lat = np.sort(rng.uniform(-85, 85, 2))
        if lat[1] - lat[0] < 0.5:
            lat[1] += 1.0
        if i % 2:
            west, east = rng.uniform(120, 179.9), rng.uniform(-179.9, -120)
            red = [lat[0], lat[1], rng.uniform(-180, east), rng.uniform(west, 180), west, east, 50, 0]
            red[2], red[3] = min(red[2], -179.0), max(red[3], 179.0)
        else:
            lon = np.sort(rng.uniform(-179, 179, 2))
            if lon[1] - lon[0] < 0.5 or lon[1] - lon[0] > 180:
                lon = np.array([-20.0, 33.3])
            red = [lat[0], lat[1], lon[0], lon[1], lon[1] if lon[1] > 0 else inf, lon[0] if lon[0] <= 0 else -inf, 50, 0]
        cases.append(([float(v) for v in red], [(10, 10), (4, 7), (2.5, 2.5)][i % 3]))
    src = tmp_path / 'probe.cpp'
    src.write_text(RANGE_PROBE)
    exe = str(tmp_path / 'probe')
    res = subprocess.run(['g++', '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'auromat_amd', 'csrc'), str(src), '-o', exe],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert res.returncode == 0, res.stdout
    args = [repr(float(v)) for red, ppd in cases for v in list(red) + list(ppd)]
    out = subprocess.run([exe] + args, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split('\n')
    kinds = set()
    for (red, ppd), line in zip(cases, out):
        f = line.split()
        ok, wrapped, laid, lay_wrapped, nx, ny = int(f[0]), int(f[7]), int(f[8]), int(f[9]), int(f[10]), int(f[11])
        lat_lo, lat_hi, west, east, lon_lo, lon_hi, lon0, lat0 = [float(f[i]) for i in (1, 2, 3, 4, 5, 6, 12, 13)]
        straddles = red[3] - red[2] > 180
        refused = straddles and not (np.isfinite(red[4]) and np.isfinite(red[5]))
        assert ok == int(not refused) and wrapped == int(straddles), red
        if refused:
            with pytest.raises(AssertionError):                  # (BoundingBox takes no such longitude either)
                bounding_box_from_reduction(red)
            assert not laid and lay_wrapped == -1                # nothing is written for a refused box
            kinds.add('refused')
            continue
        bb = bounding_box_from_reduction(red)
        assert straddles == bb.containsDiscontinuity
        assert (lat_lo, west, lat_hi, east) == (bb.latSouth, bb.lonWest, bb.latNorth, bb.lonEast), red
        want = (wrap_at_180(bb.lonWest + 180), wrap_at_180(bb.lonEast + 180)) if straddles else (bb.lonWest, bb.lonEast)
        assert (lon_lo, lon_hi) == want, red
        assert lay_wrapped == wrapped
        try:
            g = _Grid(ppd, lat_lo, lat_hi, lon_lo, lon_hi)
        except (AssertionError, IndexError):                     # fewer than one cell per axis
            g = None
        assert bool(laid) == (g is not None), red
        if g is not None:
            assert (nx, ny, lon0, lat0) == (g.nx, g.ny, g.lonCenters[0], g.latCenters[0]), red
        kinds.add(('straddling' if straddles else 'plain') + ('' if laid else ' without a grid'))
    assert kinds >= {'plain', 'straddling', 'refused', 'plain without a grid'}, kinds
