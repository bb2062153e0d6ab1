"""
The host side of the scan-line map (auromat_amd.resample: scanline_strips and the pure rules around it) and the NumPy oracle
of its kernels (tests/_scanline_oracle.py), without a GPU.  tests/test_gpu_scanline_cells.py runs the kernels against the
oracle, tests/test_gpu_scanlines.py the public functions.
"""
import numpy as np
import pytest

import _scanline_cases as K
import _scanline_oracle as O


def _geo():
    from auromat_amd.coordinates import geodesic
    return geodesic


@pytest.mark.parametrize('factor', [1, 2.5])
def test_strips_along_the_equator(factor):
    import auromat_amd.resample as R
    g = _geo()
    props = K.props_along('equator', 6, step_deg=0.2)
    consecutive = g.distance(props[0].centroid, props[1].centroid)
    for diagonal, want in ((1000.0, consecutive), (consecutive, 3 * consecutive)):      # 3 * diagonal below / above the distance
        assert (3 * diagonal > consecutive) == (want != consecutive)
        s = R.scanline_strips(props, diagonal, lineWidthFactor=factor)
        assert len(s['polygons']) == len(s['azimuths']) == 6                          # N frames give N strips
        assert s['width'] == want * factor
        bb = props[0].boundingBox
        assert s['height'] == 1.5 * g.distance(bb.topLeft, bb.bottomRight)
        assert np.max(np.abs(np.array(s['azimuths']) - 90)) < 1e-9
        assert s['azimuths'][-1] == s['azimuths'][-2]                                 # the last frame reuses the azimuth
        for p, poly in zip(props, s['polygons']):
            # the lines' first points, in the reference's order: topLeft, topRight, bottomRight, bottomLeft
            lines = [g.line(a, b) for a, b in _corner_pairs(p.centroid, s['azimuths'][0], s['width'], s['height'])]
            assert len(poly) == sum(len(l) for l in lines) - 4
            assert len(np.unique(poly, axis=0)) == len(poly)                          # no vertex twice
            starts = np.cumsum([0] + [len(l) - 1 for l in lines[:-1]])
            tl, tr, br, bl = poly[starts]
            # heading east on the equator: the strip is symmetric about the centroid in both coordinates
            np.testing.assert_allclose(tl + br, 2 * np.array(p.centroid), rtol=0, atol=1e-9)
            np.testing.assert_allclose(tr + bl, 2 * np.array(p.centroid), rtol=0, atol=1e-9)
            assert tl[0] > 0 > bl[0] and tl[1] < tr[1]                                # az - 90 is north, az is east
            # the sides run up their meridians from the equator, where they are `width` apart
            assert abs(g.distance(g.Location(0.0, tl[1]), g.Location(0.0, tr[1])) - s['width']) < 1e-6 * s['width']


def _corner_pairs(centroid, az, width, height):
    g = _geo()
    right, left = g.destination(centroid, az, width / 2), g.destination(centroid, az + 180, width / 2)
    tl, bl = g.destination(left, az - 90, height / 2), g.destination(left, az + 90, height / 2)
    tr, br = g.destination(right, az - 90, height / 2), g.destination(right, az + 90, height / 2)
    return (tl, tr), (tr, br), (br, bl), (bl, tl)


def test_meridional_track_and_short_sequences():
    import auromat_amd.resample as R
    props = K.props_along('meridian', 4, step_deg=0.2, start=10.0)
    s = R.scanline_strips(props, 1000.0)
    assert np.max(np.abs(np.array(s['azimuths']))) < 1e-9
    assert s['azimuths'][-1] == s['azimuths'][-2] and len(s['polygons']) == 4
    for n in (0, 1):
        with pytest.raises(ValueError, match='mapping sequence too short, need at least 2 mappings'):
            R.scanline_strips(props[:n], 1000.0)
    with pytest.raises(ValueError, match='pole'):
        R.scanline_strips(K.props_along('meridian', 3, step_deg=0.2, start=86.0, box_half=(1.5, 5.0)), 1000.0)


def test_longitude_frame_rule():
    import auromat_amd.resample as R
    from auromat_amd.coordinates.geodesic import Location
    from auromat_amd.mapping.mapping import BoundingBox
    assert R.scanline_longitude_frame(Location(60, 170)) and R.scanline_longitude_frame(Location(60, -91))
    assert not R.scanline_longitude_frame(Location(60, 10)) and not R.scanline_longitude_frame(Location(60, -90))
    across_180, across_0, plain = BoundingBox(50, 170, 60, -170), BoundingBox(50, -10, 60, 10), BoundingBox(50, 20, 60, 40)
    R.scanline_check_fits(plain, False, 1)
    R.scanline_check_fits(across_0, False, 1)
    R.scanline_check_fits(across_180, True, 1)
    R.scanline_check_fits(BoundingBox(50, 100, 60, 120), True, 1)
    with pytest.raises(ValueError, match=r'frame 3 \(\'id3\'\).*spans the seam of its longitude frame'):
        R.scanline_check_fits(across_180, False, 3, 'id3')                # first at lon 10, then a box across +-180
    with pytest.raises(ValueError, match='frame 2 .*spans the seam'):
        R.scanline_check_fits(across_0, True, 2)                          # first at lon 170, then a box across 0


def test_polygon_discontinuity_decision_is_the_bounding_boxes():
    import auromat_amd.resample as R
    from auromat_amd.mapping.mapping import BoundingBox
    rs = np.random.RandomState(0)
    sets = [rs.uniform(100, 179, 9), np.r_[rs.uniform(150, 180, 5), rs.uniform(-180, -150, 5)], rs.uniform(-30, 30, 8),
            np.array([179.5, -179.5]), np.array([10.0, 20.0, 10.0]), rs.uniform(-180, 180, 40), np.array([-180.0, 170.0, 175.0])]
    for lons in sets:
        box = BoundingBox.minimumBoundingBox([(0.0, lon) for lon in lons])
        assert R.lons_contain_discontinuity(lons) == box.containsDiscontinuity, lons


def test_global_indices_and_union_grid():
    """Grids of two boxes at a non-integer pxPerDeg share node indices, and the union grid's centres ARE the global nodes."""
    import auromat_amd.resample as R
    ppd = (36.0, 22.37)
    latAll, lonAll = R.scanline_global_axes(ppd)
    a = R.cached_grid(ppd, 50.013, 58.4, -20.3, 1.77)
    b = R.cached_grid(ppd, 53.2, 61.05, -11.9, 9.31)
    origins = []
    for g in (a, b):
        r0, c0 = R.scanline_global_origin(g, ppd)
        origins.append((r0, c0))
        np.testing.assert_allclose(g.latCenters, latAll[::-1][r0:r0 + g.ny], rtol=0, atol=1e-3 / 36)
        np.testing.assert_allclose(g.lonCenters, lonAll[c0:c0 + g.nx], rtol=0, atol=1e-3 / 22.37)
    # a cell both grids hold has one global index: its centres agree to rounding
    (ra, ca), (rb, cb) = origins
    row, col = max(ra, rb) + 3, max(ca, cb) + 5
    assert abs(a.latCenters[row - ra] - b.latCenters[row - rb]) < 1e-9 and abs(a.lonCenters[col - ca] - b.lonCenters[col - cb]) < 1e-9
    rowMin, rowMax = min(ra, rb), max(ra + a.ny, rb + b.ny) - 1
    colMin, colMax = min(ca, cb), max(ca + a.nx, cb + b.nx) - 1
    u = R.scanline_union_grid(ppd, rowMin, rowMax, colMin, colMax)
    assert (u.ny, u.nx) == (rowMax - rowMin + 1, colMax - colMin + 1)
    assert np.array_equal(u.latCenters, latAll[::-1][rowMin:rowMax + 1])
    assert np.array_equal(u.lonCenters, lonAll[colMin:colMax + 1])
    assert R.scanline_global_origin(u, ppd) == (rowMin, colMin)
    # corners: half a step off the centres, one more than cells, the 2-D arrays follow
    assert u.lat.shape == (u.ny + 1, u.nx + 1) and u.lat_c.shape == (u.ny, u.nx)
    assert np.all(u.lat[:-1, 0] > u.latCenters) and np.all(u.latCenters > u.lat[1:, 0])
    assert np.all(u.lon[0, :-1] < u.lonCenters) and np.all(u.lonCenters < u.lon[0, 1:])
    assert np.array_equal(u.lat_c[:, 0], u.latCenters) and np.array_equal(u.lon_c[0], u.lonCenters)


def test_window_of_a_polygon():
    import auromat_amd.resample as R
    lat, lon = K._lattice(20, 20)
    box = lambda la0, la1, lo0, lo1: np.array([(la0, lo0), (la0, lo1), (la1, lo1), (la1, lo0)], dtype=np.float64)
    assert R.scanline_window(lat, lon, box(12.5, 33, -3, 6.5)) == (0, 0, 8, 7)          # clipped north and west
    assert R.scanline_window(lat, lon, box(-4, 6.5, 12.5, 31)) == (13, 12, 7, 8)        # clipped south and east
    assert R.scanline_window(lat, lon, box(8, 10, 5, 6)) == (9, 4, 4, 3)                # one cell wider each way
    assert R.scanline_window(lat, lon, box(30, 40, 5, 6)) == (0, 0, 0, 0)
    assert R.scanline_window(lat, lon, box(8.25, 8.75, 5, 6)) == (0, 0, 0, 0)           # no corner row in the box
    for c in K.select_cases():
        # every kept cell of a whole-frame selection lies in the window
        kept = O.four_corner_rule(O.corners_inside(c.lat_axis, c.lon_axis, c.polygon), c.mask)
        if len(c.polygon) and kept.any():
            r0, c0, rows, cols = R.scanline_window(c.lat_axis, c.lon_axis, c.polygon)
            inside = np.zeros(kept.shape, dtype=bool)
            inside[r0:r0 + rows, c0:c0 + cols] = True
            assert not (kept & ~inside).any(), c.name


def test_select_oracle_on_hand_checked_cells():
    lat, lon = K._lattice(4, 4)                                       # corners lat 4..0, lon 0..4
    poly = np.array([(0.5, 0.5), (0.5, 3.5), (3.5, 3.5), (3.5, 0.5)])
    keep, stats = O.select(lat, lon, poly, np.zeros((4, 4), np.uint8), (0, 0, 4, 4))
    want = np.zeros((4, 4), np.uint8)
    want[1:3, 1:3] = 1                                                # the cells between the corners 1..3
    assert np.array_equal(keep, want) and stats.tolist() == [4, 1, 2, 1, 2]
    mask = np.zeros((4, 4), np.uint8)
    mask[1, 1] = 1
    keep, stats = O.select(lat, lon, poly, mask, (2, 0, 2, 4))        # the window's rows 2..3 only
    assert keep.tolist() == [[0, 1, 1, 0], [0, 0, 0, 0]] and stats.tolist() == [2, 2, 2, 1, 2]
    keep, stats = O.select(lat, lon, poly[:2], mask, (0, 0, 4, 4))
    assert not keep.any() and stats.tolist() == [0, O.INT64_MAX, O.INT64_MIN, O.INT64_MAX, O.INT64_MIN]
    names = [c.name for c in K.select_cases()]
    assert len(set(names)) == len(names)
    assert any(len(c.polygon) > K.CHUNK for c in K.select_cases())


def test_compose_oracle_on_hand_written_cases():
    nan = np.nan
    rec = lambda cells, v: dict(row=np.array([c[0] for c in cells], np.int32), col=np.array([c[1] for c in cells], np.int32),
                                planes=np.full((1, len(cells)), float(v)), img=np.full((1, len(cells)), v, np.uint8))
    a = rec([(10, 20), (10, 21), (11, 20)], 1)
    b = rec([(10, 21), (11, 21), (13, 23)], 2)
    for strips, frames in (([a, b], [0, 1]), ([b, a], [1, 0])):       # later wins, whatever the order of the table
        planes, img, mask, index, outside = O.compose(strips, frames, 10, 20, 4, 4, 1, 1)
        assert not outside
        assert index.tolist() == [[0, 1, -1, -1], [0, 1, -1, -1], [-1, -1, -1, -1], [-1, -1, -1, 1]]
        assert np.array_equal(mask, (index < 0).astype(np.uint8))
        assert np.array_equal(planes[..., 0], np.where(index < 0, nan, index + 1.0), equal_nan=True)
        assert np.array_equal(img[..., 0], np.where(index < 0, 0, index + 1))
    # the frame index decides, not the position: `a` as frame 5 paints over `b` as frame 2
    index = O.compose([b, a], [2, 5], 10, 20, 4, 4, 1, 1)[3]
    assert index[0].tolist() == [5, 5, -1, -1] and index[1].tolist() == [5, 2, -1, -1]
    # a record outside is reported; the others are composed
    planes, img, mask, index, outside = O.compose([a, b], [0, 1], 10, 20, 3, 3, 1, 1)
    assert outside and index.tolist() == [[0, 1, -1], [0, 1, -1], [-1, -1, -1]]
    # no strips: an empty raster
    planes, img, mask, index, outside = O.compose([], [], 0, 0, 4, 4, 2, 0)
    assert np.isnan(planes).all() and mask.all() and (index == -1).all() and img.shape == (4, 4, 0) and not outside


def test_pack_oracle_and_entry_points_are_declared():
    planes, img = K.frame_data(4, 5, 3, True, np.uint16, 0)
    keep = np.zeros((2, 3), np.uint8)
    keep[0, 2] = keep[1, 0] = 1
    r = O.pack(keep, (1, 2, 2, 3), planes, img, row_offset=100, col_offset=-7)
    assert r['row'].tolist() == [101, 102] and r['col'].tolist() == [-3, -5]
    assert np.array_equal(r['planes'][:, 0], planes[1, 4]) and np.array_equal(r['img'][:, 1], img[2, 2])
    shuffled = dict(row=r['row'][::-1], col=r['col'][::-1], planes=r['planes'][:, ::-1], img=r['img'][:, ::-1])
    back = O.sort_records(shuffled)
    assert all(np.array_equal(back[k], r[k]) for k in r)
    from auromat_amd import _native
    import ctypes as C
    for name in ('amt_scanline_select', 'amt_scanline_pack', 'amt_scanline_compose'):
        assert name in _native.exported_symbols()
    assert C.sizeof(_native.ScanLineStrip) == 48
    from auromat_amd.mapping.mapping import GenericMapping, ScanLineMapping
    assert issubclass(ScanLineMapping, GenericMapping)
