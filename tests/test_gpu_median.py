"""
Median binning on the MI355X (auromat_amd.resample.resampleMedian, amt_median_frame) against the NumPy statement of the
feature (tests/_median_oracle.py) applied to the mapping's own arrays: the same pixel set as the mean, np.median per cell
and channel, exact — image channels equal, elevation bit-equal — for cells of one pixel up to more than a million, as the
camera frames happen to fill them.  The tier boundaries, the key patterns and the pixel orders that no frame controls are
in tests/test_gpu_median_cells.py.
"""
import os
from datetime import datetime

import numpy as np
import numpy.ma as ma
import pytest

import _median_oracle as M
from conftest import GOLDEN, assert_counts_equal_up_to_edge_pixels, load_golden

pytestmark = pytest.mark.gpu

JPG = os.path.join(GOLDEN, 'resources', 'ISS030-E-102170_dc.jpg')
WCS = os.path.join(GOLDEN, 'resources', 'ISS030-E-102170_dc.wcs')
JPG_S = os.path.join(GOLDEN, 'resources', 'south', 'ISS029-E-8492.jpg')
WCS_S = os.path.join(GOLDEN, 'resources', 'south', 'ISS029-E-8492.wcs')


def _ppd(pxPerDeg):
    try:
        a, b = pxPerDeg
        return (a, b)
    except TypeError:
        return (pxPerDeg, pxPerDeg)


def run_median(m, pxPerDeg=None, arcsecPerPx=None, min_elevation=None):
    """resample_frame_median with resampleMedian's arguments (the grid comes back with it), and resampleMedian itself,
    which must give the same image and elevation."""
    from auromat_amd import resample as R
    pole = m.containsPole
    ppd = R.plateCarreeResolution(m.boundingBox, arcsecPerPx) if arcsecPerPx else _ppd(pxPerDeg)
    res = R.resample_frame_median(m.frame(), m.altitude, m.boundingBox, ppd, m.containsDiscontinuity, pole,
                                  min_elevation=min_elevation, outline=m.outline if pole else None)
    if min_elevation is None:
        r = R.resampleMedian(m, pxPerDeg=pxPerDeg, arcsecPerPx=arcsecPerPx)
        assert np.array_equal(np.asarray(ma.getdata(r.img)), res['img'])
        assert np.array_equal(ma.getmaskarray(r.img)[..., 0], res['mask'])
        if res['has_elev']:
            assert np.array_equal(ma.filled(r.elevation, np.nan), res['median'][..., -1], equal_nan=True)
    return res


def own_arrays(m):
    """(lat_c, lon_c, keep, values (n, nchan + 1)) of a mapping, host side: what the device bins."""
    lat = ma.filled(m.latsCenter, np.nan).astype(np.float64).ravel()
    lon = ma.filled(m.lonsCenter, np.nan).astype(np.float64).ravel()
    keep = ~ma.getmaskarray(m.latsCenter).ravel() & ~np.isnan(lat)
    img = np.asarray(ma.getdata(m.img))
    img = img.reshape(lat.size, -1)
    el = ma.filled(m.elevation, np.nan).astype(np.float64).ravel()
    return lat, lon, keep, img, el


def expected(res, lat, lon, keep, img, el):
    g = res['grid']
    med_img, count = M.median_bins(lon, lat, img, g.xedges, g.yedges, keep=keep)
    med_el, _ = M.median_bins(lon, lat, el[:, None], g.xedges, g.yedges, keep=keep)
    return med_img, med_el[..., 0], count


def check_exact(res, lat, lon, keep, img, el):
    from oracle import ref_numpy as O
    med_img, med_el, count = expected(res, lat, lon, keep, img, el)
    assert np.array_equal(res['count'], count)
    assert np.array_equal(res['mask'], count == 0)
    nch = img.shape[1]
    assert np.array_equal(res['median'][..., :nch], med_img, equal_nan=True)
    assert np.array_equal(res['median'][..., nch], med_el, equal_nan=True)            # bit-equal: (a + b) / 2 in float64
    want_img, _ = O.finalize_image(med_img, img.dtype)
    assert np.array_equal(res['img'], want_img)
    return count


def check_up_to_edge_pixels(res, lat, lon, keep, img, el, what):
    """Coordinates the oracle rotated / wrapped itself (~1e-11 deg from the device's): counts equal up to pixels on an edge,
    medians equal in every other cell."""
    med_img, med_el, count = expected(res, lat, lon, keep, img, el)
    g = res['grid']
    want = dict(count=count, lat=np.repeat(g.yedges[::-1][:, None], g.nx + 1, 1), lon=np.repeat(g.xedges[None], g.ny + 1, 0))
    lat_k, lon_k = np.where(keep, lat, np.nan), np.where(keep, lon, np.nan)
    assert_counts_equal_up_to_edge_pixels(want, res['count'], lat_k, lon_k, what)
    same = res['count'] == count
    nch = img.shape[1]
    assert np.array_equal(res['median'][..., :nch][same], med_img[same], equal_nan=True), what
    assert np.array_equal(res['median'][..., nch][same], med_el[same], equal_nan=True), what
    assert (count > 0).sum() > 50
    return count


@pytest.fixture(scope='module')
def real_frame():
    from auromat_amd.mapping.spacecraft import getMapping
    return getMapping(JPG, WCS, altitude=110, fastCenterCalculation=True).maskedByElevation(10)


@pytest.mark.parametrize('kw', [dict(pxPerDeg=10), dict(pxPerDeg=(4, 7)), dict(arcsecPerPx=100)])
def test_reference_frame_full_size(real_frame, kw):
    from auromat_amd.mapping.spacecraft import getMapping
    from auromat_amd.resample import resample
    m = real_frame
    res = run_median(m, **kw)
    lat, lon, keep, img, el = own_arrays(m)
    assert img.dtype == np.uint8 and img.shape[1] == 3
    count = check_exact(res, lat, lon, keep, img, el)
    assert (count > 0).sum() > 1000
    g = res['grid']
    assert M.odd_gap_pairs(lon, lat, img, g.xedges, g.yedges, keep=keep) > 0      # half-to-even rounding is exercised
    # the mean masks exactly the same cells (resample as a user calls it, on a mapping of its own)
    r = resample(getMapping(JPG, WCS, altitude=110, fastCenterCalculation=True).maskedByElevation(10), **kw)
    assert np.array_equal(ma.getmaskarray(r.img)[..., 0], res['mask'])


def _synthetic_mapping(w, h, dtype, nch, seed=3, pointing='iss030'):
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    from auromat_amd.synthetic import frame_header, frame_image
    hdr, cam, t = frame_header(w, h, pointing)
    img = frame_image(w, h, seed=seed, dtype=dtype)[..., :nch]
    return ArraySpacecraftMapping(hdr, 110, img, cam, t, 'n', fastCenterCalculation=True).maskedByElevation(10)


@pytest.mark.parametrize('dtype,nch', [(np.uint8, 3), (np.uint16, 3), (np.uint8, 1), (np.uint16, 1)])
@pytest.mark.parametrize('ppd', [10, 1])
def test_cell_sizes_synthetic(dtype, nch, ppd):
    m = _synthetic_mapping(1060, 708, dtype, nch)
    res = run_median(m, pxPerDeg=ppd)
    lat, lon, keep, img, el = own_arrays(m)
    assert img.dtype == dtype and img.shape[1] == nch
    count = check_exact(res, lat, lon, keep, img, el)
    if ppd == 1:
        assert count.max() > 1000


@pytest.mark.parametrize('dtype,nch', [(np.uint16, 3), (np.uint8, 1)])
def test_cell_sizes_full_frame(dtype, nch):
    """pxPerDeg=1 (thousands of pixels per cell) and 10-degree / 20-degree cells, of which one holds more than a million
    pixels (the tier that spreads one cell over many workgroups)."""
    m = _synthetic_mapping(4256, 2832, dtype, nch)
    lat, lon, keep, img, el = own_arrays(m)
    biggest = 0
    for ppd in (1, 0.1, 0.05):
        res = run_median(m, pxPerDeg=ppd)
        count = check_exact(res, lat, lon, keep, img, el)
        biggest = max(biggest, count.max())
    assert biggest > 1000000, biggest


def test_reference_frame_coarse_grid(real_frame):
    res = run_median(real_frame, pxPerDeg=0.05)
    lat, lon, keep, img, el = own_arrays(real_frame)
    count = check_exact(res, lat, lon, keep, img, el)
    assert count.max() > 1000000, count.max()


@pytest.mark.parametrize('south', [False, True])
def test_pole(south):
    from oracle import ref_numpy as O
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    from auromat_amd.synthetic import frame_image, pole_frame
    w, h = 1060, 708
    hdr, cam, t = pole_frame(w, h, south=south)
    m = ArraySpacecraftMapping(hdr, 110, frame_image(w, h, seed=4, dtype=np.uint8), cam, t, 'p',
                               fastCenterCalculation=True).maskedByElevation(10)
    assert m.containsPole
    res = run_median(m, pxPerDeg=10)
    lat, lon, keep, img, el = own_arrays(m)
    la, lo = O.rotate_pole(np.deg2rad(lat), np.deg2rad(lon), 110, angle=90, axis=(1, 0, 0))
    check_up_to_edge_pixels(res, np.rad2deg(la), np.rad2deg(lo), keep, img, el, 'pole south=%s' % south)


def test_date_line_mlat_mlt():
    """The southern reference frame on the MLat / MLT grid: its SM box crosses +-180 deg."""
    from oracle import ref_numpy as O
    from auromat_amd.mapping.mapping import convertMappingToSM
    from auromat_amd.mapping.spacecraft import getMapping
    from auromat_amd.resample import resampleMedianMLatMLT
    m = getMapping(JPG_S, WCS_S, altitude=110, fastCenterCalculation=True).maskedByElevation(10)
    r = resampleMedianMLatMLT(m, pxPerDeg=10)
    sm = convertMappingToSM(m)
    assert sm.containsDiscontinuity and not sm.containsPole
    res = run_median(sm, pxPerDeg=10)
    assert np.array_equal(np.asarray(ma.getdata(r.img)), res['img'])
    assert np.array_equal(ma.filled(r.elevation, np.nan), res['median'][..., -1], equal_nan=True)
    lat, lon, keep, img, el = own_arrays(sm)
    check_up_to_edge_pixels(res, lat, O.wrap_at(lon + 180, 180), keep, img, el, 'date line')


def test_miracle():
    from auromat_amd.mapping.miracle import CalibrationData, MIRACLEMapping
    from auromat_amd.mapping.mapping import BoundingBox
    z = load_golden('miracle_sod64.npz')
    n = int(z['size'])
    lat0, lon0 = float(z['cal_lat']), float(z['cal_lon'])
    bb = BoundingBox(latSouth=lat0 + float(z['cal_lat_minus']), lonWest=lon0 + float(z['cal_lon_minus']),
                     latNorth=lat0 + float(z['cal_lat_plus']), lonEast=lon0 + float(z['cal_lon_plus']))
    cal = CalibrationData(station=str(z['cal_station']), validFrom=None, validTo=None, lat=lat0, lon=lon0,
                          xc=float(z['cal_xc']), yc=float(z['cal_yc']), k=float(z['cal_k']),
                          rotation=float(z['cal_rotation']), boundingBoxSimple=bb)
    gray = np.random.RandomState(1).randint(0, 256, size=(n, n)).astype(np.uint8)
    m = MIRACLEMapping(cal, gray, datetime(2012, 3, 4, 17, 19, 0), float(z['altitude'])).maskedByElevation(0.1)
    res = run_median(m, pxPerDeg=10)
    lat, lon, keep, img, el = own_arrays(m)
    count = check_exact(res, lat, lon, keep, img, el)
    assert (count > 0).sum() > 20


def test_collection_and_determinism():
    from auromat_amd.mapping.mapping import MappingCollection
    from auromat_amd.resample import resampleMedian
    a = _synthetic_mapping(530, 354, np.uint16, 3, seed=1)
    b = _synthetic_mapping(530, 354, np.uint16, 3, seed=2, pointing='iss029')
    coll = resampleMedian(MappingCollection([a, b], 'pair'), pxPerDeg=5)
    assert isinstance(coll, MappingCollection) and len(coll.mappings) == 2
    for m, got in zip((a, b), coll.mappings):
        one = resampleMedian(m, pxPerDeg=5)
        assert np.array_equal(np.asarray(ma.getdata(one.img)), np.asarray(ma.getdata(got.img)))
        assert np.array_equal(ma.filled(one.elevation, np.nan), ma.filled(got.elevation, np.nan), equal_nan=True)
    # two identical calls: the same bits (the scatter order of the keys does not reach the result)
    m = _synthetic_mapping(1060, 708, np.uint16, 3, seed=7)
    r1, r2 = run_median(m, pxPerDeg=1), run_median(m, pxPerDeg=1)
    for k in ('median', 'img', 'mask', 'count'):
        assert np.asarray(r1[k]).tobytes() == np.asarray(r2[k]).tobytes(), k


def test_no_pixel_survives():
    m = _synthetic_mapping(530, 354, np.uint8, 3)
    res = run_median(m, pxPerDeg=10, min_elevation=91.0)
    assert res['mask'].all() and res['mask'].size > 10
    assert (res['count'] == 0).all()
    assert np.isnan(res['median']).all()
    assert (res['img'] == 0).all()
