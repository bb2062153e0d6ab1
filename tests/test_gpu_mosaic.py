"""
Mosaics on the MI355X (auromat_amd.resample.resampleMosaic, amt_mosaic_frames): a collection's members binned onto one
grid, checked bit for bit against each member's own resample_frame on the collection's grid plus the overlap rule in
NumPy, and against the NumPy statement of the feature (tests/_mosaic_oracle.py) on the members' own arrays.
"""
import os
from datetime import datetime

import numpy as np
import numpy.ma as ma
import pytest

import _mosaic_oracle as MO
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

JPG_S = os.path.join(GOLDEN, 'resources', 'south', 'ISS029-E-8492.jpg')
WCS_S = os.path.join(GOLDEN, 'resources', 'south', 'ISS029-E-8492.wcs')
T0 = datetime(2012, 3, 4, 17, 19, 0)


def _ppd(pxPerDeg):
    try:
        a, b = pxPerDeg
        return (a, b)
    except TypeError:
        return (pxPerDeg, pxPerDeg)


def _cal(z):
    from auromat_amd.mapping.miracle import CalibrationData
    from auromat_amd.mapping.mapping import BoundingBox
    lat, lon = float(z['cal_lat']), float(z['cal_lon'])
    bb = BoundingBox(latSouth=lat + float(z['cal_lat_minus']), lonWest=lon + float(z['cal_lon_minus']),
                     latNorth=lat + float(z['cal_lat_plus']), lonEast=lon + float(z['cal_lon_plus']))
    return CalibrationData(station=str(z['cal_station']), validFrom=None, validTo=None, lat=lat, lon=lon,
                           xc=float(z['cal_xc']), yc=float(z['cal_yc']), k=float(z['cal_k']),
                           rotation=float(z['cal_rotation']), boundingBoxSimple=bb)


def miracle(name, seed, rgb=False, dtype=np.uint8, size=512):
    from auromat_amd.mapping.miracle import MIRACLEMapping
    z = load_golden(name)
    hi = 255 if dtype == np.uint8 else 65535
    shape = (size, size, 3) if rgb else (size, size)
    img = np.random.RandomState(seed).randint(0, hi, shape).astype(dtype)
    return MIRACLEMapping(_cal(z), img, T0, 110).maskedByElevation(10)


def iss(k, seed=None, width=4240, height=2832):
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    from auromat_amd.synthetic import frame_image, sequence_frame
    hdr, cam, t, s = sequence_frame(k, width, height)
    return ArraySpacecraftMapping(hdr, 110, frame_image(width, height, seed=s if seed is None else seed), cam, t, 'iss%d' % k,
                                  fastCenterCalculation=True).maskedByElevation(10)


def collection(members, mayOverlap=True, identifier='net'):
    from auromat_amd.mapping.mapping import MappingCollection
    return MappingCollection(list(members), identifier, mayOverlap=mayOverlap)


def per_member(coll, pxPerDeg=None, arcsecPerPx=None, containsPole=None):
    """Every member's own resample_frame on the collection's grid, then the overlap rule in NumPy."""
    from auromat_amd import resample as R
    ms = coll.mappings
    box = coll.boundingBox
    pole = any(m.containsPole for m in ms) if containsPole is None else containsPole
    ppd = R.plateCarreeResolution(box, arcsecPerPx) if arcsecPerPx else _ppd(pxPerDeg)
    outline = np.concatenate([np.asarray(m.outline) for m in ms]) if pole else None
    res = [R.resample_frame(m.frame(), m.altitude, box, ppd, box.containsDiscontinuity and not pole, pole, outline=outline)
           for m in ms]
    count = np.array([r['count'] for r in res])
    present = count > 0
    first = np.where(present.any(0), np.argmax(present, axis=0), -1)
    nch = res[0]['img'].shape[2] if ms[0].frame().nchan else 0
    if coll.mayOverlap:
        el = np.where(present, np.array([r['mean'][..., -1] for r in res]), -np.inf)
        source = np.where(present.any(0), np.argmax(el, axis=0), -1)
        pick = np.clip(source, 0, None)
        take = lambda a: np.take_along_axis(a, pick.reshape((1,) + pick.shape + (1,) * (a.ndim - 3)), 0)[0]
        want = dict(mean=take(np.array([r['mean'] for r in res])), img=take(np.array([r['img'] for r in res])),
                    count=take(count), mask=take(np.array([r['mask'] for r in res])), source=source, exact_elev=True)
    else:
        total = count.sum(0)
        sums = np.rint(np.array([np.nan_to_num(r['mean'][..., :nch]) * r['count'][..., None] for r in res])).sum(0)
        with np.errstate(invalid='ignore'):
            mean = sums / total[..., None]
            el = np.nansum([r['mean'][..., -1] * r['count'] for r in res], axis=0) / total
        mean = np.where((total > 0)[..., None], np.concatenate([mean, el[..., None]], -1), np.nan)
        img = np.where((total > 0)[..., None], np.rint(np.nan_to_num(mean[..., :nch])), 0).astype(res[0]['img'].dtype)
        want = dict(mean=mean, img=img if nch else res[0]['img'], count=total, mask=total == 0, source=first,
                    exact_elev=False)
    return want, res[0]


def check_against_members(mos, want, first):
    got = dict(img=np.asarray(ma.getdata(mos.img)), mask=ma.getmaskarray(mos.img)[..., 0],
               source=ma.filled(mos.source, -1), elev=ma.filled(mos.elevation, np.nan))
    assert np.array_equal(got['mask'], want['mask'])
    assert np.array_equal(got['source'], want['source'])
    assert np.array_equal(got['img'], want['img'])
    if want['exact_elev']:
        assert np.array_equal(got['elev'], want['mean'][..., -1], equal_nan=True)
    else:
        assert np.allclose(got['elev'], want['mean'][..., -1], rtol=0, atol=1e-9, equal_nan=True)
    # the grid coordinates are those of resample_frame on the collection's box
    for k, a in (('lat', mos.lats), ('lon', mos.lons), ('lat_c', mos.latsCenter), ('lon_c', mos.lonsCenter)):
        assert np.array_equal(ma.getdata(a), first[k]), k


def host_members(coll, res_plan):
    """(x, y, keep, values, window) of every member in the plan's coordinates, from the members' own arrays."""
    from auromat_amd import resample as R
    from auromat_amd.mapping.mapping import wrap_at_180
    out = []
    for m, window in zip(coll.mappings, res_plan['windows']):
        lat = ma.filled(m.latsCenter, np.nan).astype(np.float64)
        lon = ma.filled(m.lonsCenter, np.nan).astype(np.float64)
        keep = ~ma.getmaskarray(m.latsCenter) & ~np.isnan(lat)
        if res_plan['pole']:
            lat, lon = R._rotate_pole_host(lat, lon, m.altitude, 90)
        elif res_plan['lon_wrap']:
            lon = wrap_at_180(lon + 180)
        img = np.asarray(ma.getdata(m.img)).reshape(lat.size, -1).astype(np.float64)
        el = ma.filled(m.elevation, np.nan).astype(np.float64).reshape(-1, 1)
        out.append((lon, lat, keep, np.concatenate([img, el], 1), window))
    return out


def check_against_oracle(coll, mos, res_plan, grid):
    """Counts, integer means and elevation against the NumPy statement where the source agrees; a cell whose source differs
    must be a near tie (its two candidates' mean elevations within 1e-9 deg), and such cells are named."""
    nch = coll.mappings[0].frame().nchan
    rule = 1 if coll.mayOverlap else 0
    want = MO.mosaic(host_members(coll, res_plan), grid.xedges, grid.yedges, rule, nch)
    src = ma.filled(mos.source, -1)
    differ = src != want['source']
    ties = []
    for r, c in np.argwhere(differ):
        assert rule == 1 and src[r, c] >= 0 and want['source'][r, c] >= 0, ('source differs', r, c)
        e = want['elev'][:, r, c]
        a, b = e[src[r, c]], e[want['source'][r, c]]
        assert abs(a - b) <= 1e-9, ('source differs beyond a tie', r, c, a, b)
        ties.append((int(r), int(c), int(src[r, c]), int(want['source'][r, c])))
    if ties:
        print('near ties (row, column, device source, oracle source):', ties)
    same = ~differ
    count = np.asarray(mos._oracle_count)
    assert np.array_equal(count[same], want['count'][same])
    filled = same & (count > 0)
    assert np.array_equal(np.asarray(ma.getdata(mos.img))[filled][:, :nch], want['img'][filled].astype(np.int64))
    el = ma.filled(mos.elevation, np.nan)
    assert np.allclose(el[same], want['mean'][..., -1][same], rtol=0, atol=1e-9, equal_nan=True)
    return src


def mosaic(coll, **kw):
    """resampleMosaic, with the count and plan of the same call kept for the oracle check"""
    from auromat_amd import resample as R
    res = R.mosaic_frames(coll, **kw)
    mos = R._mosaic_mapping(coll, res)
    mos._oracle_count = res['count']
    return mos, res


def run_both(coll, min_winners=2, **kw):
    mos, res = mosaic(coll, **kw)
    want, first = per_member(coll, **kw)
    check_against_members(mos, want, first)
    src = check_against_oracle(coll, mos, res['plan'], res['grid'])
    if coll.mayOverlap or min_winners:
        assert len(set(src[src >= 0].tolist())) >= min_winners, np.unique(src)
    return mos, res


@pytest.mark.parametrize('rule', [True, False])
@pytest.mark.parametrize('kind', ['u8-gray-ppd', 'u16-rgb-arcsec', 'u8-rgb-ppd', 'u16-gray-arcsec'])
def test_one_member_equals_resample_frame(kind, rule):
    from auromat_amd import resample as R
    dtype = np.uint16 if kind.startswith('u16') else np.uint8
    m = miracle('miracle_sod512.npz', 5, rgb='rgb' in kind, dtype=dtype)
    coll = collection([m], mayOverlap=rule)
    kw = dict(arcsecPerPx=100) if 'arcsec' in kind else dict(pxPerDeg=(20, 10))
    box = coll.boundingBox
    mos, res = mosaic(coll, **kw)
    ppd = R.plateCarreeResolution(box, kw['arcsecPerPx']) if 'arcsec' in kind else kw['pxPerDeg']
    one = R.resample_frame(m.frame(), m.altitude, box, ppd, box.containsDiscontinuity, False)
    assert np.array_equal(res['img'], one['img']) and np.array_equal(res['mask'], one['mask'])
    assert np.array_equal(res['mean'], one['mean'], equal_nan=True) and np.array_equal(res['count'], one['count'])
    for k in ('lat', 'lon', 'lat_c', 'lon_c'):
        assert np.array_equal(res[k], one[k])
    assert np.array_equal(res['source'], np.where(one['count'] > 0, 0, -1))
    # the merged box of one member is the member's box up to the degree -> radian -> degree round trip of its ends
    # (mergedBoundingBoxes, as the reference's); where it is the same box, the mosaic is resample(member)
    r = R.resample(m, **kw) if box == m.boundingBox else R.resample(_boxed(m, box), **kw)
    assert np.array_equal(np.asarray(ma.getdata(r.img)), np.asarray(ma.getdata(mos.img)))
    assert np.array_equal(ma.filled(r.elevation, np.nan), ma.filled(mos.elevation, np.nan), equal_nan=True)
    assert mos.members == [m.identifier] and mos.identifier == 'net' and mos.photoTime == m.photoTime


@pytest.mark.parametrize('rule', [True, False])
def test_miracle_sodankyla_and_kevo(rule):
    sod, kev = miracle('miracle_sod512.npz', 1), miracle('miracle_kev96.npz', 2)
    coll = collection([sod, kev], mayOverlap=rule)
    mos, _ = run_both(coll, pxPerDeg=10)
    assert mos.members == [sod.identifier, kev.identifier]
    assert np.array_equal(mos.cameraPosGCRS, sod.cameraPosGCRS)


@pytest.mark.parametrize('kw', [dict(pxPerDeg=10), dict(arcsecPerPx=100)])
def test_iss_sequence_ten_frames(kw):
    coll = collection([iss(k) for k in range(10)], mayOverlap=True, identifier='pass')
    mos, res = run_both(coll, min_winners=3, **kw)
    assert len(mos.members) == 10


def test_date_line_mlat_mlt():
    from auromat_amd.mapping.mapping import convertMappingToSM
    from auromat_amd.mapping.spacecraft import getMapping
    from auromat_amd.resample import resampleMosaicMLatMLT
    a = getMapping(JPG_S, WCS_S, altitude=110, fastCenterCalculation=True).maskedByElevation(10)
    b = _shifted(a, 2.0)
    coll = collection([a, b], mayOverlap=True)
    sm = collection([convertMappingToSM(m) for m in coll.mappings], mayOverlap=True)
    assert sm.boundingBox.containsDiscontinuity and not any(m.containsPole for m in sm.mappings)
    run_both(sm, pxPerDeg=10)
    geo = resampleMosaicMLatMLT(coll, pxPerDeg=10)
    mos, _ = mosaic(sm, pxPerDeg=10)
    assert np.array_equal(ma.filled(geo.source, -1), ma.filled(mos.source, -1))
    assert np.array_equal(np.asarray(ma.getdata(geo.img)), np.asarray(ma.getdata(mos.img)))
    assert geo.members == [a.identifier, b.identifier]


def test_members_of_different_sizes_and_an_odd_width():
    """A 512 x 512 member beside a 255 x 255 one (odd width: the launch takes the unaligned path for every member) and a
    full-size ISS frame beside a small all-sky camera: the tile prefix and the member lookup with mixed tile counts."""
    sod, kev = miracle('miracle_sod512.npz', 1), miracle('miracle_kev96.npz', 2, size=255)
    for rule in (True, False):
        run_both(collection([sod, kev], mayOverlap=rule), pxPerDeg=10)
        run_both(collection([kev, sod], mayOverlap=rule), pxPerDeg=10)
    small = iss(3, width=1061, height=709)
    run_both(collection([iss(0), small], mayOverlap=True), min_winners=2, pxPerDeg=10)


def test_same_geometry_twice_ties_to_the_first_member():
    """Two members with the same calibration and different images: every cell ties on elevation, so member 0 wins every
    cell and the mosaic is member 0's own grid, bit for bit."""
    from auromat_amd import resample as R
    a, b = miracle('miracle_sod512.npz', 1, rgb=True), miracle('miracle_sod512.npz', 7, rgb=True)
    coll = collection([a, b], mayOverlap=True)
    mos, res = mosaic(coll, pxPerDeg=10)
    box = coll.boundingBox
    one = R.resample_frame(a.frame(), a.altitude, box, (10, 10), box.containsDiscontinuity, False)
    assert (res['source'][one['count'] > 0] == 0).all() and (res['source'][one['count'] == 0] == -1).all()
    assert np.array_equal(res['img'], one['img']) and np.array_equal(res['mean'], one['mean'], equal_nan=True)
    assert np.array_equal(res['count'], one['count'])
    other = R.resample_frame(b.frame(), b.altitude, box, (10, 10), box.containsDiscontinuity, False)
    assert not np.array_equal(other['img'], one['img'])


def test_member_with_an_empty_window_bins_nothing(monkeypatch):
    """A member whose window holds no cell adds no tiles and no accumulators: the mosaic is the other member's."""
    from auromat_amd import resample as R
    sod, kev = miracle('miracle_sod512.npz', 1), miracle('miracle_kev96.npz', 2)
    layout = R.mosaic_layout

    def without_second(*a, **k):
        p = layout(*a, **k)
        p['windows'][1] = (0, 0, 0, 0)
        return p
    monkeypatch.setattr(R, 'mosaic_layout', without_second)
    coll = collection([sod, kev], mayOverlap=True)
    mos, res = mosaic(coll, pxPerDeg=10)
    box = coll.boundingBox
    one = R.resample_frame(sod.frame(), sod.altitude, box, (10, 10), box.containsDiscontinuity, False)
    assert np.array_equal(res['source'], np.where(one['count'] > 0, 0, -1))
    assert np.array_equal(res['img'], one['img']) and np.array_equal(res['mean'], one['mean'], equal_nan=True)


def _boxed(m, box):
    """The mapping `m` whose bounding box is `box` (the collection's, an ulp away)"""
    from auromat_amd.mapping.mapping import GenericMapping
    g = GenericMapping.fromMapping(m)
    g._boundingBox = box
    return g


def _shifted(m, dra):
    """A second member from the reference frame's header with CRVAL1 moved by `dra` degrees."""
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    hdr = dict(m._wcsHeader)
    hdr['CRVAL1'] = hdr['CRVAL1'] + dra
    img = np.asarray(ma.getdata(m.img))
    return ArraySpacecraftMapping(hdr, m.altitude, img[::-1].copy(), m.cameraPosGCRS, m.photoTime, 'shifted',
                                  fastCenterCalculation=True).maskedByElevation(10)


def test_pole():
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    from auromat_amd.synthetic import frame_image, pole_frame
    w, h = 1060, 708
    hdr, cam, t = pole_frame(w, h)
    p = ArraySpacecraftMapping(hdr, 110, frame_image(w, h, seed=4, dtype=np.uint8), cam, t, 'p',
                               fastCenterCalculation=True).maskedByElevation(10)
    hdr2 = dict(hdr)
    hdr2['CRVAL2'] = hdr2['CRVAL2'] - 3.0
    q = ArraySpacecraftMapping(hdr2, 110, frame_image(w, h, seed=5, dtype=np.uint8), cam, t, 'q',
                               fastCenterCalculation=True).maskedByElevation(10)
    assert p.containsPole
    coll = collection([p, q], mayOverlap=True)
    mos, res = run_both(coll, pxPerDeg=10)
    assert res['plan']['pole']


def test_stable_and_permutation():
    from auromat_amd.resample import resampleMosaic
    sod, kev = miracle('miracle_sod512.npz', 1), miracle('miracle_kev96.npz', 2)
    a, b = resampleMosaic(collection([sod, kev]), pxPerDeg=10), resampleMosaic(collection([sod, kev]), pxPerDeg=10)
    for x, y in ((a.img, b.img), (a.elevation, b.elevation), (a.source, b.source)):
        assert np.asarray(ma.getdata(x)).tobytes() == np.asarray(ma.getdata(y)).tobytes()
    c = resampleMosaic(collection([kev, sod]), pxPerDeg=10)
    sa, sc = ma.filled(a.source, -1), ma.filled(c.source, -1)
    ea, ec = ma.filled(a.elevation, np.nan), ma.filled(c.elevation, np.nan)
    # (the two stations' cell elevations never tie exactly here, so every source is permuted)
    assert np.array_equal(np.where(sa >= 0, 1 - sa, -1), sc)
    assert np.array_equal(ea, ec, equal_nan=True)
    assert np.array_equal(np.asarray(ma.getdata(a.img)), np.asarray(ma.getdata(c.img)))


def test_refusals():
    from auromat_amd.mapping.mapping import GenericMapping
    from auromat_amd.resample import resampleMosaic
    sod = miracle('miracle_sod512.npz', 1)
    with pytest.raises(ValueError, match='empty'):
        resampleMosaic(collection([]))
    kev = miracle('miracle_kev96.npz', 2)
    from auromat_amd.mapping.miracle import MIRACLEMapping
    high = MIRACLEMapping(_cal(load_golden('miracle_kev96.npz')), np.zeros((512, 512), np.uint8), T0, 120)
    with pytest.raises(ValueError, match='altitude.*' + high.identifier):
        resampleMosaic(collection([sod, high]))
    gray = GenericMapping(kev.lats, kev.lons, kev.latsCenter, kev.lonsCenter, kev.elevation, kev.altitude,
                          np.asarray(ma.getdata(kev.img))[..., :1].copy(), kev.cameraPosGCRS, kev.photoTime, 'gray')
    rgb = GenericMapping(kev.lats, kev.lons, kev.latsCenter, kev.lonsCenter, kev.elevation, kev.altitude,
                         np.repeat(np.asarray(ma.getdata(kev.img))[..., :1], 3, 2), kev.cameraPosGCRS, kev.photoTime, 'rgb')
    with pytest.raises(ValueError, match='dtype or channel.*rgb'):
        resampleMosaic(collection([gray, rgb]))
    wide = miracle('miracle_kev96.npz', 2, dtype=np.uint16)
    with pytest.raises(ValueError, match='dtype or channel'):
        resampleMosaic(collection([sod, wide]))
    noel = GenericMapping(kev.lats, kev.lons, kev.latsCenter, kev.lonsCenter, None, kev.altitude, kev.img,
                          kev.cameraPosGCRS, kev.photoTime, 'no-elevation')
    with pytest.raises(ValueError, match='no-elevation'):
        resampleMosaic(collection([sod, noel], mayOverlap=True))
    assert resampleMosaic(collection([sod, noel], mayOverlap=False), pxPerDeg=5).elevation is None


def test_netcdf_round_trip(tmp_path):
    from auromat_amd.export import netcdf
    from auromat_amd.mapping.netcdf import NetCDFMapping
    from auromat_amd.resample import resampleMosaic
    mos = resampleMosaic(collection([miracle('miracle_sod512.npz', 1), miracle('miracle_kev96.npz', 2)]), pxPerDeg=10)
    path = str(tmp_path / 'mosaic.nc')
    netcdf.write(path, mos, includeMagCoords=False)
    back = NetCDFMapping(path)
    assert np.array_equal(np.asarray(ma.getdata(back.img)), np.asarray(ma.getdata(mos.img)))
    assert np.array_equal(ma.getmaskarray(back.img), ma.getmaskarray(mos.img))
    assert np.allclose(ma.filled(back.latsCenter, np.nan), ma.filled(mos.latsCenter, np.nan), rtol=0, atol=1e-9,
                       equal_nan=True)
    assert back.photoTime == mos.photoTime
