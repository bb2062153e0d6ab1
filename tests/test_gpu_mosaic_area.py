"""
Area-weighted mosaics on the MI355X through the class API (auromat_amd.resample.resampleMosaic(statistic='area'),
mosaic_frames, amt_area_mosaic_frames) on real geometry at reduced sizes: all-sky cameras of 128 x 128 pixels, ISS frames of
424 x 283, a pole pair and a pair across +-180 deg of SM longitude.  Every output is compared bit for bit with the NumPy
statement of the feature (tests/_mosaic_area_oracle.py), fed with the host copies of the arrays the device binned (rotated
corners are read back, so the last bits of the trigonometry do not enter).  The kernels' paths, windows and limits that no
collection controls are in tests/test_gpu_mosaic_area_cells.py; tests/test_mosaic_area_cpu.py shows on the all-sky pair used
here, at the resolution used here, that the area mosaic fills the holes of the mean mosaic.
"""
from datetime import datetime

import numpy as np
import numpy.ma as ma
import pytest

import _area_cases as K
import _area_oracle as O
import _mosaic_area_oracle as MA
from conftest import load_golden

pytestmark = pytest.mark.gpu

OUT_KEYS = ('area', 'img', 'mask', 'coverage', 'source')
T0 = datetime(2012, 3, 4, 17, 19, 0)
ALLSKY_PPD = 20                 # the resolution of the hole-closing condition of tests/test_mosaic_area_cpu.py


def _cal(z):
    from auromat_amd.mapping.miracle import CalibrationData
    from auromat_amd.mapping.mapping import BoundingBox
    lat, lon = float(z['cal_lat']), float(z['cal_lon'])
    bb = BoundingBox(latSouth=lat + float(z['cal_lat_minus']), lonWest=lon + float(z['cal_lon_minus']),
                     latNorth=lat + float(z['cal_lat_plus']), lonEast=lon + float(z['cal_lon_plus']))
    return CalibrationData(station=str(z['cal_station']), validFrom=None, validTo=None, lat=lat, lon=lon,
                           xc=float(z['cal_xc']), yc=float(z['cal_yc']), k=float(z['cal_k']),
                           rotation=float(z['cal_rotation']), boundingBoxSimple=bb)


def miracle(name, seed, size=128, rgb=False, dtype=np.uint8):
    from auromat_amd.mapping.miracle import MIRACLEMapping
    hi = 255 if dtype == np.uint8 else 65535
    img = np.random.RandomState(seed).randint(0, hi, (size, size, 3) if rgb else (size, size)).astype(dtype)
    return MIRACLEMapping(_cal(load_golden(name)), img, T0, 110).maskedByElevation(10)


def iss(k, width=424, height=283, pointing='iss030', dra=0.0):
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    from auromat_amd.synthetic import frame_image, sequence_frame
    hdr, cam, t, s = sequence_frame(k, width, height, pointing)
    hdr['CRVAL1'] = hdr['CRVAL1'] + dra
    return ArraySpacecraftMapping(hdr, 110, frame_image(width, height, seed=s), cam, t, '%s-%d' % (pointing, k),
                                  fastCenterCalculation=True).maskedByElevation(10)


def collection(members, mayOverlap=True, identifier='net'):
    from auromat_amd.mapping.mapping import MappingCollection
    return MappingCollection(list(members), identifier, mayOverlap=mayOverlap)


def allsky_pair():
    return [miracle('miracle_sod512.npz', 1), miracle('miracle_kev96.npz', 2)]


def _host(t):
    return None if t is None else t.cpu().numpy()


def binned_cases(coll, res):
    """Every member as the device binned it, as an oracle case on the grid of the result `res` of mosaic_frames."""
    from auromat_amd import resample as R
    plan, g = res['plan'], res['grid']
    out = []
    for i, m in enumerate(coll.mappings):
        fd = m.frame()
        lat, lon, lat_c = fd.lat, fd.lon, fd.lat_c
        if plan['pole']:
            lat, lon = R._rotate_pole_dev(fd.ctx, fd.lat, fd.lon, m.altitude, 90)
            lat_c, _ = R._rotate_pole_dev(fd.ctx, fd.lat_c, fd.lon_c, m.altitude, 90)
        img = fd.host_image().reshape(fd.height * fd.width, -1) if fd.nchan else np.zeros((fd.height * fd.width, 0), np.uint8)
        out.append(K.AreaCase('member%d' % i, _host(lat), _host(lon), g.xedges, g.yedges, lat_c=_host(lat_c), elev=_host(fd.elev),
                              mask=_host(fd.center_mask), lon_wrap=plan['lon_wrap'], img=img))
    return out


def accumulators(coll, res):
    return [MA.member_accumulators(c, w) for c, w in zip(binned_cases(coll, res), res['plan']['windows'])]


def check(res, accs, rule, minCoverage=0.5):
    want = MA.elect(accs, rule, res['img'].dtype, O.min_weight(minCoverage))
    assert not want['over'] and res['mask'].dtype == bool and res['source'].dtype == np.int32
    got = dict(res, mask=res['mask'].astype(np.uint8))
    if accs[0].shape[0] == 2:                                   # no channels: the result carries a zero image of one channel
        want = dict(want, img=np.zeros(want['mask'].shape + (1,), res['img'].dtype))
    for key in OUT_KEYS:
        assert O.same_bits(got[key], want[key]), key
    assert np.array_equal(res['mask'], res['source'] < 0)
    return want


def run_both_rules(members, min_winners=2, **kw):
    """mosaic_frames(statistic='area') under both rules against the oracle on ONE set of accumulators."""
    from auromat_amd import resample as R
    accs, out = None, {}
    for rule in (True, False):
        coll = collection(members, mayOverlap=rule)
        res = R.mosaic_frames(coll, statistic='area', **kw)
        accs = accumulators(coll, res) if accs is None else accs
        want = check(res, accs, 1 if rule else 0)
        filled = want['mask'] == 0
        assert filled.sum() > 200 and len(np.unique(want['source'][filled])) >= min_winners
        out[rule] = (coll, res, want)
    return out, accs


@pytest.fixture(scope='module')
def allsky():
    members = allsky_pair()
    out, accs = run_both_rules(members, pxPerDeg=ALLSKY_PPD)
    return members, out, accs


def test_allsky_pair_equals_oracle(allsky):
    members, out, accs = allsky
    coll, res, want = out[True]
    assert res['plan']['rule'] == 1 and not res['plan']['pole'] and res['area'].shape == res['mask'].shape + (members[0].frame().nchan + 1,)
    # more than half of a cell asked for: cells that a member covers less stay masked although weight arrived
    assert ((want['mask'] == 1) & (want['coverage'] > 0)).sum() > 50
    for cov in (0.0, 1.0):
        from auromat_amd import resample as R
        check(R.mosaic_frames(coll, pxPerDeg=ALLSKY_PPD, statistic='area', minCoverage=cov), accs, 1, cov)


def test_one_member_equals_resample_area():
    from auromat_amd import resample as R
    m = miracle('miracle_sod512.npz', 5, rgb=True, dtype=np.uint16)
    for rule in (True, False):
        coll = collection([m], mayOverlap=rule)
        box = coll.boundingBox
        res = R.mosaic_frames(coll, pxPerDeg=(20, 10), statistic='area')
        one = R.resample_frame_area(m.frame(), m.altitude, box, (20, 10), box.containsDiscontinuity, False)
        for key in ('area', 'img', 'mask', 'coverage', 'lat', 'lon', 'lat_c', 'lon_c'):
            assert O.same_bits(res[key], one[key]), key
        assert np.array_equal(res['source'], np.where(one['mask'], -1, 0)) and (~one['mask']).sum() > 200
        mos = R.resampleMosaic(coll, pxPerDeg=(20, 10), statistic='area')
        assert np.array_equal(np.asarray(ma.getdata(mos.img))[~one['mask']], one['img'][~one['mask']])
        assert np.array_equal(ma.getmaskarray(mos.img)[..., 0], one['mask'])
        assert np.array_equal(ma.filled(mos.elevation, np.nan), one['area'][..., -1], equal_nan=True)
        assert mos.members == [m.identifier] and mos.identifier == 'net'


def test_iss_frames():
    out, _ = run_both_rules([iss(k) for k in (0, 4, 8)], min_winners=2, pxPerDeg=5)
    assert out[True][1]['area'].shape[2] == 4


def test_date_line_mlat_mlt():
    from auromat_amd import resample as R
    from auromat_amd.mapping.mapping import convertMappingToSM
    a, b = iss(0, 212, 142, 'iss029'), iss(1, 212, 142, 'iss029', dra=2.0)
    sm = [convertMappingToSM(m) for m in (a, b)]
    assert collection(sm).boundingBox.containsDiscontinuity and not any(m.containsPole for m in sm)
    out, _ = run_both_rules(sm, pxPerDeg=5)
    assert out[True][1]['plan']['lon_wrap'] == 1
    geo = R.resampleMosaicMLatMLT(collection([a, b]), pxPerDeg=5, statistic='area')
    want = out[True][2]
    assert np.array_equal(ma.filled(geo.source, -1), want['source'])
    assert np.array_equal(np.asarray(ma.getdata(geo.img))[want['mask'] == 0], want['img'][want['mask'] == 0])
    assert geo.members == [a.identifier, b.identifier]


def test_pole():
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    from auromat_amd.synthetic import frame_image, pole_frame
    w, h = 212, 142
    hdr, cam, t = pole_frame(w, h)
    hdr2 = dict(hdr)
    hdr2['CRVAL2'] = hdr2['CRVAL2'] - 3.0
    p, q = (ArraySpacecraftMapping(hd, 110, frame_image(w, h, seed=s, dtype=np.uint8), cam, t, name,
                                   fastCenterCalculation=True).maskedByElevation(10) for hd, s, name in ((hdr, 4, 'p'), (hdr2, 5, 'q')))
    assert p.containsPole
    out, _ = run_both_rules([p, q], pxPerDeg=4)
    assert out[True][1]['plan']['pole'] and out[True][1]['contains_pole']


def test_permutation(allsky):
    from auromat_amd import resample as R
    members, out, accs = allsky
    lay = lambda p: np.flipud(p.T)
    for rule in (True, False):
        _, res, want = out[rule]
        swapped = R.mosaic_frames(collection(members[::-1], mayOverlap=rule), pxPerDeg=ALLSKY_PPD, statistic='area')
        if rule:
            with np.errstate(divide='ignore', invalid='ignore'):
                el = [lay(a[-1]).astype(np.float64) / lay(a[0]).astype(np.float64) for a in accs]
            least = O.min_weight(0.5)
            tie = (lay(accs[0][0]) >= least) & (lay(accs[1][0]) >= least) & (el[0] == el[1])
            assert np.array_equal(np.where(res['source'] >= 0, 1 - res['source'], -1)[~tie], swapped['source'][~tie])
            assert (swapped['source'][tie] == 0).all() and (res['source'][tie] == 0).all()
            same = ~tie
        else:
            same = np.ones(res['mask'].shape, bool)
            assert np.array_equal(swapped['source'] >= 0, res['source'] >= 0)
        for key in ('area', 'img', 'mask', 'coverage'):
            assert O.same_bits(swapped[key][same], res[key][same]), (rule, key)


def test_refusals_and_missing_elevation():
    from auromat_amd.mapping.mapping import GenericMapping
    from auromat_amd.resample import resampleMosaic
    sod, kev = allsky_pair()
    noel = GenericMapping(kev.lats, kev.lons, kev.latsCenter, kev.lonsCenter, None, kev.altitude, kev.img,
                          kev.cameraPosGCRS, kev.photoTime, 'no-elevation')
    with pytest.raises(ValueError, match='no-elevation'):
        resampleMosaic(collection([sod, noel], mayOverlap=True), statistic='area')
    mos = resampleMosaic(collection([sod, noel], mayOverlap=False), pxPerDeg=5, statistic='area')
    assert mos.elevation is None and (~ma.getmaskarray(mos.img)).sum() > 100
    with pytest.raises(ValueError, match='empty'):
        resampleMosaic(collection([]), statistic='area')
    for kw in (dict(statistic='area', minCoverage=1.5), dict(statistic='area', q=0.5), dict(statistic='mean', minCoverage=0.5)):
        with pytest.raises(ValueError):
            resampleMosaic(collection([sod, kev]), **kw)


class _Member(object):
    """What mosaic_frames asks of a member, around a frame that is already on the device."""
    containsPole = False
    altitude = 110

    def __init__(self, fd, box, identifier):
        self.fd, self.boundingBox, self.identifier = fd, box, identifier

    def frame(self):
        return self.fd


def test_a_cell_covered_too_often_raises_value_error():
    """Two members of 200 unit squares on one cell: each below 2^40, together above — ValueError for the union only."""
    from auromat_amd import resample as R
    from auromat_amd.frame import FrameData
    from auromat_amd.mapping.mapping import BoundingBox
    box = BoundingBox(-0.5, -0.5, 2.5, 2.5)       # at 1 px/deg: 3 x 3 cells, the middle one [0.5, 1.5] x [0.5, 1.5]
    ms = []
    for i in range(2):
        case = K.coverage_limit_case(200)
        n = case.width
        fd = FrameData.from_host(case.lat + 0.5, case.lon + 0.5, np.ones((1, n)), np.ones((1, n)), case.elev, case.img.reshape(1, n, 1))
        ms.append(_Member(fd, box, 'm%d' % i))
    with pytest.raises(ValueError, match='256 times'):
        R.mosaic_frames(collection(ms, mayOverlap=False), pxPerDeg=1, statistic='area')
    res = R.mosaic_frames(collection(ms, mayOverlap=True), pxPerDeg=1, statistic='area')
    assert res['coverage'].max() == 200.0 and (res['source'] == 0).sum() == 1 and res['mask'].sum() == 8


def test_netcdf_round_trip(tmp_path, allsky):
    from auromat_amd.export import netcdf
    from auromat_amd.mapping.netcdf import NetCDFMapping
    from auromat_amd.resample import resampleMosaic
    members, out, _ = allsky
    mos = resampleMosaic(collection(members), pxPerDeg=ALLSKY_PPD, statistic='area')
    want = out[True][2]
    assert np.array_equal(ma.getmaskarray(mos.img)[..., 0], want['mask'] == 1)
    assert np.array_equal(ma.filled(mos.source, -1), want['source'])
    path = str(tmp_path / 'mosaic_area.nc')
    netcdf.write(path, mos, includeMagCoords=False)
    back = NetCDFMapping(path)
    assert np.array_equal(np.asarray(ma.getdata(back.img)), np.asarray(ma.getdata(mos.img)))
    assert np.array_equal(ma.getmaskarray(back.img), ma.getmaskarray(mos.img))
    assert np.allclose(ma.filled(back.latsCenter, np.nan), ma.filled(mos.latsCenter, np.nan), rtol=0, atol=1e-9, equal_nan=True)
    assert back.photoTime == mos.photoTime
