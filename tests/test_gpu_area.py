"""
Area-weighted resampling on the MI355X (auromat_amd.resample.resampleArea, resample_frame_area) on real geometry: every cell of
every output bit for bit against the NumPy statement of the feature (tests/_area_oracle.py).  The oracle runs on the coordinates
the device actually binned — rotated corners are read back — so the last bits of the trigonometry do not enter.  The kernels'
paths, the skip rules and the limits that no frame controls are in tests/test_gpu_area_cells.py.
"""
import numpy as np
import numpy.ma as ma
import pytest

import _area_cases as K
import _area_oracle as O
from conftest import load_golden

pytestmark = pytest.mark.gpu

OUT_KEYS = ('area', 'img', 'mask', 'coverage')


def _host(t):
    return None if t is None else t.cpu().numpy()


def binned_case(fd, res, altitude, pole, disc, min_elevation):
    """The frame as the device binned it, as an oracle case on the grid of the result."""
    from auromat_amd import resample as R
    lat, lon, lat_c = fd.lat, fd.lon, fd.lat_c
    if pole:
        lat, lon = R._rotate_pole_dev(fd.ctx, fd.lat, fd.lon, altitude, 90)
        lat_c, _ = R._rotate_pole_dev(fd.ctx, fd.lat_c, fd.lon_c, altitude, 90)
    g = res['grid']
    img = fd.host_image()
    return K.AreaCase('frame', _host(lat), _host(lon), g.xedges, g.yedges, lat_c=_host(lat_c), elev=_host(fd.elev),
                      mask=_host(fd.center_mask), min_elevation=float('-inf') if min_elevation is None else min_elevation,
                      lon_wrap=1 if (disc and not pole) else 0, img=img.reshape(fd.height * fd.width, -1))


def check_frame(fd, altitude, box, ppd, disc=False, pole=False, min_elevation=None, outline=None, minCoverage=0.5):
    from auromat_amd import resample as R
    res = R.resample_frame_area(fd, altitude, box, (ppd, ppd), disc, pole, min_elevation=min_elevation, outline=outline,
                                minCoverage=minCoverage)
    case = binned_case(fd, res, altitude, pole, disc, min_elevation)
    acc, hits = O.accumulate(case)
    want = O.finalize(acc, case.img.dtype, minCoverage)
    assert res['mask'].dtype == bool and res['img'].dtype == case.img.dtype
    got = dict(res, mask=res['mask'].astype(np.uint8))
    for key in OUT_KEYS:
        assert O.same_bits(got[key], want[key]), key
    assert res['lat_c'].shape == res['mask'].shape == case.shape
    return res, want, acc, hits


def golden_frame(name, magnetic=False, min_elevation=10.0):
    """(FrameData, box) of a golden georeferenced frame with a seeded image; magnetic: its MLat / SM longitude arrays."""
    from auromat_amd.frame import FrameData
    from auromat_amd.mapping.mapping import BoundingBox
    z = load_golden(name)
    if magnetic:
        to_lon = lambda mlt: (mlt - 12) / (24 / 360)
        lat, lon, lat_c, lon_c = z['mlat'], to_lon(z['mlt']), z['mlat_c'], to_lon(z['mlt_c'])
    else:
        lat, lon, lat_c, lon_c = z['lat'], z['lon'], z['lat_c'], z['lon_c']
    h, w = lat_c.shape
    img = np.random.RandomState(11).randint(0, 256, (h, w, 3)).astype(np.uint8)
    fd = FrameData.from_host(lat, lon, lat_c, lon_c, z['elev'], img)
    with np.errstate(invalid='ignore'):
        keep = np.isfinite(lat_c) & (z['elev'] >= min_elevation)
    corner = np.zeros(lat.shape, dtype=bool)
    for dr in (0, 1):
        for dc in (0, 1):
            corner[dr:dr + h, dc:dc + w] |= keep
    corner &= np.isfinite(lat) & np.isfinite(lon)
    la, lo = lat[corner], lon[corner]
    if lo.max() - lo.min() > 180:
        box = BoundingBox(la.min(), lo[lo > 0].min(), la.max(), lo[lo <= 0].max())
    else:
        box = BoundingBox(la.min(), lo.min(), la.max(), lo.max())
    return fd, float(z['altitude']), box, keep


@pytest.mark.parametrize('ppd', [10, 2])
def test_geographic_frame(ppd):
    fd, altitude, box, keep = golden_frame('georef_small_iss030_fast.npz')
    res, want, acc, hits = check_frame(fd, altitude, box, ppd, min_elevation=10.0)
    assert keep.sum() == 5951 and (want['mask'] == 0).sum() > (1000 if ppd == 10 else 100)
    if ppd == 10:
        # the hole the feature closes: fully covered cells that hold no pixel centre
        case = K.golden_case(load_golden('georef_small_iss030_fast.npz'), ppd)
        assert np.array_equal(case.xedges, res['grid'].xedges) and np.array_equal(case.yedges, res['grid'].yedges)
        centre = K.centre_counts(case, load_golden('georef_small_iss030_fast.npz')['lon_c'])
        filled = np.flipud((acc[0] >= O.min_weight(0.5)).T)
        assert np.array_equal(~res['mask'], filled) and (filled & np.flipud((centre == 0).T)).sum() > 1000


def test_magnetic_frame_across_the_date_line():
    fd, altitude, box, keep = golden_frame('georef_small_iss029_fast.npz', magnetic=True)
    assert box.containsDiscontinuity and box.lonWest > 0 > box.lonEast
    res, want, acc, hits = check_frame(fd, altitude, box, 10, disc=True, min_elevation=10.0)
    assert (want['mask'] == 0).sum() > 500
    # pixels on both sides of +-180 deg took part
    lon_c = fd.lon_c.cpu().numpy()
    assert (lon_c[keep] > 170).any() and (lon_c[keep] < -170).any()


def _mapping(w=128, h=96, seed=3, pointing='iss030', dtype=np.uint16, pole=False):
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    from auromat_amd.synthetic import frame_header, frame_image, pole_frame
    hdr, cam, t = pole_frame(w, h) if pole else frame_header(w, h, pointing)
    return ArraySpacecraftMapping(hdr, 110, frame_image(w, h, seed=seed, dtype=dtype), cam, t, 'n', fastCenterCalculation=True)


def test_pole_frame():
    m = _mapping(pole=True, dtype=np.uint8).maskedByElevation(10)
    assert m.containsPole
    res, want, acc, hits = check_frame(m.frame(), m.altitude, m.boundingBox, 10, m.containsDiscontinuity, True, outline=m.outline)
    assert (want['mask'] == 0).sum() > 500


# ---- the class API -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def masked():
    return _mapping().maskedByElevation(10)


def test_resample_area_equals_oracle_on_the_grid_of_resample(masked):
    from auromat_amd import resample as R
    r = R.resampleArea(masked, pxPerDeg=10)
    mean = R.resample(_mapping().maskedByElevation(10), pxPerDeg=10)
    assert np.array_equal(ma.getdata(r.lats), ma.getdata(mean.lats)) and np.array_equal(ma.getdata(r.lons), ma.getdata(mean.lons))
    m = masked
    res, want, acc, hits = check_frame(m.frame(), m.altitude, m.boundingBox, 10, m.containsDiscontinuity, m.containsPole)
    valid = want['mask'] == 0
    assert valid.sum() > 500
    assert np.array_equal(~ma.getmaskarray(r.img)[..., 0], valid)
    assert np.array_equal(np.asarray(ma.getdata(r.img))[valid], want['img'][valid])
    assert np.array_equal(ma.filled(r.elevation, np.nan), want['area'][..., -1], equal_nan=True)
    # with minCoverage=0 every cell that the mean fills is filled
    r0 = R.resampleArea(masked, pxPerDeg=10, minCoverage=0)
    filled0, filled_mean = ~ma.getmaskarray(r0.img)[..., 0], ~ma.getmaskarray(mean.img)[..., 0]
    assert not (filled_mean & ~filled0).any() and filled0.sum() > filled_mean.sum()
    assert not (valid & ~filled0).any()


def test_mlat_mlt_collection_errors_and_determinism(masked):
    from auromat_amd import resample as R
    from auromat_amd.mapping.mapping import MappingCollection
    geo = R.resampleAreaMLatMLT(masked, pxPerDeg=10)
    geo.checkGuarantees()
    assert (~ma.getmaskarray(geo.img)[..., 0]).sum() > 500
    other = _mapping(seed=5, pointing='iss029').maskedByElevation(10)
    coll = R.resampleArea(MappingCollection([masked, other], 'pair'), pxPerDeg=5)
    assert isinstance(coll, MappingCollection) and len(coll.mappings) == 2
    one = R.resampleArea(other, pxPerDeg=5)
    assert np.array_equal(np.asarray(ma.getdata(one.img)), np.asarray(ma.getdata(coll.mappings[1].img)))
    for bad in (1.5, -0.1, float('nan')):
        with pytest.raises(ValueError):
            R.resampleArea(masked, minCoverage=bad)
    with pytest.raises(ValueError):
        R.resampleAreaMLatMLT(masked, minCoverage=1.5)
    with pytest.raises(NotImplementedError):
        R.resample(masked, method='area')          # the method list stays the reference's
    m = masked
    runs = [R.resample_frame_area(m.frame(), m.altitude, m.boundingBox, (10, 10), m.containsDiscontinuity, m.containsPole)
            for _ in range(2)]
    for key in OUT_KEYS:
        assert np.asarray(runs[0][key]).tobytes() == np.asarray(runs[1][key]).tobytes(), key


def test_a_cell_covered_too_often_raises_value_error():
    """257 unit squares on one cell: sum(W) passes 2^40, the library says AMT_EDOMAIN and Python raises ValueError; 256 pass."""
    from auromat_amd import resample as R
    from auromat_amd.frame import FrameData
    from auromat_amd.mapping.mapping import BoundingBox
    box = BoundingBox(-0.5, -0.5, 2.5, 2.5)       # at 1 px/deg: 3 x 3 cells, the middle one [0.5, 1.5] x [0.5, 1.5]
    for n in (256, 257):
        case = K.coverage_limit_case(n)
        lat, lon = case.lat + 0.5, case.lon + 0.5
        fd = FrameData.from_host(lat, lon, np.ones((1, n)), np.ones((1, n)), case.elev, case.img.reshape(1, n, 1))
        if n == 256:
            res = R.resample_frame_area(fd, 110, box, (1, 1))
            assert res['mask'].shape == (3, 3) and res['coverage'][1, 1] == 256.0 and (~res['mask']).sum() == 1
        else:
            with pytest.raises(ValueError):
                R.resample_frame_area(fd, 110, box, (1, 1))
