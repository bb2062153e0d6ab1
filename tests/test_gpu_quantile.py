"""
Quantile binning on the MI355X through the public interface (auromat_amd.resample.resampleQuantile and its siblings,
FramePipeline) against the NumPy statement of the feature (tests/_quantile_oracle.py) applied to the mapping's own arrays:
the pixel set of the mean, np.quantile per cell and plane, bit for bit, as the camera frames happen to fill the cells.  The
tier boundaries, the key patterns and the quantiles that decide the rank rule are in tests/test_gpu_quantile_cells.py.
"""
import numpy as np
import numpy.ma as ma
import pytest

import _quantile_oracle as Q
from test_gpu_median import JPG, JPG_S, WCS, WCS_S, _ppd, _synthetic_mapping, own_arrays
from conftest import assert_counts_equal_up_to_edge_pixels

pytestmark = pytest.mark.gpu

QS = (0.25, 0.5, 0.75)
KEYS = ('quantile', 'img', 'mask', 'count')


def frame_quantile(m, qs, pxPerDeg=None, arcsecPerPx=None, min_elevation=None):
    """resample_frame_quantile with resampleQuantile's arguments (the grid comes back with it)."""
    from auromat_amd import resample as R
    pole = m.containsPole
    ppd = R.plateCarreeResolution(m.boundingBox, arcsecPerPx) if arcsecPerPx else _ppd(pxPerDeg)
    return R.resample_frame_quantile(m.frame(), m.altitude, m.boundingBox, ppd, qs, m.containsDiscontinuity, pole,
                                     min_elevation=min_elevation, outline=m.outline if pole else None)


def assert_mappings_equal_frame(mappings, res):
    assert len(mappings) == res['quantile'].shape[0] == res['img'].shape[0]
    for j, r in enumerate(mappings):
        assert np.array_equal(np.asarray(ma.getdata(r.img)), res['img'][j]), j
        assert np.array_equal(ma.getmaskarray(r.img)[..., 0], res['mask']), j
        assert np.array_equal(ma.filled(r.elevation, np.nan), res['quantile'][j, ..., -1], equal_nan=True), j


def expected(res, qs, lat, lon, keep, img, el):
    g = res['grid']
    values = np.concatenate([img.astype(np.float64), el[:, None]], axis=1)
    return Q.quantile_bins(lon, lat, values, g.xedges, g.yedges, qs, keep=keep)


def check_exact(res, qs, lat, lon, keep, img, el):
    from oracle import ref_numpy as O
    want, count = expected(res, qs, lat, lon, keep, img, el)
    assert np.array_equal(res['count'], count)
    assert np.array_equal(res['mask'], count == 0)
    assert res['quantile'].shape == want.shape
    assert res['quantile'].tobytes() == np.ascontiguousarray(want).tobytes()            # every cell and plane, bit for bit
    want_img, _ = O.finalize_image(want[..., :img.shape[1]], img.dtype)
    assert res['img'].dtype == img.dtype and np.array_equal(res['img'], want_img)
    return want, count


@pytest.fixture(scope='module')
def real_frame():
    from auromat_amd.mapping.spacecraft import getMapping
    return getMapping(JPG, WCS, altitude=110, fastCenterCalculation=True).maskedByElevation(10)


@pytest.mark.parametrize('kw', [dict(pxPerDeg=10), dict(arcsecPerPx=100)], ids=['ppd10', 'arcsec100'])
def test_reference_frame(real_frame, kw):
    from auromat_amd.mapping.mapping import BaseMapping
    from auromat_amd.resample import resampleMedian, resampleQuantile
    m = real_frame
    got = resampleQuantile(m, QS, **kw)
    assert isinstance(got, list) and len(got) == 3 and all(isinstance(r, BaseMapping) for r in got)
    res = frame_quantile(m, QS, **kw)
    assert_mappings_equal_frame(got, res)                        # three mappings in the order of q
    lat, lon, keep, img, el = own_arrays(m)
    assert img.dtype == np.uint8 and img.shape[1] == 3
    want, count = check_exact(res, QS, lat, lon, keep, img, el)
    assert (count > 0).sum() > 1000
    # 300 seeded non-empty cells against a literal np.quantile of the cell's pixels
    import _median_oracle as M
    g = res['grid']
    flat = np.where(keep, M.cell_index(lon, lat, g.xedges, g.yedges), -1)
    order = np.argsort(flat, kind='stable')
    start = np.searchsorted(flat[order], np.arange(g.nx * g.ny + 1))
    cells = np.random.RandomState(17).choice(np.flatnonzero(count.ravel() > 0), 300, replace=False)
    values = np.concatenate([img.astype(np.float64), el[:, None]], axis=1)
    quant = res['quantile'].reshape(3, -1, 4)
    for c in cells:
        pix = order[start[c]:start[c + 1]]
        assert len(pix) == count.ravel()[c]
        lit = np.quantile(values[pix], QS, axis=0)
        assert quant[:, c].tobytes() == np.ascontiguousarray(lit).tobytes(), c
    # the quartiles are ordered and not all equal; the 0.5 image is resampleMedian's
    assert (res['img'][0] <= res['img'][1]).all() and (res['img'][1] <= res['img'][2]).all()
    assert (res['img'][0] < res['img'][2]).any()
    med = resampleMedian(m, **kw)
    assert np.array_equal(np.asarray(ma.getdata(med.img)), np.asarray(ma.getdata(got[1].img)))
    assert np.array_equal(ma.getmaskarray(med.img), ma.getmaskarray(got[1].img))
    # a scalar q gives a mapping: the one the list holds
    one = resampleQuantile(m, 0.75, **kw)
    assert isinstance(one, BaseMapping)
    assert np.array_equal(np.asarray(ma.getdata(one.img)), np.asarray(ma.getdata(got[2].img)))
    assert np.array_equal(ma.filled(one.elevation, np.nan), ma.filled(got[2].elevation, np.nan), equal_nan=True)


def test_date_line_mlat_mlt():
    """The southern reference frame on the MLat / MLT grid: its SM box crosses +-180 deg."""
    from oracle import ref_numpy as O
    from auromat_amd.mapping.mapping import convertMappingToSM
    from auromat_amd.mapping.spacecraft import getMapping
    from auromat_amd.resample import resampleQuantileMLatMLT
    m = getMapping(JPG_S, WCS_S, altitude=110, fastCenterCalculation=True).maskedByElevation(10)
    qs = (0.1, 0.9)
    got = resampleQuantileMLatMLT(m, qs, pxPerDeg=10)
    assert isinstance(got, list) and len(got) == 2
    sm = convertMappingToSM(m)
    assert sm.containsDiscontinuity and not sm.containsPole
    res = frame_quantile(sm, qs, pxPerDeg=10)
    assert_mappings_equal_frame(got, res)
    one = resampleQuantileMLatMLT(m, 0.9, pxPerDeg=10)
    assert np.array_equal(np.asarray(ma.getdata(one.img)), res['img'][1])
    # the oracle wraps the longitudes itself (~1e-11 deg from the device's): counts equal up to pixels on an edge, quantiles
    # bit-equal in every other cell
    lat, lon, keep, img, el = own_arrays(sm)
    lon = O.wrap_at(lon + 180, 180)
    want, count = expected(res, qs, lat, lon, keep, img, el)
    g = res['grid']
    ref = dict(count=count, lat=np.repeat(g.yedges[::-1][:, None], g.nx + 1, 1), lon=np.repeat(g.xedges[None], g.ny + 1, 0))
    assert_counts_equal_up_to_edge_pixels(ref, res['count'], np.where(keep, lat, np.nan), np.where(keep, lon, np.nan),
                                          'date line')
    same = res['count'] == count
    assert (count > 0).sum() > 50 and same.mean() > 0.99
    assert np.array_equal(res['quantile'][:, same], want[:, same], equal_nan=True)


def test_collection():
    from auromat_amd.mapping.mapping import MappingCollection
    from auromat_amd.resample import resampleQuantile
    a = _synthetic_mapping(530, 354, np.uint16, 3, seed=1)
    b = _synthetic_mapping(530, 354, np.uint16, 3, seed=2, pointing='iss029')
    qs = (0.9, 0.25)
    colls = resampleQuantile(MappingCollection([a, b], 'pair'), qs, pxPerDeg=5)
    assert isinstance(colls, list) and len(colls) == 2
    for j, coll in enumerate(colls):
        assert isinstance(coll, MappingCollection) and len(coll.mappings) == 2 and coll.identifier == 'pair'
        for m, got in zip((a, b), coll.mappings):
            one = resampleQuantile(m, qs[j], pxPerDeg=5)
            assert np.array_equal(np.asarray(ma.getdata(one.img)), np.asarray(ma.getdata(got.img)))
            assert np.array_equal(ma.filled(one.elevation, np.nan), ma.filled(got.elevation, np.nan), equal_nan=True)
    single = resampleQuantile(MappingCollection([a, b], 'pair'), 0.25, pxPerDeg=5)
    assert isinstance(single, MappingCollection) and len(single.mappings) == 2
    # uint16 frames against the oracle, every cell
    res = frame_quantile(a, qs, pxPerDeg=5)
    check_exact(res, qs, *own_arrays(a))


def test_no_pixel_survives():
    m = _synthetic_mapping(530, 354, np.uint8, 3)
    res = frame_quantile(m, QS, pxPerDeg=10, min_elevation=91.0)
    assert res['quantile'].shape[0] == 3 and res['mask'].all() and res['mask'].size > 10
    assert (res['count'] == 0).all()
    assert np.isnan(res['quantile']).all()
    assert (res['img'] == 0).all()


def test_two_calls_give_the_same_bits():
    m = _synthetic_mapping(1060, 708, np.uint16, 3, seed=7)
    r1, r2 = frame_quantile(m, QS, pxPerDeg=1), frame_quantile(m, QS, pxPerDeg=1)
    assert r1['count'].max() > 1000
    for k in KEYS:
        assert np.asarray(r1[k]).tobytes() == np.asarray(r2[k]).tobytes(), k


def test_frame_pipeline_equals_the_class_api():
    from auromat_amd.pipeline import FramePipeline
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    from auromat_amd.resample import resampleQuantile
    from auromat_amd.synthetic import frame_header, frame_image
    w, h = 1060, 708
    hdr, cam, t = frame_header(w, h, 'iss030')
    img = frame_image(w, h, seed=3, dtype=np.uint16)
    m = ArraySpacecraftMapping(hdr, 110, img, cam, t, 'n', fastCenterCalculation=True).maskedByElevation(10)
    want = resampleQuantile(m, 0.9, pxPerDeg=10)
    pipe = FramePipeline(w, h)
    res = pipe.run(hdr, 110, cam, t, img=img, min_elevation=10, pxPerDeg=10, statistic='quantile', q=0.9)
    assert res['quantile'].shape[0] == 1 and res['img'].shape[0] == 1
    assert np.array_equal(res['img'][0], np.asarray(ma.getdata(want.img)))
    assert np.array_equal(res['mask'], ma.getmaskarray(want.img)[..., 0])
    assert np.array_equal(res['quantile'][0, ..., -1], ma.filled(want.elevation, np.nan), equal_nan=True)
    # q goes with the statistic
    with pytest.raises(AssertionError):
        pipe.resample(10, statistic='quantile')
    with pytest.raises(AssertionError):
        pipe.resample(10, statistic='median', q=0.5)
    with pytest.raises(ValueError):
        pipe.resample(10, statistic='quantile', q=1.5)
