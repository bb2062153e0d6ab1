"""
The gather mosaic on the host: the NumPy statement of the election (tests/_gather_mosaic_oracle.py) on hand-written cells with
known answers, the plan (its grid is mosaic_layout's for the members' boxes; every refusal comes before a device call — this
machine has no device, a device call would raise NativeError), the declared symbols, and resampleGather's unchanged refusal of
collections.
"""
import os

import numpy as np
import pytest

import _gather_mosaic_oracle as GO
import _inverse_cases as IC

N = np.nan


def test_election_on_hand_written_cells():
    #                 tie   NaN    nobody  0 < 1   only 1   NaN seen alone
    seen = np.array([[1,    1,     0,      1,      0,       1],
                     [1,    1,     0,      1,      1,       0],
                     [1,    0,     0,      0,      0,       0]], dtype=bool)
    elev = np.array([[20.,  N,     50.,    10.,    80.,     N],
                     [20.,  5.,    60.,    30.,    -2.,     70.],
                     [20.,  90.,   70.,    99.,    N,       N]])
    assert GO.elect(seen, elev, 1).tolist() == [0, 1, -1, 1, 1, -1]
    assert GO.elect(seen, elev, 0).tolist() == [0, 1, -1, 0, 1, -1]
    assert GO.elect(seen, elev, 1).dtype == np.int32
    # a tie goes to the lower index whatever the order of the others
    assert GO.elect(np.ones((3, 1), bool), np.array([[1.0], [7.0], [7.0]]), 1).tolist() == [1]
    # -inf is a number: it wins where it is alone, and loses to anything else
    assert GO.elect(np.ones((2, 2), bool), np.array([[-np.inf, -np.inf], [N, -1e300]]), 1).tolist() == [0, 1]
    # 2-d cells keep their shape
    s = GO.elect(np.ones((2, 3, 4), bool), np.stack([np.zeros((3, 4)), np.ones((3, 4))]), 1)
    assert s.shape == (3, 4) and (s == 1).all()


def test_compose_takes_the_winners_sample_and_zero_where_nobody_sees():
    a = dict(img=np.full((1, 3, 2), 7, np.uint8), mask=np.array([[False, False, True]]), elevation=np.array([[10.0, 30.0, 5.0]]))
    b = dict(img=np.full((1, 3, 2), 9, np.uint8), mask=np.array([[False, True, True]]), elevation=np.array([[20.0, 80.0, 6.0]]))
    c = GO.compose([a, b], 1)
    assert c['source'].tolist() == [[1, 0, -1]] and c['mask'].tolist() == [[False, False, True]]
    assert c['img'][0, :, 0].tolist() == [9, 7, 0] and c['img'].dtype == np.uint8
    assert c['elevation'][0, :2].tolist() == [20.0, 30.0] and np.isnan(c['elevation'][0, 2])
    assert GO.compose([a, b], 0)['source'].tolist() == [[0, 0, -1]]


class _Frame(object):
    def center_mask_tensor(self):
        return None


class _Member(object):
    """what gather_mosaic_plan asks of a member whose arrays exist"""

    def __init__(self, identifier, box, altitude=110.0, img=None, pole=False):
        from auromat_amd.mapping.mapping import BoundingBox
        self.identifier, self.altitude, self.containsPole = identifier, altitude, pole
        self.boundingBox = BoundingBox(*box)
        self._img_array = np.zeros((4, 5, 3), np.uint8) if img is None else img

    def _inverse_model(self):
        return object(), object()           # (a zenithal model: no box pass)

    def frame(self):
        return _Frame()


def _collection(members, mayOverlap=True):
    from auromat_amd.mapping.mapping import MappingCollection
    return MappingCollection(list(members), 'c', mayOverlap=mayOverlap)


@pytest.mark.parametrize('boxes', [[(40.0, 10.0, 50.0, 20.0), (45.0, 15.0, 57.3, 31.9)],
                                   [(-5.0, 170.0, 5.0, -175.0), (-2.0, 178.0, 9.0, -170.0)],          # the date line
                                   [(10.0, 0.0, 11.0, 1.0)]])
def test_plan_grid_is_the_mosaic_layout_of_the_boxes(boxes):
    from auromat_amd.resample import gather_mosaic_plan, mosaic_layout
    members = [_Member('m%d' % i, b) for i, b in enumerate(boxes)]
    for kw in (dict(pxPerDeg=10), dict(pxPerDeg=(7, 13)), dict(arcsecPerPx=400)):
        for rule in (True, False):
            plan = gather_mosaic_plan(_collection(members, rule), **kw)
            want = mosaic_layout([m.boundingBox for m in members], kw.get('pxPerDeg', 25), kw.get('arcsecPerPx'))
            g, w = plan['grid'], want['grid']
            assert (g.ny, g.nx) == (w.ny, w.nx) and g.ny > 1 and g.nx > 1
            for a in ('lat', 'lon', 'lat_c', 'lon_c'):
                assert np.array_equal(getattr(g, a), getattr(w, a)), a
            assert plan['contains_discontinuity'] == want['discontinuity'] == (boxes[0][1] > boxes[0][3])
            assert not plan['contains_pole'] and plan['rule'] == int(rule) and plan['identifiers'] == [m.identifier for m in members]
            assert len(plan['members']) == len(members) and all(m['center_mask'] is None and m['min_elevation'] is None
                                                                for m in plan['members'])
    # a list is a collection whose members may overlap
    assert gather_mosaic_plan(members, pxPerDeg=10)['rule'] == 1


#   reduction: lat_min, lat_max, lon_min, lon_max, the least positive and the largest non-positive longitude, valid pixels, poles
@pytest.mark.parametrize('red,kw,ppd,box,dateline', [
    # inside one hemisphere
    ([40.2, 50.7, 10.1, 20.3, 10.1, 0.0, 1000, 0], dict(pxPerDeg=10), (10, 10), (40.2, 50.7, 10.1, 20.3), False),
    # across the date line, 171.3 E ... 172.6 W: the grid is laid out in longitudes shifted by 180 degrees
    ([-5.5, 4.5, -179.9, 179.8, 171.3, -172.6, 1000, 0], dict(pxPerDeg=(7, 13)), (7, 13), (-5.5, 4.5, -8.7, 7.4), True),
    # a spherical resolution: px / deg from the box
    ([40.2, 50.7, 10.1, 20.3, 10.1, 0.0, 1000, 0], dict(arcsecPerPx=400), None, (40.2, 50.7, 10.1, 20.3), False)])
def test_box_grid_of_a_reduction(red, kw, ppd, box, dateline):
    from auromat_amd.mapping.mapping import BoundingBox
    from auromat_amd.resample import cached_grid, fixedGrid, gather_box_grid, plateCarreeResolution
    if ppd is None:
        ppd = plateCarreeResolution(BoundingBox(40.2, 10.1, 50.7, 20.3), 400)
        assert abs(ppd[0] - 9) < 1e-12 and 5 < ppd[1] < 7          # (3600 / 400; a degree of longitude is shorter at 45 N)
    part, used = gather_box_grid(red, kw.get('pxPerDeg'), kw.get('arcsecPerPx'))
    assert sorted(part) == ['contains_discontinuity', 'contains_pole', 'grid'] and tuple(used) == tuple(ppd)
    assert part['contains_pole'] is False and part['contains_discontinuity'] is dateline
    g, w = part['grid'], cached_grid(ppd, *box)
    nLat, nLon = fixedGrid(ppd, *box)[:2]
    assert (g.ny, g.nx) == (w.ny, w.nx) == (nLat - 2, nLon - 2) and g.ny > 1 and g.nx > 1
    for a in ('lat', 'lon', 'lat_c', 'lon_c'):
        assert np.array_equal(getattr(g, a), getattr(w, a)), a


def test_refusals_come_before_any_device_call():
    from auromat_amd.mapping.astrometry import DirectionArrayMapping
    from auromat_amd.resample import (gather_mosaic_frames, gather_mosaic_plan, resampleGatherMosaic,
                                      resampleGatherMosaicMLatMLT)
    box = (40.0, 10.0, 50.0, 20.0)
    ok = _Member('ok', box)
    for call in (resampleGatherMosaic, resampleGatherMosaicMLatMLT):
        with pytest.raises(ValueError, match='interpolation'):
            call(object(), interpolation='cubic')           # before the collection is looked at
        with pytest.raises(ValueError, match='empty'):
            call(_collection([]))
        with pytest.raises(ValueError, match='empty'):
            call([])
        with pytest.raises(ValueError, match='altitude.*high'):
            call(_collection([ok, _Member('high', box, altitude=120.0)]))
        with pytest.raises(ValueError, match='dtype or channel.*gray'):
            call(_collection([ok, _Member('gray', box, img=np.zeros((4, 5, 1), np.uint8))]))
        with pytest.raises(ValueError, match='dtype or channel.*deep'):
            call([ok, _Member('deep', box, img=np.zeros((4, 5, 3), np.uint16))])
    cam = IC.by_name('cd-rotation-37')
    dirs = np.zeros((cam['height'] + 1, cam['width'] + 1, 3))
    dirs[..., 2] = 1.0
    img = np.zeros((cam['height'], cam['width'], 3), dtype=np.uint8)
    bare = DirectionArrayMapping(dirs, 110.0, img, cam['cam'], IC.K.T0, 'bare-member')
    lens = DirectionArrayMapping(dirs, 110.0, img, cam['cam'], IC.K.T0, 'raw-member', noInverse='a raw frame with its lens distortion')
    for member, what in ((bare, 'bare-member.*direction'), (lens, 'raw-member.*lens')):
        with pytest.raises(NotImplementedError, match=what):
            resampleGatherMosaic([member])
        with pytest.raises(NotImplementedError, match=what):
            gather_mosaic_plan(_collection([member, member]), magnetic=True)
    with pytest.raises(ValueError, match='interpolation'):
        gather_mosaic_frames(dict(), interpolation='cubic')


def test_symbols_and_the_unchanged_refusal_of_resample_gather():
    from auromat_amd import _native
    from auromat_amd import resample as R
    from auromat_amd.mapping.mapping import MappingCollection
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'auromat_hip.h')).read()
    assert 'amt_gather_mosaic' in _native._SIGNATURES and 'int amt_gather_mosaic(amt_ctx* ctx' in header
    assert 'amt_gather_mosaic' in _native.exported_symbols()
    assert '#define AMT_ABI_VERSION 10' in header and _native.ABI_VERSION == 10
    for name, value in (('AMT_INTERP_LINEAR', 0), ('AMT_INTERP_LANCZOS4', 1), ('AMT_INTERP_NEAREST', 2), ('AMT_GATHER_PATH_AUTO', 0),
                        ('AMT_GATHER_PATH_STAGED', 1), ('AMT_GATHER_PATH_CELL', 2)):
        assert ('#define %s %d' % (name, value)) in header, name
    assert R._GATHER_INTERP_CODES == dict(linear=0, lanczos4=1, nearest=2) and set(R._GATHER_INTERP_CODES) == set(R.GATHER_INTERPOLATIONS)
    assert (R.GATHER_PATH_AUTO, R.GATHER_PATH_STAGED, R.GATHER_PATH_CELL) == (0, 1, 2)
    assert 'typedef struct amt_gather_member' in header and 'typedef struct amt_gather_debug' in header
    assert [f[0] for f in _native.GatherMember._fields_] == ['params', 'zenithal', 'img', 'center_mask', 'min_elevation']
    assert [f[0] for f in _native.GatherDebug._fields_] == ['force_path', 'reserved', 'tile_path']
    for name in ('gather_mosaic_plan', 'gather_mosaic_frames', 'resampleGatherMosaic', 'resampleGatherMosaicMLatMLT'):
        assert callable(getattr(R, name)), name
    # resampleGather itself still takes one mapping
    ok = _Member('ok', (40.0, 10.0, 50.0, 20.0))
    for what in ([ok], MappingCollection([ok], 'c')):
        with pytest.raises(NotImplementedError, match='collections'):
            R.resampleGather(what)
        with pytest.raises(NotImplementedError, match='collections'):
            R.resampleGatherMLatMLT(what)
