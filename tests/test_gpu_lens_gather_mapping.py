"""
The raw route's inverse in the mapping layer on the MI355X: ``getMapping(..., lens=, lensRoute='raw')`` mappings answer
``latLonToPixel`` & co. in raw pixels, are gathered through their lens by ``resampleGather*`` and ``resampleGatherMosaic``, and
``auromat-convert --gather ... --lens-route fused`` writes what the class API gives.

Round trip.  The corner ``lats`` / ``lons`` of a raw-route mapping (raw pixel corner -> ``amt_lens_undistort`` -> the TAN model
-> shell -> one-step Bowring latitude) go back through ``latLonToPixel`` (exact latitude -> the TAN model -> the lens forward)
and must land on (column - 0.5, row - 0.5) within
    M x (_inverse_cases.bowring_residual() + ACCURACY_PX) + 1e-9 px
where bowring_residual() + ACCURACY_PX is what tests/test_gpu_inverse_points.py holds the camera model's own round trip to, M is the
largest of |g| and |d(r g)/dr| over the tested corners (tests/_lens_oracle.py: how much the lens forward stretches an error of
the corrected frame, tangentially and radially), and 1e-9 px is what tests/test_gpu_lens_cells.py holds the Newton inverse to.
Measured on the MI355X: see the printed figures (-s).
"""
import json
import os

import numpy as np
import numpy.ma as ma
import pytest

import _inverse_cases as IC
import _lens_cases as K
import _lens_oracle as LO

pytestmark = pytest.mark.gpu

ACCURACY_PX = 4 * 2.160e-11        # tests/test_gpu_inverse_points.py
W, H = 131, 67


def _header(w, h, k=0):
    from auromat_amd.synthetic import sequence_frame
    hdr, cam, t, _ = sequence_frame(k, w, h)
    hdr = dict(hdr)
    hdr.update({'DATE-OBS': t.strftime('%Y-%m-%dT%H:%M:%S.%f'), 'POSX': float(cam[0]), 'POSY': float(cam[1]), 'POSZ': float(cam[2])})
    return hdr


def _lens(name, w=W, h=H):
    from auromat_amd.util.lensdistortion import LensModifier
    model, params = K.MODELS[name]
    return LensModifier(model, list(params), w, h)


def _raw_image(seed=7, w=W, h=H):
    from auromat_amd.synthetic import frame_image
    return frame_image(w, h, seed=seed)


def _raw_mapping(name, crop, w=W, h=H, k=0, seed=7, **kw):
    from auromat_amd.mapping.spacecraft import getMapping
    mod = _lens(name, w, h)
    cw, ch = mod.cropped(crop).corrected_size if crop else (w, h)
    return getMapping(_raw_image(seed, w, h), _header(cw, ch, k), lens=mod, lensRoute='raw', cropDivisibleBy=crop,
                      identifier='raw-%s-%d' % (name, k), **kw)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def round_trip_bound(name, cols, rows):
    """(M, bound [px]) of the docstring for the raw pixel corners (cols - 0.5, rows - 0.5) of a W x H frame with lens `name`"""
    model, params = K.MODELS[name]
    X, Y = LO.inverse_newton(model, list(params), W, H, cols - 0.5, rows - 0.5)
    cx, cy, norm = LO.constants(W, H)
    r = np.hypot((X - cx) * norm, (Y - cy) * norm)
    p = LO.radial_poly(model, list(params))
    slope = sum(k * p[k] * r ** (k - 1) for k in range(1, len(p)))
    M = float(max(np.abs(LO.g_of(model, list(params), r * r)).max(), np.abs(slope).max()))
    return M, M * (IC.bowring_residual() + ACCURACY_PX) + 1e-9


# ---- round trip ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,crop', [(n, c) for n in K.REALISTIC for c in (None, 17)])       # (131 x 67 cropped to 119 x 51)
def test_corners_round_trip_through_lat_lon_to_pixel(name, crop):
    from auromat_amd.coordinates.inverse import NOT_SEEN
    m = _raw_mapping(name, crop)
    lats, lons = m.lats, m.lons
    assert lats.shape == (H + 1, W + 1)
    seen = ~ma.getmaskarray(lats)
    assert seen.sum() > 1000
    rows, cols = np.nonzero(seen)
    x, y, flags = m.latLonToPixel(ma.getdata(lats)[seen], ma.getdata(lons)[seen], returnFlags=True)
    # masked both ways: a corner the mapping shows is seen by its inverse
    assert not (flags & NOT_SEEN).any() and not ma.getmaskarray(x).any() and not ma.getmaskarray(y).any()
    d = np.hypot(ma.getdata(x) - (cols - 0.5), ma.getdata(y) - (rows - 0.5))
    # how much the lens forward stretches an error of the corrected frame at these corners, from the oracle
    M, bound = round_trip_bound(name, cols, rows)
    print('%s crop %s: %d corners, largest distance %.3e px, M = %.4f, bound %.3e px' % (name, crop, len(d), d.max(), M, bound))
    assert 0.9 < M < 1.2 and d.max() <= bound


def test_corners_without_an_inverse_are_masked_and_the_rest_is_seen():
    """model 'fold': the raw corners beyond the fold's image have no place in the corrected frame (masked in the mapping); the
    corners the mapping shows come back without LENS_FOLD"""
    from auromat_amd.coordinates.inverse import LENS_FOLD, NOT_SEEN
    m = _raw_mapping('fold', None)
    model, params = K.MODELS['fold']
    x, y = LO.lattice(W, H, True)
    X, _ = LO.inverse_newton(model, list(params), W, H, x, y)
    hole = np.isnan(X)
    seen = ~ma.getmaskarray(m.lats)
    assert hole.any() and not seen[hole].any() and seen.sum() > 500
    px, py, flags = m.latLonToPixel(ma.getdata(m.lats)[seen], ma.getdata(m.lons)[seen], returnFlags=True)
    rows, cols = np.nonzero(seen)
    d = np.hypot(ma.getdata(px) - (cols - 0.5), ma.getdata(py) - (rows - 0.5))
    ok = (flags & NOT_SEEN) == 0
    M, bound = round_trip_bound('fold', cols[ok], rows[ok])
    print('fold: %d corners seen, %d of them come back; largest distance %.3e px, M = %.4f, bound %.3e px'
          % (seen.sum(), ok.sum(), d[ok].max(), M, bound))
    # (a corner within rounding of the fold may fall on its far side on the way back; the others must come back, within the
    # round trip's bound: g = 1 - k1 = 1.45 at the centre is this model's M, the slope goes to 0 towards the fold)
    assert ok.sum() >= seen.sum() - 4 and ((flags[~ok] & LENS_FOLD) != 0).all() and 1.4 < M < 1.5 and d[ok].max() <= bound
    # a point far outside the corrected frame would be mapped back into the raw frame by the polynomial: LENS_FOLD instead
    lat, lon = ma.getdata(m.lats)[seen], ma.getdata(m.lons)[seen]
    far = m.latLonToPixel(lat[:1] + 3.0, lon[:1], returnFlags=True)
    assert far[2][0] & (LENS_FOLD | NOT_SEEN) and ma.getmaskarray(far[0])[0] == bool(far[2][0] & NOT_SEEN)


def test_mlat_mlt_ra_dec_and_the_graticule():
    from auromat_amd.draw import graticulePixels
    m = _raw_mapping('ptlens', 17)
    mlat, mlt = m.mLatMlt
    seen = ~ma.getmaskarray(mlat)
    rows, cols = np.nonzero(seen)
    pick = slice(None, None, 37)
    x, y = m.mLatMltToPixel(ma.getdata(mlat)[seen][pick], ma.getdata(mlt)[seen][pick])
    d = np.hypot(ma.getdata(x) - (cols[pick] - 0.5), ma.getdata(y) - (rows[pick] - 0.5))
    M, bound = round_trip_bound('ptlens', cols[pick], rows[pick])
    print('MLat / MLT of %d corners back to their pixels: largest distance %.3e px, bound %.3e px' % (len(d), d.max(), bound))
    assert not ma.getmaskarray(x).any() and d.max() <= bound          # (the round trip's bound: no Bowring step on this way)
    # stars: a direction of the header's own sky goes through the lens as well
    from auromat_amd.coordinates.wcs import tan_pix2world
    hdr = m._cameraHeader
    ra, dec = tan_pix2world(hdr, np.array([60.0]), np.array([5.0]), 0)
    sx, sy, fl = m.raDecToPixel(ra, dec, returnFlags=True)
    mod = m._cameraLens
    want_x, want_y = LO.forward(mod.model, mod.params, W, H, np.array([60.0 + mod.crop[0]]), np.array([5.0 + mod.crop[1]]))
    assert abs(float(ma.getdata(sx)[0]) - want_x[0]) < 1e-8 and abs(float(ma.getdata(sy)[0]) - want_y[0]) < 1e-8
    par, mer = graticulePixels(m, every=2, step=0.2)
    assert par and mer
    from auromat_amd.draw import graticule_lines
    parallels, meridians = graticule_lines(m.boundingBox, 2, 0.2)
    for lines, got in ((parallels, par), (meridians, mer)):
        for deg, la, lo in lines:
            x, y = m.latLonToPixel(la, lo)
            want = np.stack((x.filled(np.nan), y.filled(np.nan)), axis=-1)
            assert same_bits(got[deg], want), deg
    inside = [v for v in par.values() if np.isfinite(v).all(axis=1).any()]
    assert inside


# ---- gathering raw-route mappings -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('magnetic', [False, True])
def test_resample_gather_is_gather_frame_on_its_plan(magnetic):
    from auromat_amd.resample import gather_frame, gather_plan, resampleGather, resampleGatherMLatMLT
    m = _raw_mapping('poly5', 17).maskedByElevation(5)
    fn = resampleGatherMLatMLT if magnetic else resampleGather
    plan = gather_plan(m, pxPerDeg=12, magnetic=magnetic)
    assert plan['lens'] is not None and (plan['lens'].width, plan['lens'].height, plan['lens'].crop_width) == (W, H, 119)
    assert (plan['params'].width, plan['params'].height) == (W, H) and plan['center_mask'] is not None
    for interpolation, n in (('linear', 1), ('lanczos4', 1), ('nearest', 1), ('linear', 3)):
        got = fn(m, pxPerDeg=12, interpolation=interpolation, supersample=n)
        want = gather_frame(plan, m._img_array, interpolation, magnetic, n)
        assert same_bits(ma.getdata(got.img)[~want['mask']], want['img'][~want['mask']]), (interpolation, n)
        assert np.array_equal(ma.getmaskarray(got.img)[..., 0], want['mask'])
        assert 0 < want['mask'].sum() < want['mask'].size
        if n > 1:
            assert np.array_equal(got.coverage, want['count'] / 9.0)


def test_identity_lens_gathers_what_the_resample_route_gathers():
    from auromat_amd.mapping.spacecraft import getMapping
    from auromat_amd.resample import resampleGather
    hdr, raw, mod = _header(W, H), _raw_image(), _lens('identity')
    a = getMapping(raw, hdr, lens=mod, lensRoute='resample', fastCenterCalculation=True)
    b = getMapping(raw, hdr, lens=mod, lensRoute='raw', fastCenterCalculation=True)
    assert b._inverse_lens() is not None and a._inverse_lens() is None
    # (the raw route's plan comes from its arrays, centre mask included: the resample route's arrays are asked for as well, so
    # that both mappings are planned the same way)
    assert a.lats.shape == b.lats.shape
    for interpolation, n in (('linear', 1), ('lanczos4', 1), ('linear', 2)):
        ga = resampleGather(a, pxPerDeg=12, interpolation=interpolation, supersample=n)
        gb = resampleGather(b, pxPerDeg=12, interpolation=interpolation, supersample=n)
        if ga.img.shape != gb.img.shape:
            pytest.fail('the two routes laid out different grids: %r, %r' % (ga.img.shape, gb.img.shape))
        assert np.array_equal(ma.getmaskarray(ga.img), ma.getmaskarray(gb.img)), (interpolation, n)
        assert same_bits(ga.img.filled(0), gb.img.filled(0)), (interpolation, n)
        assert same_bits(ga.elevation.filled(0.0), gb.elevation.filled(0.0))


def test_resample_gather_mosaic_mixes_members_with_and_without_a_lens():
    from auromat_amd.mapping.mapping import MappingCollection
    from auromat_amd.mapping.spacecraft import getMapping
    from auromat_amd.resample import gather_mosaic_frames, gather_mosaic_plan, resampleGatherMosaic
    members = [_raw_mapping('poly3', None, k=0, seed=1), getMapping(_raw_image(2), _header(W, H, 1), fastCenterCalculation=True,
                                                                    identifier='plain'),
               _raw_mapping('ptlens', None, k=2, seed=3)]
    coll = MappingCollection(members, 'mixed', mayOverlap=True)
    plan = gather_mosaic_plan(coll, pxPerDeg=8)
    assert [m['lens'] is not None for m in plan['members']] == [True, False, True]
    for interpolation, n in (('linear', 1), ('lanczos4', 2)):
        got = resampleGatherMosaic(coll, pxPerDeg=8, interpolation=interpolation, supersample=n)
        want = gather_mosaic_frames(plan, None, interpolation, supersample=n)
        assert np.array_equal(ma.getmaskarray(got.img)[..., 0], want['mask'])
        assert same_bits(ma.getdata(got.img)[~want['mask']], want['img'][~want['mask']])
        assert len(set(np.unique(want['source']).tolist()) - {-1}) >= 2


def test_convert_gathers_through_the_lens(tmp_path):
    """auromat-convert --gather linear --lens-route fused over two raw .npy frames: the files hold the arrays of the class API"""
    from auromat_amd.cli.convert import main
    from auromat_amd.mapping.netcdf import read_arrays
    from auromat_amd.mapping.spacecraft import getMapping
    from auromat_amd.resample import resampleGather
    w, h = 264, 170                      # corrected and cropped to a multiple of 16: 256 x 160
    model, params = K.MODELS['ptlens']
    mod = _lens('ptlens', w, h)
    d = tmp_path / 'frames'
    d.mkdir()
    for k in range(2):
        (d / ('raw%02d.json' % k)).write_text(json.dumps(_header(256, 160, k)))
        np.save(str(d / ('raw%02d.npy' % k)), _raw_image(seed=40 + k, w=w, h=h))
    out = str(tmp_path / 'fused')
    main(['--data', str(d), '--format', 'netcdf', '--lens-model', model, '--lens-params'] + [repr(p) for p in params] +
         ['--crop-divisible-by', '16', '--resample', '--gather', 'linear', '--px-per-deg', '12', '--grid', 'geo', '--lens-route', 'fused',
          '--out', out])
    assert sorted(os.listdir(out)) == ['raw00.nc', 'raw01.nc']
    for k in range(2):
        hdr = json.loads((d / ('raw%02d.json' % k)).read_text())
        m = getMapping(np.load(str(d / ('raw%02d.npy' % k))), hdr, fastCenterCalculation=True, lens=mod, lensRoute='raw',
                       cropDivisibleBy=16, identifier='raw%02d' % k)
        want = resampleGather(m, pxPerDeg=12, interpolation='linear')
        got = read_arrays(os.path.join(out, 'raw%02d.nc' % k))
        assert got['img'].shape == want.img.shape
        shown = ~ma.getmaskarray(want.lats)
        assert shown.any() and np.array_equal(ma.getdata(got['lats'])[shown], ma.getdata(want.lats)[shown])
        assert np.array_equal(got['img'].filled(0), want.img.filled(0))
        assert np.array_equal(ma.getmaskarray(got['img']), ma.getmaskarray(want.img))
        assert 0 < ma.getmaskarray(want.img).sum() < want.img.size
