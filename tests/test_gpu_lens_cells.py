"""
The lens kernels (auromat_amd/csrc/amt_lens.hip) on the constructed cases of tests/_lens_cases.py against the statement in
tests/_lens_oracle.py: forward coordinates to 1e-10 px (float32 form: one float32 step of the cast oracle), the inverse against
mpmath to 1e-9 px where the model is well conditioned and NaN exactly where it has no inverse, and the two remap calls on EVERY
pixel of every case — equal to the oracle's rounded value, except that an output whose exact value lies in the boundary window
(tests/test_lens_cpu.py shows how few do) may differ by one count.  Each remap case runs with the taps staged in LDS and again
with the taps gathered from global memory: the two must give the same bits, and the per-tile report says which tiles took which.
"""
import numpy as np
import pytest

import _lens_cases as K
import _lens_oracle as O

pytestmark = pytest.mark.gpu

NONE, STAGED, GATHER = 0, 1, 2


def _modifier(model_name, shape, crop=None):
    from auromat_amd.util.lensdistortion import LensModifier
    model, params = K.MODELS[model_name]
    return LensModifier(model, list(params), shape[0], shape[1], crop=crop)


@pytest.mark.parametrize('case', K.coords_cases(), ids=lambda c: c[0])
def test_forward_coordinates(case):
    from auromat_amd._native import to_host
    _, name, (w, h), crop, corner = case
    model, params = K.MODELS[name]
    mod = _modifier(name, (w, h), crop)
    want = O.forward_grid(model, list(params), w, h, crop, corner)
    got = to_host(mod.forward_coordinates_device(corner=corner))
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want))
    if not np.isnan(want).all():
        err = np.nanmax(np.abs(got - want))
        print('largest coordinate error %.3e px' % err)
        assert err <= 1e-10, err
    got32 = to_host(mod.forward_coordinates_device(corner=corner, float32=True))
    want32 = want.astype(np.float32)
    assert got32.dtype == np.float32 and np.array_equal(np.isnan(got32), np.isnan(want32))
    ok = ~np.isnan(want32)
    assert (np.abs(got32[ok].astype(np.float64) - want32[ok].astype(np.float64)) <= np.spacing(np.abs(want32[ok]))).all()
    if not corner and crop is None:
        # the public form: float32 (h, w, 2) in [x, y] order like lensfunpy's, float64 on request
        a = mod.apply_geometry_distortion()
        assert a.dtype == np.float32 and a.shape == (h, w, 2) and np.array_equal(a, got32, equal_nan=True)
        assert np.array_equal(mod.apply_geometry_distortion(float64=True), got, equal_nan=True)


@pytest.mark.parametrize('case', K.undistort_cases(), ids=lambda c: c[0])
def test_undistorted_coordinates(case):
    cid, name, (w, h), crop, corner = case
    want, slope, _ = K.undistort_reference(cid)
    got = _modifier(name, (w, h), crop).undistorted_coordinates(corner=corner)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), 'NaN exactly where the model folds or a coefficient is NaN'
    good = slope >= 0.1
    if name in K.WELL_CONDITIONED:
        assert good.all()
    if good.any():
        err = np.abs(got - want)[good].max()
        print('largest error of the inverse %.3e px (smallest slope %.3f)' % (err, np.nanmin(slope[good])))
        assert err <= 1e-9, err
    if name == 'identity':
        x, y = O.lattice(w, h, corner)
        assert np.array_equal(got[..., 0], x) and np.array_equal(got[..., 1], y)


def test_centre_maps_to_centre_exactly():
    for name in ('poly3', 'poly5', 'ptlens', 'fold', 'magnify'):
        got = _modifier(name, (7, 5)).undistorted_coordinates()
        assert tuple(got[2, 3]) == (3.0, 2.0), name
    assert np.isnan(_modifier('nan', (7, 5)).undistorted_coordinates()[2, 3]).all()


def _tiles_expected(name, shape):
    """what the per-tile report must show for a case under AMT_LENS_PATH_AUTO"""
    if name == 'nan':
        return {NONE}
    if name == 'magnify' and shape == (131, 67):
        return None                      # checked on its own below: some tiles overflow the window
    return {STAGED} if name in ('identity',) + K.REALISTIC else None


@pytest.mark.parametrize('case', K.remap_cases(), ids=lambda c: c[0])
def test_remap(case):
    cid, name, (w, h), c, dtype, content, interp = case
    im, values, support, mag = K.remap_reference(cid)
    mod = _modifier(name, (w, h))
    out = {}
    for path in (STAGED, GATHER):
        got, sup, tiles = mod.remap(im, interp, support=True, force_path=path, tile_path=True)
        assert got.dtype == im.dtype and got.shape == im.shape
        bad = O.compare(got, values, dtype, mag)
        differ = int((got != O.convert(values, dtype)).sum())
        print('%s path %d: %d of %d outputs differ from the oracle (all inside the boundary window: %s)'
              % (cid, path, differ, got.size, bad == 0))
        assert bad == 0, '%d outputs break the rule' % bad
        assert np.array_equal(sup, support), 'support'
        if path == GATHER:
            assert set(np.unique(tiles)) <= {NONE, GATHER}
        else:
            expected = _tiles_expected(name, (w, h))
            assert expected is None or set(np.unique(tiles)) == expected, np.unique(tiles)
        out[path] = got
    assert out[STAGED].tobytes() == out[GATHER].tobytes(), 'the two paths must give the same bits'
    # the default (no debug block) is the staged plan
    assert mod.remap(im, interp).tobytes() == out[STAGED].tobytes()
    if name == 'identity':
        assert out[STAGED].tobytes() == im.tobytes()

    # the same through a coordinate array made elsewhere (float32, as lensfunpy hands them out)
    from auromat_amd.util.lensdistortion import remap
    model, params = K.MODELS[name]
    xy32 = O.forward_grid(model, list(params), w, h).astype(np.float32)
    v32, s32 = O.sample(im, xy32[..., 0].astype(np.float64), xy32[..., 1].astype(np.float64), interp)
    m32 = O.sample(im, xy32[..., 0].astype(np.float64), xy32[..., 1].astype(np.float64), interp, absolute=True)[0] \
        if mag is not None else None
    both = []
    for path in (STAGED, GATHER):
        got, sup = remap(im, xy32, interp, support=True, force_path=path)
        assert O.compare(got, v32, dtype, m32) == 0 and np.array_equal(sup, s32)
        both.append(got)
    assert both[0].tobytes() == both[1].tobytes()


def test_magnified_tiles_leave_the_window():
    """Under the automatic plan the strongly magnifying model sends the tiles whose taps do not fit the staging window to the gather
    path and keeps the others staged; the image is the same as with everything gathered."""
    im = K.image(131, 67, 3, np.uint16, 'random')
    mod = _modifier('magnify', (131, 67))
    auto, tiles = mod.remap(im, 'lanczos4', tile_path=True)
    assert GATHER in tiles and tiles.shape == (3, 5), tiles
    small = _modifier('magnify', (7, 5)).remap(K.image(7, 5, 3, np.uint16, 'random'), 'lanczos4', tile_path=True)[1]
    assert small.tolist() == [[STAGED]]
    gathered = mod.remap(im, 'lanczos4', force_path=GATHER)
    assert auto.tobytes() == gathered.tobytes()


def test_arbitrary_coordinates_and_other_sizes():
    """amt_remap_coords with a destination of another size than the source, coordinates in no order (every tile gathers), NaN and
    far-away points, a 2-dimensional image"""
    from auromat_amd.util.lensdistortion import remap
    rng = np.random.default_rng(5)
    im = K.image(33, 33, 1, np.uint8, 'random')[:, :, 0]
    xy = (rng.random((41, 70, 2)) * 40 - 4).astype(np.float32)
    xy[3, 5] = np.nan
    xy[4, 6] = (1e30, 2.0)
    xy[5, 7] = (np.inf, -np.inf)
    for interp in ('linear', 'lanczos4'):
        values, support = O.sample(im, xy[..., 0].astype(np.float64), xy[..., 1].astype(np.float64), interp)
        got, sup, tiles = remap(im, xy, interp, support=True, tile_path=True)
        assert got.shape == (41, 70) and got.dtype == np.uint8
        assert O.compare(got[:, :, None], values, np.uint8) == 0 and np.array_equal(sup, support)
        assert got[3, 5] == 0 and got[4, 6] == 0 and got[5, 7] == 0 and not sup[3, 5]
        assert tiles.shape == (2, 3)


def test_device_tensor_in_and_out():
    import torch
    from auromat_amd._native import Context
    im = K.image(132, 68, 3, np.uint16, 'random')
    mod = _modifier('poly5', (132, 68)).cropped(16)
    assert mod.crop == (2, 2, 128, 64)
    host = mod.remap(im)
    t = torch.from_numpy(im.view(np.int16).copy()).to(Context.current().device)
    dev = mod.remap_device(t)
    assert dev.is_cuda and dev.dtype == torch.int16 and tuple(dev.shape) == (64, 128, 3) and dev.is_contiguous()
    assert dev.cpu().numpy().view(np.uint16).tobytes() == host.tobytes()
    # a cropped lens gives the crop of the uncropped result (reference util/image.py croppedImage)
    from auromat_amd.util.image import croppedImage
    full = _modifier('poly5', (132, 68)).remap(im)
    assert croppedImage(full, 16).tobytes() == host.tobytes()
    with pytest.raises(ValueError):
        mod.remap(im[:-1])
    with pytest.raises(TypeError):
        mod.remap(im.astype(np.float64))
