"""
The lens statement itself (tests/_lens_oracle.py), the constructed cases (tests/_lens_cases.py) and the host side of the lens
feature — no GPU.  tests/test_gpu_lens_cells.py holds the kernels to what is checked here.
"""
import json
import os

import numpy as np
import pytest

import _lens_cases as K
import _lens_oracle as O


# ---- the oracle against answers worked out by hand ------------------------------------------------------------------------
def test_poly3_known_answers():
    # 101 x 51: cx = 50, cy = 25, norm = 2 / 50.  Centre: r = 0, g = 1 - k1; the centre maps to itself whatever g is
    xs, ys = O.forward('poly3', [0.1], 101, 51, 50.0, 25.0)
    assert (xs, ys) == (50.0, 25.0)
    assert O.g_of('poly3', [0.1], 0.0) == 0.9
    # r = 1 (25 px from the centre along y): g = 1 - k1 + k1 = 1 -> the pixel itself
    assert O.g_of('poly3', [0.1], 1.0) == 1.0
    assert O.forward('poly3', [0.1], 101, 51, 50.0, 50.0) == (50.0, 50.0)
    # r = 2 along x (x = 100): g = 0.9 + 0.1 * 4 = 1.3 -> 50 + 50 * 1.3 = 115
    xs, ys = O.forward('poly3', [0.1], 101, 51, 100.0, 25.0)
    assert abs(xs - 115.0) < 1e-12 and ys == 25.0
    # r = 0.5: g = 0.9 + 0.025 = 0.925 -> 50 + 12.5 * 0.925
    xs, _ = O.forward('poly3', [0.1], 101, 51, 62.5, 25.0)
    assert abs(xs - (50 + 12.5 * 0.925)) < 1e-12


def test_ptlens_and_poly5_known_answers():
    # ptlens at r = 1: a + b + c + 1 - a - b - c = 1
    assert abs(O.g_of('ptlens', [0.03, -0.07, 0.02], 1.0) - 1.0) < 1e-16
    # ptlens at r = 2: 8 a + 4 b + 2 c + 1 - a - b - c = 1 + 7 a + 3 b + c
    assert abs(O.g_of('ptlens', [0.03, -0.07, 0.02], 4.0) - (1 + 0.21 - 0.21 + 0.02)) < 1e-15
    # poly5 at r = 2: 1 + 4 k1 + 16 k2
    assert abs(O.g_of('poly5', [0.01, 0.002], 4.0) - 1.072) < 1e-15
    # a frame one pixel wide: the radius is counted in pixels, nothing divides by zero
    assert O.forward('poly5', [0.01, 0.002], 1, 1, 0.0, 0.0) == (0.0, 0.0)
    assert O.constants(1, 9) == (0.0, 4.0, 2.0)


def test_lanczos_kernel_is_exact_at_integers():
    t = np.arange(-5, 6, dtype=np.float64)
    assert np.array_equal(O.lanczos(t), (t == 0).astype(np.float64))
    assert abs(O.lanczos(0.5) - (2 / np.pi) * (np.sin(np.pi / 8) / (np.pi / 8))) < 1e-15
    lo, w = O.tap_weights(np.array([0.0, 0.25]), 'lanczos4')
    assert lo == -3 and np.array_equal(w[0], [0, 0, 0, 1, 0, 0, 0, 0])
    assert abs(w[1].sum() - 1.0) < 1e-15 and w[1][3] == w[1].max()
    lo, w = O.tap_weights(np.array([0.25]), 'linear')
    assert lo == 0 and np.array_equal(w[0], [0.75, 0.25])


# ---- the inverse ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', K.WELL_CONDITIONED)
def test_inverse_of_forward_is_identity(name):
    """forward() of a corrected point, undone at 30 digits, is the point: to a few ulps of the coordinate times the conditioning"""
    model, params = K.MODELS[name]
    w, h = 33, 33
    out, slope, _ = O.inverse_grid(model, list(params), w, h, None, corner=True)
    assert np.isfinite(out).all() and np.nanmin(slope) >= 0.1
    # the raw lattice point IS forward(out): push the inverse through the forward statement
    xs, ys = O.forward(model, list(params), w, h, out[..., 0], out[..., 1])
    x, y = O.lattice(w, h, True)
    assert max(np.abs(xs - x).max(), np.abs(ys - y).max()) < 1e-11 * max(1.0, 1.0 / np.nanmin(slope)) * 10


@pytest.mark.parametrize('case', [c for c in K.undistort_cases() if c[2] != (131, 67)], ids=lambda c: c[0])
def test_newton_restatement_against_mpmath(case):
    """The kernel's algorithm (Newton from ru = rd, capped, NaN on a non-positive slope) restated in NumPy gives NaN exactly where
    the model has no inverse, and the root elsewhere — so that the GPU test can demand both of the kernel"""
    cid, name, (w, h), crop, corner = case
    model, params = K.MODELS[name]
    want, slope, nearest = K.undistort_reference(cid)
    # no lattice point of a case sits on the fold itself, where the two rules could disagree through rounding
    assert nearest > 1e-5, nearest
    x, y = O.lattice(w, h, corner)
    left, top = (crop[0], crop[1]) if crop else (0, 0)
    got = np.stack(O.inverse_newton(model, list(params), w, h, x, y), axis=-1) - (left, top)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    good = slope >= 0.1
    if good.any():
        assert np.nanmax(np.abs(got - want)[good]) < 1e-9


def test_fold_and_nan_models_have_holes():
    out, _, nearest = K.undistort_reference('fold-131x67-centre')
    nan = np.isnan(out[..., 0])
    assert nan.any() and not nan.all() and not nan[33, 65] and nan[33, 0] and nan[33, 130]
    out, _, _ = K.undistort_reference('nan-7x5-corner')
    assert np.isnan(out).all()
    assert O.fold_radius('poly5', [0.00613, 0.00059]) is None
    assert abs(float(O.fold_radius('poly3', [-0.4519])) - np.sqrt(1.4519 / (3 * 0.4519))) < 1e-15


# ---- sampling -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', K.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize('interp', ('linear', 'lanczos4'))
def test_identity_remap_returns_the_image(dtype, interp):
    im = K.image(33, 33, 3, dtype, 'random')
    xy = O.forward_grid('poly3', [0.0], 33, 33)
    out, support = O.remap(im, xy[..., 0], xy[..., 1], interp)
    assert out.dtype == im.dtype and out.tobytes() == im.tobytes() and support.all()


def test_border_and_non_finite_coordinates():
    im = np.full((5, 7, 1), 100, dtype=np.uint8)
    # half a pixel outside along x with linear taps: half the weight falls on the constant border (0), nothing is renormalised
    v, s = O.sample(im, np.array([[-0.5, 6.5, 3.0, np.nan, 1e300]]), np.array([[2.0, 2.0, -1.0, 2.0, 2.0]]), 'linear')
    assert np.array_equal(v[0, :, 0], [50.0, 50.0, 0.0, 0.0, 0.0]) and np.array_equal(s[0], [0, 0, 0, 0, 0])
    v, s = O.sample(im, np.array([[0.0, 6.0]]), np.array([[0.0, 4.0]]), 'lanczos4')
    assert np.array_equal(s[0], [1, 1]) and np.array_equal(v[0, :, 0], [100.0, 100.0])
    # rounding: half to even, clipped
    assert np.array_equal(O.convert(np.array([0.5, 1.5, 2.5, -3.0, 300.0]), np.uint8), [0, 2, 2, 0, 255])
    assert O.convert(np.array([70000.0]), np.uint16)[0] == 65535


@pytest.mark.parametrize('case', K.remap_cases(), ids=lambda c: c[0])
def test_few_outputs_sit_on_a_rounding_boundary(case):
    """A condition on the inputs, not a tolerance: at most 0.1 % of a case's outputs lie within 1e-6 of a rounding boundary, where
    the device may round the other way."""
    im, values, support, mag = K.remap_reference(case[0])
    share = O.near_boundary(values, im.dtype, mag).mean()
    assert share <= 1e-3, share
    name = case[1]
    if name == 'identity':
        assert O.convert(values, im.dtype).tobytes() == im.tobytes()
    if name == 'nan':
        assert not values.any() and not support.any()
    if name == 'outside' and case[2] == (131, 67):
        assert not support[:, 0].any() and support[33, 65]
    if case[5] == 'step' and name != 'identity' and case[6] == 'lanczos4' and im.dtype != np.float32:
        top = O.SAMPLE_MAX[im.dtype]
        assert values.min() < -0.5 and values.max() > top + 0.5, 'the overshoot must clip at both ends'


def test_star_centroids_survive_the_remap():
    """Gaussian stars rendered at forward(p) in a raw frame have their centroids at p after the Lanczos remap.  The oracle's largest
    centroid error is measured here and is the bar; the GPU inherits it, because it agrees with the oracle to the count."""
    w, h = 131, 67
    model, params = K.MODELS['poly5']
    stars = [(20.3, 12.6), (65.0, 33.0), (101.7, 50.2), (118.4, 9.9), (40.5, 47.5)]
    sigma = 1.6
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    raw = np.zeros((h, w))
    for px, py in stars:
        sx, sy = O.forward(model, list(params), w, h, px, py)
        raw += 1000.0 * np.exp(-((xx - sx) ** 2 + (yy - sy) ** 2) / (2 * sigma ** 2))
    xy = O.forward_grid(model, list(params), w, h)
    values, _ = O.sample(raw.astype(np.float32), xy[..., 0], xy[..., 1], 'lanczos4')
    img = values[..., 0]
    worst = 0.0
    for px, py in stars:
        x0, y0 = int(round(px)), int(round(py))
        win = (slice(max(y0 - 8, 0), y0 + 9), slice(max(x0 - 8, 0), x0 + 9))
        m = img[win]
        worst = max(worst, abs((m * xx[win]).sum() / m.sum() - px), abs((m * yy[win]).sum() / m.sum() - py))
    print('largest centroid error: %.3e px' % worst)
    # measured 1.61e-2 px, at the star nearest a corner: the displacement is curved across a star (its second derivative there
    # is 5e-3 per px), which moves a centroid by about sigma^2 times that — a property of remapping, not of the sampling.  Bar 2e-2
    assert worst < 2e-2, worst


# ---- the host side of the feature -------------------------------------------------------------------------------------
def test_cropped_image_rule():
    from auromat_amd.util.image import croppedImage, cropWindow
    assert cropWindow(2832, 4256) == (0, 0, 2832, 4256)             # the D3S frame is a multiple of 16 already
    im = np.arange(38 * 50).reshape(38, 50)
    out = croppedImage(im)                                          # 38 -> 32 (3 each side), 50 -> 48 (1 each side)
    assert out.shape == (32, 48) and out[0, 0] == im[3, 1] and out[-1, -1] == im[34, 48]
    assert croppedImage(im, divisible_by=6).shape == (36, 48)
    with pytest.raises(AssertionError):
        croppedImage(im, divisible_by=5)                            # 38 -> 35 needs 3 rows: odd
    with pytest.raises(AssertionError):
        croppedImage(np.zeros((2832, 4241)))                        # one column to crop cannot be shared
    with pytest.raises(AssertionError):
        croppedImage(np.zeros((33, 32)))


def test_modifier_arguments():
    from auromat_amd.util import lensdistortion as L
    with pytest.raises(ValueError):
        L.getLensfunModifierFromParams('poly7', [0.1], 100, 50)
    with pytest.raises(ValueError):
        L.getLensfunModifierFromParams('none', [], 100, 50)
    for model, params in (('poly3', [0.1, 0.2]), ('poly5', [0.1]), ('ptlens', [0.1, 0.2])):
        with pytest.raises(ValueError):
            L.getLensfunModifierFromParams(model, params, 100, 50)
    mod = L.getLensfunModifierFromParams('ptlens', [0.01, -0.02, 0.003], 4256, 2838)
    assert mod.corrected_size == (4256, 2838) and mod.crop is None
    c = mod.cropped(16)
    assert c.crop == (0, 3, 4256, 2832) and c.corrected_size == (4256, 2832) and c.params == mod.params
    with pytest.raises(AssertionError):
        L.getLensfunModifierFromParams('poly3', [0.1], 4241, 2832).cropped()
    with pytest.raises(ValueError):
        L.LensModifier('poly3', [0.1], 100, 50, crop=(90, 0, 20, 50))
    with pytest.raises(NotImplementedError):
        L.correctLensDistortion(np.zeros((5, 7, 3), np.uint8))
    with pytest.raises(ValueError):
        L._interpolation('cubic')
    m = mod._native()
    assert (m.kind, m.width, m.height, m.crop_width, list(m.k)) == (3, 4256, 2838, 0, [0.01, -0.02, 0.003])


def test_get_mapping_rejects_a_lens_on_other_headers():
    from auromat_amd.mapping.spacecraft import getMapping
    from auromat_amd.util.lensdistortion import LensModifier
    hdr = {'CTYPE1': 'RA---STG', 'CTYPE2': 'DEC--STG', 'DATE-OBS': '2012-01-25T09:26:57', 'IMAGEW': 7, 'IMAGEH': 5,
           'POSX': 1.0, 'POSY': 2.0, 'POSZ': 7000.0}
    with pytest.raises(NotImplementedError):
        getMapping(np.zeros((5, 7, 3), np.uint8), hdr, lens=LensModifier('poly3', [0.01], 7, 5))
    tan = dict(hdr, CTYPE1='RA---TAN', CTYPE2='DEC--TAN', LATPOLE=0.0)
    with pytest.raises(ValueError):
        getMapping(np.zeros((5, 7, 3), np.uint8), tan, lens=LensModifier('poly3', [0.01], 7, 5), lensRoute='fast')
    with pytest.raises(ValueError):          # the header must be that of the corrected, cropped image
        getMapping(np.zeros((6, 8, 3), np.uint8), tan, lens=LensModifier('poly3', [0.01], 8, 6))


def test_convert_flags_and_metadata_key(tmp_path):
    from auromat_amd.cli import convert as CV
    base = ['--data', str(tmp_path), '--format', 'netcdf']
    a = CV.parseargs(base)
    assert a.lensModel is None and a.lensParams is None and a.lensRoute == 'resample' and a.cropDivisibleBy is None
    a = CV.parseargs(base + ['--lens-model', 'ptlens', '--lens-params', '0.01', '-0.02', '0.003', '--lens-route', 'raw',
                             '--crop-divisible-by', '16'])
    assert (a.lensModel, a.lensParams, a.lensRoute, a.cropDivisibleBy) == ('ptlens', [0.01, -0.02, 0.003], 'raw', 16)
    for bad in (['--lens-model', 'poly3'], ['--lens-params', '0.1'], ['--lens-model', 'poly3', '--lens-params', '0.1', '0.2'],
                ['--lens-model', 'poly9', '--lens-params', '0.1'], ['--lens-route', 'both'], ['--crop-divisible-by', '0']):
        with pytest.raises(SystemExit):
            CV.parseargs(base + bad)
    # flags win; else the frame's own <id>.json; else metadata.json (top level, as in the archive's API data, or per sequence)
    assert CV.lens_spec(a, {'distortion_correction': {'model': 'poly3', 'params': [0.5]}}) == ('ptlens', [0.01, -0.02, 0.003])
    plain = CV.parseargs(base)
    assert CV.lens_spec(plain, {}) is None and CV.lens_spec(plain, {}, {'sequence_metadata': {}}) is None
    assert CV.lens_spec(plain, {'distortion_correction': {'model': 'poly3', 'params': [0.5]}}) == ('poly3', [0.5])
    assert CV.lens_spec(plain, {'distortion_correction': None}, {'distortion_correction': {'model': 'poly5', 'params': [1, 2]}}) == \
        ('poly5', [1.0, 2.0])
    with open(os.path.join(str(tmp_path), 'metadata.json'), 'w') as fp:
        json.dump({'sequence_metadata': {'distortion_correction': {'model': 'ptlens', 'params': [0.1, 0.2, 0.3]}},
                   'image_metadata': {}}, fp)
    meta = CV.read_metadata(str(tmp_path))
    assert CV.lens_spec(plain, {}, meta) == ('ptlens', [0.1, 0.2, 0.3])
    crop = CV.parseargs(base + ['--crop-divisible-by', '16'])
    mod = CV.lens_of(crop, {}, meta, 4256, 2838)
    assert mod.model == 'ptlens' and mod.crop == (0, 3, 4256, 2832)
    assert CV.lens_of(plain, {}, None, 4256, 2838) is None


def test_pixel_distances_shape_rule():
    """lensDistortionPixelDistances keeps the reference's centre (width / 2, height / 2); checked on the identity without a GPU"""
    from auromat_amd.util import lensdistortion as L

    class Identity(object):
        def apply_geometry_distortion(self):
            y, x = np.mgrid[0:5, 0:7]
            return np.dstack((x, y)).astype(np.float32)

    d, own, sampled = L.lensDistortionPixelDistances(Identity(), retH=True)
    assert d.shape == (5, 7) and not d.any() and own[0, 0] == np.hypot(3.5, 2.5) and np.array_equal(own, sampled)
