"""
Gathering through the lens, the parts that need no GPU: the host-only fold radius (amt_lens_fold_radius) against mpmath, the
statement of step 9 of world -> pixel (tests/_lens_gather_cases.py) on hand-computed points, the point cases' own properties, the
declared surface, the converter's flags and the mapping constructor's rules.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import _inverse_cases as IC
import _inverse_oracle as O
import _lens_cases as LC
import _lens_gather_cases as G
import _lens_oracle as LO

NEW_SYMBOLS = ('amt_world_to_pixel_lens', 'amt_grid_to_pixel_lens', 'amt_gather_mosaic_lens', 'amt_gather_mosaic_supersampled_lens',
               'amt_gather_frames_lens', 'amt_lens_fold_radius')


def native_fold(model, params):
    from auromat_amd import _native
    m = _native.LensModel()
    m.kind = G.KINDS[model]
    m.k[:] = (list(params) + [0.0, 0.0, 0.0])[:3]
    r = C.c_double(-1.0)
    assert _native.lib().amt_lens_fold_radius(C.byref(m), C.byref(r)) == 0
    return r.value


# ---- the fold radius ----------------------------------------------------------------------------------------------------------------
FOLD_MODELS = dict(LC.MODELS)
FOLD_MODELS.update({'ptlens-' + k: ('ptlens', v) for k, v in G.PTLENS_FOLDS.items()})
FOLD_MODELS.update({'poly5-two-roots': ('poly5', (-0.2, 0.01)), 'poly5-linear': ('poly5', (-0.3, 0.0)), 'poly3-centre': ('poly3', (1.5,)),
                    'poly5-nan': ('poly5', (0.1, float('nan'))), 'ptlens-nan': ('ptlens', (0.1, float('nan'), 0.0))})


@pytest.mark.parametrize('name', sorted(FOLD_MODELS))
def test_fold_radius_against_mpmath(name):
    """at most 4 ulp from the smallest positive root that mpmath finds for the slope polynomial; +inf where it finds none, 0 where
    the slope is not positive at r = 0, NaN with a NaN coefficient"""
    import mpmath as mp
    model, params = FOLD_MODELS[name]
    got = native_fold(model, params)
    want = G.fold_radius(model, tuple(params))
    if isinstance(want, float) and math.isnan(want):
        assert math.isnan(got)
    elif want == 0.0 or want == math.inf:
        assert got == want, (got, want)
    else:
        with mp.workdps(40):
            ulps = abs(mp.mpf(got) - want) / mp.mpf(float(np.spacing(float(want))))
        print('%s: r_fold = %.17g, %.2f ulp from mpmath' % (name, got, float(ulps)))
        assert ulps <= 4, (got, float(want), float(ulps))


def test_fold_radius_cases_cover_every_branch():
    kinds = {name: G.fold_radius(*[FOLD_MODELS[name][0], tuple(FOLD_MODELS[name][1])]) for name in FOLD_MODELS}
    assert kinds['identity'] == math.inf and kinds['magnify'] == math.inf and kinds['ptlens-no-root'] == math.inf
    assert kinds['ptlens-centre'] == 0.0 and kinds['ptlens-centre-zero'] == 0.0 and kinds['poly3-centre'] == 0.0
    assert math.isnan(kinds['nan']) and math.isnan(kinds['poly5-nan']) and math.isnan(kinds['ptlens-nan'])
    assert abs(float(kinds['fold']) - 1.035) < 1e-3                         # what tests/_lens_cases.py says of it
    # two positive roots of the slope: the smaller one
    import mpmath as mp
    a, b, c = G.PTLENS_FOLDS['two-roots']
    roots = sorted(float(mp.re(r)) for r in mp.polyroots([4 * a, 3 * b, 2 * c, 1 - a - b - c]) if abs(mp.im(r)) < 1e-20 and mp.re(r) > 0)
    assert len(roots) == 2 and abs(float(kinds['ptlens-two-roots']) - roots[0]) < 1e-12
    for name in ('ptlens-cubic-down', 'ptlens-quadratic', 'ptlens-linear', 'poly5-two-roots', 'poly5-linear'):
        assert 0.0 < float(kinds[name]) < math.inf, name
    assert native_fold('none', ()) == math.inf
    from auromat_amd import _native
    m = _native.LensModel()
    m.kind = 7
    r = C.c_double()
    assert _native.lib().amt_lens_fold_radius(C.byref(m), C.byref(r)) == -1
    assert _native.lib().amt_lens_fold_radius(None, C.byref(r)) == -1 and _native.lib().amt_lens_fold_radius(C.byref(m), None) == -1


# ---- the statement on hand-computed points --------------------------------------------------------------------------------------
@pytest.mark.parametrize('xp', [O.F64, None], ids=['float64', 'mpmath'])
def test_statement_on_hand_computed_points(xp):
    xp = xp or O.MP()
    cam = IC.by_name('cd-rotation-37')                                      # 40 x 30
    for crop in (False, True):
        for model in ('poly3', 'poly5', 'ptlens', 'magnify', 'fold'):
            lens = G.lens_of(cam, model, crop)
            cx, cy, _ = LO.constants(lens['width'], lens['height'])
            left, top = lens['crop'][:2] if crop else (0, 0)
            # the centre of the raw frame maps to itself: u = v = 0 whatever g is
            xs, ys, fl, _ = G.step9(xp, lens, xp.num(cx - left), xp.num(cy - top))
            assert (float(xs), float(ys), fl) == (cx, cy, 0), (model, crop)
        # the identity: the coordinate of the full corrected frame itself
        lens = G.lens_of(cam, 'identity', crop)
        left, top = lens['crop'][:2] if crop else (0, 0)
        for X, Y in ((0.0, 0.0), (12.25, 3.5), (39.0, 29.0), (-0.5, 29.5)):
            xs, ys, fl, _ = G.step9(xp, lens, xp.num(X), xp.num(Y))
            assert (float(xs), float(ys), fl) == (X + left, Y + top, 0), (X, Y, crop)
        xs, ys, fl, _ = G.step9(xp, lens, xp.num(-4.0), xp.num(2.0))
        assert fl == (0 if crop else O.OUTSIDE) and float(xs) == -4.0 + left           # (the crop's margin is part of the raw frame)
    # the fold of model 'fold' on the 40 x 30 frame: norm = 2 / 29, r_fold = 1.035...: a point on the row of the centre at
    # r = 1.03 is kept, one at r = 1.04 is not; by hand g(1.03) = 1.4519 - 0.4519 * 1.0609 = 0.97247929
    lens = G.lens_of(cam, 'fold', False)
    cx, cy, norm = LO.constants(40, 30)
    k = LC.MODELS['fold'][1][0]
    assert (norm, k) == (2.0 / 29.0, -0.4519)
    xs, ys, fl, margin = G.step9(xp, lens, xp.num(cx + 1.03 / norm), xp.num(cy))
    assert fl == 0 and abs(float(xs) - (cx + 1.03 * 0.97247929 / norm)) < 1e-9 and float(ys) == cy and 4e-3 < margin < 6e-3
    xs, ys, fl, margin = G.step9(xp, lens, xp.num(cx + 1.04 / norm), xp.num(cy))
    assert fl == G.LENS_FOLD and math.isnan(float(xs)) and math.isnan(float(ys)) and 4e-3 < margin < 6e-3
    # a NaN coefficient, and a model folded at the centre: nothing is kept, the centre included
    for lens in (G.lens_of(cam, 'nan', False), dict(G.lens_of(cam, 'poly3', False), params=(1.5,))):
        assert G.step9(xp, lens, xp.num(cx), xp.num(cy))[2] == G.LENS_FOLD
    # what has no pixel after steps 1-8 has none after step 9; a hidden point goes through the lens like any other
    lens = G.lens_of(cam, 'poly3', True)
    assert G.inverse_lens(xp, cam, lens, O.GEODETIC, 95.0, 0.0)['flags'] == O.INVALID
    pts = IC.points('cd-rotation-37')['geodetic']
    i = int(np.flatnonzero(pts['expect_hidden'])[0])
    r = G.inverse_lens(xp, cam, lens, O.GEODETIC, pts['c0'][i], pts['c1'][i])
    assert r['flags'] & O.HIDDEN and not r['flags'] & G.NO_PIXEL and math.isfinite(float(r['x']))


def test_point_cases_are_decidable_and_cover_the_flags():
    """at most 1 % of the points of the GPU point test lie within AMBIGUOUS of the fold radius, the raw frame's edge or another
    yes / no decision: only those are left out of its flag comparison; and every flag of step 9 occurs on both sides"""
    total = unsure = 0
    seen = {}
    for camera, model, crop, frame in G.point_cases():
        r = G.points(camera, model, crop, frame)
        total += len(r['sure'])
        unsure += int((~r['sure']).sum())
        key = seen.setdefault(model, dict(fold=0, outside=0, inside=0, n=0))
        key['fold'] += int(((r['flags'] & G.LENS_FOLD) != 0).sum())
        key['outside'] += int(((r['flags'] & O.OUTSIDE) != 0).sum())
        key['inside'] += int((r['flags'] == 0).sum())
        key['n'] += len(r['flags'])
        no_pixel = (r['flags'] & G.NO_PIXEL) != 0
        assert np.array_equal(np.isnan(r['x']), no_pixel) and np.array_equal(np.isnan(r['y']), no_pixel)
    print('%d points, %d ambiguous; per model: %r' % (total, unsure, seen))
    assert total >= 4800 and unsure <= 0.01 * total
    assert seen['fold']['fold'] > 0 and seen['fold']['inside'] > 0
    assert seen['nan']['inside'] == 0 and seen['nan']['fold'] > 0
    for model in ('identity', 'poly3', 'poly5', 'ptlens', 'outside', 'magnify'):
        assert seen[model]['fold'] == 0 and seen[model]['inside'] > 0 and seen[model]['outside'] > 0, model
    # the identity without a crop is the statement without a lens
    for camera in G.CAMERAS:
        for frame, _ in IC.FRAMES:
            r, ref = G.points(camera, 'identity', False, frame), IC.points(camera)[frame]['ref']
            assert np.array_equal(r['flags'], ref['flags']) and np.array_equal(r['x'], ref['x'], equal_nan=True)


# ---- surface --------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared():
    from auromat_amd import _native
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'auromat_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert name in _native._SIGNATURES and ('int %s(' % name) in header, name
        assert getattr(_native.lib(), name) is not None
    assert '#define AMT_W2P_LENS_FOLD 32' in header
    assert '#define AMT_ABI_VERSION 10' in header and _native.ABI_VERSION == 10 and _native.lib().amt_abi_version() == 10
    from auromat_amd.coordinates import inverse
    assert inverse.LENS_FOLD == 32 and inverse.NOT_SEEN & inverse.LENS_FOLD and inverse.NO_PIXEL & inverse.LENS_FOLD
    assert not inverse.NOT_SEEN & inverse.OUTSIDE


def test_convert_parser_knows_the_fused_route(capsys):
    from auromat_amd.cli.convert import getParser, parseargs
    base = ['--data', '/nonexistent', '--format', 'netcdf', '--lens-model', 'poly3', '--lens-params', '0.01']
    a = parseargs(base + ['--resample', '--gather', 'linear', '--lens-route', 'fused'])
    assert (a.gather, a.lensRoute, a.supersample) == ('linear', 'fused', 1)
    a = parseargs(base + ['--resample', '--gather', 'lanczos4', '--supersample', '3', '--lens-route', 'fused', '--grid', 'geo'])
    assert (a.lensRoute, a.supersample) == ('fused', 3)
    for bad, message in ((['--lens-route', 'fused'], '--lens-route fused needs --gather'),
                         (['--resample', '--lens-route', 'fused'], '--lens-route fused needs --gather'),
                         (['--resample', '--gather', 'linear', '--lens-route', 'raw'], '--lens-route fused'),
                         (['--resample', '--gather', 'linear', '--lens-route', 'lens'], 'invalid choice')):
        with pytest.raises(SystemExit) as e:
            parseargs(base + bad)
        assert e.value.code != 0
        assert message in capsys.readouterr().err, bad
    text = ' '.join(getParser().format_help().split())
    assert 'fused' in text and 'only with --gather' in text


def test_mapping_constructor_rules():
    from auromat_amd.mapping.astrometry import DirectionArrayMapping
    from auromat_amd.mapping.mapping import BaseMapping
    from auromat_amd.util.lensdistortion import LensModifier
    cam = IC.by_name('cd-rotation-37')
    w, h = cam['width'], cam['height']
    dirs = np.zeros((h + 1, w + 1, 3))
    dirs[..., 2] = 1.0
    img = np.zeros((h, w, 3), dtype=np.uint8)
    hdr = IC.header_of(cam)
    # noInverse= keeps working exactly as before
    m = DirectionArrayMapping(dirs, 110.0, img, cam['cam'], IC.K.T0, 'raw', noInverse='a raw frame with its lens distortion')
    assert m._inverse_lens() is None
    with pytest.raises(NotImplementedError, match='lens'):
        m.latLonToPixel([0.0], [0.0])
    assert BaseMapping._inverse_lens(m) is None
    # a lens goes with a header only, and with the sizes that belong together
    mod = LensModifier('poly3', [-0.01237], w, h)
    with pytest.raises(ValueError, match='cameraHeader'):
        DirectionArrayMapping(dirs, 110.0, img, cam['cam'], IC.K.T0, 'raw', cameraLens=mod)
    with pytest.raises(ValueError, match='corrects to'):
        DirectionArrayMapping(dirs, 110.0, img, cam['cam'], IC.K.T0, 'raw', cameraHeader=hdr, cameraLens=mod.cropped(16))
    with pytest.raises(ValueError, match='raw frame'):
        DirectionArrayMapping(dirs, 110.0, img, cam['cam'], IC.K.T0, 'raw', cameraHeader=hdr,
                              cameraLens=LensModifier('poly3', [-0.01237], w + 11, h + 7, crop=(5, 3, w, h)))
    m = DirectionArrayMapping(dirs, 110.0, img, cam['cam'], IC.K.T0, 'raw', cameraHeader=hdr, cameraLens=mod)
    lens = m._inverse_lens()
    assert (lens.kind, lens.width, lens.height, lens.k[0]) == (1, w, h, -0.01237)
    p, z = m._inverse_model()
    assert (p.width, p.height, z.width, z.height) == (w, h, w, h)
    # a cropped lens: the params hold the raw size, the zenithal block the header's
    big = np.zeros((h + 7, w + 11, 3), dtype=np.uint8)
    bdirs = np.zeros((h + 8, w + 12, 3))
    bdirs[..., 2] = 1.0
    m = DirectionArrayMapping(bdirs, 110.0, big, cam['cam'], IC.K.T0, 'raw', cameraHeader=hdr,
                              cameraLens=LensModifier('poly3', [-0.01237], w + 11, h + 7, crop=(5, 3, w, h)))
    p, z = m._inverse_model()
    assert (p.width, p.height, z.width, z.height) == (w + 11, h + 7, w, h)
    import copy
    assert copy.copy(m)._inverse_lens().crop_x == 5                         # what the masked copies of a mapping keep
