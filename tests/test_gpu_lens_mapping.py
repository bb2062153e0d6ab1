"""
Lens distortion in the mapping layer on the MI355X: ``getMapping(..., lens=, lensRoute=, cropDivisibleBy=)``, device-resident
corrected images in ``SequencePipeline`` and the ``auromat-convert`` flags, on a 424 x 284 synthetic frame that shows the sky of
the reference's ISS030 header (auromat_amd.synthetic.frame_header: its CRVAL / CD / rotation cards, CRPIX at the centre).
"""
import json
import os

import numpy as np
import numpy.ma as ma
import pytest

import _lens_cases as K
import _lens_oracle as O

pytestmark = pytest.mark.gpu

W, H = 424, 284
COORD_BAR = 2e-11          # degrees: the project's coordinate bar


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


def _same_coordinates(a, b, bar=COORD_BAR):
    for key in ('lats', 'lons', 'latsCenter', 'lonsCenter'):
        x, y = getattr(a, key), getattr(b, key)
        assert np.array_equal(ma.getmaskarray(x), ma.getmaskarray(y)), key
        d = np.abs(ma.filled(x, 0.0) - ma.filled(y, 0.0))
        d = np.minimum(d, 360.0 - d) if key.startswith('lons') else d
        assert d.max() <= bar, (key, d.max())


@pytest.mark.parametrize('name,crop', [('poly5', None), ('ptlens', 16), ('fold', None)])
def test_raw_route(name, crop):
    """Corner coordinates of the raw route against a DirectionArrayMapping built from tan_pix2world at the oracle's undistorted
    coordinates; where the model has no inverse the corners are NaN and the pixels masked."""
    from auromat_amd.coordinates.wcs import tan_pix2world
    from auromat_amd.mapping.astrometry import DirectionArrayMapping
    from auromat_amd.mapping.spacecraft import frame_inputs, getMapping
    mod = _lens(name)
    cw, ch = mod.cropped(crop).corrected_size if crop else (W, H)
    hdr = _header(cw, ch)
    img = _raw_image()
    m = getMapping(img, hdr, lens=mod, lensRoute='raw', cropDivisibleBy=crop, identifier='raw')
    assert isinstance(m, DirectionArrayMapping) and m.img.shape == (H, W, 3)

    model, params = K.MODELS[name]
    x, y = O.lattice(W, H, True)
    X, Y = O.inverse_newton(model, list(params), W, H, x, y)
    if crop:
        left, top = mod.cropped(crop).crop[:2]
        X, Y = X - left, Y - top
    dirs = tan_pix2world(hdr, X, Y, 0, ascartesian=True)
    cam, t = frame_inputs(hdr)
    want = DirectionArrayMapping(dirs, 110, img, cam, t, 'want')
    _same_coordinates(m, want)
    assert np.array_equal(ma.getmaskarray(m.img), ma.getmaskarray(want.img))
    assert np.array_equal(ma.getdata(m.img), ma.getdata(want.img))
    if name == 'fold':
        hole = np.isnan(X)
        assert hole.any() and np.isnan(ma.filled(m.lats, np.nan))[hole].all()
        assert ma.getmaskarray(m.img)[:, 0].all(), 'pixels beyond the fold are masked'
    assert not ma.getmaskarray(m.img).all()


@pytest.mark.parametrize('name,crop', [('poly5', None), ('ptlens', 16)])
def test_resample_route(name, crop):
    from auromat_amd.mapping.spacecraft import getMapping
    from auromat_amd.util.image import croppedImage
    mod = _lens(name)
    cw, ch = mod.cropped(crop).corrected_size if crop else (W, H)
    assert (cw, ch) == ((416, 272) if crop else (W, H))
    hdr = _header(cw, ch)
    raw = _raw_image()
    m = getMapping(raw, hdr, lens=mod, lensRoute='resample', cropDivisibleBy=crop, fastCenterCalculation=True)
    corrected = mod.remap(raw, 'lanczos4')
    corrected = croppedImage(corrected, crop) if crop else corrected
    assert not np.array_equal(corrected, croppedImage(raw, crop) if crop else raw)
    assert np.array_equal(ma.getdata(m.img), corrected)
    want = getMapping(np.ascontiguousarray(corrected), hdr, fastCenterCalculation=True)
    _same_coordinates(m, want, bar=0.0)
    assert np.array_equal(ma.getmaskarray(m.img), ma.getmaskarray(want.img))


def test_identity_lens_changes_nothing():
    from auromat_amd.mapping.spacecraft import getMapping
    hdr, raw, mod = _header(W, H), _raw_image(), _lens('identity')
    plain = getMapping(raw, hdr, fastCenterCalculation=True)
    for route in ('resample', 'raw'):
        m = getMapping(raw, hdr, lens=mod, lensRoute=route, fastCenterCalculation=True)
        _same_coordinates(m, plain)
        assert np.array_equal(ma.getdata(m.img), raw)
        assert np.array_equal(ma.getmaskarray(m.img), ma.getmaskarray(plain.img))


def test_sequence_pipeline_takes_corrected_device_images():
    """remap_device tensors fed to SequencePipeline give the bits of the host-corrected arrays"""
    import torch
    from auromat_amd.mapping.spacecraft import frame_inputs
    from auromat_amd.pipeline import SequencePipeline
    mod = _lens('poly5').cropped(16)
    cw, ch = mod.corrected_size
    raws = [_raw_image(seed=20 + k) for k in range(3)]
    heads = [_header(cw, ch, k) for k in range(3)]
    host_frames = [(hd,) + tuple(frame_inputs(hd)) + (mod.remap(raw),) for hd, raw in zip(heads, raws)]
    dev_frames = []
    for hd, raw in zip(heads, raws):
        t = mod.remap_device(raw)
        assert t.is_cuda and t.dtype == torch.int16 and tuple(t.shape) == (ch, cw, 3)
        dev_frames.append((hd,) + tuple(frame_inputs(hd)) + (t,))
    torch.cuda.synchronize()
    want = SequencePipeline(cw, ch, pxPerDeg=6).process(host_frames, keep_on_device=True)
    got = SequencePipeline(cw, ch, pxPerDeg=6).process(dev_frames, keep_on_device=True)
    assert len(got) == len(want) == 3 and all(r is not None for r in want)
    for a, b in zip(got, want):
        for key in ('mean', 'count', 'img', 'mask'):
            assert np.array_equal(a[key].cpu().numpy(), b[key].cpu().numpy(), equal_nan=True), key


def test_convert_with_a_lens(tmp_path):
    """auromat-convert over two raw .npy frames, once per route: the files hold the arrays of the class API"""
    from auromat_amd.cli.convert import main
    from auromat_amd.mapping.netcdf import read_arrays
    from auromat_amd.mapping.spacecraft import getMapping
    w, h = 264, 170                      # corrected and cropped to a multiple of 16: 256 x 160
    model, params = K.MODELS['ptlens']
    mod = _lens('ptlens', w, h)
    d = tmp_path / 'frames'
    d.mkdir()
    for k in range(2):
        (d / ('raw%02d.json' % k)).write_text(json.dumps(_header(256, 160, k)))
        np.save(str(d / ('raw%02d.npy' % k)), _raw_image(seed=40 + k, w=w, h=h))
    flags = ['--data', str(d), '--format', 'netcdf', '--lens-model', model, '--lens-params'] + [repr(p) for p in params] + \
        ['--crop-divisible-by', '16']
    for route in ('raw', 'resample'):
        out = str(tmp_path / route)
        main(flags + ['--lens-route', route, '--out', out])
        assert sorted(os.listdir(out)) == ['raw00.nc', 'raw01.nc']
        for k in range(2):
            hdr = json.loads((d / ('raw%02d.json' % k)).read_text())
            want = getMapping(np.load(str(d / ('raw%02d.npy' % k))), hdr, fastCenterCalculation=True, lens=mod, lensRoute=route,
                              cropDivisibleBy=16, identifier='raw%02d' % k)
            got = read_arrays(os.path.join(out, 'raw%02d.nc' % k))
            assert got['img'].shape[:2] == ((h, w) if route == 'raw' else (160, 256))
            assert np.array_equal(got['lats'].filled(np.nan), want.lats.filled(np.nan), equal_nan=True)
            assert np.array_equal(got['lons'].filled(np.nan), want.lons.filled(np.nan), equal_nan=True)
            assert np.array_equal(got['img'].filled(0), want.img.filled(0))
            assert np.array_equal(ma.getmaskarray(got['img']), ma.getmaskarray(want.img))
    # the archive's key in metadata.json stands in for the flags
    (d / 'metadata.json').write_text(json.dumps({'distortion_correction': {'model': model, 'params': list(params)}}))
    out = str(tmp_path / 'meta')
    main(['--data', str(d), '--format', 'netcdf', '--crop-divisible-by', '16', '--out', out])
    a, b = read_arrays(os.path.join(out, 'raw01.nc')), read_arrays(os.path.join(str(tmp_path / 'resample'), 'raw01.nc'))
    assert np.array_equal(a['img'].filled(0), b['img'].filled(0))


def test_providers_and_sequences_pass_the_lens_on(tmp_path):
    from auromat_amd.mapping.spacecraft import (SpacecraftMappingPathProvider, SpacecraftMappingProvider, getLensMappingSequence,
                                                getMapping)
    w, h = 264, 170
    mod = _lens('poly5', w, h)
    images, solutions = [], []
    for k in range(2):
        solutions.append(str(tmp_path / ('raw%02d.json' % k)))
        images.append(str(tmp_path / ('raw%02d.npy' % k)))
        with open(solutions[-1], 'w') as fp:
            json.dump(_header(256, 160, k), fp)
        np.save(images[-1], _raw_image(seed=60 + k, w=w, h=h))
    kw = dict(lens=mod, lensRoute='raw', cropDivisibleBy=16, fastCenterCalculation=True)
    want = [getMapping(i, s, **kw) for i, s in zip(images, solutions)]
    assert want[0].img.shape == (h, w, 3)
    sequences = (SpacecraftMappingPathProvider(images, solutions, **kw).getSequence(),
                 SpacecraftMappingProvider(images, solutions, **kw).getSequence(),
                 getLensMappingSequence(images, solutions, mod, 'raw', 16, fastCenterCalculation=True))
    for seq in sequences:
        got = list(seq)
        assert len(got) == 2
        for a, b in zip(got, want):
            _same_coordinates(a, b, bar=0.0)
            assert np.array_equal(ma.getdata(a.img), ma.getdata(b.img))
    by_id = SpacecraftMappingProvider(images, solutions, **dict(kw, lensRoute='resample')).getById('raw01')
    assert by_id.img.shape == (160, 256, 3)
