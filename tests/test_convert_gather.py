"""
``auromat-convert --gather {nearest,linear,lanczos4} [--supersample N [--min-coverage F]]`` on the MI355X: both routes — the
sequence pipeline (GatherSequence) and the mapping classes (AMT_CONVERT_CLASSES=1) — against resampleGather /
resampleGatherMLatMLT of the class API, in tests/test_convert_area.py's way, and grid_mapping on a plain elevation.  (The parser's
errors: tests/test_gather_frames_cpu.py.)
"""
import json
import os

import numpy as np
import numpy.ma as ma
import pytest

from test_convert_area import same_files
from test_convert_cli import write_frames

pytestmark = pytest.mark.gpu


def test_convert_gather_both_routes(tmp_path, monkeypatch):
    from auromat_amd.cli.convert import main
    from auromat_amd.mapping.netcdf import read_arrays
    from auromat_amd.mapping.spacecraft import getMapping
    from auromat_amd.resample import resampleGather, resampleGatherMLatMLT
    d = write_frames(tmp_path)
    names = ['frame00.nc', 'frame01.nc', 'frame02.nc']

    def both(args, tag):
        out1, out2 = str(tmp_path / ('pipe_' + tag)), str(tmp_path / ('classes_' + tag))
        main(args + ['--out', out1])
        monkeypatch.setenv('AMT_CONVERT_CLASSES', '1')
        main(args + ['--out', out2])
        monkeypatch.delenv('AMT_CONVERT_CLASSES')
        same_files(out1, out2, names)
        return out1, out2

    hdr = json.load(open(os.path.join(d, 'frame01.json')))
    m = getMapping(np.load(os.path.join(d, 'frame01.npy')), hdr, fastCenterCalculation=True,
                   identifier='frame01').maskedByElevation(10)

    def check(out, want, lats=True):
        got = read_arrays(os.path.join(out, 'frame01.nc'))
        if lats:
            assert np.array_equal(got['lats'].filled(np.nan), want.lats.filled(np.nan), equal_nan=True), out
        assert np.array_equal(got['img'].filled(0), want.img.filled(0)), out
        assert np.array_equal(ma.getmaskarray(got['img']), ma.getmaskarray(want.img)), out
        assert np.allclose(got['elevation'].filled(-1), want.elevation.filled(-1), atol=1e-4), out   # float32 zenith angle
        return got

    base = ['--data', d, '--format', 'netcdf', '--resample', '--min-elevation', '10']
    # a geographic grid at a fixed px/deg, fine enough for binning to leave holes
    geo = base + ['--grid', 'geo', '--px-per-deg', '25', '--without-mag']
    out1, out2 = both(geo + ['--gather', 'linear'], 'geo')
    want = resampleGather(m, pxPerDeg=25, interpolation='linear')
    for out in (out1, out2):
        gathered = check(out, want, lats=False)
    # ... supersampled, with a minimum coverage
    out3, out4 = both(geo + ['--gather', 'linear', '--supersample', '4', '--min-coverage', '0.5'], 'geo_x4')
    want4 = resampleGather(m, pxPerDeg=25, interpolation='linear', supersample=4, minCoverage=0.5)
    for out in (out3, out4):
        check(out, want4, lats=False)
    assert not np.array_equal(want.img.filled(0), want4.img.filled(0))
    # the --grid MLat/MLT form at --resolution (the defaults)
    out5, out6 = both(base + ['--resolution', '900', '--gather', 'linear'], 'mag')
    want = resampleGatherMLatMLT(m, arcsecPerPx=900, interpolation='linear')
    for out in (out5, out6):
        check(out, want)
    out7, out8 = both(base + ['--resolution', '900', '--gather', 'nearest', '--supersample', '2'], 'mag_x2')
    want = resampleGatherMLatMLT(m, arcsecPerPx=900, interpolation='nearest', supersample=2)
    for out in (out7, out8):
        check(out, want)
    # the gathered grid is the grid of the mean at the same arguments, without its holes, and the files hold the same variables
    main(geo + ['--out', str(tmp_path / 'mean_geo')])
    mean = read_arrays(os.path.join(str(tmp_path / 'mean_geo'), 'frame01.nc'))
    assert sorted(mean) == sorted(gathered) and mean['img'].shape == gathered['img'].shape
    assert ma.getmaskarray(mean['img']).sum() > ma.getmaskarray(gathered['img']).sum()


def test_grid_mapping_takes_a_plain_elevation():
    from auromat_amd.cli.convert import grid_mapping
    from datetime import datetime
    lat, lon = np.meshgrid(np.linspace(50, 50.3, 4), np.linspace(10, 10.4, 5), indexing='ij')
    lat_c, lon_c = (lat[:-1, :-1] + lat[1:, 1:]) / 2, (lon[:-1, :-1] + lon[1:, 1:]) / 2
    mask = np.zeros((3, 4), dtype=bool)
    mask[0, 1] = True
    elevation = np.arange(12, dtype=np.float64).reshape(3, 4) + 20.0
    elevation[0, 1] = np.nan
    res = dict(lat=lat, lon=lon, lat_c=lat_c, lon_c=lon_c, img=np.full((3, 4, 3), 7, np.uint16), mask=mask)
    cam, t = np.array([7000.0, 0.0, 0.0]), datetime(2012, 1, 25, 9, 26, 55)
    plain = grid_mapping(dict(res, elevation=elevation), cam, t, 110, 'g', False)
    block = np.dstack([np.zeros((3, 4, 3)), elevation])
    blocks = grid_mapping(dict(res, mean=block), cam, t, 110, 'g', False)
    for m in (plain, blocks):
        assert np.array_equal(np.ma.getmaskarray(m.elevation), mask)
        assert np.array_equal(m.elevation.filled(-1), np.where(mask, -1, elevation))
    # a block still has precedence, as ever
    both = grid_mapping(dict(res, elevation=elevation + 1, mean=block), cam, t, 110, 'g', False)
    assert np.array_equal(both.elevation.filled(-1), blocks.elevation.filled(-1))
