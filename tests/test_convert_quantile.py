"""
``auromat-convert --statistic quantile --quantile Q`` on the MI355X: both routes — the sequence pipeline and the mapping
classes (AMT_CONVERT_CLASSES=1) — write equal files, and a frame equals resampleQuantileMLatMLT / resampleQuantile of the
class API.  (The parser is covered without a GPU in tests/test_quantile_cpu.py.)
"""
import json
import os

import numpy as np
import numpy.ma as ma
import pytest

from test_convert_cli import write_frames

Q = 0.75


@pytest.mark.gpu
def test_convert_quantile_both_routes(tmp_path, monkeypatch):
    from auromat_amd.cli.convert import main
    from auromat_amd.mapping.netcdf import read_arrays
    from auromat_amd.mapping.spacecraft import getMapping
    from auromat_amd.resample import resampleMedian, resampleQuantile, resampleQuantileMLatMLT
    d = write_frames(tmp_path)
    names = ['frame00.nc', 'frame01.nc', 'frame02.nc']
    # MLat/MLT grid at --resolution (the defaults), through the sequence pipeline and through the classes
    args = ['--data', d, '--format', 'netcdf', '--resample', '--min-elevation', '10', '--resolution', '900', '--statistic',
            'quantile', '--quantile', str(Q)]
    out1, out2 = str(tmp_path / 'pipe'), str(tmp_path / 'classes')
    main(args + ['--out', out1])
    monkeypatch.setenv('AMT_CONVERT_CLASSES', '1')
    main(args + ['--out', out2])
    monkeypatch.delenv('AMT_CONVERT_CLASSES')
    assert sorted(os.listdir(out1)) == sorted(os.listdir(out2)) == names
    for name in names:
        a, b = read_arrays(os.path.join(out1, name)), read_arrays(os.path.join(out2, name))
        for key in ('lats', 'lons', 'img', 'elevation'):
            assert np.array_equal(ma.getmaskarray(a[key]), ma.getmaskarray(b[key])), (name, key)
            assert np.array_equal(a[key].filled(0), b[key].filled(0)), (name, key)
    hdr = json.load(open(os.path.join(d, 'frame01.json')))
    m = getMapping(np.load(os.path.join(d, 'frame01.npy')), hdr, fastCenterCalculation=True,
                   identifier='frame01').maskedByElevation(10)
    want = resampleQuantileMLatMLT(m, Q, arcsecPerPx=900)
    got = read_arrays(os.path.join(out1, 'frame01.nc'))
    assert np.array_equal(got['lats'].filled(np.nan), want.lats.filled(np.nan), equal_nan=True)
    assert np.array_equal(got['img'].filled(0), want.img.filled(0))
    assert np.array_equal(ma.getmaskarray(got['img']), ma.getmaskarray(want.img))
    assert np.allclose(got['elevation'].filled(-1), want.elevation.filled(-1), atol=1e-4)   # stored as float32 zenith angle
    # a fixed px/deg on a geographic grid
    args = ['--data', d, '--format', 'netcdf', '--resample', '--min-elevation', '10', '--grid', 'geo', '--px-per-deg', '5',
            '--statistic', 'quantile', '--quantile', str(Q), '--without-mag']
    out3, out4 = str(tmp_path / 'pipe_geo'), str(tmp_path / 'classes_geo')
    main(args + ['--out', out3])
    monkeypatch.setenv('AMT_CONVERT_CLASSES', '1')
    main(args + ['--out', out4])
    monkeypatch.delenv('AMT_CONVERT_CLASSES')
    want = resampleQuantile(m, Q, pxPerDeg=5)
    for out in (out3, out4):
        got = read_arrays(os.path.join(out, 'frame01.nc'))
        assert np.array_equal(got['img'].filled(0), want.img.filled(0)), out
        assert np.array_equal(ma.getmaskarray(got['img']), ma.getmaskarray(want.img)), out
    # the upper quartile is not the median here (the grids would not tell the two apart otherwise)
    assert not np.array_equal(resampleMedian(m, pxPerDeg=5).img.filled(0), want.img.filled(0))
