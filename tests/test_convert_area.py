"""
``auromat-convert --statistic area [--min-coverage F]``: the parser (CPU) and both routes on the MI355X — the sequence pipeline and
the mapping classes (AMT_CONVERT_CLASSES=1) — against resampleAreaMLatMLT / resampleArea of the class API.
"""
import json
import os

import numpy as np
import numpy.ma as ma
import pytest

from test_convert_cli import write_frames


def test_area_flags_parse(capsys):
    from auromat_amd.cli.convert import parseargs
    base = ['--data', '/nonexistent', '--format', 'netcdf']
    a = parseargs(base + ['--resample', '--statistic', 'area'])
    assert a.statistic == 'area' and a.minCoverage == 0.5
    a = parseargs(base + ['--resample', '--statistic', 'area', '--min-coverage', '0'])
    assert a.minCoverage == 0.0
    assert parseargs(base + ['--resample', '--statistic', 'area', '--min-coverage', '1']).minCoverage == 1.0
    assert parseargs(base + ['--resample']).minCoverage is None
    for bad, message in ((['--resample', '--statistic', 'area', '--min-coverage', '1.5'], '--min-coverage must be in the range [0, 1]'),
                         (['--resample', '--statistic', 'area', '--min-coverage', '-0.1'], '--min-coverage must be in the range [0, 1]'),
                         (['--resample', '--statistic', 'area', '--min-coverage', 'nan'], '--min-coverage must be in the range [0, 1]'),
                         (['--resample', '--min-coverage', '0.5'], '--min-coverage is only usable with --statistic area'),
                         (['--resample', '--statistic', 'median', '--min-coverage', '0.5'],
                          '--min-coverage is only usable with --statistic area'),
                         (['--statistic', 'area'], '--statistic area needs --resample'),
                         (['--statistic', 'area', '--min-coverage', '0.5'], '--statistic area needs --resample')):
        with pytest.raises(SystemExit) as e:
            parseargs(base + bad)
        assert e.value.code != 0
        assert message in capsys.readouterr().err, bad
    from auromat_amd.cli.convert import getParser
    text = getParser().format_help()
    assert '--min-coverage' in text and 'area' in text


def same_files(out1, out2, names):
    from auromat_amd.mapping.netcdf import read_arrays
    assert sorted(os.listdir(out1)) == sorted(os.listdir(out2)) == names
    for name in names:
        a, b = read_arrays(os.path.join(out1, name)), read_arrays(os.path.join(out2, name))
        assert sorted(a) == sorted(b), name                     # the variables a mean grid's files hold, on both routes
        for key in ('lats', 'lons', 'img', 'elevation'):
            assert np.array_equal(ma.getmaskarray(a[key]), ma.getmaskarray(b[key])), (name, key)
            assert np.array_equal(a[key].filled(0), b[key].filled(0)), (name, key)


@pytest.mark.gpu
def test_convert_area_both_routes(tmp_path, monkeypatch):
    from auromat_amd.cli.convert import main
    from auromat_amd.mapping.netcdf import read_arrays
    from auromat_amd.mapping.spacecraft import getMapping
    from auromat_amd.resample import resampleArea, resampleAreaMLatMLT
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

    # MLat/MLT grid at --resolution (the defaults), the default minimum coverage
    base = ['--data', d, '--format', 'netcdf', '--resample', '--min-elevation', '10']
    out1, out2 = both(base + ['--resolution', '900', '--statistic', 'area'], 'mag')
    want = resampleAreaMLatMLT(m, arcsecPerPx=900)
    for out in (out1, out2):
        check(out, want)
    # a fixed px/deg on a geographic grid, fine enough for the mean to leave holes, with --min-coverage
    geo = base + ['--grid', 'geo', '--px-per-deg', '25', '--without-mag']
    out3, out4 = both(geo + ['--statistic', 'area', '--min-coverage', '0.25'], 'geo')
    want = resampleArea(m, pxPerDeg=25, minCoverage=0.25)
    for out in (out3, out4):
        area = check(out, want, lats=False)
    assert not np.array_equal(ma.getmaskarray(want.img), ma.getmaskarray(resampleArea(m, pxPerDeg=25).img))
    # the area-weighted grid is not the mean's, and holds the variables the mean's file holds
    main(geo + ['--out', str(tmp_path / 'mean_geo')])
    mean = read_arrays(os.path.join(str(tmp_path / 'mean_geo'), 'frame01.nc'))
    assert sorted(mean) == sorted(area)
    assert mean['img'].shape == area['img'].shape
    assert ma.getmaskarray(mean['img']).sum() > ma.getmaskarray(area['img']).sum()      # the holes between the centres are filled
