"""
The plain form of bench.py (no --full): one timed region of exactly --steps steps, nothing measured beside the headline figure,
and --dump-outputs writing what the last timed step computed — the same arrays, bit for bit, in two runs with the same arguments.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(out_dir, steps):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '2',
                          '--dump-outputs', str(out_dir)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_its_steps_once_and_dumps_the_last_step(tmp_path):
    steps = 7
    out = _bench(tmp_path / 'a', steps)
    assert out['n_gpus'] == 1 and out['steps'] == steps and out['warmup'] == 2
    assert out['unit'] == 'Mpixels/s' and out['higher_is_better'] is True and out['dtype'] == 'f64'
    # one region of `steps` steps: ms_per_step is that region over the steps, and the value is the pixels over the same time
    assert out['repeats'] == 1 and len(out['regions_ms']) == 1
    assert out['ms_per_step'] == pytest.approx(out['regions_ms'][0] / steps, rel=1e-9)
    assert out['value'] == pytest.approx(steps * 4240 * 2832 / 1e6 / (out['ms_per_step'] * steps * 1e-3), rel=1e-9)
    assert out['config']['single_pass_frames'] == steps
    # nothing beside the headline figure
    assert 'variants' not in out and out['cpu_baseline'] is None and 'parity' not in out
    assert out['roofline']['measured_copy_GBs'] is None and out['roofline']['measured_fill_GBs'] is None

    files = sorted(os.listdir(str(tmp_path / 'a')))
    assert files == sorted(n + '.npy' for n in ('mean', 'count', 'img', 'mask', 'lat', 'lon', 'lat_c', 'lon_c')), files
    got = {f[:-4]: np.load(str(tmp_path / 'a' / f)) for f in files}
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    ny, nx = out['config']['grid'][:2]
    assert got['mean'].shape == (ny, nx, 4) and got['count'].shape == (ny, nx) and got['img'].shape == (ny, nx, 3)
    assert got['lat_c'].shape == (ny, nx) and got['lat'].shape == (ny + 1, nx + 1)
    filled = got['count'] > 0
    assert filled.any() and np.array_equal(got['mask'] == 1, ~filled)
    assert not got['mean'][~filled].any()                  # an empty cell's NaN mean is written as 0
    assert np.array_equal(got['img'], np.round(got['img'])) and got['img'].max() <= 65535

    # the same arguments give the same inputs, hence the same outputs
    again = _bench(tmp_path / 'b', steps)
    assert again['config']['grid'] == out['config']['grid']
    for name, a in got.items():
        assert np.array_equal(a, np.load(str(tmp_path / 'b' / (name + '.npy'))), equal_nan=True), name
