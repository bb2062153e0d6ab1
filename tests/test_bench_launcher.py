"""
`python bench.py --gpus N` without a launcher must start its ranks as CHILD processes (never exec after a GPU call),
hand on rank 0's JSON line and fail when a rank fails.  Runs the real launcher code on the CPU:
--dry-run swaps the GPU work for a sleep and RCCL for gloo.
"""
import json
import os
import subprocess
import sys

from conftest import ROOT


def _run(extra_env=None, *argv):
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(argv), env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, universal_newlines=True, timeout=300)


def test_plain_invocation_with_two_ranks_prints_one_json_line():
    res = _run(None, '--gpus', '2', '--steps', '3', '--warmup', '0', '--dry-run')
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    assert out['n_gpus'] == 2 and out['steps'] == 3 and out['dry_run'] is True and out['value'] > 0
    # the line says who took part: two ranks, two processes, each with its own time
    assert out['ranks'] == 2 and out['backend'] == 'gloo'
    assert [r['rank'] for r in out['per_rank']] == [0, 1] and len(set(r['pid'] for r in out['per_rank'])) == 2
    assert all(r['elapsed_ms'] > 0 and r['frames'] == 3 for r in out['per_rank'])


def test_a_failing_rank_fails_the_whole_run():
    res = _run({'AMT_BENCH_DRYRUN_FAIL_RANK': '1'}, '--gpus', '2', '--steps', '2', '--warmup', '0', '--dry-run')
    assert res.returncode != 0
    assert not [ln for ln in res.stdout.splitlines() if ln.startswith('{"metric"')]


def test_single_rank_runs_in_process():
    res = _run(None, '--steps', '2', '--warmup', '0', '--dry-run')
    assert res.returncode == 0, res.stderr[-2000:]
    assert json.loads(res.stdout.strip().splitlines()[-1])['n_gpus'] == 1


def test_default_steps_are_the_same_per_rank_for_every_n():
    sys.path.insert(0, ROOT)
    import bench
    # weak scaling: the same number of frames per rank whatever N is, and at least the 32 per rank of BASELINE.json
    # configs[4] (256 frames on 8 GPUs = --gpus 8 --steps 32)
    assert bench.parse_args(['--gpus', '8']).steps == bench.parse_args([]).steps >= 32
    assert bench.parse_args(['--gpus', '8', '--steps', '32']).steps * 8 == 256
    assert bench.parse_args([]).gpus == 1


def test_plain_run_is_the_default():
    sys.path.insert(0, ROOT)
    import bench
    args = bench.parse_args(['--steps', '5'])
    assert args.full is False and args.dump_outputs is None and args.steps == 5
    args = bench.parse_args(['--full', '--dump-outputs', 'out'])
    assert args.full is True and args.dump_outputs == 'out'


def test_dump_outputs_writes_the_result_arrays_as_floats_within_the_limit(tmp_path, monkeypatch):
    """--dump-outputs on a result dict of the pipeline's shape (host tensors stand in for the device ones): one .npy per array,
    float32 / float64, values unchanged except the NaN mean of empty cells, which is written as 0 (every value finite); above
    the size limit every k-th grid row of each array, and never more than the limit."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from auromat_amd.resample import cached_grid
    grid = cached_grid((10, 10), 50.0, 56.2, 10.0, 20.1)
    ny, nx = grid.lat_c.shape
    gen = torch.Generator().manual_seed(5)
    res = dict(grid=grid, contains_pole=False, contains_discontinuity=False, altitude=110.0,
               mean=torch.rand(ny, nx, 4, dtype=torch.float64, generator=gen),
               count=torch.randint(0, 9, (ny, nx), generator=gen).double(),
               img=torch.randint(-32768, 32767, (ny, nx, 3), dtype=torch.int16, generator=gen),
               mask=torch.randint(0, 2, (ny, nx), dtype=torch.uint8, generator=gen))
    empty = res['mask'].numpy() == 1
    res['mean'][torch.from_numpy(empty)] = float('nan')            # as the binning leaves an empty cell
    bench.dump_outputs(res, str(tmp_path / 'all'))
    got = {f[:-4]: np.load(str(tmp_path / 'all' / f)) for f in os.listdir(str(tmp_path / 'all'))}
    assert sorted(got) == ['count', 'img', 'lat', 'lat_c', 'lon', 'lon_c', 'mask', 'mean']
    assert all(np.isfinite(a).all() for a in got.values())
    assert got['mean'].dtype == np.float64 and np.array_equal(got['mean'], np.where(empty[..., None], 0.0, res['mean'].numpy()))
    assert got['img'].dtype == np.float32 and np.array_equal(got['img'], res['img'].numpy().view(np.uint16))
    assert got['mask'].dtype == np.float32 and np.array_equal(got['mask'], res['mask'].numpy())
    assert np.array_equal(got['lat'], grid.lat) and np.array_equal(got['lon_c'], grid.lon_c)
    total = sum(a.nbytes for a in got.values())
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', total // 10)
    bench.dump_outputs(res, str(tmp_path / 'sample'))
    part = {f[:-4]: np.load(str(tmp_path / 'sample' / f)) for f in os.listdir(str(tmp_path / 'sample'))}
    assert sum(a.nbytes for a in part.values()) <= total // 10
    assert sorted(part) == sorted(got)
    assert [k for k in range(2, ny + 1) if all(np.array_equal(a, got[name][::k]) for name, a in part.items())]
