"""Times of the three lens kernels on one device-resident 4240 x 2832 x 3 uint16 frame (ptlens at a realistic strength), beside
torch.nn.functional.grid_sample(mode='bilinear') on the same frame as the yardstick for the 2 x 2 taps.  Kept out of bench.py;
there is no threshold.

  coords      amt_lens_coords on the frame's pixels (float64 + float32 out: 24 bytes per pixel written)
  undistort   amt_lens_undistort on the corner lattice (16 bytes per corner written)
  lanczos4    amt_lens_remap, 8 x 8 taps; floor: 72 MB read + 72 MB written
  linear      amt_lens_remap, 2 x 2 taps
  gather      amt_lens_remap, 8 x 8 taps, every tile forced to take its taps from global memory
  grid_sample bilinear, align_corners=True, zeros padding, float32 (1, 3, H, W) input with a precomputed grid

usage: lens_time.py [--reps R] [--width W --height H]
           one JSON line: medians of device-event times over R calls after one warm-up call of each
       lens_time.py --trace [--calls N]
           N calls of each and nothing else, for a run of its own under
           ``rocprofv3 --kernel-trace --stats -d DIR -- python tools/lens_time.py --trace``
       lens_time.py --summarise DIR/.../<pid>_results.db
           per kernel of that run: launches and the median of the calls after the first, in microseconds"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--width', type=int, default=4240)
ap.add_argument('--height', type=int, default=2832)
ap.add_argument('--trace', action='store_true')
ap.add_argument('--calls', type=int, default=6)
ap.add_argument('--summarise')
ap.add_argument('--channels', type=int, default=3, help='1, 3 or 4 (grid_sample is left out unless 3)')
a = ap.parse_args()

if a.summarise:
    import re
    import sqlite3
    rows = sqlite3.connect(a.summarise).execute('select name, duration from kernels order by start').fetchall()
    per = {}
    for name, dur in rows:
        m = re.search(r'(k_lens_coords<[a-z]*>|k_remap<[^(]*>|grid_sampler[a-z0-9_]*)', name.replace('(anonymous namespace)::', ''))
        if m:
            per.setdefault(re.sub(r'\s+', '', m.group(1)), []).append(dur / 1e3)
    for k, v in per.items():
        # the 8-tap kernel serves two entries of the call list (staged, then forced to gather): `--calls` launches each, in that order
        groups = [v[i:i + a.calls] for i in range(0, len(v), a.calls)] if len(v) >= 2 * a.calls and len(v) % a.calls == 0 else [v]
        for g, part in enumerate(groups):
            rest = part[1:] or part
            print('%-60s %s%3d launches  median after the first %9.1f us  (min %.1f, max %.1f)'
                  % (k, 'group %d  ' % g if len(groups) > 1 else '', len(part), np.median(rest), min(rest), max(rest)))
    sys.exit(0)

import torch
from auromat_amd.synthetic import frame_image
from auromat_amd.util.lensdistortion import PATH_GATHER, LensModifier

w, h = a.width, a.height
mod = LensModifier('ptlens', [0.00211, -0.01013, 0.00397], w, h)
host = frame_image(w, h, seed=1)
host = np.ascontiguousarray(host[:, :, :a.channels]) if a.channels <= 3 else np.concatenate((host, host[:, :, :1]), axis=2)
img = torch.from_numpy(host.view(np.int16)).cuda()
imgf = torch.from_numpy(frame_image(w, h, seed=1).astype(np.float32)).cuda().permute(2, 0, 1).unsqueeze(0).contiguous()
xy = mod.forward_coordinates_device()
grid = torch.stack((xy[..., 0] / (w - 1) * 2 - 1, xy[..., 1] / (h - 1) * 2 - 1), dim=-1).to(torch.float32).unsqueeze(0).contiguous()
torch.cuda.synchronize()

calls = [('coords', lambda: mod.forward_coordinates_device(float32=True)),
         ('undistort', lambda: mod.undistorted_coordinates_device(corner=True)),
         ('lanczos4', lambda: mod.remap_device(img, 'lanczos4')),
         ('linear', lambda: mod.remap_device(img, 'linear')),
         ('gather', lambda: mod.remap_device(img, 'lanczos4', force_path=PATH_GATHER)),
         ('grid_sample', lambda: torch.nn.functional.grid_sample(imgf, grid, mode='bilinear', padding_mode='zeros', align_corners=True))]
if a.channels != 3:
    calls.pop()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


if a.trace:
    for name, fn in calls:
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
    sys.exit(0)

times = {}
for name, fn in calls:
    fn()
    torch.cuda.synchronize()
    times[name] = [timed(fn) for _ in range(a.reps)]
med = {k: float(np.median(v)) for k, v in times.items()}
print(json.dumps(dict(frame=[w, h, a.channels], dtype='uint16', reps=a.reps, ms={k: round(v, 4) for k, v in med.items()},
                      remap_bytes=2 * w * h * 2 * a.channels, all={k: [round(x, 4) for x in v] for k, v in times.items()})), flush=True)
