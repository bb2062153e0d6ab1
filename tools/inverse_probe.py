"""Times of the world -> pixel kernels and of gather resampling on one MI355X, beside resample(method='linear') on the same frame.
Kept out of bench.py; there is no threshold and no test depends on a time.

  world_to_pixel   amt_world_to_pixel on N random geodetic points inside the headline frame's footprint (device events,
                   device-resident inputs and outputs: 16 bytes read, 25 written per point)
  grid_to_pixel    amt_grid_to_pixel on the 0.1 deg grid and on the grid of the frame's own arcsecPerPx (float32 coordinates,
                   elevation and flags: 17 bytes written per cell)
  gather           resampleGather(mapping.maskedByElevation(10), ...) of the headline 4240 x 2832 frame, host clock around the whole
                   call (box pass, grid, coordinates, sampling, the copies to the host and the result mapping), 'linear'
  linear           resample(mapping.maskedByElevation(10), method='linear') on the same frame and grid, host clock

usage: inverse_probe.py [--points N] [--reps R] [--width W --height H] [--arcsec A] [--skip-linear]
           one JSON line; medians over R calls after one warm-up call of each
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--points', type=int, default=10 ** 7)
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--width', type=int, default=4240)
ap.add_argument('--height', type=int, default=2832)
ap.add_argument('--arcsec', type=float, default=None, help="arcsecPerPx of the fine grid (default: the frame's own pixel scale)")
ap.add_argument('--skip-linear', action='store_true')
a = ap.parse_args()

import ctypes as C
import torch
from auromat_amd._native import Context, ptr
from auromat_amd.coordinates.inverse import W2P_GEODETIC, grid_to_pixel
from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
from auromat_amd.resample import gather_plan, grid_coordinates, resample, resampleGather
from auromat_amd.synthetic import frame_header, frame_image

if not torch.cuda.is_available():
    sys.exit('inverse_probe.py measures on a GPU; none is visible')
ctx = Context.current()
w, h = a.width, a.height
hdr, cam, t = frame_header(w, h)
img = frame_image(w, h, seed=1)
arcsec = a.arcsec or 3600.0 * float(np.hypot(hdr['CD1_1'], hdr['CD2_1']))


def mapping():
    return ArraySpacecraftMapping(hdr, 110, img, cam, t, 'probe', fastCenterCalculation=True).maskedByElevation(10)


def events(fn, reps):
    fn()
    ctx.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = ctx.event(), ctx.event()
        ctx.record(e0)
        fn()
        ctx.record(e1)
        out.append(ctx.elapsed_ms(e0, e1))
        ctx.destroy_event(e0)
        ctx.destroy_event(e1)
    return float(np.median(out))


def clock(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


res = dict(device=ctx.device_info()['name'], frame=[w, h], reps=a.reps)
plan = gather_plan(mapping(), pxPerDeg=10)
params = plan['params']
g = plan['grid']
rng = np.random.RandomState(0)
lat = ctx.to_device(rng.uniform(g.latCenters.min(), g.latCenters.max(), a.points))
lon = ctx.to_device(rng.uniform(g.lonCenters.min(), g.lonCenters.max(), a.points))
xy, el, fl = ctx.empty((a.points, 2)), ctx.empty((a.points,)), ctx.empty((a.points,), torch.uint8)
ms = events(lambda: ctx.call('amt_world_to_pixel', C.byref(params), None, W2P_GEODETIC, ptr(lat), ptr(lon), a.points, ptr(xy), ptr(el),
                             ptr(fl)), a.reps)
res['world_to_pixel'] = dict(points=a.points, ms=ms, points_per_us=a.points / ms / 1e3, in_frame=float((fl == 0).float().mean().item()))
del lat, lon, xy, el, fl

for label, kw in (('0.1deg', dict(pxPerDeg=10)), ('own_scale', dict(arcsecPerPx=arcsec))):
    plan = gather_plan(mapping(), **kw)
    coords = grid_coordinates(plan)
    la, lo = ctx.to_device(np.ascontiguousarray(coords['lat_c'][:, 0])), ctx.to_device(np.ascontiguousarray(coords['lon_c'][0, :]))
    ms = events(lambda: grid_to_pixel(ctx, params, None, W2P_GEODETIC, la, lo), a.reps)
    res['grid_to_pixel_' + label] = dict(grid=[plan['grid'].ny, plan['grid'].nx], ms=ms, cells_per_us=plan['grid'].ny * plan['grid'].nx / ms / 1e3)
    res['gather_' + label] = dict(ms=clock(lambda: resampleGather(mapping(), interpolation='linear', **kw), max(3, a.reps // 2)), **kw)
    if not a.skip_linear and label == '0.1deg':
        res['linear_' + label] = dict(ms=clock(lambda: resample(mapping(), method='linear', **kw), 3), **kw)
print(json.dumps(res))
