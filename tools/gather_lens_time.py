"""Gathering a raw frame through its lens (one interpolation) beside correcting it first (two), on one MI355X.

Workload: one full-size (4240 x 2832) synthetic ISS frame (synthetic.sequence_frame 0) that still carries a ptlens distortion,
uint8 RGB, on the grid resampleGather lays out at `--pxPerDeg` (10 and 25 by default), linear interpolation.
  resample   getMapping(lensRoute='resample'): the Lanczos-4 remap into a corrected image (amt_lens_remap), then resampleGather
             of that image through the camera model
  raw        getMapping(lensRoute='raw'), then resampleGather through the camera model and the lens (amt_grid_to_pixel_lens):
             the raw pixels are interpolated once
Two figures each.  `device`: the work on an existing plan with the image on the device — resample: LensModifier.remap_device +
gather_frame, raw: gather_frame with the plan's lens — warmed up, then timed in alternating regions of `--reps` calls, a host clock
around work that ends in a device synchronise, the median of `--regions` regions.  `class`: the whole class call from the host
arrays, getMapping(...) + resampleGather(...), the median of `--calls` alternating calls (the raw route builds its direction array
and the frame's coordinate arrays for its bounding box, the resample route takes its box from the box pass).
usage: gather_lens_time.py [--reps 20] [--regions 7] [--calls 5] [--pxPerDeg 10 25]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from auromat_amd._native import Context
from auromat_amd.mapping.spacecraft import getMapping
from auromat_amd.resample import gather_frame, gather_plan, resampleGather
from auromat_amd.synthetic import frame_image, sequence_frame
from auromat_amd.util.lensdistortion import LensModifier

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--regions', type=int, default=7)
ap.add_argument('--calls', type=int, default=5)
ap.add_argument('--pxPerDeg', type=int, nargs='+', default=[10, 25])
ap.add_argument('--width', type=int, default=4240)
ap.add_argument('--height', type=int, default=2832)
a = ap.parse_args()

hdr, cam, t, seed = sequence_frame(0, a.width, a.height)
hdr = dict(hdr)
hdr.update({'DATE-OBS': t.strftime('%Y-%m-%dT%H:%M:%S.%f'), 'POSX': float(cam[0]), 'POSY': float(cam[1]), 'POSZ': float(cam[2])})
raw = frame_image(a.width, a.height, seed=seed, dtype=np.uint8)
mod = LensModifier('ptlens', [0.00211, -0.01013, 0.00397], a.width, a.height)
ctx = Context.current()


def mapping(route):
    return getMapping(raw, hdr, lens=mod, lensRoute=route, fastCenterCalculation=True).maskedByElevation(10)


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


result = dict(width=a.width, height=a.height, runs=[])
for ppd in a.pxPerDeg:
    plans = {route: gather_plan(mapping(route), pxPerDeg=ppd) for route in ('resample', 'raw')}
    raw_dev = ctx.to_device(raw, dtype=np.uint8)
    device = dict(resample=lambda: gather_frame(plans['resample'], mod.remap_device(raw_dev), 'linear'),
                  raw=lambda: gather_frame(plans['raw'], raw_dev, 'linear'))
    seen = {k: float((~fn()['mask']).mean()) for k, fn in device.items()}
    for fn in device.values():
        timed(fn, 3)
    regions = {k: [] for k in device}
    for _ in range(a.regions):
        for k, fn in device.items():
            regions[k].append(timed(fn, a.reps))
    classes = {k: [] for k in device}
    for _ in range(a.calls):
        for route in classes:
            classes[route].append(timed(lambda: resampleGather(mapping(route), pxPerDeg=ppd, interpolation='linear'), 1))
    run = dict(pxPerDeg=ppd, cells={k: [plans[k]['grid'].ny, plans[k]['grid'].nx] for k in plans}, seen_fraction=seen,
               device_ms={k: float(np.median(v)) for k, v in regions.items()},
               device_ms_spread={k: [float(min(v)), float(max(v))] for k, v in regions.items()},
               class_ms={k: float(np.median(v)) for k, v in classes.items()},
               class_ms_spread={k: [float(min(v)), float(max(v))] for k, v in classes.items()})
    result['runs'].append(run)
print(json.dumps(result))
