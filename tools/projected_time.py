"""Times of the map-projected resampling on one device-resident synthetic 4240 x 2832 frame (uint8 RGB, elevation >= 10 deg), as
tools/area_time.py does it for the plate-carree grid.  Kept out of bench.py; there is no threshold: these are the numbers from
which the two-pass form (project, then bin) is judged against a fused one.

  forward   amt_project_forward on the frame's 12.0 M corners (stereographic, WGS84, centred on the frame's bounding box): ms
            between two device events around one call, and the achieved GB/s against 32 bytes per point (two doubles in, two out)
  plane     amt_area_plane_frame + amt_area_frame_finalize on the projected corners at 3.092 km per pixel (100 arcsec), the
            accumulators' zeroing included
  area      resample_frame_area at 25 px/deg on the same frame (a cell is 4.4 km of latitude: the closest standard grid), host
            work and read-back included, as tools/area_time.py measures it
  whole     resampleStereographic's device work on the frame: resample_frames_projected, host work and read-back included

usage: projected_time.py [--reps R] [--width W --height H]
           one JSON line: medians over R calls after one warm-up call of each, every call's figure
       projected_time.py --trace [--calls N]
           N calls of forward + plane and nothing else, for a run of its own under
           ``rocprofv3 --kernel-trace --stats -d DIR -- python tools/projected_time.py --trace``"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--width', type=int, default=4240)
ap.add_argument('--height', type=int, default=2832)
ap.add_argument('--trace', action='store_true')
ap.add_argument('--calls', type=int, default=3)
a = ap.parse_args()

import torch
from auromat_amd import resample as R
from auromat_amd._native import ptr
from auromat_amd.coordinates.projection import Stereographic
from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
from auromat_amd.synthetic import frame_header, frame_image
from auromat_amd.util.histogram import make_axis

hdr, cam, t = frame_header(a.width, a.height)
m = ArraySpacecraftMapping(hdr, 110, frame_image(a.width, a.height, seed=1, dtype=np.uint8), cam, t, 'n', fastCenterCalculation=True)
masked = m.maskedByElevation(10)
fd, box = masked.frame(), masked.boundingBox
fd.img
ctx = fd.ctx
lat0, lon0, width, height = R.stereographic_geometry([box])
km = R.projected_km_per_px(None, 100)
xE, yE = R.projected_edges(width, km), R.projected_edges(height, km)
P = Stereographic(lat0, lon0)
(xaxis, _), (yaxis, _) = make_axis(ctx, xE, uniform=True), make_axis(ctx, yE, uniform=True)
nx, ny, nch = len(xE) - 1, len(yE) - 1, fd.nchan
n = fd.lat.numel()
x, y = ctx.empty(fd.lat.shape), ctx.empty(fd.lat.shape)
least = R.min_coverage_weight(0.5)
grid = R._PlaneGrid(xE, yE)
outs = R._bin_outputs(ctx, grid, nch, fd.img_dtype_code)
torch.cuda.synchronize()


def forward():
    ctx.call('amt_project_forward', C.byref(P.params), ptr(fd.lat), ptr(fd.lon), n, ptr(x), ptr(y))


def plane():
    acc = ctx.zeros((nch + 2, nx * ny), torch.int64)
    ctx.call('amt_area_plane_frame', ptr(x), ptr(y), ptr(fd.lat_c), ptr(fd.elev), ptr(fd.img), fd.img_dtype_code or 1, nch,
             ptr(fd.center_mask), fd.height, fd.width, float('-inf'), C.byref(xaxis), C.byref(yaxis), ptr(acc))
    area, img, mask, coverage = outs
    ctx.call('amt_area_frame_finalize', ptr(acc), nx, ny, nch, fd.img_dtype_code or 1, least, ptr(area), ptr(img), ptr(mask),
             ptr(coverage))


def area():
    return R.resample_frame_area(fd, m.altitude, box, (25, 25))


def whole():
    return R.resample_frames_projected([fd], P, xE, yE)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


if a.trace:
    for _ in range(a.calls):
        forward()
        plane()
    torch.cuda.synchronize()
    sys.exit(0)

times = {}
for name, fn in (('forward', forward), ('plane', plane), ('area', area), ('whole', whole)):
    fn()
    torch.cuda.synchronize()
    times[name] = [timed(fn) for _ in range(a.reps)]
med = {k: float(np.median(v)) for k, v in times.items()}
ra = area()
print(json.dumps(dict(frame=[a.width, a.height], corners=n, reps=a.reps, km_per_px=round(km, 6), plane_grid=[ny, nx],
                      area_grid_25ppd=list(ra['mask'].shape), forward_ms=round(med['forward'], 4),
                      forward_GBps=round(32.0 * n / (med['forward'] * 1e-3) / 1e9, 1), plane_ms=round(med['plane'], 3),
                      area_25ppd_ms=round(med['area'], 3), whole_ms=round(med['whole'], 3),
                      all={k: [round(v, 4) for v in vs] for k, vs in times.items()},
                      cells_valid_plane=int((outs[2] == 0).sum().item()), cells_valid_area=int((~ra['mask']).sum()))), flush=True)
