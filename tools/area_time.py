"""Time of the area-weighted binning (resample_frame_area: amt_area_frame + amt_area_frame_finalize) beside the mean's two-pass
binning (resample_frame(method='mean'): amt_bin_frame + amt_bin_frame_finalize) on one device-resident synthetic 4240 x 2832
frame, elevation >= 10 deg, at 10 and at 50 px/deg.  Kept out of bench.py; there is no threshold: the mean is the yardstick
beside which the number is read.

usage: area_time.py [--reps R] [--width W --height H]
           one JSON line per resolution: ms between two device events around one call (host work and read-back of the grid
           included), medians over R calls of each, the two alternating, after one warm-up call of each
       area_time.py --trace [--calls N]
           N area calls per resolution and nothing else, for a run of its own under
           ``rocprofv3 --kernel-trace --stats -d DIR -- python tools/area_time.py --trace``"""
import argparse, json, os, sys
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
from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
from auromat_amd.synthetic import frame_header, frame_image

hdr, cam, t = frame_header(a.width, a.height)
m = ArraySpacecraftMapping(hdr, 110, frame_image(a.width, a.height, seed=1, dtype=np.uint8), cam, t, 'n', fastCenterCalculation=True)
fd, box = m.frame(), m.maskedByElevation(10).boundingBox
fd.img
torch.cuda.synchronize()


def area(ppd):
    return R.resample_frame_area(fd, m.altitude, box, (ppd, ppd), min_elevation=10.0)


def mean(ppd):
    return R.resample_frame(fd, m.altitude, box, (ppd, ppd), min_elevation=10.0)


def timed(fn, ppd):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(ppd)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for ppd in (10, 50):
    if a.trace:
        for _ in range(a.calls):
            area(ppd)
        continue
    ra, rm = area(ppd), mean(ppd)
    ta, tm = [], []
    for _ in range(a.reps):
        ta.append(timed(area, ppd))
        tm.append(timed(mean, ppd))
    print(json.dumps(dict(px_per_deg=ppd, frame=[a.width, a.height], grid=list(ra['mask'].shape), reps=a.reps,
                          area_ms=round(float(np.median(ta)), 3), mean_ms=round(float(np.median(tm)), 3),
                          area_ms_all=[round(v, 3) for v in ta], mean_ms_all=[round(v, 3) for v in tm],
                          cells_filled_area=int((~ra['mask']).sum()), cells_filled_mean=int((~rm['mask']).sum()))), flush=True)
