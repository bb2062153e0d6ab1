"""Per-frame time of area-weighted sequences (SequencePipeline(statistic='area'): the native runner's area pass,
amt_area_frame_async) on full-size synthetic frames (4240 x 2832, uint8 RGB, elevation >= 10 deg) pushed as a sequence of
device-resident images, at 10 px/deg and at 100 arcsec/px, on geographic and magnetic grids.  Kept out of bench.py; there is no
threshold: the one-frame call (tools/area_time.py: resample_frame_area, host work and read-back included) and the median
sequence (tools/median_sequence_time.py) are the yardsticks beside which the numbers are read.

usage: area_sequence_time.py [--frames N] [--reps R] [--only geo-ppd10,...] [--width W --height H]
One JSON line per configuration: ms per frame between two device events around one process() call of N frames, the median over R
calls after one warm-up call, every call's figure, and the frames processed in all (for dividing a kernel trace's totals:
``rocprofv3 --kernel-trace --stats -d DIR -- python tools/area_sequence_time.py --reps 1``, in a run of its own)."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=24)
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--only', default='')
ap.add_argument('--width', type=int, default=4240)
ap.add_argument('--height', type=int, default=2832)
a = ap.parse_args()

import torch
from auromat_amd.pipeline import SequencePipeline
from auromat_amd.synthetic import frame_image, sequence_frame

w, h = a.width, a.height
imgs = [torch.from_numpy(frame_image(w, h, seed=k, dtype=np.uint8)).cuda() for k in range(4)]    # four images, used in turn
frames = [sequence_frame(k, w, h)[:3] + (imgs[k % 4],) for k in range(a.frames)]
only = set(filter(None, a.only.split(',')))

for grid in ('geo', 'mag'):
    for res, kw in (('ppd10', dict(pxPerDeg=10)), ('arcsec100', dict(arcsecPerPx=100))):
        name = '%s-%s' % (grid, res)
        if only and name not in only:
            continue
        seq = SequencePipeline(w, h, img_dtype=np.uint8, magnetic=grid == 'mag', batch=3, statistic='area', min_elevation=10.0,
                               own_image_buffers=False, **kw)
        seq.process(frames, keep_on_device=True)
        torch.cuda.synchronize()
        times = []
        for rep in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            seq.process(frames, keep_on_device=True)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / a.frames)
        print(json.dumps(dict(config=name, frame=[w, h], frames=a.frames, reps=a.reps,
                              ms_per_frame=round(float(np.median(times)), 4), ms_per_frame_all=[round(x, 4) for x in times],
                              plans=sorted(set(seq.plans)), frames_processed=a.frames * (a.reps + 1))), flush=True)
