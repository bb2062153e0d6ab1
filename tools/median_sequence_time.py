"""Per-frame wall time of median sequences (SequencePipeline(statistic='median'), the native runner's median pass) against
the mean sequence and a resampleMedian loop over the class API, on the reference's full-size test frame (4256 x 2832, uint8
RGB) pushed as a sequence of device-resident frames.  Kept out of bench.py.

usage: median_sequence_time.py [--frames N] [--reps R] [--only median-geo-ppd10,...] [--no-class]
One JSON line per configuration: ms per frame (median over R timed calls of N frames, after one warm-up call) and the
frames processed in all (for dividing a kernel trace's totals)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from auromat_amd.fits import readHeader
from auromat_amd.mapping.spacecraft import frame_inputs, getMapping
from auromat_amd.pipeline import SequencePipeline
from auromat_amd.resample import resampleMedian
from auromat_amd.util.image import loadImage

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=24)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--only', default='')
ap.add_argument('--no-class', action='store_true')
a = ap.parse_args()
G = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'resources')
arr = loadImage(os.path.join(G, 'ISS030-E-102170_dc.jpg'))
wcs = readHeader(os.path.join(G, 'ISS030-E-102170_dc.wcs'))
cam, t = frame_inputs(wcs)
h, w = arr.shape[:2]
imgs = [torch.from_numpy(np.array(arr)).cuda() for _ in range(4)]       # four device-resident images, used in turn
frames = [(wcs, cam, t, imgs[k % 4]) for k in range(a.frames)]
only = set(filter(None, a.only.split(',')))

for stat in ('median', 'mean'):
    for grid in ('geo', 'mag'):
        for res, kw in (('ppd10', dict(pxPerDeg=10)), ('arcsec100', dict(arcsecPerPx=100))):
            name = '%s-%s-%s' % (stat, grid, res)
            if only and name not in only:
                continue
            seq = SequencePipeline(w, h, img_dtype=np.uint8, magnetic=grid == 'mag', batch=3, statistic=stat,
                                   own_image_buffers=False, keep_coordinates=False, **kw)
            seq.process(frames, keep_on_device=True)
            torch.cuda.synchronize()
            times = []
            for rep in range(a.reps):
                t0 = time.perf_counter()
                seq.process(frames, keep_on_device=True)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            print(json.dumps(dict(config=name, frames=a.frames, ms_per_frame=round(1e3 * float(np.median(times)) / a.frames, 4),
                                  calls_ms=[round(1e3 * x, 2) for x in times], plans=sorted(set(seq.plans)),
                                  frames_processed=a.frames * (a.reps + 1))), flush=True)

if not a.no_class and (not only or 'class-geo-ppd10' in only):
    times = []
    for rep in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = getMapping(arr, wcs, altitude=110, fastCenterCalculation=True).maskedByElevation(10)
        resampleMedian(m, pxPerDeg=10)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    print(json.dumps(dict(config='class-geo-ppd10', what='getMapping + maskedByElevation + resampleMedian per frame',
                          ms_per_frame=round(1e3 * float(np.median(times[1:])), 3))), flush=True)
