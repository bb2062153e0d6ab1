"""resampleMedian(mapping, pxPerDeg=...) against resample(mapping, pxPerDeg=10, method='nearest') through the class API on the
reference's own test frame (4256 x 2832, image as an array), in one run: wall time per call (five calls each, the first
one warms up), and the device time of amt_median_frame alone on the frame.  usage: median_time.py"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from auromat_amd.fits import readHeader
from auromat_amd.mapping.spacecraft import getMapping
from auromat_amd.resample import resample, resampleMedian, resample_frame_median
from auromat_amd.util.image import loadImage
G = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'resources')
arr = loadImage(os.path.join(G, 'ISS030-E-102170_dc.jpg'))
wcs = readHeader(os.path.join(G, 'ISS030-E-102170_dc.wcs'))


def timed(fn, reps=5):
    times = []
    for rep in range(reps):
        mm = getMapping(arr, wcs, altitude=110, fastCenterCalculation=True).maskedByElevation(10)
        mm.frame()                  # georeferencing is not part of either method's time
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = fn(mm)
        torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
    return times[1:], r


for name, fn in (("resample(method='nearest', pxPerDeg=10)", lambda m: resample(m, pxPerDeg=10, method='nearest')),
                 ('resampleMedian(pxPerDeg=10)', lambda m: resampleMedian(m, pxPerDeg=10)),
                 ('resampleMedian(pxPerDeg=0.1)', lambda m: resampleMedian(m, pxPerDeg=0.1))):
    times, r = timed(fn)
    print('%s: %s s (median %.4f), grid %s' % (name, ' / '.join('%.4f' % t for t in times), float(np.median(times)),
                                               r.img.shape), flush=True)

# the device time of the median kernels alone (frame resident, grid cached): events around amt_median_frame
mm = getMapping(arr, wcs, altitude=110, fastCenterCalculation=True).maskedByElevation(10)
fd = mm.frame()
for ppd in (10, 1, 0.1):
    ev = []
    for rep in range(6):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        res = resample_frame_median(fd, mm.altitude, mm.boundingBox, (ppd, ppd), mm.containsDiscontinuity, False)
        e.record(); torch.cuda.synchronize()
        ev.append(s.elapsed_time(e))
    print('resample_frame_median pxPerDeg=%g: %s ms (incl. the host copy of the grid), largest cell %d px, grid %s'
          % (ppd, ' / '.join('%.3f' % t for t in ev[1:]), int(res['count'].max()), res['median'].shape[:2]), flush=True)
