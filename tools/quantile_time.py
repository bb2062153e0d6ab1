"""Device time of the median and quantile entry points on the reference's full-size frame (4256 x 2832, uint8 RGB,
maskedByElevation(10)) at 10, 1 and 0.1 px/deg: amt_median_frame and amt_median_frame_async (part 'median', which also runs
against another build's tree: --tree), amt_quantile_frame with q = (0.5,), q = (0.25, 0.5, 0.75) in one call and the same
three quantiles in three calls (part 'quantile').  Prints the time between two events around every call; under
``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/quantile_time.py --labels DIR/labels.json``
tools/quantile_trace_summary.py sums the kernels of every call instead (a call starts with k_med_count).
usage: quantile_time.py [--tree DIR] [--part median|quantile|all] [--reps N] [--labels FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument('--part', default='all', choices=['median', 'quantile', 'all'])
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--labels')
args = ap.parse_args()
sys.path.insert(0, args.tree)
import numpy as np
import torch
from auromat_amd import resample as R
from auromat_amd._native import ptr
from auromat_amd.fits import readHeader
from auromat_amd.mapping.spacecraft import getMapping
from auromat_amd.util.image import loadImage

G = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'resources')
mm = getMapping(loadImage(os.path.join(G, 'ISS030-E-102170_dc.jpg')), readHeader(os.path.join(G, 'ISS030-E-102170_dc.wcs')),
                altitude=110, fastCenterCalculation=True).maskedByElevation(10)
fd = mm.frame()
ctx = fd.ctx
labels = []


def entry(name, ppd, qs=None):
    """A closure that calls one entry point on the frame with outputs allocated once."""
    grid, lat_c, lon_c, lon_wrap = R._frame_grid(fd, mm.altitude, mm.boundingBox, (ppd, ppd), mm.containsDiscontinuity, False,
                                                 None, None, None)
    xaxis, yaxis = grid.axes(ctx)
    lead = () if qs is None else (len(qs),)
    out = [ctx.empty(lead + (grid.ny, grid.nx, 4)), ctx.empty(lead + (grid.ny, grid.nx, 3), torch.uint8),
           ctx.empty((grid.ny, grid.nx), torch.uint8), ctx.empty((grid.ny, grid.nx))]
    a = [ptr(lat_c), ptr(lon_c), ptr(fd.elev), ptr(fd.img), fd.img_dtype_code, 3, ptr(fd.center_mask), fd.height, fd.width,
         float('-inf'), C.byref(xaxis), C.byref(yaxis), lon_wrap]
    if name.endswith('_async'):
        a.append(0)
    if qs is not None:
        a += [(C.c_double * len(qs))(*qs), len(qs)]
    a += [ptr(t) for t in out]
    keep = (grid, lat_c, lon_c, xaxis, yaxis, out)
    return lambda: (ctx.call(name, *a), keep)[0]


def timed(label, fns):
    """Event time of args.reps rounds of the calls `fns` (one round = every call once), the first round not reported."""
    ms = []
    for rep in range(args.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for fn in fns:
            fn()
            labels.append(label)
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    print('%-44s %s  median %.4f ms' % (label, ' '.join('%.3f' % t for t in ms[1:]), float(np.median(ms[1:]))), flush=True)


for ppd in (10, 1, 0.1):
    if args.part in ('median', 'all'):
        timed('%g px/deg amt_median_frame' % ppd, [entry('amt_median_frame', ppd)])
        timed('%g px/deg amt_median_frame_async' % ppd, [entry('amt_median_frame_async', ppd)])
    if args.part in ('quantile', 'all'):
        for name in ('amt_quantile_frame', 'amt_quantile_frame_async'):
            timed('%g px/deg %s q=(0.5,)' % (ppd, name), [entry(name, ppd, (0.5,))])
            timed('%g px/deg %s q=(0.25,0.5,0.75) one call' % (ppd, name), [entry(name, ppd, (0.25, 0.5, 0.75))])
            timed('%g px/deg %s three calls of one' % (ppd, name), [entry(name, ppd, (q,)) for q in (0.25, 0.5, 0.75)])
if args.labels:
    with open(args.labels, 'w') as fp:
        json.dump(dict(reps=args.reps, labels=labels), fp)
