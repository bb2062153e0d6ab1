"""resampleMesh beside resample(method='linear') on the reference's own test frame (ISS030-E-102170_dc, 4256 x 2832,
maskedByElevation(10)) at pxPerDeg=10 and 250.  Per resolution: the wall time of a call through the class API (a
fresh mapping per call, georeferencing excluded, results on the host: median of five after a warm-up) and the device time of the
frame-level call alone (events on the context's stream around regions of ten enqueued calls, median of seven regions after a
warm-up; for the mesh that is one amt_mesh_frame per call).  usage: mesh_time.py [pxPerDeg ...]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from auromat_amd.fits import readHeader
from auromat_amd.mapping.spacecraft import getMapping
from auromat_amd.resample import resample, resampleMesh, resample_frame_mesh
from auromat_amd.util.image import loadImage
G = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'resources')
arr = loadImage(os.path.join(G, 'ISS030-E-102170_dc.jpg'))
wcs = readHeader(os.path.join(G, 'ISS030-E-102170_dc.wcs'))
CALLS, REGIONS, REPEATS = 10, 7, 5


def mapping():
    mm = getMapping(arr, wcs, altitude=110, fastCenterCalculation=True).maskedByElevation(10)
    mm.frame()                      # georeferenced and masked before the clock starts
    torch.cuda.synchronize()
    return mm


def wall(fn):
    """median wall time of REPEATS calls of fn(fresh mapping), one warm-up first"""
    times = []
    for rep in range(REPEATS + 1):
        mm = mapping()
        t0 = time.perf_counter()
        r = fn(mm)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times[1:])), r


def device(fn):
    """median over REGIONS regions of CALLS enqueued calls of fn(), per call, in seconds: events on the current stream, which the
    context follows; one region as a warm-up"""
    per_call = []
    for region in range(REGIONS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        b.synchronize()
        per_call.append(a.elapsed_time(b) / CALLS / 1e3)
    return float(np.median(per_call[1:]))


for ppd in [float(v) for v in sys.argv[1:]] or [10, 250]:
    t_mesh, r = wall(lambda mm: resampleMesh(mm, pxPerDeg=ppd))
    t_lin, _ = wall(lambda mm: resample(mm, pxPerDeg=ppd, method='linear'))
    mm = mapping()
    args = (mm.frame(), mm.altitude, mm.boundingBox, (ppd, ppd), mm.containsDiscontinuity, mm.containsPole)
    d_mesh = device(lambda: resample_frame_mesh(*args, keep_on_device=True))
    print('pxPerDeg=%g, grid %s: resampleMesh %.4f s per call, resample(method=\'linear\') %.4f s per call, ratio %.1f; '
          'resample_frame_mesh on the device %.6f s per call (%.0f x below method=\'linear\')'
          % (ppd, r.img.shape[:2], t_mesh, t_lin, t_lin / t_mesh, d_mesh, t_lin / d_mesh), flush=True)
