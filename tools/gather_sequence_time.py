"""Gathered frames in batches (amt_gather_frames, GatherSequence) beside what exists without them, on one MI355X.

(a) kernel   16 full-size (4240 x 2832) constructed TAN cameras of a synthetic ISS pass (synthetic.sequence_frame 0 ... 15), each
             with maskedByElevation(10) as its threshold and its own grid (gather_plan) at `--pxPerDeg` (10: a grid of about eight
             tiles, where a launch is what is paid for; 100: cells of 0.01 deg, a hundred times as many, where the kernel is),
             linear taps, uint8 RGB images resident on the device, `--supersample` 1 or more.
               loop     16 back-to-back one-member amt_gather_mosaic (amt_gather_mosaic_supersampled) calls: existing code
               batched  ONE amt_gather_frames call of 16 jobs
             Both write into the same kind of outputs and are compared bit for bit before timing.  They are warmed up, then timed
             in alternating regions of `--reps` repetitions each, a host clock around work that ends in a device synchronise; the
             figure is the median of `--regions` regions.
(b) sequence `--frames` (64) frames of the same synthetic sequence with device-resident uint16 images through
             GatherSequence.process at pxPerDeg 10, and through SequencePipeline (mean binning) beside it for context, in the same
             alternating way, `--seq-reps` passes per region; ms per frame.  `--part a` or `--part b` runs one of the two.
usage: gather_sequence_time.py [--part ab] [--pxPerDeg 10] [--supersample 1] [--reps 100] [--regions 7] [--jobs 16]"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from auromat_amd._native import Context, GatherJob, GatherMember, ptr
from auromat_amd.coordinates.inverse import W2P_GEODETIC
from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
from auromat_amd.resample import gather_frames_coordinates, gather_plan, supersample_min_count
from auromat_amd.synthetic import frame_image, sequence_frame

ap = argparse.ArgumentParser()
ap.add_argument('--part', default='ab')
ap.add_argument('--reps', type=int, default=100)
ap.add_argument('--seq-reps', dest='seq_reps', type=int, default=3)
ap.add_argument('--pxPerDeg', type=int, default=10)
ap.add_argument('--supersample', type=int, default=1)
ap.add_argument('--regions', type=int, default=7)
ap.add_argument('--jobs', type=int, default=16)
ap.add_argument('--frames', type=int, default=64)
ap.add_argument('--width', type=int, default=4240)
ap.add_argument('--height', type=int, default=2832)
a = ap.parse_args()
ctx = Context.current()
device = ctx.device_info()['name']


def regions(fns, reps):
    """alternating regions of `reps` calls of each function -> dict name -> list of ms per call"""
    def region(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3
    for _ in range(2):
        for fn in fns.values():
            region(fn)
    ms = {k: [] for k in fns}
    for _ in range(a.regions):
        for k, fn in fns.items():
            ms[k].append(region(fn))
    return ms


if 'a' in a.part:
    n = a.supersample
    min_count = 1 if n == 1 else supersample_min_count(None, n)
    # one shared image: what is timed does not depend on the samples, and sixteen full-size images need not be made
    host_image = frame_image(a.width, a.height, seed=1, dtype=np.uint8)
    image = ctx.to_device(host_image, dtype=np.uint8)
    plans = []
    for i in range(a.jobs):
        hdr, cam, t, seed = sequence_frame(i, a.width, a.height)
        m = ArraySpacecraftMapping(hdr, 110, host_image, cam, t, 'f%d' % i, fastCenterCalculation=True).maskedByElevation(10)
        plans.append(gather_plan(m, pxPerDeg=a.pxPerDeg))
        assert plans[-1]['min_elevation'] == 10.0
    sizes, flat = gather_frames_coordinates(plans, n)
    coords = ctx.to_device(flat)
    members = (GatherMember * a.jobs)()
    jobs = (GatherJob * a.jobs)()
    outs = {}
    at = 0
    for k, (plan, (na, nb, points)) in enumerate(zip(plans, sizes)):
        assert not points
        ny, nx = plan['grid'].ny, plan['grid'].nx
        C.memmove(C.byref(members[k].params), C.byref(plan['params']), C.sizeof(plan['params']))
        members[k].img, members[k].min_elevation = ptr(image).value, 10.0
        for side in ('loop', 'batched'):
            outs[side, k] = dict(img=torch.empty((ny, nx, 3), dtype=torch.uint8, device=ctx.device), mask=ctx.empty((ny, nx), torch.uint8),
                                 elev=ctx.empty((ny, nx)), source=ctx.empty((ny, nx), torch.int32), count=ctx.empty((ny, nx), torch.uint8))
        j, o = jobs[k], outs['batched', k]
        C.memmove(C.byref(j.member), C.byref(members[k]), C.sizeof(members[k]))
        j.ny, j.nx = ny, nx
        j.lat, j.lon = coords.data_ptr() + 8 * at, coords.data_ptr() + 8 * (at + na)
        j.out_img, j.out_mask, j.out_elev, j.out_count = (ptr(o[key]).value for key in ('img', 'mask', 'elev', 'count'))
        at += na + nb

    def loop():
        for k in range(a.jobs):
            j, o = jobs[k], outs['loop', k]
            table = C.cast(C.byref(members[k]), C.POINTER(GatherMember))
            if n == 1:
                ctx.call('amt_gather_mosaic', table, 1, W2P_GEODETIC, j.lat, j.ny, j.lon, j.nx, None, None, 1, 3, 0, 1, ptr(o['img']),
                         ptr(o['mask']), ptr(o['elev']), ptr(o['source']), None, None)
            else:
                ctx.call('amt_gather_mosaic_supersampled', table, 1, W2P_GEODETIC, j.lat, j.ny, j.lon, j.nx, None, None, n, min_count,
                         1, 3, 0, 1, ptr(o['img']), ptr(o['mask']), ptr(o['elev']), ptr(o['source']), ptr(o['count']), None)

    def batched():
        ctx.call('amt_gather_frames', jobs, a.jobs, W2P_GEODETIC, n, min_count, 1, 3, 0, None)

    loop()
    batched()
    torch.cuda.synchronize()
    keys = ('img', 'mask', 'elev') + (('count',) if n > 1 else ())
    differs = sum(int(not torch.equal(outs['loop', k][key].view(torch.uint8), outs['batched', k][key].view(torch.uint8)))
                  for k in range(a.jobs) for key in keys)
    T = 32 // n
    cells = [p['grid'].ny * p['grid'].nx for p in plans]
    tiles = [((p['grid'].ny + T - 1) // T) * ((p['grid'].nx + T - 1) // T) for p in plans]
    print(json.dumps(dict(part='a', pxPerDeg=a.pxPerDeg, supersample=n, jobs=a.jobs, frame=[a.width, a.height],
                          grid_first=[plans[0]['grid'].ny, plans[0]['grid'].nx], cells=sum(cells), tiles=sum(tiles),
                          unmasked=int(sum((outs['batched', k]['mask'] == 0).sum() for k in range(a.jobs))),
                          outputs_that_differ=differs)), flush=True)
    assert differs == 0, 'the batched call and the loop disagree'
    ms = regions(dict(loop=loop, batched=batched), a.reps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print(json.dumps(dict(part='a', reps=a.reps, regions=a.regions, ms_per_16_frames=ms, median_ms=med,
                          batched_over_loop=med['batched'] / med['loop'], ms_per_frame={k: v / a.jobs for k, v in med.items()},
                          device=device)), flush=True)

if 'b' in a.part:
    from auromat_amd.pipeline import GatherSequence, SequencePipeline
    image = ctx.to_device(frame_image(a.width, a.height, seed=1, dtype=np.uint16), dtype=np.uint16)
    frames = [sequence_frame(k, a.width, a.height)[:3] + (image,) for k in range(a.frames)]
    gather = GatherSequence(a.width, a.height, pxPerDeg=10, min_elevation=10.0)
    mean = SequencePipeline(a.width, a.height, pxPerDeg=10, min_elevation=10.0, keep_coordinates=False, own_image_buffers=False)

    def run_gather():
        gather.process(frames, keep_on_device=True)

    def run_mean():
        mean.process(frames, keep_on_device=True)

    run_gather()
    torch.cuda.synchronize()
    plans = list(gather.plans)
    ms = regions(dict(gather_sequence=run_gather, sequence_pipeline_mean=run_mean), a.seq_reps)
    per_frame = {k: [v / a.frames for v in vs] for k, vs in ms.items()}
    print(json.dumps(dict(part='b', frames=a.frames, batch=gather.batch, gather_calls=gather.gather_calls,
                          plans={p: plans.count(p) for p in set(plans)}, passes_per_region=a.seq_reps, regions=a.regions,
                          ms_per_frame=per_frame, median_ms_per_frame={k: float(np.median(v)) for k, v in per_frame.items()},
                          device=device)), flush=True)
