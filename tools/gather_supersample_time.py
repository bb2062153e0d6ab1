"""The fused supersampled gather (amt_gather_mosaic_supersampled) beside the composition it replaces, on one MI355X.

Workload: the four full-size (4240 x 2832) constructed TAN cameras of tools/gather_mosaic_time.py (synthetic.sequence_frame 0, 20,
40, 60), each remembering maskedByElevation(10), linear interpolation, uint8 RGB images resident on the device.  For n = 2, 4, 8 the
common grid is laid out at 10 / n px per degree, so that the sub-sample grid is always the 0.1 deg one.
  composition  amt_gather_mosaic on the sub-sample points (the fine grid's img, mask, elevation, source go to device memory), then
               the block reduction in torch: counts, integer sums and rint, the mean elevation, the majority source
               (only calls that exist without amt_gather_mosaic_supersampled; its float64 sums are torch's, not the ordered ones)
  fused        one amt_gather_mosaic_supersampled call
Both are warmed up, then timed in alternating regions of `--reps` calls each, a host clock around work that ends in a device
synchronise; the figure is the median of `--regions` regions.  The two results are compared cell by cell before timing.
usage: gather_supersample_time.py [--reps 50] [--regions 7] [--members 4] [--factors 2,4,8]"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from auromat_amd._native import Context, GatherMember, ptr
from auromat_amd.coordinates.inverse import W2P_GEODETIC
from auromat_amd.mapping.mapping import MappingCollection
from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
from auromat_amd.resample import gather_mosaic_plan, gather_subsample_coordinates, supersample_min_count
from auromat_amd.synthetic import frame_image, sequence_frame

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=50)
ap.add_argument('--regions', type=int, default=7)
ap.add_argument('--members', type=int, default=4)
ap.add_argument('--factors', default='2,4,8')
ap.add_argument('--finePxPerDeg', type=float, default=10.0)
ap.add_argument('--width', type=int, default=4240)
ap.add_argument('--height', type=int, default=2832)
a = ap.parse_args()

members = []
for i in range(a.members):
    hdr, cam, t, seed = sequence_frame(20 * i, a.width, a.height)
    members.append(ArraySpacecraftMapping(hdr, 110, frame_image(a.width, a.height, seed=seed, dtype=np.uint8), cam, t, 'f%d' % i,
                                          fastCenterCalculation=True).maskedByElevation(10))
collection = MappingCollection(members, 'pass', mayOverlap=True)
ctx = Context.current()
srcs = None


def region(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


for n in [int(f) for f in a.factors.split(',')]:
    plan = gather_mosaic_plan(collection, pxPerDeg=a.finePxPerDeg / n)
    ny, nx = plan['grid'].ny, plan['grid'].nx
    fy, fx = ny * n, nx * n
    least = supersample_min_count(None, n)
    sub = gather_subsample_coordinates(plan, n)
    lat_ax, lon_ax = ctx.to_device(sub['lat']), ctx.to_device(sub['lon'])
    if srcs is None:
        srcs = [ctx.to_device(m['image'], dtype=np.uint8) for m in plan['members']]
    table = (GatherMember * len(srcs))()
    for t, m, src in zip(table, plan['members'], srcs):
        C.memmove(C.byref(t.params), C.byref(m['params']), C.sizeof(m['params']))
        t.img, t.min_elevation = ptr(src).value, float(m['min_elevation'])
    fine = dict(img=torch.empty((fy, fx, 3), dtype=torch.uint8, device=ctx.device), mask=ctx.empty((fy, fx), torch.uint8),
                elev=ctx.empty((fy, fx)), source=ctx.empty((fy, fx), torch.int32))
    out = dict(img=torch.empty((ny, nx, 3), dtype=torch.uint8, device=ctx.device), mask=ctx.empty((ny, nx), torch.uint8),
               elev=ctx.empty((ny, nx)), source=ctx.empty((ny, nx), torch.int32), count=ctx.empty((ny, nx), torch.uint8))
    member_ids = torch.arange(len(srcs), device=ctx.device).view(-1, 1, 1, 1, 1)

    def blocks(t):
        """(fy, fx, ...) -> (ny, n, nx, n, ...)"""
        return t.view(ny, n, nx, n, *t.shape[2:])

    def composition():
        ctx.call('amt_gather_mosaic', table, len(srcs), W2P_GEODETIC, ptr(lat_ax), fy, ptr(lon_ax), fx, None, None, 1, 3, 0, 1,
                 ptr(fine['img']), ptr(fine['mask']), ptr(fine['elev']), ptr(fine['source']), None, None)
        seen = blocks(fine['mask']) == 0
        count = seen.sum((1, 3))
        valid = count >= least
        total = (blocks(fine['img']).to(torch.int32) * seen[..., None]).sum((1, 3))
        img = torch.where(valid[..., None], torch.round(total.to(torch.float64) / count[..., None]), 0.0).to(torch.uint8)
        elev = torch.where(valid, torch.where(seen, blocks(fine['elev']), 0.0).sum((1, 3)) / count, float('nan'))
        won = ((blocks(fine['source'])[None] == member_ids) & seen[None]).sum((2, 4))
        source = torch.where(valid, won.argmax(0), -1).to(torch.int32)
        return img, ~valid, elev, source, count.to(torch.uint8)

    def fused():
        ctx.call('amt_gather_mosaic_supersampled', table, len(srcs), W2P_GEODETIC, ptr(lat_ax), ny, ptr(lon_ax), nx, None, None, n,
                 least, 1, 3, 0, 1, ptr(out['img']), ptr(out['mask']), ptr(out['elev']), ptr(out['source']), ptr(out['count']), None)
        return out['img'], out['mask'], out['elev'], out['source'], out['count']

    # ---- the two agree (torch sums the elevations in its own order: those are compared to a relative 1e-12; argmax may take
    # another member than the lower index on a tie of the counts: those cells are counted apart) ----
    c_img, c_mask, c_elev, c_src, c_count = composition()
    f_img, f_mask, f_elev, f_src, f_count = fused()
    torch.cuda.synchronize()
    both = ~c_mask & (f_mask == 0)
    agree = dict(cells=ny * nx, valid=int((f_mask == 0).sum()), partly_seen=int(((f_count > 0) & (f_count < n * n)).sum()),
                 count_differs=int((c_count != f_count).sum()), mask_equal=bool(torch.equal(c_mask, f_mask != 0)),
                 image_differs=int((c_img != f_img).any(-1).sum()), source_differs=int((c_src != f_src).sum()),
                 elevation_beyond_1e12=int(((c_elev[both] - f_elev[both]).abs() > 1e-12 * f_elev[both].abs()).sum()))
    print(json.dumps(dict(factor=n, grid=[ny, nx], fine_grid=[fy, fx], members=len(srcs), frame=[a.width, a.height], min_count=least,
                          agreement=agree)), flush=True)

    for fn in (composition, fused, composition, fused):
        region(fn, max(1, a.reps // 5))
    ms = dict(composition=[], fused=[])
    for _ in range(a.regions):
        ms['composition'].append(region(composition, a.reps))
        ms['fused'].append(region(fused, a.reps))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    print(json.dumps(dict(factor=n, reps=a.reps, regions=a.regions, ms_per_call=ms, median_ms=med,
                          fused_over_composition=med['fused'] / med['composition'], device=ctx.device_info()['name'])), flush=True)
    del fine, out
