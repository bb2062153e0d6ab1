"""The fused gather mosaic (amt_gather_mosaic) beside the composition it replaces, on one MI355X.

Workload: four full-size (4240 x 2832) constructed TAN cameras of a synthetic ISS pass (synthetic.sequence_frame 0, 20, 40, 60:
footprints that overlap for the most part), each remembering maskedByElevation(10), on the common grid at 0.1 deg (pxPerDeg=10),
linear interpolation, uint8 RGB images resident on the device.
  baseline   per member amt_grid_to_pixel + amt_remap_coords + the masks on the common grid, then torch: argmax of the elevation
             over the unmasked members and a gather of the winner (only calls that exist without amt_gather_mosaic)
  fused      one amt_gather_mosaic call
Both are warmed up, then timed in alternating regions of `--reps` calls each, a host clock around work that ends in a device
synchronise; the figure is the median of `--regions` regions.  The two results are compared cell by cell before timing.
`--pxPerDeg 100` is the same collection on cells of 0.01 deg, where the grid is a million cells and the kernels, not their
launches, are what is timed.
usage: gather_mosaic_time.py [--reps 200] [--regions 7] [--members 4] [--pxPerDeg 10]"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from auromat_amd._native import Context, GatherMember, ptr
from auromat_amd.coordinates.inverse import W2P_GEODETIC, grid_to_pixel
from auromat_amd.mapping.mapping import MappingCollection
from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
from auromat_amd.resample import gather_mosaic_plan, grid_coordinates
from auromat_amd.synthetic import frame_image, sequence_frame

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=200)
ap.add_argument('--pxPerDeg', type=int, default=10)
ap.add_argument('--regions', type=int, default=7)
ap.add_argument('--members', type=int, default=4)
ap.add_argument('--width', type=int, default=4240)
ap.add_argument('--height', type=int, default=2832)
a = ap.parse_args()

members = []
for i in range(a.members):
    hdr, cam, t, seed = sequence_frame(20 * i, a.width, a.height)
    members.append(ArraySpacecraftMapping(hdr, 110, frame_image(a.width, a.height, seed=seed, dtype=np.uint8), cam, t, 'f%d' % i,
                                          fastCenterCalculation=True).maskedByElevation(10))
plan = gather_mosaic_plan(MappingCollection(members, 'pass', mayOverlap=True), pxPerDeg=a.pxPerDeg)
ctx = Context.current()
grid = plan['grid']
ny, nx = grid.ny, grid.nx
coords = grid_coordinates(plan)
lat_ax = ctx.to_device(np.ascontiguousarray(coords['lat_c'][:, 0]))
lon_ax = ctx.to_device(np.ascontiguousarray(coords['lon_c'][0, :]))
srcs = [ctx.to_device(m['image'], dtype=np.uint8) for m in plan['members']]
least = [float(m['min_elevation']) for m in plan['members']]
NEG = torch.tensor(float('-inf'), dtype=torch.float64, device=ctx.device)


def baseline():
    imgs, masks, elevs = [], [], []
    for m, src, e in zip(plan['members'], srcs, least):
        xy32, _, elev, flags = grid_to_pixel(ctx, m['params'], None, W2P_GEODETIC, lat_ax, lon_ax)
        dst = torch.empty((ny, nx, 3), dtype=torch.uint8, device=ctx.device)
        support = torch.empty((ny, nx), dtype=torch.uint8, device=ctx.device)
        ctx.call('amt_remap_coords', ptr(src), a.width, a.height, 1, 3, ptr(xy32), nx, ny, 0, ptr(dst), ptr(support), None)
        masks.append((flags != 0) | (support == 0) | ~(elev >= e))
        imgs.append(dst)
        elevs.append(elev)
    E, M = torch.stack(elevs), torch.stack(masks)
    win = torch.where(M, NEG, E).argmax(0)
    nobody = M.all(0)
    img = torch.gather(torch.stack(imgs), 0, win[None, :, :, None].expand(1, ny, nx, 3))[0]
    img[nobody] = 0
    elev = torch.gather(E, 0, win[None])[0]
    elev[nobody] = float('nan')
    return img, nobody, elev, torch.where(nobody, -1, win).to(torch.int32)


table = (GatherMember * len(srcs))()
for t, m, src, e in zip(table, plan['members'], srcs, least):
    C.memmove(C.byref(t.params), C.byref(m['params']), C.sizeof(m['params']))
    t.img, t.min_elevation = ptr(src).value, e
out = dict(img=torch.empty((ny, nx, 3), dtype=torch.uint8, device=ctx.device), mask=ctx.empty((ny, nx), torch.uint8),
           elev=ctx.empty((ny, nx)), source=ctx.empty((ny, nx), torch.int32))


def fused():
    ctx.call('amt_gather_mosaic', table, len(srcs), W2P_GEODETIC, ptr(lat_ax), ny, ptr(lon_ax), nx, None, None, 1, 3, 0, 1,
             ptr(out['img']), ptr(out['mask']), ptr(out['elev']), ptr(out['source']), None, None)
    return out['img'], out['mask'], out['elev'], out['source']


# ---- the two agree (argmax may take another member than the first on an exact tie: those cells are counted apart) ----
b_img, b_none, b_elev, b_src = baseline()
f_img, f_mask, f_elev, f_src = fused()
torch.cuda.synchronize()
same_src = b_src == f_src
same_elev = torch.nan_to_num(b_elev, nan=-1e9) == torch.nan_to_num(f_elev, nan=-1e9)
agree = dict(cells=ny * nx, unmasked=int((f_src >= 0).sum()), winners=[int((f_src == i).sum()) for i in range(len(srcs))],
             mask_equal=bool(torch.equal(b_none, f_mask != 0)), elevation_differs=int((~same_elev).sum()),
             source_differs=int((~same_src).sum()), image_differs_where_source_agrees=int(((b_img != f_img).any(-1) & same_src).sum()))
print(json.dumps(dict(pxPerDeg=a.pxPerDeg, grid=[ny, nx], members=len(srcs), frame=[a.width, a.height], agreement=agree)), flush=True)


def region(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / a.reps * 1e3


for fn in (baseline, fused, baseline, fused):
    region(fn)
ms = dict(baseline=[], fused=[])
for _ in range(a.regions):
    ms['baseline'].append(region(baseline))
    ms['fused'].append(region(fused))
med = {k: float(np.median(v)) for k, v in ms.items()}
print(json.dumps(dict(reps=a.reps, regions=a.regions, ms_per_call=ms, median_ms=med, fused_over_baseline=med['fused'] / med['baseline'],
                      device=ctx.device_info()['name'])), flush=True)
