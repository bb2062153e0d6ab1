"""Times amt_scanline_select + amt_scanline_pack per frame and amt_scanline_compose once on the ten-frame real sequence at
arcsecPerPx=100, against amt_points_in_polygon over all corners + the torch mask operations of maskedByPolygon (what the
composition resample(m).maskedByPolygon(strip) runs per frame).  Host clock around REPS calls that end in a device synchronise,
median / min / max of REGIONS such regions after a warm-up, both ways alternating in one process; the cells both ways keep are
compared first.  Usage: python tools/scanline_time.py [out.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
import auromat_amd.resample as R
from auromat_amd._native import Context, ptr
from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
from test_real_frame import real_sequence

REPS, REGIONS = 40, 9
maps = [ArraySpacecraftMapping(h, 110, img, cam, t, 'f%d' % k, fastCenterCalculation=True).maskedByElevation(10)
        for k, (h, cam, t, img) in enumerate(real_sequence())]
props = [m.properties for m in maps]
ppd = R.plateCarreeResolution(props[0].boundingBox, 100)
shifted = R.scanline_longitude_frame(props[0].centroid)
frames = [R._scanline_frame(m, k, p, ppd, shifted) for k, (m, p) in enumerate(zip(maps, props))]
rule = R.scanline_strips(props, R.scanline_first_cell_diagonal(frames[0]), 1)
ctx = frames[0]['ctx']

def sync():
    torch.cuda.synchronize()

def median_ms(fn):
    for _ in range(5):
        fn()
    sync()
    out = []
    for _ in range(REGIONS):
        t0 = time.perf_counter()
        for _ in range(REPS):
            fn()
        sync()
        out.append((time.perf_counter() - t0) / REPS * 1e3)
    return statistics.median(out), min(out), max(out)

rows, strips = [], []
for res, polygon in zip(frames, rule['polygons']):
    grid = res['grid']
    cmin, cmax = R._scanline_free_columns(res)
    own = res['lon_own_host'][cmin:cmax + 2]
    lonAxis, poly = R.scanline_prepare(res['lon_own'], polygon, bool(own.max() - own.min() > 180))
    lonAxis = lonAxis.contiguous()
    window = R.scanline_window(res['lat_axis_host'], lonAxis.cpu().numpy(), poly)
    d_poly = ctx.to_device(np.ascontiguousarray(poly))
    ny, nx = grid.ny, grid.nx
    keep = ctx.empty((window[2], window[3]), torch.uint8)
    stats = ctx.empty((5,), torch.int64)
    ctx.call('amt_scanline_select', ptr(res['lat_axis']), ptr(lonAxis), ny, nx, ptr(d_poly), len(poly), ptr(res['mask']), *window, ptr(keep), ptr(stats))
    count = int(stats[0].item())
    rec = R.scanline_pack(ctx, keep, window, res['mean'], res['img'], res['img_dtype_code'], res['nchan'], res['origin'][0], res['origin'][1], count)
    strips.append(rec)

    def new_way():
        ctx.call('amt_scanline_select', ptr(res['lat_axis']), ptr(lonAxis), ny, nx, ptr(d_poly), len(poly), ptr(res['mask']), *window, ptr(keep), ptr(stats))
        ctx.call('amt_scanline_pack', ptr(keep), *window, ptr(res['mean']), res['nchan'] + 1, ptr(res['img']), res['img_dtype_code'] or 1, res['nchan'],
                 ny, nx, res['origin'][0], res['origin'][1], count, ptr(rec['row']), ptr(rec['col']), ptr(rec['planes']), ptr(rec['img']))

    def select_only():
        ctx.call('amt_scanline_select', ptr(res['lat_axis']), ptr(lonAxis), ny, nx, ptr(d_poly), len(poly), ptr(res['mask']), *window, ptr(keep), ptr(stats))

    # the parent's way: the 2-D corner arrays of the resampled mapping, all corners through amt_points_in_polygon, torch masks
    lat2 = res['lat_axis'][:, None].expand(ny + 1, nx + 1).contiguous()
    lon2 = lonAxis[None, :].expand(ny + 1, nx + 1).contiguous()
    free = res['mask'] == 0
    corner_mask = torch.ones((ny + 1, nx + 1), dtype=torch.bool, device=ctx.device)
    for dy in (0, 1):
        for dx in (0, 1):
            corner_mask[dy:dy + ny, dx:dx + nx] &= ~free
    inside = ctx.empty((ny + 1, nx + 1), torch.uint8)
    box = {}

    def old_way():
        ctx.call('amt_points_in_polygon', ptr(lat2), ptr(lon2), lat2.numel(), ptr(d_poly), len(poly), ptr(inside))
        mask = (inside == 0) | corner_mask
        if bool(mask.all().item()):
            raise ValueError
        box['center'] = (mask[:-1, :-1] | mask[1:, :-1] | mask[:-1, 1:] | mask[1:, 1:]).to(torch.uint8).contiguous()

    def points_only():
        ctx.call('amt_points_in_polygon', ptr(lat2), ptr(lon2), lat2.numel(), ptr(d_poly), len(poly), ptr(inside))

    old_way(); new_way(); sync()
    kept_old = (box['center'] == 0) & free
    kept_new = torch.zeros((ny, nx), dtype=torch.bool, device=ctx.device)
    kept_new[window[0]:window[0] + window[2], window[1]:window[1] + window[3]] = keep != 0
    same = bool(torch.equal(kept_old, kept_new))
    a, b, c, d = median_ms(new_way), median_ms(old_way), median_ms(select_only), median_ms(points_only)
    a2, b2 = median_ms(new_way), median_ms(old_way)
    rows.append(dict(frame=res['frame'], ny=ny, nx=nx, vertices=len(poly), window=list(window), kept=count, same_cells=same,
                     select_pack_ms=a, parent_ms=b, select_only_ms=c, points_in_polygon_only_ms=d, select_pack_ms_again=a2, parent_ms_again=b2))
    print(rows[-1], flush=True)

ext = np.array([[r['row'].min().item(), r['row'].max().item(), r['col'].min().item(), r['col'].max().item()] for r in strips])
rowMin, rowMax, colMin, colMax = int(ext[:, 0].min()), int(ext[:, 1].max()), int(ext[:, 2].min()), int(ext[:, 3].max())
nch = frames[0]['nchan']
def compose():
    R.scanline_compose(ctx, strips, range(len(strips)), nch, nch + 1, frames[0]['img_dtype_code'], rowMin, colMin, rowMax - rowMin + 1, colMax - colMin + 1)
comp = median_ms(compose)
out = dict(frames=rows, compose_ms=comp, raster=[rowMax - rowMin + 1, colMax - colMin + 1], records=int(sum(s['count'] for s in strips)),
           median_select_pack_ms=statistics.median(r['select_pack_ms'][0] for r in rows),
           median_parent_ms=statistics.median(r['parent_ms'][0] for r in rows),
           median_select_only_ms=statistics.median(r['select_only_ms'][0] for r in rows),
           median_points_only_ms=statistics.median(r['points_in_polygon_only_ms'][0] for r in rows),
           reps=REPS, regions=REGIONS, device=ctx.device_info()['name'])
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as fp:
        json.dump(out, fp, indent=1)
print(json.dumps({k: v for k, v in out.items() if k != 'frames'}))
