"""Time of the area-weighted mosaic (mosaic_frames(statistic='area'): amt_area_mosaic_frames) on the mean mosaic's two workloads
(tools/mosaic_time.py): ten full-size synthetic ISS frames at 10 px/deg and twenty 512 x 512 all-sky members at 25 px/deg, both
overlap rules.  The members' frames are materialised before the timed calls.  Kept out of bench.py; there is no threshold.

Beside it, for rule 0 (the union), what the library could do before: one amt_area_frame per member on the common axes into that
member's own accumulators on the whole common grid, read back, added on the host and finalised there with
amt_area_frame_finalize's arithmetic in NumPy.  (Not through the public API either: resample_frame_area returns no accumulators
and lays out its own grid.)  Rule 1 (highest elevation wins) had no earlier form at all: the election needs every member's own
sum(W) and sum(W * E) per cell, which no call returned.  The mean mosaic of the same collection is the yardstick beside which
the number is read.

usage: mosaic_area_time.py [--case iss10|sky20|all] [--reps R] [--out DIR (default profiles/r15)]
           one JSON line per case and rule, appended to DIR/mosaic_area_time.txt: ms between two device events around one call
           (host work and read-back included), medians over R calls; the forms alternate after one warm-up call of each"""
import argparse, ctypes as C, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--case', default='all')
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r15'))
a = ap.parse_args()

import torch
from auromat_amd import resample as R
from auromat_amd._native import ptr
from auromat_amd.mapping.mapping import MappingCollection


def iss10():
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    from auromat_amd.synthetic import frame_image, sequence_frame
    ms = []
    for k in range(10):
        hdr, cam, t, s = sequence_frame(k)
        ms.append(ArraySpacecraftMapping(hdr, 110, frame_image(4240, 2832, seed=s), cam, t, 'iss%d' % k,
                                         fastCenterCalculation=True).maskedByElevation(10))
    return ms, dict(pxPerDeg=10)


def sky20():
    from datetime import datetime
    from auromat_amd.mapping.mapping import BoundingBox
    from auromat_amd.mapping.miracle import CalibrationData, MIRACLEMapping
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'miracle_sod512.npz'))
    ms = []
    for k in range(20):
        lat, lon = float(z['cal_lat']) + 1.5 * (k // 5), float(z['cal_lon']) + 3.0 * (k % 5)
        bb = BoundingBox(latSouth=lat + float(z['cal_lat_minus']), lonWest=lon + float(z['cal_lon_minus']),
                         latNorth=lat + float(z['cal_lat_plus']), lonEast=lon + float(z['cal_lon_plus']))
        cal = CalibrationData(station='S%02d' % k, validFrom=None, validTo=None, lat=lat, lon=lon, xc=float(z['cal_xc']),
                              yc=float(z['cal_yc']), k=float(z['cal_k']), rotation=float(z['cal_rotation']),
                              boundingBoxSimple=bb)
        img = np.random.RandomState(k).randint(0, 255, (512, 512)).astype(np.uint8)
        ms.append(MIRACLEMapping(cal, img, datetime(2012, 3, 4, 17, 19, 0), 110).maskedByElevation(10))
    return ms, dict(pxPerDeg=25)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def per_member(coll, kw, least=1 << 31):
    """Rule 0 before the feature: amt_area_frame per member on the common axes, the accumulators added and finalised on the host."""
    plan = R.mosaic_plan(coll, **kw)
    grid, frames = plan['grid'], plan['frames']
    ctx, nch = frames[0].ctx, frames[0].nchan
    xaxis, yaxis = grid.axes(ctx)
    total = np.zeros((nch + 2, grid.nx * grid.ny), dtype=np.int64)
    for fd in frames:
        acc = ctx.zeros((nch + 2, grid.nx * grid.ny), torch.int64)
        ctx.call('amt_area_frame', ptr(fd.lat), ptr(fd.lon), ptr(fd.lat_c), ptr(fd.elev), ptr(fd.img), fd.img_dtype_code or 1, nch,
                 ptr(fd.center_mask), fd.height, fd.width, float('-inf'), C.byref(xaxis), C.byref(yaxis), plan['lon_wrap'], ptr(acc))
        total += acc.cpu().numpy()
    lay = lambda p: np.flipud(p.reshape(grid.nx, grid.ny).T)
    w = lay(total[0])
    valid = w >= least
    with np.errstate(divide='ignore', invalid='ignore'):
        planes = [np.where(valid, lay(total[1 + k]).astype(np.float64) / w.astype(np.float64), np.nan) for k in range(nch)]
        planes.append(np.where(valid, lay(total[1 + nch]).astype(np.float64) / w.astype(np.float64) / 65536.0, np.nan))
    return dict(area=np.dstack(planes), mask=~valid, coverage=w / 4294967296.0)


lines = []
for name, make in (('iss10', iss10), ('sky20', sky20)):
    if a.case not in ('all', name):
        continue
    ms, kw = make()
    for m in ms:
        m.frame(), m.boundingBox
    torch.cuda.synchronize()
    for rule in (1, 0):
        coll = MappingCollection(ms, name, mayOverlap=bool(rule))
        forms = [('area', lambda: R.mosaic_frames(coll, statistic='area', **kw)), ('mean', lambda: R.mosaic_frames(coll, **kw))]
        if rule == 0:
            forms.append(('per_member', lambda: per_member(coll, kw)))
        first = {k: fn() for k, fn in forms}                   # the warm-up call of each form
        times = {k: [] for k, _ in forms}
        for _ in range(a.reps):
            for k, fn in forms:
                times[k].append(timed(fn)[1])
        res = first['area']
        line = dict(case=name, members=len(ms), rule=rule, grid=[res['grid'].ny, res['grid'].nx], reps=a.reps,
                    cells_filled_area=int((~res['mask']).sum()), cells_filled_mean=int((~first['mean']['mask']).sum()),
                    largest_coverage=round(float(res['coverage'].max()), 3), **kw)
        for k, _ in forms:
            line['%s_ms' % k] = round(float(np.median(times[k])), 3)
            line['%s_ms_all' % k] = [round(v, 3) for v in times[k]]
        if rule == 0:
            old = first['per_member']
            # (the earlier form has no windows: a cell may differ where a member's pixels reach past its own bounding box)
            line['cells_differing_from_per_member'] = int(((old['mask'] != res['mask']) | (old['coverage'] != res['coverage']) |
                                                           ~np.all((old['area'] == res['area']) | np.isnan(old['area']) &
                                                                   np.isnan(res['area']), axis=2)).sum())
            line['per_member_over_area'] = round(line['per_member_ms'] / line['area_ms'], 2)
        else:
            line['note'] = 'rule 1 had no earlier form: no call returned the members\' own sums'
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
if a.out:
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'mosaic_area_time.txt'), 'a') as fp:
        fp.write('\n'.join(lines) + '\n')
