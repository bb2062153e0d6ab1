"""Time of a mosaic (resampleMosaic: amt_mosaic_frames) against the per-member loop it replaces — every member's
resample_frame on the common grid, read back, and merged on the host by the highest-elevation rule — for two collections:
ten full-size synthetic ISS frames (synthetic.sequence_frame(k), k = 0..9) and twenty 512 x 512 all-sky members (the
Sodankylae calibration moved about in latitude and longitude).  The members' frames are materialised before the timed
calls.  Kept out of bench.py.

usage: mosaic_time.py [--case iss10|sky20|all] [--reps R] [--out DIR (default profiles/r9)]
One JSON line per case, also appended to DIR/mosaic_time.txt: ms of stream time between events around one mosaic call and
around one loop (host work inside them included), wall ms of both, medians over R calls.  The mosaic runs R + 2 times and the
loop R + 1 times (`calls`, `loop_calls`): under rocprofv3 --kernel-trace --stats the per-call k_mosaic_bin time compares with
the per-call sum of k_bin_frame over the same members on the same grid."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from auromat_amd import resample as R
from auromat_amd.mapping.mapping import MappingCollection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--case', default='all')
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r9'))
a = ap.parse_args()


def iss10():
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    from auromat_amd.synthetic import frame_image, sequence_frame
    ms = []
    for k in range(10):
        hdr, cam, t, s = sequence_frame(k)
        ms.append(ArraySpacecraftMapping(hdr, 110, frame_image(4240, 2832, seed=s), cam, t, 'iss%d' % k,
                                         fastCenterCalculation=True).maskedByElevation(10))
    return MappingCollection(ms, 'iss10', mayOverlap=True), dict(pxPerDeg=10)


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
    return MappingCollection(ms, 'sky20', mayOverlap=True), dict(pxPerDeg=25)


def device_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return out, s.elapsed_time(e), 1e3 * (time.perf_counter() - t0)


def loop(coll, kw):
    """the per-member loop: resample_frame on the common grid per member, then the highest-elevation merge on the host"""
    box = coll.boundingBox
    ppd = R.plateCarreeResolution(box, kw['arcsecPerPx']) if 'arcsecPerPx' in kw else R._px_per_deg(kw['pxPerDeg'])
    res = [R.resample_frame(m.frame(), m.altitude, box, ppd, box.containsDiscontinuity, False) for m in coll.mappings]
    el = np.array([np.where(r['count'] > 0, r['mean'][..., -1], -np.inf) for r in res])
    src = np.argmax(el, axis=0)
    img = np.take_along_axis(np.array([r['img'] for r in res]), src[None, ..., None], 0)[0]
    return src, img


lines = []
for name, make in (('iss10', iss10), ('sky20', sky20)):
    if a.case not in ('all', name):
        continue
    coll, kw = make()
    for m in coll.mappings:
        m.frame(), m.boundingBox
    R.mosaic_frames(coll, **kw)
    loop(coll, kw)
    mos_dev, mos_wall, loop_dev, loop_wall = [], [], [], []
    for rep in range(a.reps):
        _, d, w = device_ms(lambda: R.mosaic_frames(coll, **kw))
        mos_dev.append(d), mos_wall.append(w)
        _, d, w = device_ms(lambda: loop(coll, kw))
        loop_dev.append(d), loop_wall.append(w)
    res = R.mosaic_frames(coll, **kw)
    src = res['source']
    line = dict(case=name, members=len(coll.mappings), grid=[res['grid'].ny, res['grid'].nx], **kw,
                mosaic_ms=round(float(np.median(mos_dev)), 3), mosaic_wall_ms=round(float(np.median(mos_wall)), 3),
                loop_ms=round(float(np.median(loop_dev)), 3), loop_wall_ms=round(float(np.median(loop_wall)), 3),
                winners=int(len(np.unique(src[src >= 0]))), calls=a.reps + 2, loop_calls=a.reps + 1)
    lines.append(json.dumps(line))
    print(lines[-1], flush=True)
if a.out:
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'mosaic_time.txt'), 'a') as fp:
        fp.write('\n'.join(lines) + '\n')
