"""Time of the median and quantile mosaics (resampleMosaic(statistic='median' | 'quantile'): amt_mosaic_median_frames,
amt_mosaic_quantile_frames) on the mean mosaic's two workloads (tools/mosaic_time.py): ten full-size synthetic ISS frames at
10 px/deg and twenty 512 x 512 all-sky members at 25 px/deg; both overlap rules; the median and q = (0.25, 0.5, 0.75) in one
call.  The members' frames are materialised before the timed calls.  Kept out of bench.py.

The yardstick for rule 1 (mayOverlap=True) is what the library could do before: the mean mosaic for `source`, every member's
own resample_frame_median / resample_frame_quantile on the collection's grid, read back, and a host pick by `source`.  Rule 0
(the union) had no counterpart: a union's median is not a function of the members' medians.

usage: mosaic_quantile_time.py [--case iss10|sky20|all] [--reps R] [--out DIR (default profiles/r12)]
           one JSON line per case, rule and statistic, appended to DIR/mosaic_quantile_time.txt: ms between two events around one
           call (host work inside included) and wall ms, medians over R calls; for rule 1 the same for the loop, and the ratio
       mosaic_quantile_time.py --trace LABELS [--case ...] [--calls N]
           N calls per case, rule and statistic and nothing else, for a run of its own under
           ``rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mosaic_quantile_time.py --trace DIR/labels.json``
       mosaic_quantile_time.py --summarise DIR LABELS
           per label, from the kernel trace: launches per call (all; of the count pass; of the fill pass) and the device time
           per call split by kernel, medians over the calls after the first.  A call ends with its k_med_small and whatever
           upper-tier kernels follow it."""
import argparse, csv, glob, json, os, re, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--case', default='all')
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r12'))
ap.add_argument('--trace')
ap.add_argument('--calls', type=int, default=4)
ap.add_argument('--summarise', nargs=2)
a = ap.parse_args()
Q3 = (0.25, 0.5, 0.75)
STATS = (('median', None), ('quantile', Q3))
FRONT = ('k_bin_frame', 'k_mosaic_select', 'k_med_count_members', 'k_med_source', 'k_cell_scan_sums', 'k_cell_scan_blocks',
         'k_cell_scan_apply', 'k_med_fill_members', 'k_med_small')


def summarise(trace_dir, labels_file):
    paths = glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True)
    assert len(paths) == 1, paths
    labels = json.load(open(labels_file))['labels']
    rows = []
    with open(paths[0]) as fp:
        for r in csv.DictReader(fp):
            r = {k.lower(): v for k, v in r.items()}
            m = re.search(r'(k_med_[a-z_]+|k_cell_scan_[a-z]+|k_mosaic_select|k_bin_frame)', r['kernel_name'])
            if m:
                rows.append((int(r['start_timestamp']), int(r['end_timestamp']), m.group(1),
                             int(r.get('scratch_size', r.get('private_segment_size', 0)) or 0)))
    rows.sort()
    calls, closed = [], True
    for start, end, name, _ in rows:
        if name in FRONT and closed:
            calls.append([])
            closed = False
        calls[-1].append((name, (end - start) / 1e3))
        if name == 'k_med_small':
            closed = True               # (upper-tier kernels still belong to this call; the next front kernel opens a new one)
    assert len(calls) == len(labels), (len(calls), len(labels))
    print('%d calls; scratch bytes of every dispatch: %s' % (len(calls), sorted({s for _, _, _, s in rows})))
    seen = []
    for lab in labels:
        if lab not in seen:
            seen.append(lab)
    for lab in seen:
        mine = [c for l, c in zip(labels, calls) if l == lab][1:]
        launches = sorted({len(c) for c in mine})
        count = sorted({sum(1 for n, _ in c if n == 'k_med_count_members') for c in mine})
        fill = sorted({sum(1 for n, _ in c if n == 'k_med_fill_members') for c in mine})
        total = np.median([sum(t for _, t in c) for c in mine])
        names = []
        for c in mine:
            for n, _ in c:
                if n not in names:
                    names.append(n)
        split = ', '.join('%s %.1f (x%d)' % (n, np.median([sum(t for k, t in c if k == n) for c in mine]),
                                            int(np.median([sum(1 for k, _ in c if k == n) for c in mine]))) for n in names)
        print('%-34s launches per call %s (count pass %s, fill pass %s)  kernels %9.1f us: %s' % (lab, launches, count, fill, total, split))


if a.summarise:
    summarise(*a.summarise)
    sys.exit(0)

import torch
from auromat_amd import resample as R
from auromat_amd.mapping.mapping import MappingCollection


def iss10(rule):
    from auromat_amd.mapping.spacecraft import ArraySpacecraftMapping
    from auromat_amd.synthetic import frame_image, sequence_frame
    ms = []
    for k in range(10):
        hdr, cam, t, s = sequence_frame(k)
        ms.append(ArraySpacecraftMapping(hdr, 110, frame_image(4240, 2832, seed=s), cam, t, 'iss%d' % k,
                                         fastCenterCalculation=True).maskedByElevation(10))
    return ms, dict(pxPerDeg=10)


def sky20(rule):
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


def device_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return out, s.elapsed_time(e), 1e3 * (time.perf_counter() - t0)


def loop(coll, kw, statistic, qs):
    """rule 1 without the feature: the mean mosaic for `source`, every member's own statistic on the common grid, a host pick"""
    box = coll.boundingBox
    ppd = R._px_per_deg(kw['pxPerDeg'])
    src = R.mosaic_frames(coll, **kw)['source']
    if statistic == 'median':
        res = [R.resample_frame_median(m.frame(), m.altitude, box, ppd, box.containsDiscontinuity, False) for m in coll.mappings]
        planes, imgs = np.array([r['median'] for r in res]), np.array([r['img'] for r in res])
        pick = np.clip(src, 0, None)[None, ..., None]
    else:
        res = [R.resample_frame_quantile(m.frame(), m.altitude, box, ppd, list(qs), box.containsDiscontinuity, False)
               for m in coll.mappings]
        planes, imgs = np.array([r['quantile'] for r in res]), np.array([r['img'] for r in res])
        pick = np.clip(src, 0, None)[None, None, ..., None]
    return np.take_along_axis(planes, pick, 0)[0], np.take_along_axis(imgs, pick, 0)[0], src


lines, labels = [], []
for name, make in (('iss10', iss10), ('sky20', sky20)):
    if a.case not in ('all', name):
        continue
    ms, kw = make(None)
    for m in ms:
        m.frame(), m.boundingBox
    for rule in (1, 0):
        coll = MappingCollection(ms, name, mayOverlap=bool(rule))
        for statistic, qs in STATS:
            call = lambda: R.mosaic_frames(coll, statistic=statistic, q=qs, **kw)
            label = '%s rule %d %s' % (name, rule, statistic if qs is None else 'q=(0.25,0.5,0.75)')
            if a.trace:
                for _ in range(a.calls):
                    call()
                    labels.append(label)
                torch.cuda.synchronize()
                continue
            res = call()
            dev, wall, ldev, lwall = [], [], [], []
            for rep in range(a.reps):
                _, d, w = device_ms(call)
                dev.append(d), wall.append(w)
            line = dict(case=name, members=len(ms), rule=rule, statistic=statistic, q=qs, grid=[res['grid'].ny, res['grid'].nx],
                        largest_cell=int(res['count'].max()), cells_above_16384=int((res['count'] > 16384).sum()),
                        cells_65_to_16384=int(((res['count'] > 64) & (res['count'] <= 16384)).sum()), **kw)
            line.update(call_ms=round(float(np.median(dev)), 3), call_wall_ms=round(float(np.median(wall)), 3))
            if rule == 1:
                want = loop(coll, kw, statistic, qs)
                got = res[statistic]
                sel = res['source'] >= 0
                assert np.array_equal(got[..., sel, :], want[0][..., sel, :], equal_nan=True), label
                for rep in range(a.reps):
                    _, d, w = device_ms(lambda: loop(coll, kw, statistic, qs))
                    ldev.append(d), lwall.append(w)
                line.update(loop_ms=round(float(np.median(ldev)), 3), loop_wall_ms=round(float(np.median(lwall)), 3),
                            loop_over_call=round(float(np.median(ldev) / np.median(dev)), 2),
                            loop_over_call_wall=round(float(np.median(lwall) / np.median(wall)), 2))
            else:
                line.update(loop_ms=None, note='no counterpart before: the union\'s statistic is not a function of the members\'')
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
if a.trace:
    with open(a.trace, 'w') as fp:
        json.dump(dict(calls=a.calls, labels=labels), fp)
elif a.out:
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'mosaic_quantile_time.txt'), 'a') as fp:
        fp.write('\n'.join(lines) + '\n')
