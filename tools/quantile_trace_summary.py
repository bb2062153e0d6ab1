"""Per-call device time of the median / quantile kernels from the kernel trace (CSV) of a rocprofv3 run of
tools/quantile_time.py and the labels it wrote: every call starts with k_med_count, the calls come in the tool's order.  Per
label the median over its calls (the first round left out) of the summed kernel time, with the front passes (count, scan,
fill) and the rest apart; 'three calls of one' is reported per round of three.
usage: quantile_trace_summary.py <dir with *_kernel_trace.csv> <labels.json>"""
import csv
import glob
import json
import os
import re
import sys
from collections import OrderedDict

import numpy as np

paths = glob.glob(os.path.join(sys.argv[1], '**', '*kernel_trace.csv'), recursive=True)
assert len(paths) == 1, paths
meta = json.load(open(sys.argv[2]))
rows = []
with open(paths[0]) as fp:
    for r in csv.DictReader(fp):
        r = {k.lower(): v for k, v in r.items()}
        rows.append((int(r['start_timestamp']), int(r['end_timestamp']), r['kernel_name'], int(r.get('scratch_size', r.get('private_segment_size', 0)) or 0)))
rows.sort()
calls = []
for start, end, name, scratch in rows:
    m = re.search(r'(k_med_[a-z_]+|k_cell_scan_[a-z]+)', name)
    if not m:
        continue
    if m.group(1) == 'k_med_count':
        calls.append([0.0, 0.0])
    front = m.group(1) in ('k_med_count', 'k_cell_scan_sums', 'k_cell_scan_blocks', 'k_cell_scan_apply', 'k_med_fill')
    calls[-1][0 if front else 1] += (end - start) / 1e3
labels = meta['labels']
assert len(calls) == len(labels), (len(calls), len(labels))
print('%d calls; scratch bytes of every k_med_* dispatch: %s' % (len(calls), sorted({s for _, _, n, s in rows if 'k_med_' in n})))
by = OrderedDict()
for lab, c in zip(labels, calls):
    by.setdefault(lab, []).append(c)
for lab, cs in by.items():
    per_round = len(cs) // meta['reps']
    rounds = np.array(cs).reshape(meta['reps'], per_round, 2).sum(axis=1)[1:]
    tot = rounds.sum(axis=1)
    print('%-58s total %8.1f us (min %8.1f max %8.1f)  front %7.1f  selection %7.1f' %
          (lab, np.median(tot), tot.min(), tot.max(), np.median(rounds[:, 0]), np.median(rounds[:, 1])))
