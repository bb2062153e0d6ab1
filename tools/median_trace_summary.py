"""Per-call device time of amt_median_frame's kernels from a rocprofv3 --kernel-trace database of tools/median_time.py
(every call starts with k_med_count; the calls come in the tool's order).  usage: median_trace_summary.py <results.db>"""
import re
import sqlite3
import sys
from collections import OrderedDict

db = sqlite3.connect(sys.argv[1])
rows = db.execute("select name, duration, scratch_size from kernels order by start").fetchall()
calls, cur = [], None
for name, dur, scratch in rows:
    m = re.search(r'(k_med_[a-z_]+|k_cell_scan_[a-z]+)', name)
    if not m:
        continue
    k = m.group(1)
    if k == 'k_med_count':
        cur = OrderedDict()
        calls.append(cur)
    cur.setdefault(k, [0.0, 0, scratch])
    cur[k][0] += dur / 1e3
    cur[k][1] += 1
print('%d amt_median_frame calls; scratch bytes of every k_med_* dispatch: %s'
      % (len(calls), sorted({s for n, _, s in rows if 'k_med_' in n})))
for i, c in enumerate(calls):
    total = sum(v[0] for v in c.values())
    print('call %2d: %8.1f us  ' % (i, total) + '  '.join('%s %.1f%s' % (k[6:], v[0], '' if v[1] == 1 else ' (x%d)' % v[1])
                                                      for k, v in c.items()))
