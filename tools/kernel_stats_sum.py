"""Sum of the kernels' device time in a rocprofv3 --kernel-trace --stats run (its *kernel_stats.csv), per frame.
usage: kernel_stats_sum.py STATS_CSV FRAMES"""
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
frames = int(sys.argv[2])
total = sum(float(r['TotalDurationNs']) for r in rows)
for r in sorted(rows, key=lambda r: -float(r['TotalDurationNs']))[:12]:
    print('%10.1f us/frame  %6d calls  %s' % (float(r['TotalDurationNs']) / 1e3 / frames, int(r['Calls']), r['Name'][:90]))
print('all kernels: %.4f ms per frame over %d frames' % (total / 1e6 / frames, frames))
