#!/usr/bin/env python3
"""Launch classes of a rocprofv3 kernel trace: the launches of every kernel whose name contains one of the patterns,
grouped by (kernel, grid size), with count / average / min / max duration in ms and every launch's duration in the
order of the trace.  A kernel such as maxpool_kernel runs at several image sizes per step; the per-kernel stats file
averages over all of them, this one keeps them apart.

    python3 scripts/trace_launch_classes.py TRACE_DIR OUT.csv [pattern ...]
"""
import csv
import glob
import os
import sys
from collections import defaultdict

src, dst = sys.argv[1], sys.argv[2]
pats = sys.argv[3:] or ['maxpool_kernel', 'proj_kernel', 'fc_row_kernel', 'pk_row_kernel']
acc = defaultdict(list)
for f in glob.glob(os.path.join(src, '**', '*_kernel_trace.csv'), recursive=True):
    for r in csv.DictReader(open(f)):
        name = r.get('Kernel_Name') or r.get('kernel_name')
        if not any(p in name for p in pats):
            continue
        grid = r.get('Grid_Size') or 'x'.join(r.get(k, '?') for k in ('Grid_Size_X', 'Grid_Size_Y', 'Grid_Size_Z'))
        acc[(name, grid)].append((int(r['Start_Timestamp']), (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6))
with open(dst, 'w') as o:
    o.write('kernel,grid,launches,avg_ms,min_ms,max_ms,total_ms,each_ms\n')
    for (name, grid), td in sorted(acc.items(), key=lambda kv: (kv[0][0], -sum(d for _, d in kv[1]))):
        d = [x for _, x in sorted(td)]
        o.write('"%s",%s,%d,%.4f,%.4f,%.4f,%.3f,%s\n' % (name, grid, len(d), sum(d) / len(d), min(d), max(d), sum(d),
                                                        ' '.join('%.3f' % x for x in d)))
print('wrote', dst)
