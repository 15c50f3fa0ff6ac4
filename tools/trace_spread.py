"""Per kernel name of a rocprofv3 kernel trace: the dispatches, and the min / median / max duration in µs of those
behind the first SKIP of that name (the warm-up), in start order.

  python tools/trace_spread.py OUT SKIP

OUT is the directory given to `rocprofv3 --kernel-trace --output-format csv -d OUT`. rocprofv3's own --stats has no
median and counts the warm-up launches; this is where profiles/sign/dispatch_spread_P*.txt come from. CPU only."""
import csv
import glob
import statistics
import sys

out, skip = sys.argv[1], int(sys.argv[2])
spans = {}
for path in glob.glob(out + '/**/*kernel_trace.csv', recursive=True):
    with open(path) as fh:
        for r in csv.DictReader(fh):
            spans.setdefault(r['Kernel_Name'], []).append((int(r['Start_Timestamp']), int(r['End_Timestamp'])))
for name, se in sorted(spans.items()):
    d = [(e - s) / 1e3 for s, e in sorted(se)]
    d = d[skip:] if len(d) > skip + 4 else d  # (a kernel launched a few times only: all of them)
    print(f'{len(se):5d} kept {len(d):4d}  min {min(d):10.1f}  med {statistics.median(d):10.1f}  max {max(d):10.1f}  {name[:110]}')
