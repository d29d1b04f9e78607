"""The phases of a wave of k_search_refill, from the lab library's wave trace:
    TDTK_LIB=lab TDTK_WAVE_TRACE=5,6,7,15 python bench.py --steps 20 --warmup 5 2> trace.txt ; python tools/cert_phases.py < trace.txt
(launches 5, 6, 7 and 15 of the bench pair are the cold pass and passes 1, 2 and 10 of the timed loop behind five warm-up launches).  Reads the
`WTRACE_LAUNCH` / `WTRACE` lines (workgroup, wave, XCD / HW_ID, then the 100 MHz clock at entry, second-search pass left, end of
the certificate sweep, end of order_piece, first hand-out done, main loop left, sums done) and prints, per traced launch and per
phase, the mean and the 5 / 50 / 95 % points over the launch's waves in microseconds.  A wave that hands out nothing (its whole
slab answered by certificates) has no first hand-out: that phase is empty for it."""
import re
import sys

PH = ["sweep", "order_piece", "first hand-out", "main loop", "second search", "sums", "whole wave"]


def pct(v, p):
    v = sorted(v)
    return v[min(len(v) - 1, int(p * len(v)))]


def table(head, rows):
    print(head)
    print("  %-15s %8s %8s %8s %8s   %s" % ("phase", "mean", "5 %", "50 %", "95 %", "waves"))
    cols = {k: [] for k in PH}
    for entry, redo, sweep, order, first, loop, sums in rows:
        if first == 0:
            first = order
        for k, a, b in (("sweep", entry, sweep), ("order_piece", sweep, order), ("first hand-out", order, first), ("main loop", first, loop),
                        ("second search", loop, redo), ("sums", redo, sums), ("whole wave", entry, sums)):
            cols[k].append((b - a) / 100.0)
    for k in PH:
        v = cols[k]
        print("  %-15s %8.2f %8.2f %8.2f %8.2f   %d" % (k, sum(v) / len(v), pct(v, 0.05), pct(v, 0.5), pct(v, 0.95), len(v)))
    t0, t1 = min(r[0] for r in rows), max(r[6] for r in rows)
    print("  first entry to last wave done: %.2f us" % ((t1 - t0) / 100.0))


head, rows = None, []
for line in sys.stdin:
    if line.startswith("WTRACE_LAUNCH"):
        if head and rows:
            table(head, rows)
        head, rows = line.strip(), []
        continue
    m = re.match(r"^WTRACE (\d+) (\d+) (\d+) (\d+) (\d+) (\d+) (\d+) (\d+) (\d+) (\d+)$", line)
    if m and int(m.group(4)) and int(m.group(10)):
        g = [int(x) for x in m.groups()]
        rows.append((g[3], g[4], g[5], g[6], g[7], g[8], g[9]))
if head and rows:
    table(head, rows)
