"""Timeline of one steady-state step from a `rocprofv3 --kernel-trace --output-format csv` run of the pipelined bench.py:
which kernels of the other batch start while a search launch is resident, and the longest dispatch of every kernel.

    python tools/trace_timeline.py <dir or *_kernel_trace.csv> [--launch -3] > profiles/<name>.txt

The reference launch is the --launch'th (default: third from the end) dispatch of the search kernel that lasts more than
half of the longest one.  Every dispatch of the run that starts between that launch's start and the next long launch's
start is listed with its queue, its start and end relative to the launch's start, and its duration."""
import csv
import glob
import os
import re
import sys


def short(name):
    name = re.sub(r"\(.*", "", name)
    name = re.sub(r"^void ", "", name)
    m = re.search(r"(k_\w+(<[^>]*>)?)", name)
    if m:
        return m.group(1)
    m = re.search(r"rocprim::(?:detail::)?(\w+)", name)
    return ("rocprim " + m.group(1)) if m else name[:60]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = -3
    if "--launch" in sys.argv:
        which = int(sys.argv[sys.argv.index("--launch") + 1])
    path = args[0]
    if os.path.isdir(path):
        path = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))[0]
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "?"), short(r["Kernel_Name"])))
    rows.sort()
    search = [r for r in rows if r[3].startswith("k_backtrack")]
    longest = max(e - s for s, e, _, _ in search)
    big = [r for r in search if r[1] - r[0] > longest // 2]
    ref = big[which]
    nxt = [r for r in big if r[0] > ref[0]]
    t0, t_end = ref[0], ref[1]
    t_next = nxt[0][0] if nxt else t_end
    ms = lambda t: (t - t0) * 1e-6
    print("trace: %s" % os.path.basename(path))
    print("long search launches: %d, durations ms: %s" % (len(big), " ".join("%.1f" % ((e - s) * 1e-6) for s, e, _, _ in big)))
    print("start of the next long launch relative to the end of each (ms; negative: submitted launch began before the running one ended): %s" %
          " ".join("%.1f" % ((big[i + 1][0] - big[i][1]) * 1e-6) for i in range(len(big) - 1)))
    print("start-to-start of consecutive long launches (ms): %s" % " ".join("%.1f" % ((big[i + 1][0] - big[i][0]) * 1e-6) for i in range(len(big) - 1)))
    print()
    print("reference launch: queue %s, 0.0 .. %.1f ms; next long launch starts at %.1f ms" % (ref[2], ms(t_end), ms(t_next)))
    print("%-10s %10s %10s %10s  %s" % ("queue", "start_ms", "end_ms", "dur_ms", "kernel"))
    for s, e, q, n in rows:
        if t0 <= s <= t_next and (s, e, q, n) != ref:
            print("%-10s %10.2f %10.2f %10.2f  %s%s" % (q, ms(s), ms(e), (e - s) * 1e-6, n, "" if s >= t_end else "   [started beside the launch]"))
    print()
    print("longest dispatch per kernel from the first long search launch on (set-up and index build left out), ms; search launch = %.1f:" % (longest * 1e-6))
    worst = {}
    for s, e, q, n in rows:
        if s >= big[0][0]:
            worst[n] = max(worst.get(n, 0), e - s)
    for n, d in sorted(worst.items(), key=lambda kv: -kv[1]):
        print("%10.2f  %s%s" % (d * 1e-6, n, "   > a tenth of a search launch" if (d > longest / 10 and not n.startswith("k_backtrack")) else ""))


if __name__ == "__main__":
    main()
