#!/usr/bin/env python3
"""Where a training cycle's time between kernels goes, from a rocprofv3 --kernel-trace sqlite database of a bench run.
  (a) the gap from the end of a cycle's last k_gemm_lds_adam to the start of the next cycle's k_cycle_open: the cycle boundary, which
      holds the host's staging of the fresh episodes and their H2D copy in front of the cached cycle graph;
  (b) the gap between consecutive kernels inside a cycle.
(a) - (b) is what removing the copy hop at the boundary can recover per cycle.  Only whole steady-state cycles count: those with the
most common number of launches, between two k_cycle_open.  A kernel trace does not see the copy itself -- a pinned H2D copy of this
size goes to the copy engine, not to a copy kernel -- only the gap it leaves.  Usage: cycle_gap.py trace_results.db"""
import sqlite3
import statistics
import sys
from collections import Counter


def short_kernel(name):
    n = name.strip()
    if n.startswith("void "):
        n = n[5:]
    return n.split("(")[0].split("::")[-1]


def line(label, xs):
    xs = sorted(xs)
    q = lambda p: xs[min(len(xs) - 1, int(p * len(xs)))]   # noqa: E731
    return (f"{label:58s} n={len(xs):6d} median {statistics.median(xs):7.2f}  p10 {q(0.10):7.2f}  p90 {q(0.90):7.2f}  "
            f"min {xs[0]:7.2f}  max {xs[-1]:7.2f}  mean {statistics.fmean(xs):7.2f}")


def main():
    db = sqlite3.connect(sys.argv[1])
    ks = [(s, e, short_kernel(n)) for s, e, n in db.execute("select start,end,name from kernels order by start")]
    opens = [i for i, k in enumerate(ks) if k[2] == "k_cycle_open"]
    if len(opens) < 3:
        sys.exit("fewer than three k_cycle_open launches: not a trace of the cycle path with the opening launch on")
    n_launch = Counter(b - a for a, b in zip(opens, opens[1:])).most_common(1)[0][0]
    boundary, inside, period, busy, inside_sum = [], [], [], [], []
    for a, b in zip(opens, opens[1:]):
        if b - a != n_launch or a == 0 or ks[a - 1][2] != "k_gemm_lds_adam" or ks[b - 1][2] != "k_gemm_lds_adam":
            continue
        cyc = ks[a:b]
        boundary.append((ks[a][0] - ks[a - 1][1]) / 1e3)
        gaps = [(cyc[i + 1][0] - cyc[i][1]) / 1e3 for i in range(len(cyc) - 1)]
        inside += gaps
        inside_sum.append(sum(gaps))
        busy.append(sum(e - s for s, e, _ in cyc) / 1e3)
        period.append((ks[b][0] - ks[a][0]) / 1e3)
    if not boundary:
        sys.exit("no whole steady-state cycle found")
    a_med, b_med = statistics.median(boundary), statistics.median(inside)
    print(f"# tools/cycle_gap.py: {len(boundary)} whole cycles of {n_launch} launches each (us)")
    print(line("(a) last k_gemm_lds_adam end -> next k_cycle_open start", boundary))
    print(line("(b) gap between consecutive kernels inside a cycle", inside))
    print(f"(a) - (b), medians: {a_med - b_med:.2f} us per cycle")
    print(line("sum of the gaps inside one cycle", inside_sum))
    print(line("kernel time of one cycle", busy))
    print(line("cycle period, k_cycle_open start to the next one", period))


if __name__ == "__main__":
    main()
