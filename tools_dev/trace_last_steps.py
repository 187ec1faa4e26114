"""Per-kernel table and dispatches per step over 8 whole steps of a rocprofv3 (rocpd sqlite) kernel trace of bench.py.

    python tools_dev/trace_last_steps.py results.db

A step starts at its stem launch; the window is the 8 steps in front of the last stem launch (the last step's tail runs
past it)."""
import sqlite3
import sys

cur = sqlite3.connect(sys.argv[1]).cursor()
stems = [r[0] for r in cur.execute("select start from kernels where name like '%stem_conv7x7_pool%' order by start")]
t_end = list(cur.execute("select max(end) from kernels"))[0][0]
# the last step's tail (transformer, heads) runs past the last stem launch: take the 8 whole steps in front of it
t0, t1 = stems[-9], stems[-1]
rows = list(cur.execute("select name, count(*), sum(end-start), avg(end-start), min(end-start), max(end-start) from kernels "
                        f"where start >= {t0} and start < {t1} group by name order by 3 desc"))
n = sum(r[1] for r in rows)
total = sum(r[2] for r in rows)
print(f"# rocprofv3 --kernel-trace --stats on bench.py --steps 10 --warmup 3: the 8 steps in front of the last stem launch "
      f"({len(stems)} stem launches in all)")
print(f"# {n} dispatches = {n / 8:.2f} per step; kernel time {total / 8e6:.4f} ms per step; wall {(t1 - t0) / 8e6:.4f} ms per step")
print(f"{'total_ms':>10} {'pct':>6} {'calls':>6} {'avg_us':>10} {'min_us':>10} {'max_us':>10}  kernel")
for name, c, tot, avg, mn, mx in rows[:60]:
    print(f"{tot / 1e6:10.3f} {100 * tot / total:6.2f} {c:6d} {avg / 1e3:10.1f} {mn / 1e3:10.1f} {mx / 1e3:10.1f}  {name[:150]}")
