#!/usr/bin/env python
"""Hardware counters per launch of every bottleneck64 variant on the layer1 shape.

    python tools_dev/bottleneck_pmc.py [--variants 1,3,4,5] [--out FILE]

Runs tools_dev/bottleneck_probe.py once per counter set under `rocprofv3 --pmc` (counters alone, kernel trace only) with
--iters 2 --rounds 1.  Variants 2 .. 5 are one kernel, so the launches are told apart by their order, which the probe
fixes: variant 1 once, every variant once (the bit check), then 3 + iters launches per variant."""
import argparse
import collections
import csv
import glob
import os
import subprocess
import sys
import tempfile

SETS = ["FETCH_SIZE", "WRITE_SIZE", "TCC_HIT_sum TCC_MISS_sum", "SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_BUSY_CYCLES",
        "SQ_VALU_MFMA_BUSY_CYCLES TA_TA_BUSY_sum"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--variants', default='1,3,4,5')
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    variants = [int(v) for v in a.variants.split(',')]
    iters = 2
    order = [1] + variants + [v for v in variants for _ in range(3 + iters)]
    acc = collections.defaultdict(lambda: [0, 0.0])          # (cin, variant, counter) -> n, sum
    for i, cset in enumerate(SETS):
        d = tempfile.mkdtemp(prefix='bnpmc_')
        cmd = ['rocprofv3', '--pmc'] + cset.split() + ['--kernel-trace', '--output-format', 'csv',
               '--kernel-include-regex', 'bottleneck64', '-d', d, '-o', 'p', '--', sys.executable,
               os.path.join(ROOT, 'tools_dev', 'bottleneck_probe.py'), '--variants', a.variants, '--iters', str(iters),
               '--rounds', '1']
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=d)
        if res.returncode != 0:
            sys.stderr.write(res.stdout[-2000:] + res.stderr[-2000:])
            raise SystemExit(f"rocprofv3 failed on counter set {cset!r} (exit {res.returncode})")
        paths = glob.glob(os.path.join(d, '**', '*counter_collection.csv'), recursive=True)
        if not paths:
            raise SystemExit(f"no counter_collection.csv for {cset!r}")
        rows = [r for p in paths for r in csv.DictReader(open(p))]
        for cin, tag in ((256, '<256, false>'), (64, '<64, true>')):
            ids = sorted({int(r['Dispatch_Id']) for r in rows if tag in r['Kernel_Name']})
            if len(ids) != len(order):
                raise SystemExit(f"{len(ids)} launches of {tag}, expected {len(order)}")
            which = dict(zip(ids, order))
            for r in rows:
                if tag in r['Kernel_Name']:
                    v = which[int(r['Dispatch_Id'])]
                    assert ('_v2_' in r['Kernel_Name']) == (v != 1), (r['Kernel_Name'], v)
                    k = acc[(cin, v, r['Counter_Name'])]
                    k[0] += 1
                    k[1] += float(r['Counter_Value'])
    lines = ["# rocprofv3 --pmc (one counter set per run, kernel trace only) over tools_dev/bottleneck_probe.py, 6 x 232 x 400;",
             "# mean per launch.  variant 1 = first kernel, 3 / 4 / 5 = second kernel with tile order 0 / 1 / 2.",
             "# FETCH_SIZE / WRITE_SIZE in KB as rocprofv3 reports them (bytes read = 2 x FETCH_SIZE x 1024, as profiles/ computes it)"]
    names = sorted({c for (_, _, c) in acc})
    for cin in (256, 64):
        lines.append(f"cin {cin}")
        lines.append(f"  {'counter':28s}" + ''.join(f"{'variant ' + str(v):>16s}" for v in variants))
        for c in names:
            lines.append(f"  {c:28s}" + ''.join(f"{acc[(cin, v, c)][1] / max(acc[(cin, v, c)][0], 1):16.5g}" for v in variants))
    text = '\n'.join(lines) + '\n'
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)
    print(text)


if __name__ == '__main__':
    main()
