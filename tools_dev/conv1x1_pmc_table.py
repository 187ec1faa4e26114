#!/usr/bin/env python
"""Per-launch PMC table of the backbone 1x1 convolution kernels from rocprofv3 counter CSVs (one counter set per run of
`tools_dev/conv_probe.py c1`, counters alone): MfmaUtil, TA busy, wait share, FETCH / WRITE size per (kernel, grid).
usage: conv1x1_pmc_table.py a_counter_collection.csv [b_counter_collection.csv ...]"""
import collections
import csv
import re
import sys


def main():
    acc = collections.defaultdict(lambda: collections.defaultdict(lambda: [0, 0.0]))
    for path in sys.argv[1:]:
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row['Kernel_Name']
                if 'conv1x1' not in name:
                    continue
                m = re.search(r'(conv1x1_\w+)<([^>]*)>', name)
                k = (f"{m.group(1)}<{m.group(2)}>" if m else name[:60], int(row['Grid_Size']) // 256)
                a = acc[k][row['Counter_Name']]
                a[0] += 1
                a[1] += float(row['Counter_Value'])
    print("# per-launch means.  kcyc = SQ_BUSY_CYCLES / 32 (XCD x SE instances); MfmaUtil = SQ_VALU_MFMA_BUSY_CYCLES / (kcyc * 1024")
    print("# SIMDs); TA = TA_BUSY_avr / kcyc; wait = SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES; FETCH / WRITE_SIZE in MB as reported (KB units)")
    print(f"{'kernel<K, RT, NTW, RES, MINB, RD> | tiled <NT, RT>':58s} {'blocks':>7s} {'n':>4s} {'kcyc':>8s} {'Mfma':>6s} {'TA':>6s} "
          f"{'wait':>6s} {'FETCH_MB':>9s} {'WRITE_MB':>9s}")
    for k, c in sorted(acc.items()):
        def mean(n):
            return c[n][1] / c[n][0] if n in c and c[n][0] else float('nan')
        dur = mean('SQ_BUSY_CYCLES') / 32
        print(f"{k[0][:58]:58s} {k[1]:7d} {max(v[0] for v in c.values()):4d} {dur / 1e3:8.1f} "
              f"{mean('SQ_VALU_MFMA_BUSY_CYCLES') / (dur * 1024):6.3f} {mean('TA_BUSY_avr') / dur:6.3f} "
              f"{mean('SQ_WAIT_INST_ANY') / mean('SQ_WAVE_CYCLES'):6.3f} {mean('FETCH_SIZE') / 1e3:9.1f} {mean('WRITE_SIZE') / 1e3:9.1f}")


if __name__ == '__main__':
    main()
