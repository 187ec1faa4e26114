#!/usr/bin/env python
"""Derived PMC table of the conv3x3 kernels from rocprofv3 --pmc csv files (one counter set per file), grouped by
kernel instantiation and grid (= shape).  usage: conv3x3_pmc_table.py pmc_*_counters.csv
MfmaUtil = SQ_VALU_MFMA_BUSY_CYCLES / (SQ_BUSY_CYCLES/32 * 1024); TA = TA_BUSY_avr / (SQ_BUSY_CYCLES/32);
L1hit = 1 - TCP_TCC_READ_REQ / TCP_TOTAL_CACHE_ACCESSES; L2hit = TCC_HIT / (TCC_HIT + TCC_MISS);
LDScf = SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE; waitAny / waitInst = SQ_WAIT_ANY / SQ_WAIT_INST_ANY over SQ_WAVE_CYCLES."""
import collections
import csv
import sys


def main(paths):
    acc = collections.defaultdict(lambda: collections.defaultdict(lambda: [0, 0.0]))
    for path in paths:
        for row in csv.DictReader(open(path)):
            name = row['Kernel_Name'].split('(')[0].replace('void ', '').replace('occ::', '')
            a = acc[(name, int(row['Grid_Size']))][row['Counter_Name']]
            a[0] += 1
            a[1] += float(row['Counter_Value'])
    print(f"{'kernel':44s} {'grid':>9s} {'n':>3s} {'kcyc':>7s} {'Mfma':>6s} {'TA':>6s} {'L1hit':>6s} {'L2hit':>6s} "
          f"{'LDScf':>6s} {'waitAny':>7s} {'waitInst':>8s}")
    for k, c in sorted(acc.items()):
        def m(n):
            return c[n][1] / c[n][0] if n in c and c[n][0] else float('nan')

        def q(a, b):
            return a / b if b else float('nan')
        if not m('SQ_BUSY_CYCLES') > 0:
            continue
        dur = m('SQ_BUSY_CYCLES') / 32
        hit, miss = m('TCC_HIT_sum'), m('TCC_MISS_sum')
        print(f"{k[0][:44]:44s} {k[1]:9d} {c['SQ_BUSY_CYCLES'][0]:3d} {dur / 1e3:7.1f} "
              f"{m('SQ_VALU_MFMA_BUSY_CYCLES') / (dur * 1024):6.3f} {m('TA_BUSY_avr') / dur:6.3f} "
              f"{1 - q(m('TCP_TCC_READ_REQ_sum'), m('TCP_TOTAL_CACHE_ACCESSES_sum')):6.3f} {q(hit, hit + miss):6.3f} "
              f"{q(m('SQ_LDS_BANK_CONFLICT'), m('SQ_LDS_IDX_ACTIVE')):6.3f} {q(m('SQ_WAIT_ANY'), m('SQ_WAVE_CYCLES')):7.3f} "
              f"{q(m('SQ_WAIT_INST_ANY'), m('SQ_WAVE_CYCLES')):8.3f}")


if __name__ == '__main__':
    main(sys.argv[1:])
