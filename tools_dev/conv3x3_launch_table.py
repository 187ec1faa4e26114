#!/usr/bin/env python
"""Per-launch table of the conv3x3 kernels of one e2e inference step, from `rocpd_summary.py DB --dump conv3x3 N` output:
every run of 17 consecutive implicit-GEMM launches whose grids match the step's 17 shapes in order (the grid of each
launch is checked against the shape it must come from, whatever tile the launcher chose) is one inference step; each
launch position gets its median over those steps.
usage: conv3x3_launch_table.py trace_conv3x3_dispatch.txt"""
import re
import statistics
import sys

# launch order of one inference step (base config, 6 cameras): ResNet-50 layer2..4 conv2, FPN outputs L0..L2, FPN extra
# level; (name, Ho, Wo, Cout, stride)
STEP = ([("layer2 b0 s2", 116, 200, 128, 2)] + [(f"layer2 b{i} s1", 116, 200, 128, 1) for i in (1, 2, 3)] +
        [("layer3 b0 s2", 58, 100, 256, 2)] + [(f"layer3 b{i} s1", 58, 100, 256, 1) for i in range(1, 6)] +
        [("layer4 b0 s2", 29, 50, 512, 2)] + [(f"layer4 b{i} s1", 29, 50, 512, 1) for i in (1, 2)] +
        [("FPN out L0", 116, 200, 256, 1), ("FPN out L1", 58, 100, 256, 1), ("FPN out L2", 29, 50, 256, 1),
         ("FPN extra s2", 15, 25, 256, 2)])


def fits(row, shape, batch=6):
    """Does the launch's grid (blocks, channel blocks) and template belong to this shape under some tile?"""
    _, ho, wo, cout, s = shape
    m = re.search(r"kernel<(\d+), (\d+), \d+(?:, (\d+), \d+)?>", row[3])
    if not m or int(m.group(2)) != s:
        return False
    nt = int(m.group(1))
    rt = int(m.group(3)) if m.group(3) else (4 if s == 1 else 2)
    return row[2] == cout // (128 * nt) and row[1] == batch * ((wo + 15) // 16) * ((ho + 2 * rt - 1) // (2 * rt))


def main(path):
    rows = []
    for line in open(path):
        m = re.match(r"\s*([\d.]+) us\s+grid \((\d+), (\d+)\)\s+(.*)", line)
        if m:
            rows.append((float(m.group(1)), int(m.group(2)) // 256, int(m.group(3)), m.group(4)))
    rows = [r for r in rows if 'pack_weight' not in r[3]]
    steps = [rows[i:i + len(STEP)] for i in range(len(rows) - len(STEP) + 1)
             if all(fits(r, sh) for r, sh in zip(rows[i:i + len(STEP)], STEP))]
    if not steps:
        sys.exit("no inference step (17 launches without weight packing) in the dump")
    print(f"# {len(steps)} inference steps; median per launch position")
    print(f"{'launch':30s} {'blocks':>12s} {'us':>7s}  kernel")
    tot = 0.0
    for i, sh in enumerate(STEP):
        name = f"{sh[0]} {sh[3]}ch {sh[1]}x{sh[2]}"
        us = statistics.median(s[i][0] for s in steps)
        tot += us
        k = re.sub(r"\(.*", "", steps[-1][i][3]).replace("void occ::", "")
        print(f"{name:30s} {steps[-1][i][1]:>6d} x {steps[-1][i][2]:<3d} {us:7.1f}  {k}")
    print(f"{'total':30s} {'':>12s} {tot:7.1f}")


if __name__ == '__main__':
    main(sys.argv[1])
