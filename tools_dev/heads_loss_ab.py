"""A/B of the training tail: the fused heads + loss node (ext.OccHeadsLossFunction) against today's module chain (X3Linear heads,
bricks.CrossEntropyLoss with the camera mask, bricks.L1Loss), forward + backward from the decoder features to all nine gradients.

    python -m tools_dev.heads_loss_ab [--rows 640000] [--classes 18] [--passes 5] [--json OUT]

Same process, one stream, alternating A / B after 2 warm-up passes of each; a pass is bracketed by two events on the stream, the
figure is the median of the timed passes.  torch.cuda.max_memory_allocated is taken over one further pass of each from a reset
counter (the inputs are allocated before the reset, so the figure is inputs + what the pass allocates).  Prints one JSON line."""
import argparse
import json
import statistics

import torch
import torch.nn as nn

from occnet_amd import ext
from occnet_amd.plugin.bricks import CrossEntropyLoss, L1Loss, X3Linear


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=640000)
    ap.add_argument('--classes', type=int, default=18)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev, n, ncls = 'cuda', a.rows, a.classes
    g = torch.Generator().manual_seed(0)
    feat = torch.randn(n, 32, generator=g).to(dev).requires_grad_(True)
    pred = nn.Sequential(X3Linear(32, 64), nn.Softplus(), X3Linear(64, ncls)).to(dev)
    flow_pred = nn.Sequential(X3Linear(32, 64), nn.ReLU(), X3Linear(64, 2)).to(dev)
    params = [t for m in (pred[0], pred[2], flow_pred[0], flow_pred[2]) for t in (m.weight, m.bias)]
    labels = torch.randint(0, ncls, (n,), generator=g).to(torch.uint8).to(dev)
    flow_gt = torch.randn(n, 2, generator=g).to(dev)
    mask = (torch.rand(n, generator=g) > 0.3).to(dev)
    lo, lf = CrossEntropyLoss(), L1Loss(loss_weight=0.25)

    def clear():
        feat.grad = None
        for p in params:
            p.grad = None

    def chain():
        clear()
        flow, occ = flow_pred(feat), pred(feat)
        loss = lo(occ, labels.long(), mask, avg_factor=mask.sum()) + lf(flow, flow_gt)
        loss.backward()
        return loss.detach()

    def fused():
        clear()
        l_occ, l_flow = ext.heads_loss(feat, *params, labels, flow_gt, mask, None, lo.ignore_index, lo.reduction)
        loss = lo.loss_weight * l_occ + lf.loss_weight * l_flow
        loss.backward()
        return loss.detach()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(2):
        chain(), fused()
    ta, tb = [], []
    for _ in range(a.passes):
        ta.append(timed(chain))
        tb.append(timed(fused))

    def peak(fn):
        clear()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(), base

    pa, base_a = peak(chain)
    pb, base_b = peak(fused)
    la, lb = float(chain()), float(fused())
    out = {"rows": n, "classes": ncls, "passes": a.passes,
           "chain_ms": statistics.median(ta), "fused_ms": statistics.median(tb), "chain_ms_all": ta, "fused_ms_all": tb,
           "chain_peak_mb": pa / 2 ** 20, "fused_peak_mb": pb / 2 ** 20, "resident_before_pass_mb": [base_a / 2 ** 20, base_b / 2 ** 20],
           "loss_chain": la, "loss_fused": lb}
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, 'w') as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
