"""A/B of one training decoder layer: the combined Conv3d + BatchNorm3d + ReLU node (ext.Conv3dBNReLUFunction) against today's
chain (ext.Conv3dX3Function -> F.batch_norm on the rows view -> relu_ -> for layer 2 permute().contiguous()), forward + backward to
the gradients of x, weight, gamma, beta.

    python -m tools_dev.decoder_bn_ab [--bev 200] [--z 16] [--passes 5] [--json OUT]

Layer 1 reads the (1, bev*bev, 16*z) BEV embedding through the lifter view (Cin = 16), layer 2 a (1, bev, bev, z, 32) activation
and writes the (B, X, Y, Z, C) order.  Same process, one stream, alternating A / B after 2 warm-up passes of each; a pass is
bracketed by two events on the stream, the figure is the median of the timed passes.  torch.cuda.max_memory_allocated is taken
over one further pass of each from a reset counter (inputs are allocated before the reset).  Prints one JSON line per layer."""
import argparse
import json
import statistics

import torch
import torch.nn.functional as F

from occnet_amd import ext


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bev', type=int, default=200)
    ap.add_argument('--z', type=int, default=16)
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    dev, H, Z = 'cuda', a.bev, a.z
    g = torch.Generator().manual_seed(0)
    lines = []
    for layer, cin in ((1, 16), (2, 32)):
        shape = (1, H * H, cin * Z) if layer == 1 else (1, H, H, Z, cin)
        x = torch.randn(shape, generator=g).to(dev).requires_grad_(True)
        w = (torch.randn(32, cin, 3, 3, 3, generator=g) * (2.0 / (cin * 27)) ** 0.5).to(dev).requires_grad_(True)
        gamma = (1.0 + 0.3 * torch.randn(32, generator=g)).to(dev).requires_grad_(True)
        beta = (0.5 * torch.randn(32, generator=g)).to(dev).requires_grad_(True)
        rm, rv = torch.zeros(32, device=dev), torch.ones(32, device=dev)
        go = torch.randn(1, H, H, Z, 32, generator=g).to(dev)
        leaves = (x, w, gamma, beta)
        lay = 1 if layer == 1 else 0

        def clear():
            for t in leaves:
                t.grad = None

        def chain():
            clear()
            y = ext.conv3d_autograd(x, w, Z, H, H, in_layout=lay)
            o = torch.relu_(F.batch_norm(y.view(-1, 32), rm, rv, gamma, beta, True, 0.1, 1e-5)).view(1, H, H, Z, 32)
            if layer == 2:
                o = o.permute(0, 2, 1, 3, 4).contiguous()
            o.backward(go)
            return o.detach()

        def node():
            clear()
            o = ext.conv3d_bn_relu_autograd(x, w, gamma, beta, rm, rv, 0.1, 1e-5, Z, H, H, in_layout=lay, out_xy_major=layer == 2)
            o.backward(go)
            return o.detach()

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        def peak(fn):
            clear()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            return torch.cuda.max_memory_allocated() / 2 ** 20, base / 2 ** 20

        for _ in range(2):
            chain(), node()
        ta, tb = [], []
        for _ in range(a.passes):
            ta.append(timed(chain))
            tb.append(timed(node))
        pa, base_a = peak(chain)
        pb, base_b = peak(node)
        oa, ob = chain(), node()
        out = {"layer": layer, "rows": H * H * Z, "cin": cin, "passes": a.passes,
               "chain_ms": statistics.median(ta), "node_ms": statistics.median(tb), "chain_ms_all": ta, "node_ms_all": tb,
               "chain_peak_mb": pa, "node_peak_mb": pb, "resident_before_pass_mb": [base_a, base_b],
               "out_max_abs_diff": float((oa - ob).abs().max())}
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
        del x, w, gamma, beta, go, oa, ob
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, 'w') as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
