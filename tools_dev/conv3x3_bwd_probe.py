"""Dev probe: per-launch times of conv3x3_wgrad_nhwc / conv3x3_dgrad_nhwc and of ATen's convolution_backward for the 3x3 shapes of
layers 2-4 and the FPN at the base config (6 cameras, 928 x 1600)."""
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from occnet_amd import ext

SHAPES = [  # name, Cin, Cout, H, W (input), stride
    ("layer2.0.conv2", 128, 128, 232, 400, 2), ("layer2.x.conv2", 128, 128, 116, 200, 1),
    ("layer3.0.conv2", 256, 256, 116, 200, 2), ("layer3.x.conv2", 256, 256, 58, 100, 1),
    ("layer4.0.conv2", 512, 512, 58, 100, 2), ("layer4.x.conv2", 512, 512, 29, 50, 1),
    ("fpn_convs.0", 256, 256, 116, 200, 1), ("fpn_convs.1", 256, 256, 58, 100, 1), ("fpn_convs.2", 256, 256, 29, 50, 1),
    ("fpn_convs.3 (extra)", 256, 256, 29, 50, 2)]
N = 6
cl = torch.channels_last


def timed(fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return 1e3 * t[len(t) // 2], 1e3 * (t[-2] - t[1])


print("# us per call, median of 10 and (spread: 2nd largest - 2nd smallest) (HIP events around the whole call: the wgrad figure holds "
      "its reduce launch, the dgrad figure the weight flip + pack); floor = max(2 (P Cout + P_in Cin) B / 8 TB/s, "
      "2 P 9 Cin Cout flop / 2.5 PF/s)")
print(f"# {'shape':20s} {'Cin':>4s} {'Cout':>4s} {'P':>7s} s {'floor':>6s} | {'own wgrad':>14s} {'aten wgrad':>14s} | "
      f"{'own dgrad':>14s} {'aten dgrad':>14s}")
for name, Cin, Cout, H, W, s in SHAPES:
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    P = N * Ho * Wo
    x = torch.randn(N, Cin, H, W, device='cuda').to(torch.bfloat16).contiguous(memory_format=cl)
    g = torch.randn(N, Cout, Ho, Wo, device='cuda').to(torch.bfloat16).contiguous(memory_format=cl)
    w = (torch.randn(Cout, Cin, 3, 3, device='cuda') * 0.02).to(torch.bfloat16).contiguous(memory_format=cl)
    floor = 1e6 * max(2.0 * (P * Cout + N * H * W * Cin) / 8e12, 2.0 * P * 9 * Cin * Cout / 2.5e15)
    cb = lambda mask: torch.ops.aten.convolution_backward(g, x, w, None, (s, s), (1, 1), (1, 1), False, (0, 0), 1, mask)
    fmt = lambda t: f"{t[0]:8.1f} ({t[1]:4.1f})" if t is not None else f"{'-':>14s}"
    t_w = timed(lambda: ext.conv3x3_wgrad_nhwc(g, x, s, out_dtype=torch.bfloat16))
    t_aw = timed(lambda: cb((False, True, False)))
    t_d = timed(lambda: ext.conv3x3_dgrad_nhwc(g, w)) if s == 1 else None
    t_ad = timed(lambda: cb((True, False, False)))
    print(f"  {name:20s} {Cin:4d} {Cout:4d} {P:7d} {s} {floor:6.1f} | {fmt(t_w)} {fmt(t_aw)} | {fmt(t_d)} {fmt(t_ad)}", flush=True)
    del x, g, w
