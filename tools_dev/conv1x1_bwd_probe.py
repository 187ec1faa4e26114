"""Dev probe: per-launch times of conv1x1_wgrad_nhwc / conv1x1_dgrad_nhwc and of ATen's convolution_backward for the 1x1 shapes of
layers 2-4 and the FPN laterals at the base config (6 cameras, 928 x 1600)."""
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from occnet_amd import ext

SHAPES = [  # name, Cin, Cout, H, W (input), stride
    ("layer2.0.conv1", 256, 128, 232, 400, 1), ("layer2.0.downsample", 256, 512, 232, 400, 2),
    ("layer2.x.conv3", 128, 512, 116, 200, 1), ("layer2.x.conv1", 512, 128, 116, 200, 1),
    ("layer3.0.conv1", 512, 256, 116, 200, 1), ("layer3.0.downsample", 512, 1024, 116, 200, 2),
    ("layer3.x.conv3", 256, 1024, 58, 100, 1), ("layer3.x.conv1", 1024, 256, 58, 100, 1),
    ("layer4.0.conv1", 1024, 512, 58, 100, 1), ("layer4.0.downsample", 1024, 2048, 58, 100, 2),
    ("layer4.x.conv3", 512, 2048, 29, 50, 1), ("layer4.x.conv1", 2048, 512, 29, 50, 1),
    ("lateral0", 512, 256, 116, 200, 1), ("lateral1", 1024, 256, 58, 100, 1), ("lateral2", 2048, 256, 29, 50, 1)]
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
    return 1e3 * t[len(t) // 2]


print("# us per call, median of 10 (HIP events around the whole call: the wgrad figure holds its reduce launch, the dgrad figure the "
      "weight pack); floor = max(2 P (Cin + Cout) B / 8 TB/s, 2 P Cin Cout flop / 2.5 PF/s)")
print(f"# {'shape':22s} {'Cin':>5s} {'Cout':>5s} {'P':>7s} s {'floor':>7s} | {'own wgrad':>9s} {'aten wgrad':>10s} | {'own dgrad':>9s} {'aten dgrad':>10s}")
for name, Cin, Cout, H, W, s in SHAPES:
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    P = N * Ho * Wo
    x = torch.randn(N, Cin, H, W, device='cuda').to(torch.bfloat16).contiguous(memory_format=cl)
    g = torch.randn(N, Cout, Ho, Wo, device='cuda').to(torch.bfloat16).contiguous(memory_format=cl)
    w = (torch.randn(Cout, Cin, 1, 1, device='cuda') * 0.05).to(torch.bfloat16).contiguous(memory_format=cl)
    floor = 1e6 * max(2.0 * P * (Cin + Cout) / 8e12, 2.0 * P * Cin * Cout / 2.5e15)
    cb = lambda mask: torch.ops.aten.convolution_backward(g, x, w, None, (s, s), (0, 0), (1, 1), False, (0, 0), 1, mask)
    t_w = timed(lambda: ext.conv1x1_wgrad_nhwc(g, x, s, out_dtype=torch.bfloat16))
    t_aw = timed(lambda: cb((False, True, False)))
    t_d = timed(lambda: ext.conv1x1_dgrad_nhwc(g, w)) if s == 1 else float('nan')
    t_ad = timed(lambda: cb((True, False, False)))
    print(f"  {name:22s} {Cin:5d} {Cout:5d} {P:7d} {s} {floor:7.1f} | {t_w:9.1f} {t_aw:10.1f} | {t_d:9.1f} {t_ad:10.1f}", flush=True)
    del x, g, w
