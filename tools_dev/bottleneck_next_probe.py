"""Dev probe: ext.bottleneck64_next_nhwc and the three launches it replaces (bottleneck64_nhwc, conv1x1_nhwc 256 -> 128 with
ReLU, conv1x1_nhwc 256 -> 512 at stride 2) on the layer1 map of a base-config step (6 x 232 x 400), alternately.

    python tools_dev/bottleneck_next_probe.py [iters]

Meant to run under `rocprofv3 --pmc <one counter set> --kernel-include-regex "bottleneck64|conv1x1_resident"` (counters alone):
the launches are told apart by kernel name.  Prints whether the two routes returned the same bits."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from occnet_amd import ext  # noqa: E402

N, H, W, CM = 6, 232, 400, 128
g = torch.Generator().manual_seed(0)
x = torch.randn(N, 256, H, W, generator=g).cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
w1 = (torch.randn(64, 256, 1, 1, generator=g) / 16.0).cuda()
w2 = (torch.randn(64, 64, 3, 3, generator=g) / 24.0).cuda()
w3 = (torch.randn(256, 64, 1, 1, generator=g) / 8.0).cuda()
b1, b2, b3 = (torch.randn(n, generator=g).cuda() * 0.3 for n in (64, 64, 256))
pack = ext.bottleneck64_pack(w1, b1, w2, b2, w3, b3)
wn = ext.conv1x1_pack_weight((torch.randn(CM, 256, generator=g) / 16.0).cuda())
wd = ext.conv1x1_pack_weight((torch.randn(4 * CM, 256, generator=g) / 16.0).cuda())
bn, bd = (torch.randn(n, generator=g).cuda() * 0.3 for n in (CM, 4 * CM))
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 3
for _ in range(iters):
    mid = ext.bottleneck64_nhwc(x, pack)
    y0 = ext.conv1x1_nhwc(mid, wn, bn, relu=True)
    s0 = ext.conv1x1_nhwc(mid, wd, bd, stride=2)
    y1, s1 = ext.bottleneck64_next_nhwc(x, pack, wn, bn, wd, bd)
torch.cuda.synchronize()
print("equal", bool(torch.equal(y0, y1)), bool(torch.equal(s0, s1)))
