"""Dev probe: per-shape timing of the backbone convolution kernels on the ResNet-50 / FPN shapes of the base
config (6 cameras, 928 x 1600 padded input)."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from occnet_amd import ext


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main(which):
    g = torch.Generator().manual_seed(0)
    N = 6
    mk = lambda *s: (torch.randn(*s, generator=g) * 0.05).cuda()
    act = lambda c, h, w: torch.randn(N, c, h, w, generator=g).cuda().to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    if 'c3' in which or 'c3v' in which:
        # c3v: every forced tile (occ_conv3x3_nhwc_bf16_variant) next to the launcher's choice, interleaved over 5 rounds
        # (median): a variant timed first or last on a shape must not win by clock drift
        def variants(s, cout):
            if 'c3v' not in which:
                return (None,)
            vs = (12, 13, 14, 16, 18, 22, 23, 24) if s == 1 else (12, 13, 22)
            return (None,) + tuple(v for v in vs if cout % (128 * (v // 10)) == 0)
        for (cin, cout, h, w, s) in [(128, 128, 232, 400, 2), (128, 128, 116, 200, 1), (256, 256, 116, 200, 2),
                                     (256, 256, 58, 100, 1), (512, 512, 58, 100, 2), (512, 512, 29, 50, 1),
                                     (256, 256, 116, 200, 1), (256, 256, 29, 50, 1),
                                     (256, 256, 29, 50, 2)]:
            x, wp, b = act(cin, h, w), ext.conv3x3_pack_weight(mk(cout, cin, 3, 3)), mk(cout)
            vs = variants(s, cout)
            rounds = 5 if len(vs) > 1 else 1
            times = {v: [] for v in vs}
            for _ in range(rounds):
                for v in vs:
                    times[v].append(timeit(lambda: ext.conv3x3_nhwc(x, wp, b, cout, relu=True, stride=s, variant=v)))
            for v in vs:
                us = sorted(times[v])[rounds // 2]
                ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
                fl = 2.0 * N * ho * wo * cout * cin * 9
                tag = 'auto' if v is None else f'v{v}'
                print(f"conv3x3 {cin:4d}->{cout:4d} {h:3d}x{w:3d} s{s} {tag:4s}: {us:7.1f} us  {fl / us * 1e-6:6.1f} TF/s")
    if 'c1' in which or 'c1v' in which or 'c1x' in which:
        # res: 0 none, 1 plain, 2 = the coarser lateral, added nearest-upsampled x2 (residual_upsample2, as the plan
        # launches FPN laterals 0 and 1).  c1v: tiled (1) against activation-resident (2) next to the launcher's
        # choice, 5 interleaved rounds, median and min-max; c1x adds the resident tiles and column splits.
        def variants(cin, cout, res):
            if 'c1v' not in which and 'c1x' not in which:
                return (None,)
            if cin > 512:
                return (None, 1)
            vs = [None, 1, 2]
            if 'c1x' in which:
                np_ = cout // (256 if cout % 256 == 0 else 128)
                tiles = (24, 22) if cin == 512 else (24,)
                vs += [100 * d + t for t in tiles for d in range(1, np_ + 1) if np_ % d == 0]
            return tuple(vs)
        for (cin, cout, h, w, s, res, relu) in [(256, 128, 232, 400, 1, 0, 1), (128, 512, 116, 200, 1, 1, 1),
                                                (512, 128, 116, 200, 1, 0, 1), (256, 512, 232, 400, 2, 0, 0),
                                                (512, 256, 116, 200, 1, 0, 1), (256, 1024, 58, 100, 1, 1, 1),
                                                (1024, 256, 58, 100, 1, 0, 1), (512, 1024, 116, 200, 2, 0, 0),
                                                (1024, 512, 58, 100, 1, 0, 1), (512, 2048, 29, 50, 1, 1, 1),
                                                (2048, 512, 29, 50, 1, 0, 1), (1024, 2048, 58, 100, 2, 0, 0),
                                                (512, 256, 116, 200, 1, 2, 0), (1024, 256, 58, 100, 1, 2, 0),
                                                (2048, 256, 29, 50, 1, 0, 0)]:
            x, wp, b = act(cin, h, w), ext.conv1x1_pack_weight(mk(cout, cin)), mk(cout)
            ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
            r = act(cout, ho, wo) if res == 1 else act(cout, ho // 2, wo // 2) if res == 2 else None
            vs = variants(cin, cout, res)
            rounds = 5 if len(vs) > 1 else 1
            times = {v: [] for v in vs}
            for _ in range(rounds):
                for v in vs:
                    times[v].append(timeit(lambda: ext.conv1x1_nhwc(x, wp, b, residual=r, relu=bool(relu), stride=s,
                                                                    residual_upsample2=res == 2, variant=v)))
            fl = 2.0 * N * ho * wo * cout * cin
            mb = N * (ho * wo * (cin + cout * (2 if res == 1 else 1.25 if res == 2 else 1))) * 2 / 1e6
            for v in vs:
                t = sorted(times[v])
                us = t[rounds // 2]
                tag = 'auto' if v is None else f'v{v}'
                print(f"conv1x1 {cin:4d}->{cout:4d} {h:3d}x{w:3d} s{s} res{res} {tag:5s}: {us:7.1f} us "
                      f"[{t[0]:6.1f} - {t[-1]:6.1f}]  {fl / us * 1e-6:6.1f} TF/s  {mb / us:5.2f} TB/s", flush=True)
    if 'f31' in which:
        # conv2 + conv3 of a layer2 / layer3 bottleneck: the pair of launches (the launchers' choices) against the fused
        # launch (ext.conv3x3_conv1x1_nhwc) at every tile it has for the shape, 5 interleaved rounds, median and min-max
        for (cmid, h, w, s) in [(128, 116, 200, 1), (128, 232, 400, 2), (256, 58, 100, 1), (256, 116, 200, 2)]:
            cout = 4 * cmid
            ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
            x, r = act(cmid, h, w), act(cout, ho, wo)
            w2, b2 = ext.conv3x3_pack_weight(mk(cmid, cmid, 3, 3)), mk(cmid)
            w3, b3 = ext.conv1x1_pack_weight(mk(cout, cmid)), mk(cout)
            pick = ext.conv3x3_conv1x1_pick(N, h, w, cmid, cout, s)
            tiles = {(128, 1): (12,), (128, 2): (12, 13), (256, 1): (22, 23, 24), (256, 2): (22,)}[(cmid, s)]
            fns = {'pair': lambda: ext.conv1x1_nhwc(ext.conv3x3_nhwc(x, w2, b2, cmid, relu=True, stride=s), w3, b3,
                                                    residual=r, relu=True)}
            for v in tiles:
                fns[f'f{v}'] = lambda v=v: ext.conv3x3_conv1x1_nhwc(x, w2, b2, cmid, w3, b3, r, stride=s, variant=v)
            times = {k: [] for k in fns}
            for _ in range(5):
                for k, fn in fns.items():
                    times[k].append(timeit(fn))
            fl = 2.0 * N * ho * wo * (9 * cmid * cmid + cmid * cout)
            for k in fns:
                t = sorted(times[k])
                print(f"conv3x3+1x1 {cmid:3d}->{cout:4d} {h:3d}x{w:3d} s{s} pick {pick:2d} {k:5s}: {t[2]:7.1f} us "
                      f"[{t[0]:6.1f} - {t[-1]:6.1f}]  {fl / t[2] * 1e-6:6.1f} TF/s", flush=True)


def vp():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(256, 256, generator=g) / 16).cuda()
    gb = torch.randn(6, 256, generator=g).cuda()
    total = 23200 + 5800 + 1450 + 375
    out = torch.empty(6 * total, 256, device='cuda')
    hws = (23200, 5800, 1450, 375)
    a_list = [torch.randn(6 * hw, 256, generator=g).cuda().to(torch.bfloat16) for hw in hws]
    gb4 = gb.unsqueeze(0).repeat(4, 1, 1).contiguous()
    starts = [0, 23200, 29000, 30450]
    us = timeit(lambda: ext.value_proj_bf16(a_list, w, gb4, out, rows_per_group=list(hws), out_group_rows=total,
                                            out_row0=starts))
    mb = 6 * total * 256 * (2 + 4) / 1e6
    print(f"value_proj_bf16 all levels M={6 * total}: {us:7.1f} us  {mb / us:5.2f} TB/s")
    x = torch.randn(6 * total, 256, generator=g).cuda()
    b = torch.randn(256, generator=g).cuda()
    us = timeit(lambda: ext.linear(x, w, b))
    print(f"linear bf16x3 f32 in M={6 * total}: {us:7.1f} us")


if __name__ == '__main__':
    if 'vp' in sys.argv[1:]:
        vp()
    main(sys.argv[1:] or ['c3', 'c1'])
