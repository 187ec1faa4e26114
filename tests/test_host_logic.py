"""not-gpu: host-side logic of the path — query processing order, visibility packing, sample sharding
and the world_size-2 gloo run of the data-parallel plumbing."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from occnet_amd import synthetic
from occnet_amd.dist import shard_indices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('hw', [(200, 200), (50, 50), (400, 400), (12, 12), (7, 13)])
def test_bev_tile_order_is_a_permutation(hw):
    o = synthetic.bev_tile_order(*hw)
    assert o.dtype == np.int32 and np.array_equal(np.sort(o), np.arange(hw[0] * hw[1]))


@pytest.mark.parametrize("hw,patch", [((200, 200), (2, 4)), ((38, 38), (2, 4)), ((50, 50), (4, 2)), ((16, 24), (1, 8))])
def test_bev_tile_order_with_query_patches_is_a_permutation(hw, patch):
    """The head-major SCA gather's order (plain tile walk, a wave's 8 consecutive entries = one ph x pw BEV patch inside full 8 x 8
    tiles; ragged edge tiles keep row order): still a permutation, and full tiles really come out in patches."""
    import numpy as np
    o = synthetic.bev_tile_order(*hw, n_xcd=1, patch=patch)
    assert sorted(o.tolist()) == list(range(hw[0] * hw[1]))
    ph, pw = patch
    first = o[:8]                                             # tile (0, 0) is a full tile for all cases here
    ys, xs = first // hw[1], first % hw[1]
    assert ys.max() - ys.min() == ph - 1 and xs.max() - xs.min() == pw - 1
    assert len(np.unique(first)) == 8


def test_bev_tile_order_xcd_contiguity():
    """Hardware block b runs on XCD b % 8: the queries an XCD processes form one contiguous 1/8 of the
    tile sequence, i.e. a compact band of the BEV plane."""
    o = synthetic.bev_tile_order(200, 200).reshape(-1, 4)            # 4 waves (queries) per block
    rows = o // 200
    for x in range(8):
        r = rows[x::8]
        assert r.max() - r.min() < 200 // 8 + 8                      # one band of ~25 rows (+ tile)


def test_pack_vis_bits():
    from occnet_amd.plugin.spatial_cross_attention import pack_vis_bits
    g = torch.Generator().manual_seed(0)
    m = torch.rand(6, 2, 50, 8, generator=g) > 0.9
    bits = pack_vis_bits(m)
    assert bits.shape == (2, 50) and bits.dtype == torch.int32
    for c in range(6):
        assert torch.equal(((bits >> c) & 1).bool(), m[c].any(-1))


def test_rig_visibility_is_realistic():
    import oracle.model as om
    g = synthetic.BASE
    ref3d = om.get_reference_points(200, 200, 6.4, 8, '3d', 1)
    _, mask = om.point_sampling(ref3d, list(g['pc_range']), synthetic.make_img_metas(g))
    rows = [int(mask[c, 0].any(-1).sum()) for c in range(6)]
    assert 40000 < sum(rows) < 50000 and max(rows) < 11000           # R ~ 44.5 k


def test_shard_indices():
    assert shard_indices(10, 0, 4) == [0, 4, 8] and shard_indices(10, 3, 4) == [3, 7, 1]
    assert shard_indices(10, 1, 4, drop_last=True) == [1, 5]
    allidx = sorted(i for r in range(8) for i in shard_indices(64, r, 8))
    assert allidx == list(range(64))
    assert shard_indices(0, 0, 2) == []
    with pytest.raises(ValueError):
        shard_indices(4, 2, 2)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from occnet_amd import dist as od
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        assert od.env_world() == (rank, rank, world)
        mine = od.shard_indices(7, rank, world)
        # every rank "processes" its samples; no data-path collective — only timing is reduced
        elapsed = 1.0 + rank
        od.barrier()
        tmax = od.max_over_ranks(elapsed)
        thr = od.throughput(len(mine), elapsed)
        # DDP-style gradient all-reduce(mean): the one collective training needs
        g = torch.full((5,), float(rank + 1))
        dist.all_reduce(g)
        g /= world
        q.put((rank, mine, tmax, thr, g.tolist()))
    finally:
        dist.destroy_process_group()


def test_gloo_world2_plumbing():
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][1] == [0, 2, 4, 6] and res[1][1] == [1, 3, 5, 0]
    for r in res:
        assert r[2] == 2.0                      # max over ranks
        assert abs(r[3] - 2 * 4 / 2.0) < 1e-9   # all ranks' units / max time
        assert r[4] == [1.5] * 5


class _ToyDetector(torch.nn.Module):
    """Stands in for BEVFormerOcc in the DDP wiring test: same forward(return_loss=True, **kw) call shape,
    same `backbone_autocast_dtype` knob, a 'backbone' and a 'head' parameter group."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.img_backbone = torch.nn.Linear(6, 5)
        self.pts_bbox_head = torch.nn.Linear(5, 3)
        self.backbone_autocast_dtype = None
        self.saw_autocast = []

    def forward(self, return_loss=True, img=None, img_metas=None, voxel_semantics=None, voxel_flow=None,
                mask_camera=None):
        ac = self.backbone_autocast_dtype
        self.saw_autocast.append(ac)
        with torch.autocast('cpu', dtype=ac or torch.bfloat16, enabled=ac is not None):
            f = self.img_backbone(img)
        out = self.pts_bbox_head(f.float())
        return dict(loss_occ=(out - voxel_flow).pow(2).mean(), loss_flow=out.abs().mean() * 0.25)


def _ddp_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from occnet_amd.train import make_optimizer, train_step, wrap_ddp
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        res = {}
        for autocast in (False, True):
            net = _ToyDetector()
            ddp = wrap_ddp(net, torch.device('cpu'))
            assert ddp is not net                           # really wrapped
            opt = make_optimizer(ddp, lr=0.0)               # lr 0: parameters stay put, grads are what we check
            g = torch.Generator().manual_seed(100 + rank)   # every rank its own sample
            img, tgt = torch.randn(4, 6, generator=g), torch.randn(4, 3, generator=g)
            train_step(ddp, opt, img, None, None, tgt, None, max_norm=1e9, autocast_backbone=autocast)
            grads = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
            # the same sample through the bare module: the rank-local gradient DDP must have averaged
            ref = _ToyDetector()
            ref.backbone_autocast_dtype = torch.bfloat16 if autocast else None
            sum(ref(img=img, voxel_flow=tgt).values()).backward()
            local = torch.cat([p.grad.reshape(-1) for p in ref.parameters()])
            res[autocast] = (grads.tolist(), local.tolist(), [str(a) for a in net.saw_autocast])
        q.put((rank, res))
    finally:
        dist.destroy_process_group()


def test_train_step_goes_through_ddp_forward_world2():
    """train_step must drive the DDP wrapper's forward for BOTH autocast settings, or the
    reducer is never armed and every rank keeps its local gradient.  Two gloo ranks, different samples:
    after one step the gradients are identical on both ranks and equal the mean of the rank-local ones."""
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_ddp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for autocast in (False, True):
        g0, l0, seen0 = res[0][autocast]
        g1, l1, _ = res[1][autocast]
        assert seen0 == ['torch.bfloat16' if autocast else 'None']
        assert g0 == g1                                                 # all-reduced: bitwise the same
        mean = [(a + b) / 2 for a, b in zip(l0, l1)]
        assert max(abs(a - b) for a, b in zip(g0, mean)) < (2e-3 if autocast else 1e-6)
        assert max(abs(a - b) for a, b in zip(l0, l1)) > 1e-3           # the local gradients did differ


def test_cache_epoch_invalidation():
    """derived-weight caches also key on an epoch that load_state_dict and invalidate_caches()
    bump (writes through param.data do not touch tensor._version).  ADVICE r2 (medium): a train()/eval() flip does
    NOT bump it (obtain_history_bev flips twice per training step); in-place training updates are seen through
    tensor._version, and the folded inference backbone re-checks its sources' signature after training mode."""
    import occnet_amd
    from occnet_amd.plugin.spatial_cross_attention import _CatLinearCache
    from occnet_amd.plugin.bricks import BaseModule

    class M(BaseModule):
        def __init__(self):
            super().__init__()
            self.a, self.b = torch.nn.Linear(3, 2), torch.nn.Linear(3, 4)

    m = M()
    cache = _CatLinearCache()
    w0, _ = cache.get((m.a, m.b))
    assert cache.get((m.a, m.b))[0] is w0                       # hit
    m.a.weight.data.mul_(2.0)                                   # invisible to _version ...
    assert cache.get((m.a, m.b))[0] is w0                       # ... so still (stale) a hit,
    occnet_amd.invalidate_caches()                              # until the owner says so
    w1, _ = cache.get((m.a, m.b))
    assert w1 is not w0 and torch.equal(w1[:2], m.a.weight)
    e = occnet_amd.cache_epoch()
    m.load_state_dict(m.state_dict())                           # post hook
    assert occnet_amd.cache_epoch() > e
    e = occnet_amd.cache_epoch()
    m.train(False)
    m.train(True)
    assert occnet_amd.cache_epoch() == e                        # mode flips do not invalidate anything ...
    w2, _ = cache.get((m.a, m.b))
    with torch.no_grad():
        m.a.weight.add_(1.0)                                    # ... an in-place (optimizer-style) update does
    w3, _ = cache.get((m.a, m.b))
    assert w3 is not w2 and torch.equal(w3[:2], m.a.weight)


def test_folded_plan_signature_rechecked_after_training_mode():
    """The folded inference backbone holds COPIES of the backbone weights: after the detector has been in training
    mode its (data_ptr, _version) signature is compared once; unchanged parameters keep the plan (the history-BEV
    eval()/train() flip of every training step), changed ones rebuild it."""
    from occnet_amd.plugin.bevformer_occ import BEVFormerOcc
    det = BEVFormerOcc.__new__(BEVFormerOcc)
    torch.nn.Module.__init__(det)
    det.img_backbone = torch.nn.Conv2d(3, 4, 3)
    built = []

    class Plan:
        pass

    def enable(**kw):
        import occnet_amd
        plan = Plan()
        plan.built_epoch, plan.signature = occnet_amd.cache_epoch(), det._backbone_signature()
        built.append(plan)
        object.__setattr__(det, '_inference_backbone', plan)
    det.enable_fused_backbone = enable
    object.__setattr__(det, '_inference_backbone_args', {})
    enable()
    det.eval()
    assert det._current_plan() is built[0]
    det.train()
    det.eval()                                                  # mode flip, nothing trained
    assert det._current_plan() is built[0] and len(built) == 1
    det.train()
    with torch.no_grad():
        det.img_backbone.weight.mul_(0.5)                       # an optimizer step
    det.eval()
    assert det._current_plan() is built[1] and len(built) == 2
    assert det._current_plan() is built[1]                      # clean again: no signature walk, no rebuild


def test_grid_mask_follows_reference_rng_and_geometry():
    """GridMask(True, True, rotate=1, ratio=0.5, mode=1, prob=0.7) as BEVFormerOcc builds it (reference
    bevformer_occ.py:52-53): eval -> identity; train -> kept pixels form the complement of a square lattice of
    (d - l)-wide holes, drawn from numpy's global RNG in the reference's order."""
    import numpy as np
    from occnet_amd.plugin.grid_mask import GridMask
    gm = GridMask(True, True, rotate=1, offset=False, ratio=0.5, mode=1, prob=0.7)
    x = torch.ones(2, 3, 40, 64)
    gm.eval()
    assert gm(x) is x
    gm.train()
    np.random.seed(3)
    outs = [gm(x) for _ in range(40)]
    n_kept = sum(o is x for o in outs)
    assert 3 <= n_kept <= 25                                                    # prob 0.7 of being applied
    np.random.seed(11)
    while True:
        y = gm(x)
        if y is not x:
            break
    np.random.seed(11)
    while np.random.rand() > gm.prob:
        pass
    h, w = 40, 64
    d = np.random.randint(2, h)
    l = min(max(int(d * 0.5 + 0.5), 1), d - 1)
    st_h, st_w = np.random.randint(d), np.random.randint(d)
    rows = np.zeros(60, bool)
    cols = np.zeros(96, bool)
    for i in range(60 // d):
        rows[d * i + st_h:min(d * i + st_h + l, 60)] = True
    for i in range(96 // d):
        cols[d * i + st_w:min(d * i + st_w + l, 96)] = True
    keep = (rows[:, None] | cols[None, :])[10:50, 16:80]                       # mode 1: 1 - (1-rows)(1-cols)
    assert torch.equal(y[1, 2], torch.from_numpy(keep.astype(np.float32)))


def test_folded_backbone_plan_on_cpu_matches_modules():
    """The BatchNorm fold and the plan's control flow (stem, bottlenecks with/without projection, FPN top-down,
    extra levels) on stock torch ops: fp32 on the CPU the folded plan equals the modules to rounding."""
    from occnet_amd.plugin.backbone import FPN, FusedInferenceBackbone, ResNet
    torch.manual_seed(0)
    bb = ResNet(depth=50, num_stages=4, out_indices=(1, 2, 3), frozen_stages=1, norm_eval=True).eval()
    bb.init_weights()
    g = torch.Generator().manual_seed(1)
    for m in bb.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 0.5 + 0.75)
            m.weight.data.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    nk = FPN(in_channels=[512, 1024, 2048], out_channels=256, start_level=0, add_extra_convs='on_output',
             num_outs=4, relu_before_extra_convs=True).eval()
    x = torch.randn(1, 3, 64, 96, generator=g)
    with torch.no_grad():
        ref = nk(bb(x))
        plan = FusedInferenceBackbone(bb, nk, dtype=torch.float32, hip_tail=True)   # fp32: hip_tail switches off
        assert not plan.hip_tail and not plan._bneck and not plan._stem_fused
        out = plan(x)
    assert len(out) == len(ref) == 4
    for a, b in zip(ref, out):
        assert a.shape == b.shape
        rel = float((a - b).abs().max() / a.abs().max())
        assert rel < 2e-5, rel


def test_sca_pixel_pair_layout_round_trip_and_addresses():
    """ext.sca_pair_layout (host restatement of the order the value projection's fp16 epilogue writes and the fused gather
    reads, csrc/sca_fused.hip): element (b, pix, head, d) lives at [b][pix >> 1][head][pix & 1][d]; odd pixel counts are
    padded by one zero row; sca_unpair_layout inverts it."""
    from occnet_amd import ext
    g = torch.Generator().manual_seed(0)
    for S in (6, 7, 31):
        BN, M, D = 2, 8, 32
        v = torch.randn(BN, S, M, D, generator=g).half()
        p = ext.sca_pair_layout(v)
        Sp = S + (S & 1)
        assert p.shape == (BN, Sp, M, D) and p.is_contiguous()
        flat = p.reshape(BN, -1)
        for b, pix, m, d in ((0, 0, 0, 0), (1, S - 1, 7, 31), (0, 3, 2, 5), (1, 4, 5, 17)):
            addr = ((pix >> 1) * M + m) * 2 * D + (pix & 1) * D + d
            assert flat[b, addr] == v[b, pix, m, d]
        if S & 1:       # the pad row is zero
            assert float(ext.sca_unpair_layout(p)[:, S:].abs().max()) == 0.0
        assert torch.equal(ext.sca_unpair_layout(p, S), v)
        # the byte-offset transform the gather applies to a row-order offset pix * 512 (fp16, 8 heads x 32 channels)
        for pix in range(S):
            o = pix * 512
            assert ((o & ~1023) | ((o >> 3) & 64)) == (pix >> 1) * 1024 + (pix & 1) * 64


def test_lazy_features_only_for_backbone_format_inputs():
    from occnet_amd.plugin.transformer_occ import LazyFeatures
    f32 = [torch.zeros(1, 6, 256, 4, 5)]
    bf16 = [torch.zeros(1, 6, 256, 4, 5, dtype=torch.bfloat16)]
    with torch.no_grad():
        assert not LazyFeatures.eligible(f32) and not LazyFeatures.eligible(bf16)     # host tensors: never
    assert not LazyFeatures.eligible([])


def test_bench_self_launches_n_ranks():
    """`python bench.py --gpus 2` with no torchrun environment must start 2 ranks itself (the reference's
    tools/dist_train.sh:9-11 role) and rank 0 must print ONE JSON line with n_gpus = 2.
    --launcher-selftest exercises exactly the launch / rank-env / barrier / MAX-reduce code of the real run
    (gloo, no model), so it runs without a GPU."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items()
           if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR')}
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '4',
                          '--warmup', '1', '--launcher-selftest'], env=env, capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out['n_gpus'] == 2 and out['steps'] == 4 and out['config']['parallelism'] == 'dp2'
    # whole-job value = all ranks' steps / max-over-ranks time; rank 1 sleeps 2 ms per step
    assert out['ms_per_step'] >= 2.0
    assert abs(out['value'] - 2 * 4 / (out['ms_per_step'] * 4e-3)) / out['value'] < 1e-6


def test_bench_launcher_at_eight_ranks_binds_disjoint_core_slices():
    """The shape the driver's 8-GPU run takes: `bench.py --gpus 8` self-launches 8 ranks, every rank
    pins itself to its own slice of the host cores (occnet_amd/dist.py::bind_rank_threads), rank 0 prints ONE JSON
    line with n_gpus = 8.  gloo, no model, no GPU."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items()
           if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR', 'LOCAL_WORLD_SIZE')}
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '8', '--steps', '3',
                          '--warmup', '0', '--launcher-selftest'], env=env, capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out['n_gpus'] == 8 and out['config']['parallelism'] == 'dp8'
    assert out['ms_per_step'] >= 8.0                       # rank 7 sleeps 8 ms per step: MAX over ranks
    slices = out['host_cores_per_rank']
    assert len(slices) == 8
    if hasattr(os, 'sched_getaffinity') and len(os.sched_getaffinity(0)) >= 8:
        assert all(s for s in slices)
        flat = [c for s in slices for c in s]
        assert len(flat) == len(set(flat))                 # disjoint
        assert all(s == list(range(s[0], s[0] + len(s))) or sorted(s) == s for s in slices)


def test_ddp_comm_stats_reports_allreduce_time():
    """occnet_amd.dist.ddp_comm_stats on a 2-rank gloo DDP toy model: the fields bench.py --mode train --gpus N puts
    under "ddp" (gradient all-reduce time per step, how much of it ran under the backward pass) exist and are sane."""
    import json
    import subprocess
    import textwrap
    code = textwrap.dedent("""
        import json, os, sys, torch, torch.distributed as dist
        sys.path.insert(0, %r)
        from occnet_amd.dist import ddp_comm_stats
        dist.init_process_group('gloo')
        torch.manual_seed(0)
        m = torch.nn.Sequential(torch.nn.Linear(256, 512), torch.nn.ReLU(), torch.nn.Linear(512, 64))
        ddp = torch.nn.parallel.DistributedDataParallel(m)
        ddp._set_ddp_runtime_logging_sample_rate(1)
        opt = torch.optim.SGD(ddp.parameters(), lr=0.1)
        for i in range(12):
            opt.zero_grad()
            ddp(torch.randn(32, 256)).square().mean().backward()
            opt.step()
        st = ddp_comm_stats(ddp)
        if dist.get_rank() == 0:
            print('STATS ' + json.dumps(st))
        dist.destroy_process_group()
    """ % ROOT)
    env = dict(os.environ, MASTER_ADDR='127.0.0.1')
    res = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                          '--master-addr', '127.0.0.1', '--master-port', '29541', '-c', code] if False else
                         [sys.executable, '-c', "import subprocess,sys,os,tempfile\n"
                          "f=tempfile.NamedTemporaryFile('w',suffix='.py',delete=False);f.write(%r);f.close()\n"
                          "sys.exit(subprocess.call([sys.executable,'-m','torch.distributed.run','--nnodes=1',"
                          "'--nproc-per-node','2','--master-addr','127.0.0.1','--master-port','29541',f.name]))" % code],
                         env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [l for l in res.stdout.splitlines() if l.startswith('STATS ')][-1]
    st = json.loads(line[6:])
    assert st is not None and set(st) >= {'allreduce_ms', 'backward_compute_ms', 'allreduce_overlapped_ms'}
    assert st['backend'] == 'gloo'
    assert st['allreduce_ms'] is None or st['allreduce_ms'] >= 0.0


def test_conv_bn_folded_matches_eval_batchnorm_with_gradients():
    """Training with norm_eval=True: conv -> eval BN computed as one convolution with folded weights must give the
    same output and the same gradients for the input, the convolution weight and the BN affine parameters."""
    import torch.nn as nn
    from occnet_amd.plugin.backbone import conv_bn_folded
    torch.manual_seed(3)
    conv = nn.Conv2d(8, 16, 3, stride=2, padding=1, bias=False).double()
    bn = nn.BatchNorm2d(16).double()
    with torch.no_grad():
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.normal_()
        bn.bias.normal_()
    bn.eval()
    x = torch.randn(2, 8, 9, 11, dtype=torch.double, requires_grad=True)
    go = torch.randn(2, 16, 5, 6, dtype=torch.double)
    y_ref = bn(conv(x))
    g_ref = torch.autograd.grad(y_ref, [x, conv.weight, bn.weight, bn.bias], go)
    y = conv_bn_folded(x, conv, bn)
    g = torch.autograd.grad(y, [x, conv.weight, bn.weight, bn.bias], go)
    assert float((y - y_ref).abs().max()) < 1e-12
    for a, b in zip(g, g_ref):
        assert float((a - b).abs().max()) < 1e-10 * max(1.0, float(b.abs().max()))


def test_sca_rebatch_plan_index_maps_are_inverse_relations():
    """SpatialCrossAttention._rebatch_plan (training path): the padded per-camera row list, its inverse map and the
    rebatched reference points, against a brute-force construction (host tensors: pure index arithmetic)."""
    from occnet_amd.plugin.spatial_cross_attention import SpatialCrossAttention
    torch.manual_seed(4)
    nc, bs, Q, Z = 5, 2, 60, 4
    sca = SpatialCrossAttention(embed_dims=32, num_cams=nc,
                                deformable_attention=dict(type='MSDeformableAttention3D', embed_dims=32, num_heads=4,
                                                          num_levels=1, num_points=4))
    bev_mask = torch.rand(nc, bs, Q, Z) > 0.8
    ref = torch.randn(nc, bs, Q, Z, 2)
    plan = sca._rebatch_plan(bev_mask, ref)
    lists = [m[0].sum(-1).nonzero().squeeze(-1) for m in bev_mask]
    max_len = max(len(l) for l in lists)
    assert plan['max_len'] == max_len
    r2q = plan['row_to_query'].view(nc, max_len)
    for c, l in enumerate(lists):
        assert r2q[c, :len(l)].tolist() == l.tolist() and (r2q[c, len(l):] == -1).all()
        assert torch.equal(plan['ref'][:, c, :len(l)], ref[c][:, l])
        assert float(plan['ref'][:, c, len(l):].abs().max() if len(l) < max_len else 0.0) == 0.0
    q2r = plan['query_to_rows']
    for q in range(Q):
        exp = [c * max_len + int((lists[c] == q).nonzero()[0]) for c in range(nc) if (lists[c] == q).any()]
        assert [int(v) for v in q2r[q] if v >= 0] == exp
    # cached on the mask tensor: the encoder's layers share one plan
    assert sca._rebatch_plan(bev_mask, ref) is plan


def test_x3linear_on_host_is_a_plain_linear():
    """X3Linear without a device tensor / without autograd is F.linear (the training kernels are device-only; the
    module must still construct, load state and run its reference arithmetic anywhere)."""
    import torch.nn as nn
    import torch.nn.functional as F
    from occnet_amd.plugin.bricks import X3Linear
    m = X3Linear(16, 8)
    ref = nn.Linear(16, 8)
    ref.load_state_dict(m.state_dict())
    x = torch.randn(3, 5, 16, requires_grad=True)
    y = m(x)
    assert torch.equal(y, F.linear(x, m.weight, m.bias))
    assert torch.equal(m(x, act='relu'), torch.relu(y))
    y.sum().backward()
    assert m.weight.grad is not None and x.grad is not None


def test_fp16_value_range_terms_and_aten_scale():
    """Range-safe fp16 SCA value rows.  LazyFeatures._range_terms: the weight-side constants of the
    a-priori bound (largest absolute row sum of W, largest |group bias|) are derived once per weight state, stay on the
    device, and follow in-place updates; ext.f16_range_scaled (the ATen counterpart for fp32-projected rows): a power-of-two scale that puts
    max|v| into [2^14, 2^15], exact to undo, 1 for all-zero / non-finite rows."""
    from occnet_amd import ext
    from occnet_amd.plugin.transformer_occ import LazyFeatures
    lf = LazyFeatures.__new__(LazyFeatures)
    vp = torch.nn.Linear(8, 4)
    with torch.no_grad():
        vp.weight.copy_(torch.arange(32.).view(4, 8) - 10.0)
    gb = torch.tensor([[[0.5, -7.25, 1.0, 2.0]]])
    t = lf._range_terms(vp, gb)                                # a 2-element tensor on the weights' device: never read back
    l1, bm = float(t[0]), float(t[1])
    assert l1 == float(vp.weight.abs().sum(1).max()) and bm == 7.25
    assert lf._range_terms(vp, gb) is t and vp._occ_range_terms.keys()[0][0][1] == vp.weight._version
    with torch.no_grad():
        vp.weight.mul_(3.0)                                    # in-place update: new weight state, measured again
    assert float(lf._range_terms(vp, gb)[0]) == 3.0 * l1
    for amp in (1e-6, 0.37, 6.0, 1.8e4, 1e5, 1e7, 3e30):
        v = torch.randn(5, 7, 16) * amp
        h, s = ext.f16_range_scaled(v)
        m, e = torch.frexp(s)
        assert h.dtype == torch.float16 and s.shape == (1,) and float(m) == 0.5                  # a power of two
        top = float((v.abs().max() * s))
        assert 2.0 ** 14 <= top <= 2.0 ** 15 and torch.isfinite(h).all() and float(h.abs().max()) < 65504
        back = h.float() / s
        assert float((back - v).abs().max()) <= float(v.abs().max()) * 2.0 ** -11
    for bad in (torch.zeros(3, 4), torch.tensor([1.0, float('inf')]), torch.tensor([float('nan'), 2.0])):
        assert float(ext.f16_range_scaled(bad)[1]) == 1.0


def test_value_range_a_priori_bound_dominates_every_projection():
    """csrc/value_range.hip's inequality, restated on the host: for ANY map x with max|x| = a,
    |x . W[n] + gbias[n]| <= a * max_n sum_k |W[n][k]| * (1 + 2^-8) + max|gbias| =: bound, and with s = 2^(15 - e) for
    bound = m * 2^e (m in [0.5, 1)) every scaled value stays <= 2^15 — half of fp16's largest finite number — also for the
    adversarial map that attains the bound (x = a * sign(W[n*])), and the fp16 rows keep 11 significant bits relative to the
    plane's bound.  (The kernel itself against torch: tests/test_gpu_value_range.py.)"""
    import math
    g = torch.Generator().manual_seed(5)
    for amp in (1e-3, 6.0, 1.8e4, 1e7, 3e30):
        W = ((torch.rand(64, 96, generator=g) * 2 - 1) * 0.1).double()
        gb = (torch.randn(64, generator=g) * 3).double()
        x = (torch.randn(200, 96, generator=g) * amp).to(torch.bfloat16)
        nstar = int(W.abs().sum(1).argmax())
        a = float(x.abs().max())
        x[0] = (torch.sign(W[nstar]) * a).to(torch.bfloat16)          # attains a * rowL1(W[n*]) exactly (a is a bf16 number)
        v = x.double() @ W.T + gb
        l1, bm = float(W.abs().sum(1).max()), float(gb.abs().max())
        bound = float(torch.tensor(l1, dtype=torch.float32) * torch.tensor(a, dtype=torch.float32) * 1.00390625
                      + torch.tensor(bm, dtype=torch.float32))     # the kernel's fp32 arithmetic
        assert float(v.abs().max()) <= bound
        assert float(v.abs().max()) >= 0.99 * (a * l1 - bm)            # ... and the bound is tight: the adversarial row reaches it
        m, e = math.frexp(bound)
        k = max(-100, min(100, 15 - e))
        s = 2.0 ** k
        if -100 < 15 - e < 100:
            assert 2.0 ** 14 <= bound * s <= 2.0 ** 15
        h = (v * s).float().half()
        assert torch.isfinite(h).all() and float(h.abs().max()) <= 2.0 ** 15
        back = h.double() / s
        assert float((back - v).abs().max()) <= bound * 2.0 ** -11 + 2.0 ** -24 / s   # 11 bits of the bound; subnormal floor
