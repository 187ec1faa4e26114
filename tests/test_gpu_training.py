"""-m gpu: gradients through the MI355X path (HIP forward + backward deformable-attention kernels inside
the reference-shaped autograd graph) vs torch.autograd through the CPU oracle, and one DDP/RCCL
training step on a single-rank process group."""
import os

import pytest
import torch

from occnet_amd import synthetic
from tests.train_glue_ref import keep_mask as _keep_mask          # host restatement of csrc/ln_dropout_train.hip's keep decision
from tests.util import build_pair, small_cfg

pytestmark = pytest.mark.gpu


def _targets(g, batch=1, seed=0):
    from occnet_amd.train import synthetic_targets
    return synthetic_targets(g['bev_h'], g['bev_w'], g['pillar_h'], num_classes=17, batch=batch, seed=seed)


@pytest.mark.parametrize("prev", [False, True])
def test_loss_gradients_match_oracle(prev):
    g = small_cfg(bev=(20, 20), num_layers=2)
    prod, ora = build_pair(g, seed=3)      # eval(): BN uses running stats, dropout off, grads on
    feats = synthetic.make_features(g, seed=3)
    metas = synthetic.make_img_metas(g)
    sem, flow, mask = _targets(g)
    prev_bev = None
    if prev:
        prev_bev = torch.randn(1, g['bev_h'] * g['bev_w'], g['embed_dims'],
                               generator=torch.Generator().manual_seed(8)) * 0.5
    out_p = prod([f.cuda() for f in feats], metas, prev_bev=None if prev_bev is None else prev_bev.cuda())
    lp = prod.loss(sem.cuda(), flow.cuda(), mask.cuda(), out_p)
    (lp['loss_occ'] + lp['loss_flow']).backward()
    out_o = ora(feats, metas, prev_bev=prev_bev)
    lo = ora.loss(sem, flow, mask, out_o)
    (lo['loss_occ'] + lo['loss_flow']).backward()
    for k in ('loss_occ', 'loss_flow'):
        d = abs(float(lp[k]) - float(lo[k]))
        print(f"{k}: hip {float(lp[k]):.6f} oracle {float(lo[k]):.6f}")
        assert d < 1e-4
    po = dict(ora.named_parameters())
    checked = 0
    for name, p in prod.named_parameters():
        if p.grad is None:
            assert po[name].grad is None or float(po[name].grad.abs().max()) == 0.0, name
            continue
        ref = po[name].grad
        scale = float(ref.abs().max())
        d = float((p.grad.cpu() - ref).abs().max())
        # 2e-3 of the tensor's largest gradient + an absolute floor: tensors whose gradient is a sum of
        # thousands of cancelling O(1) terms (sampling_offsets.weight: |grad| ~ 1e-4) sit at fp32
        # accumulation noise (~5e-6) in both implementations (float atomics reorder the sum)
        # the decoder's convolution weights (round 4: their forward / dx / dW run on the bf16x3 kernels): a sum over all
        # voxels of terms that largely cancel, fed by a dY that went through three bf16x3 stages — floor 5e-5
        floor = 5e-5 if name.endswith('conv.weight') and '.decoder.' in name else 2e-5
        assert d < 2e-3 * scale + floor, (name, d, scale)
        checked += 1
    print(f"prev={prev}: {checked} parameter gradients within 2e-3*max|grad| + 2e-5")
    assert checked > 40


def test_ddp_train_step_single_rank():
    """DDP (RCCL process group of one rank) + AdamW + grad clip on a reduced base config: parameters move,
    losses are finite, every trainable parameter receives a gradient (find_unused_parameters=False)."""
    import torch.distributed as dist
    from occnet_amd.plugin import Config, build_model, import_plugin
    from occnet_amd.train import make_optimizer, synthetic_targets, train_step, wrap_ddp
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Config.fromfile(os.path.join(root, 'configs', 'occ_base_200x200x16.py'))
    # the base model (ResNet-50 + FPN + 4 encoder layers) on small images and a 40x40x16 grid
    cfg.merge_from_dict({'model.pts_bbox_head.bev_h': 40, 'model.pts_bbox_head.bev_w': 40,
                         'model.pts_bbox_head.positional_encoding.row_num_embed': 40,
                         'model.pts_bbox_head.positional_encoding.col_num_embed': 40,
                         'model.pts_bbox_head.transformer.rotate_center': [20, 20]})
    import_plugin(cfg)
    torch.manual_seed(0)
    model = build_model(cfg.model)
    model.init_weights()
    device = torch.device('cuda', 0)
    model = model.to(device).train()
    created = False
    if not dist.is_initialized():
        dist.init_process_group('nccl', init_method='tcp://127.0.0.1:29533', rank=0, world_size=1,
                                device_id=device)
        created = True
    try:
        ddp = wrap_ddp(model, device)
        opt = make_optimizer(ddp)
        geo = dict(synthetic.BASE, img_h=128, img_w=224)
        img = synthetic.make_images(geo, batch=1, seed=0, device=device)
        metas = synthetic.make_img_metas(geo, batch=1)
        head = model.pts_bbox_head
        sem, flow, mask = synthetic_targets(head.bev_h, head.bev_w, head.transformer.pillar_h,
                                            num_classes=head.num_classes, device=device)
        before = head.bev_embedding.weight.detach().clone()
        for _ in range(2):      # the 2nd step trips DDP's unused-parameter check if any were missed
            losses = train_step(ddp, opt, img, metas, sem, flow, mask)
        vals = {k: float(v) for k, v in losses.items()}
        print("train step losses:", vals)
        assert all(v == v and abs(v) < 1e6 for v in vals.values())
        assert float((head.bev_embedding.weight - before).abs().max()) > 0.0
        missing = [n for n, p in model.named_parameters() if p.requires_grad and p.grad is None]
        assert not missing, missing
    finally:
        if created:
            dist.destroy_process_group()


def test_history_bev_inside_training_keeps_the_derived_caches():
    """obtain_history_bev flips a training model to eval() and back every step.  That must not
    invalidate the derived-weight caches (packed Linear weights, folded positional terms, group biases): the epoch stays,
    and a second call packs nothing new and reproduces the first call's BEV (the stock backbone runs on MIOpen, whose
    solver choice may differ between the first and later calls: compared to 1e-3 of the BEV's scale)."""
    import occnet_amd
    from occnet_amd import ext
    from occnet_amd.plugin import Config, build_model, import_plugin
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Config.fromfile(os.path.join(root, 'configs', 'occ_base_200x200x16.py'))
    cfg.merge_from_dict({'model.pts_bbox_head.bev_h': 40, 'model.pts_bbox_head.bev_w': 40,
                         'model.pts_bbox_head.positional_encoding.row_num_embed': 40,
                         'model.pts_bbox_head.positional_encoding.col_num_embed': 40,
                         'model.pts_bbox_head.transformer.rotate_center': [20, 20]})
    import_plugin(cfg)
    torch.manual_seed(0)
    model = build_model(cfg.model)
    model.init_weights()
    device = torch.device('cuda', 0)
    model = model.to(device).train()
    geo = dict(synthetic.BASE, img_h=128, img_w=224)
    frames = torch.stack([synthetic.make_images(geo, batch=1, seed=s, device=device) for s in (0, 1)], 1)
    metas = []
    for i in range(2):
        m = synthetic.make_img_metas(geo, batch=1)[0]
        m['prev_bev_exists'] = i > 0
        metas.append(m)
    metas_list = [{0: metas[0], 1: metas[1]}]
    epoch0 = occnet_amd.cache_epoch()
    bev1 = model.obtain_history_bev(frames, metas_list)
    assert model.training                                   # mode restored
    packs1, ptrs1 = len(ext._PACKED_W), set(ext._PACKED_W.keys())
    bev2 = model.obtain_history_bev(frames, metas_list)
    assert occnet_amd.cache_epoch() == epoch0
    assert len(ext._PACKED_W) == packs1 and set(ext._PACKED_W.keys()) == ptrs1
    assert float((bev1 - bev2).abs().max()) <= 1e-3 * float(bev1.abs().max())


def test_ddp_two_ranks_gradients_identical():
    """1-vs-N gradient equality: two DDP ranks with different samples end
    one training step with IDENTICAL gradients, equal to the mean of their rank-local gradients — with and
    without the bf16 backbone autocast.  Ranks share the box's single GPU over gloo (tests/ddp_grad_worker.py);
    the multi-GPU run takes the same code with RCCL."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", "29547", os.path.join(root, "tests", "ddp_grad_worker.py")]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert res.returncode == 0, res.stderr[-3000:]
    line = [l for l in res.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    for mode in ("fp32", "autocast"):
        r = out[mode]
        print(mode, r)
        assert r["ddp"][0] == r["ddp"][1]                         # bitwise the same reduced gradient on both ranks
        assert r["local"][0] != r["local"][1]                     # the un-reduced ones differ (different samples)
        # backward is not bitwise reproducible (integer-atomic slot order in grad_value; bf16 autocast), so the
        # re-computed local gradients carry run-to-run noise
        assert r["rel_err_vs_mean_of_local"] < (2e-2 if mode == "autocast" else 1e-3), r
        assert r["n_grad"] > 1e6


@pytest.mark.parametrize("angle", [0.0, 7.5, -33.0, 90.0, 180.0])
def test_history_bev_rotation_matches_oracle(angle):
    """prev-BEV rotation (torchvision rotate in the reference, transformer_occ.py:195-205): product vs
    the oracle's independent affine-grid restatement; nearest sampling -> exact equality."""
    import oracle.model as om
    from occnet_amd.plugin.transformer_occ import rotate_bev_nearest
    x = torch.randn(5, 40, 40, generator=torch.Generator().manual_seed(1))
    ref = om.rotate_nearest(x, angle, center=[20, 20])
    got = rotate_bev_nearest(x.cuda(), angle, [20, 20]).cpu()
    frac = float((ref != got).float().mean())
    print(f"angle {angle}: mismatching pixels {frac:.5f}")
    assert frac < 2e-3           # a sample landing exactly between two pixels may round either way


def test_head_forward_with_rotated_history_bev():
    from tests.util import TOL, maxdiff
    g = small_cfg()
    prod, ora = build_pair(g, seed=4)
    feats = synthetic.make_features(g, seed=4)
    metas = synthetic.make_img_metas(g)
    for m in metas:
        m['can_bus'][-1] = 11.25
    prev_bev = torch.randn(1, g['bev_h'] * g['bev_w'], g['embed_dims'],
                           generator=torch.Generator().manual_seed(9)) * 0.5
    with torch.no_grad():
        out_o = ora(feats, metas, prev_bev=prev_bev.clone())
        out_p = prod([f.cuda() for f in feats], metas, prev_bev=prev_bev.cuda())
    for k in ('bev_embed', 'occ', 'flow'):
        d = maxdiff(out_p[k], out_o[k])
        print(f"rotated prev_bev {k}: max|hip - oracle| = {d:.3e}")
        assert d < TOL


def test_sca_training_path_projected_rebatch_equals_reference_order():
    """SpatialCrossAttention's autograd path: the query-side Linears applied once per BEV query with their OUTPUT
    rows dealt to the cameras (default) vs the reference's literal order (rebatch the queries, then the Linears)
    — same losses, same parameter gradients (a Linear is row-wise; only the summation order of the weight gradient
    differs)."""
    from occnet_amd.plugin.spatial_cross_attention import SpatialCrossAttention
    g = small_cfg(bev=(20, 20), num_layers=2)
    feats = synthetic.make_features(g, seed=5)
    metas = synthetic.make_img_metas(g)
    sem, flow, mask = _targets(g)
    res = {}
    for flag in (True, False):
        SpatialCrossAttention.rebatch_projected = flag
        try:
            prod, _ = build_pair(g, seed=5)
            out = prod([f.cuda() for f in feats], metas)
            lp = prod.loss(sem.cuda(), flow.cuda(), mask.cuda(), out)
            (lp['loss_occ'] + lp['loss_flow']).backward()
            res[flag] = ({k: float(v) for k, v in lp.items()},
                         {n: p.grad.detach().clone() for n, p in prod.named_parameters() if p.grad is not None})
        finally:
            SpatialCrossAttention.rebatch_projected = True
    for k in res[True][0]:
        assert abs(res[True][0][k] - res[False][0][k]) < 1e-5
    assert res[True][1].keys() == res[False][1].keys()
    worst = 0.0
    for n, gr in res[False][1].items():
        d = float((res[True][1][n] - gr).abs().max())
        floor = 3e-5 if n.endswith('conv.weight') and '.decoder.' in n else 1e-5      # see test_loss_gradients_match_oracle
        assert d < 1e-3 * float(gr.abs().max()) + floor, (n, d)
        worst = max(worst, d / (float(gr.abs().max()) + 1e-12))
    print(f"projected-rebatch vs reference order: worst relative gradient difference {worst:.2e}")


def test_rows_gather_sum_matches_torch_index_ops_and_gradient():
    """ext.rows_gather_sum (the SCA training path's rebatch / scatter-back) vs index_select / index_add_, forward
    and gradient, incl. padding (-1), queries seen by 0..3 cameras and a batch of 2."""
    from occnet_amd import ext
    g = torch.Generator().manual_seed(11)
    Q, nc, F = 300, 4, 64
    lists = [torch.nonzero(torch.rand(Q, generator=g) > 0.55).squeeze(-1) for _ in range(nc)]
    max_len = max(len(l) for l in lists)
    r2q = torch.full((nc * max_len, 1), -1, dtype=torch.long)
    for i, l in enumerate(lists):
        r2q[i * max_len:i * max_len + len(l), 0] = l
    kmax = max(int(torch.bincount(torch.cat(lists), minlength=Q).max()), 1)
    q2r = torch.full((Q, kmax), -1, dtype=torch.long)
    fill = [0] * Q
    for i, l in enumerate(lists):
        for j, q in enumerate(l.tolist()):
            q2r[q, fill[q]] = i * max_len + j
            fill[q] += 1
    x = torch.randn(2, Q, F, generator=g)
    # reference on the host in float64
    xr = x.double().requires_grad_()
    valid = (r2q[:, 0] >= 0).double().view(1, -1, 1)
    yr = xr.index_select(1, r2q[:, 0].clamp(min=0)) * valid
    go = torch.randn(2, nc * max_len, F, generator=g)
    yr.backward(go.double())
    xd = x.cuda().requires_grad_()
    y = ext.RowsGatherSumFunction.apply(xd, r2q.cuda(), q2r.cuda())
    y.backward(go.cuda())
    torch.cuda.synchronize()
    from tests.grad_bounds import ROWS_GATHER_GRAD_ABS, ROWS_GATHER_OUT_ABS
    assert float((y.detach().cpu().double() - yr.detach()).abs().max()) == ROWS_GATHER_OUT_ABS          # a copy
    assert float((xd.grad.cpu().double() - xr.grad).abs().max()) < ROWS_GATHER_GRAD_ABS
    # the other direction: scatter-back = gather-sum over the inverse map
    o = torch.randn(2, nc * max_len, F, generator=g)
    s_ref = torch.zeros(2, Q, F, dtype=torch.double).index_add_(1, r2q[:, 0].clamp(min=0), o.double() * valid)
    s = ext.rows_gather_sum(o.cuda(), q2r.cuda())
    assert float((s.cpu().double() - s_ref).abs().max()) < 1e-5


def test_sca_prep_function_matches_torch_ops_and_gradient():
    """ext.SCAPrepFunction (rebatch + softmax + offset normalisation + anchor add, and its backward) vs the same
    arithmetic in float64 torch ops with autograd."""
    from occnet_amd import ext
    g = torch.Generator().manual_seed(12)
    bs, Q, nc, M, L, P, Z = 2, 150, 3, 8, 4, 8, 4
    lists = [torch.nonzero(torch.rand(Q, generator=g) > 0.5).squeeze(-1) for _ in range(nc)]
    max_len = max(len(l) for l in lists)
    R = nc * max_len
    r2q = torch.full((R, 1), -1, dtype=torch.long)
    for i, l in enumerate(lists):
        r2q[i * max_len:i * max_len + len(l), 0] = l
    kmax = max(int(torch.bincount(torch.cat(lists), minlength=Q).max()), 1)
    q2r = torch.full((Q, kmax), -1, dtype=torch.long)
    fill = [0] * Q
    for i, l in enumerate(lists):
        for j, q in enumerate(l.tolist()):
            q2r[q, fill[q]] = i * max_len + j
            fill[q] += 1
    shapes = torch.tensor([[20, 30], [10, 15], [5, 8], [3, 4]])
    proj = torch.randn(bs, Q, 3 * M * L * P, generator=g)
    ref = torch.rand(bs, R, Z, 2, generator=g)
    g_loc = torch.randn(bs, R, M, L, P, 2, generator=g)
    g_att = torch.randn(bs, R, M, L, P, generator=g)
    # float64 reference with autograd
    pr = proj.double().requires_grad_()
    valid = (r2q[:, 0] >= 0).double().view(1, R, 1)
    rb = pr.index_select(1, r2q[:, 0].clamp(min=0)) * valid
    n_off = M * L * P * 2
    off = rb[..., :n_off].reshape(bs, R, M, L, P, 2)
    att = rb[..., n_off:].reshape(bs, R, M, L * P).softmax(-1).view(bs, R, M, L, P)
    norm = torch.stack([shapes[:, 1], shapes[:, 0]], -1).double()
    off = off / norm[None, None, None, :, None, :]
    loc = ref.double()[:, :, None, None, None, :, :] + off.view(bs, R, M, L, P // Z, Z, 2)
    loc = loc.view(bs, R, M, L, P, 2)
    (loc * g_loc.double()).sum().add((att * g_att.double()).sum()).backward()
    pd = proj.cuda().requires_grad_()
    loc_d, att_d = ext.SCAPrepFunction.apply(pd, r2q.cuda(), q2r.cuda(), ref.cuda(), shapes.cuda(), M, L, P)
    ((loc_d * g_loc.cuda()).sum() + (att_d * g_att.cuda()).sum()).backward()
    torch.cuda.synchronize()
    e_loc = float((loc_d.detach().cpu().double() - loc.detach()).abs().max())
    e_att = float((att_d.detach().cpu().double() - att.detach()).abs().max())
    e_g = float((pd.grad.cpu().double() - pr.grad).abs().max() / pr.grad.abs().max())
    print(f"sca_prep: loc {e_loc:.2e} attn {e_att:.2e} grad rel {e_g:.2e}")
    from tests.grad_bounds import SCA_PREP_ATTN_ABS, SCA_PREP_GRAD_REL, SCA_PREP_LOC_ABS
    assert e_loc < SCA_PREP_LOC_ABS and e_att < SCA_PREP_ATTN_ABS and e_g < SCA_PREP_GRAD_REL


def test_data_copy_before_eval_is_caught_by_the_content_fingerprint():
    """a weight rewritten through `.data.copy_` (mmcv's EMAHook swap before validation) leaves
    (address, _version) unchanged, so every derived-weight cache would serve the OLD weights in eval.  The detector's
    train -> eval transition fingerprints the contents and bumps the cache epoch when they moved; the eval <-> train
    flips of obtain_history_bev do not (checked above)."""
    import copy
    import occnet_amd
    from occnet_amd import synthetic
    from occnet_amd.plugin import Config, build_model, import_plugin
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Config.fromfile(os.path.join(root, 'configs', 'occ_tiny_50x50x4.py'))
    import_plugin(cfg)
    torch.manual_seed(0)
    model = build_model(cfg.model)
    model.init_weights()
    device = torch.device('cuda', 0)
    model = model.to(device)
    geo = dict(synthetic.BASE)
    geo.update(cfg.get("input_geometry", {}))
    head = model.pts_bbox_head
    geo.update(bev_h=head.bev_h, bev_w=head.bev_w)
    feats = [f.to(device) for f in synthetic.make_features(geo, batch=1, seed=3)]
    metas = synthetic.make_img_metas(geo, batch=1, seed=3)
    model.train()
    model.eval()                                            # first transition: fingerprint recorded
    with torch.no_grad():
        out1 = head(feats, metas)['occ'].clone()
    e0 = occnet_amd.cache_epoch()
    model.train()
    model.eval()                                            # nothing changed: no bump
    assert occnet_amd.cache_epoch() == e0
    model.train()
    fc = head.transformer.encoder.layers[0].ffns[0].layers[1]
    fresh = copy.deepcopy(fc.weight.data) * 0.5 + 0.01
    v0 = fc.weight._version
    fc.weight.data.copy_(fresh)                             # the EMA swap: invisible to _version
    assert fc.weight._version == v0
    model.eval()
    assert occnet_amd.cache_epoch() > e0                    # ... but not to the fingerprint
    with torch.no_grad():
        out2 = head(feats, metas)['occ'].clone()
    assert float((out2 - out1).abs().max()) > 1e-4          # the new weights are what ran
    occnet_amd.invalidate_caches()
    with torch.no_grad():
        out3 = head(feats, metas)['occ']
    assert float((out3 - out2).abs().max()) < 1e-6          # and an explicit invalidation changes nothing further
    # a NORM-PRESERVING rewrite (sign flip; two equal-norm tensors trading places) is invisible to a sum of
    # per-tensor norms — the fingerprint is order-sensitive per tensor
    e1 = occnet_amd.cache_epoch()
    model.train()
    fc.weight.data.neg_()
    model.eval()
    assert occnet_amd.cache_epoch() > e1
    e2 = occnet_amd.cache_epoch()
    model.train()
    n0, n1 = (head.transformer.encoder.layers[i].norms[0].weight for i in (0, 1))
    n0.data.fill_(1.25), n1.data.fill_(0.75)
    model.eval()
    e3 = occnet_amd.cache_epoch()
    assert e3 > e2
    model.train()
    n0.data.fill_(0.75), n1.data.fill_(1.25)                # the two tensors swap contents: same multiset of norms
    model.eval()
    assert occnet_amd.cache_epoch() > e3


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rows", [5, 4003])
def test_dropout_add_layernorm_node_matches_torch(rows, p, monkeypatch):
    """ext.DropoutAddLayerNormFunction (one launch forward, one + a fixed-order reduce backward) against torch ops with the SAME
    keep mask (restated on the host from the kernel's counter-based hash): y, the gradients of x, residual, gamma and beta; the
    library's host copy of the hash equals the restatement; the keep rate is 1 - p."""
    import ctypes
    import numpy as np
    from occnet_amd import _lib, ext
    from tests.grad_bounds import DROPOUT_LN_REL
    g = torch.Generator().manual_seed(rows)
    C = 256
    x0 = torch.randn(2, rows, C, generator=g).cuda()
    r0 = torch.randn(2, rows, C, generator=g).cuda()
    gy = torch.randn(2, rows, C, generator=g).cuda()
    ln = torch.nn.LayerNorm(C).cuda()
    with torch.no_grad():
        ln.weight.copy_(torch.rand(C, generator=g).cuda() + 0.5)
        ln.bias.copy_(torch.randn(C, generator=g).cuda() * 0.1)
    seeds = []
    real = torch.randint
    monkeypatch.setattr(torch, "randint", lambda *a, **k: (lambda t: (seeds.append(int(t.item())), t)[1])(real(*a, **k)))
    x, r = x0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
    assert ext.dropout_add_layernorm_ok(x, r, ln)
    y = ext.dropout_add_layernorm(x, r, ln, p, True)
    monkeypatch.undo()
    y.backward(gy)
    got = [y.detach(), x.grad.clone(), r.grad.clone(), ln.weight.grad.clone(), ln.bias.grad.clone()]
    ln.weight.grad = ln.bias.grad = None
    n = x0.numel()
    if p > 0:
        assert len(seeds) == 1
        keep = _keep_mask(n, seeds[0], p)
        lib = _lib.lib()
        thr = int(p * 4294967296.0)
        for i in (0, 1, 255, 256, n - 1):
            assert (lib.occ_ln_dropout_hash(ctypes.c_uint32(i), ctypes.c_uint32(seeds[0] & 0xffffffff),
                                            ctypes.c_uint32(seeds[0] >> 32)) >= thr) == bool(keep[i])
        assert abs(float(keep.mean()) - (1 - p)) < 4 * (p * (1 - p) / n) ** 0.5 + 1e-4
        mask = torch.from_numpy(keep.astype(np.float32)).cuda().view_as(x0) / (1 - p)
    else:
        assert not seeds
        mask = torch.ones_like(x0)
    x, r = x0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
    yr = ln(x * mask + r)
    yr.backward(gy)
    want = [yr.detach(), x.grad, r.grad, ln.weight.grad, ln.bias.grad]
    for a, b, name in zip(got, want, ("y", "gx", "gres", "dgamma", "dbeta")):
        err = float((a - b).abs().max() / (b.abs().max() + 1e-12))
        assert err < DROPOUT_LN_REL, (name, err)


def test_layer_with_the_fused_tail_matches_the_aten_tail(monkeypatch):
    """A BEVFormerLayer under autograd, dropout inactive (eval mode): the fused dropout + residual + LayerNorm nodes (default)
    against the ATen tail (fused_train_tail = False) — same output, same parameter gradients."""
    from occnet_amd.plugin.encoder import BEVFormerLayer
    g = small_cfg(bev=(20, 20), num_layers=1)
    prod, _ = build_pair(g, seed=5)
    prod = prod.eval()
    feats = [f.cuda() for f in synthetic.make_features(g, seed=5)]
    metas = synthetic.make_img_metas(g)
    layers = [m for m in prod.modules() if isinstance(m, BEVFormerLayer)]
    assert layers
    res = {}
    for fused in (True, False):
        for m in layers:
            m.fused_train_tail = fused
        prod.zero_grad(set_to_none=True)
        out = prod(feats, metas)
        (out['occ'].float().square().mean() + out['flow'].float().square().mean()).backward()
        res[fused] = (out['bev_embed'].detach().clone(),
                      {n: p.grad.detach().clone() for n, p in prod.named_parameters() if p.grad is not None})
    assert res[True][1].keys() == res[False][1].keys() and len(res[True][1]) > 40
    assert float((res[True][0] - res[False][0]).abs().max()) < 2e-5
    for n, gb in res[False][1].items():
        err = float((res[True][1][n] - gb).abs().max() / (gb.abs().max() + 1e-12))
        assert err < 2e-4, (n, err)
