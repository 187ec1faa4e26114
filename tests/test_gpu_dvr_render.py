"""-m gpu: the differentiable ray renderer (ext.dvr_render, csrc/dvr_render_train.hip), its autograd node, RayDepthLoss and the
head's opt-in `loss_depth`, against the float64 restatement of the reference's kernel (tests/dvr_render_ref.py).

Bounds (the same in every test that looks at grad_sigma; nothing here compares two runs with each other — float atomics do
not promise equal last bits):
  gt_dist     bit-equal to float32(gt_d)
  pred_dist   within one float32 ulp of float32(exp_d)  (the device's double exp and libm's may differ in the last bits)
  grad_sigma  per voxel |got - g64| <= (2 n + 4) 2^-24 A + 1e-11 A  (dvr_render_ref.grad_bound), exactly 0 where no ray passed
Precondition of every case: no ray has |exp_d - gt_d| <= 1e-9 max(1, gt_d) unless every sigma on its path is exactly 0 (the
exact tie, which the summation order settles) or every term of the ray is exactly 0 under either sign (a path of one voxel) —
any other ray nearer than that could take either sign of the L1 gradient."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import dvr_render_ref as R
from tests.test_gpu_dvr import _case

pytestmark = pytest.mark.gpu

LOSSES = ("l1", "l2", "absrel")


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """CPU float32 tensors (sigma, origin, points, tindex) of one case; never modified."""
    g = torch.Generator().manual_seed(1234)

    def expo(shape, keep):
        s = torch.empty(shape).exponential_(1.0, generator=g) * 0.05
        return s * (torch.rand(shape, generator=g) < keep).float()
    if name == "small_dense":
        _, origin, points, tindex = _case(1, 1, 1, 4, 6, 8, 300, 0.3)
        sigma = torch.rand(1, 1, 4, 6, 8, generator=g) * 0.8
    elif name == "time_indexed":
        _, origin, points, tindex = _case(2, 2, 3, 8, 20, 24, 2000, 0.05)
        sigma = expo((2, 3, 8, 20, 24), 0.3)
        # ... and nothing in the outermost shell: a ray whose only density lies in its exit voxel renders (1 - T) d + T d against
        # the target d, a tie up to the last bit of exp() (about 1 % of these rays otherwise: the precondition below)
        shell = torch.ones(8, 20, 24, dtype=torch.bool)
        shell[1:-1, 1:-1, 1:-1] = False
        sigma[:, :, shell] = 0.0
    elif name == "empty":
        _, origin, points, tindex = _case(4, 1, 1, 16, 50, 50, 500, 0.0)
        sigma = torch.zeros(1, 1, 16, 50, 50)
    elif name == "outside":
        _, origin, points, tindex = _case(5, 1, 1, 16, 40, 40, 800, 0.1, outside=True)
        sigma = torch.rand(1, 1, 16, 40, 40, generator=g) * 0.5
    elif name == "one_origin":
        _, _, points, _ = _case(6, 1, 1, 16, 200, 200, 512, 0.0)
        origin = torch.tensor([[[100.3, 99.6, 6.2]]])
        tindex = torch.zeros(1, 512)
        sigma = expo((1, 1, 16, 200, 200), 0.3)
    elif name == "step_cap":
        sigma = torch.rand(1, 1, 1, 1, 1100, generator=g) * 0.01
        origin = torch.tensor([[[0.5, 0.5, 0.5], [0.5, 0.3, 0.4]]])
        sigma = sigma.expand(1, 2, 1, 1, 1100).contiguous()
        points = torch.tensor([[[1099.5, 0.5, 0.5], [1099.5, 0.6, 0.7]]])
        tindex = torch.tensor([[0.0, 1.0]])
    elif name == "degenerate":
        sigma = _inputs("small_dense")[0].expand(1, 2, 4, 6, 8).contiguous()
        origin = torch.tensor([[[3.3, 2.2, 1.1], [float('inf'), 2.0, 1.0]]])
        points = torch.tensor([[[3.3, 2.2, 1.1], [5.0, float('nan'), 1.0], [4.0, 4.0, 2.0], [6.0, 1.0, 3.0],
                                [6.0, 1.0, 3.0], [6.0, 1.0, 3.0]]])
        tindex = torch.tensor([[0.0, 0.0, 1.0, -1.0, 2.0, float('nan')]])      # ... and a tindex >= T, a NaN tindex
    else:
        raise KeyError(name)
    return tuple(t.contiguous() for t in (sigma, origin, points, tindex))


@functools.lru_cache(maxsize=None)
def _reference(name, loss):
    return R.render(*(t.numpy() for t in _inputs(name)), loss)


def _assert_precondition(ref):
    close = 0
    for r in ref['rays'].values():
        if not r['entered'] or abs(r['exp_d'] - r['gt_d']) > 1e-9 * max(1.0, r['gt_d']):
            continue
        # a near tie: harmless when every sigma on the path is 0 (the exact tie) or when the ray adds nothing under either sign
        if any(s != 0 for s in r['sigma']) and any(v != 0 for v in r['dd']):
            close += 1
    assert close == 0, f"{close} rays within 1e-9 of a tie: pick another seed"


def _compare(tag, got, ref, grad_scale=1.0):
    """got: (pred, gt, grad) arrays; grad is compared with grad_scale * g64 (one more rounding when the scale is not 1)."""
    pred, gt, grad = got
    want_gt = ref['gt'].astype(np.float32)
    want_pred = ref['pred'].astype(np.float32)
    assert np.array_equal(gt.view(np.uint32), want_gt.view(np.uint32)), tag
    ulps = np.abs(pred.astype(np.float64) - want_pred) / np.spacing(np.abs(want_pred))
    err = np.abs(grad.astype(np.float64) - grad_scale * ref['g64'])
    bound = abs(grad_scale) * R.grad_bound(ref['n'], ref['A'])
    if grad_scale != 1.0:
        bound = bound + 2.0 ** -24 * np.abs(grad_scale * ref['g64'])
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"{tag}: rays rendered {int((pred >= 0).sum())} of {pred.size}, pred max {float(ulps.max()):.2f} ulp, "
          f"grad max |err| {float(err.max()):.3e}, max err / bound {worst:.3f}, voxels hit {int((ref['n'] > 0).sum())}, "
          f"max n {int(ref['n'].max())}")
    assert float(ulps.max()) <= 1.0, tag
    assert not grad[ref['n'] == 0].any(), tag
    assert (err <= bound).all(), (tag, worst)


def _run(name, loss):
    from occnet_amd import ext
    out = ext.dvr_render(*(t.cuda() for t in _inputs(name)), loss)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", ["small_dense", "time_indexed", "empty", "outside", "one_origin", "step_cap"])
def test_render_against_the_restatement(name, loss):
    ref = _reference(name, loss)
    _assert_precondition(ref)
    entered = [r for r in ref['rays'].values() if r['entered']]
    if name == "empty":
        assert all(r['exp_d'] == r['d'][-1] for r in entered)          # sigma == 0: the expected depth IS the exit distance
        beyond = [r for r in entered if r['gt_d'] == r['d'][-1]]       # rays that end beyond the grid: the exact tie
        assert len(beyond) >= 0.3 * len(entered) and all(r['exp_d'] == r['gt_d'] for r in beyond)
        if loss != "l2":
            assert all(r['dl_dd'] > 0 for r in entered) and float(np.abs(ref['g64']).sum()) > 1.0
    if name == "outside":
        cast = len(ref['rays'])
        assert len(entered) >= 0.1 * cast and cast - len(entered) >= 0.1 * cast, (len(entered), cast)
    if name == "one_origin":
        assert int(ref['n'][0, 0, 6, 99, 100]) == 512 and np.mean([len(r['path']) for r in entered]) > 50
    if name == "step_cap":
        assert [len(r['path']) for r in ref['rays'].values()] == [1001, 1001]
    got = _run(name, loss)
    _compare(f"{name}/{loss}", got, ref)
    if name == "small_dense" and loss == "l1":
        bce = _run(name, "bce")
        assert np.array_equal(bce[0].view(np.uint32), got[0].view(np.uint32))
        assert np.array_equal(bce[1].view(np.uint32), got[1].view(np.uint32))
        _compare("small_dense/bce", bce, ref)


@pytest.mark.parametrize("loss", LOSSES)
def test_degenerate_rays_are_padded(loss):
    """zero length, NaN end point, +inf origin, tindex -1 / >= T / NaN: outputs -1, nothing added."""
    pred, gt, grad = _run("degenerate", loss)
    assert (pred == -1).all() and (gt == -1).all() and not grad.any()
    assert not _reference("degenerate", loss)['rays']


def test_autograd_node():
    from occnet_amd import ext
    from occnet_amd.plugin.ray_depth_loss import DvrRenderLoss
    sigma, origin, points, tindex = (t.cuda() for t in _inputs("time_indexed"))
    for loss in LOSSES:
        ref = _reference("time_indexed", loss)
        s, o, p = sigma.clone().requires_grad_(), origin.clone().requires_grad_(), points.clone().requires_grad_()
        loss_sum, n_valid = DvrRenderLoss.apply(s, o, p, tindex, loss)
        assert loss_sum.dim() == 0 and n_valid.dim() == 0 and loss_sum.is_cuda and n_valid.is_cuda and not n_valid.requires_grad
        pred, gt, _ = ext.dvr_render(sigma, origin, points, tindex, loss)
        v = pred >= 0
        d = (pred[v] - gt[v]).double()
        per_ray = {"l1": d.abs(), "l2": 0.5 * d * d, "absrel": d.abs() / gt[v].double()}[loss]
        want = float(per_ray.sum())
        tol = (int(v.sum()) + 3) * 2.0 ** -24 * float(per_ray.abs().sum())      # float32 terms, any float32 summation order
        print(f"autograd/{loss}: loss_sum {float(loss_sum.detach()):.6f} vs {want:.6f} (tol {tol:.2e}), n_valid {int(n_valid)}")
        assert abs(float(loss_sum.detach()) - want) <= tol
        assert int(n_valid) == int(v.sum()) == sum(r['entered'] for r in ref['rays'].values())
        loss_sum.backward(torch.tensor(2.5, device=loss_sum.device))
        assert o.grad is None and p.grad is None
        _compare(f"autograd/{loss}", (pred.cpu().numpy(), gt.cpu().numpy(), s.grad.cpu().numpy()), ref, grad_scale=2.5)


def test_ray_depth_loss_gradient_to_the_logits():
    from occnet_amd.plugin import build_loss
    from occnet_amd.plugin.ray_depth_loss import DvrRenderLoss
    g = torch.Generator().manual_seed(7)
    X, Y, Z, C, M = 10, 12, 4, 17, 256
    logits = torch.randn(1, X, Y, Z, C, generator=g) * 2.0
    dims = torch.tensor([X, Y, Z], dtype=torch.float32)
    origin = (torch.rand(1, 2, 3, generator=g) * dims).cuda()
    points = ((torch.rand(1, M, 3, generator=g) * 3.0 - 1.0) * dims).cuda()
    tindex = torch.randint(0, 2, (1, M), generator=g).float()
    tindex[:, ::13] = -1.0
    tindex = tindex.cuda()
    for loss, weight in (("l1", 0.5), ("l2", 2.0), ("absrel", 1.0)):
        m = build_loss(dict(type='RayDepthLoss', loss=loss, loss_weight=weight, pc_range=[0, 0, 0, 5, 6, 2], voxel_size=0.5))
        occ = logits.cuda().requires_grad_()
        out = m(occ, origin, points, tindex)
        out.backward()
        # the density the kernel read, copied back: the reference consumes these float32 values
        sigma_dev = m.density(occ.detach()).expand(1, 2, Z, Y, X).contiguous()
        ref = R.render(sigma_dev.cpu().numpy(), origin.cpu().numpy(), points.cpu().numpy(), tindex.cpu().numpy(), loss)
        _assert_precondition(ref)
        _, n_valid = DvrRenderLoss.apply(sigma_dev, origin, points, tindex, loss)
        n_ref = sum(r['entered'] for r in ref['rays'].values())
        assert int(n_valid) == n_ref > M // 4
        unit = {"l1": 0.5, "l2": 0.25, "absrel": 1.0}[loss]
        scale = weight * unit / n_ref
        p32, g32 = ref['pred'].astype(np.float32).astype(np.float64), ref['gt'].astype(np.float32).astype(np.float64)
        v = ref['pred'] >= 0
        d = p32[v] - g32[v]
        per_ray = {"l1": np.abs(d), "l2": 0.5 * d * d, "absrel": np.abs(d) / g32[v]}[loss]
        # pred within one ulp per ray, float32 terms and sum, two roundings of the scale
        dper = {"l1": 1.0, "l2": np.abs(d) + 1e-6, "absrel": 1.0 / g32[v]}[loss] * np.spacing(np.float32(p32[v])).astype(np.float64)
        tol = scale * (dper.sum() + (n_ref + 6) * 2.0 ** -24 * per_ray.sum())
        want = scale * per_ray.sum()
        print(f"RayDepthLoss/{loss}: loss {float(out.detach()):.7f} vs {want:.7f} (tol {tol:.2e}), n_valid {n_ref}")
        assert abs(float(out.detach()) - want) <= tol
        # float64 autograd chained onto g64 (summed over the two copies of the grid)
        G = torch.from_numpy(ref['g64'].sum(1)).permute(0, 3, 2, 1) * scale                          # (1, Z, Y, X) -> (1, X, Y, Z)
        occ64 = logits.double().requires_grad_()
        ((torch.logsumexp(occ64, -1) - occ64[..., C - 1]) * G).sum().backward()
        want_grad = occ64.grad.numpy()
        vb = R.grad_bound(ref['n'].sum(1), ref['A'].sum(1)).transpose(0, 3, 2, 1) * scale             # (1, X, Y, Z)
        bound = vb[..., None] + 2.0 ** -20 * np.abs(want_grad)
        err = np.abs(occ.grad.cpu().numpy().astype(np.float64) - want_grad)
        print(f"RayDepthLoss/{loss}: logits grad max |err| {float(err.max()):.3e}, max err / bound "
              f"{float((err / np.where(bound > 0, bound, 1.0)).max()):.3f}, max |grad| {float(np.abs(want_grad).max()):.3e}")
        assert float(np.abs(want_grad).max()) > 0 and (err <= bound).all()


def _scene():
    sem = np.full((1, 50, 50, 4), 16, np.uint8)
    sem[..., 0] = 10                                        # ground layer
    sem[0, 30:34, 20:26, 1:3] = 3                           # two boxes
    sem[0, 10:13, 35:38, 1:4] = 7
    return torch.from_numpy(sem).cuda()


@functools.lru_cache(maxsize=None)
def _targets():
    """(module, sem, origin_vox, points, tindex, per-origin hard casts of the ORIGINAL rays: [(dist, hit, end points)])."""
    from occnet_amd import ext
    from occnet_amd.plugin import build_loss
    m = build_loss(dict(type='RayDepthLoss', free_id=16, voxel_size=1.6))
    sem = _scene()
    origins = torch.tensor([[[0.98, 0.0, 1.84], [-6.0, 9.5, 1.2]]])
    origin_vox, points, tindex = m.targets_from_occupancy(sem, origins)
    rays = m.lidar_rays(sem.device)
    occ = (sem != 16).permute(0, 3, 2, 1)[:, None].float().contiguous()
    off = torch.tensor([-40.0, -40.0, -1.0], device=sem.device)
    vs = torch.tensor([1.6] * 3, device=sem.device)         # a tensor divisor, as process_one_sample's `scaler`: a true division
    casts = []
    for t in range(2):
        o = origins[:, t:t + 1].cuda()
        o_vox = ((o - off) / vs).float().contiguous()
        e_vox = (((rays[None] + o) - off) / vs).float().contiguous()
        dist, _, coord = ext.dvr_render_forward(occ, o_vox, e_vox, torch.zeros(1, rays.shape[0], device=sem.device), None, "test")
        c = coord[0].long()
        cls = sem[0, c[:, 0], c[:, 1], c[:, 2]]
        casts.append((dist[0].cpu().numpy(), ((dist[0] >= 0) & (cls != 16)).cpu().numpy(), e_vox[0].cpu().numpy()))
        assert torch.equal(o_vox, origin_vox[:, t:t + 1])
    torch.cuda.synchronize()
    return m, sem, origin_vox.cpu().numpy(), points.cpu().numpy(), tindex.cpu().numpy(), casts


def test_targets_from_occupancy_mark_the_rays_that_hit():
    """tindex >= 0 exactly on the rays whose hard cast reports a non-free voxel, and their end points stay on their rays:
    within 1e-2 voxels of origin + direction * distance (a hundredth of a voxel, against RayIoU's finest threshold of 2.5
    voxels; end_points_at moves a point off the rounded one to meet the distance)."""
    _, _, origin_vox, points, tindex, casts = _targets()
    R_ = casts[0][0].shape[0]
    assert points.shape == (1, 2 * R_, 3) and tindex.shape == (1, 2 * R_) and points.dtype == tindex.dtype == np.float32
    for t, (dist, hit, e_vox) in enumerate(casts):
        ti, p = tindex[0, t * R_:(t + 1) * R_], points[0, t * R_:(t + 1) * R_].astype(np.float64)
        assert 0.1 < hit.mean() < 1.0
        assert np.array_equal(ti >= 0, hit) and (ti[hit] == t).all() and (ti[~hit] == -1).all()
        o = origin_vox[0, t].astype(np.float64)
        d = e_vox.astype(np.float64) - o
        exact = o + d / np.linalg.norm(d, axis=1, keepdims=True) * dist.astype(np.float64)[:, None]
        off = np.linalg.norm(p[hit] - exact[hit], axis=1)
        print(f"origin {t}: {int(hit.sum())} of {R_} rays hit, end points at most {float(off.max()):.3e} voxels off the exact point")
        assert float(off.max()) <= 1e-2
        assert np.array_equal(p[~hit].astype(np.float32), e_vox[~hit])         # padded rays keep the evaluator's end point


def test_targets_from_occupancy_distance_to_one_ulp():
    """|points - origin| (in double, from the float32 coordinates: what the renderer takes as its target) equals the hard
    cast's distance to one float32 ulp of that distance."""
    _, _, origin_vox, points, _, casts = _targets()
    R_ = casts[0][0].shape[0]
    worst, within, total = 0.0, 0, 0
    for t, (dist, hit, _) in enumerate(casts):
        p = points[0, t * R_:(t + 1) * R_].astype(np.float64)
        norm = np.linalg.norm(p[hit] - origin_vox[0, t].astype(np.float64), axis=1)
        ulps = np.abs(norm - dist[hit]) / np.spacing(dist[hit])
        worst, within, total = max(worst, float(ulps.max())), within + int((ulps <= 1).sum()), total + int(hit.sum())
    print(f"|p - o| vs hit distance: {within} of {total} rays within one ulp of the distance, worst {worst:.2f} ulp")
    assert worst <= 1.0


def _tiny_model(extra):
    from occnet_amd import synthetic
    from occnet_amd.plugin import Config, build_model, import_plugin
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Config.fromfile(os.path.join(root, 'configs', 'occ_tiny_50x50x4.py'))
    import_plugin(cfg)
    model_cfg = dict(cfg.model)
    model_cfg['pts_bbox_head'] = dict(model_cfg['pts_bbox_head'], **extra)
    torch.manual_seed(0)
    np.random.seed(0)
    model = build_model(model_cfg)
    model.init_weights()
    model = model.cuda().train()
    geo = dict(synthetic.BASE)
    geo.update(cfg.get("input_geometry", {}))
    head = model.pts_bbox_head
    geo.update(bev_h=head.bev_h, bev_w=head.bev_w)
    feats = [f.cuda() for f in synthetic.make_features(geo, batch=1, seed=3)]
    model.extract_feat = lambda img=None, img_metas=None, len_queue=None: feats       # the tiny config takes features in
    return model, synthetic.make_img_metas(geo, batch=1, seed=3)


def test_head_with_loss_depth():
    sem = _scene()
    flow = torch.randn((1, 50, 50, 4, 2), generator=torch.Generator().manual_seed(5)).cuda()
    origins = torch.tensor([[[0.98, 0.0, 1.84], [-6.0, 9.5, 1.2]]])

    def losses(model, metas, **kw):
        torch.manual_seed(11)                                            # dropout
        np.random.seed(11)
        return model(return_loss=True, img_metas=metas, img=None, voxel_semantics=sem, voxel_flow=flow, **kw)
    model, metas = _tiny_model(dict(loss_depth=dict(type='RayDepthLoss', loss='l1', loss_weight=0.5)))
    head = model.pts_bbox_head
    with pytest.raises(ValueError, match='lidar_origins'):
        losses(model, metas)
    out = losses(model, metas, lidar_origins=origins)
    assert sorted(out) == ['loss_depth', 'loss_flow', 'loss_occ']
    again = head.forward_loss(model.extract_feat(), metas, None, sem, flow, None, lidar_origins=origins)
    assert sorted(again) == ['loss_depth', 'loss_flow', 'loss_occ']
    depth = float(out['loss_depth'])
    print(f"tiny config: loss_occ {float(out['loss_occ']):.4f} loss_flow {float(out['loss_flow']):.4f} loss_depth {depth:.4f} m")
    assert np.isfinite(depth) and depth > 0
    out['loss_depth'].backward()
    for name, p in (('predicter', head.transformer.predicter[0].weight), ('bev_embedding', head.bev_embedding.weight)):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
    del model
    none, metas_n = _tiny_model(dict(loss_depth=None))
    absent, metas_a = _tiny_model({})
    a, b = losses(none, metas_n), losses(absent, metas_a)
    assert sorted(a) == sorted(b) == ['loss_flow', 'loss_occ']
    for k in a:
        assert torch.equal(a[k], b[k]), k
