"""gpu: camera visibility masks (csrc/visibility.hip) byte for byte against the reference restatement of
tests/visibility_ref.py — itself pinned to the plain-C caster on the CPU (tests/test_visibility_host.py) — and the masked
confusion counts, exactly, against numpy; then the classes and the two call sites built on them."""
import os

import numpy as np
import pytest
import torch

from tests import render_cases as rc, visibility_cases as vc, visibility_ref as vr

pytestmark = pytest.mark.gpu

DTYPES = ('uint8', 'int64')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _scene(name, dtype, size, seed=0):
    """-> (sem (2, X, Y, Z) device tensor, cams (2, 3, 12) device tensor)"""
    sems, cams = vc.batch(name, np.dtype(dtype), size, seed)
    return _dev(np.stack(sems)), _dev(cams)


def _views(sem, cams, size, **kw):
    from occnet_amd import ext
    return ext.visibility_views(sem, cams, rc.PC_MIN, rc.VOXEL, size, free_id=rc.FREE, far=rc.FAR, **kw)


@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(rc.GRIDS))
def test_mask_equals_reference(name, dtype, size):
    """B = 2 with different cameras per sample (a view taken from the wrong sample's cameras would show), uint16 and uint32
    pillar words, the top bit, Z = 1, rasters with partial tiles in both directions, ids outside 0..free_id."""
    sem, cams = _scene(name, dtype, size)
    got = _views(sem, cams, size)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(sem.shape)
    want = vr.case_mask(name, dtype, size)
    got = got.cpu().numpy()
    print(f"{name} {dtype} {size}: marked {int(want.sum())} of {want.size}, differing {int((got != want).sum())}")
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", list(rc.GRIDS))
def test_mask_of_views_is_the_union_of_single_views(name):
    size = (16, 24)
    sem, cams = _scene(name, 'int64', size)
    whole = _views(sem, cams, size)
    single = [_views(sem, cams[:, v:v + 1].contiguous(), size) for v in range(cams.shape[1])]
    assert torch.equal(whole, single[0] | single[1] | single[2])
    want = vr.case_view_masks(name, 'int64', size)
    for v in range(3):
        assert np.array_equal(single[v].cpu().numpy(), want[:, v]), v
    assert not single[1][1].any()                                        # sample 1's second view looks away: nothing marked


def test_reused_workspace_and_out_need_no_clearing():
    """Scene A, then scene B on the same workspace and the same `out`, pre-filled with 0xAA: what a fresh call with B gives —
    no visibility word of A survives and every byte is written.  Then a smaller grid in the same two buffers."""
    from occnet_amd import ext
    size = (9, 70)
    sem_a, cams_a = _scene('7x5x17', 'uint8', size, seed=0)
    sem_b, cams_b = _scene('7x5x17', 'uint8', size, seed=1)
    fresh_a, fresh_b = _views(sem_a, cams_a, size), _views(sem_b, cams_b, size)
    assert not torch.equal(fresh_a, fresh_b)
    ws = torch.full((ext.visibility_workspace_bytes(*sem_a.shape),), 0xAA, dtype=torch.uint8, device='cuda')
    out = torch.full((sem_a.numel() + 7,), 0xAA, dtype=torch.uint8, device='cuda')
    got_a = _views(sem_a, cams_a, size, out=out, workspace=ws)
    assert got_a.data_ptr() == out.data_ptr() and torch.equal(got_a, fresh_a)
    got_b = _views(sem_b, cams_b, size, out=out, workspace=ws)
    assert torch.equal(got_b, fresh_b)
    assert bool((out[sem_a.numel():] == 0xAA).all())                     # nothing written behind the mask
    sem_c, cams_c = _scene('5x6x4', 'int64', size)
    assert torch.equal(_views(sem_c, cams_c, size, out=out, workspace=ws), _views(sem_c, cams_c, size))
    # an `out` that is not 4-byte aligned takes the byte-wise expansion
    odd = torch.full((sem_c.numel() + 1,), 0xAA, dtype=torch.uint8, device='cuda')[1:]
    assert torch.equal(_views(sem_c, cams_c, size, out=odd, workspace=ws), _views(sem_c, cams_c, size))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(rc.GRIDS))
def test_what_the_renderer_hits_is_marked(name, dtype):
    """For every pixel where render_views reports a hit, at least one voxel of class `label` is marked."""
    from occnet_amd import ext
    size = (16, 24)
    sem, cams = _scene(name, dtype, size)
    mask = _views(sem, cams, size).cpu().numpy()
    r = ext.render_views(sem, cams, rc.PC_MIN, rc.VOXEL, size, free_id=rc.FREE, far=rc.FAR, want=('label', 'depth'))
    label, depth = r['label'].cpu().numpy(), r['depth'].cpu().numpy()
    hits = 0
    for b in range(2):
        marked = set((sem[b].cpu().numpy()[mask[b] == 1].astype(np.int64) & 0xff).tolist())
        hit = depth[b] >= 0
        assert set(label[b][hit].tolist()) <= marked, (b, sorted(set(label[b][hit].tolist()) - marked))
        hits += int(hit.sum())
    assert hits > 0


# ---- confusion counts ------------------------------------------------------------------------------------------------------
def _grids(n, dtype, seed, ids):
    rng = np.random.default_rng(seed)
    pred = rng.choice(np.array(ids, np.int64), n).astype(dtype)
    gt = rng.choice(np.array(ids, np.int64), n).astype(dtype)
    mask = rng.random(n) < 0.6
    return pred, gt, mask


IN_RANGE = list(range(17))
U8_IDS = IN_RANGE + [17, 200, 255]
I64_IDS = IN_RANGE + [17, 300, -3, 2 ** 31, -2 ** 40]


def _state(free_id=16):
    from occnet_amd import ext
    return torch.zeros(ext.confusion_state_words(free_id), dtype=torch.int64, device='cuda')


@pytest.mark.parametrize("mask_kind", [None, 'bool', 'uint8'])
@pytest.mark.parametrize("dtype,ids", [('uint8', U8_IDS), ('int64', I64_IDS)], ids=DTYPES)
@pytest.mark.parametrize("n", [1, 4097, 200 * 200 * 16])
def test_confusion_counts_are_exact(n, dtype, ids, mask_kind):
    from occnet_amd import ext
    pred, gt, mask = _grids(n, dtype, 7 + n % 5, ids)
    if n == 1:
        mask[:] = True
    m = None if mask_kind is None else _dev(mask if mask_kind == 'bool' else mask.astype(np.uint8) * 3)
    state = _state()
    ext.confusion_accumulate(state, _dev(pred), _dev(gt), mask=m, free_id=16)
    want = vr.confusion(pred, gt, None if mask_kind is None else mask, 16)
    assert want[17, 1] == (n if mask_kind is None else int(mask.sum())) and (n == 1 or want[17, 0] > 0)
    assert np.array_equal(state.cpu().numpy().reshape(18, 17), want)
    # a second accumulation, of other grids, adds up exactly
    pred2, gt2, _ = _grids(n, dtype, 99, IN_RANGE)
    ext.confusion_accumulate(state, _dev(pred2), _dev(gt2), free_id=16)
    assert np.array_equal(state.cpu().numpy().reshape(18, 17), want + vr.confusion(pred2, gt2, None, 16))


def test_confusion_counts_with_one_contended_counter_and_mixed_dtypes():
    from occnet_amd import ext
    n = 200 * 200 * 16
    pred, gt = np.full(n, 3, np.uint8), np.full(n, 5, np.int64)
    state = _state()
    ext.confusion_accumulate(state, _dev(pred), _dev(gt), free_id=16)
    want = np.zeros((18, 17), np.int64)
    want[5, 3], want[17, 1] = n, n
    assert np.array_equal(state.cpu().numpy().reshape(18, 17), want)
    small = _state(2)                                                    # free_id = 2: ids 3.. are outside
    ext.confusion_accumulate(small, _dev(pred[:1000]), _dev(gt[:1000]), free_id=2)
    assert small.cpu().tolist() == [0] * 9 + [1000, 1000, 0]


def test_voxel_miou_against_the_reference():
    from occnet_amd.metrics import VoxelMIoU
    shape = (7, 5, 17)
    pc_range = rc.pc_range(shape)
    n = 2 * int(np.prod(shape))
    a, b = VoxelMIoU(pc_range, rc.VOXEL), VoxelMIoU(pc_range, rc.VOXEL)
    total = np.zeros((18, 17), np.int64)
    for k, metric in enumerate((a, b)):
        pred, gt, mask = _grids(n, np.int64 if k else np.uint8, 40 + k, list(range(12)) + [16] * 6 + [40])
        metric.update(_dev(pred).view(2, *shape), gt.reshape(2, *shape), mask.reshape(2, *shape))     # device and host inputs
        want = vr.confusion(pred, gt, mask, 16)
        total += want
        got = metric.compute()
        iou, miou, occupied = vr.iou(want[:17], 16)
        assert np.array_equal(got['iou'], iou, equal_nan=True) and np.isnan(got['iou'][12:16]).all()
        assert got['miou'] == pytest.approx(miou, rel=1e-12) and got['iou_occupied'] == occupied
        assert got['voxels'] == int(mask.sum()) and got['skipped'] == want[17, 0] > 0
        assert np.array_equal(got['confusion'], want[:17])
    a.merge(b)
    got = a.compute()
    iou, miou, occupied = vr.iou(total[:17], 16)
    assert np.array_equal(got['iou'], iou, equal_nan=True) and got['miou'] == pytest.approx(miou, rel=1e-12)
    assert got['voxels'] == total[17, 1] and got['skipped'] == total[17, 0]
    assert int(a.reset().state.abs().sum()) == 0
    a.update(_dev(pred).view(2, *shape), _dev(gt).view(2, *shape))                   # no mask: every voxel
    assert a.compute()['voxels'] == n


# ---- the call sites --------------------------------------------------------------------------------------------------------
def _sparse_semantics(bev_w, bev_h, Z, seed):
    """(1, W, H, Z) uint8: free space over a ground layer, with scattered boxes — a scene the cameras can see into."""
    rng = np.random.default_rng(seed)
    sem = np.full((1, bev_w, bev_h, Z), 16, np.uint8)
    sem[..., 0] = 10
    boxes = rng.random(sem.shape) < 0.04
    sem[boxes] = rng.integers(0, 10, int(boxes.sum())).astype(np.uint8)
    return sem


@pytest.fixture(scope='module')
def tiny_model():
    from occnet_amd import synthetic
    from occnet_amd.plugin import Config, build_model, import_plugin
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Config.fromfile(os.path.join(root, 'configs', 'occ_tiny_50x50x4.py'))
    import_plugin(cfg)
    torch.manual_seed(0)
    model = build_model(cfg.model)
    model.init_weights()
    model = model.cuda().train()
    geo = dict(synthetic.BASE)
    geo.update(cfg.get("input_geometry", {}))
    head = model.pts_bbox_head
    geo.update(bev_h=head.bev_h, bev_w=head.bev_w)
    feats = [f.cuda() for f in synthetic.make_features(geo, batch=1, seed=3)]
    model.extract_feat = lambda img=None, img_metas=None, len_queue=None: feats       # the tiny config takes features in
    metas = synthetic.make_img_metas(geo, batch=1, seed=3)
    sem = torch.from_numpy(_sparse_semantics(head.bev_w, head.bev_h, head.transformer.pillar_h, 5)).cuda()
    flow = torch.randn((1, head.bev_w, head.bev_h, head.transformer.pillar_h, 2), generator=torch.Generator().manual_seed(5)).cuda()
    return model, metas, sem, flow


@pytest.mark.parametrize("fused", [True, False], ids=['fused_loss', 'modules'])
def test_forward_train_builds_the_mask_it_is_not_given(tiny_model, fused):
    from occnet_amd.visibility import CameraVisibility
    from tests.test_gpu_heads_loss import _graph_names_until
    model, metas, sem, flow = tiny_model
    head = model.pts_bbox_head
    had = {k: head.__dict__.get(k) for k in ('fused_loss', 'use_mask') if k in head.__dict__}

    def losses(mask_camera):
        torch.manual_seed(11)                                            # dropout
        np.random.seed(11)
        out = model(return_loss=True, img_metas=metas, img=None, voxel_semantics=sem, voxel_flow=flow, mask_camera=mask_camera)
        names = _graph_names_until(out['loss_occ'].grad_fn, 'OccHeadsLossFunction')
        assert any(n.startswith('OccHeadsLossFunction') for n in names) == fused, names      # the route that was asked for
        return {k: v.detach().clone() for k, v in out.items()}
    try:
        head.fused_loss, head.use_mask = fused, True
        pc_range = [float(v) for v in head.pc_range]
        explicit = CameraVisibility(pc_range, (pc_range[3] - pc_range[0]) / head.bev_w, free_id=head.num_classes - 1)(sem, metas)
        share = float(explicit.float().mean())
        print(f"mask_camera admits {share:.3f} of the voxels")
        assert tuple(explicit.shape) == tuple(sem.shape) and 0.02 < share < 0.98
        built, given = losses(None), losses(explicit)
        for k in ('loss_occ', 'loss_flow'):
            assert torch.equal(built[k], given[k]), (k, float(built[k]), float(given[k]))
        other = losses(torch.ones_like(explicit))                        # a given mask is used as given
        assert not torch.equal(other['loss_occ'], built['loss_occ'])
        head.use_mask = False
        plain = losses(None)
        assert not torch.equal(plain['loss_occ'], built['loss_occ'])
    finally:
        for k in ('fused_loss', 'use_mask'):
            head.__dict__.pop(k, None)
        head.__dict__.update(had)


class _StubModel:
    """simple_test returns prepared device tensors, as BEVFormerOcc.simple_test does: (bev_embed, occ_cls, flow)"""

    def __init__(self, outs):
        self.outs, self.calls = outs, 0

    def simple_test(self, img_metas, img):
        self.calls += 1
        return None, self.outs[self.calls - 1], None


def test_run_test_feeds_the_masked_miou():
    from occnet_amd import synthetic
    from occnet_amd.metrics import VoxelMIoU
    from occnet_amd.eval_loop import run_test
    from occnet_amd.visibility import CameraVisibility
    pc_range, voxel = [-40.0, -40.0, -1.0, 40.0, 40.0, 5.4], 1.6
    samples, outs = [], []
    for i in range(2):
        gt = _sparse_semantics(50, 50, 4, 20 + i)
        pred = gt.copy()
        flip = np.random.default_rng(30 + i).random(gt.shape) < 0.2
        pred[flip] = 3
        outs.append(torch.from_numpy(pred.astype(np.int64)).cuda())
        samples.append(dict(token=f's{i}', img=None, img_metas=synthetic.make_img_metas(synthetic.BASE, batch=1, seed=i, jitter=2.0),
                            voxel_semantics=gt if i else torch.from_numpy(gt).cuda()))       # host and device ground truth
    vis = CameraVisibility(pc_range, voxel, size=(58, 100))
    miou = VoxelMIoU(pc_range, voxel)
    assert run_test(_StubModel(outs), iter(samples), miou=miou, visibility=vis) == 2
    direct, unmasked = VoxelMIoU(pc_range, voxel), VoxelMIoU(pc_range, voxel)
    for s, occ_cls in zip(samples, outs):
        mask = vis(s['voxel_semantics'], s['img_metas'])
        assert 0.02 < float(mask.float().mean()) < 0.98
        direct.update(occ_cls, s['voxel_semantics'], mask)
        unmasked.update(occ_cls, s['voxel_semantics'])
    assert torch.equal(miou.state, direct.state) and not torch.equal(miou.state, unmasked.state)
    res = miou.compute()
    assert 0 < res['voxels'] < 2 * 50 * 50 * 4 and 0.0 < res['miou'] < 1.0
    alone = VoxelMIoU(pc_range, voxel)
    assert run_test(_StubModel(outs), samples, miou=alone) == 2          # no visibility: every voxel
    assert torch.equal(alone.state, unmasked.state)
    with pytest.raises(ValueError):
        run_test(_StubModel(outs), samples, visibility=vis)
    # beside another consumer the loop is test_loop.run_test's, the model behind the tap: one simple_test per sample
    from occnet_amd.vis import OccRenderer
    r, both, model = OccRenderer(pc_range, voxel, size=(29, 50)), VoxelMIoU(pc_range, voxel), _StubModel(outs)
    assert run_test(model, iter(samples), renderer=r, miou=both, visibility=vis) == 2
    assert model.calls == 2 and torch.equal(both.state, direct.state) and list(r.results()) == ['s0', 's1']
    # and without a miou it is that loop, with its own refusals
    r2 = OccRenderer(pc_range, voxel, size=(29, 50))
    assert run_test(_StubModel(outs), samples, renderer=r2) == 2
    assert all(np.array_equal(r2.results()[t]['views'], r.results()[t]['views']) for t in ('s0', 's1'))
    with pytest.raises(ValueError):
        run_test(_StubModel(outs), samples)
