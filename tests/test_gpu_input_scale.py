"""The image-scale input kernel (csrc/input_scale_u8.hip, ext.input_u8_scaled) and the detector / test-loop routes built on it.

Every accuracy comparison is against the float64 restatement of tests/input_scale_ref.py under that file's bound
    max|got - ref| <= max(4 * E32, 24 * 2^-23 * max|ref|)
(E32 = the float32 numpy chain's own distance from the float64 restatement on the same inputs).  The resize is the project's
definition ("Image scale on the device"); no pixel is excluded from any comparison and no test reads the
reference tree."""
import os

import numpy as np
import pytest
import torch

from occnet_amd import ext, io
from tests import input_scale_ref as S
from tests import train_input_ref as R

pytestmark = pytest.mark.gpu


def _run(fr, rec, mean, std, to_rgb, scale, gm=None, **kw):
    out, hw = ext.input_u8_scaled(torch.from_numpy(np.ascontiguousarray(fr)).cuda(), rec, mean, std, to_rgb, scale,
                                  grid_mask=gm, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), hw


@pytest.mark.parametrize('grid', S.GRIDS)
@pytest.mark.parametrize('norm', list(R.NORMS))
@pytest.mark.parametrize('scale', S.SCALES)
@pytest.mark.parametrize('shape', S.SHAPES)
def test_kernel_against_float64(shape, scale, norm, grid):
    c = S.case(shape, norm, scale)
    assert c['info']['min_abs_v'] >= 0.1                  # the conditioning, asserted on the float64 reference
    (hd, wd), (H, W) = S.sizes(*shape, scale)
    gm = R.grid_cases(H, W)[grid]
    m64 = R.mask64(H, W, gm)
    ref, f32 = c['ref'] * m64, (c['f32'] * m64.astype(np.float32)).astype(np.float32)
    got, hw = _run(c['frames'], R.RECORDS, c['mean'], c['std'], c['to_rgb'], scale, gm)
    assert hw == (hd, wd) and got.shape == ref.shape == (R.NI, 3, H, W) and got.dtype == np.float32
    e32 = float(np.abs(f32 - ref).max())
    err, tol = float(np.abs(got - ref).max()), S.bound(e32, ref)
    print(f"input_scale {shape} x{scale} {norm} {grid}: max|hip - f64| {err:.3e}  E32 {e32:.3e}  bound {tol:.3e}  "
          f"ratio to bound {err / tol if tol else 0.0:.3f}  bit-equal to the f32 chain: "
          f"{int((got.view(np.uint32) == f32.view(np.uint32)).sum())} of {got.size}")
    assert err <= tol
    assert not got[:, :, hd:].any() and not got[:, :, :, wd:].any()           # the pad area is exactly 0


@pytest.mark.parametrize('grid', S.GRIDS)
@pytest.mark.parametrize('scale', S.SCALES + [1.0])
@pytest.mark.parametrize('shape', S.SHAPES)
def test_resize_is_exact_on_grey_frames(shape, scale, grid):
    """Identity records on grey frames: the HSV round trip is exact there, so the normalised taps are the host chain's bits
    and only the resize arithmetic — indices, weights, the order and rounding of the blends — is on trial.  Bit for bit,
    every element, the pad area and the masked pixels included."""
    fr = S.grey_frames(*shape)
    mean, std, to_rgb = R.NORMS['imagenet_rgb']
    _, (H, W) = S.sizes(*shape, scale)
    gm = R.grid_cases(H, W)[grid]
    ident = io.identity_photometric(len(fr))
    got, _ = _run(fr, ident, mean, std, to_rgb, scale, gm)
    want = S.chain32(fr, ident, mean, std, to_rgb, scale, gm)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize('grid', S.GRIDS)
@pytest.mark.parametrize('shape', S.SHAPES)
def test_scale_one_is_the_existing_kernel(shape, grid):
    fr = torch.from_numpy(R.frames(*shape)).cuda()
    H, W = R.padded(*shape)
    gm = R.grid_cases(H, W)[grid]
    for norm in R.NORMS:
        mean, std, to_rgb = R.NORMS[norm]
        want = ext.train_input_u8(fr, R.RECORDS, mean, std, to_rgb, grid_mask=gm)
        got, hw = ext.input_u8_scaled(fr, R.RECORDS, mean, std, to_rgb, 1.0, grid_mask=gm)
        assert hw == shape and torch.equal(got, want)


def test_memory_discipline():
    """Guards around the output stay bit-unchanged and every element of it is written; nothing around the frames is read:
    they end where their allocation ends, another allocation holds poison, and bytes around them inside one allocation are
    poisoned both ways."""
    shape, scale = (37, 53), 0.8
    c = S.case(shape, 'imagenet_rgb', scale)
    fr = c['frames']
    _, (H, W) = S.sizes(*shape, scale)
    gm = R.grid_cases(H, W)['both_mode1']
    args = (R.RECORDS, c['mean'], c['std'], c['to_rgb'], scale)
    plain, _ = _run(fr, *args, gm)
    n, guard = plain.size, 4096
    big = torch.full((guard + n + guard,), float('nan'), device='cuda')
    before = big.view(torch.int32).clone()
    out = big[guard:guard + n].view(plain.shape)
    outs = []
    for fill, lead, trail in ((0, 37, 0), (255, 37, 0), (0, 37, 91), (255, 64, 91)):
        buf = torch.full((lead + fr.size + trail,), fill, dtype=torch.uint8, device='cuda')
        poison = torch.full((1 << 16,), fill, dtype=torch.uint8, device='cuda')          # whatever follows the frames
        buf[lead:lead + fr.size] = torch.from_numpy(fr.reshape(-1)).cuda()
        frames = buf[lead:lead + fr.size].view(fr.shape)
        assert frames.is_contiguous()
        big.fill_(float('nan'))
        ext.input_u8_scaled(frames, *args, grid_mask=gm, out=out)
        torch.cuda.synchronize()
        after = big.view(torch.int32)
        assert torch.equal(after[:guard], before[:guard]) and torch.equal(after[guard + n:], before[guard + n:])
        assert not bool(torch.isnan(out).any())                 # every element written
        outs.append(out.cpu().numpy().copy())
        del poison
    for o in outs:
        assert np.array_equal(o.view(np.uint32), plain.view(np.uint32))


def test_wrapper_argument_checks():
    fr = torch.zeros(2, 5, 9, 3, dtype=torch.uint8, device='cuda')
    ident = io.identity_photometric(2)
    with pytest.raises(ext.OccAmdError, match='records'):
        ext.input_u8_scaled(fr, io.identity_photometric(3), [0, 0, 0], [1, 1, 1], False, 0.5)
    with pytest.raises(ext.OccAmdUnsupported):
        ext.input_u8_scaled(fr.float(), ident, [0, 0, 0], [1, 1, 1], False, 0.5)
    with pytest.raises(ext.OccAmdUnsupported, match='multiple of 4'):
        ext.input_u8_scaled(fr, ident, [0, 0, 0], [1, 1, 1], False, 1.0, size_divisor=3)         # W = 9
    with pytest.raises(ext.OccAmdError, match='leaves no pixel'):
        ext.input_u8_scaled(fr, ident, [0, 0, 0], [1, 1, 1], False, 0.1)
    with pytest.raises(ext.OccAmdError, match='out must be'):
        ext.input_u8_scaled(fr, ident, [0, 0, 0], [1, 1, 1], False, 0.5, out=torch.zeros(2, 3, 64, 64, device='cuda'))


# ----------------------------------------------------------------------------------------------------- detector
NORM_CFG = dict(mean=[103.530, 116.280, 123.675], std=[1.0, 1.0, 1.0], to_rgb=False)
HS, WS, SCALE = 240, 440, 0.5           # -> 120 x 220 -> 128 x 224, the image size of the reduced base model


@pytest.fixture(scope='module')
def detector():
    """The base config at 40 x 40 BEV queries (the smallest config WITH an image backbone), use_grid_mask=True as the
    reference configures it; frames of 240 x 440, metas of the unscaled (256 x 448 padded) and of the scaled images."""
    from occnet_amd import synthetic
    from occnet_amd.plugin import Config, build_model, import_plugin
    from occnet_amd.train import synthetic_targets
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
    model = model.cuda().train()
    assert model.use_grid_mask
    head = model.pts_bbox_head
    geo = dict(synthetic.BASE, img_h=256, img_w=448)
    plain = synthetic.make_img_metas(geo, batch=1)
    scaled = [io.scale_img_metas(m, SCALE, (HS, WS)) for m in plain]
    assert scaled[0]['img_shape'] == [(128, 224, 3)] * 6
    sem, flow, mask = synthetic_targets(head.bev_h, head.bev_w, head.transformer.pillar_h, num_classes=head.num_classes,
                                        device='cuda')
    rng = np.random.RandomState(11)
    frames = torch.from_numpy(rng.randint(0, 256, size=(1, 6, HS, WS, 3)).astype(np.uint8)).cuda()
    return model, dict(voxel_semantics=sem, voxel_flow=flow, mask_camera=mask), frames, plain, scaled


def _losses(model, kw, seed, **inp):
    np.random.seed(seed)                         # GridMask
    torch.manual_seed(seed)                      # dropout
    with torch.no_grad():
        return {k: float(v) for k, v in model(return_loss=True, **kw, **inp).items()}


def _masked_input(model, frames, aug, seed):
    """The tensor forward_train builds under `seed`: ext.input_u8_scaled with the GridMask module's own draws."""
    np.random.seed(seed)
    _, (H, W) = S.sizes(HS, WS, SCALE)
    g = model.grid_mask
    drawn = g.train().sample_params(H, W)
    gm = None if drawn is None else tuple(drawn) + (int(bool(g.use_h)), int(bool(g.use_w)), int(g.mode))
    x, _ = ext.input_u8_scaled(frames[0], aug, NORM_CFG['mean'], NORM_CFG['std'], NORM_CFG['to_rgb'], SCALE, grid_mask=gm)
    return x[None], gm


def test_forward_train_at_a_scale(detector):
    model, kw, frames, plain, scaled = detector
    model.train()
    np.random.seed(4)
    aug = io.sample_photometric(6)
    seed = next(s for s in range(100) if np.random.RandomState(s).rand() <= 0.7)          # the mask is applied
    img, gm = _masked_input(model, frames, aug, seed)
    assert gm is not None and float((img == 0).float().mean()) > 0.05
    model.use_grid_mask = False                  # `img` carries the mask already
    try:
        _losses(model, kw, seed, img=img, img_metas=scaled)          # lets the convolution library settle on its solvers
        want = _losses(model, kw, seed, img=img, img_metas=scaled)
    finally:
        model.use_grid_mask = True
    got = _losses(model, kw, seed, img_u8=frames, img_norm_cfg=NORM_CFG, img_aug=aug, img_scale=SCALE, img_metas=scaled)
    assert got == want, (got, want)
    with pytest.raises(ValueError, match='io.scale_img_metas'):
        _losses(model, kw, seed, img_u8=frames, img_norm_cfg=NORM_CFG, img_aug=aug, img_scale=SCALE, img_metas=plain)
    with pytest.raises(ValueError, match='img_scale'):
        _losses(model, kw, seed, img=img, img_scale=SCALE, img_metas=scaled)


def test_forward_train_without_a_scale_is_what_it_was(detector):
    """img_scale=None: the losses of forward_train(img=) fed ext.train_input_u8's tensor under the GridMask module's own draws,
    bit for bit: without a scale the uint8 route still goes through the kernel it went through."""
    model, kw, frames, _, metas = detector
    model.train()
    np.random.seed(4)
    aug = io.sample_photometric(6)
    seed = next(s for s in range(100) if np.random.RandomState(s).rand() <= 0.7)          # the mask is applied
    small = frames[:, :, :120, :220].contiguous()           # pads to the 128 x 224 of `metas` as it is
    np.random.seed(seed)
    g = model.grid_mask
    gm = tuple(g.sample_params(128, 224)) + (int(bool(g.use_h)), int(bool(g.use_w)), int(g.mode))
    img = ext.train_input_u8(small[0], aug, NORM_CFG['mean'], NORM_CFG['std'], NORM_CFG['to_rgb'], grid_mask=gm)[None]
    model.use_grid_mask = False                  # `img` carries the mask already
    try:
        _losses(model, kw, seed, img=img, img_metas=metas)
        want = _losses(model, kw, seed, img=img, img_metas=metas)
    finally:
        model.use_grid_mask = True
    args = dict(img_u8=small, img_norm_cfg=NORM_CFG, img_aug=aug, img_metas=metas)
    assert _losses(model, kw, seed, **args) == want
    assert _losses(model, kw, seed, img_scale=None, **args) == want


def _test_outputs(model, metas, *img, **inp):
    np.random.seed(0)
    with torch.no_grad():
        _, occ_cls, flow = model.simple_test(metas, *img, **inp)
    torch.cuda.synchronize()
    return occ_cls, flow


@pytest.mark.parametrize('fused', [False, True], ids=['modules', 'fused_backbone'])
def test_simple_test_at_a_scale(detector, fused):
    model, _, frames, plain, scaled = detector
    model.eval()
    if fused:
        model.enable_fused_backbone()
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True          # the stock convolutions of the module route: deterministic solvers only
    try:
        img, _ = ext.input_u8_scaled(frames[0], io.identity_photometric(6), NORM_CFG['mean'], NORM_CFG['std'],
                                     NORM_CFG['to_rgb'], SCALE)
        _test_outputs(model, scaled, img=img[None])
        want = _test_outputs(model, scaled, img=img[None])
        got = _test_outputs(model, scaled, img_u8=frames, img_norm_cfg=NORM_CFG, img_scale=SCALE)
        assert want[0].shape[1:3] == (40, 40) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        with pytest.raises(ValueError, match='io.scale_img_metas'):
            _test_outputs(model, plain, img_u8=frames, img_norm_cfg=NORM_CFG, img_scale=SCALE)
        # no scale: the uint8 route of extract_feat_u8, as before; and the img route under its old signature
        small = frames[:, :, :120, :220].contiguous()       # pads to the 128 x 224 of `scaled` as it is
        np.random.seed(0)
        with torch.no_grad():
            _, occ_old, flow_old = model.simple_test_pts(model.extract_feat_u8(small, NORM_CFG)[0], scaled)
        got = _test_outputs(model, scaled, img_u8=small, img_norm_cfg=NORM_CFG)
        assert torch.equal(got[0], occ_old) and torch.equal(got[1], flow_old)
        assert all(torch.equal(a, b) for a, b in zip(_test_outputs(model, scaled, img[None]), want))
    finally:
        torch.backends.cudnn.deterministic = was
        if fused:
            model.enable_fused_backbone(dtype=None)
        model.train()


def test_history_bev_at_a_scale(detector):
    """obtain_history_bev on a uint8 queue with img_scale: the BEV of the queue of prepared tensors, bit for bit (inference
    plan on, so both routes run the same own kernels), and the same check of the metas."""
    model, _, frames, plain, scaled = detector
    rng = np.random.RandomState(8)
    queue = torch.stack([frames[0], torch.from_numpy(rng.randint(0, 256, size=(6, HS, WS, 3)).astype(np.uint8)).cuda()])[None]
    metas = [[dict(scaled[0], prev_bev_exists=False), dict(scaled[0], prev_bev_exists=True)]]
    model.eval()
    model.enable_fused_backbone()
    try:
        x, _ = ext.input_u8_scaled(queue.reshape(12, HS, WS, 3), io.identity_photometric(12), NORM_CFG['mean'], NORM_CFG['std'],
                                   NORM_CFG['to_rgb'], SCALE)
        want = model.obtain_history_bev(x.view(1, 2, 6, 3, 128, 224), metas)
        got = model.obtain_history_bev(queue, metas, img_norm_cfg=NORM_CFG, img_scale=SCALE)
        assert torch.equal(got, want) and not model.training
        with pytest.raises(ValueError, match='io.scale_img_metas'):
            model.obtain_history_bev(queue, [[plain[0], plain[0]]], img_norm_cfg=NORM_CFG, img_scale=SCALE)
    finally:
        model.enable_fused_backbone(dtype=None)
        model.train()


def test_run_test_takes_uint8_samples(detector):
    """Two samples carrying img_u8 + img_norm_cfg + img_scale instead of img through eval_loop.run_test into a RayMetrics, and
    into a RayMetrics and a VoxelMIoU together: the state words of test_loop.run_test fed the prepared img tensors (under
    the inference plan)."""
    from occnet_amd import eval_loop, test_loop
    from occnet_amd.metrics import RayMetrics
    from occnet_amd.metrics.voxel_miou import VoxelMIoU
    model, _, frames, _, scaled = detector
    model.eval()
    model.enable_fused_backbone()                # the inference configuration: both loops run the plan's kernels
    try:
        rng = np.random.RandomState(5)
        u8 = [frames, torch.from_numpy(rng.randint(0, 256, size=(1, 6, HS, WS, 3)).astype(np.uint8)).cuda()]
        imgs = [ext.input_u8_scaled(f[0], io.identity_photometric(6), NORM_CFG['mean'], NORM_CFG['std'], NORM_CFG['to_rgb'],
                                    SCALE)[0][None] for f in u8]
        occ_cls, _ = _test_outputs(model, scaled, img=imgs[0])
        X, Y, Z = occ_cls.shape[1:4]
        v = 0.4
        pc_range = [-X * v / 2, -Y * v / 2, -1.0, X * v / 2, Y * v / 2, -1.0 + Z * v]
        common = []
        for i in range(2):
            common.append(dict(token=f's{i}', img_metas=scaled,
                               lidar_origins=torch.tensor([[[0.3 * i, -0.2, 0.5], [1.0, 0.7 * i, 1.1]]]),
                               voxel_semantics=torch.from_numpy(rng.randint(0, 17, size=(1, X, Y, Z)).astype(np.uint8)).cuda(),
                               voxel_flow=torch.from_numpy(rng.randn(1, X, Y, Z, 2).astype(np.float32)).cuda()))
        want, got, both = RayMetrics(pc_range, v), RayMetrics(pc_range, v), RayMetrics(pc_range, v)
        assert test_loop.run_test(model, [dict(c, img=x) for c, x in zip(common, imgs)], metric=want) == 2
        u8_samples = [dict(c, img_u8=f, img_norm_cfg=NORM_CFG, img_scale=SCALE) for c, f in zip(common, u8)]
        assert eval_loop.run_test(model, iter(u8_samples), metric=got) == 2
        assert int(want.state[:17].sum()) > 0 and torch.equal(got.state, want.state)
        miou_img, miou_u8 = (VoxelMIoU(pc_range, v) for _ in range(2))
        assert eval_loop.run_test(model, [dict(c, img=x) for c, x in zip(common, imgs)], miou=miou_img) == 2
        assert eval_loop.run_test(model, u8_samples, metric=both, miou=miou_u8) == 2
        assert torch.equal(both.state, want.state)
        assert int(miou_img.state.sum()) > 0 and torch.equal(miou_u8.state, miou_img.state)
    finally:
        model.enable_fused_backbone(dtype=None)
        model.train()
