"""not-gpu: the differentiable ray renderer's host side — the float64 restatement (tests/dvr_render_ref.py) against central
differences and against the oracle's hard caster, the new header's binding and argument checks, the wrapper's refusals, and
the opt-in wiring of RayDepthLoss into the head."""
import ctypes
import os

import numpy as np
import pytest
import torch

from occnet_amd import _lib
from tests import dvr_render_ref as R
from tests.test_gpu_dvr import _case


def test_analytic_gradient_against_central_differences():
    """d exp_d / d sigma of the restatement's three backward loops is the true derivative: 4x6x8, 50 rays, h = 1e-6,
    1e-6 absolute on every visited voxel."""
    rng = np.random.default_rng(0)
    grid = rng.uniform(0, 0.8, (4, 6, 8)).astype(np.float32).astype(np.float64)   # float64 copies of float32 values, then nudged
    dims = np.array([8, 6, 4], dtype=np.float32)
    worst, checked = 0.0, 0
    for _ in range(50):
        o = (rng.random(3).astype(np.float32) * dims)
        e = ((rng.random(3).astype(np.float32) * 3 - 1) * dims)
        r = R.render_ray(grid, o, e, 0)
        assert r is not None and r['entered']
        h = 1e-6
        for k, (x, y, z) in enumerate(r['path']):
            gp, gm = grid.copy(), grid.copy()
            gp[z, y, x] += h
            gm[z, y, x] -= h
            num = (R.render_ray(gp, o, e, 0)['exp_d'] - R.render_ray(gm, o, e, 0)['exp_d']) / (2 * h)
            worst = max(worst, abs(num - r['dd'][k]))
            checked += 1
    print(f"analytic vs central difference: {checked} voxels, max |diff| {worst:.3e}")
    assert checked > 200 and worst <= 1e-6


@pytest.mark.parametrize("name,args", [("small", (1, 1, 1, 4, 6, 8, 300, 0.3)), ("sparse", (2, 1, 1, 16, 50, 50, 1000, 0.02))])
def test_restatement_is_pinned_to_the_oracle_traversal(name, args):
    """With sigma = 1e6 * occupancy the expected depth is the hard caster's: float32(exp_d) and gt_d equal the oracle's "train"
    phase on every ray the restatement enters (rays whose first occupied voxel is crossed over less than 1e-4 are skipped: at
    most 1 %)."""
    from oracle import ray_metrics_ref as oref
    try:
        oref.dvr_lib()
    except FileNotFoundError:
        pytest.skip("oracle/_build/libdvr_ref.so not built (make -C oracle)")
    seed, N, T, Z, Y, X, M, occ = args
    sigma, origin, points, tindex = _case(seed, N, T, Z, Y, X, M, occ)
    pred, gt, _ = oref.render_forward(sigma, origin, points, tindex, "train")
    ref = R.render((sigma * 1e6).numpy(), origin.numpy(), points.numpy(), tindex.numpy(), "l1")
    entered = skipped = 0
    worst = 0.0
    for (n, c), r in ref['rays'].items():
        if not r['entered']:
            continue
        entered += 1
        first = next((i for i, s in enumerate(r['sigma']) if s > 0), None)
        if first is not None and r['dt'][first] < 1e-4:
            skipped += 1
            continue
        a, b = np.float32(r['exp_d']), float(pred[n, c])
        worst = max(worst, abs(float(a) - b) / max(abs(b), 1e-30))
        assert float(np.float32(r['gt_d'])) == float(gt[n, c]), (n, c)
        assert float(a) == b, (n, c, float(a), b)
    print(f"{name}: {entered} rays entered, {skipped} skipped, max relative difference {worst:.3e}")
    assert entered > M // 2 and skipped <= 0.01 * entered


def _protos():
    with open(_lib.DVR_HEADER) as f:
        return _lib.prototypes(f.read())


def test_new_header_is_bound():
    protos = _protos()
    assert sorted(protos) == ['occ_dvr_render_f32']
    assert _lib.DVR_HEADER in _lib.EXTENSION_HEADERS
    lib = _lib.lib()
    restype, params = protos['occ_dvr_render_f32']
    fn = lib.occ_dvr_render_f32
    assert fn.restype is restype is ctypes.c_int
    assert list(fn.argtypes) == [t for t, _ in params] == [_lib.DevicePtr] * 7 + [ctypes.c_int] * 8 + [_lib.DevicePtr]
    assert [n for _, n in params] == ['sigma', 'origin', 'points', 'tindex', 'pred_dist', 'gt_dist', 'grad_sigma', 'N', 'T', 'Z',
                                      'Y', 'X', 'M', 'point_stride', 'loss_type', 'stream']
    main = _lib.prototypes()                 # the main header is as it was
    assert sorted(main) == _lib.declared_symbols() and not set(main) & set(protos)
    assert lib.occ_abi_version() == _lib.ABI == 3


def test_entry_validates_without_gpu():
    """occ_dvr_render_f32 refuses bad arguments before any device call."""
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))

    def call(ptrs=(p,) * 7, dims=(1, 1, 2, 2, 2, 4), stride=3, loss=0):
        return lib.occ_dvr_render_f32(*ptrs, *dims, stride, loss, null)
    for k in range(7):
        assert call(ptrs=tuple(null if i == k else p for i in range(7))) == -1 and b'null' in lib.occ_last_error(), k
    assert call(loss=3) == -1 and b'loss_type' in lib.occ_last_error()
    assert call(loss=-1) == -1 and b'loss_type' in lib.occ_last_error()
    assert call(stride=2) == -1 and b'3 coordinates' in lib.occ_last_error()
    for k in range(6):
        assert call(dims=tuple(0 if i == k else v for i, v in enumerate((1, 1, 2, 2, 2, 4)))) == -1, k
        assert b'bad dimension' in lib.occ_last_error()
    big = 2 ** 31 - 1
    assert call(dims=(60000, big, big, big, big, 4)) == -1 and b'too large' in lib.occ_last_error()
    assert call(dims=(70000, 1, 2, 2, 2, 4)) == -1 and b'65535' in lib.occ_last_error()
    assert b'dvr_render' in lib.occ_last_error()


def test_ext_wrapper_refusals():
    from occnet_amd import ext
    s, o, p, t = torch.zeros(1, 1, 2, 2, 2), torch.zeros(1, 1, 3), torch.zeros(1, 4, 3), torch.zeros(1, 4)
    for name in ("l1", "l2", "absrel", "bce"):
        with pytest.raises(_lib.OccAmdError, match='no CPU fallback'):
            ext.dvr_render(s, o, p, t, name)
    for name in ("huber", "L1", "", None):
        with pytest.raises(_lib.OccAmdError, match='UNKNOWN LOSS TYPE'):
            ext.dvr_render(s, o, p, t, name)


def test_ray_depth_loss_builds_through_the_registry():
    from occnet_amd.plugin import LOSSES, build_loss
    from occnet_amd.plugin.ray_depth_loss import RayDepthLoss
    assert LOSSES.get('RayDepthLoss') is RayDepthLoss
    m = build_loss(dict(type='RayDepthLoss'))
    assert (m.loss, m.loss_weight, m.free_id, m.voxel_size) == ('l1', 1.0, None, 0.4)
    assert m.pc_range == [-40.0, -40.0, -1.0, 40.0, 40.0, 5.4] and not m.state_dict()
    m = build_loss(dict(type='RayDepthLoss', loss='absrel', loss_weight=0.25, free_id=16, voxel_size=1.6))
    assert (m.loss, m.loss_weight, m.free_id, m.voxel_size) == ('absrel', 0.25, 16, 1.6)
    with pytest.raises(ValueError):
        build_loss(dict(type='RayDepthLoss', loss='bce'))
    with pytest.raises(ValueError, match='voxel_size'):
        m._check_grid(200, 200, 16)
    m._check_grid(50, 50, 4)
    # density rule and layout: sigma[b, 0, z, y, x] = -log softmax(occ[b, x, y, z])[free]
    occ = torch.randn(2, 5, 4, 3, 17, generator=torch.Generator().manual_seed(0))
    sigma = m.density(occ)
    want = -torch.log_softmax(occ.double(), -1)[..., 16].permute(0, 3, 2, 1)[:, None]
    assert tuple(sigma.shape) == (2, 1, 3, 4, 5) and float((sigma - want).abs().max()) < 1e-5 and float(sigma.min()) >= 0


def _tiny_head(**extra):
    from occnet_amd.plugin import Config, build_head, import_plugin
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = Config.fromfile(os.path.join(root, 'configs', 'occ_tiny_50x50x4.py'))
    import_plugin(cfg)
    head_cfg = dict(cfg.model['pts_bbox_head'])
    head_cfg.update(extra)
    torch.manual_seed(0)
    return build_head(head_cfg)


def test_head_without_loss_depth_is_unchanged():
    """loss_depth=None: the same state_dict keys and loss() keys as a head whose config has no such key; configured, the module
    takes the head's geometry, adds no parameter, closes the fused route and asks for lidar_origins."""
    absent, none = _tiny_head(), _tiny_head(loss_depth=None)
    assert absent.loss_depth is None and none.loss_depth is None
    assert list(absent.state_dict()) == list(none.state_dict())
    B, X, Y, Z, C = 1, 50, 50, 4, absent.num_classes
    g = torch.Generator().manual_seed(1)
    preds = dict(occ=torch.randn(B, X, Y, Z, C, generator=g), flow=torch.randn(B, X, Y, Z, 2, generator=g))
    sem = torch.randint(0, C, (B, X, Y, Z), generator=g)
    flow = torch.randn(B, X, Y, Z, 2, generator=g)
    a, b = absent.loss(sem, flow, None, preds), none.loss(sem, flow, None, preds)
    assert sorted(a) == sorted(b) == ['loss_flow', 'loss_occ']
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert sorted(none.loss(sem, flow, None, preds, lidar_origins=torch.zeros(1, 1, 3))) == ['loss_flow', 'loss_occ']

    depth = _tiny_head(loss_depth=dict(type='RayDepthLoss', loss='l1', loss_weight=0.5))
    ld = depth.loss_depth
    assert list(depth.state_dict()) == list(absent.state_dict())
    assert (ld.loss_weight, ld.free_id, ld.pc_range) == (0.5, C - 1, [float(v) for v in depth.pc_range])
    assert abs(ld.voxel_size - 1.6) < 1e-12
    with pytest.raises(ValueError, match='lidar_origins'):
        depth.loss(sem, flow, None, preds)
    depth.fused_loss = True
    assert not depth._fused_loss_ok([torch.zeros(1)])
