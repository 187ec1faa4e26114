"""not-gpu: the host side of the image-scale input (occnet_amd/io.py: random_scale_multiview, scale_img_metas, scaled_size;
the C entry's argument checks; the wrapper's refusals).  The resize is the project's own definition ("Image scale
on the device"); tests/input_scale_ref.py restates it in float64 and gives the bound."""
import ctypes

import numpy as np
import pytest

from occnet_amd import _lib, io, synthetic
from tests import input_scale_ref as S
from tests import train_input_ref as R


def _image(hs=37, ws=53):
    return (np.random.RandomState(7).randn(hs, ws, 3) * 2).astype(np.float32)


def test_scale_one_returns_the_input_bit_for_bit():
    x = _image()
    (y,), meta = io.random_scale_multiview([x], 1.0)
    assert y.dtype == np.float32 and y is not x and np.array_equal(y.view(np.uint32), x.view(np.uint32))
    assert meta['img_shape'] == [(37, 53, 3)]


@pytest.mark.parametrize('scale', S.SCALES)
def test_resize_against_the_float64_restatement(scale):
    x = _image()
    (y,), _ = io.random_scale_multiview([x], scale)
    (hd, wd), _ = S.sizes(37, 53, scale)
    ref, clamps = S.resize64(x.astype(np.float64).transpose(2, 0, 1), hd, wd)
    assert y.dtype == np.float32 and y.shape == (hd, wd, 3)
    err = float(np.abs(y.transpose(2, 0, 1) - ref).max())
    tol = 8 * 2.0 ** -23 * float(np.abs(ref).max())          # the eight rounded operations of the resize alone
    print(f"resize {scale}: max|f32 - f64| {err:.3e}  bound {tol:.3e}  clamps {clamps}")
    assert err <= tol
    if scale == 1.25:
        assert min(clamps['rows']) >= 1 and min(clamps['columns']) >= 1
    if scale == 0.5:
        assert clamps['rows'] == (0, 0) and clamps['columns'] == (0, 0)


def test_host_chain_against_the_float64_restatement():
    """E32 of every GPU case is rounding, not a disagreement about the arithmetic, and the conditioning holds."""
    for shape in S.SHAPES:
        for scale in S.SCALES:
            for norm in R.NORMS:
                c = S.case(shape, norm, scale)
                e32 = float(np.abs(c['f32'] - c['ref']).max())
                assert c['f32'].shape == c['ref'].shape == (R.NI, 3) + c['info']['padded']
                assert e32 <= 4 * 24 * 2.0 ** -23 * float(np.abs(c['ref']).max()), (shape, scale, norm, e32)      # four times the floor
                assert c['info']['min_abs_v'] >= 0.1
                hd, wd = c['info']['resized']
                assert not c['f32'][:, :, hd:].any() and not c['f32'][:, :, :, wd:].any()


def test_sizes():
    assert io.scaled_size(900, 1600, 0.8) == (720, 1280)
    assert io.scaled_size(900, 1600, 0.5) == (450, 800)
    assert io.scaled_size(900, 1600, 0.3) == (270, 480)
    assert io.scaled_size(5, 9, 0.3) == (1, 2)
    for scale in (0.1, float('nan'), float('inf'), 0.0, -0.5):
        with pytest.raises(ValueError):
            io.scaled_size(5, 9, scale)
    with pytest.raises(ValueError):
        io.random_scale_multiview([_image(5, 9)], 0.1)


def _project(meta, pts):
    """ego points (n, 3) float64 -> per view (n, 2) pixel coordinates, as point_sampling forms them"""
    p = np.concatenate([pts, np.ones((len(pts), 1))], 1)
    out = []
    for l2i in meta['lidar2img']:
        cam = (np.asarray(l2i, dtype=np.float64) @ np.asarray(meta['ego2lidar'], dtype=np.float64) @ p.T).T
        out.append(cam[:, :2] / cam[:, 2:3])
    return np.stack(out)


def test_scale_img_metas():
    geo = dict(synthetic.BASE, img_h=928, img_w=1600)
    (meta,) = synthetic.make_img_metas(geo, batch=1)
    meta['cam_intrinsic'] = [np.eye(4) * (v + 1) for v in range(6)]
    s = 0.8
    out = io.scale_img_metas(meta, s, (900, 1600))
    assert out is not meta and meta['img_shape'] == [(928, 1600, 3)] * 6           # the input is left alone
    for a, b in zip(meta['lidar2img'], out['lidar2img']):
        assert np.array_equal(b[:2], a[:2] * s) and np.array_equal(b[2:], a[2:])
    assert np.array_equal(out['ego2lidar'], meta['ego2lidar'])
    assert all(np.array_equal(a, b) for a, b in zip(out['cam_intrinsic'], meta['cam_intrinsic']))
    assert out['ori_shape'] == [(720, 1280, 3)] * 6
    assert out['img_shape'] == out['pad_shape'] == [(736, 1280, 3)] * 6
    pts = np.random.RandomState(3).uniform([-40, -40, -1], [40, 40, 5.4], size=(200, 3))
    want, got = _project(meta, pts), _project(out, pts)
    assert float(np.abs(got - s * want).max() / np.abs(want).max()) <= 1e-12
    # a frame whose scaled size needs no pad: the normalised coordinates the sampling uses do not move
    geo = dict(synthetic.BASE, img_h=128, img_w=256)
    (meta,) = synthetic.make_img_metas(geo, batch=1)
    out = io.scale_img_metas(meta, 0.5, (128, 256))
    assert out['ori_shape'] == out['img_shape'] == [(64, 128, 3)] * 6
    want = _project(meta, pts) / np.array([256.0, 128.0])
    got = _project(out, pts) / np.array([128.0, 64.0])
    assert float(np.abs(got - want).max() / np.abs(want).max()) <= 1e-12


def _header_prototypes():
    with open(_lib.INPUT_HEADER) as f:
        return _lib.prototypes(f.read())


def test_new_header_is_exported_and_bound():
    protos = _header_prototypes()
    assert sorted(protos) == ['occ_input_u8_scaled_f32']
    assert _lib.INPUT_HEADER in _lib.EXTENSION_HEADERS and set(_lib.EXTRA_HEADERS) <= set(_lib.EXTENSION_HEADERS)
    lib = _lib.lib()
    restype, params = protos['occ_input_u8_scaled_f32']
    fn = lib.occ_input_u8_scaled_f32
    assert fn.restype is restype is ctypes.c_int
    assert list(fn.argtypes) == [t for t, _ in params]
    assert [n for _, n in params] == ['x', 'records', 'out', 'n_images', 'Hs', 'Ws', 'Hd', 'Wd', 'H', 'W', 'mean', 'std', 'to_rgb',
                                      'grid_mask', 'stream']
    assert [t for t, _ in params] == [_lib.DevicePtr] * 3 + [ctypes.c_int] * 7 + [_lib.DevicePtr] * 2 + [ctypes.c_int] + \
        [_lib.DevicePtr] * 2
    main = _lib.prototypes()                 # the main header is as it was
    assert sorted(main) == _lib.declared_symbols() and not set(main) & set(protos)
    assert lib.occ_abi_version() == _lib.ABI == 3


def test_entry_validates_without_gpu():
    """occ_input_u8_scaled_f32 refuses bad arguments before any launch (no compute call is made)."""
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = ctypes.c_void_p(base)
    mean, std = (ctypes.c_float * 3)(1, 2, 3), (ctypes.c_float * 3)(1, 1, 1)

    def call(x=p, rec=p, out=p, n=1, hs=37, ws=53, hd=18, wd=26, H=32, W=32, mean=mean, std=std, gm=None):
        g = None if gm is None else (ctypes.c_int32 * 8)(*gm)
        return lib.occ_input_u8_scaled_f32(x, rec, out, n, hs, ws, hd, wd, H, W, mean, std, 1, g, null)
    for kw in (dict(x=null), dict(rec=null), dict(out=null), dict(mean=None), dict(std=None)):
        assert call(**kw) == -1 and b'null' in lib.occ_last_error(), kw
    assert call(out=ctypes.c_void_p(base + 4)) == -1 and b'aligned' in lib.occ_last_error()
    assert call(rec=ctypes.c_void_p(base + 2)) == -1 and b'aligned' in lib.occ_last_error()
    assert call(n=0) == -1 and call(hs=0) == -1 and call(ws=0) == -1 and call(n=70000) == -1
    assert call(hd=0) == -1 and b'empty dimension' in lib.occ_last_error()
    assert call(wd=0) == -1 and b'empty dimension' in lib.occ_last_error()
    assert call(H=16) == -1 and b'smaller than the resized image' in lib.occ_last_error()
    assert call(W=24) == -1 and b'smaller than the resized image' in lib.occ_last_error()
    assert call(hs=40000) == -1 and b'beyond 32768' in lib.occ_last_error()
    assert call(wd=26, W=32772, H=4, hd=4) == -1 and b'beyond 32768' in lib.occ_last_error()
    assert call(std=(ctypes.c_float * 3)(1, 0, 1)) == -1 and b'zero std' in lib.occ_last_error()
    rc = call(W=30)
    assert rc == -3 and b'multiple of 4' in lib.occ_last_error()
    with pytest.raises(_lib.OccAmdUnsupported):
        _lib.check(rc, 'input_u8_scaled')
    assert call(gm=(1, 1, 1, 0, 0, 1, 1, 1)) == -1 and b'd = 1' in lib.occ_last_error()
    assert call(gm=(1, 7, 0, 0, 0, 1, 1, 1)) == -1 and b'l = 0' in lib.occ_last_error()
    assert call(gm=(1, 7, 7, 0, 0, 1, 1, 1)) == -1 and b'l = 7' in lib.occ_last_error()
    assert call(gm=(1, 7, 3, 7, 0, 1, 1, 1)) == -1 and b'start' in lib.occ_last_error()
    assert call(gm=(1, 7, 3, 0, -1, 1, 1, 1)) == -1 and b'start' in lib.occ_last_error()
    assert b'input_u8_scaled' in lib.occ_last_error()


def test_ext_wrapper_refusals():
    import torch
    from occnet_amd import ext
    fr, ident = torch.zeros(1, 5, 9, 3, dtype=torch.uint8), io.identity_photometric(1)
    with pytest.raises(_lib.OccAmdError, match='no CPU fallback'):
        ext.input_u8_scaled(fr, ident, [0, 0, 0], [1, 1, 1], False, 0.5)
    for scale in (float('nan'), float('inf'), -float('inf'), 0.0, -0.5):
        with pytest.raises(_lib.OccAmdError, match='finite and positive'):
            ext.input_u8_scaled(fr, ident, [0, 0, 0], [1, 1, 1], False, scale)
