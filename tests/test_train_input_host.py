"""not-gpu: the host side of the uint8 training input (occnet_amd/io.py: sample_photometric, photometric_distort;
GridMask.sample_params / mask_from_params; the C entry's argument checks).

tests/golden/train_input.npz was written by tools_dev/gen_train_input_golden.py from the reference's own
PhotoMetricDistortionMultiViewImage -> NormalizeMultiviewImage -> PadMultiViewImage (transform_3d.py, run in place).
Both sides are float32 numpy making the same statements, so the comparison is bit for bit."""
import ctypes
import os

import numpy as np
import pytest

from occnet_amd import _lib, io
from occnet_amd.plugin.grid_mask import GridMask
from tests import train_input_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_input.npz')


def _host_chain(z):
    np.random.seed(int(z['seed']))
    rec = io.sample_photometric(len(z['frames']))
    imgs = io.photometric_distort(list(z['frames']), rec)
    imgs, _ = io.normalize_multiview(imgs, z['mean'], z['std'], bool(z['to_rgb']))
    imgs, meta = io.pad_multiview(imgs, size_divisor=32)
    return rec, np.stack(imgs)


def test_host_chain_reproduces_the_reference_run_bit_for_bit():
    z = np.load(GOLDEN)
    assert z['frames'].shape == (6, 33, 50, 3) and z['frames'].dtype == np.uint8 and z['out'].shape == (6, 64, 64, 3)
    rec, got = _host_chain(z)
    assert rec.dtype == np.float32 and rec.shape == (6, 8)
    # the seed draws something in every column: the comparison exercises every stage
    ident = io.identity_photometric(6)
    assert all((rec[:, c] != ident[:, c]).any() for c in range(5)) and (rec[:, 5:] != ident[:, 5:]).any()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), z['out'].view(np.uint32))
    assert not z['out'][:, 33:].any() and not z['out'][:, :, 50:].any()


def test_host_chain_equals_the_reference_class_run_live():
    """The same comparison against the reference's class executed now, where its tree is present."""
    from oracle import refshim
    if not os.path.isdir(refshim.REF_ROOT):
        pytest.skip('reference tree absent')
    from tools_dev import gen_train_input_golden as gen
    t3d = gen.reference_module()
    z = np.load(GOLDEN)
    want = gen.reference_run(t3d, z['frames'], z['mean'], z['std'], bool(z['to_rgb']), int(z['seed']))
    state_ref = np.random.get_state()[1].copy()
    _, got = _host_chain(z)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np.random.get_state()[1], state_ref)         # the same number of draws
    assert np.array_equal(want.view(np.uint32), z['out'].view(np.uint32))      # the committed fixture is this run
    assert np.array_equal(gen.make_frames(), z['frames'])


def test_identity_records_are_a_no_op_up_to_the_hsv_round_trip():
    fr = R.frames(5, 9)
    out = io.photometric_distort(list(fr), io.identity_photometric(len(fr)))
    # grey pixels come back exactly; the others to the round trip's rounding
    grey = (fr[..., 0] == fr[..., 1]) & (fr[..., 1] == fr[..., 2])
    assert grey.any() and np.array_equal(np.stack(out)[grey], fr.astype(np.float32)[grey])
    assert np.abs(np.stack(out) - fr).max() < 1e-3


def test_float32_chain_against_the_float64_restatement():
    """E32 of the decision set is rounding, not a disagreement about the arithmetic; the conditioning holds; every
    branch the GPU test relies on is taken."""
    for shape in R.SHAPES:
        for norm in R.NORMS:
            c = R.case(shape, norm)
            info = c['info']
            e32 = float(np.abs(c['f32'] - c['ref']).max())
            assert e32 <= 64 * 2.0 ** -23 * float(np.abs(c['ref']).max()), (shape, norm, e32)
            assert info['min_abs_v'] >= 0.1
            assert info['wrap_over'] > 0 and info['wrap_under'] > 0 and info['grey'] > 0 and info['negative_v'] > 0
            assert info['sectors'] == [0, 1, 2, 3, 4, 5] and min(info['ties']) > 0
            assert len(np.unique(c['frames'])) == 256
    rec = R.RECORDS
    assert (np.abs(rec[:, 0] - np.round(rec[:, 0]))[rec[:, 0] != 0] >= 0.25).all()
    assert sorted(tuple(int(v) for v in p) for p in rec[:, 5:]) == sorted(
        [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)])
    ident = io.PHOTOMETRIC_IDENTITY
    for c in range(5):
        assert (rec[:, c] == ident[c]).any() and (rec[:, c] != ident[c]).any()


def _module(**kw):
    args = dict(use_h=True, use_w=True, rotate=1, offset=False, ratio=0.5, mode=1, prob=0.7)
    args.update(kw)
    return GridMask(**args).train()


def test_sample_params_consumes_the_rng_as_forward_does():
    import torch
    applied = 0
    for seed in range(50):
        for training in (True, False):
            gm = _module().train(training)
            np.random.seed(seed)
            gm(torch.zeros(1, 3, 33, 50))
            want = np.random.get_state()[1].copy()
            np.random.seed(seed)
            p = gm.sample_params(33, 50)
            assert np.array_equal(np.random.get_state()[1], want), seed
            assert training or p is None
            applied += p is not None
    assert 20 < applied < 50            # prob 0.7: both outcomes occur


@pytest.mark.parametrize('hw', [(5, 9), (33, 50), (64, 64), (928, 1600)])
def test_mask_from_params_equals_make_mask(hw):
    h, w = hw
    for seed in range(50):
        gm = _module(mode=seed % 2, use_h=seed % 3 != 1, use_w=seed % 3 != 2, prob=1.0)
        np.random.seed(seed)
        np.random.rand()                 # forward's apply draw, which sample_params makes too
        want = gm.make_mask(h, w)
        np.random.seed(seed)
        p = gm.sample_params(h, w)
        got = GridMask.mask_from_params(h, w, *p, use_h=gm.use_h, use_w=gm.use_w, mode=gm.mode)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)), (hw, seed, p)
    if h <= 64:      # the independent loop form of the GPU tests' reference agrees as well
        for name, g in R.grid_cases(*R.padded(h, w)).items():
            if g is not None:
                H, W = R.padded(h, w)
                assert np.array_equal(GridMask.mask_from_params(H, W, *g[:4], bool(g[4]), bool(g[5]), g[6]), R.mask64(H, W, g))


def test_train_input_entry_validates_without_gpu():
    """occ_train_input_u8_f32 refuses bad arguments before any launch (no compute call is made)."""
    lib = _lib.lib()
    assert 'occ_train_input_u8_f32' in _lib.declared_symbols()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = ctypes.c_void_p(base)
    mean, std = (ctypes.c_float * 3)(1, 2, 3), (ctypes.c_float * 3)(1, 1, 1)

    def call(x=p, rec=p, out=p, n=1, hs=5, ws=9, H=32, W=32, mean=mean, std=std, gm=None):
        g = None if gm is None else (ctypes.c_int32 * 8)(*gm)
        return lib.occ_train_input_u8_f32(x, rec, out, n, hs, ws, H, W, mean, std, 1, g, null)
    for kw in (dict(x=null), dict(rec=null), dict(out=null), dict(mean=None), dict(std=None)):
        assert call(**kw) == -1 and b'null' in lib.occ_last_error(), kw
    assert call(out=ctypes.c_void_p(base + 4)) == -1 and b'aligned' in lib.occ_last_error()
    assert call(rec=ctypes.c_void_p(base + 2)) == -1 and b'aligned' in lib.occ_last_error()
    assert call(n=0) == -1 and call(hs=0) == -1 and call(n=70000) == -1
    assert call(H=4) == -1 and b'smaller than the frames' in lib.occ_last_error()
    assert call(W=8) == -1 and b'smaller than the frames' in lib.occ_last_error()
    assert call(std=(ctypes.c_float * 3)(1, 0, 1)) == -1 and b'zero std' in lib.occ_last_error()
    rc = call(W=30)
    assert rc == -3 and b'multiple of 4' in lib.occ_last_error()
    with pytest.raises(_lib.OccAmdUnsupported):
        _lib.check(rc, 'train_input_u8')
    assert call(gm=(1, 1, 1, 0, 0, 1, 1, 1)) == -1 and b'd = 1' in lib.occ_last_error()
    assert call(gm=(1, 7, 0, 0, 0, 1, 1, 1)) == -1 and b'l = 0' in lib.occ_last_error()
    assert call(gm=(1, 7, 7, 0, 0, 1, 1, 1)) == -1 and b'l = 7' in lib.occ_last_error()
    assert call(gm=(1, 7, 3, 7, 0, 1, 1, 1)) == -1 and b'start' in lib.occ_last_error()
    assert call(gm=(1, 7, 3, 0, -1, 1, 1, 1)) == -1 and b'start' in lib.occ_last_error()
    assert lib.occ_abi_version() == 3


def test_ext_wrapper_refuses_host_frames():
    import torch
    from occnet_amd import ext
    with pytest.raises(_lib.OccAmdError, match='no CPU fallback'):
        ext.train_input_u8(torch.zeros(1, 5, 9, 3, dtype=torch.uint8), io.identity_photometric(1), [0, 0, 0], [1, 1, 1], False)
