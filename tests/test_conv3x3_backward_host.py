"""not-gpu: the 3x3 convolution's weight-gradient entry points size their workspace and reject bad arguments before any
launch; the Python wrappers refuse what the kernels cannot take; the training switch is off unless the environment sets it;
the data gradient's weight transform is the flipped, transposed weight."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from occnet_amd import _lib, ext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wgrad_workspace_and_argument_checks_without_gpu():
    lib = _lib.lib()
    ws = lib.occ_conv3x3_wgrad_workspace_bytes
    one = 9 * 128 * 256 * 4                                       # one f32 partial of the (Cout, 3, 3, Cin) output
    n = ws(2, 12, 20, 256, 128, 1, 0)
    assert n > 0 and n % one == 0
    assert ws(2, 12, 20, 256, 128, 1, 7) == 7 * one               # a positive `splits` is honoured
    assert ws(2, 12, 20, 256, 128, 2, 5) == 5 * one
    n2 = ws(2, 12, 20, 256, 128, 2, 0)
    assert n2 > 0 and n2 % one == 0
    assert ws(2, 12, 20, 48, 128, 1, 0) == 0                      # Cin % 32
    assert ws(2, 12, 20, 256, 40, 1, 0) == 0                      # Cout % 32
    assert ws(2, 12, 20, 256, 4096, 1, 0) == 0                    # Cout > 2048
    assert ws(2, 12, 20, 256, 128, 3, 0) == 0                     # stride 3
    assert ws(2, 12, 20, 256, 128, 1, -1) == 0                    # negative splits
    assert ws(0, 12, 20, 256, 128, 1, 0) == 0                     # empty batch

    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = lib.occ_conv3x3_wgrad_nhwc_bf16
    for args in ((null, p, p, 0, p), (p, null, p, 0, p), (p, p, null, 1, p), (p, p, p, 0, null)):
        assert f(*args, 2, 12, 20, 256, 128, 1, 0, null) == -1
        assert b'null' in lib.occ_last_error()
    assert f(p, p, p, 0, p, 2, 12, 20, 48, 128, 1, 0, null) == -3         # Cin % 32
    assert f(p, p, p, 0, p, 2, 12, 20, 256, 40, 1, 0, null) == -3         # Cout % 32
    assert f(p, p, p, 0, p, 2, 12, 20, 256, 4096, 1, 0, null) == -3       # Cout > 2048
    assert f(p, p, p, 1, p, 2, 12, 20, 256, 128, 3, 0, null) == -3        # stride 3
    assert b'stride' in lib.occ_last_error()
    with pytest.raises(_lib.OccAmdUnsupported):
        _lib.check(-3, 'conv3x3_wgrad')
    assert f(p, p, p, 0, p, 2, 12, 20, 256, 128, 1, -1, null) == -1       # negative splits
    assert b'splits' in lib.occ_last_error()
    assert f(p, p, p, 0, p, 0, 12, 20, 256, 128, 1, 0, null) == -1        # empty batch


def test_python_wrappers_refuse_what_the_kernels_cannot_take():
    cl = torch.channels_last
    g = torch.zeros(2, 128, 12, 20, dtype=torch.bfloat16).contiguous(memory_format=cl)
    x = torch.zeros(2, 256, 12, 20, dtype=torch.bfloat16).contiguous(memory_format=cl)
    w = torch.zeros(128, 256, 3, 3, dtype=torch.bfloat16)
    for gg, xx in ((g, x),                                          # host tensors
                   (g.float(), x.float()),                          # fp32
                   (g.contiguous(), x.contiguous())):               # NCHW
        assert not gg.is_cuda
        with pytest.raises(_lib.OccAmdUnsupported):
            ext.conv3x3_wgrad_nhwc(gg, xx)
        with pytest.raises(_lib.OccAmdUnsupported):
            ext.conv3x3_wgrad_nhwc(gg, xx, stride=2, out_dtype=torch.bfloat16, splits=3)
        with pytest.raises(_lib.OccAmdUnsupported):
            ext.conv3x3_dgrad_nhwc(gg, w)


def test_the_switch_is_off_unless_the_environment_sets_it():
    code = ("from occnet_amd.plugin.backbone import ConvBNActFunction; "
            "print('own_conv3x3_backward', ConvBNActFunction.own_conv3x3_backward, "
            "'own_conv1x1_backward', ConvBNActFunction.own_conv1x1_backward)")
    env = {k: v for k, v in os.environ.items() if k not in ("OCC_TRAIN_CONV3X3_BWD", "OCC_TRAIN_CONV1X1_BWD")}
    off = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert off.returncode == 0, off.stderr
    assert "own_conv3x3_backward False" in off.stdout
    on = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, OCC_TRAIN_CONV3X3_BWD="1"), capture_output=True,
                        text=True)
    assert on.returncode == 0, on.stderr
    assert "own_conv3x3_backward True" in on.stdout
    assert "own_conv1x1_backward False" in on.stdout                # the two switches are independent


def test_dgrad_weight_is_the_flipped_transposed_weight():
    """conv2d(g, conv3x3_dgrad_weight(W), padding=1) is the input gradient of a stride-1, pad-1 conv2d with W (float64, a
    4 -> 6 channel weight on a 5 x 7 map), element by element Wd[i, o, ky, kx] = W[o, i, 2 - ky, 2 - kx]."""
    gen = torch.Generator().manual_seed(3)
    W = torch.randn(6, 4, 3, 3, generator=gen, dtype=torch.float64)
    g = torch.randn(2, 6, 5, 7, generator=gen, dtype=torch.float64)
    Wd = ext.conv3x3_dgrad_weight(W)
    assert Wd.shape == (4, 6, 3, 3)
    for ky in range(3):
        for kx in range(3):
            assert torch.equal(Wd[:, :, ky, kx], W[:, :, 2 - ky, 2 - kx].t())
    want = torch.nn.grad.conv2d_input((2, 4, 5, 7), W, g, stride=1, padding=1)
    got = torch.nn.functional.conv2d(g, Wd, padding=1)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    with pytest.raises(_lib.OccAmdError):
        ext.conv3x3_dgrad_weight(torch.zeros(6, 4, 1, 1))
