"""The decoder's training BatchNorm3d + ReLU entry points (csrc/bn3d_relu_train.hip) without a GPU: scratch sizing and the
argument / shape checks that run before any launch; the module switch is off unless asked for."""
import ctypes
import os
import subprocess
import sys

from occnet_amd import _lib

i64, f32 = ctypes.c_int64, ctypes.c_float
INVALID, UNSUPPORTED = -1, -3


def _buf():
    buf = (ctypes.c_float * 4096)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_partial_floats():
    lib = _lib.lib()
    q = lib.occ_bn3d_relu_train_partial_floats
    assert q.restype is ctypes.c_int64          # registered in _lib's list of int64 size queries
    assert q(i64(40000), 32) == 1024 * 64       # <= 1024 blocks of 32 rows, 32 channels x 2 sums per block
    assert q(i64(2), 32) == 64 and q(i64(33), 32) == 128
    assert q(i64(40000), 16) == 0               # C = 32 only
    assert q(i64(1), 32) == 0                   # torch raises for one value per channel too
    assert q(i64(2 ** 26), 32) == 0 and q(i64(2 ** 26 - 1), 32) == 1024 * 64     # fewer than 2^31 elements
    assert q(i64(2 ** 62), 32) == 0


def test_entry_points_validate_before_any_launch():
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    keep, p = _buf()
    stats, fwd, bwd = lib.occ_bn3d_relu_train_stats_f32, lib.occ_bn3d_relu_train_fwd_f32, lib.occ_bn3d_relu_train_bwd_f32
    # NULL pointers
    assert stats(null, p, p, p, p, f32(0.1), f32(1e-5), i64(64), 32, null) == INVALID
    assert stats(p, null, p, p, p, f32(0.1), f32(1e-5), i64(64), 32, null) == INVALID
    assert stats(p, p, null, p, p, f32(0.1), f32(1e-5), i64(64), 32, null) == INVALID
    assert stats(p, p, p, p, null, f32(0.1), f32(1e-5), i64(64), 32, null) == INVALID      # one running buffer without the other
    assert b'running' in lib.occ_last_error()
    for k in range(5):
        a = [p] * 5
        a[k] = null
        assert fwd(*a, 1, 4, 2, 2, 32, i64(512), i64(256), i64(128), null) == INVALID
    for k in (0, 4, 5, 6, 7, 8, 9):       # grad_out, y, mean_rstd, gamma, beta, partial, grad_gamma_beta
        a = [p, i64(512), i64(256), i64(128), p, p, p, p, p, p, p, p]
        a[k] = null
        assert bwd(*a, 1, 4, 2, 2, 32, null) == INVALID
    assert fwd(p, p, p, p, p, 0, 4, 2, 2, 32, i64(512), i64(256), i64(128), null) == INVALID
    # C = 16, one row, 2^31 elements
    assert stats(p, p, p, null, null, f32(0.1), f32(1e-5), i64(64), 16, null) == UNSUPPORTED
    assert b'C = 32' in lib.occ_last_error()
    assert stats(p, p, p, null, null, f32(0.1), f32(1e-5), i64(1), 32, null) == UNSUPPORTED
    assert stats(p, p, p, null, null, f32(0.1), f32(1e-5), i64(2 ** 26), 32, null) == UNSUPPORTED
    assert fwd(p, p, p, p, p, 1, 4, 2, 2, 16, i64(256), i64(128), i64(64), null) == UNSUPPORTED
    assert fwd(p, p, p, p, p, 1, 1, 1, 1, 32, i64(32), i64(32), i64(32), null) == UNSUPPORTED
    assert fwd(p, p, p, p, p, 8, 32, 512, 512, 32, i64(1), i64(1), i64(1), null) == UNSUPPORTED
    assert bwd(p, i64(256), i64(128), i64(64), p, p, p, p, p, p, p, p, 1, 4, 2, 2, 16, null) == UNSUPPORTED
    assert bwd(p, i64(32), i64(32), i64(32), p, p, p, p, p, p, null, null, 1, 1, 1, 1, 32, null) == UNSUPPORTED
    assert bwd(p, i64(1), i64(1), i64(1), p, p, p, p, p, p, p, p, 8, 32, 512, 512, 32, null) == UNSUPPORTED
    del keep


def test_switch_defaults_to_off():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("from occnet_amd.plugin.transformer_occ import TransformerOcc as T; "
            "print(int(T.train_decoder_fused_bn))")
    for value, want in ((None, "0"), ("1", "1"), ("0", "0")):
        env = {k: v for k, v in os.environ.items() if k != "OCC_TRAIN_DECODER_BN"}
        if value is not None:
            env["OCC_TRAIN_DECODER_BN"] = value
        res = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        assert res.stdout.strip().splitlines()[-1] == want, (value, res.stdout)
