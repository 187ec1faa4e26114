"""not-gpu: the fused SCA backward's C ABI (occ_sca_fused_backward_f32 / _workspace_bytes) checks its arguments before any
launch, sizes its scratch as documented, and ext.sca_fused_backward / ext.SCAFusedFunction refuse bad inputs up front."""
import ctypes

import pytest
import torch

from occnet_amd import _lib, ext

i64 = ctypes.c_int64


def _align(x):
    return (x + 255) & ~255


def _ws_bytes(B, NC, S, M, L, P, Nq):
    """Restatement of sca_bwd_ws_layout: the msda backward's binned layout for B*NC value entries of Nq queries, then the
    softmax / camera-count plane and the normalised-offset plane."""
    Bv = B * NC
    n_items = Bv * Nq * M
    bins_per_bm = S // 32 + L + 1
    n_bins = Bv * M * bins_per_bm
    max_items = 4 * n_items * L * P
    off_cnt = _align(n_items)
    off_cur = off_cnt + _align((n_bins + 1) * 4)
    off_work = off_cur + _align((n_bins + 1) * 4)
    work_cap = n_bins + max_items // 2048 + 1
    off_items = off_work + _align((work_cap + 1) * 16)
    max_split = max_items // 2048 + 1
    off_meta = _align(off_items + max_items * 12)
    off_tiles = _align(off_meta + max_split * 8)
    off_aux = _align(off_tiles + max_split * (32 * 32 + 32) * 8)
    nbytes = off_aux + 3 * 1024 * 4
    n = B * Nq * M * L * P
    off_aw = _align(nbytes)
    off_oxy = _align(off_aw + n * 4)
    return off_oxy + n * 8


def _lib_ws():
    lib = _lib.lib()
    return lib


def test_symbols_declared_and_exported():
    lib = _lib.lib()
    for s in ('occ_sca_fused_backward_f32', 'occ_sca_fused_backward_workspace_bytes'):
        assert s in _lib.declared_symbols()
        assert hasattr(lib, s)
    assert lib.occ_abi_version() == 3


@pytest.mark.parametrize("B,NC,S,L,P,Nq", [(1, 6, 1957, 4, 8, 400), (2, 6, 1825, 2, 8, 1600), (1, 1, 1450, 1, 8, 7),
                                           (1, 6, 30825, 4, 4, 40000)])
def test_workspace_size_arithmetic(B, NC, S, L, P, Nq):
    lib = _lib_ws()
    assert lib.occ_sca_fused_backward_workspace_bytes(B, NC, S, 8, 32, L, P, Nq) == _ws_bytes(B, NC, S, 8, L, P, Nq)
    assert ext.sca_fused_backward_workspace_bytes(B, NC, S, 8, 32, L, P, Nq) == _ws_bytes(B, NC, S, 8, L, P, Nq)


def test_workspace_size_zero_without_a_kernel():
    lib = _lib_ws()
    assert lib.occ_sca_fused_backward_workspace_bytes(1, 6, 1957, 8, 64, 4, 8, 400) == 0      # D != 32
    assert lib.occ_sca_fused_backward_workspace_bytes(1, 6, 1957, 4, 32, 4, 8, 400) == 0      # M != 8
    assert lib.occ_sca_fused_backward_workspace_bytes(1, 6, 1957, 8, 32, 3, 8, 400) == 0      # (L, P) = (3, 8)
    assert lib.occ_sca_fused_backward_workspace_bytes(1, 6, 1957, 8, 32, 4, 2, 400) == 0      # (L, P) = (4, 2)
    assert lib.occ_sca_fused_backward_workspace_bytes(0, 6, 1957, 8, 32, 4, 8, 400) == 0
    assert lib.occ_sca_fused_backward_workspace_bytes(1, 33, 1957, 8, 32, 4, 8, 400) == 0
    # a largest level whose bins overflow the binning pass's LDS histogram
    assert lib.occ_sca_fused_backward_workspace_bytes(1, 6, 400000, 8, 32, 4, 8, 400) == 0


def _call(p, null, *, ptrs=None, dims=(1, 6, 1957, 8, 32, 4, 8, 4, 400), strides=(512, 256, 512, 256),
          ws_bytes=1 << 40):
    lib = _lib.lib()
    a = [p] * 12 if ptrs is None else ptrs
    value, shapes, lstart, offs, logits, ref_cam, vis, gslots, gvalue, goffs, glogits, ws = a
    so, sl, sgo, sgl = strides
    return lib.occ_sca_fused_backward_f32(value, shapes, lstart, offs, i64(so), logits, i64(sl), ref_cam, vis, gslots,
                                          gvalue, goffs, i64(sgo), glogits, i64(sgl), *dims, ws, i64(ws_bytes), null)


def test_argument_checks_before_any_launch():
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 4)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    for i in range(12):                                                    # every pointer argument
        ptrs = [p] * 12
        ptrs[i] = null
        assert _call(p, null, ptrs=ptrs) == -1 and b'null' in lib.occ_last_error(), i
    assert _call(p, null, dims=(1, 6, 1957, 8, 64, 4, 8, 4, 400)) == -3                      # D = 64
    assert b'D=64' in lib.occ_last_error()
    with pytest.raises(_lib.OccAmdUnsupported):
        _lib.check(-3, 'sca_fused_backward')
    assert _call(p, null, dims=(1, 6, 1957, 4, 32, 4, 8, 4, 400)) == -3                      # M = 4
    assert _call(p, null, dims=(1, 6, 1957, 8, 32, 3, 8, 4, 400)) == -3                      # (L, P) = (3, 8)
    assert b'L=3 P=8' in lib.occ_last_error()
    assert _call(p, null, dims=(1, 6, 1957, 8, 32, 4, 2, 2, 400)) == -3                      # (L, P) = (4, 2)
    assert _call(p, null, dims=(1, 6, 1957, 8, 32, 4, 8, 3, 400)) == -1                      # Z does not divide P
    assert _call(p, null, dims=(0, 6, 1957, 8, 32, 4, 8, 4, 400)) == -1                      # B = 0
    assert _call(p, null, dims=(1, 33, 1957, 8, 32, 4, 8, 4, 400)) == -1                     # 33 cameras
    assert _call(p, null, strides=(511, 256, 512, 256)) == -1                                # offs row too short
    assert _call(p, null, strides=(512, 256, 512, 255)) == -1                                # grad_logits row too short
    assert b'row strides' in lib.occ_last_error()
    need = _ws_bytes(1, 6, 1957, 8, 4, 8, 400)
    aligned = ctypes.c_void_p(1 << 20)                                      # never dereferenced: the check fails first
    ptrs = [p] * 11 + [aligned]
    assert _call(p, null, ptrs=ptrs, ws_bytes=need - 1) == -1
    assert b'workspace too small' in lib.occ_last_error()
    ptrs = [p] * 11 + [ctypes.c_void_p((1 << 20) + 16)]
    assert _call(p, null, ptrs=ptrs, ws_bytes=need) == -1                   # not 256-byte aligned


def test_python_validation_before_any_launch():
    v = torch.zeros(6, 1957, 8, 32)
    with pytest.raises(TypeError):
        ext.sca_fused_backward(None, None, None, None, None, None, None, None, 8, 4, 8)
    with pytest.raises(_lib.OccAmdError, match="device"):
        ext.sca_fused_backward(v, torch.zeros(4, 2, dtype=torch.int64), torch.zeros(4, dtype=torch.int64),
                               torch.zeros(1, 10, 512), torch.zeros(1, 10, 256), torch.zeros(6, 1, 10, 4, 2),
                               torch.zeros(1, 10, dtype=torch.int32), torch.zeros(1, 10, 256), 8, 4, 8)
    # the autograd node refuses a shape without a backward kernel before it runs anything (the caller falls back)
    with pytest.raises(_lib.OccAmdUnsupported):
        ext.SCAFusedFunction.apply(torch.zeros(6, 1957, 8, 32), torch.zeros(1, 10, 8 * 3 * 8 * 2),
                                   torch.zeros(1, 10, 8 * 3 * 8), torch.zeros(6, 1, 10, 4, 2),
                                   torch.zeros(1, 10, dtype=torch.int32), None, None, 8, 3, 8)
