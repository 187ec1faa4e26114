"""not-gpu: the fused TSA backward's C ABI (occ_tsa_fused_backward_f32 / _workspace_bytes) checks its arguments before any
launch and sizes its scratch as documented, and ext.tsa_fused_backward / ext.TSAFusedFunction refuse bad inputs up front."""
import ctypes

import pytest
import torch

from occnet_amd import _lib, ext
from tests.tsa_ref import CASE_IDS, CASES

i64 = ctypes.c_int64


def _align(x):
    return (x + 255) & ~255


def _ws_bytes(B, Nq, M=8, P=4):
    """Restatement of tsa_bwd_ws_layout: the msda backward's binned layout for B*2 value entries of Nq pixels and Nq queries
    at one level, then the location plane and the attention plane."""
    Bv, S, L = B * 2, Nq, 1
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
    n = Bv * Nq * M * P
    off_loc = _align(nbytes)
    off_attn = _align(off_loc + n * 8)
    return off_attn + n * 4


def test_symbols_declared_and_exported():
    lib = _lib.lib()
    for s in ('occ_tsa_fused_backward_f32', 'occ_tsa_fused_backward_workspace_bytes'):
        assert s in _lib.declared_symbols()
        assert hasattr(lib, s)
    assert lib.occ_abi_version() == 3


@pytest.mark.parametrize("B,H,W", [c[:3] for c in CASES] + [(1, 200, 200)], ids=CASE_IDS + ["B1_200x200"])
def test_workspace_size(B, H, W):
    lib = _lib.lib()
    got = lib.occ_tsa_fused_backward_workspace_bytes(B, H * W, H, W, 8, 32, 4)
    assert got > 0
    assert got == _ws_bytes(B, H * W)
    assert ext.tsa_fused_backward_workspace_bytes(B, H * W, H, W, 8, 32, 4) == got


def test_workspace_size_zero_without_a_kernel():
    f = _lib.lib().occ_tsa_fused_backward_workspace_bytes
    assert f(1, 168, 12, 14, 8, 32, 4) > 0
    assert f(1, 168, 12, 14, 4, 32, 4) == 0           # M != 8
    assert f(1, 168, 12, 14, 8, 64, 4) == 0           # D != 32
    assert f(1, 168, 12, 14, 8, 32, 8) == 0           # P != 4
    assert f(0, 168, 12, 14, 8, 32, 4) == 0
    assert f(1, 70, 12, 14, 8, 32, 4) == 0            # a query band: the row pipeline has no backward
    assert f(1, 1500 * 1500, 1500, 1500, 8, 32, 4) == 0      # a map beyond the buffer loads' offset range


def _call(p, null, *, ptrs=None, dims=(1, 168, 12, 14, 8, 32, 4), strides=(128, 64, 128, 64), bt=168 * 256,
          ws_bytes=1 << 40):
    lib = _lib.lib()
    a = [p] * 11 if ptrs is None else ptrs
    value, offs, logits, ref_2d, gout, shapes, lstart, gvalue, goffs, glogits, ws = a
    so, sl, sgo, sgl = strides
    return lib.occ_tsa_fused_backward_f32(value, i64(bt), offs, i64(so), logits, i64(sl), ref_2d, gout, shapes, lstart,
                                          gvalue, goffs, i64(sgo), glogits, i64(sgl), *dims, ws, i64(ws_bytes), null)


def test_argument_checks_before_any_launch():
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    base = (ctypes.addressof(buf) + 63) & ~63
    p = ctypes.c_void_p(base)                                                # 64-byte aligned, never dereferenced
    for i in (0, 1, 2, 3, 4, 5, 6, 10):                                      # every input pointer and the workspace
        ptrs = [p] * 11
        ptrs[i] = null
        assert _call(p, null, ptrs=ptrs) == -1 and b'null' in lib.occ_last_error(), i
    # outputs: grad_value, or grad_offs AND grad_logits, may be NULL (not wanted) — not one of the pair, not all three
    for nulls in ((8,), (9,), (7, 8, 9), (7, 8), (7, 9)):
        ptrs = [p] * 11
        for i in nulls:
            ptrs[i] = null
        assert _call(p, null, ptrs=ptrs) == -1 and b'null' in lib.occ_last_error(), nulls
    assert _call(p, null, dims=(1, 168, 12, 14, 8, 64, 4)) == -3                                # D = 64
    assert b'D=64' in lib.occ_last_error()
    with pytest.raises(_lib.OccAmdUnsupported):
        _lib.check(-3, 'tsa_fused_backward')
    assert _call(p, null, dims=(1, 168, 12, 14, 4, 32, 4)) == -3                                # M = 4
    assert _call(p, null, dims=(1, 168, 12, 14, 8, 32, 8)) == -3                                # P = 8
    assert b'P=8' in lib.occ_last_error()
    assert _call(p, null, dims=(1, 70, 12, 14, 8, 32, 4)) == -3                                 # a query band
    assert _call(p, null, dims=(0, 168, 12, 14, 8, 32, 4)) == -1                                # B = 0
    assert _call(p, null, dims=(1, 168, 0, 14, 8, 32, 4)) == -1                                 # bev_h = 0
    assert _call(p, null, dims=(1, 1500 * 1500, 1500, 1500, 8, 32, 4)) == -1                    # map >= kOobOffset bytes
    assert b'too large' in lib.occ_last_error()
    assert _call(p, null, bt=-4) == -1                                                          # negative value stride
    assert _call(p, null, strides=(127, 64, 128, 64)) == -1                                     # offs row too short
    assert _call(p, null, strides=(128, 63, 128, 64)) == -1
    assert _call(p, null, strides=(128, 64, 126, 64)) == -1
    assert _call(p, null, strides=(128, 64, 128, 63)) == -1                                     # grad_logits row too short
    assert b'row strides' in lib.occ_last_error()
    assert _call(p, null, strides=(129, 64, 128, 64)) == -1 and b'even' in lib.occ_last_error() # odd offs stride
    assert _call(p, null, strides=(128, 64, 129, 64)) == -1 and b'even' in lib.occ_last_error() # odd grad_offs stride
    p4, p8 = ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 8)
    for i, bad, word in ((1, p4, b'8-byte'), (8, p4, b'8-byte'), (3, p4, b'ref_2d'), (0, p8, b'16-byte'),
                         (4, p8, b'16-byte'), (7, p8, b'16-byte')):
        ptrs = [p] * 11
        ptrs[i] = bad
        assert _call(p, null, ptrs=ptrs) == -1 and word in lib.occ_last_error(), i
    assert _call(p, null, bt=168 * 256 + 2) == -1 and b'16-byte' in lib.occ_last_error()        # value stride % 4
    need = _ws_bytes(1, 168)
    aligned = ctypes.c_void_p(1 << 20)                                       # never dereferenced: the check fails first
    assert _call(p, null, ptrs=[p] * 10 + [aligned], ws_bytes=need - 1) == -1
    assert b'workspace too small' in lib.occ_last_error()
    assert _call(p, null, ptrs=[p] * 10 + [ctypes.c_void_p((1 << 20) + 16)], ws_bytes=need) == -1    # not 256-byte aligned
    assert b'256-byte' in lib.occ_last_error()


def test_python_validation_before_any_launch():
    v = torch.zeros(2, 168, 8, 32)
    with pytest.raises(_lib.OccAmdError, match="device"):
        ext.tsa_fused_backward(v, torch.zeros(1, 168, 128), torch.zeros(1, 168, 64), torch.zeros(2, 168, 1, 2),
                               torch.zeros(1, 168, 256), 12, 14, 8, 4)
    # the autograd node refuses shapes without a backward kernel, and row bands, before it runs anything
    with pytest.raises(_lib.OccAmdUnsupported):
        ext.TSAFusedFunction.apply(torch.zeros(2, 168, 8, 32), torch.zeros(1, 168, 8 * 2 * 8 * 2),
                                   torch.zeros(1, 168, 8 * 2 * 8), torch.zeros(2, 168, 1, 2), 12, 14, 8, 8)
    with pytest.raises(_lib.OccAmdUnsupported):
        ext.TSAFusedFunction.apply(torch.zeros(2, 168, 8, 64), torch.zeros(1, 168, 128), torch.zeros(1, 168, 64),
                                   torch.zeros(2, 168, 1, 2), 12, 14, 8, 4)
    with pytest.raises(_lib.OccAmdUnsupported, match="value_rows"):
        ext.TSAFusedFunction.apply(torch.zeros(2, 168, 8, 32), torch.zeros(1, 28, 128), torch.zeros(1, 28, 64),
                                   torch.zeros(2, 28, 1, 2), 12, 14, 8, 4, False, None, 168)
