"""Fused occupancy heads + loss node, everything that needs no GPU: the C ABI's argument checks and workspace sizing (they run
before any launch), the gate of BEVFormerOccHead.forward_loss, and the fallback's bit-identity on the host."""
import copy
import ctypes
import types

import pytest
import torch
import torch.nn as nn

from occnet_amd import _lib


def _aligned(n_floats=256):
    buf = (ctypes.c_float * (n_floats + 4))()
    addr = (ctypes.addressof(buf) + 15) & ~15
    return buf, ctypes.c_void_p(addr)


def test_c_abi_validates_before_any_launch():
    lib = _lib.lib()
    i64, i32 = ctypes.c_int64, ctypes.c_int
    null = ctypes.c_void_p(0)
    keep, p = _aligned()
    ws_bytes = lib.occ_heads_loss_workspace_bytes
    record = (128 * 32 + 128 + 32 * 128 + 32) * 4          # one wave's partial parameter gradients, bytes
    # backward: one record per wave, 4 waves per block, one block per 4 tiles of 32 rows up to 256 blocks (or max_blocks)
    assert ws_bytes(i64(640000), 18, 0) == 256 * 4 * record
    assert ws_bytes(i64(640000), 18, 3) == 3 * 4 * record
    assert ws_bytes(i64(60), 3, 0) == 4 * record and ws_bytes(i64(280), 30, 0) == 3 * 4 * record
    assert ws_bytes(i64(280), 31, 0) == 0 and ws_bytes(i64(0), 18, 0) == 0 and ws_bytes(i64(280), 0, 0) == 0
    assert ws_bytes(i64(280), 18, -1) == 0

    def fwd(feat=p, w=p, labels=p, dtype=1, flow=p, losses=p, ws=p, ws_n=1 << 30, n=64, C=32, hidden=64, ncls=18, mb=0,
            mean=1):
        return lib.occ_heads_loss_fwd_f32(feat, w, p, p, p, p, p, p, p, labels, i32(dtype), flow, null, null, i64(-100),
                                          i32(mean), losses, ws, i64(ws_n), i64(n), i32(C), i32(hidden), i32(ncls), i32(mb),
                                          null)

    def bwd(feat=p, gl=p, den=p, dfeat=p, dw=p, ws=p, ws_n=1 << 30, n=64, C=32, hidden=64, ncls=18, mb=0, dtype=0):
        return lib.occ_heads_loss_bwd_f32(feat, p, p, p, p, p, p, p, p, p, i32(dtype), p, null, null, i64(255), i32(1), gl,
                                          den, dfeat, dw, dw, dw, dw, dw, dw, dw, dw, ws, i64(ws_n), i64(n), i32(C),
                                          i32(hidden), i32(ncls), i32(mb), null)

    for call in (fwd, bwd):
        assert call(feat=null) == -1 and b'null pointer' in lib.occ_last_error()
        assert call(ws=null) == -1
        assert call(n=0) == -1 and b'bad dimension' in lib.occ_last_error()
        assert call(ncls=0) == -1
        assert call(dtype=2) == -1 and b'labels_dtype' in lib.occ_last_error()
        assert call(mb=-1) == -1 and b'max_blocks' in lib.occ_last_error()
        assert call(ncls=31) == -3 and b'no fused kernel' in lib.occ_last_error()
        assert call(C=16) == -3 and call(hidden=128) == -3
        assert call(ws_n=64) == -1 and b'workspace too small' in lib.occ_last_error()
        assert call(feat=ctypes.c_void_p(p.value + 4)) == -1 and b'aligned' in lib.occ_last_error()
    assert fwd(w=null) == -1 and fwd(labels=null) == -1 and fwd(flow=null) == -1 and fwd(losses=null) == -1
    assert fwd(mean=2) == -1 and b'reduction_mean' in lib.occ_last_error()
    assert bwd(gl=null) == -1 and bwd(den=null) == -1
    assert bwd(dfeat=null, dw=null) == -1 and b'no gradient requested' in lib.occ_last_error()
    del keep


def _host_head(num_classes=17, loss_occ=None):
    from occnet_amd.plugin import build_head
    from tests.util import head_cfg, randomize, small_cfg
    g = small_cfg(bev=(4, 4), feat_shapes=((2, 2), (1, 1), (1, 1), (1, 1)), num_layers=1)
    cfg = copy.deepcopy(head_cfg(g, num_classes=num_classes))
    if loss_occ is not None:
        cfg['loss_occ'].update(loss_occ)
    head = build_head(cfg)
    randomize(head, seed=1)
    return g, head.eval()


@pytest.mark.parametrize("use_mask", [False, True])
def test_host_head_with_the_switch_on_runs_todays_path_bit_for_bit(use_mask):
    """No fused node on the host: forward_loss with fused_loss = True is loss(forward(...)), the same bits.  (The encoder has no
    host path, so a fixed BEV embedding stands in for it; decoder, heads and losses are the real modules.)"""
    from occnet_amd import synthetic
    from occnet_amd.train import synthetic_targets
    g, head = _host_head()
    head.use_mask = use_mask
    bev = torch.randn(1, g['bev_h'] * g['bev_w'], g['embed_dims'], generator=torch.Generator().manual_seed(2))
    head.transformer.get_bev_features = lambda *a, **k: bev
    feats, metas = synthetic.make_features(g), synthetic.make_img_metas(g)
    sem, flow, mask = synthetic_targets(g['bev_h'], g['bev_w'], g['pillar_h'], num_classes=17)
    want = head.loss(sem, flow, mask, head(feats, metas, None))
    head.fused_loss = True
    got = head.forward_loss(feats, metas, None, sem, flow, mask)
    assert set(got) == set(want) == {'loss_occ', 'loss_flow'}
    for k in want:
        assert got[k].requires_grad and torch.equal(got[k], want[k]), k


def test_gate_refuses_what_the_node_does_not_cover():
    dev_feat = [types.SimpleNamespace(is_cuda=True, dtype=torch.float32)]       # the gate reads these two attributes only
    g, head = _host_head()
    head.fused_loss = False
    assert not head._fused_loss_ok(dev_feat)                                  # the switch is off
    head.fused_loss = True
    assert head._fused_loss_ok(dev_feat)
    assert not head._fused_loss_ok([types.SimpleNamespace(is_cuda=False, dtype=torch.float32)])
    with torch.no_grad():
        assert not head._fused_loss_ok(dev_feat)
    t = head.transformer
    softplus = t.predicter[1]
    for act in (nn.ELU(), nn.Softplus(threshold=10), nn.Softplus(beta=2)):
        t.predicter[1] = act
        assert not head._fused_loss_ok(dev_feat), act
    t.predicter[1] = softplus
    relu = t.flow_predicter[1]
    t.flow_predicter[1] = nn.LeakyReLU()
    assert not head._fused_loss_ok(dev_feat)
    t.flow_predicter[1] = relu
    assert head._fused_loss_ok(dev_feat)
    for attr, loss in (('loss_occ', head.loss_occ), ('loss_flow', head.loss_flow)):
        loss.reduction = 'none'
        assert not head._fused_loss_ok(dev_feat), attr
        loss.reduction = 'mean'
    head.loss_flow.reduction = 'sum'                                          # one reduction for both losses
    assert not head._fused_loss_ok(dev_feat)
    head.loss_occ.reduction = 'sum'
    assert head._fused_loss_ok(dev_feat)
    head.loss_flow = nn.SmoothL1Loss()
    assert not head._fused_loss_ok(dev_feat)
    _, head31 = _host_head(num_classes=31)
    head31.fused_loss = True
    assert not head31._fused_loss_ok(dev_feat)
    _, head30 = _host_head(num_classes=30)
    head30.fused_loss = True
    assert head30._fused_loss_ok(dev_feat)


def test_detector_takes_forward_loss_only_with_the_switch_on():
    from occnet_amd.plugin.bevformer_occ import BEVFormerOcc
    calls = []

    class Head(nn.Module):
        fused_loss = False

        def forward(self, *a, **k):
            calls.append('forward')
            return {}

        def loss(self, *a, **k):
            calls.append('loss')
            return {}

        def forward_loss(self, *a, **k):
            calls.append('forward_loss')
            return {}

    det = BEVFormerOcc()
    det.pts_bbox_head = Head()
    det.forward_pts_train(None, None, None, None, None, None, None)
    assert calls == ['forward', 'loss']
    det.pts_bbox_head.fused_loss = True
    det.forward_pts_train(None, None, None, None, None, None, None)
    assert calls == ['forward', 'loss', 'forward_loss']
