"""-m gpu: the fused occupancy heads + loss node (csrc/occ_heads_loss.hip, ext.OccHeadsLossFunction) against a float64
restatement in plain torch on the CPU — the two Sequential heads, F.cross_entropy(reduction='none', weight, ignore_index), the
mask / denominator rule of bricks.CrossEntropyLoss, bricks.L1Loss — then determinism, the out-of-range label rule, the autograd
contract, and the node inside BEVFormerOccHead.forward_loss and a whole training step.

Bound of the op-level checks: max|got - ref| / max|ref| <= grad_bounds.LINEAR_X3_REL for both losses and all nine gradients (the
bound of the Linear node this replaces).  Every parity case also runs today's module chain (X3Linear heads + bricks losses) on
the device against the same reference and prints both errors per tensor."""
import functools
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import autograd_contract as ac
from tests import grad_bounds as gb

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAMES = ('feat', 'w1_occ', 'b1_occ', 'w2_occ', 'b2_occ', 'w1_flow', 'b1_flow', 'w2_flow', 'b2_flow')

# shape (B, W, H, Z), classes, max_blocks, mask ('none' | 'rand' | 'tile': rows 32..63 blanked), class weights, label dtype,
# ignore_index (255 is present in the uint8 labels), reduction, incoming gradients (None: that output is left out of backward)
CASES = {
    'r60_c3':        dict(shape=(1, 5, 3, 4), ncls=3, max_blocks=0, mask='none', cw=False, ldt=torch.int64, ignore=-100,
                          reduction='mean', gos=(1.0, 1.0)),
    'r280_c18_tile': dict(shape=(2, 7, 5, 4), ncls=18, max_blocks=0, mask='tile', cw=True, ldt=torch.uint8, ignore=255,
                          reduction='mean', gos=(0.7, -1.3)),
    'r280_c18_mb1':  dict(shape=(2, 7, 5, 4), ncls=18, max_blocks=1, mask='none', cw=True, ldt=torch.int64, ignore=-100,
                          reduction='sum', gos=(1.0, 1.0)),
    'r280_c30_mb1':  dict(shape=(2, 7, 5, 4), ncls=30, max_blocks=1, mask='rand', cw=False, ldt=torch.uint8, ignore=255,
                          reduction='sum', gos=(0.7, -1.3)),
    'r1584_c30_occ': dict(shape=(1, 11, 9, 16), ncls=30, max_blocks=2, mask='rand', cw=False, ldt=torch.uint8, ignore=255,
                          reduction='mean', gos=(1.0, None)),
    'r1584_c18_flow': dict(shape=(1, 11, 9, 16), ncls=18, max_blocks=2, mask='none', cw=True, ldt=torch.int64, ignore=-100,
                           reduction='sum', gos=(None, -1.3)),
}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """CPU float32 / integer inputs of a case: features scaled so that some Softplus inputs exceed the threshold of 20 and the
    ReLU side sees both signs."""
    c = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    n, ncls = c['shape'][0] * c['shape'][1] * c['shape'][2] * c['shape'][3], c['ncls']
    feat = torch.randn(c['shape'] + (32,), generator=g) * 4.0
    params = [torch.randn(64, 32, generator=g) * 0.3, torch.randn(64, generator=g) * 0.5,
              torch.randn(ncls, 64, generator=g) * 0.2, torch.randn(ncls, generator=g) * 0.5,
              torch.randn(64, 32, generator=g) * 0.3, torch.randn(64, generator=g) * 0.5,
              torch.randn(2, 64, generator=g) * 0.2, torch.randn(2, generator=g) * 0.5]
    pre_o = feat.view(-1, 32) @ params[0].t() + params[1]
    pre_f = feat.view(-1, 32) @ params[4].t() + params[5]
    assert bool((pre_o > 20).any()) and bool((pre_o < 0).any()) and bool((pre_f > 0).any()) and bool((pre_f < 0).any())
    labels = torch.randint(0, ncls, c['shape'], generator=g)
    if c['ignore'] == 255:
        labels.view(-1)[::7] = 255
    labels = labels.to(c['ldt'])
    flow_gt = torch.randn(c['shape'] + (2,), generator=g)
    # d|f - g| / df = sign(f - g) jumps at f = g: no target within 1e-2 of its prediction, so that the gradient is defined to
    # every implementation's forward error (the float32 chain's is ~1e-5 on these magnitudes)
    f64 = F.linear(F.relu(F.linear(feat.double().view(-1, 32), params[4].double(), params[5].double())), params[6].double(),
                   params[7].double())
    near = (f64 - flow_gt.view(-1, 2).double()).abs() < 1e-2
    flow_gt.view(-1, 2)[near] -= 0.5
    mask = None
    if c['mask'] != 'none':
        mask = torch.rand(c['shape'], generator=g) > 0.3
        if c['mask'] == 'tile':
            mask.view(-1)[32:64] = False
    cw = torch.rand(ncls, generator=g) + 0.5 if c['cw'] else None
    return feat, params, labels, flow_gt, mask, cw


def _ref_losses(feat, params, labels, flow_gt, mask, cw, ignore, reduction, keep=None):
    """The restatement, in the dtype of its inputs.  keep: None, or a per-row 0 / 1 weight on the cross-entropy terms."""
    w1o, b1o, w2o, b2o, w1f, b1f, w2f, b2f = params
    x = feat.reshape(-1, 32)
    occ = F.linear(F.softplus(F.linear(x, w1o, b1o)), w2o, b2o)
    flow = F.linear(F.relu(F.linear(x, w1f, b1f)), w2f, b2f)
    ce = F.cross_entropy(occ, labels.reshape(-1).long(), weight=cw, reduction='none', ignore_index=ignore)
    if keep is not None:
        ce = ce * keep
    if mask is not None:        # bricks.CrossEntropyLoss: weight = mask, avg_factor = mask.sum()
        loss_occ = (ce * mask.reshape(-1).to(ce.dtype)).sum() / mask.sum()
    else:
        loss_occ = ce.mean() if reduction == 'mean' else ce.sum()
    l1 = (flow - flow_gt.reshape(-1, 2)).abs()
    return loss_occ, (l1.mean() if reduction == 'mean' else l1.sum())


def _backward(losses, gos):
    use = [k for k in (0, 1) if gos[k] is not None]
    torch.autograd.backward([losses[k] for k in use], [torch.as_tensor(gos[k], dtype=losses[k].dtype, device=losses[k].device)
                                                       for k in use])


@functools.lru_cache(maxsize=None)
def _reference(name):
    """float64 losses and gradients of a case, computed once."""
    c = CASES[name]
    feat, params, labels, flow_gt, mask, cw = _inputs(name)
    leaves = [t.double().requires_grad_(True) for t in [feat] + params]
    losses = _ref_losses(leaves[0], leaves[1:], labels, flow_gt.double(), mask, None if cw is None else cw.double(),
                         c['ignore'], c['reduction'])
    _backward(losses, c['gos'])
    return [l.detach() for l in losses], [l.grad for l in leaves]


def _dev(t):
    return None if t is None else t.to(DEV)


def _run_node(name):
    from occnet_amd import ext
    c = CASES[name]
    feat, params, labels, flow_gt, mask, cw = _inputs(name)
    leaves = [t.to(DEV).requires_grad_(True) for t in [feat] + params]
    losses = ext.heads_loss(*leaves, _dev(labels), _dev(flow_gt), _dev(mask), _dev(cw), c['ignore'], c['reduction'],
                            c['max_blocks'])
    _backward(losses, c['gos'])
    return [l.detach() for l in losses], [l.grad for l in leaves]


def _run_chain(name):
    """Today's modules on the device: X3Linear heads (transformer_occ.py) + bricks losses as loss_single calls them."""
    from occnet_amd.plugin.bricks import CrossEntropyLoss, L1Loss, X3Linear
    c = CASES[name]
    feat, params, labels, flow_gt, mask, cw = _inputs(name)
    ncls = c['ncls']
    pred = nn.Sequential(X3Linear(32, 64), nn.Softplus(), X3Linear(64, ncls)).to(DEV)
    flow_pred = nn.Sequential(X3Linear(32, 64), nn.ReLU(), X3Linear(64, 2)).to(DEV)
    mods = [pred[0], pred[2], flow_pred[0], flow_pred[2]]
    with torch.no_grad():
        for m, (w, b) in zip(mods, zip(params[0::2], params[1::2])):
            m.weight.copy_(w)
            m.bias.copy_(b)
    x = feat.to(DEV).requires_grad_(True)
    lo = CrossEntropyLoss(reduction=c['reduction'], class_weight=None if cw is None else cw.tolist(),
                          ignore_index=None if c['ignore'] == -100 else c['ignore'])
    lf = L1Loss(reduction=c['reduction'])
    flow, occ = flow_pred(x), pred(x)
    y = labels.to(DEV).long().reshape(-1)
    if mask is not None:
        m = mask.to(DEV).reshape(-1)
        loss_occ = lo(occ.reshape(-1, ncls), y, m, avg_factor=m.sum())
    else:
        loss_occ = lo(occ.reshape(-1, ncls), y)
    loss_flow = lf(flow.reshape(-1, 2), flow_gt.to(DEV).reshape(-1, 2))
    _backward((loss_occ, loss_flow), c['gos'])
    grads = [x.grad] + [t for m in mods for t in (m.weight.grad, m.bias.grad)]
    return [loss_occ.detach(), loss_flow.detach()], grads


def _rel(got, ref):
    scale = float(ref.abs().max())
    return float((got.detach().double().cpu() - ref).abs().max()) / scale if scale > 0 else float(got.abs().max())


@pytest.mark.parametrize("name", list(CASES))
def test_node_matches_float64_restatement(name):
    c = CASES[name]
    ref_losses, ref_grads = _reference(name)
    losses, grads = _run_node(name)
    ch_losses, ch_grads = _run_chain(name)
    rows = []
    for k, what in enumerate(('loss_occ', 'loss_flow')):
        rows.append((what, _rel(losses[k], ref_losses[k]), _rel(ch_losses[k], ref_losses[k])))
    for i, what in enumerate(NAMES):
        r = ref_grads[i]
        # a head whose loss is left out of the backward has zero gradients in the reference
        used = c['gos'][0] is not None if 1 <= i <= 4 else c['gos'][1] is not None if i >= 5 else True
        if not used:
            assert r is None or float(r.abs().max()) == 0.0
            assert float(grads[i].abs().max()) == 0.0, what
            continue
        assert grads[i].shape == r.shape
        rows.append(('d' + what, _rel(grads[i], r), _rel(ch_grads[i], r)))
    print(f"\n{name}: max|got - ref| / max|ref|      fused node    module chain")
    for what, ef, ec in rows:
        print(f"    {what:<12} {ef:12.3e} {ec:12.3e}" + ("   (> 2 x chain)" if ef > 2 * ec else ""))
    for what, ef, _ in rows:
        assert ef <= gb.LINEAR_X3_REL, (what, ef)


def _raw_call(name, fill):
    """The C ABI itself on caller-owned buffers, workspace and every output pre-filled with `fill`."""
    from occnet_amd import _lib
    from occnet_amd._lib import i32, i64, ptr, stream_ptr
    c = CASES[name]
    feat, params, labels, flow_gt, mask, cw = _inputs(name)
    feat, labels, flow_gt, mask, cw = _dev(feat), _dev(labels), _dev(flow_gt), _dev(mask), _dev(cw)
    params = [p.to(DEV) for p in params]
    lib = _lib.lib()
    n, ncls = feat.numel() // 32, c['ncls']
    nbytes = int(lib.occ_heads_loss_workspace_bytes(i64(n), i32(ncls), i32(c['max_blocks'])))
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), fill, device=DEV)
    losses = torch.full((3,), fill, device=DEV)
    code = 0 if labels.dtype == torch.uint8 else 1
    mean = 1 if c['reduction'] == 'mean' else 0
    common = [ptr(feat)] + [ptr(p) for p in params] + [ptr(labels), i32(code), ptr(flow_gt), ptr(mask), ptr(cw),
                                                       i64(c['ignore']), i32(mean)]
    tail = [ptr(ws), i64(nbytes), i64(n), i32(32), i32(64), i32(ncls), i32(c['max_blocks']), stream_ptr(feat.device)]
    assert lib.occ_heads_loss_fwd_f32(*common, ptr(losses), *tail) == 0, lib.occ_last_error()
    gos = torch.tensor([0.0 if v is None else v for v in c['gos']], device=DEV)
    ws.fill_(fill)
    outs = [torch.full_like(t, fill) for t in [feat] + params]
    assert lib.occ_heads_loss_bwd_f32(*common, ptr(gos), ptr(losses[2:]), *[ptr(t) for t in outs], *tail) == 0, \
        lib.occ_last_error()
    torch.cuda.synchronize()
    return [losses] + outs


@pytest.mark.parametrize("name", ['r280_c18_tile', 'r280_c30_mb1', 'r1584_c30_occ'])
def test_bit_identical_runs_and_every_output_written(name):
    a = _raw_call(name, 0.0)
    b = _raw_call(name, 0.0)
    n = _raw_call(name, float('nan'))
    for what, x, y, z in zip(('losses',) + NAMES, a, b, n):
        assert bool(torch.isfinite(z).all()), f"{what}: NaN pre-fill shows through"
        assert torch.equal(x, y), f"{what}: two runs differ"
        assert torch.equal(x, z), f"{what}: depends on the buffers' previous contents"
    ref_losses, ref_grads = _reference(name)
    assert _rel(a[0][0], ref_losses[0]) <= gb.LINEAR_X3_REL and _rel(a[0][1], ref_losses[1]) <= gb.LINEAR_X3_REL


def test_out_of_range_label_contributes_nothing():
    """Labels in [ncls, 254] (not ignore_index): no fault, and losses and gradients equal the reference with those rows'
    cross-entropy weight set to 0 (torch itself raises a device assert on such a label)."""
    from occnet_amd import ext
    name = 'r280_c18_tile'
    c = CASES[name]
    feat, params, labels, flow_gt, mask, cw = _inputs(name)
    labels = labels.clone()
    bad = torch.zeros(labels.numel(), dtype=torch.bool)
    bad[3::11] = True
    bad &= labels.view(-1) != 255
    labels.view(-1)[bad] = torch.arange(int(bad.sum())).to(torch.uint8) % (254 - c['ncls'] + 1) + c['ncls']
    assert int(labels.view(-1)[bad].min()) >= c['ncls'] and int(labels.view(-1)[bad].max()) <= 254 and int(bad.sum()) > 10
    leaves64 = [t.double().requires_grad_(True) for t in [feat] + params]
    safe = labels.clone()
    safe.view(-1)[bad] = 0
    ref = _ref_losses(leaves64[0], leaves64[1:], safe, flow_gt.double(), mask, cw.double(), c['ignore'], c['reduction'],
                      keep=(~bad).double())
    _backward(ref, c['gos'])
    leaves = [t.to(DEV).requires_grad_(True) for t in [feat] + params]
    got = ext.heads_loss(*leaves, _dev(labels), _dev(flow_gt), _dev(mask), _dev(cw), c['ignore'], c['reduction'])
    _backward(got, c['gos'])
    torch.cuda.synchronize()
    for k in (0, 1):
        assert _rel(got[k], ref[k].detach()) <= gb.LINEAR_X3_REL
    for what, l, r in zip(NAMES, leaves, leaves64):
        assert _rel(l.grad, r.grad) <= gb.LINEAR_X3_REL, what


def _contract_spec():
    from occnet_amd import ext
    name = 'r280_c18_tile'
    c = CASES[name]
    feat, params, labels, flow_gt, mask, cw = _inputs(name)
    dl, df, dm, dc = _dev(labels), _dev(flow_gt), _dev(mask), _dev(cw)

    def run(l):
        lo, lf = ext.heads_loss(*l, dl, df, dm, dc, c['ignore'], c['reduction'], 1)
        return lo.view(1), lf.view(1)

    def ref(l64):
        lo, lf = _ref_losses(l64[0], l64[1:], labels, flow_gt.double(), mask, cw.double(), c['ignore'], c['reduction'])
        # both outputs of the node hang on every leaf that requires grad; so do the reference's (a zero term: under a mask
        # that leaves one head without such a leaf, its loss would otherwise have no graph to run backward through)
        tie = sum(t.sum() * 0.0 for t in l64 if t.requires_grad)
        return (lo + tie).view(1), (lf + tie).view(1)

    def truth(what, got, ref_, mask_, grad_outs):
        d = float((got - ref_).abs().max()) / float(ref_.abs().max())
        assert d <= gb.LINEAR_X3_REL, f"max diff / max|ref| = {d:.3e}"

    return ac.NodeSpec("OccHeadsLoss", lambda: [t.to(DEV) for t in [feat] + params], run, ref, tuple(range(9)), truth,
                       node_name='OccHeadsLossFunction')


def test_autograd_contract():
    """Nine leaves: the full mask, each single leaf (feat alone among them), the eight parameters without feat, each head's
    four parameters.  The node is deterministic, so gradients are the same bits under every mask."""
    spec = _contract_spec()
    masks = [tuple(range(9))] + [(i,) for i in range(9)] + [tuple(range(1, 9)), (1, 2, 3, 4), (5, 6, 7, 8)]
    report = ac.check_masks(spec, masks)
    assert len(report) == len(masks) and all(v in ('full mask', 'bit-identical') for v in report.values())
    ac.check_grad_layouts(spec)
    assert ac.check_retain_graph(spec) >= 10      # nine leaves' worth of inputs + targets + the denominator, nothing larger
    _, outs = ac._forward(spec, tuple(range(9)))
    node = ac.find_node(outs[0], 'OccHeadsLossFunction')
    feat_numel = _inputs('r280_c18_tile')[0].numel()
    assert max(t.numel() for t in node.saved_tensors if t is not None) == feat_numel      # inputs only: no hidden tensor


def _graph_names_until(fn, stop):
    """Type names of the autograd nodes reachable from fn without passing through a node whose name starts with `stop`."""
    seen, names, queue = set(), [], [fn]
    while queue:
        f = queue.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.append(type(f).__name__)
        if not type(f).__name__.startswith(stop):
            queue += [nf for nf, _ in f.next_functions]
    return names


@pytest.mark.parametrize("use_mask", [False, True])
def test_head_forward_loss_matches_oracle(use_mask):
    """test_gpu_training.py::test_loss_gradients_match_oracle with the fused node: same geometry, same bounds (losses 1e-4;
    gradients 2e-3 * max|ref| + 2e-5, 5e-5 for the decoder's convolution weights — that test's comments give the reasons)."""
    from occnet_amd import synthetic
    from occnet_amd.train import synthetic_targets
    from tests.util import build_pair, small_cfg
    g = small_cfg(bev=(20, 20), num_layers=2)
    prod, ora = build_pair(g, seed=3)
    prod.use_mask = use_mask
    prod.fused_loss = True
    feats = synthetic.make_features(g, seed=3)
    metas = synthetic.make_img_metas(g)
    sem, flow, mask = synthetic_targets(g['bev_h'], g['bev_w'], g['pillar_h'], num_classes=17, batch=1, seed=0)
    lp = prod.forward_loss([f.cuda() for f in feats], metas, None, sem.cuda(), flow.cuda(), mask.cuda())
    names = _graph_names_until(lp['loss_occ'].grad_fn, 'OccHeadsLossFunction')
    assert any(n.startswith('OccHeadsLossFunction') for n in names), names
    assert not any(n.startswith('LinearX3Function') or n.startswith('LinearWgradFunction') for n in names), names
    (lp['loss_occ'] + lp['loss_flow']).backward()
    out_o = ora(feats, metas, prev_bev=None)
    lo = ora.loss(sem, flow, mask, out_o)
    if use_mask:
        # the oracle's loss() is the reference's unmasked branch only; its masked branch (bevformer_occ_head.py:183-188:
        # CrossEntropyLoss(weight = mask_camera, avg_factor = mask_camera.sum())) restated here on the oracle's logits
        ce = F.cross_entropy(out_o['occ'].reshape(-1, ora.num_classes), sem.long().reshape(-1), reduction='none')
        lo['loss_occ'] = ora.loss_occ_weight * (ce * mask.reshape(-1).float()).sum() / mask.sum()
    (lo['loss_occ'] + lo['loss_flow']).backward()
    for k in ('loss_occ', 'loss_flow'):
        print(f"{k}: hip {float(lp[k].detach()):.6f} oracle {float(lo[k].detach()):.6f}")
        assert abs(float(lp[k].detach()) - float(lo[k].detach())) < 1e-4
    po = dict(ora.named_parameters())
    checked = 0
    for name, p in prod.named_parameters():
        if p.grad is None:
            assert po[name].grad is None or float(po[name].grad.abs().max()) == 0.0, name
            continue
        ref = po[name].grad
        scale = float(ref.abs().max())
        d = float((p.grad.cpu() - ref).abs().max())
        floor = 5e-5 if name.endswith('conv.weight') and '.decoder.' in name else 2e-5
        assert d < 2e-3 * scale + floor, (name, d, scale)
        checked += 1
    assert checked > 40
    for name in ('transformer.predicter.0.weight', 'transformer.predicter.2.bias', 'transformer.flow_predicter.2.weight'):
        assert dict(prod.named_parameters())[name].grad is not None, name


def _seed(v):
    import numpy as np
    torch.manual_seed(v)        # dropout masks
    np.random.seed(v)           # GridMask


def test_two_train_steps_with_the_switch_on():
    """The reduced base model of test_gpu_training.py::test_ddp_train_step_single_rank, no process group: the first step's
    losses with the switch on against the same model, same seed, switch off; then a second step."""
    from occnet_amd import synthetic
    from occnet_amd.plugin import Config, build_model, import_plugin
    from occnet_amd.train import make_optimizer, synthetic_targets, train_step
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
    device = torch.device('cuda', 0)
    model = model.to(device).train()
    head = model.pts_bbox_head
    opt = make_optimizer(model)
    geo = dict(synthetic.BASE, img_h=128, img_w=224)
    img = synthetic.make_images(geo, batch=1, seed=0, device=device)
    metas = synthetic.make_img_metas(geo, batch=1)
    sem, flow, mask = synthetic_targets(head.bev_h, head.bev_w, head.transformer.pillar_h, num_classes=head.num_classes,
                                        device=device)
    kw = dict(return_loss=True, img_metas=metas, img=img, voxel_semantics=sem, voxel_flow=flow, mask_camera=mask)
    had = 'fused_loss' in head.__dict__
    try:
        head.fused_loss = False
        off = None
        for _ in range(2):      # the first pass lets the convolution library settle on its solvers
            _seed(5)
            off = {k: float(v.detach()) for k, v in model(**kw).items()}
        head.fused_loss = True
        before = head.bev_embedding.weight.detach().clone()
        _seed(5)
        first = {k: float(v.detach()) for k, v in train_step(model, opt, img, metas, sem, flow, mask).items()}
        missing = [n for n, p in model.named_parameters() if p.requires_grad and p.grad is None]
        assert not missing, missing
        bad = [n for n, p in model.named_parameters() if p.grad is not None and not bool(torch.isfinite(p.grad).all())]
        assert not bad, bad
        second = {k: float(v.detach()) for k, v in train_step(model, opt, img, metas, sem, flow, mask).items()}
        print("switch off:", off, "\nswitch on, step 1:", first, "\nswitch on, step 2:", second)
        for k in ('loss_occ', 'loss_flow'):
            assert abs(first[k] - off[k]) < 1e-4, (k, first[k], off[k])
            assert second[k] == second[k] and abs(second[k]) < 1e6
        assert float((head.bev_embedding.weight - before).abs().max()) > 0.0
    finally:
        if had:
            head.fused_loss = False
        else:
            head.__dict__.pop('fused_loss', None)
