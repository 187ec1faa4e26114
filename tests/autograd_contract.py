"""Contract checks for hand-written autograd nodes (a plain module: tests import it, pytest collects nothing here).

A node is described by a `NodeSpec`: how to make its leaf tensors, how to build its output(s) from them, the same operation
restated in plain torch ops (run in float64), which leaves are differentiable, and the bound its parity test already
asserts.  The checks below then hold for ANY node:

  check_masks          for each requires_grad mask over the differentiable leaves: every masked leaf's gradient agrees with the
                       float64 reference differentiated UNDER THE SAME MASK ('truth'); masked leaves have a finite gradient
                       that is not identically zero where the reference's is not, unmasked leaves have none ('presence');
                       the forward output and, for deterministic nodes, each gradient are the same bits under every mask
                       ('mask_independence').
  check_grad_layouts   the incoming gradient as a contiguous tensor, as a stride-0 expansion (what sum().backward() sends), as
                       a permuted view and as a column slice of a wider tensor: the same gradients ('layout').
  check_retain_graph   backward twice over a retained graph: the same gradients ('retain'), and neither the saved tensors
                       nor the output have changed ('saved').

Every failure raises ContractViolation, whose `.check` names the check that found it."""
import itertools

import torch


class ContractViolation(AssertionError):
    def __init__(self, check, message):
        super().__init__(f"[{check}] {message}")
        self.check = check


class NodeSpec:
    """make_leaves() -> list of fresh leaf tensors (None for an absent optional input; same values on every call);
    run(leaves) -> output tensor or tuple of tensors of the node under test;
    ref(leaves64) -> the same from plain torch ops (leaves64: float64 copies on `ref_device`, integer leaves as they are);
    diff: indices of the differentiable leaves;
    truth(what, got, ref, mask, grad_outs): raise / assert unless `got` is within the node's bound of `ref` (float64); what
        is ('grad', leaf index) or ('out', output index); mask and grad_outs (None: the default incoming gradients) let a
        bound that is relative to another implementation's error run that implementation under the same conditions;
    deterministic: the backward's gradients are bit-reproducible; node_name: prefix of the grad_fn's type name."""

    def __init__(self, name, make_leaves, run, ref, diff, truth, deterministic=True, ref_device='cpu', node_name=None,
                 before_run=None):
        self.name, self.make_leaves, self.run, self.ref = name, make_leaves, run, ref
        self.diff, self.truth, self.deterministic = tuple(diff), truth, deterministic
        self.ref_device, self.node_name, self.before_run = ref_device, node_name, before_run
        self._grad_out = self._out_dtypes = None


def all_masks(diff):
    """Every non-empty subset of `diff`, the full mask first."""
    diff = tuple(diff)
    masks = [diff]
    for n in range(1, len(diff)):
        masks += list(itertools.combinations(diff, n))
    return masks


def _tuple(out):
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def _forward(spec, mask):
    leaves = spec.make_leaves()
    for i in spec.diff:
        leaves[i] = leaves[i].detach().requires_grad_(i in mask)
    if spec.before_run is not None:
        spec.before_run()
    outs = _tuple(spec.run(leaves))
    spec._out_dtypes = [o.dtype for o in outs]
    return leaves, outs


def default_grad_outs(spec, outs):
    """One fixed incoming gradient per output (seeded; the outputs' shape, dtype and device)."""
    if spec._grad_out is None:
        g = torch.Generator().manual_seed(1234)
        spec._grad_out = [torch.randn(o.shape, generator=g, dtype=torch.float64) for o in outs]
    return [go.to(device=o.device, dtype=o.dtype) for go, o in zip(spec._grad_out, outs)]


def run_node(spec, mask, grad_outs=None, use_outputs=None):
    """-> (outputs, {leaf index: gradient or None}) of the node under `mask`; use_outputs: indices of the outputs that get a
    gradient (the others are left out of the backward call, as a loss that ignores them does)."""
    leaves, outs = _forward(spec, mask)
    gos = default_grad_outs(spec, outs) if grad_outs is None else grad_outs
    use = range(len(outs)) if use_outputs is None else use_outputs
    torch.autograd.backward([outs[k] for k in use], [gos[k] for k in use])
    return [o.detach() for o in outs], {i: leaves[i].grad for i in spec.diff}


def run_reference(spec, mask, grad_outs=None, use_outputs=None):
    """The float64 reference under the same mask -> (outputs, {leaf index: gradient or None})."""
    leaves = spec.make_leaves()
    l64 = []
    for i, t in enumerate(leaves):
        if t is not None and t.is_floating_point():
            t = t.detach().to(device=spec.ref_device, dtype=torch.float64).requires_grad_(i in mask)
        elif t is not None:
            t = t.to(spec.ref_device)
        l64.append(t)
    outs = _tuple(spec.ref(l64))
    if grad_outs is None:       # the node's incoming gradient: the default one rounded to the node's output dtype
        dts = spec._out_dtypes or [torch.float64] * len(outs)
        grad_outs = [g.to(dt) for g, dt in zip(default_grad_outs(spec, outs), dts)]
    gos = grad_outs
    gos = [g.detach().to(device=o.device, dtype=torch.float64) for g, o in zip(gos, outs)]
    use = range(len(outs)) if use_outputs is None else use_outputs
    torch.autograd.backward([outs[k] for k in use], [gos[k] for k in use])
    return [o.detach() for o in outs], {i: l64[i].grad for i in spec.diff}


def _truth(spec, what, got, ref, mask, grad_outs=None):
    if got.shape != ref.shape:
        raise ContractViolation('truth', f"{spec.name} {what} mask {mask}: shape {tuple(got.shape)} vs {tuple(ref.shape)}")
    try:
        spec.truth(what, got.detach().to(device=ref.device, dtype=torch.float64), ref, mask, grad_outs)
    except ContractViolation:
        raise
    except AssertionError as e:
        raise ContractViolation('truth', f"{spec.name} {what} mask {mask}: {e}") from e


def _presence(spec, mask, grads, ref_grads):
    for i in spec.diff:
        g, r = grads[i], ref_grads[i]
        if i not in mask:
            if g is not None:
                raise ContractViolation('presence', f"{spec.name} leaf {i} is outside mask {mask} but has a gradient")
            continue
        if r is None:
            raise AssertionError(f"{spec.name}: the reference gives leaf {i} no gradient under mask {mask}")
        if g is None:
            raise ContractViolation('presence', f"{spec.name} leaf {i} is in mask {mask} and has no gradient")
        if not bool(torch.isfinite(g).all()):
            raise ContractViolation('presence', f"{spec.name} leaf {i} mask {mask}: non-finite gradient")
        if float(r.abs().max()) > 0.0 and float(g.abs().max()) == 0.0:
            raise ContractViolation('presence', f"{spec.name} leaf {i} mask {mask}: all-zero gradient, the reference's is not")


def _check_one_mask(spec, mask, full, base, use_outputs):
    outs, grads = run_node(spec, mask, use_outputs=use_outputs)
    ref_outs, ref_grads = run_reference(spec, mask, use_outputs=use_outputs)
    _presence(spec, mask, grads, ref_grads)
    if mask == full:
        for k, (o, r) in enumerate(zip(outs, ref_outs)):
            _truth(spec, ('out', k), o, r, mask)
    for i in mask:
        _truth(spec, ('grad', i), grads[i], ref_grads[i], mask)
    if base is None:
        return outs, grads
    for k, (o, b) in enumerate(zip(outs, base[0])):
        if not _bits_equal(o, b):
            raise ContractViolation('mask_independence', f"{spec.name} output {k} under mask {mask} differs from the "
                                    f"full mask's: max diff {float((o.double() - b.double()).abs().max()):.3e}")
    if spec.deterministic:
        for i in mask:
            if not _bits_equal(grads[i], base[1][i]):
                d = float((grads[i].double() - base[1][i].double()).abs().max())
                raise ContractViolation('mask_independence', f"{spec.name} leaf {i}: gradient under mask {mask} is not "
                                        f"the full mask's bits (max diff {d:.3e})")
    return outs, grads


def check_masks(spec, masks=None, use_outputs=None):
    """Truth, presence and mask independence over `masks` (default: every non-empty subset of spec.diff); the full mask
    always runs, first.  Every mask is run even after one has failed: the ContractViolation raised at the end lists them all
    (`.violations`: [(mask, ContractViolation)]; `.check`: the first one's).
    -> {mask: 'full mask' | 'bit-identical' | 'reference bound only'} for the report."""
    masks = [tuple(m) for m in (all_masks(spec.diff) if masks is None else masks)]
    full = tuple(spec.diff)
    if full not in masks:
        masks = [full] + masks
    masks.sort(key=lambda m: m != full)
    report, base, bad = {}, None, []
    for mask in masks:
        try:
            res = _check_one_mask(spec, mask, full, base, use_outputs)
        except ContractViolation as e:
            bad.append((mask, e))
            if mask == full:
                break       # nothing to compare the other masks with
            continue
        if base is None:
            base = res
        report[mask] = 'full mask' if mask == full else 'bit-identical' if spec.deterministic else 'reference bound only'
    if bad:
        err = ContractViolation(bad[0][1].check, f"{len(bad)} of {len(masks)} masks fail:\n" + "\n".join(str(e) for _, e in bad))
        err.violations = bad
        raise err
    return report


def grad_layouts(g):
    """Tensors equal to g in value, laid out differently: contiguous, permuted (dims reversed in memory), a column slice of a
    wider tensor; 4-D: channels_last as well (contiguous then is channels-first)."""
    g = g.contiguous()
    rev = tuple(reversed(range(g.dim())))
    wide = torch.zeros(g.shape[:-1] + (g.shape[-1] + 8,), dtype=g.dtype, device=g.device)
    wide[..., 3:3 + g.shape[-1]] = g
    out = {'contiguous': g, 'permuted': g.permute(rev).contiguous().permute(rev), 'sliced': wide[..., 3:3 + g.shape[-1]]}
    if g.dim() == 4:
        out['channels_last'] = g.contiguous(memory_format=torch.channels_last)
    return out


def _same_grads(spec, check, label, grads, base, mask):
    for i in mask:
        if grads[i] is None:
            raise ContractViolation(check, f"{spec.name} leaf {i}: no gradient ({label})")
        if spec.deterministic:
            if not _bits_equal(grads[i], base[i]):
                d = float((grads[i].double() - base[i].double()).abs().max())
                raise ContractViolation(check, f"{spec.name} leaf {i}: gradient differs ({label}), max diff {d:.3e}")


def check_grad_layouts(spec):
    """Full mask.  Deterministic nodes: bit-identical gradients for every layout of the same incoming gradient; the others:
    every layout's gradients within the node's bound of the reference."""
    full = tuple(spec.diff)
    _, outs = _forward(spec, full)
    gos = default_grad_outs(spec, outs)
    variants = {}
    for k, g in enumerate(gos):
        for name, t in grad_layouts(g).items():
            variants.setdefault(name, list(gos))[k] = t
    const = [torch.full((), 0.37 * (k + 1), dtype=g.dtype, device=g.device).expand(g.shape) for k, g in enumerate(gos)]
    groups = [(variants.pop('contiguous'), variants), ([c.contiguous() for c in const], {'expanded (stride 0)': const})]
    for base_gos, others in groups:
        _, base = run_node(spec, full, grad_outs=base_gos)
        _, ref_grads = run_reference(spec, full, grad_outs=base_gos)
        for i in full:
            _truth(spec, ('grad', i), base[i], ref_grads[i], full, base_gos)
        for name, v in others.items():
            assert all(torch.equal(a, b) for a, b in zip(v, base_gos))
            try:
                _, grads = run_node(spec, full, grad_outs=v)
            except RuntimeError as e:       # a backward that assumes its layout (view() of a non-contiguous gradient, ...)
                raise ContractViolation('layout', f"{spec.name}: backward fails on a {name} gradient: {e}") from e
            _same_grads(spec, 'layout', name, grads, base, full)
            if not spec.deterministic:
                try:
                    for i in full:
                        _truth(spec, ('grad', i), grads[i], ref_grads[i], full, base_gos)
                except ContractViolation as e:
                    raise ContractViolation('layout', f"{name}: {e}") from e


def find_node(out, name):
    """The autograd node behind `out` whose type name starts with `name` (breadth first from out.grad_fn)."""
    seen, queue = set(), [out.grad_fn]
    while queue:
        fn = queue.pop(0)
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if name is None or type(fn).__name__.startswith(name):
            return fn
        queue += [nf for nf, _ in fn.next_functions]
    raise AssertionError(f"no {name} node behind the output")


def check_retain_graph(spec):
    """Full mask: backward(retain_graph=True) twice -> the same gradients; saved tensors and outputs unchanged."""
    full = tuple(spec.diff)
    leaves, outs = _forward(spec, full)
    gos = default_grad_outs(spec, outs)
    node = find_node(outs[0], spec.node_name)
    saved = getattr(node, 'saved_tensors', ())
    snap = [None if t is None else t.detach().clone() for t in saved]
    out_snap = [o.detach().clone() for o in outs]
    runs = []
    for _ in range(2):
        for i in full:
            leaves[i].grad = None
        torch.autograd.backward(list(outs), list(gos), retain_graph=True)
        runs.append({i: None if leaves[i].grad is None else leaves[i].grad.detach().clone() for i in full})
    _same_grads(spec, 'retain', 'second backward over the retained graph', runs[1], runs[0], full)
    _, ref_grads = run_reference(spec, full)
    try:
        for i in full:
            _truth(spec, ('grad', i), runs[1][i], ref_grads[i], full)
    except ContractViolation as e:
        raise ContractViolation('retain', f"second backward: {e}") from e
    for k, (t, s) in enumerate(zip(getattr(node, 'saved_tensors', ()), snap)):
        if s is not None and not _bits_equal(t.detach(), s):
            raise ContractViolation('saved', f"{spec.name}: saved tensor {k} changed during backward")
    for k, (o, s) in enumerate(zip(outs, out_snap)):
        if not _bits_equal(o.detach(), s):
            raise ContractViolation('saved', f"{spec.name}: output {k} changed during backward")
    return len([s for s in snap if s is not None])


# ---- ConvBNActFunction: the masks the sweep runs and the restatement its truth is built on

CONV_BN_ACT_LEAVES = ('x', 'weight', 'gamma', 'beta', 'conv_bias', 'residual')


def conv_bn_act_masks(present):
    """present: indices (into CONV_BN_ACT_LEAVES) of the leaves a case has.  Up to four: every non-empty subset.  More: every
    single leaf, every pair drawn from {weight, gamma, beta}, all-but-one, and all."""
    present = tuple(present)
    if len(present) <= 4:
        return all_masks(present)
    masks = [present] + [(i,) for i in present]
    masks += [m for m in itertools.combinations([i for i in (1, 2, 3) if i in present], 2)]
    masks += [tuple(j for j in present if j != i) for i in present]
    return list(dict.fromkeys(masks))


def folded_conv_bn(x, weight, gamma, beta, conv_bias, running_mean, running_var, eps, stride, padding):
    """occnet_amd.plugin.backbone.conv_bn_folded on bare tensors (it reads attributes only, so two attribute bags stand in for
    the Conv2d and the eval-mode BatchNorm2d); without a norm (gamma None) the biased convolution itself."""
    import types
    from occnet_amd.plugin.backbone import conv_bn_folded
    if gamma is None:
        return torch.nn.functional.conv2d(x, weight, conv_bias, stride, padding)
    conv = types.SimpleNamespace(weight=weight, bias=conv_bias, stride=stride, padding=padding, dilation=(1, 1), groups=1)
    bn = types.SimpleNamespace(weight=gamma, bias=beta, running_mean=running_mean, running_var=running_var, eps=eps)
    return conv_bn_folded(x, conv, bn)
