"""Image backbone + neck named by the occ configs (`ResNet`, `FPN`), restated on stock torch.nn.

Out of the hot path's kernel scope ("backbone/neck stay stock PyTorch-ROCm
(MIOpen), no custom kernels"); they exist so `build_model(cfg.model)` works and end-to-end samples/s
(images -> voxels) can be measured.  Module/parameter names follow mmdet's (`conv1`, `bn1`,
`layer{1..4}.{i}.{conv,bn}{1,2,3}`, `downsample.{0,1}`; `lateral_convs.{i}.conv`, `fpn_convs.{i}.conv`)
so a reference checkpoint's `img_backbone.*` / `img_neck.*` keys load.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import cache_epoch, derived, ext
from .backbone_plan import FusedInferenceBackbone, own_conv_kind
from .bricks import BaseModule, ConvModule
from .registry import BACKBONES, NECKS


def conv_bn_folded(x, conv, bn):
    """conv -> eval-mode BatchNorm as ONE convolution with autograd intact: y = conv(x, W * s) + t with
    s = gamma / sqrt(running_var + eps), t = beta - running_mean * s.  Identical function and identical gradients for
    W, gamma and beta (they flow through the small weight-side products), but no BatchNorm kernel ever touches the
    activation: the reference trains its ResNet with `norm_eval=True` (projects/configs/bevformer/
    bevformer_base_occ.py:55), and torch's eval-mode BN backward costs two passes over every activation
    (batch_norm_backward_reduce + elementwise: 19 ms of the 137 ms training step on MI355X)."""
    # the statistics are frozen (eval mode): 1/sqrt(var + eps) and mean/sqrt(var + eps) are constants, cached per
    # BatchNorm until a buffer is written (three small launches per convolution instead of six, fewer in backward)
    rstd, mean_rstd = _bn_fold_constants(bn)
    s = bn.weight * rstd
    w = conv.weight * s.view(-1, 1, 1, 1)
    b = torch.addcmul(bn.bias, bn.weight, mean_rstd, value=-1.0)
    if conv.bias is not None:
        b = b + conv.bias * s
    return F.conv2d(x, w, b, conv.stride, conv.padding, conv.dilation, conv.groups)


def _bn_fold_constants(bn):
    """(1 / sqrt(var + eps), mean / sqrt(var + eps)) of an eval-mode BatchNorm, cached until a buffer is written."""
    def build():
        with torch.no_grad():
            rstd = torch.rsqrt(bn.running_var + bn.eps)
            return rstd, bn.running_mean * rstd
    return derived.owned(bn, '_occ_fold').get((bn.running_mean, bn.running_var), build)


class ConvBNActFunction(torch.autograd.Function):
    """conv -> eval-mode BatchNorm -> (+ residual) -> (ReLU) as ONE autograd node on bf16 channels_last activations: the
    training step's form of the inference plan's fused convolutions (the reference trains its ResNet with `norm_eval=True`,
    projects/configs/bevformer/bevformer_base_occ.py:55, under DDP: P/bevformer/apis/mmdet_train.py:71-79).
    Forward: the BatchNorm is folded into the weights (conv_bn_folded's arithmetic) and the convolution runs on this
    repository's 1x1 / 3x3 NHWC kernels with bias, residual and ReLU in their epilogues (other shapes: MIOpen + ONE fused
    tail launch) — under torch.autocast the same chain costs a convolution, a bias add, a residual add and a clamp, three
    more passes over the activation.  Backward: ONE pass makes the ReLU-masked gradient and the bias gradient
    (ext.bias_act_bwd_nhwc; ATen: threshold_backward + a bf16 column reduction + an add at the residual join), MIOpen's data /
    weight gradients follow, and the fold's chain rule gives the gradients of W, gamma and beta.  Same function and the same
    gradients as conv_bn_folded up to bf16 rounding (the tail adds in fp32 and rounds once instead of three times).
    own_conv1x1_backward (opt-in, OCC_TRAIN_CONV1X1_BWD=1): the nodes whose forward ran conv1x1_nhwc take their weight
    gradient from ext.conv1x1_wgrad_nhwc and, at stride 1, their data gradient from ext.conv1x1_dgrad_nhwc instead of MIOpen.
    own_conv3x3_backward (opt-in, OCC_TRAIN_CONV3X3_BWD=1, independent of the 1x1 switch): the nodes whose forward ran
    conv3x3_nhwc take their weight gradient from ext.conv3x3_wgrad_nhwc and, at stride 1, their data gradient from
    ext.conv3x3_dgrad_nhwc (the forward kernel on the flipped, transposed weight); the data gradient at stride 2, and at
    stride 1 where Cin is no multiple of 128 (the forward kernel needs that of its output channels), stays on ATen."""

    own_conv1x1_backward = os.environ.get("OCC_TRAIN_CONV1X1_BWD", "0") == "1"
    own_conv3x3_backward = os.environ.get("OCC_TRAIN_CONV3X3_BWD", "0") == "1"

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, rstd, mean_rstd, conv_bias, residual, stride, padding, relu):
        O, I = weight.shape[:2]
        cl = torch.channels_last
        w16 = None
        one_launch = (gamma is not None and conv_bias is None and weight.dtype == torch.float32 and weight.is_contiguous()
                      and all(t.dtype == torch.float32 and t.is_contiguous() for t in (gamma, beta, rstd, mean_rstd)))
        if one_launch:
            wf, w16, b = ext.conv_bn_fold_fwd(weight, gamma, beta, rstd, mean_rstd)      # the whole fold: one launch
        elif gamma is not None:
            s = gamma * rstd
            wf = weight * s.view(-1, 1, 1, 1)
            b = torch.addcmul(beta, gamma, mean_rstd, value=-1.0)
            if conv_bias is not None:
                b = b + conv_bias * s
        else:
            wf = weight
            b = conv_bias if conv_bias is not None else weight.new_zeros(O)
        wf, b = wf.float(), b.float().contiguous()
        x16 = x if (x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=cl)) else \
            x.to(torch.bfloat16).contiguous(memory_format=cl)
        r16 = None
        if residual is not None:
            r16 = residual if (residual.dtype == torch.bfloat16 and residual.is_contiguous(memory_format=cl)) else \
                residual.to(torch.bfloat16).contiguous(memory_format=cl)
        if w16 is None:
            w16 = wf.to(torch.bfloat16).contiguous(memory_format=cl)
        stride, padding = tuple(stride), tuple(padding)
        # the node's convolutions are dense (dilation 1, groups 1: _plain_conv); the 3x3 kernel has no residual input
        route = own_conv_kind(weight.shape, stride, padding)
        if route == '3x3' and r16 is not None:
            route = None
        if route == '1x1':
            y = ext.conv1x1_nhwc(x16, ext.conv1x1_pack_weight(wf.reshape(O, I)), b, residual=r16, relu=relu, stride=stride[0])
        elif route == '3x3':
            y = ext.conv3x3_nhwc(x16, ext.conv3x3_pack_weight(wf.contiguous()), b, O, relu=relu, stride=stride[0])
        else:
            y = torch.ops.aten.convolution(x16, w16, None, stride, padding, (1, 1), False, (0, 0), 1)
            if not y.is_contiguous(memory_format=cl):
                y = y.contiguous(memory_format=cl)
            y = ext.bias_act_nhwc_(y, b, residual=r16, relu=relu)
        ctx.conv = (stride, padding, bool(relu), residual is not None and residual.dtype, one_launch, route)
        ctx.save_for_backward(x16, w16, y if relu else None, weight, gamma, rstd, mean_rstd, conv_bias)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x16, w16, y, weight, gamma, rstd, mean_rstd, conv_bias = ctx.saved_tensors
        stride, padding, relu, res_dtype, one_launch, route = ctx.conv
        need = ctx.needs_input_grad
        s = None if (gamma is None or one_launch) else gamma * rstd
        cl = torch.channels_last
        if not (gy.dtype == torch.bfloat16 and gy.is_contiguous(memory_format=cl)):
            gy = gy.to(torch.bfloat16).contiguous(memory_format=cl)
        g, gb = ext.bias_act_bwd_nhwc(gy, y, relu=relu)
        if (ConvBNActFunction.own_conv1x1_backward and route == '1x1' and g.data_ptr() % 4 == 0
                and x16.data_ptr() % 4 == 0):
            # the nodes whose forward took conv1x1_nhwc: the weight gradient on conv1x1_wgrad_nhwc, the stride-1 data gradient
            # on the forward kernel with the transposed weight; the stride-2 data gradient (a scatter) stays on ATen (as does a
            # view at an odd element offset: the kernels load dwords)
            gx = gw = None
            if need[1] or need[2]:
                gw = ext.conv1x1_wgrad_nhwc(g, x16, stride[0], out_dtype=torch.bfloat16)
            if need[0] and stride[0] == 1:
                gx = ext.conv1x1_dgrad_nhwc(g, w16)
            elif need[0]:
                gx = torch.ops.aten.convolution_backward(g, x16, w16, None, stride, padding, (1, 1), False, (0, 0), 1,
                                                         (True, False, False))[0]
        elif (ConvBNActFunction.own_conv3x3_backward and route == '3x3' and g.data_ptr() % 4 == 0
                and x16.data_ptr() % 4 == 0):
            # the nodes whose forward took conv3x3_nhwc, in the same way: conv3x3_wgrad_nhwc, and at stride 1 the forward kernel
            # on the flipped, transposed weight where that kernel has the shape (Cin % 128 == 0: its output channels); every
            # other data gradient (stride 2 is a scatter) stays on ATen.  The stride-2 WEIGHT gradients are not gated back to
            # ATen: ahead of it on all four base-config shapes (EXPERIMENTS.md 8o)
            gx = gw = None
            if need[1] or need[2]:
                gw = ext.conv3x3_wgrad_nhwc(g, x16, stride[0], out_dtype=torch.bfloat16)
            if need[0] and stride[0] == 1 and x16.shape[1] % 128 == 0:
                gx = ext.conv3x3_dgrad_nhwc(g, w16)
            elif need[0]:          # stride 2, or Cin % 128: the forward kernel on the swapped channels has no such shape
                gx = torch.ops.aten.convolution_backward(g, x16, w16, None, stride, padding, (1, 1), False, (0, 0), 1,
                                                         (True, False, False))[0]
        else:
            gx, gw, _ = torch.ops.aten.convolution_backward(g, x16, w16, None, stride, padding, (1, 1), False, (0, 0), 1,
                                                            (bool(need[0]), bool(need[1] or need[2]), False))
        dW = dgamma = dbeta = dcb = None
        if gw is not None and one_launch:
            # the fold's chain rule, one launch, makes dW and dgamma together; a mask that wants one of them (frozen BatchNorm
            # affine parameters, frozen convolution weights) takes the same launch and drops the other: the same bits as under
            # the full mask
            dW, dgamma = ext.conv_bn_fold_bwd(gw, weight, gamma, rstd, mean_rstd, gb)
            if not need[1]:
                dW = None
            if not need[2]:
                dgamma = None
        elif gw is not None:
            gwf = gw.float()
            if s is not None:
                if need[1]:
                    dW = gwf * s.view(-1, 1, 1, 1)
                if need[2]:
                    dot = (gwf * weight).sum((1, 2, 3))
                    dgamma = rstd * dot - mean_rstd * gb
                    if conv_bias is not None:
                        dgamma = dgamma + rstd * conv_bias * gb
            elif need[1]:
                dW = gwf
        if gamma is not None:
            if need[3]:
                dbeta = gb
            if conv_bias is not None and need[6]:
                dcb = s * gb
        elif conv_bias is not None and need[6]:
            dcb = gb
        dres = None
        if need[7]:
            dres = g if res_dtype == torch.bfloat16 else g.to(res_dtype)
        return gx, dW, dgamma, dbeta, None, None, dcb, dres, None, None, None


def _fused_train_ok(x):
    """The fused training nodes serve the bf16-autocast backbone of the training step (device tensors only)."""
    return (Bottleneck.fused_train_nodes and torch.is_grad_enabled() and x.is_cuda and torch.is_autocast_enabled()
            and torch.get_autocast_dtype('cuda') == torch.bfloat16)


def conv_bn_act(x, conv, bn, relu=False, residual=None):
    """ConvBNActFunction on a Conv2d (+ eval-mode BatchNorm2d or None)."""
    if bn is not None:
        rstd, mean_rstd = _bn_fold_constants(bn)
        return ConvBNActFunction.apply(x, conv.weight, bn.weight, bn.bias, rstd, mean_rstd, conv.bias, residual,
                                       conv.stride, conv.padding, relu)
    return ConvBNActFunction.apply(x, conv.weight, None, None, None, None, conv.bias, residual, conv.stride, conv.padding,
                                   relu)


def _plain_conv(conv):
    return (tuple(conv.dilation) == (1, 1) and conv.groups == 1 and conv.padding_mode == 'zeros'
            and isinstance(conv.padding, tuple) and conv.weight.shape[0] % 8 == 0 and conv.weight.shape[0] <= 2048)


class Bottleneck(nn.Module):
    expansion = 4
    fold_eval_bn = True     # class-wide switch (OCC_TRAIN_FOLD_BN=0 clears it)
    fused_train_nodes = os.environ.get("OCC_TRAIN_FUSED_CONV", "1") != "0"    # ConvBNActFunction under bf16 autocast

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        # style='pytorch': the stride sits on the 3x3 conv
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        if (self.fold_eval_bn and torch.is_grad_enabled() and not self.bn1.training and x.is_cuda
                and self.bn1.affine and self.bn1.track_running_stats):
            if _fused_train_ok(x) and all(_plain_conv(c) for c in (self.conv1, self.conv2, self.conv3)) and \
                    (self.downsample is None or _plain_conv(self.downsample[0])):
                identity = x if self.downsample is None else conv_bn_act(x, self.downsample[0], self.downsample[1])
                out = conv_bn_act(x, self.conv1, self.bn1, relu=True)
                out = conv_bn_act(out, self.conv2, self.bn2, relu=True)
                return conv_bn_act(out, self.conv3, self.bn3, relu=True, residual=identity)
            identity = x if self.downsample is None else conv_bn_folded(x, self.downsample[0], self.downsample[1])
            out = self.relu(conv_bn_folded(x, self.conv1, self.bn1))
            out = self.relu(conv_bn_folded(out, self.conv2, self.bn2))
            out = conv_bn_folded(out, self.conv3, self.bn3)
            return self.relu(out + identity)
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + identity)


if os.environ.get("OCC_TRAIN_FOLD_BN", "1") == "0":
    Bottleneck.fold_eval_bn = False


@BACKBONES.register_module()
class ResNet(BaseModule):
    arch = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}

    def __init__(self, depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=-1,
                 norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, style='pytorch',
                 with_cp=False, pretrained=None, in_channels=3, base_channels=64, init_cfg=None,
                 **kwargs):
        super().__init__(init_cfg)
        if depth not in self.arch:
            raise KeyError(f'invalid depth {depth} for resnet (bottleneck depths only)')
        assert style == 'pytorch'
        self.depth, self.num_stages = depth, num_stages
        self.out_indices, self.frozen_stages, self.norm_eval = out_indices, frozen_stages, norm_eval
        self.norm_requires_grad = bool(dict(norm_cfg or {}).get('requires_grad', True))
        self.conv1 = nn.Conv2d(in_channels, base_channels, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(base_channels)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        inplanes = base_channels
        self.res_layers = []
        for i, n in enumerate(self.arch[depth][:num_stages]):
            planes = base_channels * 2 ** i
            stride = 1 if i == 0 else 2
            blocks = []
            for j in range(n):
                ds = None
                if j == 0 and (stride != 1 or inplanes != planes * 4):
                    ds = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * 4))
                blocks.append(Bottleneck(inplanes, planes, stride if j == 0 else 1, ds))
                inplanes = planes * 4
            name = f'layer{i + 1}'
            self.add_module(name, nn.Sequential(*blocks))
            self.res_layers.append(name)
        if not self.norm_requires_grad:     # norm_cfg=dict(type='BN', requires_grad=False): frozen affine parameters
            for m in self.modules():
                if isinstance(m, nn.BatchNorm2d):
                    for p_ in m.parameters():
                        p_.requires_grad = False
        self._freeze_stages()

    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            for m in (self.conv1, self.bn1):
                m.eval()
                for p in m.parameters():
                    p.requires_grad = False
        for i in range(1, self.frozen_stages + 1):
            m = getattr(self, self.res_layers[i - 1])
            m.eval()
            for p in m.parameters():
                p.requires_grad = False

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    use_frozen_prefix_plan = os.environ.get("OCC_TRAIN_FROZEN_PREFIX", "1") != "0"

    def _frozen_prefix(self, x):
        """Training with frozen_stages >= 1: the stem and the frozen stages need no autograd graph, so they run on
        the inference plan's kernels (whole stem + whole-bottleneck launches, bf16 NHWC) instead of MIOpen.
        -> (activation after the last frozen stage, number of stages done) or (None, 0)."""
        n = self.frozen_stages
        if not (self.use_frozen_prefix_plan and self.training and n >= 1 and x.is_cuda and x.dtype == torch.float32
                and torch.is_autocast_enabled() and torch.get_autocast_dtype('cuda') == torch.bfloat16
                and not any(i < n for i in self.out_indices)):
            return None, 0
        plan = getattr(self, '_prefix_plan', None)
        if plan is None or plan.built_epoch != cache_epoch():
            plan = FusedInferenceBackbone(self, None, dtype=torch.bfloat16, prefix_stages=n)
            plan.built_epoch = cache_epoch()
            object.__setattr__(self, '_prefix_plan', plan)      # not a sub-module: owns folded copies
        if not plan._stem_fused:
            return None, 0
        return plan.forward_prefix(x.contiguous()), n

    def forward(self, x):
        x0, done = self._frozen_prefix(x)
        if x0 is not None:
            x = x0
        else:
            x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        outs = []
        for i, name in enumerate(self.res_layers):
            if i < done:
                continue
            x = getattr(self, name)(x)
            if i in self.out_indices:
                outs.append(x)
        return tuple(outs)

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, nn.modules.batchnorm._BatchNorm):
                    m.eval()
        return self


@NECKS.register_module()
class FPN(BaseModule):
    """1x1 laterals, top-down nearest upsample-add, 3x3 output convs, extra stride-2 levels."""

    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1,
                 add_extra_convs=False, relu_before_extra_convs=False, no_norm_on_lateral=False,
                 conv_cfg=None, norm_cfg=None, act_cfg=None, upsample_cfg=dict(mode='nearest'),
                 init_cfg=None, **kwargs):
        super().__init__(init_cfg)
        assert isinstance(in_channels, (list, tuple))
        self.in_channels, self.out_channels = in_channels, out_channels
        self.num_ins, self.num_outs = len(in_channels), num_outs
        self.relu_before_extra_convs = relu_before_extra_convs
        self.upsample_cfg = dict(upsample_cfg)
        self.backbone_end_level = self.num_ins if end_level in (-1, self.num_ins - 1) else end_level + 1
        self.start_level = start_level
        if add_extra_convs is True:
            add_extra_convs = 'on_input'
        assert add_extra_convs in (False, 'on_input', 'on_lateral', 'on_output')
        self.add_extra_convs = add_extra_convs
        self.lateral_convs = nn.ModuleList()
        self.fpn_convs = nn.ModuleList()
        for i in range(self.start_level, self.backbone_end_level):
            self.lateral_convs.append(ConvModule(in_channels[i], out_channels, 1, conv_cfg=conv_cfg,
                                                 norm_cfg=None if no_norm_on_lateral else norm_cfg,
                                                 act_cfg=act_cfg, inplace=False))
            self.fpn_convs.append(ConvModule(out_channels, out_channels, 3, padding=1,
                                             conv_cfg=conv_cfg, norm_cfg=norm_cfg, act_cfg=act_cfg,
                                             inplace=False))
        extra_levels = num_outs - self.backbone_end_level + self.start_level
        if self.add_extra_convs and extra_levels >= 1:
            for i in range(extra_levels):
                cin = self.in_channels[self.backbone_end_level - 1] \
                    if (i == 0 and self.add_extra_convs == 'on_input') else out_channels
                self.fpn_convs.append(ConvModule(cin, out_channels, 3, stride=2, padding=1,
                                                 conv_cfg=conv_cfg, norm_cfg=norm_cfg,
                                                 act_cfg=act_cfg, inplace=False))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    @staticmethod
    def _run(cm, x):
        """A bias-only ConvModule of the neck: under the training step's bf16 autocast one fused autograd node
        (ConvBNActFunction: bias in the convolution's epilogue, bias gradient in one pass), otherwise the module itself."""
        if (_fused_train_ok(x) and not getattr(cm, 'with_norm', False) and not getattr(cm, 'with_activation', False)
                and isinstance(getattr(cm, 'conv', None), nn.Conv2d) and _plain_conv(cm.conv)):
            return conv_bn_act(x, cm.conv, None)
        return cm(x)

    def forward(self, inputs):
        assert len(inputs) == len(self.in_channels)
        laterals = [self._run(conv, inputs[i + self.start_level]) for i, conv in enumerate(self.lateral_convs)]
        n = len(laterals)
        for i in range(n - 1, 0, -1):
            laterals[i - 1] = laterals[i - 1] + F.interpolate(
                laterals[i], size=laterals[i - 1].shape[2:], **self.upsample_cfg)
        outs = [self._run(self.fpn_convs[i], laterals[i]) for i in range(n)]
        if self.num_outs > len(outs):
            if not self.add_extra_convs:
                for _ in range(self.num_outs - n):
                    outs.append(F.max_pool2d(outs[-1], 1, stride=2))
            else:
                if self.add_extra_convs == 'on_input':
                    src = inputs[self.backbone_end_level - 1]
                elif self.add_extra_convs == 'on_lateral':
                    src = laterals[-1]
                else:
                    src = outs[-1]
                outs.append(self._run(self.fpn_convs[n], src))
                for i in range(n + 1, self.num_outs):
                    src = F.relu(outs[-1]) if self.relu_before_extra_convs else outs[-1]
                    outs.append(self._run(self.fpn_convs[i], src))
        return tuple(outs)
