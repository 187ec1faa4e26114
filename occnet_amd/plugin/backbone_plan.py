"""Inference-time execution plan of the image backbone (ResNet + FPN): one record per folded convolution, one rule for
which convolution runs on which of this repository's kernels, and the plan that walks the records.  A leaf module: it
imports nothing from backbone.py (which holds the modules the plan is built from, and the training-time nodes)."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.utils.fusion import fuse_conv_bn_weights

from .. import ext
from .._lib import OccAmdUnsupported

_CL = torch.channels_last


def own_conv_kind(weight_shape, stride, padding, dilation=(1, 1), groups=1):
    """Which own kernel computes a convolution of this shape: '1x1' (ext.conv1x1_nhwc), '3x3' (ext.conv3x3_nhwc) or None
    (MIOpen + one fused tail launch).  Shape conditions only; what depends on the call (bf16 kernels switched on, device
    tensors, channels_last layout, and for the 3x3 kernel "no residual") is checked where the call is made."""
    cout, cin, kh, kw = weight_shape
    stride, padding = tuple(stride), tuple(padding)
    if tuple(dilation) != (1, 1) or groups != 1 or cin % 32:
        return None
    if (kh, kw) == (1, 1) and padding == (0, 0) and stride[0] == stride[1] and cout % 32 == 0:
        return '1x1'
    if (kh, kw) == (3, 3) and padding == (1, 1) and stride in ((1, 1), (2, 2)) and cout % 128 == 0:
        return '3x3'
    return None


class _FoldedConv(nn.Module):
    """One convolution of the plan with its BatchNorm already folded in: weight (plan dtype, channels_last), bias (fp32
    under hip_tail, else plan dtype), `kind` = the own kernel it runs on (own_conv_kind; None without hip_tail or off the
    device) and `pack` = that kernel's weight operand.  Non-persistent buffers: .to() / .cuda() reach them, state_dict()
    does not."""

    def __init__(self, w, b, conv, dtype, hip_tail):
        super().__init__()
        w = w.detach().to(dtype).contiguous(memory_format=_CL)
        if b is None:
            b = torch.zeros(w.shape[0], device=w.device)
        b = b.detach().float() if hip_tail else b.detach().to(dtype)
        self.stride, self.padding, self.dilation, self.groups = conv.stride, conv.padding, conv.dilation, conv.groups
        self.kind = None
        if hip_tail and w.is_cuda:
            self.kind = own_conv_kind(w.shape, conv.stride, conv.padding, conv.dilation, conv.groups)
        pack = None
        if self.kind == '1x1':      # the fused bf16 GEMM (occ_conv1x1_nhwc_bf16): (Cout, Cin) weight matrix
            pack = ext.conv1x1_pack_weight(w.reshape(w.shape[0], w.shape[1]))
        elif self.kind == '3x3':    # own implicit-GEMM kernel (bias + ReLU fused)
            pack = ext.conv3x3_pack_weight(w.float().contiguous())
        self.register_buffer('weight', w, persistent=False)
        self.register_buffer('bias', b, persistent=False)
        self.register_buffer('pack', pack, persistent=False)

    @property
    def cout(self):
        return self.weight.shape[0]


class _FusedBottleneck(nn.Module):
    """The operand set of ext.bottleneck64_nhwc for one 64-mid-channel block (ext.bottleneck64_pack's entries as
    non-persistent buffers); ext reads it by bottleneck64_pack's keys."""
    _OPERANDS = dict(w1='conv1_frag', b1='conv1_bias', w2='conv2_frag', b2='conv2_bias', w3='conv3_frag', b3='conv3_bias')

    def __init__(self, pk):
        super().__init__()
        for key, name in self._OPERANDS.items():
            self.register_buffer(name, pk[key], persistent=False)
        self.cin, self.ds = pk['cin'], pk['ds']

    def __getitem__(self, key):
        return self._buffers[self._OPERANDS[key]] if key in self._OPERANDS else self.__dict__[key]


class FusedInferenceBackbone(nn.Module):
    """Inference-time execution plan for ResNet + FPN: eval-mode BatchNorm folded into the preceding
    convolution (`fuse_conv_bn_weights`), bf16, channels_last (NHWC) memory end to end, so the FPN outputs are
    already in the (Cam, H, W, C) layout the hot path reads.  With `hip_tail` (bf16, default) every layer of the
    configs' ResNet-50 + FPN runs on this repository's kernels: whole stem (ext.stem_conv7x7_pool), whole
    64-mid-channel bottlenecks (ext.bottleneck64_nhwc; with `fuse_next_stage` the last one of a stage that is no FPN input
    also computes the next block's conv1 and shortcut, ext.bottleneck64_next_nhwc), 1x1 / 3x3 convolutions with bias,
    residual and ReLU fused (ext.conv1x1_nhwc incl. the FPN top-down step, ext.conv3x3_nhwc); convolutions of other shapes fall back to
    MIOpen + one fused bias/residual/ReLU launch.  `hip_tail=False` keeps stock torch ops (any dtype).  Built from the
    live modules' parameters (it owns folded COPIES: rebuild after changing weights).  The backbone is outside
    SURVEY.md §8's hand-written scope; these kernels exist because end-to-end samples/s (images -> voxels) is the
    headline metric."""

    def __init__(self, backbone, neck, dtype=torch.bfloat16, hip_tail=True, fused_bottleneck=True, prefix_stages=None,
                 fuse_next_stage=False):
        super().__init__()
        # fuse_next_stage: a stage's last whole bottleneck also computes the next stage's conv1 and shortcut where
        # _next_block_operands allows it (the same bits, two launches and the stage's output map less).  Opt-in: a plan
        # built without it launches every block's convolutions one by one, as callers that watch or replace those
        # launches expect; the model's enable_fused_backbone asks for it.
        self.fuse_next_stage = bool(fuse_next_stage)
        # prefix_stages = k: fold only the stem and the first k stages, no neck (forward_prefix: the frozen part of
        # a training step)
        self.prefix_stages = prefix_stages
        # hip_tail: bias + (residual) + ReLU after each convolution as ONE in-place HIP launch
        # (occ_bias_act_nhwc_bf16) instead of PyTorch's add / add_ / relu_ launches (bf16 only)
        self.hip_tail = hip_tail and dtype == torch.bfloat16
        self.use_graph = False      # set True to replay the plan as one hipGraph per input shape
        self._graphs = {}
        assert not backbone.training or backbone.norm_eval, "folding BN needs eval-mode statistics"
        self.dtype = dtype
        self.out_indices = backbone.out_indices
        # every record, in build order: what .to() / .cuda() walk (stages / laterals / fpn below are plain lists of them)
        self._records = nn.ModuleList()

        def add(w, b, conv):
            self._records.append(_FoldedConv(w, b, conv, dtype, self.hip_tail))
            return self._records[-1]

        def fold(conv, bn):
            return add(*fuse_conv_bn_weights(conv.weight, conv.bias, bn.running_mean, bn.running_var,
                                             bn.eps, bn.weight, bn.bias), conv)

        self.stem = fold(backbone.conv1, backbone.bn1)
        # whole stem (7x7/s2 convolution + bias + ReLU + 3x3/s2 max pooling) as one kernel reading the fp32 NCHW
        # images directly
        c1, mp = backbone.conv1, backbone.maxpool
        pool_ok = (mp.kernel_size, mp.stride, mp.padding) in ((3, 2, 1), ((3, 3), (2, 2), (1, 1)))
        sw = self.stem.weight
        self._stem_fused = (self.hip_tail and sw.is_cuda and tuple(sw.shape) == (64, 3, 7, 7) and pool_ok
                            and tuple(c1.stride) == (2, 2) and tuple(c1.padding) == (3, 3)
                            and tuple(c1.dilation) == (1, 1) and c1.groups == 1
                            and getattr(mp, 'dilation', 1) in (1, (1, 1)) and not getattr(mp, 'ceil_mode', False))
        if self._stem_fused:
            self.register_buffer('stem_frag', ext.stem_pack_weight(sw), persistent=False)
        self.stages = []
        for name in (backbone.res_layers if prefix_stages is None else backbone.res_layers[:prefix_stages]):
            blocks = []
            for blk in getattr(backbone, name):
                ds = None if blk.downsample is None else fold(blk.downsample[0], blk.downsample[1])
                blocks.append((fold(blk.conv1, blk.bn1), fold(blk.conv2, blk.bn2),
                               fold(blk.conv3, blk.bn3), ds))
            self.stages.append(blocks)
        # whole-bottleneck kernel for the 64-mid-channel stride-1 blocks (ResNet-50 layer1: every layer of those
        # blocks is HBM-bound at stride 4, the fused kernel keeps the 64-channel intermediates in LDS)
        self._bneck = {}            # (stage, block) -> _FusedBottleneck
        if fused_bottleneck and self.hip_tail and sw.is_cuda:
            for si, blocks in enumerate(self.stages):
                for bi, (c1, c2, c3, ds) in enumerate(blocks):
                    ok = (tuple(c2.weight.shape) == (64, 64, 3, 3) and tuple(c3.weight.shape[:2]) == (256, 64)
                          and c2.stride == (1, 1) and c2.padding == (1, 1)
                          and ((ds is None and c1.weight.shape[1] == 256) or
                               (ds is not None and c1.weight.shape[1] == 64 and ds.stride == (1, 1))))
                    if not ok:
                        continue
                    pk = ext.bottleneck64_pack(c1.weight, c1.bias, c2.weight, c2.bias, c3.weight, c3.bias,
                                               None if ds is None else ds.weight, None if ds is None else ds.bias)
                    self._bneck[(si, bi)] = _FusedBottleneck(pk)
                    self._records.append(self._bneck[(si, bi)])
        # the live neck, for its settings only (the plan owns folded copies of its weights): not a sub-module
        object.__setattr__(self, 'neck', neck)
        if neck is None:
            self.laterals, self.fpn = [], []
            return
        self.laterals = [add(m.conv.weight, m.conv.bias, m.conv) for m in neck.lateral_convs]
        self.fpn = [add(m.conv.weight, m.conv.bias, m.conv) for m in neck.fpn_convs]
        for m in list(neck.lateral_convs) + list(neck.fpn_convs):
            assert not m.with_norm and not m.with_activation, "FPN ConvModules with norm/act not folded"

    def _conv(self, c, x, relu=False, add=None, amax=None):
        """One folded convolution (+ add) (+ ReLU; an add implies it).  amax: 8 device words the 3x3 kernel folds
        max|out| into (_forward_stages passes them only where every FPN output convolution takes that kernel)."""
        nhwc = x.is_contiguous(memory_format=_CL) and (add is None or add.is_contiguous(memory_format=_CL))
        if c.kind == '1x1' and nhwc:
            return ext.conv1x1_nhwc(x, c.pack, c.bias, residual=add, relu=relu or add is not None, stride=c.stride[0])
        if c.kind == '3x3' and add is None and nhwc:
            return ext.conv3x3_nhwc(x, c.pack, c.bias, c.cout, relu=relu, stride=c.stride[0], amax=amax)
        w, b = c.weight, c.bias
        if self.hip_tail and w.shape[0] % 8 == 0:
            y = F.conv2d(x, w, None, c.stride, c.padding, c.dilation, c.groups)
            if y.is_contiguous(memory_format=_CL) and (add is None or add.is_contiguous(memory_format=_CL)):
                return ext.bias_act_nhwc_(y, b, residual=add, relu=relu or add is not None)
            y = y + b.to(y.dtype).view(1, -1, 1, 1)
        else:
            y = F.conv2d(x, w, b.to(w.dtype), c.stride, c.padding, c.dilation, c.groups)
        if add is not None:
            y = y.add_(add)
        return y.relu_() if (relu or add is not None) else y

    @torch.no_grad()
    def forward(self, x):
        """x (N, 3, H, W) any float dtype -> tuple of FPN maps (N, C, h, w), dtype self.dtype, NHWC.
        With `use_graph` the whole plan (≈ 120 short launches) is captured into one hipGraph per input
        shape after two eager warm-up calls (MIOpen's find must not run under capture) and replayed; the
        returned maps are then the graph's static output buffers, valid until the next call."""
        if not self.use_graph or not x.is_cuda:
            return self._forward_eager(x)
        key = (tuple(x.shape), x.dtype, str(x.device))
        st = self._graphs.setdefault(key, dict(calls=0))
        st['calls'] += 1
        if st['calls'] <= 2:
            return self._forward_eager(x)
        if 'graph' not in st:
            st['in'] = x.clone()
            torch.cuda.synchronize(x.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                st['out'] = self._forward_eager(st['in'])
            st['graph'] = g
        st['in'].copy_(x)
        st['graph'].replay()
        return st['out']

    def forward_u8(self, x_u8, mean, std, to_rgb=False, size_divisor=32):
        """Raw camera images in: x_u8 (N, Hs, Ws, 3) uint8 HWC on the device; normalise + pad happen inside the stem
        kernel (ext.stem_conv7x7_pool_u8).  -> (FPN maps, padded (H, W)).  Needs the fused HIP stem."""
        if not self._stem_fused:
            raise OccAmdUnsupported("forward_u8 needs the fused stem kernel (bf16 plan, 7x7/s2 stem + 3x3/s2 pool)")
        x, hw = ext.stem_conv7x7_pool_u8(x_u8, self.stem_frag, self.stem.bias, mean, std,
                                         to_rgb=to_rgb, size_divisor=size_divisor)
        return self._forward_stages(x), hw

    def _forward_eager(self, x):
        stem = self.stem
        if self._stem_fused and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous():
            return self._forward_stages(ext.stem_conv7x7_pool(x, self.stem_frag, stem.bias))
        x = x.to(self.dtype).contiguous(memory_format=_CL)
        if self.hip_tail and stem.cout % 8 == 0 and x.is_cuda:
            # stem tail (bias + ReLU + 3x3/s2 max pooling) as one pass over the raw convolution output
            y = F.conv2d(x, stem.weight, None, stem.stride, stem.padding, stem.dilation, stem.groups)
            if y.is_contiguous(memory_format=_CL):
                x = ext.bias_relu_maxpool_nhwc(y, stem.bias)
            else:
                x = F.max_pool2d((y + stem.bias.to(y.dtype).view(1, -1, 1, 1)).relu_(), kernel_size=3, stride=2, padding=1)
        else:
            x = F.max_pool2d(self._conv(stem, x, relu=True), kernel_size=3, stride=2, padding=1)
        return self._forward_stages(x)

    def _next_block_operands(self, si):
        """(conv1, downsample) records of stage si + 1's first block where stage si's last launch can compute both
        (ext.bottleneck64_next_nhwc), else None.  The conditions that do not depend on the input: the plan was built with
        fuse_next_stage; the last block of the stage is a whole identity bottleneck; its output has no other reader (the stage is not an FPN input and the plan does not
        end there); and the two readers are a stride-1 conv1 (256 -> cmid) and a stride-2 1x1 downsample (256 -> 4 cmid) on
        the own 1x1 kernel."""
        whole = self._bneck.get((si, len(self.stages[si]) - 1)) if self.fuse_next_stage else None
        if whole is None or whole['ds'] or whole['cin'] != 256:
            return None
        if si in self.out_indices or si + 1 >= len(self.stages):
            return None
        c1, _, _, ds = self.stages[si + 1][0]
        if ds is None or c1.kind != '1x1' or ds.kind != '1x1':
            return None
        if tuple(c1.stride) != (1, 1) or tuple(ds.stride) != (2, 2) or c1.weight.shape[1] != 256 \
                or ds.weight.shape[1] != 256 or ds.cout != 4 * c1.cout:
            return None
        return c1, ds

    def _run_stage(self, si, x, head=None, fuse_next=True):
        """One stage -> (x, head).  head = (y, identity) of the NEXT stage's first block when this stage's last launch
        computed them in place of its own output (x is then None), else None; the `head` argument is what the previous
        stage handed over.  fuse_next=False keeps every stage's own output (forward_prefix)."""
        last = len(self.stages[si]) - 1
        for bi, (c1, c2, c3, ds) in enumerate(self.stages[si]):
            if bi == 0 and head is not None:
                y, identity = head
                fused = self._conv23_fused(c2, c3, y, identity)
                x = fused if fused is not None else self._conv(c3, self._conv(c2, y, relu=True), add=identity)
                continue
            whole = self._bneck.get((si, bi))
            if whole is not None and x.is_contiguous(memory_format=_CL):
                # OCC_BOTTLENECK64_NEXT=0 keeps the block's own output and the two 1x1 launches (development A/B inside one
                # build; the same bits)
                nxt = self._next_block_operands(si) if fuse_next and bi == last else None
                if nxt is not None and not os.environ.get('OCC_BOTTLENECK64_NEXT', '1').startswith('0') \
                        and x.dtype == torch.bfloat16 \
                        and ext.bottleneck64_next_pick(x.shape[0], x.shape[2], x.shape[3], nxt[0].cout):
                    n1, nds = nxt
                    return None, ext.bottleneck64_next_nhwc(x, whole, n1.pack, n1.bias, nds.pack, nds.bias)
                # OCC_BOTTLENECK64_V2=0 keeps the first kernel (development A/B inside one build; the same bits)
                first = os.environ.get('OCC_BOTTLENECK64_V2', '1').startswith('0')
                x = ext.bottleneck64_nhwc(x, whole, variant=1 if first else 0)
                continue
            identity = x if ds is None else self._conv(ds, x)
            y = self._conv(c1, x, relu=True)
            fused = self._conv23_fused(c2, c3, y, identity)
            x = fused if fused is not None else self._conv(c3, self._conv(c2, y, relu=True), add=identity)
        return x, None

    def _conv23_fused(self, c2, c3, y, identity):
        """conv2 (3x3) + conv3 (1x1 + residual + ReLU) as one launch where ext.conv3x3_conv1x1_pick fuses the shape
        (OCC_CONV3X3_FUSE_1X1=0 keeps the two launches: development A/B inside one build); None otherwise."""
        if not (c2.kind == '3x3' and c3.kind == '1x1') or os.environ.get('OCC_CONV3X3_FUSE_1X1', '1').startswith('0'):
            return None
        if not (y.is_cuda and y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=_CL)
                and identity.dtype == torch.bfloat16 and identity.is_contiguous(memory_format=_CL)):
            return None
        cmid, stride = c2.cout, c2.stride[0]
        if c3.stride != (1, 1) or c3.weight.shape[1] != cmid:
            return None
        n, _, h, w = y.shape
        if not ext.conv3x3_conv1x1_pick(n, h, w, cmid, c3.cout, stride):
            return None
        return ext.conv3x3_conv1x1_nhwc(y, c2.pack, c2.bias, cmid, c3.pack, c3.bias, identity, stride=stride)

    @torch.no_grad()
    def forward_prefix(self, x):
        """x (N, 3, H, W) fp32 contiguous -> activation after the folded stages, (N, C, h, w) bf16 channels_last."""
        x = ext.stem_conv7x7_pool(x, self.stem_frag, self.stem.bias)
        for si in range(len(self.stages)):
            x, _ = self._run_stage(si, x, fuse_next=False)
        return x

    def _forward_stages(self, x):
        feats = []
        head = None
        for si in range(len(self.stages)):
            x, head = self._run_stage(si, x, head)
            if si in self.out_indices:
                feats.append(x)
        nk = self.neck
        inputs = feats
        n = len(self.laterals)
        lat = [None] * n
        nearest = nk.upsample_cfg.get('mode', 'nearest') == 'nearest' and 'scale_factor' not in nk.upsample_cfg
        for i in range(n - 1, -1, -1):      # top-down: lateral 1x1 conv + nearest x2 upsample of the coarser level
            xin = inputs[i + nk.start_level]
            li = self.laterals[i]
            up = lat[i + 1] if i + 1 < n else None
            if up is not None and nearest and li.kind == '1x1' and xin.shape[2] == 2 * up.shape[2] \
                    and xin.shape[3] == 2 * up.shape[3] and xin.is_contiguous(memory_format=_CL):
                # one launch: the upsampled coarser lateral is the GEMM's residual
                lat[i] = ext.conv1x1_nhwc(xin, li.pack, li.bias, residual=up, relu=False, residual_upsample2=True)
                continue
            lat[i] = self._conv(li, xin)
            if up is not None:
                lat[i] = lat[i] + F.interpolate(up, size=lat[i].shape[2:], **nk.upsample_cfg)
        extra = nk.num_outs > n and bool(nk.add_extra_convs)
        # the output convolutions fold max|out| into 8 device words while they store the maps: the fp16 range scale of the SCA
        # value rows needs max|x| over exactly these maps (csrc/value_range.hip), and a separate pass over them costs 52 us.
        # Decided once, here: the words are complete only if EVERY output convolution takes the 3x3 kernel, i.e. its record
        # routes there and its input is NHWC (the extra levels fed by a routed convolution's own output always are); otherwise
        # no map carries a maximum and the consumer measures it (ext.value_range_scale).
        srcs = list(lat)
        if extra and nk.add_extra_convs == 'on_input':
            srcs.append(inputs[nk.backbone_end_level - 1])
        amax = None
        if (lat[0].is_cuda and self.dtype == torch.bfloat16
                and all(c.kind == '3x3' for c in self.fpn[:nk.num_outs if extra else n])
                and all(s.is_contiguous(memory_format=_CL) for s in srcs)):
            amax = ext.new_absmax_words(lat[0].device)
        outs = [self._conv(self.fpn[i], lat[i], amax=amax) for i in range(n)]
        if nk.num_outs > n:
            if not nk.add_extra_convs:
                for _ in range(nk.num_outs - n):                    # a subset of outs[-1]: the maximum still bounds it
                    outs.append(F.max_pool2d(outs[-1], 1, stride=2))
            else:
                if nk.add_extra_convs == 'on_input':
                    src = inputs[nk.backbone_end_level - 1]
                elif nk.add_extra_convs == 'on_lateral':
                    src = lat[-1]
                else:
                    src = outs[-1]
                outs.append(self._conv(self.fpn[n], src, amax=amax))
                for i in range(n + 1, nk.num_outs):
                    src = F.relu(outs[-1]) if nk.relu_before_extra_convs else outs[-1]
                    outs.append(self._conv(self.fpn[i], src, amax=amax))
        if amax is not None:
            for o in outs:
                ext.attach_absmax(o, amax)    # rides on the tensor OBJECTS (with their version counter): a consumer that reshapes them re-attaches it
        return tuple(outs)
