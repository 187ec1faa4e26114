"""not-gpu: the backbone plan's routing rule (which convolution runs on which own kernel) over every convolution of the
configs' ResNet-50 + FPN, and the shape of a plan built on the CPU: records instead of numbered attributes, nothing in its
state_dict."""
import re

import pytest
import torch

from occnet_amd.plugin.backbone_plan import own_conv_kind

# every distinct convolution of ResNet-50 (out_indices (1, 2, 3)) + FPN(512 / 1024 / 2048 -> 256, 4 outs, on_output):
# (Cout, Cin, k, stride, padding) -> the kernel it runs on
ROUTES = {
    (64, 3, 7, 2, 3): None,                                              # stem (ext.stem_conv7x7_pool takes it whole)
    # layer1 (ext.bottleneck64_nhwc takes these blocks whole; convolution by convolution they route like this)
    (64, 64, 1, 1, 0): '1x1', (64, 256, 1, 1, 0): '1x1', (64, 64, 3, 1, 1): None, (256, 64, 1, 1, 0): '1x1',
    # layer2
    (128, 256, 1, 1, 0): '1x1', (128, 512, 1, 1, 0): '1x1', (128, 128, 3, 2, 1): '3x3', (128, 128, 3, 1, 1): '3x3',
    (512, 128, 1, 1, 0): '1x1', (512, 256, 1, 2, 0): '1x1',
    # layer3
    (256, 512, 1, 1, 0): '1x1', (256, 1024, 1, 1, 0): '1x1', (256, 256, 3, 2, 1): '3x3', (256, 256, 3, 1, 1): '3x3',
    (1024, 256, 1, 1, 0): '1x1', (1024, 512, 1, 2, 0): '1x1',
    # layer4
    (512, 1024, 1, 1, 0): '1x1', (512, 2048, 1, 1, 0): '1x1', (512, 512, 3, 2, 1): '3x3', (512, 512, 3, 1, 1): '3x3',
    (2048, 512, 1, 1, 0): '1x1', (2048, 1024, 1, 2, 0): '1x1',
    # FPN: laterals (512 -> 256 is layer3's first conv1 shape), output convolutions (layer3's conv2 shapes: stride 1,
    # and stride 2 for the extra level)
    (256, 2048, 1, 1, 0): '1x1',
}


@pytest.fixture(scope="module")
def modules():
    from occnet_amd.plugin.backbone import FPN, ResNet
    torch.manual_seed(0)
    bb = ResNet(depth=50, num_stages=4, out_indices=(1, 2, 3), frozen_stages=1, norm_eval=True).eval()
    nk = FPN(in_channels=[512, 1024, 2048], out_channels=256, start_level=0, add_extra_convs='on_output',
             num_outs=4, relu_before_extra_convs=True).eval()
    return bb, nk


def test_routing_rule_over_resnet50_fpn_and_off_each_edge(modules):
    seen = set()
    for net in modules:
        for m in net.modules():
            if isinstance(m, torch.nn.Conv2d):
                assert m.kernel_size[0] == m.kernel_size[1] and m.stride[0] == m.stride[1] and m.padding[0] == m.padding[1]
                key = (m.out_channels, m.in_channels, m.kernel_size[0], m.stride[0], m.padding[0])
                assert key in ROUTES, key
                assert own_conv_kind(m.weight.shape, m.stride, m.padding, m.dilation, m.groups) == ROUTES[key], key
                seen.add(key)
    assert seen == set(ROUTES)                                          # the table lists these convolutions and no others
    # one step off each edge of the rule
    assert own_conv_kind((128, 128, 3, 3), (1, 1), (1, 1), (1, 1), 1) == '3x3'
    assert own_conv_kind((64, 128, 3, 3), (1, 1), (1, 1), (1, 1), 1) is None         # Cout 64 for a 3x3
    assert own_conv_kind((128, 128, 3, 3), (1, 2), (1, 1), (1, 1), 1) is None        # stride (1, 2)
    assert own_conv_kind((128, 128, 3, 3), (1, 1), (2, 2), (2, 2), 1) is None        # dilation 2
    assert own_conv_kind((128, 64, 3, 3), (1, 1), (1, 1), (1, 1), 2) is None         # groups 2
    assert own_conv_kind((128, 48, 3, 3), (1, 1), (1, 1), (1, 1), 1) is None         # Cin 48
    assert own_conv_kind((128, 128, 3, 3), (1, 1), (0, 0), (1, 1), 1) is None        # no padding
    assert own_conv_kind((128, 128, 3, 3), (3, 3), (1, 1), (1, 1), 1) is None        # stride 3
    assert own_conv_kind((64, 64, 1, 1), (3, 3), (0, 0), (1, 1), 1) == '1x1'         # any equal strides for a 1x1
    assert own_conv_kind((64, 64, 1, 1), (1, 2), (0, 0), (1, 1), 1) is None
    assert own_conv_kind((64, 64, 1, 1), (1, 1), (0, 0), (2, 2), 1) is None
    assert own_conv_kind((64, 32, 1, 1), (1, 1), (0, 0), (1, 1), 2) is None
    assert own_conv_kind((64, 48, 1, 1), (1, 1), (0, 0), (1, 1), 1) is None
    assert own_conv_kind((48, 64, 1, 1), (1, 1), (0, 0), (1, 1), 1) is None          # Cout 48
    assert own_conv_kind((64, 64, 1, 1), (1, 1), (1, 1), (1, 1), 1) is None          # a padded 1x1
    assert own_conv_kind((64, 64, 1, 1), [2, 2], [0, 0]) == '1x1'                    # lists, dense by default


def test_plan_on_cpu_holds_records_and_an_empty_state_dict(modules):
    from occnet_amd.plugin.backbone import FusedInferenceBackbone
    from occnet_amd.plugin.backbone_plan import _FoldedConv
    bb, nk = modules
    with torch.no_grad():
        plan = FusedInferenceBackbone(bb, nk, dtype=torch.float32, hip_tail=True)   # fp32: hip_tail switches off
    assert len(plan.state_dict()) == 0
    assert not plan.hip_tail and len(plan._bneck) == 0 and not plan._stem_fused
    records = [plan.stem] + [c for blocks in plan.stages for blk in blocks for c in blk if c is not None] \
        + plan.laterals + plan.fpn
    assert len(plan.stages) == 4 and len(records) == 1 + 16 * 3 + 4 + 3 + 4
    assert all(isinstance(c, _FoldedConv) and c.kind is None and c.pack is None for c in records)
    assert {id(m) for m in plan.modules()} == {id(plan), id(plan._records)} | {id(c) for c in records}
    old = re.compile(r"(w|b|m|p)\d+|k\d+_.*")
    for m in plan.modules():
        names = set(vars(m)) | set(m._buffers) | set(m._parameters) | {n for n, _ in m.named_buffers()}
        assert not [n for n in names if old.fullmatch(n.rsplit('.', 1)[-1])], type(m)
    assert len(list(plan.buffers())) == 2 * len(records)                    # weight + bias each; no pack off the device
