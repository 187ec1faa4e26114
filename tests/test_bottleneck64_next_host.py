"""not-gpu: occ_bottleneck64_next_pick is a pure function of the shape that follows the 1x1 launcher's default rule, the
entry point refuses bad arguments before any launch, and the plan's routing conditions on records built on the CPU."""
import ctypes

import pytest
import torch

from occnet_amd import _lib


def test_pick_follows_the_1x1_launchers_default_rule():
    pick = _lib.lib().occ_bottleneck64_next_pick
    # layer1 maps of the configs: base and hi-res (6 cameras, 928 x 1600), tiny (1 camera, 256 x 256)
    assert pick(6, 232, 400, 128) != 0
    assert pick(1, 64, 64, 128) != 0
    assert pick(6, 232, 400, 128) == pick(6, 232, 400, 128)
    # the stride-2 output decides: M = 23 * 22 = 506 stays on the three launches, 23 * 23 = 529 and 16 * 32 = 512 fuse
    assert pick(1, 46, 44, 128) == 0 and pick(1, 45, 43, 128) == 0
    assert pick(1, 45, 45, 128) != 0
    assert pick(1, 31, 63, 128) != 0 and pick(1, 32, 64, 128) != 0       # 16 * 32 = 512 exactly
    assert pick(1, 31, 62, 128) == 0                                     # 16 * 31 = 496
    assert pick(2, 16, 31, 128) == 0 and pick(2, 16, 63, 128) != 0       # over images: 2 * 8 * 16 = 256, 2 * 8 * 32 = 512
    # no kernel for other mid channels; degenerate shapes
    for cm in (0, 32, 64, 96, 256, 512):
        assert pick(6, 232, 400, cm) == 0, cm
    for args in [(0, 232, 400, 128), (6, 0, 400, 128), (6, 232, 0, 128), (-1, 232, 400, 128)]:
        assert pick(*args) == 0, args


def test_entry_point_refuses_bad_arguments_without_gpu():
    lib = _lib.lib()
    buf = [ctypes.create_string_buffer(64) for _ in range(13)]
    good = [ctypes.cast(b, ctypes.c_void_p) for b in buf]
    f, null = lib.occ_bottleneck64_next_nhwc_bf16, None
    for i in range(13):                                                          # each pointer in turn
        a = list(good)
        a[i] = null
        assert f(*a, 1, 4, 4, 128, null) == -1
    for dims in [(0, 4, 4), (1, 0, 4), (1, 4, -1)]:
        assert f(*good, *dims, 128, null) == -1
    a = list(good)
    a[12] = a[11]                                                                # y and shortcut the same buffer
    assert f(*a, 1, 4, 4, 128, null) == -1
    for cm in (64, 256, 0):
        assert f(*good, 1, 4, 4, cm, null) == -3
        assert b'no kernel for cmid_next' in lib.occ_last_error()
    assert f(*good, 1 << 15, 1 << 10, 1 << 10, 128, null) == -3                  # 2^35 pixels
    assert b'too large' in lib.occ_last_error()


@pytest.fixture()
def plan():
    """A ResNet-50 + FPN plan built on the CPU (no own kernels: kind None, no whole bottlenecks), with the records the rule
    looks at marked as a device plan marks them."""
    from occnet_amd.plugin.backbone import FPN, FusedInferenceBackbone, ResNet
    torch.manual_seed(0)
    bb = ResNet(depth=50, num_stages=4, out_indices=(1, 2, 3), frozen_stages=1, norm_eval=True).eval()
    nk = FPN(in_channels=[512, 1024, 2048], out_channels=256, start_level=0, add_extra_convs='on_output',
             num_outs=4, relu_before_extra_convs=True).eval()
    with torch.no_grad():
        p = FusedInferenceBackbone(bb, nk, dtype=torch.float32, fuse_next_stage=True)
    assert len(p._bneck) == 0
    for bi, blk in enumerate(p.stages[0]):
        p._bneck[(0, bi)] = dict(cin=blk[0].weight.shape[1], ds=blk[3] is not None)
    for blocks in p.stages[1:]:
        for c1, c2, c3, ds in blocks:
            c1.kind, c2.kind, c3.kind = '1x1', '3x3', '1x1'
            if ds is not None:
                ds.kind = '1x1'
    return p


def test_plan_routing_conditions(plan):
    c1, _, _, ds = plan.stages[1][0]
    assert plan._next_block_operands(0) == (c1, ds)
    assert (c1.cout, ds.cout, tuple(c1.stride), tuple(ds.stride)) == (128, 512, (1, 1), (2, 2))
    # a plan built without fuse_next_stage keeps one launch per convolution
    plan.fuse_next_stage = False
    assert plan._next_block_operands(0) is None
    plan.fuse_next_stage = True
    # layer2 and layer3 end in blocks the whole-bottleneck kernel does not take; layer4 has no successor
    assert [plan._next_block_operands(si) for si in (1, 2, 3)] == [None, None, None]
    # the stage's output is an FPN input
    plan.out_indices = (0, 1, 2, 3)
    assert plan._next_block_operands(0) is None
    plan.out_indices = (1, 2, 3)
    # the last block is not a whole bottleneck / is the projection block
    whole = plan._bneck.pop((0, 2))
    assert plan._next_block_operands(0) is None
    plan._bneck[(0, 2)] = dict(cin=64, ds=True)
    assert plan._next_block_operands(0) is None
    plan._bneck[(0, 2)] = whole
    # either reader off the own 1x1 kernel
    for rec in (c1, ds):
        rec.kind = None
        assert plan._next_block_operands(0) is None
        rec.kind = '1x1'
    # strides: a conv1 that carries the stride (caffe style), a stride-1 shortcut
    c1.stride, ds.stride = (2, 2), (2, 2)
    assert plan._next_block_operands(0) is None
    c1.stride, ds.stride = (1, 1), (1, 1)
    assert plan._next_block_operands(0) is None
    c1.stride, ds.stride = (1, 1), (2, 2)
    assert plan._next_block_operands(0) == (c1, ds)
    # a shortcut that is not 4 x the mid channels
    w = ds.weight
    ds.weight = w[:256]
    assert plan._next_block_operands(0) is None
    ds.weight = w
    # no downsample record
    blk = plan.stages[1][0]
    plan.stages[1][0] = (c1, blk[1], blk[2], None)
    assert plan._next_block_operands(0) is None
    plan.stages[1][0] = blk
    assert plan._next_block_operands(0) == (c1, ds)
    # a plan that ends at the stage (prefix_stages = 1)
    plan.stages = plan.stages[:1]
    assert plan._next_block_operands(0) is None


def test_the_model_asks_for_the_route_and_a_plain_plan_does_not():
    """enable_fused_backbone passes fuse_next_stage (default on) through to the plan it builds and keeps it among the
    arguments a rebuild repeats; FusedInferenceBackbone's own default is off."""
    import inspect
    from occnet_amd.plugin.backbone import FusedInferenceBackbone
    from occnet_amd.plugin.bevformer_occ import BEVFormerOcc
    assert inspect.signature(FusedInferenceBackbone.__init__).parameters['fuse_next_stage'].default is False
    assert inspect.signature(BEVFormerOcc.enable_fused_backbone).parameters['fuse_next_stage'].default is True

    class Stub:
        training = False
        _backbone_signature = lambda self: None
    stub = Stub()
    BEVFormerOcc.enable_fused_backbone(stub, dtype=None)
    assert stub._inference_backbone_args['fuse_next_stage'] is True and stub._inference_backbone is None
    BEVFormerOcc.enable_fused_backbone(stub, dtype=None, fuse_next_stage=False)
    assert stub._inference_backbone_args['fuse_next_stage'] is False
