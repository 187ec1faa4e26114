"""not-gpu: the C-ABI library loads and exports every symbol include/occnet_amd.h declares; argument
validation runs without a GPU (no compute call is made); the product refuses host tensors."""
import ctypes

import pytest
import torch

from occnet_amd import _lib, ext


def test_library_exports_declared_symbols():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    assert 'occ_ms_deform_attn_forward_f32' in declared and 'occ_sca_fused_forward_f32' in declared
    missing = [s for s in declared if not hasattr(lib, s)]
    assert not missing, missing
    assert lib.occ_abi_version() == _lib.ABI == 3


def test_every_prototype_is_bound_from_the_header():
    """_lib.lib() sets restype and argtypes on every function of the header, from the header's own text."""
    import re
    protos = _lib.prototypes()
    assert sorted(protos) == _lib.declared_symbols() and len(protos) == 102
    lib = _lib.lib()
    for name, (restype, params) in protos.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), name
        assert fn.restype is restype and restype is not None, name
    with open(_lib.HEADER_PATH) as f:
        wide = set(re.findall(r"\bint64_t\s+(occ_[a-z0-9_]+)\s*\(", f.read()))
    assert len(wide) == 20
    for name in wide:
        assert getattr(lib, name).restype is ctypes.c_int64, name
    # spot checks of the three kinds of parameter: scalar widths as declared, every pointer the tensor-accepting type
    kinds = [t for t, _ in protos["occ_ms_deform_attn_backward_ws_f32"][1]]
    assert kinds[:9] == [_lib.DevicePtr] * 9 and kinds[9:17] == [ctypes.c_int] * 8
    assert kinds[17:] == [_lib.DevicePtr, ctypes.c_int64, _lib.DevicePtr]
    assert [n for _, n in protos["occ_sca_rows_encode_q16"][1]] == ["v", "out", "scale", "groups", "S", "C", "stream"]
    assert protos["occ_last_error"] == (ctypes.c_char_p, []) and protos["occ_ln_dropout_hash"][0] is ctypes.c_uint


def test_int64_answers_arrive_whole():
    lib = _lib.lib()
    assert lib.occ_linear_chain_packed_bytes(1 << 20, 1 << 11) == 1 << 33
    assert lib.occ_submission_rays_bytes(64, 8, 1 << 22) == 7 * (1 << 31)


def test_binding_mistakes_stop_on_the_host():
    """A wrong argument count or kind raises before the library is entered: its last error stays what it was."""
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    assert lib.occ_ms_deform_attn_forward_f32(null, null, null, null, null, null, 1, 1, 1, 1, 1, 1, 1, 64, null) == -1
    before = lib.occ_last_error()
    assert b'null' in before
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    with pytest.raises(TypeError):                                 # one argument short
        lib.occ_ms_deform_attn_forward_f32(p, p, p, p, p, p, 1, 1, 1, 1, 1, 1, 1, 64)
    with pytest.raises(ctypes.ArgumentError):                      # a float where int B is expected
        lib.occ_ms_deform_attn_forward_f32(p, p, p, p, p, p, 1.0, 1, 1, 1, 1, 1, 1, 64, null)
    with pytest.raises(ctypes.ArgumentError):                      # a c_int in the int64_t workspace_bytes slot
        lib.occ_ms_deform_attn_backward_ws_f32(p, p, p, p, p, p, p, p, p, 1, 1, 1, 1, 1, 1, 1, 64, p, ctypes.c_int(1), null)
    assert lib.occ_last_error() == before


def test_pointer_parameters_take_what_the_callers_pass():
    """None, an int, a c_void_p, a ctypes array, byref(...) and a torch.Tensor all cross a foreign call as the address they
    stand for (the callee here is a ctypes callback with the binding's pointer type as its argtype)."""
    echo = ctypes.CFUNCTYPE(ctypes.c_size_t, _lib.DevicePtr)(lambda p: p.value or 0)
    buf = (ctypes.c_float * 4)()
    addr = ctypes.addressof(buf)
    t = torch.zeros(4)
    assert echo(None) == 0
    for a in (addr, ctypes.c_void_p(addr), buf, ctypes.byref(buf), ctypes.cast(buf, ctypes.c_void_p)):
        assert echo(a) == addr
    assert echo(t) == t.data_ptr() != 0 and echo(t[1:]) == t.data_ptr() + 4
    with pytest.raises(ctypes.ArgumentError):
        echo(1.5)


def test_parser_refuses_a_type_it_does_not_know():
    assert list(_lib.prototypes("/* c */\n#define X 1\nint occ_y(const void* const* a, int64_t n);")["occ_y"][1]) == \
        [(_lib.DevicePtr, "a"), (ctypes.c_int64, "n")]
    with pytest.raises(_lib.OccAmdError, match="occ_x"):
        _lib.prototypes("int occ_x(double v);")
    with pytest.raises(_lib.OccAmdError, match="occ_z"):
        _lib.prototypes("double occ_z(int v);")


def test_argument_validation_without_gpu():
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    rc = lib.occ_ms_deform_attn_forward_f32(null, null, null, null, null, null, 1, 1, 1, 1, 1, 1, 1,
                                            64, null)
    assert rc == -1 and b'null' in lib.occ_last_error()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = lib.occ_ms_deform_attn_forward_f32(p, p, p, p, p, p, 3, 1, 1, 1, 1, 1, 1, 2, null)
    assert rc == -1 and b'im2col_step' in lib.occ_last_error()     # batch 3 vs step 2
    rc = lib.occ_sca_fused_forward_f32(p, p, p, p, ctypes.c_int64(512), p, ctypes.c_int64(256), p, p,
                                       null, p, null, 1, 6, 100, 4, 64, 4, 8, 8, 10, null)
    assert rc == -3                                                # M=4,D=64: no fused kernel
    with pytest.raises(_lib.OccAmdUnsupported):
        _lib.check(rc, 'sca')
    rc = lib.occ_point_sampling_f32(p, p, p, p, ctypes.c_float(0.0), ctypes.c_float(1.0), p, p, null,
                                    1, 6, 4, 8, null)
    assert rc == -1


def test_backbone_and_projection_entry_points_validate_without_gpu():
    """The newer entry points reject bad arguments / unsupported shapes before any launch."""
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    i64 = ctypes.c_int64
    assert lib.occ_conv1x1_nhwc_bf16(null, p, p, null, p, 1, 4, 4, 32, 32, 1, 0, 0, null) == -1
    assert lib.occ_conv1x1_nhwc_bf16(p, p, p, null, p, 1, 4, 4, 48, 32, 1, 0, 0, null) == -3      # Cin % 32
    assert lib.occ_conv1x1_nhwc_bf16(p, p, p, null, p, 1, 4, 4, 32, 40, 1, 0, 0, null) == -3      # Cout % 32
    assert lib.occ_conv1x1_nhwc_bf16(p, p, p, p, p, 1, 5, 4, 32, 32, 1, 0, 1, null) == -1         # odd size, up2
    assert b'upsampled residual' in lib.occ_last_error()
    assert lib.occ_conv3x3_nhwc_bf16(p, p, p, p, 1, 4, 4, 32, 128, 3, 1, null) == -3              # stride 3
    assert lib.occ_conv3x3_nhwc_bf16(p, p, p, p, 1, 4, 4, 32, 64, 1, 1, null) == -3               # Cout % 128
    assert lib.occ_bottleneck64_nhwc_bf16(p, p, p, p, p, p, p, p, 1, 4, 4, 128, 0, null) == -3    # Cin 128
    assert lib.occ_bottleneck64_nhwc_bf16(p, p, p, p, p, p, p, p, 1, 4, 4, 64, 0, null) == -3     # 64 needs ds
    assert lib.occ_mfma_pack_b_frag_bf16(p, p, 48, 16, null) == -3                                # N % 32
    assert lib.occ_stem_conv7x7_pool_f32_bf16(p, p, p, null, 1, 8, 8, null) == -1
    assert lib.occ_bias_relu_maxpool_nhwc_bf16(p, p, p, 1, 4, 4, 12, null) == -3                  # C % 8
    assert lib.occ_conv3d_pack_weight_bf16x3(p, p, 24, 32, null) == -3                            # Cin % 16
    assert lib.occ_conv3d_bn_relu_bf16x3_f32(p, p, p, p, p, 1, 6, 4, 4, 32, 32, 0, i64(1), i64(1), i64(1), 1,
                                             null) == -3                                          # Z = 6
    # value projection: segment table checks
    ptrs = (ctypes.c_void_p * 1)(ctypes.addressof(buf))
    one = (ctypes.c_int64 * 1)(64)
    zero = (ctypes.c_int64 * 1)(0)
    args = lambda n, lda, K, N: (n, ptrs, lda, one, one, zero, null, 0, p, p, i64(256), K, N, i64(64), null)
    assert lib.occ_value_proj_bf16_f32(*args(0, one, 64, 256)) == -1                              # no segments
    assert lib.occ_value_proj_bf16_f32(*args(9, one, 64, 256)) == -1                              # > 8 segments
    assert lib.occ_value_proj_bf16_f32(*args(1, one, 48, 256)) == -3                              # K % 32
    assert lib.occ_value_proj_bf16_f32(*args(1, (ctypes.c_int64 * 1)(32), 64, 256)) == -1         # lda < K
    # stacked projections (round 3): plane geometry
    pargs = lambda n_planes, plane_cols, stride: (1, ptrs, one, one, one, zero, null, 0, p, p, 1, i64(256), 64, n_planes,
                                                  plane_cols, i64(stride), i64(64), null, null)
    assert lib.occ_value_proj_bf16_planes(*pargs(0, 256, 1 << 20)) == -1                          # no planes
    assert lib.occ_value_proj_bf16_planes(*pargs(4, 256, 0)) == -1                                # plane stride
    assert lib.occ_value_proj_bf16_planes(*pargs(4, 192, 1 << 20)) == -3                          # plane_cols % 256
    assert b'plane_cols' in lib.occ_last_error()
    # range scales of the fp16 value rows (round 5): argument checks
    f4 = (ctypes.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    rargs = lambda n, lda, K, planes, l1=f4: (n, ptrs, lda, one, K, planes, l1, f4, p, p, null)
    assert lib.occ_value_range_scale_bf16(*rargs(0, one, 64, 4)) == -1                            # no segments
    assert lib.occ_value_range_scale_bf16(*rargs(1, one, 64, 9)) == -1                            # > 8 planes
    assert lib.occ_value_range_scale_bf16(*rargs(1, one, 60, 4)) == -3                            # K % 8
    assert lib.occ_value_range_scale_bf16(*rargs(1, (ctypes.c_int64 * 1)(32), 64, 4)) == -1       # lda < K
    # (round 6, abi 3: row_l1 / bias_max are DEVICE arrays — their sign cannot be checked on the host; the kernel takes |.|)
    assert lib.occ_value_range_scale_from_amax(null, 4, f4, f4, p, null) == -1                      # no maxima
    assert lib.occ_value_range_scale_from_amax(p, 9, f4, f4, p, null) == -1                         # > 8 planes
    assert lib.occ_conv3x3_nhwc_bf16_amax(p, p, p, p, 1, 4, 4, 32, 128, 1, 1, null, null) == -1     # null amax8
    assert lib.occ_value_range_scale_bf16(1, ptrs, one, one, 64, 4, f4, f4, null, p, null) == -1  # no output
    # fused second convolution + heads + decode (round 3)
    assert lib.occ_conv3d_heads_pack_bytes() == 16 * 1024 + 16 * 1024 + 128 * 4 + 32 * 4
    hargs = lambda Z, Cin, ncls, occ=p: (p, p, p, p, p, occ, p, null, 1, Z, 4, 4, Cin, ncls, null)
    assert lib.occ_conv3d_heads_decode_bf16x3_f32(*hargs(16, 32, 17, null)) == -1                 # null output
    assert lib.occ_conv3d_heads_decode_bf16x3_f32(*hargs(8, 32, 17)) == -3                        # Z = 8 (16 and 32 have kernels)
    assert lib.occ_conv3d_heads_decode_bf16x3_f32(*hargs(16, 16, 17)) == -3                       # Cin = 16
    assert lib.occ_conv3d_heads_decode_bf16x3_f32(*hargs(16, 32, 40)) == -3                       # > 30 classes
    # row-local Linear chains (round 4): argument checks before any launch
    assert lib.occ_linear_chain_packed_bytes(768, 256) == 768 * 256 * 4
    assert lib.occ_linear_chain_packed_bytes(192, 256) == 256 * 256 * 4                           # padded to a 256-row group
    assert lib.occ_linear_chain_pack_bf16x3(p, p, 256, 40, null) == -3                            # K % 16
    f = ctypes.c_float(1e-5)
    assert lib.occ_linear_ln_chain_bf16x3_f32(null, i64(256), p, i64(256), p, p, p, p, f, p, i64(256), p, i64(768),
                                              768, 0, 64, null) == -1                             # null input
    assert lib.occ_linear_ln_chain_bf16x3_f32(p, i64(256), p, i64(256), p, p, p, p, f, p, i64(256), p, i64(768),
                                              770, 0, 64, null) == -1                             # ldz < n2
    assert lib.occ_linear_ln_chain_bf16x3_f32(p, i64(256), p, i64(256), p, p, p, p, f, p, i64(256), p, i64(800),
                                              776, 0, 64, null) == -3                             # n2 % 32
    assert lib.occ_linear_pair_chain_bf16x3_f32(p, i64(256), p, p, null, i64(0), null, i64(192), 192, p, i64(256), 64,
                                                null) == -1                                       # null zq
    assert lib.occ_linear_pair_chain_bf16x3_f32(p, i64(256), p, p, null, i64(0), p, i64(192), 200, p, i64(256), 64,
                                                null) == -1                                       # ldzq < nq
    assert lib.occ_linear_pair_chain_bf16x3_f32(p, i64(256), p, p, null, i64(0), p, i64(192), 160, p, i64(256), 64,
                                                null) == -3                                       # nq % 64
    assert lib.occ_linear_ln_chain_bf16x3_f32(p, i64(256), p, i64(256), p, p, p, p, f, p, i64(256), p, i64(1536),
                                              1536, 0, 64, null) == -3                            # more tail columns than staged parameters
    assert lib.occ_encoder_ffn_chain_bf16x3_f32(p, i64(256), p, i64(256), p, p, p, p, f, p, p, f, p, i64(256), null,
                                                i64(0), p, i64(192), 192, null, i64(256), 64, null) == -1   # zq without zv
    assert lib.occ_encoder_ffn_chain_bf16x3_f32(p, i64(256), p, i64(256), p, p, p, p, f, p, p, f, p, i64(256), null,
                                                i64(0), p, i64(200), 200, p, i64(256), 64, null) == -3      # nq % 64
    with pytest.raises(_lib.OccAmdUnsupported):
        ext.conv1x1_pack_weight(torch.zeros(8, 32))
    with pytest.raises(_lib.OccAmdUnsupported):
        ext.stem_pack_weight(torch.zeros(64, 3, 3, 3))


def test_product_refuses_host_tensors():
    v = torch.zeros(1, 4, 8, 32)
    shapes = torch.tensor([[2, 2]])
    start = torch.tensor([0])
    loc = torch.zeros(1, 3, 8, 1, 2, 2)
    aw = torch.zeros(1, 3, 8, 1, 2)
    with pytest.raises(_lib.OccAmdError, match='no CPU fallback'):
        ext.ms_deform_attn_forward(v, shapes, start, loc, aw, im2col_step=64)
    from occnet_amd.plugin import build_head
    from tests.util import head_cfg, small_cfg
    from occnet_amd import synthetic
    g = small_cfg(bev=(4, 4), feat_shapes=((2, 2), (1, 1), (1, 1), (1, 1)), num_layers=1)
    head = build_head(head_cfg(g)).eval()
    with pytest.raises(_lib.OccAmdError, match='no CPU fallback'), torch.no_grad():
        head(synthetic.make_features(g), synthetic.make_img_metas(g))


def test_ext_loader_surface():
    from occnet_amd import ext_loader
    m = ext_loader.load_ext('_ext', ['ms_deform_attn_backward', 'ms_deform_attn_forward'])
    assert callable(m.ms_deform_attn_forward) and callable(m.ms_deform_attn_backward)
    with pytest.raises(AssertionError):
        ext_loader.load_ext('_ext', ['no_such_op'])
    from occnet_amd.plugin import (MultiScaleDeformableAttnFunction_fp16,
                                   MultiScaleDeformableAttnFunction_fp32)
    assert hasattr(MultiScaleDeformableAttnFunction_fp32, 'apply')
    assert hasattr(MultiScaleDeformableAttnFunction_fp16, 'apply')


def test_training_entry_points_validate_without_gpu():
    """Round-2 training entry points (Linear weight gradient, row gather-sum, SCA query-side preparation, backward
    with caller-provided scratch): argument checks and workspace sizing run before any launch."""
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    i64 = ctypes.c_int64
    # one partial (N*K + N floats) per row chunk; 512 blocks when the rows allow it
    ws = lib.occ_linear_wgrad_workspace_bytes(40000, 512, 256)
    assert ws > 0 and ws % ((512 * 256 + 512) * 4) == 0 and ws // ((512 * 256 + 512) * 4) == 63    # 640-row chunks
    assert lib.occ_linear_wgrad_workspace_bytes(10, 512, 256) == (512 * 256 + 512) * 4           # one chunk
    assert lib.occ_linear_wgrad_workspace_bytes(0, 512, 256) == 0
    assert lib.occ_linear_wgrad_bf16x3_f32(null, i64(8), p, i64(8), p, p, p, i64(1 << 20), 4, 8, 8, null) == -1
    assert lib.occ_linear_wgrad_bf16x3_f32(p, i64(4), p, i64(8), p, p, p, i64(1 << 20), 4, 8, 8, null) == -1
    assert b'row strides' in lib.occ_last_error()
    assert lib.occ_linear_wgrad_bf16x3_f32(p, i64(8), p, i64(8), p, p, p, i64(16), 4, 8, 8, null) == -1
    assert b'workspace too small' in lib.occ_last_error()
    idx = (ctypes.c_int64 * 4)(0, 1, -1, 2)
    ip = ctypes.cast(idx, ctypes.c_void_p)
    assert lib.occ_rows_gather_sum_f32(null, i64(16), ip, 1, p, 1, i64(4), i64(4), 4, null) == -1
    assert lib.occ_rows_gather_sum_f32(p, i64(16), ip, 1, p, 1, i64(4), i64(4), 6, null) == -1   # F % 4
    assert b'16-byte aligned' in lib.occ_last_error()
    assert lib.occ_sca_prep_forward_f32(p, i64(768), 768, ip, p, ip, p, p, 1, i64(4), 4, 4, 8, 4, null) == -3   # M=4
    assert lib.occ_sca_prep_forward_f32(p, i64(768), 768, ip, p, ip, p, p, 1, i64(4), 8, 4, 8, 3, null) == -1   # P % Z
    assert lib.occ_sca_prep_forward_f32(p, i64(512), 512, ip, p, ip, p, p, 1, i64(4), 8, 4, 8, 4, null) == -1   # short rows
    assert lib.occ_sca_prep_backward_f32(p, p, p, ip, 2, ip, p, 768, 1, i64(4), i64(2), 8, 2, 8, null) == -3
    # backward scratch: flags + counters + work list + 4 * samples row items of 12 bytes + (deterministic mode) one tile of
    # 32 x 32 + 32 64-bit words per possible split bin (more than 2 048 items); 0 for other head sizes
    B, S, M, D, L, Lq, P = 6, 30825, 8, 32, 4, 9900, 8
    need = lib.occ_ms_deform_attn_backward_workspace_bytes(B, S, M, D, L, Lq, P)
    items = 4 * (B * Lq * M * L * P)
    tiles = (items // 2048 + 1) * (32 * 32 + 32) * 8
    assert need > items * 12 + tiles and need < 1.1 * items * 12 + tiles + (64 << 20)
    assert lib.occ_ms_deform_attn_backward_workspace_bytes(B, S, M, 64, L, Lq, P) == 0
    rc = lib.occ_ms_deform_attn_backward_ws_f32(p, p, p, p, p, p, p, p, p, 1, 4, 8, 32, 1, 4, 4, 64, p, i64(16), null)
    assert rc == -1 and b'workspace too small' in lib.occ_last_error()


def test_round6_training_nodes_validate_without_gpu():
    """Round-6 training entry points (masked gradient + bias gradient pass, BatchNorm fold, dropout + residual + LayerNorm
    node): scratch sizing, argument checks before any launch, and the keep-mask hash — a HOST function of the library — against
    its numpy restatement (the restatement the GPU test derives its reference mask from)."""
    import numpy as np
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    i64, f32 = ctypes.c_int64, ctypes.c_float
    # bias_act backward: <= 512 blocks of 256 / (C / 8) rows each, one row of C partial sums per block; C % 8 == 0, C <= 2048
    assert lib.occ_bias_act_bwd_partial_floats(i64(6 * 116 * 200), 512) == 512 * 512
    assert lib.occ_bias_act_bwd_partial_floats(i64(7), 64) == 1 * 64
    assert lib.occ_bias_act_bwd_partial_floats(i64(100), 12) == 0 and lib.occ_bias_act_bwd_partial_floats(i64(100), 4096) == 0
    assert lib.occ_bias_act_bwd_nhwc_bf16(null, p, p, p, p, i64(8), 64, 1, null) == -1
    assert lib.occ_bias_act_bwd_nhwc_bf16(p, null, null, p, p, i64(8), 64, 1, null) == -1        # relu needs y and g
    assert lib.occ_bias_act_bwd_nhwc_bf16(p, null, null, p, p, i64(8), 12, 0, null) == -3        # C % 8
    assert lib.occ_conv_bn_fold_fwd_f32(null, p, p, p, p, p, p, p, 8, 8, 1, 1, null) == -1
    assert lib.occ_conv_bn_fold_bwd_f32(p, i64(8), i64(1), i64(1), i64(1), p, p, p, p, p, p, p, 0, 8, 1, 1, null) == -1
    # dropout + residual + LayerNorm: C = 256 only; <= 1024 blocks of 4 rows, 2 C partial sums per block
    assert lib.occ_dropout_add_ln_bwd_partial_floats(i64(40000), 256) == 1024 * 512
    assert lib.occ_dropout_add_ln_bwd_partial_floats(i64(5), 256) == 2 * 512
    assert lib.occ_dropout_add_ln_bwd_partial_floats(i64(5), 128) == 0
    u64 = ctypes.c_uint64
    assert lib.occ_dropout_add_ln_fwd_f32(null, p, p, p, f32(1e-5), f32(0.1), u64(1), p, p, p, i64(4), 256, null) == -1
    assert lib.occ_dropout_add_ln_fwd_f32(p, p, p, p, f32(1e-5), f32(1.0), u64(1), p, p, p, i64(4), 256, null) == -1      # p < 1
    assert lib.occ_dropout_add_ln_fwd_f32(p, p, p, p, f32(1e-5), f32(0.1), u64(1), p, p, p, i64(4), 128, null) == -3
    assert b'C = 256' in lib.occ_last_error()
    assert lib.occ_dropout_add_ln_bwd_f32(p, p, p, p, f32(0.1), u64(1), null, p, p, p, i64(4), 256, null) == -1            # p > 0 needs grad_x
    # the keep-mask hash
    seed = 0x1234567_89abcdef
    idx = np.concatenate([np.arange(4096, dtype=np.uint32), np.array([2 ** 31, 2 ** 32 - 1], dtype=np.uint32)])
    s0, s1 = np.uint32(seed & 0xffffffff), np.uint32(seed >> 32)
    with np.errstate(over='ignore'):
        h = idx ^ s0
        h ^= h >> np.uint32(16); h *= np.uint32(0x85ebca6b); h ^= h >> np.uint32(13); h *= np.uint32(0xc2b2ae35); h ^= h >> np.uint32(16)
        h += s1
        h ^= h >> np.uint32(15); h *= np.uint32(0x2c1b3c6d); h ^= h >> np.uint32(12)
    got = np.array([lib.occ_ln_dropout_hash(ctypes.c_uint32(int(i)), ctypes.c_uint32(int(s0)), ctypes.c_uint32(int(s1))) for i in idx],
                   dtype=np.uint32)
    assert np.array_equal(got, h)
    keep = (h[:4096] >= np.uint32(int(0.1 * 4294967296.0))).mean()
    assert abs(keep - 0.9) < 0.03


CHAIN_SLOTS = (2, 16, 208, 512, 608)


def _chain_split(M, slots):
    nfull, ntiles = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib.lib().occ_linear_chain_tile_split(M, slots, ctypes.byref(nfull), ctypes.byref(ntiles)) == 0
    return nfull.value, ntiles.value


@pytest.mark.parametrize("slots", CHAIN_SLOTS)
def test_linear_chain_tile_split_covers_every_row_once(slots):
    """occ_linear_chain_tile_split, the pure function behind the launch of the three chain programs: blocks [0, nfull) own
    64-row tiles, blocks [nfull, ntiles) 32-row tiles of the rows behind them (the kernel's own block -> row formula)."""
    # every boundary: around each multiple of 32 and 64 rows up to three rounds of tiles, and around the rounds themselves
    edges = set(range(1, 200))
    for r in range(0, 3 * slots + 3):
        edges.update(64 * r + d for d in (-33, -32, -31, -1, 0, 1, 31, 32, 33))
    for n64 in (slots, slots + 1, slots + slots // 2, slots + slots // 2 + 1, 2 * slots, 2 * slots + 1, 3 * slots - 1):
        edges.update(64 * n64 + d for d in (-64, -63, -1, 0, 1, 63, 64))
    halves = 0
    for M in sorted(m for m in edges if m > 0):
        nfull, ntiles = _chain_split(M, slots)
        n64 = (M + 63) // 64
        rem = n64 % slots
        half = n64 > slots and 0 < 2 * rem <= slots
        assert nfull == (n64 - rem if half else n64), (M, slots)
        # the tiles as the kernel walks them
        tiles = [(64 * b, 64) for b in range(nfull)] + [(64 * nfull + 32 * (b - nfull), 32) for b in range(nfull, ntiles)]
        assert tiles[0][0] == 0 and all(t[0] + t[1] == u[0] for t, u in zip(tiles, tiles[1:])), (M, slots)      # no gap, no overlap
        assert tiles[-1][0] < M <= tiles[-1][0] + tiles[-1][1], (M, slots)          # the last tile holds the last row, none is empty
        assert (ntiles > nfull) == half, (M, slots)                                  # half tiles exactly under the rule
        assert ntiles == nfull + ((M - 64 * nfull + 31) // 32 if half else 0), (M, slots)
        if half:
            assert nfull % slots == 0 and ntiles - nfull <= slots, (M, slots)        # whole rounds in front, one round of half tiles
        halves += half
    assert halves > 0
    lib = _lib.lib()
    n = ctypes.c_int(0)
    assert lib.occ_linear_chain_tile_split(0, slots, ctypes.byref(n), ctypes.byref(n)) == -1
    assert lib.occ_linear_chain_tile_split(64, 0, ctypes.byref(n), ctypes.byref(n)) == -1
    assert lib.occ_linear_chain_tile_split(64, slots, None, ctypes.byref(n)) == -1


def test_linear_chain_tile_split_of_the_tested_row_counts():
    """The M of tests/exact_cases.py on the 512 slots of 256 CUs: 8229 rows are 129 full tiles (blockIdx >> 3 = 0 .. 16: all
    16 rotations), chain_m_half() rows are 512 full tiles and 129 half tiles, the last with one row."""
    from tests import exact_cases as ec
    assert _chain_split(ec.CHAIN_M_FULL, 512) == (129, 129)
    assert {(b >> 3) & 15 for b in range(129)} == set(range(16))
    for cus in (256, 304, 104):
        M = ec.chain_m_half(cus)
        assert _chain_split(M, 2 * cus) == (2 * cus, 2 * cus + 129)
        assert {(b >> 3) & 15 for b in range(2 * cus, 2 * cus + 129)} == set(range(16))
        assert M - 64 * 2 * cus - 32 * 128 == 1


def test_linear_chain_refuses_rows_beyond_the_4gb_of_a_buffer_resource():
    """(M + 64) * ld * 4 >= 2^32 for any of the six leading dimensions is OccAmdUnsupported, before any launch."""
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    i64, f = ctypes.c_int64, ctypes.c_float(1e-5)
    big_m = 2 ** 22 - 64                              # (M + 64) * 256 * 4 == 2^32
    big_ld = 2 ** 20                                   # (1024 + 64) * 2^20 * 4 > 2^32

    def pair(M, lda=256, ldq=192, ldzq=192, ldzv=256):
        return lib.occ_linear_pair_chain_bf16x3_f32(p, i64(lda), p, p, p, i64(ldq), p, i64(ldzq), 192, p, i64(ldzv), M, null)

    def prog_a(M, lda=256, ldres=256, ldy=256, ldz=768):
        return lib.occ_linear_ln_chain_bf16x3_f32(p, i64(lda), p, i64(ldres), p, p, p, p, f, p, i64(ldy), p, i64(ldz), 768, 0,
                                                  M, null)

    def prog_b(M, ldy=256, ldzv=256):
        return lib.occ_encoder_ffn_chain_bf16x3_f32(p, i64(256), p, i64(256), p, p, p, p, f, p, p, f, p, i64(ldy), p, i64(192),
                                                    p, i64(192), 192, p, i64(ldzv), M, null)
    for rc in (pair(big_m), prog_a(big_m), prog_b(big_m), pair(1024, lda=big_ld), pair(1024, ldq=big_ld), pair(1024, ldzq=big_ld),
               pair(1024, ldzv=big_ld), prog_a(1024, ldres=big_ld), prog_a(1024, ldy=big_ld), prog_a(1024, ldz=big_ld),
               prog_b(1024, ldy=big_ld), prog_b(1024, ldzv=big_ld)):
        assert rc == -3 and b'4 GB' in lib.occ_last_error()
