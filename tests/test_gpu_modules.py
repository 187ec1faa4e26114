"""-m gpu: the MI355X modules (fused HIP path through the C ABI) vs the CPU oracle, same weights,
same seeded inputs.  Tolerance: north_star's 1e-3 (fp32); observed differences are printed."""
import numpy as np
import pytest
import torch

from occnet_amd import synthetic
from tests.util import TOL, build_pair, maxdiff, small_cfg

pytestmark = pytest.mark.gpu


def _metas(g, batch=1, seed=0, jitter=0.0):
    return synthetic.make_img_metas(g, batch=batch, seed=seed, jitter=jitter)


def test_point_sampling_matches_oracle():
    import oracle.model as om
    from occnet_amd.plugin import BEVFormerEncoder
    g = dict(synthetic.BASE)
    metas = _metas(g, batch=2, jitter=1.0)
    pcr = list(g['pc_range'])
    ref_3d = om.get_reference_points(g['bev_h'], g['bev_w'], pcr[5] - pcr[2], 8, '3d', bs=2)
    rc_o, m_o = om.point_sampling(ref_3d, pcr, metas)
    enc = BEVFormerEncoder.__new__(BEVFormerEncoder)
    ref_3d_g = BEVFormerEncoder.get_reference_points(g['bev_h'], g['bev_w'], pcr[5] - pcr[2], 8, '3d',
                                                     bs=2, device='cuda')
    assert torch.equal(ref_3d_g.cpu(), ref_3d)      # host-evaluated grid: bit-identical
    rc, m, vis = BEVFormerEncoder.point_sampling(enc, ref_3d_g, pcr, metas, return_vis=True)
    m, rc, vis = m.cpu(), rc.cpu(), vis.cpu()
    # float64 from the same fp32 inputs, with the set of points whose mask the kernel's roundings cannot flip
    # (tests/train_glue_ref.py): the mask may differ from the oracle's or from float64 at an undecidable point, nowhere else
    from tests import train_glue_ref as tg
    r64 = tg.point_sampling_ref(ref_3d, torch.from_numpy(np.asarray([mt['lidar2img'] for mt in metas], dtype=np.float32)),
                                torch.from_numpy(np.asarray(metas[0]['ego2lidar'], dtype=np.float32)), pcr,
                                metas[0]['img_shape'][0][0], metas[0]['img_shape'][0][1])
    undecidable = int((~r64.decidable).sum())
    assert undecidable <= tg.POINT_CAP * m.numel()
    ratio = tg.assert_point_sampling(rc, m, vis, r64)
    mism = int((m != m_o).sum())
    print(f"bev_mask mismatches: {mism} of {m.numel()} ({undecidable} undecidable); ref_cam err / bound vs float64 {ratio:.3f}")
    assert not bool(((m != m_o) & r64.decidable).any())
    # coordinates agree wherever the point is in front of the camera (elsewhere they are x/1e-5 huge)
    front = m_o | (rc_o.abs().amax(-1) < 4.0)
    rel = ((rc - rc_o).abs() / (1.0 + rc_o.abs()))[front].max()
    print(f"ref_cam max rel diff (in front): {float(rel):.3e}")
    assert float(rel) < 1e-5
    bits = sum((m_o[c].any(-1).long() << c) for c in range(m_o.shape[0]))
    q_ok = r64.decidable.all(-1).all(0)              # queries none of whose points is undecidable
    assert not bool(((vis.long() != bits) & q_ok).any())
    rows = [int(m_o[c, 0].any(-1).sum()) for c in range(6)]
    print("visible queries per camera:", rows, "total", sum(rows))


def _run_pair(g, batch=1, prev=False, seed=0):
    prod, ora = build_pair(g, seed=seed)
    feats = synthetic.make_features(g, batch=batch, seed=seed)
    metas = _metas(g, batch=batch)
    prev_bev = None
    if prev:
        gen = torch.Generator().manual_seed(seed + 5)
        prev_bev = torch.randn(batch, g['bev_h'] * g['bev_w'], g['embed_dims'], generator=gen) * 0.5
        for m in metas:
            m['can_bus'][-1] = 0.0   # rotation by 0 degrees: identity
    with torch.no_grad():
        out_o = ora(feats, metas, prev_bev=None if prev_bev is None else prev_bev.clone())
        out_p = prod([f.cuda() for f in feats], metas,
                     prev_bev=None if prev_bev is None else prev_bev.cuda())
    torch.cuda.synchronize()
    return prod, ora, out_p, out_o


@pytest.mark.parametrize("batch", [1, 2])
def test_head_forward_matches_oracle(batch):
    g = small_cfg()
    prod, ora, out_p, out_o = _run_pair(g, batch=batch)
    for k in ('bev_embed', 'occ', 'flow'):
        d = maxdiff(out_p[k], out_o[k])
        print(f"bs={batch} {k}: shape {tuple(out_p[k].shape)} max|hip - oracle| = {d:.3e}")
        assert out_p[k].shape == out_o[k].shape
        assert d < TOL
    occ_p, _ = prod.get_occ(out_p)
    occ_o, _ = ora.get_occ(out_o)
    agree = float((occ_p.cpu() == occ_o).float().mean())
    print(f"argmax agreement {agree:.6f}")
    assert agree > 0.999


@pytest.mark.parametrize("batch,rows", [(1, "f16"), (2, "f16"), (1, "q16")])
def test_bf16_nhwc_features_take_the_direct_value_projection(batch, rows, monkeypatch):
    """Backbone-format input (bf16 NHWC maps): the SCA value projection runs straight off the maps
    (ext.value_proj_bf16_planes: ONE launch for all layers and levels; ext.value_proj_bf16 per layer when the
    layers' projections do not stack; embeddings folded into a per-(level, camera) bias) — same result as the oracle
    on the same (bf16-representable) feature values."""
    from occnet_amd import ext
    g = small_cfg()
    prod, ora = build_pair(g, seed=3)
    # (the launch count is asserted for fp16 rows; q16 rows at this small geometry take the tiled projection to fp32 +
    # ext.sca_rows_encode_q16 — more launches, same contract: parity only)
    monkeypatch.setattr(ext, "SCA_VALUES", rows)
    feats = [f.to(torch.bfloat16).float() for f in synthetic.make_features(g, batch=batch, seed=3)]
    metas = _metas(g, batch=batch)
    calls = []
    real = ext.value_proj_bf16
    real_planes = ext.value_proj_bf16_planes
    monkeypatch.setattr(ext, 'value_proj_bf16', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(ext, 'value_proj_bf16_planes',
                        lambda a, w, *r, **k: (calls.append(len(w)), real_planes(a, w, *r, **k))[1])

    def nhwc(f):
        B, N, C, h, w = f.shape
        return f.cuda().reshape(B * N, C, h, w).to(torch.bfloat16).contiguous(
            memory_format=torch.channels_last).view(B, N, C, h, w)
    with torch.no_grad():
        out_o = ora(feats, metas, prev_bev=None)
        out_p = prod([nhwc(f) for f in feats], metas, prev_bev=None)
        n_direct, n_layers_projected = len(calls), sum(calls)
        prod.transformer.use_lazy_features = False
        out_f = prod([nhwc(f) for f in feats], metas, prev_bev=None)      # flatten path on the same maps
    # every layer's projection came off the maps, in one stacked launch or one launch per layer; none on the flatten path
    assert len(calls) == n_direct
    if rows == "f16":
        assert n_layers_projected == g['num_layers'] and n_direct in (1, g['num_layers'])
    for k in ('bev_embed', 'occ', 'flow'):
        d, d2 = maxdiff(out_p[k], out_o[k]), maxdiff(out_p[k], out_f[k].cpu())
        print(f"bs={batch} {k}: direct vs oracle {d:.3e}, direct vs flatten path {d2:.3e}")
        assert d < TOL and d2 < TOL


def test_head_forward_with_history_bev():
    g = small_cfg()
    prod, ora, out_p, out_o = _run_pair(g, batch=1, prev=True)
    for k in ('bev_embed', 'occ', 'flow'):
        d = maxdiff(out_p[k], out_o[k])
        print(f"prev_bev {k}: max|hip - oracle| = {d:.3e}")
        assert d < TOL


def test_tiny_config_matches_oracle():
    """BASELINE configs[0]: 1 camera 256x256, 50x50x4 voxels (4 z-anchors, 8 points -> 2 per anchor)."""
    g = dict(synthetic.TINY, num_points=8, num_layers=2)
    prod, ora, out_p, out_o = _run_pair(g)
    for k in ('bev_embed', 'occ', 'flow'):
        d = maxdiff(out_p[k], out_o[k])
        print(f"tiny {k}: shape {tuple(out_p[k].shape)} max|hip - oracle| = {d:.3e}")
        assert d < TOL
    assert out_p['occ'].shape == (1, 50, 50, 4, 17)


def test_unfused_path_matches_fused():
    """Three execution levels agree: (a) everything fused (MFMA Linear epilogues, fused gathers, MFMA
    decoder), (b) fused gathers with library GEMMs / torch LayerNorm / MIOpen decoder, (c) the
    reference-shaped decomposition (rebatch + operator boundary)."""
    from occnet_amd.plugin import BEVFormerLayer, SpatialCrossAttention, TemporalSelfAttention
    g = small_cfg()
    prod, ora = build_pair(g)
    feats = [f.cuda() for f in synthetic.make_features(g)]
    metas = _metas(g)
    with torch.no_grad():
        a = prod(feats, metas)
        for m in prod.modules():
            if isinstance(m, BEVFormerLayer):
                m.use_fused = False
        prod.transformer.use_fused_decoder = False
        b = prod(feats, metas)
        for m in prod.modules():
            if isinstance(m, (SpatialCrossAttention, TemporalSelfAttention)):
                m.use_fused = False
        c = prod(feats, metas)
    for k in ('bev_embed', 'occ', 'flow'):
        d1, d2 = maxdiff(a[k], b[k]), maxdiff(b[k], c[k])
        print(f"all-fused vs gather-fused {k}: {d1:.3e}; gather-fused vs unfused {k}: {d2:.3e}")
        # level (a) gathers fp16 value rows (the default), (b) and (c) fp32 ones: 11 significant bits on the values
        assert d1 < 5e-4 and d2 < 2e-4


def test_gather_stats_match_oracle_count():
    """N_in / row counters of the fused kernel (used for the roofline's algorithmic bytes) equal the
    oracle's count on the same sampling locations."""
    from oracle.msda import count_inbounds_corners
    g = small_cfg(num_layers=1)
    prod, ora = build_pair(g)
    feats = synthetic.make_features(g)
    metas = _metas(g)
    stats = torch.zeros(2, dtype=torch.int64, device='cuda')
    enc = prod.transformer.encoder
    sca = enc.layers[0].attentions[1]
    sca.gather_stats = stats
    with torch.no_grad():
        prod([f.cuda() for f in feats], metas)
        ora(feats, metas)
    o_sca = ora.transformer.encoder.layers[0].attentions[1]
    rows = sum(o_sca.last_rows)
    locs = o_sca.deformable_attention.last_sampling_locations      # (6, max_len, 8, L, P, 2) padded
    n_in = 0
    shapes = torch.tensor(g['feat_shapes'])
    for c, r in enumerate(o_sca.last_rows):
        n_in += count_inbounds_corners(shapes, locs[c:c + 1, :r])
    s = stats.cpu().tolist()
    print(f"rows hip {s[0]} oracle {rows}; N_in hip {s[1]} oracle {n_in}")
    assert s[0] == rows
    assert abs(s[1] - n_in) <= max(8, n_in * 1e-5)


@pytest.mark.parametrize('name', ['base_struct_nohist', 'base_struct_hist', 'base_struct_bs2', 'tiny_struct'])
def test_product_matches_reference_golden(name):
    """HIP path vs the committed golden vectors (outputs of the reference's own module files,
    oracle/gen_golden.py) — no oracle in the loop."""
    import os
    from occnet_amd.plugin import build_head
    from tests.golden_cases import CASES, case_inputs, checksum
    from tests.util import head_cfg, randomize
    case = CASES[name]
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', f'{name}.npz'))
    head = build_head(head_cfg(case['geometry']))
    randomize(head, case['seed'])
    assert abs(checksum(head.state_dict().values()) - float(gold['weights_checksum'])) < 1e-3
    head = head.cuda().eval()
    feats, metas, prev_bev = case_inputs(case)
    assert abs(checksum(feats) - float(gold['inputs_checksum'])) < 1e-3
    with torch.no_grad():
        out = head([f.cuda() for f in feats], metas,
                   prev_bev=None if prev_bev is None else prev_bev.cuda())
    for k in ('bev_embed', 'occ', 'flow'):
        d = float(np.abs(out[k].cpu().numpy() - gold[k]).max())
        print(f"golden {name}/{k}: max|hip - reference| = {d:.3e}")
        assert d < TOL


_SCA_SHAPES = {
    "L4P8": dict(),
    "L4P4_Z4": dict(num_points=4, z_anchors=4),
    "L2P8": dict(feat_shapes=((15, 25), (8, 13))),
    "L1P8": dict(feat_shapes=((15, 25),)),
    "L4P8_Z4": dict(z_anchors=4),              # two points per z-anchor (point p pairs with anchor p % Z)
}


@pytest.mark.parametrize("shape", sorted(_SCA_SHAPES))
@pytest.mark.parametrize("values", ["f32", "f16", "q16", "f16-hm", "q16-hm"])
def test_sca_gather_kernels_match_oracle(values, shape, monkeypatch):
    """The SCA gather kernels (fp32 value rows: sca_fused_kernel; fp16 rows and q16 block-floating-point rows: sca_fused_h_kernel)
    on every (levels, points, z-anchors) combination with a fused kernel, batch 2 (the reference takes the camera
    lists of batch element 0 for every element, spatial_cross_attention.py:138-140), ragged tail (Nq = 1 444 is not
    a multiple of the 4 queries of a block), vs the oracle head."""
    from occnet_amd import ext
    kernel = values
    # "-hm": the head-major kernel (one wave = 8 queries x one head, heads dealt to the XCDs) instead of the query-major one
    monkeypatch.setenv("OCC_SCA_HEAD_MAJOR", "1" if values.endswith("-hm") else "0")
    values = values.split("-")[0]
    monkeypatch.setattr(ext, "SCA_VALUES", values)
    g = small_cfg(bev=(38, 38), num_layers=1, **_SCA_SHAPES[shape])
    prod, ora = build_pair(g, seed=31)
    feats = synthetic.make_features(g, batch=2, seed=31)
    metas = synthetic.make_img_metas(g, batch=2, seed=31, jitter=2.0)
    calls = []
    orig = ext.sca_fused_forward
    monkeypatch.setattr(ext, "sca_fused_forward", lambda *a, **k: (calls.append(a[0].dtype), orig(*a, **k))[1])
    with torch.no_grad():
        out_o = ora(feats, metas, only_bev=True)
        out_p = prod([f.cuda() for f in feats], metas, only_bev=True)
    want_dtype = {"f16": torch.float16, "q16": torch.int16, "f32": torch.float32}[values]
    assert calls and all(c == want_dtype for c in calls), calls
    d = maxdiff(out_p, out_o)
    print(f"kernel {kernel} {shape}: bev max|hip - oracle| = {d:.3e}")
    assert d < TOL


def test_sca_gather_ignores_non_finite_values_outside_the_maps():
    """corners outside the map must not be read — both gather kernels fetch them with an
    out-of-range buffer offset (hardware returns 0), so a NaN / Inf at element 0 of a value map (the address round 1's
    dummy loads hit, 0 * Inf = NaN) cannot poison border samples."""
    from occnet_amd import ext
    g = small_cfg(bev=(24, 24), num_layers=1)
    B, NC, M, D, L, P, Z = 1, 6, 8, 32, 4, 8, 8
    shapes = torch.tensor(g['feat_shapes'])
    S = int(shapes.prod(1).sum())
    start = torch.cat([shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]])
    gen = torch.Generator().manual_seed(3)
    Nq = 24 * 24
    value = torch.randn(B * NC, S, M, D, generator=gen)
    offs = torch.randn(B, Nq, M * L * P * 2, generator=gen) * 3
    logits = torch.randn(B, Nq, M * L * P, generator=gen)
    ref_cam = torch.rand(NC, B, Nq, Z, 2, generator=gen) * 1.2 - 0.1          # some anchors off the image
    vis = torch.full((B, Nq), 0b111111, dtype=torch.int32)
    args = (shapes.cuda(), start.cuda(), offs.cuda(), logits.cuda(), ref_cam.cuda(), vis.cuda(), M, L, P)
    clean = ext.sca_fused_forward(value.cuda(), *args)
    value[:, 0] = float('inf')          # pixel (0, 0) of level 0 of every camera
    value[:, 0, :, ::2] = float('nan')
    dirty = ext.sca_fused_forward(value.cuda(), *args)
    touched = ~torch.isfinite(dirty).all(-1)
    # rows that really sample pixel (0,0) of level 0 are legitimately non-finite; everything else must be
    # bit-identical to the clean run
    assert 0.0 < float(touched.float().mean()) < 0.8
    assert torch.equal(dirty[~touched], clean[~touched])
    other = ext.sca_fused_forward(value.half().cuda(), *args)          # the fp16-value kernel: same rows touched
    assert torch.equal(~torch.isfinite(other).all(-1), touched)


@pytest.mark.parametrize("feat_format", ["bf16_nhwc", "f32"])
def test_sca_fp16_values_vs_fp32_values(feat_format, monkeypatch):
    """The default fp16 value rows against OCC_SCA_VALUES=f32 and the oracle, two layers end to end: the sampling
    arithmetic is the same, the results differ by the rounding of the value elements (11 significant bits) only, and
    both stay inside the path's 1e-3 bound."""
    from occnet_amd import ext
    g = small_cfg(num_layers=2)
    prod, ora = build_pair(g, seed=33)
    feats = synthetic.make_features(g, seed=33)
    if feat_format == "bf16_nhwc":
        feats = [f.to(torch.bfloat16) for f in feats]
    metas = synthetic.make_img_metas(g)

    def dev(f):
        if feat_format == "f32":
            return f.cuda()
        B, N, C, h, w = f.shape
        return f.reshape(B * N, C, h, w).cuda().contiguous(memory_format=torch.channels_last).view(B, N, C, h, w)
    with torch.no_grad():
        out_o = ora([f.float() for f in feats], metas)
        monkeypatch.setattr(ext, "SCA_VALUES", "f32")
        exact = prod([dev(f) for f in feats], metas)
        monkeypatch.setattr(ext, "SCA_VALUES", "f16")
        half = prod([dev(f) for f in feats], metas)
        monkeypatch.setattr(ext, "SCA_VALUES", "q16")
        q16 = prod([dev(f) for f in feats], metas)
    for k in ('bev_embed', 'occ', 'flow'):
        d_exact, d_half, d_q = maxdiff(exact[k], out_o[k]), maxdiff(half[k], out_o[k]), maxdiff(q16[k], out_o[k])
        print(f"{feat_format} {k}: fp32 values {d_exact:.3e}, fp16 values {d_half:.3e}, q16 values {d_q:.3e} vs oracle; "
              f"q16 vs fp32 rows {maxdiff(q16[k], exact[k]):.3e}, fp16 vs fp32 rows {maxdiff(half[k], exact[k]):.3e}")
        assert d_exact < TOL and d_half < TOL and d_q < TOL
        assert maxdiff(half[k], exact[k]) > 0.0            # different kernels really ran
        assert maxdiff(q16[k], exact[k]) > 0.0 and maxdiff(q16[k], exact[k]) < maxdiff(half[k], exact[k])


def test_fp16_value_kernels_in_isolation():
    """The two kernels of the fp16-value mode, separately: (a) the gather on fp16 values equals the fp32-value
    gather on the same (rounded) values to fp32 accumulation noise; (b) the fp16-output value projection equals
    the fp32-output one rounded to fp16."""
    from occnet_amd import ext
    g = small_cfg(bev=(24, 24), num_layers=1)
    B, NC, M, D, L, P, Z = 2, 6, 8, 32, 4, 8, 8
    shapes = torch.tensor(g['feat_shapes'])
    S = int(shapes.prod(1).sum())
    start = torch.cat([shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]])
    gen = torch.Generator().manual_seed(5)
    Nq = 24 * 24
    value = torch.randn(B * NC, S, M, D, generator=gen).half()
    offs = torch.randn(B, Nq, M * L * P * 2, generator=gen) * 2
    logits = torch.randn(B, Nq, M * L * P, generator=gen)
    ref_cam = torch.rand(NC, B, Nq, Z, 2, generator=gen) * 1.2 - 0.1
    vis = torch.randint(0, 64, (B, Nq), generator=gen, dtype=torch.int32)
    args = (shapes.cuda(), start.cuda(), offs.cuda(), logits.cuda(), ref_cam.cuda(), vis.cuda(), M, L, P)
    a = ext.sca_fused_forward(value.cuda(), *args)
    b = ext.sca_fused_forward(value.float().cuda(), *args)
    d = maxdiff(a, b)
    print(f"fp16-value gather vs fp32 gather on the same values: {d:.3e}")
    assert d < 1e-5
    # (b) value projection
    feats = [torch.randn(NC, h, w, 256, generator=gen).to(torch.bfloat16).cuda() for h, w in g['feat_shapes']]
    rows = [f.view(-1, 256) for f in feats]
    wgt = (torch.randn(256, 256, generator=gen) / 16).cuda()
    gb = torch.randn(len(feats), NC, 256, generator=gen).cuda()
    hw = [h * w for h, w in g['feat_shapes']]
    starts = [int(v) for v in start]
    o32 = torch.empty(NC * S, 256, device='cuda')
    Sp = S + (S & 1)                      # fp16 maps are written in pixel pairs: an even number of rows per camera
    o16 = torch.zeros(NC * Sp, 256, device='cuda', dtype=torch.float16)
    ext.value_proj_bf16(rows, wgt, gb, o32, rows_per_group=hw, out_group_rows=S, out_row0=starts)
    ext.value_proj_bf16(rows, wgt, gb, o16, rows_per_group=hw, out_group_rows=Sp, out_row0=starts)
    back = ext.sca_unpair_layout(o16.view(NC, Sp, 8, 32), S)
    assert torch.equal(back, o32.half().view(NC, S, 8, 32))
    # and the pair order round-trips
    assert torch.equal(ext.sca_unpair_layout(ext.sca_pair_layout(back), S), back)
