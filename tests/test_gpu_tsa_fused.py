"""-m gpu: the fused temporal self-attention gather (ext.tsa_fused_forward -> occ_tsa_fused_forward_f32) against the float64
reference of tests/tsa_ref.py, in every calling mode of the wrapper.  Every test is a few launches on maps of at most 168
pixels; the properties of the cases themselves are asserted on the CPU in tests/test_tsa_fused_host.py."""
import functools

import pytest
import torch

from occnet_amd.synthetic import bev_tile_order
from tests.tsa_ref import CASE_IDS, CASES, GPU_TOL, SEED, D, M, P, tsa_case, tsa_gather_ref

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(i):
    """CPU inputs, their device copies and the float64 reference of case i, computed once and never written to."""
    B, H, W, spread = CASES[i]
    inp = tsa_case(B, H, W, SEED, spread)
    return inp, tuple(t.cuda() for t in inp), tsa_gather_ref(*inp, H, W, M, P)


def _idx(B, H, W):
    return next(i for i, c in enumerate(CASES) if c[:3] == (B, H, W))


def _err(out, ref):
    return float((out.double().cpu() - ref).abs().max())


def _randperm32(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed)).to(torch.int32)


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_matches_reference(i):
    from occnet_amd import ext
    B, H, W, _ = CASES[i]
    _, (value, offs, logits, ref_2d), ref = _case(i)
    out = ext.tsa_fused_forward(value, offs, logits, ref_2d, H, W, M, P)
    d = _err(out, ref)
    print(f"{CASE_IDS[i]}: max|hip - reference(f64)| = {d:.3e}")
    assert out.shape == (B, H * W, M * D) and out.dtype == torch.float32
    assert d < GPU_TOL


@pytest.mark.parametrize("B,H,W", [(1, 9, 7), (2, 9, 7)], ids=["B1_stride0_alias", "B2_stack"])
def test_shared_queue(B, H, W):
    """No history BEV: both queue entries are one projected map (B = 1: value_bt_stride = 0; B > 1: stacked)."""
    from occnet_amd import ext
    (value, offs, logits, ref_2d), (_, offs_d, logits_d, ref_d), _ = _case(_idx(B, H, W))
    Nq = H * W
    v = value.view(B, 2, Nq, M, D)[:, 1].contiguous()                       # (B, Nq, M, D)
    stacked = torch.stack([v, v], 1).reshape(B * 2, Nq, M, D)
    ref = tsa_gather_ref(stacked, offs, logits, ref_2d, H, W, M, P)
    out = ext.tsa_fused_forward(v.cuda(), offs_d, logits_d, ref_d, H, W, M, P, shared_queue=True)
    d = _err(out, ref)
    print(f"shared_queue B={B}: max|hip - reference(f64)| = {d:.3e}")
    assert d < GPU_TOL
    if B == 1:      # the same arithmetic on the same numbers, read through one buffer or through two
        assert torch.equal(out, ext.tsa_fused_forward(stacked.cuda(), offs_d, logits_d, ref_d, H, W, M, P))


@pytest.mark.parametrize("B,H,W", [(1, 12, 14), (2, 9, 7), (1, 5, 31)], ids=["B1_12x14", "B2_9x7", "B1_5x31"])
@pytest.mark.parametrize("kind", ["random", "tiles"])
def test_order_only_decides_which_wave_computes_a_row(B, H, W, kind):
    from occnet_amd import ext
    _, (value, offs, logits, ref_2d), _ = _case(_idx(B, H, W))
    Nq = H * W
    order = _randperm32(Nq, 11) if kind == "random" else torch.from_numpy(bev_tile_order(H, W))
    assert order.dtype == torch.int32 and torch.equal(order.long().sort().values, torch.arange(Nq))
    plain = ext.tsa_fused_forward(value, offs, logits, ref_2d, H, W, M, P)
    order = order.cuda()
    # the result's future storage holds NaN: a row that no wave writes cannot pass by luck
    junk = torch.full((B, Nq, M * D), float('nan'), device='cuda')
    del junk
    out = ext.tsa_fused_forward(value, offs, logits, ref_2d, H, W, M, P, order=order)
    assert not bool(torch.isnan(out).any())
    assert torch.equal(out, plain)


@pytest.mark.parametrize("B,H,W", [(1, 12, 14), (2, 9, 7)], ids=["B1", "B2"])
@pytest.mark.parametrize("cols", [192, 200])
def test_column_slices_of_one_linear_output(B, H, W, cols):
    """offs / logits as column slices of one wider Linear output (how the production callers pass them), without and with
    trailing pad columns."""
    from occnet_amd import ext
    _, (value, offs, logits, ref_2d), _ = _case(_idx(B, H, W))
    lin = torch.full((B, H * W, cols), float('nan'), device='cuda')
    lin[..., :128] = offs
    lin[..., 128:192] = logits
    o, l = lin[..., :128], lin[..., 128:192]
    assert not o.is_contiguous() and o.stride(1) == cols and l.data_ptr() == lin.data_ptr() + 512
    out = ext.tsa_fused_forward(value, o, l, ref_2d, H, W, M, P)
    assert torch.equal(out, ext.tsa_fused_forward(value, offs, logits, ref_2d, H, W, M, P))


@pytest.mark.parametrize("r0,r1", [(3, 8), (5, 6)], ids=["rows_3_to_7", "one_row"])
def test_row_band(r0, r1):
    """value_rows: the queries are rows r0 .. r1-1 of the BEV, the value maps the whole BEV."""
    from occnet_amd import ext
    B, H, W = 1, 12, 14
    (value_c, offs_c, logits_c, ref_c), (value, offs, logits, ref_2d), _ = _case(_idx(B, H, W))
    q0, q1 = r0 * W, r1 * W
    n = q1 - q0
    full = ext.tsa_fused_forward(value, offs, logits, ref_2d, H, W, M, P)
    band = (offs[:, q0:q1], logits[:, q0:q1], ref_2d[:, q0:q1].contiguous())
    out = ext.tsa_fused_forward(value, *band, H, W, M, P, value_rows=H * W)
    assert out.shape == (1, n, M * D)
    assert torch.equal(out, full[:, q0:q1])
    junk = torch.full((1, n, M * D), float('nan'), device='cuda')
    del junk
    permuted = ext.tsa_fused_forward(value, *band, H, W, M, P, value_rows=H * W, order=_randperm32(n, 12).cuda())
    assert torch.equal(permuted, out)
    ref = tsa_gather_ref(value_c, offs_c[:, q0:q1], logits_c[:, q0:q1], ref_c[:, q0:q1], H, W, M, P)
    d = _err(out, ref)
    print(f"band rows {r0}..{r1 - 1}: max|hip - reference(f64)| = {d:.3e}")
    assert d < GPU_TOL


def test_non_finite_locations_contribute_nothing():
    """A sample whose location is +-Inf or NaN fails the admission test (csrc/common.h bilinear_terms: `top` / `bot` carry
    `adm`, every corner flag is an AND with one of them): weight 0 and the dead offset on all four corners, no load."""
    from occnet_amd import ext
    B, H, W = 1, 12, 14
    (value_c, offs_c, logits_c, ref_c), (value, _, logits, ref_2d), _ = _case(_idx(B, H, W))
    offs_c = offs_c.clone()
    o = offs_c.view(B, H * W, M, 2, P, 2)
    inf, nan = float('inf'), float('nan')
    o[0, 20, 0:4] = inf                                   # heads 0-3: all 8 samples
    o[0, 20, 5, 0, 1, 0] = inf                            # head 5: one sample, x only
    o[0, 77, 2] = -inf
    o[0, 77, 6, 1] = -inf                                 # head 6: every sample of queue entry 1
    o[0, 150, 7] = nan
    o[0, 150, 1, 0, 2, 1] = nan
    o[0, 150, 3, :, :, 0] = nan                           # head 3: all 8 samples through x alone
    dead = [(20, 0), (20, 1), (20, 2), (20, 3), (77, 2), (150, 7), (150, 3)]
    ref = tsa_gather_ref(value_c, offs_c, logits_c, ref_c, H, W, M, P)
    assert bool(torch.isfinite(ref).all())
    out = ext.tsa_fused_forward(value, offs_c.cuda(), logits, ref_2d, H, W, M, P)
    assert bool(torch.isfinite(out).all())
    d = _err(out, ref)
    print(f"non-finite offsets: max|hip - reference(f64)| = {d:.3e}")
    assert d < GPU_TOL
    rows, rows_ref = out.view(H * W, M, D), ref.view(H * W, M, D)
    for q, m in dead:
        assert float(rows[q, m].abs().max()) == 0.0 and float(rows_ref[q, m].abs().max()) == 0.0, (q, m)
    for q, m in [(20, 5), (77, 6), (150, 1)]:             # partly dead heads still gather their live samples
        assert float(rows_ref[q, m].abs().max()) > 0.0 and float(rows[q, m].abs().max()) > 0.0, (q, m)


def test_refusals_launch_nothing():
    from occnet_amd import ext
    from occnet_amd._lib import OccAmdError
    B, H, W = 2, 9, 7
    Nq = H * W
    _, (value, offs, logits, ref_2d), _ = _case(_idx(B, H, W))
    f = lambda v=value, o=offs, l=logits, r=ref_2d, **kw: ext.tsa_fused_forward(v, o, l, r, H, W, M, P, **kw)
    perm = _randperm32(Nq, 13)
    with pytest.raises(OccAmdError, match="order"):       # what torch.randperm returns: the kernel would read its low and
        f(order=perm.long().cuda())                       # high words as two indices
    with pytest.raises(OccAmdError, match="order"):
        f(order=perm[:-1].contiguous().cuda())
    with pytest.raises(OccAmdError, match="order"):
        f(order=perm)                                     # on the CPU
    with pytest.raises(OccAmdError, match="order"):
        f(order=torch.stack([perm, perm], 1).cuda()[:, 0])          # every second int32
    wide = torch.zeros(B, Nq, 194, device='cuda')
    odd = torch.zeros(B, Nq, 193, device='cuda')
    with pytest.raises(OccAmdError, match="even row stride"):
        f(o=odd[..., :128])
    with pytest.raises(OccAmdError, match="8-byte aligned"):
        f(o=wide[..., 1:129])
    assert f(o=wide[..., 2:130]).shape == (B, Nq, M * D)  # an even column of an even-stride buffer is fine
    flat = torch.zeros(value.numel() + 4, device='cuda')
    with pytest.raises(OccAmdError, match="16-byte aligned"):
        f(v=flat[1:1 + value.numel()].view(value.shape))
    with pytest.raises(OccAmdError, match="band needs B == 1"):
        f(value_rows=Nq)
    with pytest.raises(OccAmdError, match="ref_2d"):
        f(r=ref_2d[:B].contiguous())
    with pytest.raises(OccAmdError, match="ref_2d"):
        f(r=ref_2d.view(B * 2, Nq, 2))
    torch.cuda.synchronize()


def test_tsa_fused_never_reads_corners_outside_the_map():
    """A corner outside its map must not be loaded at all: non-finite values at pixel 0 of both BEV value maps may only show
    up in rows that really sample that pixel; every other row is bit-identical to the clean run."""
    from occnet_amd import ext
    g = torch.Generator().manual_seed(22)
    B, M, D, P, bh, bw = 1, 8, 32, 4, 12, 14
    Nq = bh * bw
    value = torch.randn(B * 2, Nq, M, D, generator=g)
    offs = torch.randn(B, Nq, M * 2 * P * 2, generator=g) * 4.0
    logits = torch.randn(B, Nq, M * 2 * P, generator=g)
    ref = torch.rand(B * 2, Nq, 1, 2, generator=g)
    args = (offs.cuda(), logits.cuda(), ref.cuda(), bh, bw, M, P)
    clean = ext.tsa_fused_forward(value.cuda(), *args).view(B, Nq, M, D)
    value[:, 0] = float('inf')
    value[:, 0, :, ::2] = float('nan')
    dirty = ext.tsa_fused_forward(value.cuda(), *args).view(B, Nq, M, D)
    touched = ~torch.isfinite(dirty).all(-1)
    assert 0.0 < float(touched.float().mean()) < 0.6
    assert torch.equal(dirty[~touched], clean[~touched])
    # rows that cannot reach pixel (0, 0): all of a head's 8 samples at h_im >= 1 or w_im >= 1
    o = offs.view(B, Nq, M, 2, P, 2)
    lx = (ref.view(B, 2, Nq, 1, 1, 2)[..., 0].permute(0, 2, 3, 1, 4) + o[..., 0] / bw) * bw - 0.5   # (B,Nq,M,2,P)
    ly = (ref.view(B, 2, Nq, 1, 1, 2)[..., 1].permute(0, 2, 3, 1, 4) + o[..., 1] / bh) * bh - 0.5
    may = ((lx > -1) & (lx < 1) & (ly > -1) & (ly < 1)).flatten(3).any(-1)
    assert not bool((touched.cpu() & ~may).any())
