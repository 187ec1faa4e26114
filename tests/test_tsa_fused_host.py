"""not-gpu: the float64 reference of the fused TSA gather (tests/tsa_ref.py) is anchored to oracle.model.TemporalSelfAttention,
the cases of tests/test_gpu_tsa_fused.py can tell a wrongly indexed kernel from a right one, and occ_tsa_fused_forward_f32 /
ext.tsa_fused_forward refuse bad arguments before any launch."""
import ctypes
import functools

import pytest
import torch

from occnet_amd import _lib, ext
from oracle import model as omodel
from tests.tsa_ref import (CASE_IDS, CASES, GPU_TOL, SEED, D, M, P, tsa_case, tsa_gather_ref, tsa_gather_weighted,
                           tsa_locations_weights)

i64 = ctypes.c_int64


@functools.lru_cache(maxsize=None)
def _case(i):
    B, H, W, spread = CASES[i]
    inp = tsa_case(B, H, W, SEED, spread)
    return inp, tsa_gather_ref(*inp, H, W, M, P)


@pytest.mark.parametrize("B,H,W,history", [(2, 6, 5, True), (1, 4, 7, False)], ids=["B2_history", "B1_no_history"])
def test_reference_matches_the_oracle_module(B, H, W, history):
    """Both sides are float64 runs of the same algebra (2.2e-16 measured): bound 1e-12."""
    g = torch.Generator().manual_seed(3)
    Nq, C = H * W, M * D
    tsa = omodel.TemporalSelfAttention(embed_dims=C, num_heads=M, num_levels=1, num_points=P, dropout=0.0).double().eval()
    with torch.no_grad():
        tsa.output_proj.weight.copy_(torch.eye(C, dtype=torch.float64))
        tsa.output_proj.bias.zero_()
        for lin, scale in ((tsa.sampling_offsets, 0.15), (tsa.attention_weights, 0.1)):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g, dtype=torch.float64) * scale)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g, dtype=torch.float64))
    query = torch.randn(B, Nq, C, generator=g, dtype=torch.float64)
    value = torch.randn(B * 2, Nq, C, generator=g, dtype=torch.float64) if history else None
    ref_2d = torch.rand(B * 2, Nq, 1, 2, generator=g, dtype=torch.float64)
    shapes = torch.tensor([[H, W]])
    with torch.no_grad():
        want = tsa(query, value=value, reference_points=ref_2d, spatial_shapes=shapes) - query
        # the module's own Linear outputs (its query is cat([value[:bs], query]); without history value = [query, query])
        val = torch.stack([query, query], 1).reshape(B * 2, Nq, C) if value is None else value
        qcat = torch.cat([val[:B], query], -1)
        offs, logits = tsa.sampling_offsets(qcat), tsa.attention_weights(qcat)
        v = tsa.value_proj(val).reshape(B * 2, Nq, M, D)
        got = tsa_gather_ref(v, offs, logits, ref_2d, H, W, M, P)
    assert float(offs.abs().mean()) > 0.5 and float(logits.std()) > 0.5         # not the grid initialisation
    d = float((got - want).abs().max())
    print(f"max|tsa_gather_ref - TemporalSelfAttention| = {d:.3e}")
    assert got.shape == (B, Nq, C) and d < 1e-12


def _perturbed(name, inp, H, W):
    value, offs, logits, ref_2d = (t.double() for t in inp)
    B, Nq = offs.shape[:2]
    if name == "ref_2d of entry 0 for both":
        ref_2d = ref_2d.view(B, 2, Nq, 1, 2)[:, :1].expand(B, 2, Nq, 1, 2).reshape(B * 2, Nq, 1, 2)
    elif name == "value of entry 0 for both":
        value = value.view(B, 2, Nq, M, D)[:, :1].expand(B, 2, Nq, M, D).reshape(B * 2, Nq, M, D)
    elif name == "normalisers swapped":
        H, W = W, H                                       # of the offsets only: see the gather call below
    elif name == "offset x/y swapped":
        offs = offs.view(B, Nq, -1, 2).flip(-1).reshape(B, Nq, -1)
    loc, aw = tsa_locations_weights(offs, logits, ref_2d, H, W, M, P)
    if name == "normalisers swapped":
        H, W = W, H
    if name == "softmax over all 8 samples of a head":
        aw = logits.view(B, Nq, M, 2 * P).softmax(-1).view(B, Nq, M, 2, 1, P)
        aw = aw.permute(0, 3, 1, 2, 4, 5).reshape(B * 2, Nq, M, 1, P)
    return tsa_gather_weighted(value, loc, aw, H, W, reduce="sum" if name == "sum instead of mean" else "mean")


PERTURBATIONS = ["ref_2d of entry 0 for both", "value of entry 0 for both", "normalisers swapped", "offset x/y swapped",
                 "softmax over all 8 samples of a head", "sum instead of mean"]


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_cases_tell_a_wrongly_indexed_kernel_apart(i):
    """Each indexing mistake this kernel can make moves the result by more than 100x the GPU tolerance, on every case."""
    B, H, W, _ = CASES[i]
    inp, ref = _case(i)
    assert float((_perturbed("none", inp, H, W) - ref).abs().max()) == 0.0      # the pieces compose to tsa_gather_ref
    for name in PERTURBATIONS:
        if name == "normalisers swapped" and H == W:
            continue                                       # the 1x1 map: (W, H) = (H, W), an identity by construction
        d = float((_perturbed(name, inp, H, W) - ref).abs().max())
        print(f"{CASE_IDS[i]}: {name}: max change {d:.3e}")
        assert d > 100 * GPU_TOL, name


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_case_conditions_and_f32_floor(i):
    """The GPU test cannot pass on nothing: the reference is finite and not small, a good share of the samples (but not most)
    contribute nothing because they fail the admission test -1 < h_im < H, -1 < w_im < W, few rows are exactly zero; and
    plain float32 rounding of the same algebra stays below a quarter of the GPU tolerance."""
    B, H, W, _ = CASES[i]
    inp, ref = _case(i)
    assert bool(torch.isfinite(ref).all())
    rms = float(ref.pow(2).mean().sqrt())
    loc, _ = tsa_locations_weights(inp[1].double(), inp[2].double(), inp[3].double(), H, W, M, P)
    x, y = loc[..., 0] * W - 0.5, loc[..., 1] * H - 0.5
    outside = float((~((x > -1) & (x < W) & (y > -1) & (y < H))).double().mean())
    zero_rows = float((ref.view(B, H * W, M, D) == 0).all(-1).double().mean())
    floor = float((tsa_gather_ref(*inp, H, W, M, P, dtype=torch.float32).double() - ref).abs().max())
    print(f"{CASE_IDS[i]}: rms {rms:.3f}, outside share {outside:.3f}, zero rows {zero_rows:.4f}, f32 floor {floor:.3e}")
    assert rms > 0.1
    assert 0.10 <= outside <= 0.60
    assert zero_rows < 0.10
    assert floor < GPU_TOL / 4


def _call(a, *, value=None, offs=None, logits=None, ref_2d=None, order=None, out=None, vstride=1024, so=128, sl=64,
          dims=(1, 4, 2, 2, 8, 32, 4)):
    null = ctypes.c_void_p(0)
    pick = lambda x: a if x is None else x
    return _lib.lib().occ_tsa_fused_forward_f32(pick(value), i64(vstride), pick(offs), i64(so), pick(logits), i64(sl),
                                                pick(ref_2d), null if order is None else order, pick(out), *dims, null)


def test_argument_checks_before_any_launch():
    """Every call fails on a check that comes before the launch (there is no device here, and the pointers are host memory)."""
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 12)()
    base = (ctypes.addressof(buf) + 15) & ~15              # a 16-byte aligned window of 4 floats inside the buffer
    a = ctypes.c_void_p(base)
    last = lambda: lib.occ_last_error()
    for name in ("value", "offs", "logits", "ref_2d", "out"):
        assert _call(a, **{name: null}) == -1 and b'null' in last(), name
    assert _call(a, dims=(0, 4, 2, 2, 8, 32, 4)) == -1 and b'dimension' in last()            # B = 0
    assert _call(a, dims=(1, 0, 2, 2, 8, 32, 4)) == -1 and b'dimension' in last()            # Nq = 0
    assert _call(a, dims=(1, 4, 0, 2, 8, 32, 4)) == -1 and b'dimension' in last()            # bev_h = 0
    assert _call(a, vstride=-1024) == -1 and b'negative' in last()
    assert _call(a, so=127) == -1 and b'row strides' in last()
    assert _call(a, sl=63) == -1 and b'row strides' in last()
    # 2048 x 1024 pixels of M*D*4 = 1024 bytes = 2^31 bytes: past kOobOffset = 0x7fffff00, the offset of a dead corner
    assert _call(a, dims=(1, 4, 2048, 1024, 8, 32, 4)) == -1 and b'too large' in last()
    # alignment: float2 reads of offs rows and ref_2d, 16-byte pieces of value rows, 16-byte stores
    assert _call(a, offs=ctypes.c_void_p(base + 4)) == -1 and b'offs must be 8-byte aligned' in last()
    assert _call(a, so=129) == -1 and b'even' in last()
    assert _call(a, value=ctypes.c_void_p(base + 4)) == -1 and b'value must be 16-byte aligned' in last()
    assert _call(a, value=ctypes.c_void_p(base + 8)) == -1 and b'value must be 16-byte aligned' in last()
    assert _call(a, vstride=1026) == -1 and b'value must be 16-byte aligned' in last()
    assert _call(a, ref_2d=ctypes.c_void_p(base + 4)) == -1 and b'ref_2d' in last()
    assert _call(a, out=ctypes.c_void_p(base + 8)) == -1 and b'out' in last()
    # shapes without a fused kernel; a null `order` passes every check up to here
    assert _call(a, dims=(1, 4, 2, 2, 4, 32, 4)) == -3 and b'M=4' in last()
    assert _call(a, dims=(1, 4, 2, 2, 8, 64, 4)) == -3 and b'D=64' in last()
    assert _call(a, dims=(1, 4, 2, 2, 8, 32, 8), so=256, sl=128) == -3 and b'P=8' in last()
    with pytest.raises(_lib.OccAmdUnsupported):
        _lib.check(-3, 'tsa_fused_forward')


def test_python_validation_before_any_launch():
    with pytest.raises(TypeError):
        ext.tsa_fused_forward(None, None, None, None, 2, 2, 8, 4)
    with pytest.raises(_lib.OccAmdError, match="device"):
        ext.tsa_fused_forward(torch.zeros(2, 4, 8, 32), torch.zeros(1, 4, 128), torch.zeros(1, 4, 64),
                              torch.zeros(2, 4, 1, 2), 2, 2, 8, 4)
