"""not-gpu: the float64 reference of the fused SCA gather (tests/sca_ref.py) is anchored to oracle.model.SpatialCrossAttention,
the cases of tests/test_gpu_sca_fused.py can tell a wrongly indexed kernel from a right one, and occ_sca_fused_forward_* /
ext.sca_fused_forward refuse bad arguments before any launch."""
import ctypes
import functools

import pytest
import torch

from occnet_amd import _lib, ext
from oracle import model as omodel
from tests.sca_ref import (CASE_IDS, CASES, GPU_TOL, MAPS, POINTS, D, M, case_ref, level_starts, outside_share, popcount,
                           sca_camera_mean, sca_camera_outputs, sca_case, sca_counts, sca_gather_ref, sca_locations_weights)

i64 = ctypes.c_int64


@functools.lru_cache(maxsize=None)
def _case(i):
    c = sca_case(*CASES[i])
    return c, case_ref(c)


@pytest.mark.parametrize("maps,Z,B", [("L4P8", 4, 2), ("L4P4", 2, 1), ("L1P8", 8, 2)])
def test_reference_matches_the_oracle_module(maps, Z, B):
    """sca_gather_ref on the module's own Linear outputs against oracle.model.SpatialCrossAttention (rebatch by batch 0's
    index lists, padded MSDeformableAttention3D, scatter-add, count, divide).  Both sides are float64 runs of the same
    algebra in another order: bound 1e-12, as tests/test_tsa_fused_host.py."""
    g = torch.Generator().manual_seed(5)
    NC, Nq, C = 6, 21, M * D
    shapes = torch.tensor(MAPS[maps], dtype=torch.int64)
    L, P = shapes.shape[0], POINTS[maps]
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    sca = omodel.SpatialCrossAttention(embed_dims=C, num_cams=NC, dropout=0.0, deformable_attention=dict(
        embed_dims=C, num_heads=M, num_levels=L, num_points=P)).double().eval()
    da = sca.deformable_attention
    with torch.no_grad():
        for lin in (sca.output_proj, da.value_proj):
            lin.weight.copy_(torch.eye(C, dtype=torch.float64))
            lin.bias.zero_()
        for lin, scale in ((da.sampling_offsets, 0.1), (da.attention_weights, 0.1)):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g, dtype=torch.float64) * scale)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g, dtype=torch.float64))
    query = torch.randn(B, Nq, C, generator=g, dtype=torch.float64)
    value = torch.randn(NC, S, B, C, generator=g, dtype=torch.float64)
    ref_cam = torch.rand(NC, B, Nq, Z, 2, generator=g, dtype=torch.float64) * 1.3 - 0.15
    bev_mask = torch.rand(NC, B, Nq, Z, generator=g) < 0.15            # a camera sees a query through any of its anchors
    bev_mask[:, :, :3] = False
    vis = (bev_mask.any(-1).permute(1, 2, 0).to(torch.int64) << torch.arange(NC)).sum(-1).to(torch.int32)
    with torch.no_grad():
        want = sca(query, value, value, reference_points_cam=ref_cam, bev_mask=bev_mask, spatial_shapes=shapes,
                   level_start_index=level_starts(shapes)) - query
        offs, logits = da.sampling_offsets(query), da.attention_weights(query)
        v = value.permute(2, 0, 1, 3).reshape(B * NC, S, M, D)
        got = sca_gather_ref(v, shapes, offs, logits, ref_cam, vis, P, Z)
    assert float(offs.abs().mean()) > 0.5 and float(logits.std()) > 0.5         # not the grid initialisation
    if B == 2:
        assert bool((vis[0] != vis[1]).any())
    d = float((got - want).abs().max())
    print(f"{maps} Z={Z} B={B}: max|sca_gather_ref - SpatialCrossAttention| = {d:.3e} (rms {float(want.pow(2).mean().sqrt()):.3f})")
    assert got.shape == (B, Nq, C) and float(want.abs().max()) > 0.1 and d < 1e-12


# ---- what a wrong kernel would compute ------------------------------------------------------------------------------------------
PERTURBATIONS = ["anchor p // (P//Z)", "cameras by the own batch's mask", "divisor from batch 0's mask", "normalisers swapped",
                 "offset x/y swapped", "softmax per level", "level l at level l+1's start", "value entry c*B + b",
                 "ref_cam read as [b][c]", "pair layout skipped"]


def _identity(name, c):
    """The perturbations that change nothing on a case, by construction."""
    B, NC, L, P, Z = c['B'], c['NC'], c['L'], c['P'], c['Z']
    return {"anchor p // (P//Z)": Z == 1 or Z == P,            # p // P = 0 = p % 1; p // 1 = p = p % P
            "cameras by the own batch's mask": B == 1,         # the own batch element IS element 0
            "divisor from batch 0's mask": B == 1 or NC == 1,      # one camera: 0 or 1 of them, clamped to 1
            "softmax per level": L == 1,
            "level l at level l+1's start": L == 1,            # the only level's next start is its own (wrapped)
            "value entry c*B + b": B == 1 or NC == 1,          # c*1 + 0 = 0*NC + c; 0*B + b = b*1 + 0
            "ref_cam read as [b][c]": B == 1 or NC == 1}.get(name, False)


def _perturbed(name, c):
    B, NC, Nq, S, L, P, Z = (c[k] for k in ('B', 'NC', 'Nq', 'S', 'L', 'P', 'Z'))
    value, offs, logits, ref_cam = (c[k].double() for k in ('value', 'offs', 'logits', 'ref_cam'))
    shapes, vis = c['shapes'], c['vis']
    norm_shapes = shapes
    if name == "normalisers swapped":
        norm_shapes = shapes.flip(-1)                         # of the offsets only: the gather keeps the maps
    elif name == "offset x/y swapped":
        offs = offs.view(B, Nq, -1, 2).flip(-1).reshape(B, Nq, -1)
    elif name == "ref_cam read as [b][c]":
        ref_cam = ref_cam.reshape(B, NC, Nq, Z, 2).transpose(0, 1)
    elif name == "value entry c*B + b":
        value = value.view(NC, B, S, M, D).transpose(0, 1).reshape(B * NC, S, M, D)
    elif name == "level l at level l+1's start":
        starts = level_starts(shapes)
        idx = torch.cat([(starts[(l + 1) % L] + torch.arange(int(h * w))) % S for l, (h, w) in enumerate(shapes.tolist())])
        value = value[:, idx]
    elif name == "pair layout skipped":
        # the kernel reads pixel pix of head m at [pix >> 1][m][pix & 1] of whatever memory it is given
        pad = torch.cat([value, value.new_zeros(B * NC, S & 1, M, D)], 1)
        value = ext.sca_unpair_layout(pad, S)
    loc, aw = sca_locations_weights(offs, logits, ref_cam, norm_shapes, P, Z)
    if name == "anchor p // (P//Z)":
        norm = torch.stack([shapes[:, 1], shapes[:, 0]], -1).double()
        off = offs.reshape(B, Nq, M, L, Z, P // Z, 2) / norm[None, None, None, :, None, None, :]
        loc = (ref_cam[:, :, :, None, None, :, None, :] + off[None]).reshape(NC, B, Nq, M, L, P, 2)
    elif name == "softmax per level":
        aw = logits.reshape(B, Nq, M, L, P).softmax(-1)
    per_cam = sca_camera_outputs(value, shapes, loc, aw)
    select = vis if name == "cameras by the own batch's mask" else vis[0]
    divide = vis[0] if name == "divisor from batch 0's mask" else vis
    return sca_camera_mean(per_cam, select, divide)


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_cases_tell_a_wrongly_indexed_kernel_apart(i):
    """Each indexing mistake these kernels can make moves the result by more than 100x the GPU tolerance, on every case where
    it is not an identity by construction (_identity)."""
    c, ref = _case(i)
    assert float((_perturbed("none", c) - ref).abs().max()) == 0.0             # the pieces compose to sca_gather_ref
    smallest = None
    for name in PERTURBATIONS:
        d = float((_perturbed(name, c) - ref).abs().max())
        if _identity(name, c):
            assert d == 0.0, name
            continue
        print(f"{CASE_IDS[i]}: {name}: max change {d:.3e}")
        smallest = d if smallest is None else min(smallest, d)
        assert d > 100 * GPU_TOL, name
    print(f"{CASE_IDS[i]}: smallest perturbation effect {smallest:.3e}")


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_case_conditions_and_f32_floor(i):
    """The GPU test cannot pass on nothing: see the assertions.  Two conditions have no meaning on the one-query tail and are
    asserted from two queries on: an unseen query, and a query that lacks a camera of its wave's union."""
    c, ref = _case(i)
    B, NC, Nq = c['B'], c['NC'], c['Nq']
    geo = (c['shapes'], c['offs'], c['logits'], c['ref_cam'])
    assert bool(torch.isfinite(ref).all())
    rms = float(ref.pow(2).mean().sqrt())
    outside = outside_share(*geo, c['P'], c['Z'])
    floor = float((case_ref(c, dtype=torch.float32).double() - ref).abs().max())
    rows, corners, near = sca_counts(*geo, c['vis'], c['P'], c['Z'])
    print(f"{CASE_IDS[i]}: rms {rms:.3f}, outside share {outside:.3f}, f32 floor {floor:.3e}, visible rows {rows}, "
          f"corners {corners}, near a deciding integer {near}")
    assert rms > 0.1
    assert 0.20 <= outside <= 0.60
    assert floor < GPU_TOL / 4
    assert near <= 8 and corners > 100 * near
    vis = c['vis'].to(torch.int64)
    seen0 = vis[0] != 0
    zero = (ref == 0).all(-1)                                                   # (B, Nq)
    assert not bool((zero & seen0).any())                                       # no seen query's row is all zero
    assert bool(zero[:, ~seen0].all())                                          # every unseen query's row is exactly zero
    assert rows == B * int(popcount(vis[0], NC).sum()) and rows > 0
    if Nq > 1:
        assert bool((~seen0).any())
        groups = [vis[0, s:s + 8] for s in range(0, Nq, 8)]                     # the head-major kernel's waves, order=None
        union = [functools.reduce(lambda a, b: a | b, g.tolist()) for g in groups]
        assert any(bool((g != u).any()) for g, u in zip(groups, union))         # a dead sample inside a live camera loop
        if Nq >= 24:
            assert union[0] == 0                                                # a whole wave without a camera
    if B == 2:
        differ = float((vis[0] != vis[1]).double().mean())
        print(f"{CASE_IDS[i]}: batch masks differ on {differ:.2f} of the queries")
        assert differ >= 0.20
        own = vis[1] != 0
        assert bool((seen0 & ~own).any())                                       # divisor clamped to 1
        if Nq > 2:
            assert bool((~seen0 & own).any())                                   # no camera loop: exactly 0


def test_16bit_rows_see_the_pad_pixel_and_odd_level_starts():
    """The L4P8 maps are what the pixel-pair remap needs: an odd S (a pad pixel) and levels that start at odd pixels."""
    c, _ = _case(0)
    assert c['maps'] == "L4P8" and c['S'] == 177 and c['starts'].tolist() == [0, 126, 161, 173]
    pairs = ext.sca_pair_layout(c['value'])
    assert pairs.shape[1] == 178 and torch.equal(ext.sca_unpair_layout(pairs, 177), c['value'])


# ---- argument checks ----------------------------------------------------------------------------------------------------------
def _call(a, fmt="f32", *, value=None, offs=None, logits=None, ref_cam=None, slots=None, so=512, sl=256,
          dims=(1, 6, 178, 8, 32, 4, 8, 4, 4)):
    """occ_sca_fused_forward_{f32,f16v,q16v} on host pointers: dims = (B, NC, S, M, D, L, P, Z, Nq)."""
    null = ctypes.c_void_p(0)
    pick = lambda x: a if x is None else x
    fn = getattr(_lib.lib(), {"f32": "occ_sca_fused_forward_f32", "f16": "occ_sca_fused_forward_f16v",
                              "q16": "occ_sca_fused_forward_q16v"}[fmt])
    tail = (null,) if fmt == "f32" else (null, null)
    return fn(pick(value), a, a, pick(offs), i64(so), pick(logits), i64(sl), pick(ref_cam), a, null, pick(slots), null,
              *dims, *tail)


def test_argument_checks_before_any_launch(monkeypatch):
    """Every call fails on a check that comes before the launch (there is no device here, and the pointers are host memory)."""
    monkeypatch.delenv("OCC_SCA_HEAD_MAJOR", raising=False)
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 16)()
    base = (ctypes.addressof(buf) + 15) & ~15              # a 16-byte aligned window inside the buffer
    a = ctypes.c_void_p(base)
    at = lambda n: ctypes.c_void_p(base + n)
    last = lambda: lib.occ_last_error()
    for fmt in ("f32", "f16", "q16"):
        for name in ("value", "offs", "logits", "ref_cam", "slots"):
            assert _call(a, fmt, **{name: null}) == -1 and b'null' in last(), (fmt, name)
        assert _call(a, fmt, dims=(0, 6, 178, 8, 32, 4, 8, 4, 4)) == -1 and b'dimension' in last()
        assert _call(a, fmt, dims=(1, 6, 178, 8, 32, 4, 8, 3, 4)) == -1 and b'multiple of Z' in last()
        assert _call(a, fmt, so=510) == -1 and b'row strides' in last()
        assert _call(a, fmt, sl=255) == -1 and b'row strides' in last()
        # alignment: 16-byte pieces of value rows and 16-byte stores, float2 reads of offset pairs and anchors
        for off in (4, 8):
            assert _call(a, fmt, value=at(off)) == -1 and b'value must be 16-byte aligned' in last(), (fmt, off)
            assert _call(a, fmt, slots=at(off)) == -1 and b'slots must be 16-byte aligned' in last(), (fmt, off)
        assert _call(a, fmt, ref_cam=at(4)) == -1 and b'ref_cam must be 8-byte aligned' in last()
        assert _call(a, fmt, offs=at(4)) == -1 and b'offs must be 8-byte aligned' in last()
        assert _call(a, fmt, so=513) == -1 and b'even' in last()
    assert _call(a, "f16", dims=(1, 6, 177, 8, 32, 4, 8, 4, 4)) == -1 and b'even' in last()          # S: pixel pairs
    # fp32 rows: float2 is the widest read of offs / ref_cam, logits are read one by one — these pass the alignment checks
    # and stop at the shape without a kernel
    unsupported = (1, 6, 178, 4, 32, 4, 8, 4, 4)
    assert _call(a, "f32", offs=at(8), ref_cam=at(8), logits=at(4), so=514, sl=257, dims=unsupported) == -3 and b'M=4' in last()
    # 16-bit rows, L*P = 32: 16-byte reads of four logits / four offset pairs
    for fmt in ("f16", "q16"):
        assert _call(a, fmt, offs=at(8)) == -1 and b'offs and logits must be 16-byte aligned' in last()
        assert _call(a, fmt, logits=at(4)) == -1 and b'offs and logits must be 16-byte aligned' in last()
        assert _call(a, fmt, logits=at(8)) == -1 and b'offs and logits must be 16-byte aligned' in last()
        assert _call(a, fmt, so=514) == -1 and b'multiples of 4' in last()
        assert _call(a, fmt, sl=258) == -1 and b'multiples of 4' in last()
        # L*P = 16: float2 / single reads only
        lp16 = (1, 6, 178, 4, 32, 4, 4, 4, 4)
        assert _call(a, fmt, offs=at(8), logits=at(4), ref_cam=at(8), so=258, sl=129, dims=lp16) == -3 and b'M=4' in last()
        # the head-major kernel's two 16-byte anchor loads (Z % 4 == 0); the query-major kernel and Z = 2 read float2
        monkeypatch.setenv("OCC_SCA_HEAD_MAJOR", "1")
        assert _call(a, fmt, ref_cam=at(8)) == -1 and b'ref_cam must be 16-byte aligned' in last()
        assert _call(a, fmt, ref_cam=at(8), dims=(1, 6, 178, 4, 32, 4, 8, 2, 4)) == -3 and b'M=4' in last()
        monkeypatch.setenv("OCC_SCA_HEAD_MAJOR", "0")
        assert _call(a, fmt, ref_cam=at(8), dims=(1, 6, 178, 4, 32, 4, 8, 4, 4)) == -3 and b'M=4' in last()
        monkeypatch.delenv("OCC_SCA_HEAD_MAJOR")
    # shapes without a fused kernel; aligned pointers pass every check up to here
    assert _call(a, dims=(1, 6, 178, 8, 64, 4, 8, 4, 4)) == -3 and b'D=64' in last()
    assert _call(a, dims=(1, 6, 178, 8, 32, 3, 8, 4, 4), so=384, sl=192) == -3 and b'L=3' in last()
    with pytest.raises(_lib.OccAmdUnsupported):
        _lib.check(-3, 'sca_fused_forward')


def test_python_validation_before_any_launch():
    with pytest.raises(_lib.OccAmdError, match="device"):
        z = torch.zeros
        ext.sca_fused_forward(z(6, 178, 8, 32), z(4, 2, dtype=torch.long), z(4, dtype=torch.long), z(1, 4, 512), z(1, 4, 256),
                              z(6, 1, 4, 4, 2), z(1, 4, dtype=torch.int32), 8, 4, 8)
