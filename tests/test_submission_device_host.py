"""not-gpu: the device-resident submission writer's host side — the packed layout against its restatement, the byte queries,
every argument check of occ_submission_rays through the C ABI (each returns its code before any launch: this machine may
have no GPU at all), io.merge_submission_parts, the int8 rule for class ids above 127 and the float16 rounding table the GPU
test relies on."""
import ctypes
import gzip
import pickle

import numpy as np
import pytest
import torch

from occnet_amd import _lib, ext, io as oio
from tests import submission_ref as sref


def _lib64():
    lib = _lib.lib()
    return lib


def test_symbols_declared_and_exported():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name in ('occ_submission_rays', 'occ_submission_rays_bytes', 'occ_submission_rays_workspace_bytes'):
        assert name in declared and hasattr(lib, name), name
    assert lib.occ_abi_version() == _lib.ABI == 3                  # entries were added, no signature changed


@pytest.mark.parametrize('B,T,R', [(1, 1, 1), (1, 8, 14040), (3, 3, 300), (8, 8, 14040), (2, 5, 255), (1, 1, 256), (1, 2, 129)])
def test_packed_layout_matches_restatement(B, T, R):
    lib = _lib64()
    n, off_cls, off_dist, off_flow, total = sref.layout(B, T, R)
    assert ext.submission_rays_layout(B, T, R) == (n, off_cls, off_dist, off_flow, total)
    assert lib.occ_submission_rays_bytes(B, T, R) == total == ext.submission_rays_bytes(B, T, R)
    assert off_cls == 0 and off_dist % 256 == 0 and off_flow % 256 == 0 and total % 256 == 0
    assert off_dist >= n and off_flow - off_dist >= 2 * n and total - off_flow >= 4 * n       # sections do not overlap
    assert off_dist - n < 256 and off_flow - off_dist - 2 * n < 256 and total - off_flow - 4 * n < 256
    # the views of ext over a host buffer land on those offsets
    buf = torch.arange(total, dtype=torch.int64).to(torch.uint8)
    cls, dist, flow = ext.submission_rays_views(buf, B, T, R)
    assert cls.dtype == torch.int8 and dist.dtype == torch.float16 and flow.dtype == torch.float16
    assert tuple(cls.shape) == (B, T, R) and tuple(dist.shape) == (B, T, R) and tuple(flow.shape) == (B, T, R, 2)
    base = buf.data_ptr()
    assert (cls.data_ptr() - base, dist.data_ptr() - base, flow.data_ptr() - base) == (off_cls, off_dist, off_flow)


def test_byte_queries():
    lib = _lib64()
    assert lib.occ_submission_rays_bytes(1, 8, 14040) == 112384 + 224768 + 449280
    assert lib.occ_submission_rays_bytes(0, 8, 14040) == 0 and lib.occ_submission_rays_bytes(1, 0, 14040) == 0
    assert lib.occ_submission_rays_bytes(1, 8, 0) == 0
    assert lib.occ_submission_rays_workspace_bytes(1, 200, 200, 16) == (200 * 200 * 2 + 255) // 256 * 256   # uint16 masks, prediction only
    assert lib.occ_submission_rays_workspace_bytes(2, 400, 400, 32) == 2 * 400 * 400 * 4       # uint32 masks
    assert lib.occ_submission_rays_workspace_bytes(1, 6, 5, 3) == 256
    assert lib.occ_submission_rays_workspace_bytes(3, 7, 9, 20) == (3 * 7 * 9 * 4 + 255) // 256 * 256
    assert lib.occ_submission_rays_workspace_bytes(1, 200, 200, 33) == 0
    assert ext.submission_rays_workspace_bytes(1, 200, 200, 33) == 0
    assert lib.occ_submission_rays_workspace_bytes(0, 200, 200, 16) == 0
    # one grid's masks: two samples here take what the evaluator needs for the two grids of one
    assert lib.occ_submission_rays_workspace_bytes(2, 200, 200, 16) == lib.occ_ray_metrics_workspace_bytes(1, 200, 200, 16)


@pytest.mark.parametrize('B,X,Y,Z', [(1, 6, 5, 3), (3, 7, 9, 20), (1, 200, 200, 16), (2, 400, 400, 32), (1, 200, 200, 33),
                                     (0, 200, 200, 16)])
def test_workspace_queries_agree(B, X, Y, Z):
    """One formula behind the three queries: `grids` grids of B * X * Y mask words (2 bytes up to Z = 16, 4 up to 32), rounded up
    to 256 bytes; 0 where there are no masks.  The evaluator holds two grids, the writer one, the renderer one or two."""
    lib = _lib64()

    def want(batch, grids):
        if batch <= 0 or Z > 32:
            return 0
        return (grids * batch * X * Y * (2 if Z <= 16 else 4) + 255) // 256 * 256

    two = lib.occ_ray_metrics_workspace_bytes(B, X, Y, Z)
    assert two == want(B, 2)
    assert lib.occ_render_workspace_bytes(B, X, Y, Z, 1) == two
    assert lib.occ_submission_rays_workspace_bytes(2 * B, X, Y, Z) == two
    one = lib.occ_render_workspace_bytes(B, X, Y, Z, 0)
    assert one == want(B, 1) == lib.occ_submission_rays_workspace_bytes(B, X, Y, Z)
    raw = B * X * Y * (2 if Z <= 16 else 4)                       # one grid's bytes before the round-up
    if raw % 256 == 0 or one == 0:
        assert two == 2 * one
    else:                                                         # the round-up bites: two grids are rounded once, not twice
        assert two == (2 * raw + 255) // 256 * 256 and two <= 2 * one


def test_argument_checks_without_gpu():
    lib = _lib64()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f, i64 = ctypes.c_float, ctypes.c_int64

    def call(sem=p, dt=0, flow=p, origins=p, odt=0, counts=null, rays=p, voxel=0.4, free_id=16, out=p, out_bytes=1 << 20,
             ws=p, ws_bytes=1 << 20, B=1, T=2, X=4, Y=4, Z=4, R=8):
        return lib.occ_submission_rays(sem, dt, flow, origins, odt, counts, rays, f(-40.0), f(-40.0), f(-1.0), f(voxel),
                                       free_id, out, i64(out_bytes), ws, i64(ws_bytes), B, T, X, Y, Z, R, null)

    for name in ('sem', 'flow', 'origins', 'rays', 'out', 'ws'):
        assert call(**{name: null}) == -1 and b'null' in lib.occ_last_error(), name
    for dim in ('B', 'X', 'Y', 'Z', 'R'):
        assert call(**{dim: 0}) == -1 and b'dimension' in lib.occ_last_error(), dim
    assert call(B=65536) == -1 and b'dimension' in lib.occ_last_error()
    assert call(X=8192, Y=8192, Z=32, ws_bytes=1 << 40) == -1 and b'too large' in lib.occ_last_error()
    assert call(Z=33) == -3 and b'Z = 33' in lib.occ_last_error()
    with pytest.raises(_lib.OccAmdUnsupported):
        _lib.check(-3, 'submission_rays')
    assert call(T=0) == -1 and call(T=9) == -1 and b'1..8' in lib.occ_last_error()
    assert call(dt=2) == -1 and call(dt=-1) == -1 and b'class dtype' in lib.occ_last_error()
    assert call(odt=2) == -1 and call(odt=-1) == -1 and b'origins dtype' in lib.occ_last_error()
    assert call(free_id=0) == -1 and call(free_id=32) == -1 and b'1..31' in lib.occ_last_error()
    assert call(voxel=0.0) == -1 and call(voxel=-0.4) == -1 and b'voxel_size' in lib.occ_last_error()
    need = lib.occ_submission_rays_bytes(1, 2, 8)
    assert call(out_bytes=need - 1) == -1 and b'output too small' in lib.occ_last_error()
    need_ws = lib.occ_submission_rays_workspace_bytes(1, 4, 4, 4)
    assert call(ws_bytes=need_ws - 1) == -1 and b'workspace too small' in lib.occ_last_error()
    odd = ctypes.c_void_p(p.value + 1)
    assert call(out=odd) == -1 and call(ws=odd) == -1 and b'aligned' in lib.occ_last_error()


def test_ext_and_writer_refuse_host_tensors():
    from occnet_amd.metrics import SubmissionWriter
    sem = torch.full((1, 6, 5, 3), 16, dtype=torch.uint8)
    flow = torch.zeros(1, 6, 5, 3, 2)
    with pytest.raises(_lib.OccAmdError, match='no CPU fallback'):
        ext.submission_rays(sem, flow, torch.zeros(1, 1, 3), torch.zeros(4, 3), [0.0, 0.0, 0.0], 0.5)
    w = SubmissionWriter([0, 0, 0, 3.0, 2.5, 1.5], 0.5, rays=np.zeros((4, 3), np.float32), device='cpu')
    assert w.occ_size == [6, 5, 3]
    with pytest.raises(_lib.OccAmdError, match='no CPU fallback'):
        w.add('a', sem, flow, torch.zeros(1, 1, 3))
    with pytest.raises(ValueError, match='depth'):
        SubmissionWriter([0, 0, 0, 3.0, 2.5, 1.5], 0.5, depth=0, device='cpu')


def _part(path, tokens):
    rows = {t: {'pcd_cls': np.full(3, i, np.int8), 'pcd_dist': np.full(3, i, np.float16),
                'pcd_flow': np.full((3, 2), i, np.float16)} for i, t in tokens}
    with open(path, 'wb') as f:
        f.write(gzip.compress(pickle.dumps(rows), mtime=0))
    return str(path)


def test_merge_submission_parts_order_and_duplicates(tmp_path):
    from occnet_amd.dist import shard_indices
    tokens = [f'tok{i}' for i in range(7)]
    world = 3
    parts = [_part(tmp_path / f'part{r}.gz', [(i, tokens[i]) for i in shard_indices(len(tokens), r, world)])
             for r in range(world)]
    sub = oio.read_submission(oio.merge_submission_parts(parts, str(tmp_path / 'rr')))
    assert list(sub['results']) == tokens                                           # round-robin default = dataset order
    assert {k: v for k, v in sub.items() if k != 'results'} == oio.SUBMISSION_HEADER
    for i, t in enumerate(tokens):
        assert int(sub['results'][t]['pcd_cls'][0]) == i and sub['results'][t]['pcd_flow'].shape == (3, 2)
    # the merged file is the one a single writer of all samples in that order writes
    whole = oio.write_submission({t: sub['results'][t] for t in tokens}, str(tmp_path / 'whole'))
    with open(whole, 'rb') as a, open(tmp_path / 'rr' / 'submission.gz', 'rb') as b:
        assert a.read() == b.read()
    # an explicit order and a header of the caller's
    order = tokens[::-1]
    sub = oio.read_submission(oio.merge_submission_parts(parts, str(tmp_path / 'rev'), header={'method': 'm'}, order=order))
    assert list(sub['results']) == order and sub['method'] == 'm' and sorted(sub) == ['method', 'results']
    # 7 samples on 3 ranks: the sharding wrapped tok0 and tok1 onto ranks 1 and 2, and the merge dropped those repeats
    assert [len(shard_indices(7, r, 3)) for r in range(3)] == [3, 3, 3]
    # ... but a repeat whose rows differ is an error, and so is a token held twice anywhere else
    bad = _part(tmp_path / 'bad.gz', [(1, 'tok1'), (4, 'tok4'), (5, 'tok0')])
    with pytest.raises(ValueError, match='tok0'):
        oio.merge_submission_parts([parts[0], bad, parts[2]], str(tmp_path / 'x'))
    six = [_part(tmp_path / f'six{r}.gz', [(i, tokens[i]) for i in shard_indices(6, r, 3)]) for r in range(3)]
    assert list(oio.read_submission(oio.merge_submission_parts(six, str(tmp_path / 'six')))['results']) == tokens[:6]
    dup = _part(tmp_path / 'dup.gz', [(3, 'tok3')])
    with pytest.raises(ValueError, match='tok3'):
        oio.merge_submission_parts(six + [dup], str(tmp_path / 'x'))
    with pytest.raises(ValueError, match='tok3'):
        oio.merge_submission_parts(six + [dup], str(tmp_path / 'x'), order=tokens[:6])
    # an order that leaves a token out, names a stranger, or names one twice
    # part sizes that no round-robin sharding produces need an explicit order
    lop = [_part(tmp_path / 'a.gz', [(0, 'a')]), _part(tmp_path / 'b.gz', [(1, 'b'), (2, 'c'), (3, 'd')])]
    with pytest.raises(ValueError, match='round-robin'):
        oio.merge_submission_parts(lop, str(tmp_path / 'x'))
    assert list(oio.read_submission(oio.merge_submission_parts(lop, str(tmp_path / 'y'), order='abcd'))['results']) == list('abcd')


def test_class_ids_above_127_wrap():
    """ids 0..127: what astype(np.int8) on the float row defines; 128..255: two's-complement wrap, id - 256."""
    ids = np.arange(256)
    got = sref.cls_int8(ids)
    assert got.dtype == np.int8
    assert np.array_equal(got[:128], ids[:128].astype(np.float32).astype(np.int8))
    assert np.array_equal(got[128:].astype(np.int64), ids[128:] - 256)
    assert np.array_equal(got, ids.astype(np.uint8).view(np.int8))
    assert np.array_equal(sref.cls_int8(np.array([300, -3, 2 ** 40 + 5])), np.array([44, -3, 5], np.int8))


# float32 input -> float16 bits, round to nearest even, overflow to inf, gradual underflow: IEEE 754 binary16
F16_EDGES = [(65504.0, 0x7bff), (65519.996, 0x7bff), (65520.0, 0x7c00), (2049.0, 0x6800), (2051.0, 0x6802),
             (2.0 ** -24, 0x0001), (2.0 ** -25, 0x0000), (1e-8, 0x0000), (-0.0, 0x8000), (float('inf'), 0x7c00),
             (float('-inf'), 0xfc00)]


def test_float16_rounding_table_is_numpys():
    with np.errstate(over='ignore'):
        got = np.array([v for v, _ in F16_EDGES], np.float32).astype(np.float16).view(np.uint16)
    assert [int(g) for g in got] == [b for _, b in F16_EDGES]
    assert np.float32(65519.996) < np.float32(65520.0)             # the float32 nearest to it is still below the tie
