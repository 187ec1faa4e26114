"""not-gpu: the renderer's host side — vis.view_rays against the projection it inverts, every argument check of
occ_render_views / occ_render_bev through the C ABI (each returns its code before any launch: this machine may have no GPU at
all, and on one that has, a call that passed them would launch on host pointers: only refused calls are made), the workspace
query, vis.save_png and OccRenderer.mosaic on CPU tensors."""
import ctypes
import struct
import zlib

import numpy as np
import pytest
import torch

from occnet_amd import _lib, ext, synthetic, vis


# ---- view_rays --------------------------------------------------------------------------------------------------------------
def _metas():
    metas = synthetic.make_img_metas(synthetic.BASE, batch=2, seed=3, jitter=1.0)
    c, s = np.cos(0.02), np.sin(0.02)
    metas[1]['ego2lidar'] = np.array([[c, -s, 0, -0.94], [s, c, 0, 0.01], [0, 0, 1, -1.84], [0, 0, 0, 1.0]])
    return metas


@pytest.mark.parametrize('render_hw', [(928, 1600), (232, 400), (7, 13)])
def test_view_rays_rebuild_projected_points(render_hw):
    metas = _metas()
    rays = vis.view_rays64(metas, render_hw)
    assert rays.shape == (2, 6, 12) and rays.dtype == np.float64
    rng = np.random.default_rng(11)
    h, w = render_hw
    seen = 0
    for b, meta in enumerate(metas):
        for v, l2i in enumerate(meta['lidar2img']):
            M = np.asarray(l2i, np.float64) @ np.asarray(meta['ego2lidar'], np.float64)
            pts = rng.uniform([-40, -40, -1], [40, 40, 5.4], size=(200, 3))
            proj = pts @ M[:3, :3].T + M[:3, 3]
            front = proj[:, 2] > 0.5
            pts, proj = pts[front], proj[front]
            seen += len(pts)
            depth = proj[:, 2]
            H_img, W_img = meta['img_shape'][v][:2]
            px = proj[:, 0] / depth * (w / W_img)                     # pixel coordinates of the RENDERED image
            py = proj[:, 1] / depth * (h / H_img)
            o, D = rays[b, v, :3], rays[b, v, 3:].reshape(3, 3)
            back = o + depth[:, None] * (np.stack([px, py, np.ones_like(px)], -1) @ D.T)
            err = np.abs(back - pts).max() / np.abs(pts).max()
            assert err < 1e-9, (b, v, err)
    assert seen > 1000
    # rounded once
    got = vis.view_rays(metas, render_hw)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), rays.astype(np.float32))
    # an explicit image size is the default one here
    assert np.array_equal(vis.view_rays64(metas, render_hw, img_hw=(928, 1600)), rays)


def test_view_rays_refuses_a_projective_matrix():
    metas = _metas()
    metas[0]['lidar2img'][2][3] = [0.0, 0.0, 1e-3, 1.0]
    with pytest.raises(ValueError, match='affine'):
        vis.view_rays(metas, (8, 8))
    metas = _metas()
    metas[0]['lidar2img'][2][3] = [0.0, 0.0, 0.0, 1.0 + 5e-7]         # within 1e-6: taken
    vis.view_rays(metas, (8, 8))


# ---- the C ABI without a GPU --------------------------------------------------------------------------------------------------
def test_symbols_declared_and_exported():
    lib = _lib.lib()
    declared = _lib.declared_symbols()
    for name in ('occ_render_views', 'occ_render_bev', 'occ_render_workspace_bytes'):
        assert name in declared and hasattr(lib, name), name
    assert lib.occ_abi_version() == _lib.ABI == 3                  # entries were added, no signature changed


def test_workspace_query():
    q = _lib.lib().occ_render_workspace_bytes
    assert q.restype is ctypes.c_int64
    assert q(1, 200, 200, 16, 0) == (200 * 200 * 2 + 255) // 256 * 256                # uint16 masks, prediction only
    assert q(1, 200, 200, 16, 1) == 200 * 200 * 2 * 2
    assert q(1, 200, 200, 17, 0) == 200 * 200 * 4                                     # uint32 from Z = 17
    assert q(2, 400, 400, 32, 1) == 2 * 400 * 400 * 4 * 2
    assert q(1, 5, 6, 4, 0) == 256 and q(1, 5, 6, 4, 1) == 256 and q(3, 7, 5, 17, 1) == (3 * 7 * 5 * 8 + 255) // 256 * 256
    assert q(1, 200, 200, 33, 0) == 0 and q(0, 200, 200, 16, 0) == 0 and q(1, 0, 200, 16, 0) == 0 and q(1, 2, 2, 0, 1) == 0
    assert ext.render_workspace_bytes(1, 200, 200, 16) == q(1, 200, 200, 16, 0)
    assert ext.render_workspace_bytes(1, 200, 200, 32, diff=True) == q(1, 200, 200, 32, 1)
    assert ext.render_workspace_bytes(1, 200, 200, 33) == 0


def test_argument_checks_without_gpu():
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f, i64 = ctypes.c_float, ctypes.c_int64
    err = lib.occ_last_error

    def views(sem=p, dt=0, gt=null, gdt=0, cams=p, frames=null, Hs=0, Ws=0, pal=p, cat=p, voxel=0.5, free_id=16, far=100.0,
              tol=2.0, alpha=160, bg=0, label=p, depth=p, rgb=p, ws=p, ws_bytes=1 << 20, B=1, V=2, X=4, Y=4, Z=4, h=8, w=8):
        return lib.occ_render_views(sem, dt, gt, gdt, cams, frames, Hs, Ws, pal, cat, f(-1.5), f(-1.0), f(-0.5), f(voxel), free_id,
                                    f(far), f(tol), alpha, bg, label, depth, rgb, ws, i64(ws_bytes), B, V, X, Y, Z, h, w, null)

    def bev(sem=p, dt=0, gt=null, gdt=0, pal=p, cat=p, free_id=16, bg=0, label=p, rgb=p, ws=p, ws_bytes=1 << 20, B=1, X=4, Y=4,
            Z=4):
        return lib.occ_render_bev(sem, dt, gt, gdt, pal, cat, free_id, bg, label, rgb, ws, i64(ws_bytes), B, X, Y, Z, null)

    for call, what in ((views, b'render_views'), (bev, b'render_bev')):
        for name, word in (('sem', b'(sem)'), ('ws', b'(workspace)'), ('pal', b'palette')):
            assert call(**{name: null}) == -1 and b'null' in err() and word in err() and what in err(), (what, name, err())
        assert call(gt=p, cat=null) == -1 and b'cat_palette' in err()
        for dim in ('B', 'X', 'Y', 'Z'):
            assert call(**{dim: 0}) == -1 and b'dimension' in err(), dim
            assert call(**{dim: -1}) == -1 and b'dimension' in err(), dim
        assert call(X=8192, Y=8192, Z=32, ws_bytes=1 << 40) == -1 and b'too large' in err()
        assert call(Z=33) == -3 and b'Z = 33' in err() and what in err()
        assert call(Z=33, sem=null, ws=null) == -3                       # reported before the pointer checks
        assert call(dt=2) == -1 and call(dt=-1) == -1 and b'sem_dtype' in err()
        assert call(gt=p, gdt=2) == -1 and b'sem_gt_dtype' in err()
        assert call(free_id=0) == -1 and call(free_id=32) == -1 and b'free_id' in err()
        assert call(bg=-1) == -1 and call(bg=1 << 24) == -1 and b'bg_rgb' in err()
        for diff, need in ((null, lib.occ_render_workspace_bytes(1, 4, 4, 4, 0)), (p, lib.occ_render_workspace_bytes(1, 4, 4, 4, 1))):
            assert call(gt=diff, ws_bytes=need - 1) == -1 and b'workspace too small' in err()
        assert call(X=40, Y=40, ws_bytes=40 * 40 * 2 * 2 - 1, gt=p) == -1 and b'workspace too small' in err()
        assert call(ws=ctypes.c_void_p(p.value + 1)) == -1 and b'aligned' in err()
    with pytest.raises(_lib.OccAmdUnsupported):
        _lib.check(-3, 'render_views')
    # the views' own arguments
    assert views(cams=null) == -1 and b'(cams)' in err()
    assert views(label=null, depth=null, rgb=null) == -1 and b'at least one' in err()
    assert bev(label=null, rgb=null) == -1 and b'at least one' in err()
    for dim in ('V', 'h', 'w'):
        assert views(**{dim: 0}) == -1 and b'dimension' in err(), dim
    assert views(B=256, V=256, ws_bytes=1 << 30) == -1 and b'dimension' in err()
    assert views(h=16385) == -1 and views(w=16385) == -1 and b'dimension' in err()
    assert views(frames=p, Hs=0, Ws=4) == -1 and views(frames=p, Hs=4, Ws=0) == -1 and b'Hs' in err()
    assert views(voxel=0.0) == -1 and views(voxel=-0.5) == -1 and b'voxel_size' in err()
    assert views(far=0.0) == -1 and views(far=-1.0) == -1 and views(far=float('nan')) == -1 and b'far' in err()
    assert views(far=float('inf')) == -1 and b'far' in err()
    assert views(tol=-1.0) == -1 and views(tol=float('nan')) == -1 and b'tol' in err()
    assert views(alpha=-1) == -1 and views(alpha=257) == -1 and b'alpha' in err()
    assert views(depth=ctypes.c_void_p(p.value + 2)) == -1 and b'aligned' in err()


def test_ext_and_renderer_refuse_host_tensors():
    sem = torch.full((1, 6, 5, 3), 16, dtype=torch.uint8)
    with pytest.raises(_lib.OccAmdError, match='no CPU fallback'):
        ext.render_views(sem, torch.zeros(1, 1, 12), [0.0, 0.0, 0.0], 0.5, (4, 4))
    with pytest.raises(_lib.OccAmdError, match='no CPU fallback'):
        ext.render_bev(sem)
    r = vis.OccRenderer([0, 0, 0, 3.0, 2.5, 1.5], 0.5, size=(4, 6), device='cpu')
    assert r.occ_size == [6, 5, 3] and r.size == (4, 6)
    with pytest.raises(_lib.OccAmdError, match='no CPU fallback'):
        r.bev(sem)
    with pytest.raises(_lib.OccAmdError, match='no CPU fallback'):
        r.enqueue('a', sem, synthetic.make_img_metas(synthetic.TINY))
    with pytest.raises(ValueError, match='depth'):
        vis.OccRenderer([0, 0, 0, 3.0, 2.5, 1.5], 0.5, depth=0, device='cpu')
    with pytest.raises(ValueError, match='palette'):
        vis.OccRenderer([0, 0, 0, 3.0, 2.5, 1.5], 0.5, palette=np.zeros((17, 3), np.uint8), device='cpu')


def test_default_palette():
    pal = vis.default_palette()
    assert pal.shape == (256, 3) and pal.dtype == np.uint8
    assert len({tuple(c) for c in pal[:18]}) == 18                      # the named classes are told apart
    assert vis.category_palette().shape == (6, 3) and vis.category_palette().dtype == np.uint8


# ---- save_png -----------------------------------------------------------------------------------------------------------------
def _chunks(data):
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    at, out = 8, []
    while at < len(data):
        n, tag = struct.unpack('>I4s', data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack('>I', data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        out.append((tag, body))
        at += 12 + n
    return out


@pytest.mark.parametrize('shape', [(5, 7, 3), (1, 1, 3), (6, 4)])
def test_save_png(tmp_path, shape):
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, shape).astype(np.uint8)
    path = vis.save_png(str(tmp_path / 'sub' / 'a.png'), torch.from_numpy(img) if len(shape) == 3 else img)
    with open(path, 'rb') as fh:
        chunks = _chunks(fh.read())
    assert [t for t, _ in chunks] == [b'IHDR', b'IDAT', b'IEND'] and chunks[2][1] == b''
    assert chunks[0][1] == struct.pack('>IIBBBBB', shape[1], shape[0], 8, 2 if len(shape) == 3 else 0, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(shape[0], -1)
    assert (raw[:, 0] == 0).all() and np.array_equal(raw[:, 1:].reshape(shape), img)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        assert np.array_equal(np.asarray(Image.open(path)), img)
    with pytest.raises(ValueError):
        vis.save_png(str(tmp_path / 'b.png'), img.astype(np.float32))
    with pytest.raises(ValueError):
        vis.save_png(str(tmp_path / 'b.png'), np.zeros((4, 4, 4), np.uint8))


# ---- mosaic -------------------------------------------------------------------------------------------------------------------
def test_mosaic_geometry():
    V, h, w, X, Y = 6, 3, 5, 4, 8
    views = torch.stack([torch.full((h, w, 3), 10 * (v + 1), dtype=torch.uint8) for v in range(V)])
    bev = (torch.arange(X)[:, None] * 16 + torch.arange(Y)[None, :]).to(torch.uint8)[..., None].repeat(1, 1, 3)
    m = vis.OccRenderer.mosaic(views, bev)
    H = 2 * h
    bw = (H * Y + X // 2) // X
    assert m.dtype == torch.uint8 and tuple(m.shape) == (H, 3 * w + bw, 3)
    for r, row in enumerate(((2, 0, 1), (4, 3, 5))):
        for c, v in enumerate(row):
            assert (m[r * h:(r + 1) * h, c * w:(c + 1) * w] == 10 * (v + 1)).all()
    part = m[:, 3 * w:, 0].numpy()
    for r in range(H):
        for c in range(bw):
            x = X - 1 - ((2 * r + 1) * X) // (2 * H)                  # ego x up
            y = Y - 1 - ((2 * c + 1) * Y) // (2 * bw)                 # ego y to the left
            assert part[r, c] == x * 16 + y
    # a caller's grid with a hole, fewer views
    m = vis.OccRenderer.mosaic(views[:2], bev, layout=((0, None), (None, 1)))
    assert tuple(m.shape) == (H, 2 * w + bw, 3)
    assert (m[:h, w:2 * w] == 0).all() and (m[h:, :w] == 0).all() and (m[h:, w:2 * w] == 20).all()
    with pytest.raises(ValueError, match='view 5'):
        vis.OccRenderer.mosaic(views[:2], bev, layout=((0, 5),))
