"""-m gpu: occupancy rendered on the device (csrc/occ_render.hip through ext.render_views / ext.render_bev, vis.OccRenderer and
test_loop.run_test) against the numpy restatement on the reference-pinned caster (tests/render_ref.py), on the small scenes of
tests/render_cases.py.  Every pixel of every output is compared bit for bit: rgb and label / category as bytes, depth as float32
bits.  What the scenes are there for is asserted on the REFERENCE's output, never on the code under test.

One condition of the issue cannot hold as worded and is mended here: "the two inside cameras each give >= 10 % hits and >= 10 %
misses".  A camera inside an OCCUPIED voxel hits that voxel with every ray (the traversal's first step is inside the grid with
its bit set), so it cannot miss; it is asserted to hit everywhere with that voxel's class, and the 10 % / 10 % condition is
asserted for the two cameras inside the grid that can meet it: the one in a free voxel and the one on a voxel face."""
import ctypes

import numpy as np
import pytest
import torch

from tests import render_cases as rc
from tests import render_ref as rr

pytestmark = pytest.mark.gpu

FILL, FILL2, GUARD = 0xA5, 0x5A, 64
# (frames: None | 'same' | 'other', alpha): every frames mode and every alpha of the issue
COLOURINGS = [(None, 100), (None, 256), ('same', 0), ('same', 256), ('other', 100)]


def _other_size(size):
    """a source size that is no integer multiple of the render size (17 x 33 for 7 x 13)"""
    return (2 * size[0] + 3, 2 * size[1] + 7)


def _outs(B, V, h, w, fill):
    """pre-filled outputs, each GUARD elements larger than needed"""
    n = B * V * h * w
    return {'label': torch.full((n + GUARD,), fill, dtype=torch.uint8, device='cuda'),
            'depth': torch.full(((n + GUARD) * 4,), fill, dtype=torch.uint8, device='cuda').view(torch.float32),
            'rgb': torch.full((3 * n + GUARD,), fill, dtype=torch.uint8, device='cuda')}


def _check_views(got, outs, want, fill, what):
    """got: ext.render_views' dict (views into `outs`), want: per sample render_ref.views dicts"""
    B = len(want)
    for key, dt in (('label', np.uint8), ('rgb', np.uint8), ('depth', np.uint32)):
        g = got[key].cpu().numpy()
        w_ = np.stack([w[key] for w in want])
        assert g.shape == w_.shape and g.dtype == w_.dtype, (what, key, g.shape, w_.shape)
        assert np.array_equal(g.view(dt), w_.view(dt)), (what, key, int((g.view(dt) != w_.view(dt)).sum()), g.size)
        raw = outs[key].cpu().numpy()
        assert np.array_equal(raw[:g.size].view(dt), w_.reshape(-1).view(dt)), (what, key, 'not at the front of out')
        assert (raw[g.size:].view(np.uint8) == fill).all(), (what, key, 'guard')
    assert B == got['label'].shape[0]


class _Case:
    """One (grid, dtype, size) batch with its reference casts, computed once"""

    def __init__(self, name, dtype, size):
        self.name, self.size = name, size
        self.sems, self.gts, self.cams = rc.batch(name, dtype, size)
        self.casts = [rr.cast_views(s, self.cams[b], rc.PC_MIN, rc.VOXEL, size, rc.FREE, sem_gt=self.gts[b], far=rc.FAR)
                      for b, s in enumerate(self.sems)]
        self.pal, self.cat = rc.palettes()
        self._dev = None

    @property
    def dev(self):
        if self._dev is None:
            self._dev = dict(sem=torch.from_numpy(np.stack(self.sems)).cuda(), gt=torch.from_numpy(np.stack(self.gts)).cuda(),
                             cams=torch.from_numpy(self.cams).cuda(), pal=torch.from_numpy(self.pal).cuda(),
                             cat=torch.from_numpy(self.cat).cuda())
        return self._dev

    def want(self, diff, frames, alpha, b=None, v=None):
        out = []
        for k in range(2) if b is None else [b]:
            vs = slice(None) if v is None else slice(v, v + 1)
            out.append(rr.views(self.sems[k], self.cams[k][vs], rc.PC_MIN, rc.VOXEL, self.size, rc.FREE,
                                sem_gt=self.gts[k] if diff else None, frames=None if frames is None else frames[k][vs],
                                palette=self.pal, cat_palette=self.cat, far=rc.FAR, tol=rc.TOL, alpha=alpha, bg_rgb=rc.BG,
                                casts=self.casts[k][vs]))
        return out

    def run(self, diff, frames, alpha, fill=FILL, b=None, v=None, **kw):
        from occnet_amd import ext
        d = self.dev
        bs = slice(None) if b is None else slice(b, b + 1)
        vs = slice(None) if v is None else slice(v, v + 1)
        cams = d['cams'][bs, vs].contiguous()
        outs = _outs(cams.shape[0], cams.shape[1], self.size[0], self.size[1], fill)
        fr = None if frames is None else torch.from_numpy(np.ascontiguousarray(frames[bs, vs])).cuda()
        got = ext.render_views(d['sem'][bs].contiguous(), cams, rc.PC_MIN, rc.VOXEL, self.size, free_id=rc.FREE,
                               sem_gt=d['gt'][bs].contiguous() if diff else None, frames=fr, palette=d['pal'],
                               cat_palette=d['cat'], far=rc.FAR, tol=rc.TOL, alpha=alpha, bg_rgb=rc.BG, out=outs, **kw)
        return got, outs

    def frames(self, mode):
        if mode is None:
            return None
        return rc.frames(2, 3, self.size if mode == 'same' else _other_size(self.size), 5)


_CASES = {}


def _case(name, dtype, size):
    key = (name, np.dtype(dtype).name, size)
    if key not in _CASES:
        _CASES[key] = _Case(name, dtype, size)
    return _CASES[key]


# ---- the scenes are what they claim to be (asserted on the reference) -------------------------------------------------------
@pytest.mark.parametrize('name', sorted(rc.GRIDS))
@pytest.mark.parametrize('size', rc.SIZES[1:], ids=lambda s: f'{s[0]}x{s[1]}')
def test_scenes_are_not_vacuous(name, size):
    c = _case(name, np.uint8, size)
    inside, outside = c.want(False, None, 256)
    for v, cam in ((0, 'inside_free'), (2, 'on_face')):
        frac = inside['hit'][v].mean()
        assert 0.1 <= frac <= 0.9, (cam, frac)
    occ_voxel = rc._voxel_near_centre(c.sems[0], True)
    assert inside['hit'][1].all() and (inside['label'][1] == c.sems[0][tuple(occ_voxel)]).all()     # inside an occupied voxel
    assert inside['hit'][2].any() and outside['hit'][0].any() and not outside['hit'][0].all()        # outside, looking in
    # outside looking away: every pixel misses, and the class of voxel (0, 0, 0), which such a ray reports, does not appear
    assert c.sems[1][0, 0, 0] == 3 and not outside['hit'][1].any()
    assert (outside['label'][1] == rc.FREE).all() and (outside['depth'][1] == -1).all()
    # the axis-aligned camera: the pixel at the principal point has two direction components that are exactly zero
    cam = c.cams[1, 2]
    k, m = size[1] // 2, size[0] // 2
    px, py = np.float32(k) + np.float32(0.5), np.float32(m) + np.float32(0.5)
    assert (cam[6] * px + cam[7] * py) + cam[8] == 0 and (cam[9] * px + cam[10] * py) + cam[11] == 0
    assert (cam[3] * px + cam[4] * py) + cam[5] == 1
    # the shade's clamp is met and not met, class ids above 127 are seen
    depths = np.concatenate([w['depth'][w['hit']] for w in (inside, outside)])
    assert (depths > rc.FAR).any() and (depths < rc.FAR / 2).any()
    assert (np.concatenate([w['label'][w['hit']] for w in (inside, outside)]) > 127).any()
    if name == '7x5x17':                                                # the diff scene
        cats = np.concatenate([w['label'].reshape(-1) for w in c.want(True, None, 256)])
        assert sorted(set(cats.tolist())) == [0, 1, 2, 3, 4, 5]
    if name == '4x4x32':
        assert rr.bev(c.sems[0])['label'][1, 1] == 200 and c.sems[0][1, 1, 31] == 200                 # bit 31 of a uint32 mask


# ---- every pixel, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(rc.GRIDS))
@pytest.mark.parametrize('dtype', [np.uint8, np.int64], ids=['u8', 'i64'])
@pytest.mark.parametrize('size', rc.SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_views_equal_reference(name, dtype, size):
    c = _case(name, dtype, size)
    for diff in (False, True):
        for mode, alpha in COLOURINGS:
            frames = c.frames(mode)
            got, outs = c.run(diff, frames, alpha)
            _check_views(got, outs, c.want(diff, frames, alpha), FILL, (name, size, diff, mode, alpha))
    # a second pre-fill: equal to the reference under both, so every output byte is written
    frames = c.frames('other')
    for diff in (False, True):
        got, outs = c.run(diff, frames, 100, fill=FILL2)
        _check_views(got, outs, c.want(diff, frames, 100), FILL2, (name, size, diff, 'fill 2'))
    if dtype == np.int64:
        ids = np.concatenate([w['label'][w['hit']] for w in c.want(False, None, 256)])
        if size != (1, 1) and name != '3x9x1':                          # (the one-layer grid shows too few voxels)
            assert np.isin(ids, [300 & 0xff, -3 & 0xff]).any()          # ids beyond a byte were met


@pytest.mark.parametrize('size', [(1, 1), (7, 13)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_single_view_single_sample(size):
    """B = 1, V = 1: each camera on its own, and a subset of the outputs"""
    from occnet_amd import ext
    c = _case('5x6x4', np.int64, size)
    frames = c.frames('other')
    for b in range(2):
        for v in range(3):
            for diff in (False, True):
                got, outs = c.run(diff, frames, 100, b=b, v=v)
                _check_views(got, outs, c.want(diff, frames, 100, b=b, v=v), FILL, (b, v, diff))
    d = c.dev
    want = c.want(False, None, 160, b=0)[0]
    only = ext.render_views(d['sem'][:1].contiguous(), d['cams'][:1].contiguous(), rc.PC_MIN, rc.VOXEL, size, far=rc.FAR,
                            want=('depth',))
    assert sorted(only) == ['depth'] and np.array_equal(only['depth'][0].cpu().numpy().view(np.uint32), want['depth'].view(np.uint32))
    only = ext.render_views(d['sem'][:1].contiguous(), d['cams'][:1].contiguous(), rc.PC_MIN, rc.VOXEL, size, far=rc.FAR,
                            want=('label',))                           # no palette needed without rgb
    assert sorted(only) == ['label'] and np.array_equal(only['label'][0].cpu().numpy(), want['label'])


@pytest.mark.parametrize('name', sorted(rc.GRIDS))
@pytest.mark.parametrize('dtype', [np.uint8, np.int64], ids=['u8', 'i64'])
def test_bev_equals_reference(name, dtype):
    from occnet_amd import ext
    c = _case(name, dtype, (7, 13))
    d = c.dev
    B, (X, Y, Z) = 2, rc.GRIDS[name]
    for diff in (False, True):
        for fill in (FILL, FILL2):
            outs = {'label': torch.full((B * X * Y + GUARD,), fill, dtype=torch.uint8, device='cuda'),
                    'rgb': torch.full((B * X * Y * 3 + GUARD,), fill, dtype=torch.uint8, device='cuda')}
            got = ext.render_bev(d['sem'], free_id=rc.FREE, sem_gt=d['gt'] if diff else None, palette=d['pal'],
                                 cat_palette=d['cat'], bg_rgb=rc.BG, out=outs)
            want = [rr.bev(c.sems[b], rc.FREE, c.gts[b] if diff else None, c.pal, c.cat, rc.BG) for b in range(B)]
            for key in ('label', 'rgb'):
                g, w = got[key].cpu().numpy(), np.stack([x[key] for x in want])
                assert g.shape == w.shape and np.array_equal(g, w), (name, diff, key, int((g != w).sum()))
                raw = outs[key].cpu().numpy()
                assert np.array_equal(raw[:g.size], w.reshape(-1)) and (raw[g.size:] == fill).all(), (name, diff, key, 'guard')
        if name == '3x9x1':                                             # one layer: empty pillars, and every category
            codes = set(np.concatenate([w['label'].reshape(-1) for w in want]).tolist())
            assert codes >= ({0, 1, 3, 4, 5} if diff else {rc.FREE, 3})


# ---- determinism and entry points -----------------------------------------------------------------------------------------
def test_determinism_workspace_c_abi_and_stream():
    from occnet_amd import _lib, ext
    size = (9, 70)
    c = _case('7x5x17', np.int64, size)
    frames = c.frames('other')
    B, V, (X, Y, Z), (h, w) = 2, 3, rc.GRIDS['7x5x17'], size
    _, first = c.run(True, frames, 100)
    first = {k: t.cpu().numpy().view(np.uint8) for k, t in first.items()}
    _, again = c.run(True, frames, 100)
    for k in first:
        assert np.array_equal(again[k].cpu().numpy().view(np.uint8), first[k]), k
    # a workspace of the caller's, full of junk, with nothing written past the size the query gives
    need = ext.render_workspace_bytes(B, X, Y, Z, diff=True)
    ws = torch.full((need + 512,), 0xFF, dtype=torch.uint8, device='cuda')
    _, junk = c.run(True, frames, 100, workspace=ws)
    for k in first:
        assert np.array_equal(junk[k].cpu().numpy().view(np.uint8), first[k]), k
    assert (ws[need:] == 0xFF).all()
    # the C ABI, called directly
    d = c.dev
    fr = torch.from_numpy(frames).cuda()
    outs = _outs(B, V, h, w, FILL)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    p, f = (lambda t: ctypes.c_void_p(t.data_ptr())), ctypes.c_float
    rc_ = _lib.lib().occ_render_views(p(d['sem']), 1, p(d['gt']), 1, p(d['cams']), p(fr), fr.shape[2], fr.shape[3], p(d['pal']),
                                      p(d['cat']), f(rc.PC_MIN[0]), f(rc.PC_MIN[1]), f(rc.PC_MIN[2]), f(rc.VOXEL), rc.FREE,
                                      f(rc.FAR), f(rc.TOL), 100, rc.BG, p(outs['label']), p(outs['depth']), p(outs['rgb']), p(ws),
                                      ctypes.c_int64(ws.numel()), B, V, X, Y, Z, h, w,
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc_ == 0
    for k in first:
        assert np.array_equal(outs[k].cpu().numpy().view(np.uint8), first[k]), k
    # a stream of the caller's
    side = torch.cuda.Stream()
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(side):
        _, other = c.run(True, frames, 100)
    side.synchronize()
    for k in first:
        assert np.array_equal(other[k].cpu().numpy().view(np.uint8), first[k]), k


def test_unsupported_depth():
    from occnet_amd import ext
    from occnet_amd._lib import OccAmdUnsupported
    sem = torch.full((1, 4, 4, 33), 16, dtype=torch.uint8).cuda()
    out = {'label': torch.full((1024,), FILL, dtype=torch.uint8, device='cuda')}
    with pytest.raises(OccAmdUnsupported):
        ext.render_views(sem, torch.zeros(1, 1, 12).cuda(), rc.PC_MIN, rc.VOXEL, (4, 4), want=('label',), out=out)
    with pytest.raises(OccAmdUnsupported):
        ext.render_bev(sem, want=('label',), out=out)
    assert (out['label'] == FILL).all()


# ---- the renderer and the loop ------------------------------------------------------------------------------------------------
def _metas_from(cams, size):
    """img_metas whose view_rays are (up to the float64 inverse's rounding) the given cameras: lidar2img = inverse of [D o; 0 1]"""
    metas = []
    for sample in cams:
        mats = []
        for cam in sample:
            inv = np.eye(4)
            inv[:3, :3], inv[:3, 3] = cam[3:].reshape(3, 3).astype(np.float64), cam[:3].astype(np.float64)
            mats.append(np.linalg.inv(inv))
        metas.append(dict(lidar2img=mats, ego2lidar=np.eye(4), img_shape=[(size[0], size[1], 3)] * len(sample)))
    return metas


def _want_from_views_rays(r, sems, gts, metas, frames):
    """the reference's images for the cameras OccRenderer derives from the metas"""
    from occnet_amd import vis
    cams = vis.view_rays(metas, r.size).numpy()
    pal, cat = vis.default_palette(), vis.category_palette()
    out = []
    for b, sem in enumerate(sems):
        gt = None if gts is None else gts[b]
        v = rr.views(sem, cams[b], rc.PC_MIN, rc.VOXEL, r.size, rc.FREE, sem_gt=gt, frames=None if frames is None else frames[b],
                     palette=pal, cat_palette=cat, far=r.far, tol=r.tol, alpha=r.alpha, bg_rgb=r.bg_rgb)
        out.append((v['rgb'], rr.bev(sem, rc.FREE, gt, pal, cat, r.bg_rgb)['rgb']))
    return out


def test_renderer_enqueue_in_token_order():
    from occnet_amd import vis
    size, name = (7, 13), '7x5x17'
    shape = rc.GRIDS[name]
    batches = []
    for i, B in enumerate((1, 2, 1)):
        sems, gts, cams = rc.batch(name, (np.uint8, np.int64)[i % 2], size, seed=i)
        sems, gts, cams = sems[:B], gts[:B], cams[:B]
        batches.append(dict(tokens=[f't{i}_{b}' for b in range(B)], sems=sems, gts=gts if i != 1 else None,
                            metas=_metas_from(cams, size), frames=rc.frames(B, 3, _other_size(size), 40 + i) if i != 2 else None))
    r = vis.OccRenderer(rc.pc_range(shape), rc.VOXEL, free_id=rc.FREE, size=size, far=rc.FAR, tol=rc.TOL, alpha=100, depth=2)
    direct = vis.OccRenderer(rc.pc_range(shape), rc.VOXEL, free_id=rc.FREE, size=size, far=rc.FAR, tol=rc.TOL, alpha=100)
    assert r.occ_size == list(shape)
    want = {}
    for bt in batches:
        sem = torch.from_numpy(np.stack(bt['sems'])).cuda()
        gt = None if bt['gts'] is None else torch.from_numpy(np.stack(bt['gts'])).cuda()
        fr = None if bt['frames'] is None else torch.from_numpy(bt['frames']).cuda()
        r.enqueue(bt['tokens'], sem, bt['metas'], frames=fr, sem_gt=gt)
        v = direct.views(sem, bt['metas'], frames=fr, sem_gt=gt)['rgb'].cpu().numpy()
        b_ = direct.bev(sem, sem_gt=gt)['rgb'].cpu().numpy()
        ref = _want_from_views_rays(direct, bt['sems'], bt['gts'], bt['metas'], bt['frames'])
        for b, tok in enumerate(bt['tokens']):
            want[tok] = (v[b], b_[b])
            assert np.array_equal(v[b], ref[b][0]) and np.array_equal(b_[b], ref[b][1]), tok     # not merely wrong alike
    with pytest.raises(ValueError, match='t0_0'):
        r.enqueue(['fresh', 't0_0'], sem, bt['metas'] * 2)
    res = r.results()
    assert list(res) == list(want) == ['t0_0', 't1_0', 't1_1', 't2_0']
    for tok in want:
        assert res[tok]['views'].shape == (3,) + size + (3,) and res[tok]['bev'].shape == shape[:2] + (3,)
        assert np.array_equal(res[tok]['views'], want[tok][0]) and np.array_equal(res[tok]['bev'], want[tok][1]), tok
    assert r.drain() is r and r.results() is res


class _StubModel:
    def __init__(self, outs):
        self.outs, self.k = outs, 0

    def simple_test(self, img_metas, img):
        self.k += 1
        return (None,) + self.outs[self.k - 1]


def test_vis_loop_feeds_the_renderer_and_leaves_the_rest_alone(tmp_path):
    from occnet_amd import vis
    from occnet_amd.test_loop import run_test
    from occnet_amd.metrics import RayMetrics, SubmissionScore, SubmissionWriter
    size, name = (7, 13), '7x5x17'
    shape = rc.GRIDS[name]
    pc_range = rc.pc_range(shape)
    rng = np.random.default_rng(3)
    rays = rng.normal(size=(70, 3))
    rays = torch.from_numpy((rays / np.linalg.norm(rays, axis=1, keepdims=True)).astype(np.float32))
    samples, outs, scenes = [], [], []
    for i in range(3):
        sems, gts, cams = rc.batch(name, np.int64, size, seed=10 + i)
        sp, sg = sems[0], gts[0].astype(np.uint8 if i else np.int64)
        fp = (rng.normal(size=shape + (2,)) * 2).astype(np.float32)
        fg = (fp + rng.normal(size=shape + (2,)) * 0.5).astype(np.float32)
        metas = _metas_from(cams[:1], size)
        fr = rc.frames(1, 3, _other_size(size), 60 + i) if i != 1 else None
        vox = rng.uniform([1, 1, 1], [shape[0] - 1, shape[1] - 1, shape[2] - 1], size=(1, 2, 3))
        origins = torch.tensor(np.asarray(rc.PC_MIN) + vox * rc.VOXEL, dtype=torch.float32)
        outs.append((torch.from_numpy(sp)[None].cuda(), torch.from_numpy(fp)[None].cuda()))
        s = dict(token=f's{i}', img_metas=metas, img=i, lidar_origins=origins, voxel_semantics=torch.from_numpy(sg)[None].cuda(),
                 voxel_flow=torch.from_numpy(fg)[None].cuda())
        if fr is not None:
            s['frames'] = torch.from_numpy(fr).cuda()
        samples.append(s)
        scenes.append((sp, sg, metas, fr))

    def consumers():
        return (RayMetrics(pc_range, rc.VOXEL, rays=rays), SubmissionWriter(pc_range, rc.VOXEL, rays=rays), SubmissionScore())

    m0, w0, s0 = consumers()
    assert run_test(_StubModel(outs), samples, metric=m0, writer=w0, score=s0) == 3
    m1, w1, s1 = consumers()
    r = vis.OccRenderer(pc_range, rc.VOXEL, free_id=rc.FREE, size=size, far=rc.FAR, tol=rc.TOL, alpha=100, depth=2)
    model = _StubModel(outs)
    assert run_test(model, iter(samples), metric=m1, writer=w1, score=s1, renderer=r, out_dir=str(tmp_path)) == 3
    assert model.k == 3                                                       # the model ran once per sample
    assert torch.equal(m1.state, m0.state) and torch.equal(s1.state, s0.state) and int(m0.state.sum()) > 0
    a, b = w1.results(), w0.results()
    assert list(a) == list(b) == ['s0', 's1', 's2']
    for tok in a:
        assert all(a[tok][k].tobytes() == b[tok][k].tobytes() for k in ('pcd_cls', 'pcd_dist', 'pcd_flow'))
    res = r.results()
    assert list(res) == ['s0', 's1', 's2']
    for i, tok in enumerate(res):
        sp, sg, metas, fr = scenes[i]
        want_v, want_b = _want_from_views_rays(r, [sp], [sg], metas, fr)[0]
        assert np.array_equal(res[tok]['views'], want_v) and np.array_equal(res[tok]['bev'], want_b), tok
        with open(tmp_path / f'{tok}.png', 'rb') as fh:
            assert fh.read(8) == b'\x89PNG\r\n\x1a\n'
    # every second sample, nothing but the renderer; all consumers but the renderer: the same as run_test without a renderer
    r2 = vis.OccRenderer(pc_range, rc.VOXEL, free_id=rc.FREE, size=size, far=rc.FAR, tol=rc.TOL, alpha=100, depth=1)
    assert run_test(_StubModel(outs), samples, renderer=r2, every=2) == 3
    assert list(r2.results()) == ['s0', 's2'] and np.array_equal(r2.results()['s2']['views'], res['s2']['views'])
    m2, w2, s2 = consumers()
    assert run_test(_StubModel(outs), samples, metric=m2, writer=w2, score=s2) == 3
    assert torch.equal(m2.state, m0.state) and torch.equal(s2.state, s0.state)
