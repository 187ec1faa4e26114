"""Reference restatement of the camera visibility masks and the masked confusion counts (test infrastructure for
csrc/visibility.hip), after tests/render_ref.py.

The ray statements are numpy float32, one rounding per operation, in the order of the kernel's header comment; the traversal
set-up and the walk are Python floats (binary64: every operation correctly rounded, as the device's double arithmetic is) and
Python ints.  `walk` returns the visited voxels of one ray in order, and the ray parameter at which the ray leaves the last one
— what the first-hit caster reports for that ray, which tests/test_visibility_host.py pins to the plain-C caster of oracle/."""
import functools
import math

import numpy as np

F32 = np.float32
DBL_MAX = 1.7976931348623157e308


def pixel_rays(cam, pc_min, voxel_size, size, far):
    """One camera (12 float32) -> (origin (3) float32, points (h * w, 3) float32) in voxel units, pixel (i, j) at i * w + j."""
    h, w = size
    cam = np.asarray(cam, F32)
    o, D = cam[:3], cam[3:].reshape(3, 3)
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    px = jj.astype(F32) + F32(0.5)
    py = ii.astype(F32) + F32(0.5)
    vs = F32(voxel_size)
    origin, points = [], []
    for k in range(3):
        off = F32(pc_min[k])
        d = (D[k, 0] * px + D[k, 1] * py) + D[k, 2]
        ray = d * F32(far)
        end = ray + o[k]
        origin.append((o[k] - off) / vs)
        points.append(((end - off) / vs).reshape(-1))
    assert all(p.dtype == F32 for p in points) and all(np.asarray(v).dtype == F32 for v in origin)
    return np.array(origin, F32), np.stack(points, -1)


def walk(occ, origin, point):
    """occ (X, Y, Z) bool, origin / point: 3 float32 each -> (visited [(x, y, z), ...] in order, dist float32; -1 when the
    ray never enters the grid)."""
    X, Y, Z = occ.shape
    o = [float(v) for v in origin]
    e = [float(v) for v in point]
    v = [int(c) for c in o]                                             # (int): truncation toward zero
    r = [e[k] - o[k] for k in range(3)]
    norm = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    with np.errstate(all='ignore'):
        d = [float(np.float64(r[k]) / np.float64(norm)) for k in range(3)]      # 0 / 0 -> NaN as in C, no exception
    step = [1 if d[k] >= 0 else -1 for k in range(3)]
    border = [v[k] + (0 if step[k] < 0 else 1) for k in range(3)]
    t_max = [(border[k] - o[k]) / d[k] if d[k] != 0 else DBL_MAX for k in range(3)]
    t_delta = [step[k] / d[k] if d[k] != 0 else DBL_MAX for k in range(3)]
    visited, was_inside, last_d = [], False, 0.0
    vx, vy, vz = v
    tx, ty, tz = t_max
    for _ in range(1001):                                               # steps 0..1000
        inside = 0 <= vx < X and 0 <= vy < Y and 0 <= vz < Z
        if not inside and was_inside:
            break
        c = (vx, vy, vz)
        if tx < ty:
            if tx < tz:
                dist = tx; vx += step[0]; tx += t_delta[0]
            else:
                dist = tz; vz += step[2]; tz += t_delta[2]
        else:
            if ty < tz:
                dist = ty; vy += step[1]; ty += t_delta[1]
            else:
                dist = tz; vz += step[2]; tz += t_delta[2]
        if inside:
            was_inside = True
            last_d = dist
            visited.append(c)
            if occ[c]:
                break
    return visited, (F32(last_d) if was_inside else F32(-1))


def view_walks(sem, cam, pc_min, voxel_size, size, free_id=16, far=100.0):
    """One camera through one grid -> [(visited, dist)] per pixel, pixel (i, j) at i * w + j."""
    occ = np.asarray(sem) != free_id
    origin, points = pixel_rays(cam, pc_min, voxel_size, size, far)
    return [walk(occ, origin, p) for p in points]


def mask_of(walks, shape):
    m = np.zeros(shape, np.uint8)
    for visited, _ in walks:
        for c in visited:
            m[c] = 1
    return m


def visibility(sems, cams, pc_min, voxel_size, size, free_id=16, far=100.0):
    """sems: B grids (X, Y, Z), cams (B, V, 12) -> mask (B, X, Y, Z) uint8: the OR over the views of each sample."""
    out = []
    for sem, views in zip(sems, cams):
        m = np.zeros(np.asarray(sem).shape, np.uint8)
        for cam in views:
            m |= mask_of(view_walks(sem, cam, pc_min, voxel_size, size, free_id, far), m.shape)
        out.append(m)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def case_walks(name, dtype_name, size, camera, b=0, seed=0, scenes='visibility'):
    """The walks of camera `camera` (a name of render_cases.CAMERAS) through sample b of the scene (name, dtype, size, seed) of
    tests/visibility_cases.py — or, with scenes='render', of tests/render_cases.py: computed once per process, shared by the
    host and the GPU tests, never modified."""
    from tests import render_cases as rc, visibility_cases as vc
    if scenes == 'visibility':
        sems = vc.batch(name, np.dtype(dtype_name), size, seed)[0]
        cam = vc.cameras(name, sems[b], size)[camera]
    else:
        sems = rc.batch(name, np.dtype(dtype_name), size, seed)[0]
        cam = rc.cameras(sems[b], size)[camera]
    return tuple(view_walks(sems[b], cam, rc.PC_MIN, rc.VOXEL, size, rc.FREE, rc.FAR))


@functools.lru_cache(maxsize=None)
def case_view_masks(name, dtype_name, size, seed=0):
    """(2, 3, X, Y, Z) uint8, read-only: the mask of each view of visibility_cases.batch(name, dtype, size, seed) taken alone."""
    from tests import render_cases as rc
    shape = rc.GRIDS[name]
    out = np.stack([np.stack([mask_of(case_walks(name, dtype_name, size, camera, b, seed), shape)
                              for camera in rc.CAMERAS[3 * b:3 * b + 3]]) for b in range(2)])
    out.setflags(write=False)
    return out


def case_mask(name, dtype_name, size, seed=0):
    """(2, X, Y, Z) uint8: the mask of visibility_cases.batch(name, dtype, size, seed), the OR over each sample's three views."""
    return np.bitwise_or.reduce(case_view_masks(name, dtype_name, size, seed), axis=1)


def confusion(sem_pred, sem_gt, mask=None, free_id=16):
    """-> the (ncls + 1, ncls) int64 state of csrc/visibility.hip: row g, column p over the admitted voxels with both ids in
    0..free_id; last row [skipped, admitted, 0 ...]."""
    ncls = free_id + 1
    p = np.asarray(sem_pred).reshape(-1).astype(np.int64)
    g = np.asarray(sem_gt).reshape(-1).astype(np.int64)
    keep = np.ones(p.shape, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    p, g = p[keep], g[keep]
    ok = (p >= 0) & (p < ncls) & (g >= 0) & (g < ncls)
    state = np.zeros((ncls + 1, ncls), np.int64)
    np.add.at(state, (g[ok], p[ok]), 1)
    state[ncls, 0] = int((~ok).sum())
    state[ncls, 1] = int(keep.sum())
    return state


def iou(conf, free_id):
    """conf (ncls, ncls), row = ground truth -> (iou per class, NaN where TP + FP + FN = 0; miou over 0..free_id-1;
    occupied-vs-free IoU), float64, written class by class."""
    conf = np.asarray(conf, np.int64)
    ncls = free_id + 1
    out = np.full(ncls, np.nan)
    for c in range(ncls):
        tp = int(conf[c, c])
        fn = int(conf[c].sum()) - tp
        fp = int(conf[:, c].sum()) - tp
        if tp + fp + fn:
            out[c] = tp / (tp + fp + fn)
    present = [v for v in out[:free_id] if not math.isnan(v)]
    miou = sum(present) / len(present) if present else float('nan')
    both = int(conf[:free_id, :free_id].sum())
    union = int(conf.sum()) - int(conf[free_id, free_id])
    return out, miou, (both / union if union else float('nan'))
