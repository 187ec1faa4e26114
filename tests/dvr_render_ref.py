"""Float64, pure-Python restatement of the reference's differentiable ray renderer (`render_cuda_kernel`,
tools/ray_iou/lib/dvr/dvr.cu:391-636): its traversal loop and its three backward loops in its own order, one ray at a time.
Test infrastructure of tests/test_dvr_render_host.py and tests/test_gpu_dvr_render.py.

It reads the float32 inputs exactly as they are given to the device (every value widened to a Python float, as the kernel
widens to double).  Two statements differ from the literal text, both on purpose:
  - the term of a ray's LAST voxel is set to 0.  Its true value is 0 (sigma of the last voxel does not move the expected
    depth); the literal text computes (p_out * max_d) * dt - (dt * p_out) * max_d, which is 0 or one rounding of either
    product — noise that no implementation can be asked to reproduce;
  - the padded-ray rule is the one of include/occnet_amd_dvr.h (tindex < 0, NaN or >= T; zero length; a non-finite
    coordinate), where the reference would divide 0 / 0 or read past `origin`.
"""
import math

import numpy as np

DBL_MAX = 1.7976931348623157e308
LOSS_CODES = {"l1": 0, "l2": 1, "absrel": 2, "bce": 0}


def render_ray(grid, o, e, loss_type):
    """grid: (Z, Y, X) float32 array; o, e: three float32 values each.  None for a ray that is not cast (zero length /
    non-finite), else a dict: entered, and when entered exp_d, gt_d, path [(x, y, z)], d, dt, sigma, terms (the summands
    this ray adds to grad_sigma along its path), dl_dd."""
    xo, yo, zo = (float(v) for v in o)
    xe, ye, ze = (float(v) for v in e)
    if not all(math.isfinite(v) for v in (xo, yo, zo, xe, ye, ze)):
        return None
    vzsize, vysize, vxsize = grid.shape
    vx, vy, vz = int(xo), int(yo), int(zo)
    rx, ry, rz = xe - xo, ye - yo, ze - zo
    gt_d = math.sqrt(rx * rx + ry * ry + rz * rz)
    if not gt_d > 0.0:
        return None
    dx, dy, dz = rx / gt_d, ry / gt_d, rz / gt_d
    stepX = 1 if dx >= 0 else -1
    stepY = 1 if dy >= 0 else -1
    stepZ = 1 if dz >= 0 else -1
    bx = float(vx + (0 if stepX < 0 else 1))
    by = float(vy + (0 if stepY < 0 else 1))
    bz = float(vz + (0 if stepZ < 0 else 1))
    tMaxX = (bx - xo) / dx if dx != 0 else DBL_MAX
    tMaxY = (by - yo) / dy if dy != 0 else DBL_MAX
    tMaxZ = (bz - zo) / dz if dz != 0 else DBL_MAX
    tDeltaX = stepX / dx if dx != 0 else DBL_MAX
    tDeltaY = stepY / dy if dy != 0 else DBL_MAX
    tDeltaZ = stepZ / dz if dz != 0 else DBL_MAX

    path, csd, p, d, dt, sig = [], [], [], [], [], []
    step = 0
    last_d = 0.0
    was_inside = False
    while True:
        inside = (0 <= vx < vxsize) and (0 <= vy < vysize) and (0 <= vz < vzsize)
        if inside:
            was_inside = True
            cur = (vx, vy, vz)
        elif was_inside:
            break
        elif last_d > gt_d:
            break
        if tMaxX < tMaxY:
            if tMaxX < tMaxZ:
                _d = tMaxX; vx += stepX; tMaxX += tDeltaX
            else:
                _d = tMaxZ; vz += stepZ; tMaxZ += tDeltaZ
        else:
            if tMaxY < tMaxZ:
                _d = tMaxY; vy += stepY; tMaxY += tDeltaY
            else:
                _d = tMaxZ; vz += stepZ; tMaxZ += tDeltaZ
        if inside:
            _sigma = float(grid[cur[2], cur[1], cur[0]])
            _delta = max(0.0, _d - last_d)
            sd = _sigma * _delta
            if not path:
                csd.append(sd)
                p.append(1 - math.exp(-sd))
            else:
                csd.append(csd[-1] + sd)
                p.append(math.exp(-csd[-2]) - math.exp(-csd[-1]))
            path.append(cur); d.append(_d); dt.append(_delta); sig.append(_sigma)
        last_d = _d
        step += 1
        if step > 1000:
            break
    count = len(path)
    if count == 0:
        return dict(entered=False)
    exp_d = 0.0
    for i in range(count):
        exp_d += p[i] * d[i]
    p_out = math.exp(-csd[count - 1])
    max_d = d[count - 1]
    exp_d += p_out * max_d
    gt_d = min(gt_d, max_d)
    dd = [0.0] * count
    for i in range(count - 1, -1, -1):
        if i == count - 1:
            dd[i] = p_out * max_d
        else:
            dd[i] = dd[i + 1] - math.exp(-csd[i]) * (d[i + 1] - d[i])
    for i in range(count - 1, -1, -1):
        dd[i] *= dt[i]
    for i in range(count - 1, -1, -1):
        dd[i] -= dt[i] * p_out * max_d
    dd[count - 1] = 0.0                         # see the module text
    if loss_type == 0:
        dl_dd = 1.0 if exp_d >= gt_d else -1.0
    elif loss_type == 1:
        dl_dd = exp_d - gt_d
    else:
        dl_dd = (1.0 / gt_d) if exp_d >= gt_d else -(1.0 / gt_d)
    return dict(entered=True, exp_d=exp_d, gt_d=gt_d, path=path, d=d, dt=dt, sigma=sig, dd=dd, dl_dd=dl_dd,
                terms=[dl_dd * v for v in dd])


def render(sigma, origin, points, tindex, loss_name):
    """float32 arrays (anything np.asarray takes; device tensors copied back by the caller) in the shapes of ext.dvr_render.
    -> dict: pred, gt (N, M) float64, -1 where a ray is not rendered; g64, A (N, T, Z, Y, X) float64: the summed gradient and
    the sum of |term| per voxel; n (same shape, int64): how many rays crossed the voxel; rays: {(n, c): render_ray's dict} of
    the rays that were cast."""
    sigma, origin, points, tindex = (np.asarray(a, dtype=np.float32) for a in (sigma, origin, points, tindex))
    loss_type = LOSS_CODES[loss_name]
    N, T = sigma.shape[:2]
    M = points.shape[1]
    pred = -np.ones((N, M))
    gt = -np.ones((N, M))
    g64 = np.zeros(sigma.shape)
    A = np.zeros(sigma.shape)
    cnt = np.zeros(sigma.shape, dtype=np.int64)
    rays = {}
    for n in range(N):
        for c in range(M):
            tf = float(tindex[n, c])
            if not (tf >= 0 and tf < T):
                continue
            t = int(tf)
            ts = 0 if T == 1 else t
            r = render_ray(sigma[n, ts], origin[n, t], points[n, c, :3], loss_type)
            if r is None:
                continue
            rays[(n, c)] = r
            if not r['entered']:
                continue
            pred[n, c], gt[n, c] = r['exp_d'], r['gt_d']
            for (x, y, z), term in zip(r['path'], r['terms']):
                g64[n, ts, z, y, x] += term
                A[n, ts, z, y, x] += abs(term)
                cnt[n, ts, z, y, x] += 1
    return dict(pred=pred, gt=gt, g64=g64, A=A, n=cnt, rays=rays)


def grad_bound(n, A):
    """The per-voxel bound of a float32 accumulation of the terms against g64: one rounding of each double term to float, one
    rounding per float add, at most 2 n adds for any summation tree, and 1e-11 relative for double-exp differences."""
    return (2.0 * n + 4.0) * 2.0 ** -24 * A + 1e-11 * A
