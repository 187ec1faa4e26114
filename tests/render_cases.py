"""The scenes of tests/test_gpu_render.py: seeded small grids, hand-placed cameras as the 12 floats the kernel takes, a ground
truth derived from a prediction by seeded edits.  Kept apart from the test so that a CPU run can put the plain-C caster of oracle/
behind tests/render_ref.py and check that no scene is vacuous before any GPU run."""
import numpy as np

VOXEL = 0.5
PC_MIN = (-1.5, -1.0, -0.5)
FREE = 16
FAR = 2.5                  # metres: shorter than what the cameras see (2.9 to 4.9 m), so the shade's clamp is met
TOL = 0.75                 # metres: depth differences on these grids are a few voxels of 0.5 m
BG = 0x123456
IDS_U8 = [0, 3, 15, 17, 127, 128, 200, 255]
IDS_I64 = IDS_U8 + [300, -3]
GRIDS = {'5x6x4': (5, 6, 4), '7x5x17': (7, 5, 17), '4x4x32': (4, 4, 32), '3x9x1': (3, 9, 1)}
SIZES = [(1, 1), (7, 13), (16, 24), (9, 70)]
CAMERAS = ('inside_free', 'inside_occupied', 'on_face', 'outside_in', 'outside_away', 'axis_zero')
# look directions of the inside_free and the on_face camera per grid, chosen (with the plain-C caster of oracle/, on the CPU) so
# that each sees between a quarter and three quarters of its pixels hit at every render size but 1 x 1
LOOK = {(5, 6, 4): ((1.0, 0.3, -0.1), (0.2, -1.0, -0.1)), (7, 5, 17): ((0.3, -0.4, -0.8), (-1.0, 0.5, 0.2)),
        (4, 4, 32): ((1.0, 0.3, -0.1), (1.0, 0.3, -0.1)), (3, 9, 1): ((0.2, -1.0, -0.1), (0.2, -1.0, -0.1))}


def pc_range(shape):
    return list(PC_MIN) + [PC_MIN[k] + shape[k] * VOXEL for k in range(3)]


def grid(shape, dtype, seed, density=0.25):
    ids = IDS_U8 if np.dtype(dtype) == np.uint8 else IDS_I64
    rng = np.random.default_rng(seed)
    sem = np.full(shape, FREE, dtype)
    occ = rng.random(shape) < density
    sem[occ] = rng.choice(np.array(ids, dtype=np.int64), int(occ.sum())).astype(dtype)
    sem[0, 0, 0] = 3                      # the voxel that a ray which never enters the grid reports: occupied
    if shape[2] == 32:
        sem[1:3, 1:3, 31] = 200           # the top bit of a uint32 mask
    return sem


def edited(sem, seed):
    """A ground truth for `sem`: a sixth of its occupied voxels relabelled, a sixth removed, and as many free ones filled."""
    rng = np.random.default_rng(seed)
    gt = sem.copy()
    occ = sem != FREE
    r = rng.random(sem.shape)
    gt[occ & (r < 1 / 6)] = 15 if sem.dtype == np.uint8 else 300
    gt[(gt == sem) & occ & (r < 1 / 6)] = 7                         # those that already held the new label
    gt[occ & (r >= 1 / 6) & (r < 2 / 6)] = FREE
    gt[~occ & (r < 0.08)] = 127
    return gt


def _voxel_near_centre(sem, occupied, skip=0):
    X, Y, Z = sem.shape
    c = np.array([(X - 1) / 2, (Y - 1) / 2, (Z - 1) / 2])
    idx = np.argwhere((sem != FREE) == occupied)
    idx = idx[np.argsort(((idx - c) ** 2).sum(1), kind='stable')]
    return idx[min(skip, len(idx) - 1)]


def _cam(centre_vox, fwd, f, cx, cy, up=(0.0, 0.0, 1.0)):
    """centre in voxel coordinates, a look direction, focal length and principal point in pixels of the rendered image"""
    o = np.asarray(PC_MIN, np.float64) + np.asarray(centre_vox, np.float64) * VOXEL
    fwd = np.asarray(fwd, np.float64)
    fwd = fwd / np.linalg.norm(fwd)
    right = np.cross(fwd, np.asarray(up, np.float64))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    D = np.stack([right / f, down / f, fwd - cx / f * right - cy / f * down], 1)       # columns: px, py, 1
    return np.concatenate([o, D.reshape(-1)]).astype(np.float32)


def cameras(sem, size):
    """{name: 12 float32} for CAMERAS, placed for this grid and render size"""
    h, w = size
    X, Y, Z = sem.shape
    f, cx, cy = 0.4 * max(w, h), w / 2.0, h / 2.0
    free = _voxel_near_centre(sem, False)
    occ = _voxel_near_centre(sem, True)
    look_free, look_face = LOOK[tuple(sem.shape)]
    out = {
        'inside_free': _cam(free + np.array([0.3, 0.6, 0.45]), look_free, f, cx, cy),
        'inside_occupied': _cam(occ + np.array([0.5, 0.4, 0.6]), (-0.4, 1.0, 0.15), f, cx, cy),
        'on_face': _cam(free + np.array([0.0, 0.5, 0.5]), look_face, f, cx, cy),                  # x exactly on a voxel face
        'outside_in': _cam((-2.5, Y * 0.45, Z * 0.6), (1.0, 0.1, -0.05), f, cx, cy),
        'outside_away': _cam((-2.5, Y * 0.45, Z * 0.6), (-1.0, 0.1, 0.05), f, cx, cy),
    }
    # looking along +x with right = -y, down = -z, a power-of-two focal length and the principal point on a pixel centre: the
    # pixel there has dir_y = dir_z = 0 exactly, so its ray has two zero components (the DBL_MAX branch of the set-up)
    k, m = w // 2, h // 2
    o = np.asarray(PC_MIN) + np.array([-1.25, min(Y - 1, 2) + 0.25, min(Z - 1, 1) + 0.75]) * VOXEL
    fa = 8.0
    D = np.array([[0.0, 0.0, 1.0], [-1 / fa, 0.0, (k + 0.5) / fa], [0.0, -1 / fa, (m + 0.5) / fa]])
    out['axis_zero'] = np.concatenate([o, D.reshape(-1)]).astype(np.float32)
    assert tuple(out) == CAMERAS
    return out


def batch(name, dtype, size, seed=0):
    """B = 2, V = 3: sample 0 sees its grid through the three cameras inside it, sample 1 through the three outside ones.
    -> sems [2 x (X, Y, Z)], gts, cams (2, 3, 12) float32"""
    shape = GRIDS[name]
    sems = [grid(shape, dtype, 100 + 7 * seed + b) for b in range(2)]
    gts = [edited(s, 200 + 7 * seed + b) for b, s in enumerate(sems)]
    cams = np.stack([np.stack([cameras(s, size)[c] for c in CAMERAS[3 * b:3 * b + 3]]) for b, s in enumerate(sems)])
    return sems, gts, cams


def frames(B, V, hw, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, V, hw[0], hw[1], 3)).astype(np.uint8)


def palettes(seed=9):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (256, 3)).astype(np.uint8), rng.integers(0, 256, (6, 3)).astype(np.uint8)
