"""The scenes of the camera visibility tests: those of tests/render_cases.py where the cameras inside the grid see between 5 %
and 95 % of its voxels at every raster but 1 x 1, with an occupied voxel seen and an occupied voxel hidden, and seeded scenes
of the same make otherwise.

'4x4x32' at render_cases' density of 0.25 stops a ray after four voxels on average, and a 9 x 70 raster then sees 3.5 % of the
512 voxels: its scene here is the same seeded grid at a lower density (the top-bit voxels of render_cases.grid included), with
the two free-standing inside cameras turned to look along the grid's long axis.  '3x9x1' at 0.25 has three occupied voxels in
sample 0, all of them seen: its scene here is the same seeded grid at a higher density, which hides four of seven.
tests/test_visibility_host.py checks the conditions for every scene from the reference alone."""
import numpy as np

from tests import render_cases as rc

DENSITY = {'4x4x32': 0.06, '3x9x1': 0.4}             # grids whose scene is made here; every other grid is render_cases.batch's
# their inside_free and on_face cameras look along the long axis of the grid instead of across its four voxels
LOOK = {'4x4x32': ((0.15, 0.1, -1.0), (0.1, -0.15, 1.0))}


def cameras(name, sem, size):
    """{camera name: 12 float32} in render_cases.CAMERAS' order, placed for this grid and raster"""
    out = rc.cameras(sem, size)
    if name in LOOK:
        h, w = size
        f, cx, cy = 0.4 * max(w, h), w / 2.0, h / 2.0
        free = rc._voxel_near_centre(sem, False)
        look_free, look_face = LOOK[name]
        out['inside_free'] = rc._cam(free + np.array([0.3, 0.6, 0.45]), look_free, f, cx, cy, up=(0.0, 1.0, 0.0))
        out['on_face'] = rc._cam(free + np.array([0.0, 0.5, 0.5]), look_face, f, cx, cy, up=(0.0, 1.0, 0.0))
    return out


def batch(name, dtype, size, seed=0):
    """B = 2, V = 3 in render_cases.batch's layout -> sems [2 x (X, Y, Z)], cams (2, 3, 12) float32"""
    if name in DENSITY:
        sems = [rc.grid(rc.GRIDS[name], dtype, 100 + 7 * seed + b, DENSITY[name]) for b in range(2)]
    else:
        sems = rc.batch(name, dtype, size, seed)[0]
    cams = np.stack([np.stack([cameras(name, s, size)[c] for c in rc.CAMERAS[3 * b:3 * b + 3]]) for b, s in enumerate(sems)])
    return sems, cams
