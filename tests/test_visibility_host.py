"""not-gpu: the reference of the camera visibility masks (tests/visibility_ref.py) is pinned to the plain-C caster of oracle/,
its scenes are shown not to be vacuous from the reference alone, the IoU reference is checked on a hand-worked example, and the
C ABI of include/occnet_amd_visibility.h is bound and validates its arguments without a GPU."""
import ctypes
import math

import numpy as np
import pytest

from occnet_amd import _lib
from tests import render_cases as rc, render_ref, visibility_cases as vc, visibility_ref as vr

DTYPES = ('uint8', 'int64')


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(rc.GRIDS))
def test_reference_walk_ends_where_the_plain_c_caster_does(name, dtype):
    """Every ray's last visited voxel and its dist equal what the plain-C caster reports, bit for bit, on the scenes of
    tests/render_cases.py (and on those tests/visibility_cases.py makes itself): all sizes, all six cameras, each through its
    sample of batch()'s B = 2, V = 3 layout.  The rays go to the caster through render_ref.cast_view's own float32 statements,
    so the reference's ray statements are pinned with its walk."""
    oracle = render_ref.oracle_caster()
    own = name in vc.DENSITY                          # a scene of tests/visibility_cases.py: pinned as well
    rays = 0
    for scenes in ('render', 'visibility') if own else ('render',):
        for size in rc.SIZES:
            sems, cams = vc.batch(name, np.dtype(dtype), size) if scenes == 'visibility' else \
                rc.batch(name, np.dtype(dtype), size)[::2]
            for b in range(2):
                for k, camera in enumerate(rc.CAMERAS[3 * b:3 * b + 3]):
                    seen = {}

                    def recording(sigma, origin, points, tindex):
                        dist, coord = oracle(sigma, origin, points, tindex)
                        seen['dist'], seen['coord'] = dist[0].numpy().astype(np.float32), coord[0].numpy().astype(np.int64)
                        return dist, coord
                    render_ref.cast_view(sems[b], cams[b, k], rc.PC_MIN, rc.VOXEL, size, rc.FREE, rc.FAR, recording)
                    walks = vr.case_walks(name, dtype, size, camera, b, scenes=scenes)
                    assert len(walks) == size[0] * size[1] == len(seen['dist'])
                    for n, (visited, dist) in enumerate(walks):
                        last = visited[-1] if visited else (0, 0, 0)
                        assert tuple(seen['coord'][n]) == last, (scenes, size, camera, n)
                        assert np.float32(dist).view(np.uint32) == seen['dist'][n].view(np.uint32), (scenes, size, camera, n)
                        assert (dist == -1) == (not visited)
                    rays += len(walks)
    assert rays == (2 if own else 1) * 6 * sum(h * w for h, w in rc.SIZES)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(rc.GRIDS))
def test_no_scene_is_vacuous(name, dtype):
    """A condition on the inputs, from the reference alone: sample 0 (cameras inside the grid) has between 5 % and 95 % of its
    voxels marked, with an occupied voxel marked and an occupied voxel unmarked; the camera that looks away marks nothing."""
    for size in rc.SIZES:
        if size == (1, 1):
            continue
        sems, _ = vc.batch(name, np.dtype(dtype), size)
        mask = vr.case_mask(name, dtype, size)
        share = float(mask[0].mean())
        assert 0.05 <= share <= 0.95, (name, size, share)
        occupied = sems[0] != rc.FREE
        assert (mask[0][occupied] == 1).any() and (mask[0][occupied] == 0).any(), (name, size)
        away = vr.mask_of(vr.case_walks(name, dtype, size, 'outside_away', 1), sems[1].shape)
        assert not away.any(), (name, size)
        assert all(not visited and dist == -1 for visited, dist in vr.case_walks(name, dtype, size, 'outside_away', 1))


def test_walk_consequences_of_the_definition():
    """A camera inside an occupied voxel marks only that voxel; the walk is not cut at `far`."""
    sems, _ = vc.batch('5x6x4', np.dtype('uint8'), (7, 13))
    walks = vr.case_walks('5x6x4', 'uint8', (7, 13), 'inside_occupied', 0)
    cells = {c for visited, _ in walks for c in visited}
    assert len(cells) == 1 and sems[0][next(iter(cells))] != rc.FREE
    cam = rc.cameras(sems[0], (7, 13))['inside_free']
    near = vr.view_walks(sems[0], cam, rc.PC_MIN, rc.VOXEL, (7, 13), rc.FREE, far=0.05)
    far = vr.view_walks(sems[0], cam, rc.PC_MIN, rc.VOXEL, (7, 13), rc.FREE, far=rc.FAR)
    longest = max(len(v) for v, _ in near)
    assert longest * rc.VOXEL > 10 * 0.05                                # walks run many times further than far = 5 cm
    assert sum(v1 == v2 for (v1, _), (v2, _) in zip(near, far)) > len(near) // 2      # and mostly visit the same voxels


def test_iou_reference_on_a_hand_worked_example():
    """free_id = 2 (classes 0, 1 and free).  Nine admitted voxels, ground truth -> prediction:
         0 -> 0 twice, 0 -> free once, free -> free four times, free -> 0 once, and one voxel with prediction id 7 (skipped).
       class 0: TP 2, FN 1, FP 1 -> 2 / 4.  class 1: in neither grid -> NaN.  free: TP 4, FN 1, FP 1 -> 4 / 6.
       miou = nanmean(0.5, NaN) = 0.5.  occupied vs free: both occupied 2, union = 8 - 4 = 4 -> 0.5.  Two more voxels are masked
       out and change nothing."""
    gt = np.array([0, 0, 0, 2, 2, 2, 2, 2, 2, 1, 0], np.int64)
    pred = np.array([0, 0, 2, 2, 2, 2, 2, 0, 7, 1, 1], np.int64)
    mask = np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0], np.uint8)
    state = vr.confusion(pred, gt, mask, free_id=2)
    assert state.tolist() == [[2, 0, 1], [0, 0, 0], [1, 0, 4], [1, 9, 0]]
    iou, miou, occupied = vr.iou(state[:3], 2)
    assert iou[0] == 0.5 and math.isnan(iou[1]) and iou[2] == 4 / 6
    assert miou == 0.5 and occupied == 0.5
    unmasked = vr.confusion(pred, gt, None, free_id=2)
    assert unmasked[3].tolist() == [1, 11, 0] and unmasked[1, 1] == 1 and unmasked[0, 1] == 1
    # the product's host arithmetic (VoxelMIoU.compute) agrees with the class-by-class reference, NaN included
    from occnet_amd.metrics.voxel_miou import iou_from_confusion
    got_iou, got_miou, got_occupied = iou_from_confusion(state[:3], 2)
    assert np.array_equal(got_iou, iou, equal_nan=True) and got_miou == miou and got_occupied == occupied
    empty_iou, empty_miou, empty_occ = iou_from_confusion(np.zeros((3, 3), np.int64), 2)
    assert np.isnan(empty_iou).all() and math.isnan(empty_miou) and math.isnan(empty_occ)


def _header_prototypes():
    (header,) = _lib.EXTRA_HEADERS
    with open(header) as f:
        return _lib.prototypes(f.read())


def test_new_header_is_exported_and_bound():
    protos = _header_prototypes()
    assert sorted(protos) == ['occ_confusion_accumulate', 'occ_confusion_state_words', 'occ_visibility_views',
                              'occ_visibility_workspace_bytes']
    lib = _lib.lib()
    for name, (restype, params) in protos.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params) and list(fn.argtypes) == [t for t, _ in params], name
        assert fn.restype is restype and restype is not None, name
    for name in ('occ_visibility_workspace_bytes', 'occ_confusion_state_words'):
        assert getattr(lib, name).restype is ctypes.c_int64, name
    assert lib.occ_visibility_views.restype is ctypes.c_int and lib.occ_confusion_accumulate.restype is ctypes.c_int
    assert [n for _, n in protos['occ_confusion_accumulate'][1]] == ['sem_pred', 'sem_pred_dtype', 'sem_gt', 'sem_gt_dtype',
                                                                     'mask', 'free_id', 'state', 'n_voxels', 'stream']
    assert protos['occ_visibility_views'][1][11] == (ctypes.c_int64, 'workspace_bytes')
    # the defaults keep reading the main header only
    main = _lib.prototypes()
    assert sorted(main) == _lib.declared_symbols() and not set(main) & set(protos)
    assert lib.occ_abi_version() == _lib.ABI == 3


def test_size_queries():
    lib = _lib.lib()
    # uint16 pillar masks up to Z = 16, uint32 beyond, each section rounded up to 256 bytes; one uint32 word per pillar behind
    assert lib.occ_visibility_workspace_bytes(1, 200, 200, 16) == 200 * 200 * 2 + 200 * 200 * 4 + 128
    assert lib.occ_visibility_workspace_bytes(2, 7, 5, 17) == 512 + 512
    assert lib.occ_visibility_workspace_bytes(1, 4, 4, 33) == 0 and lib.occ_visibility_workspace_bytes(0, 4, 4, 4) == 0
    assert lib.occ_visibility_workspace_bytes(1 << 10, 1 << 10, 1 << 10, 32) == (1 << 30) * 8
    assert lib.occ_confusion_state_words(16) == 18 * 17 and lib.occ_confusion_state_words(1) == 6
    assert lib.occ_confusion_state_words(31) == 33 * 32
    assert lib.occ_confusion_state_words(0) == 0 and lib.occ_confusion_state_words(32) == 0


def test_argument_validation_without_gpu():
    """Every refusal comes back as an error code with occ_last_error text, before any launch."""
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_double * 512)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 1)
    f = ctypes.c_float
    i64 = ctypes.c_int64

    def views(sem=p, dtype=0, cams=p, voxel=0.5, free_id=16, far=100.0, mask=p, ws=p, ws_bytes=4096, B=1, V=1, X=4, Y=4, Z=4,
              h=8, w=8):
        return lib.occ_visibility_views(sem, dtype, cams, f(0.0), f(0.0), f(0.0), f(voxel), free_id, f(far), mask, ws,
                                        i64(ws_bytes), B, V, X, Y, Z, h, w, null)

    def refused(rc, code, text):
        assert rc == code and text in lib.occ_last_error(), (rc, lib.occ_last_error())

    refused(views(sem=null), -1, b'null pointer')
    refused(views(ws=null), -1, b'null pointer')
    refused(views(cams=null), -1, b'null pointer')
    refused(views(mask=null), -1, b'null pointer')
    for bad in (dict(B=0), dict(X=0), dict(Y=-1), dict(Z=0), dict(V=0)):
        refused(views(**bad), -1, b'bad dimension')
    refused(views(Z=33), -3, b'Z <= 32')
    with pytest.raises(_lib.OccAmdUnsupported):
        _lib.check(views(Z=33), 'visibility_views')
    refused(views(free_id=0), -1, b'free_id')
    refused(views(free_id=32), -1, b'free_id')
    refused(views(dtype=2), -1, b'dtype code')
    need = lib.occ_visibility_workspace_bytes(1, 4, 4, 4)
    assert need == 512
    refused(views(ws_bytes=need - 1), -1, b'workspace too small')
    refused(views(ws_bytes=255), -1, b'workspace too small')             # short of the pillar masks alone
    refused(views(ws=odd), -1, b'4-byte aligned')
    refused(views(h=0), -1, b'bad dimension')
    refused(views(w=0), -1, b'bad dimension')
    refused(views(w=16385), -1, b'bad dimension')
    refused(views(B=256, V=256, ws_bytes=1 << 20), -1, b'bad dimension')             # B * V > 65535
    refused(views(voxel=0.0), -1, b'voxel_size')
    refused(views(far=0.0), -1, b'far')
    refused(views(far=float('inf')), -1, b'far')

    def conf(pred=p, pd=0, gt=p, gd=0, mask=null, free_id=16, state=p, n=64):
        return lib.occ_confusion_accumulate(pred, pd, gt, gd, mask, free_id, state, i64(n), null)

    refused(conf(pred=null), -1, b'null pointer')
    refused(conf(gt=null), -1, b'null pointer')
    refused(conf(state=null), -1, b'null pointer')
    refused(conf(pd=2), -1, b'dtype code')
    refused(conf(gd=-1), -1, b'dtype code')
    refused(conf(free_id=0), -1, b'free_id')
    refused(conf(free_id=32), -1, b'free_id')
    refused(conf(n=0), -1, b'bad dimension')
    refused(conf(n=(1 << 40) + 1), -1, b'bad dimension')
    refused(conf(state=odd), -1, b'8-byte aligned')
    refused(conf(pred=odd, pd=1), -1, b'8-byte aligned')


def test_python_wrappers_refuse_host_tensors():
    import torch
    from occnet_amd import ext
    sem = torch.zeros(1, 4, 4, 4, dtype=torch.uint8)
    with pytest.raises(_lib.OccAmdError, match='no CPU fallback'):
        ext.visibility_views(sem, torch.zeros(1, 1, 12), (0., 0., 0.), 0.5, (4, 4))
    with pytest.raises(_lib.OccAmdError, match='no CPU fallback'):
        ext.confusion_accumulate(torch.zeros(18 * 17, dtype=torch.int64), sem, sem)
    with pytest.raises(_lib.OccAmdError, match='free_id'):
        ext.confusion_state_words(0)
    assert ext.visibility_workspace_bytes(1, 4, 4, 4) == 512 and ext.confusion_state_words(16) == 306
