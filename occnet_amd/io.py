"""Data formats either side of the hot path: what the reference's dataset / pipeline
classes hand to the model and what its evaluation writes — restated on numpy/torch without mmcv, pyquaternion
or the nuScenes devkit.  Host-side formatting only (no model compute lives here).

  pad_multiview / normalize_multiview / to_batch   P/datasets/pipelines/transform_3d.py:12-101
                                                   (PadMultiViewImage size_divisor=32, NormalizeMultiviewImage)
  random_scale_multiview / scale_img_metas         P/datasets/pipelines/transform_3d.py:292-331
                                                   (RandomScaleImageMultiViewImage: the resize as this project defines it,
                                                   DESIGN.md "Image scale on the device", and the meta keys it rewrites;
                                                   the device chain is ext.input_u8_scaled)
  sample_photometric / photometric_distort         P/datasets/pipelines/transform_3d.py:102-189
                                                   (PhotoMetricDistortionMultiViewImage: the draws, and the host chain;
                                                   the device chain is ext.train_input_u8)
  quaternion_rotation_matrix, transform_matrix     pyquaternion / nuscenes.utils.geometry_utils, as used at
                                                   P/datasets/nuscenes_occ.py:82-86
  camera_matrices                                  P/datasets/nuscenes_occ.py:87-120 (lidar2img = K_pad @ lidar2cam)
  load_occ_gt / save_occ_gt                        P/datasets/pipelines/loading.py:21-33 (.npz: semantics, flow)
  make_img_meta                                    the img_metas keys the path consumes (encoder.py:94-101,133-134)
  lidar_origins                                    tools/ray_iou/ego_pose_extractor.py:84-121 (origins the rays start from)
  format_submission / read_submission              P/datasets/nuscenes_occ.py:189-257 (submission.gz)
  format_submission_device                         the same file from device tensors (metrics.SubmissionWriter: the one
                                                   exception to "no compute here" — it drives csrc/submission_rays.hip)
  merge_submission_parts                           the parts of a multi-rank run -> one submission.gz (host only)
"""
import gzip
import os
import pickle

import numpy as np
import torch


# ----------------------------------------------------------------------------- images
def pad_multiview(imgs, size_divisor=32, size=None, pad_val=0):
    """imgs: list of (H, W, C) arrays -> (padded list, meta dict).  Pads bottom/right to `size` (h, w) or to
    the next multiple of `size_divisor` (mmcv.impad / impad_to_multiple semantics): 900x1600 -> 928x1600."""
    assert (size is None) != (size_divisor is None)
    out = []
    for img in imgs:
        h, w = img.shape[:2]
        if size is not None:
            ph, pw = size
        else:
            ph = int(np.ceil(h / size_divisor)) * size_divisor
            pw = int(np.ceil(w / size_divisor)) * size_divisor
        assert ph >= h and pw >= w
        pad = np.full((ph, pw) + img.shape[2:], pad_val, dtype=img.dtype)
        pad[:h, :w] = img
        out.append(pad)
    meta = dict(ori_shape=[i.shape for i in imgs], img_shape=[i.shape for i in out],
                pad_shape=[i.shape for i in out], pad_fixed_size=size, pad_size_divisor=size_divisor)
    return out, meta


def normalize_multiview(imgs, mean, std, to_rgb=True):
    """((img[..., ::-1] if to_rgb) - mean) * (1 / std) in float32: mmcv.imnormalize subtracts the mean and multiplies
    by the reciprocal of std (formed in float64), it does not divide (NormalizeMultiviewImage, transform_3d.py:82-94)."""
    mean = np.asarray(mean, dtype=np.float32).reshape(1, 1, -1)
    std = np.asarray(std, dtype=np.float32).reshape(1, 1, -1)
    stdinv = (1 / np.float64(std)).astype(np.float32)
    out = []
    for img in imgs:
        x = img.astype(np.float32)
        if to_rgb:
            x = x[..., ::-1]
        out.append((x - mean) * stdinv)
    return out, dict(mean=mean.reshape(-1), std=std.reshape(-1), to_rgb=to_rgb)


def check_scale(scale):
    """-> float(scale); ValueError unless it is finite and positive."""
    s = float(scale)
    if not (np.isfinite(s) and s > 0.0):
        raise ValueError(f"image scale must be finite and positive, got {scale!r}")
    return s


def scaled_size(h, w, scale):
    """(Hd, Wd) = (int(h * scale), int(w * scale)): RandomScaleImageMultiViewImage truncates after a double multiply.
    ValueError for a scale that is not finite and positive, or that leaves no pixel."""
    s = check_scale(scale)
    hd, wd = int(h * s), int(w * s)
    if hd < 1 or wd < 1:
        raise ValueError(f"image scale {s} leaves no pixel of a ({h}, {w}) image: ({hd}, {wd})")
    return hd, wd


def resize_taps(n_src, n_dst, reset_fraction):
    """One axis of the linear resize n_src -> n_dst (DESIGN.md "Image scale on the device"): for every destination index d
        f = float32((d + 0.5) * scale - 0.5), scale = 1.0 / (n_dst / n_src) in float64;  i = floor(f);  f = f - float32(i)
    reset_fraction (the columns): i < 0 -> i = 0, f = 0 and i >= n_src - 1 -> i = n_src - 1, f = 0; otherwise (the rows) f
    stays and only the indices are clipped.  -> (i0, i1 int64 (n_dst,), w0 = 1 - f, w1 = f float32 (n_dst,))."""
    scale = 1.0 / (np.float64(n_dst) / np.float64(n_src))
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    fl = np.floor(f)
    i = fl.astype(np.int64)
    f = f - fl
    if reset_fraction:
        f = np.where((i < 0) | (i >= n_src - 1), np.float32(0), f)
    i0 = np.clip(i, 0, n_src - 1)
    i1 = np.clip(i + 1, 0, n_src - 1) if not reset_fraction else np.minimum(i0 + 1, n_src - 1)
    return i0, i1, np.float32(1) - f, f


def random_scale_multiview(imgs, scale):
    """RandomScaleImageMultiViewImage(scales=[scale]) on the images: list of float32 (H, W, C) arrays -> (resized list of
    (int(H * scale), int(W * scale), C) float32 arrays, meta dict).  The bilinear resize in float32, every operation
    rounded: columns first (h = x[r, c0] * a0 + x[r, c1] * a1 for both rows), then rows (h0 * b0 + h1 * b1), taps and
    weights from resize_taps.  The metas' side of the transform is scale_img_metas."""
    out = []
    for img in imgs:
        assert img.dtype == np.float32 and img.ndim == 3
        hd, wd = scaled_size(img.shape[0], img.shape[1], scale)
        r0, r1, b0, b1 = resize_taps(img.shape[0], hd, reset_fraction=False)
        c0, c1, a0, a1 = resize_taps(img.shape[1], wd, reset_fraction=True)
        a0, a1 = a0[None, :, None], a1[None, :, None]
        h0 = img[r0][:, c0] * a0 + img[r0][:, c1] * a1
        h1 = img[r1][:, c0] * a0 + img[r1][:, c1] * a1
        out.append(h0 * b0[:, None, None] + h1 * b1[:, None, None])
    return out, dict(scale=float(scale), img_shape=[i.shape for i in out], ori_shape=[i.shape for i in out])


def scale_img_metas(meta, scale, src_hw, size_divisor=32):
    """The img_meta of one sample after RandomScaleImageMultiViewImage(scales=[scale]) and PadMultiViewImage(size_divisor) on
    (Hs, Ws) = src_hw frames -> a copy of `meta` with
        lidar2img     diag(scale, scale, 1, 1) @ lidar2img per view (the scale itself, not the size ratio, as the reference)
        ori_shape     (Hd, Wd, 3) per view
        img_shape, pad_shape   (H, W, 3) per view, the padded size the model is fed
    and every other key (cam_intrinsic among them, as in the reference) as it was."""
    hd, wd = scaled_size(src_hw[0], src_hw[1], scale)
    d = int(size_divisor)
    H, W = (hd + d - 1) // d * d, (wd + d - 1) // d * d
    factor = np.eye(4)
    factor[0, 0] = factor[1, 1] = float(scale)
    out = dict(meta)
    out['lidar2img'] = [factor @ np.asarray(m) for m in meta['lidar2img']]
    views = len(out['lidar2img'])
    out['ori_shape'] = [(hd, wd, 3)] * views
    out['img_shape'] = [(H, W, 3)] * views
    out['pad_shape'] = [(H, W, 3)] * views
    return out


_EPS32 = np.float32(np.finfo(np.float32).eps)     # FLT_EPSILON


def bgr2hsv_f32(img):
    """(..., 3) float32 BGR -> HSV (h in degrees, s, v): OpenCV's float path (RGB2HSV_f) restated in float32 numpy
    — what mmcv.bgr2hsv runs on a float32 image.  cv2 is not vendored by the reference; this is a restatement from
    the published algorithm ("Training input from uint8 frames")."""
    assert img.dtype == np.float32
    b, g, r = img[..., 0], img[..., 1], img[..., 2]
    v = np.maximum(np.maximum(b, g), r)
    vmin = np.minimum(np.minimum(b, g), r)
    diff = v - vmin
    s = diff / (np.abs(v) + _EPS32)
    k = np.float32(60) / (diff + _EPS32)
    h = np.where(v == r, (g - b) * k, np.where(v == g, (b - r) * k + np.float32(120), (r - g) * k + np.float32(240)))
    h = np.where(h < 0, h + np.float32(360), h)
    return np.stack([h, s, v], -1).astype(np.float32)


def hsv2bgr_f32(img):
    """(..., 3) float32 HSV (h in degrees) -> BGR: OpenCV's float path (HSV2RGB_f) restated in float32 numpy."""
    assert img.dtype == np.float32
    h, s, v = img[..., 0], img[..., 1], img[..., 2]
    h = h * np.float32(1.0 / 60.0)
    while (h < 0).any():
        h = np.where(h < 0, h + np.float32(6), h)
    while (h >= 6).any():
        h = np.where(h >= 6, h - np.float32(6), h)
    fl = np.floor(h)
    over = fl >= 6
    sector = np.where(over, 0, fl).astype(np.int64)
    f = np.where(over, np.float32(0), h - fl)
    one = np.float32(1)
    tab = np.stack([v, v * (one - s), v * (one - s * f), v * (one - s * (one - f))], -1)
    idx = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    bgr = np.take_along_axis(tab, idx[sector], -1)
    return np.where((s == 0)[..., None], v[..., None], bgr).astype(np.float32)


PHOTOMETRIC_IDENTITY = np.array([0, 1, 1, 0, 1, 0, 1, 2], dtype=np.float32)


def identity_photometric(n_images):
    """Records that switch every stage of the distortion off."""
    return np.tile(PHOTOMETRIC_IDENTITY, (int(n_images), 1))


def sample_photometric(n_images, brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5),
                       hue_delta=18):
    """The random draws of PhotoMetricDistortionMultiViewImage for `n_images` images, made from numpy's GLOBAL RNG in
    the reference's order (transform_3d.py:146-186), so a run seeded like the reference distorts alike.
    -> (n_images, 8) float32 records [delta, alpha_pre, sat, hue, alpha_post, perm0, perm1, perm2]: a stage that was
    not drawn holds its identity (0, 1, 1, 0, 1, 0 1 2).  alpha_pre is the contrast applied before the HSV round trip
    (the reference's mode == 1), alpha_post the one after it (mode == 0).  Values are rounded to float32: the
    reference applies them in place to float32 arrays."""
    rng = np.random
    lo_c, hi_c = contrast_range
    lo_s, hi_s = saturation_range
    rec = identity_photometric(n_images)
    for r in rec:
        if rng.randint(2):
            r[0] = rng.uniform(-brightness_delta, brightness_delta)
        mode = rng.randint(2)
        if mode == 1:
            if rng.randint(2):
                r[1] = rng.uniform(lo_c, hi_c)
        if rng.randint(2):
            r[2] = rng.uniform(lo_s, hi_s)
        if rng.randint(2):
            r[3] = rng.uniform(-hue_delta, hue_delta)
        if mode == 0:
            if rng.randint(2):
                r[4] = rng.uniform(lo_c, hi_c)
        if rng.randint(2):
            r[5:8] = rng.permutation(3)
    return rec


def photometric_distort(imgs, records):
    """PhotoMetricDistortionMultiViewImage.__call__ with the draws given: imgs = list of (H, W, 3) uint8 or float32 BGR
    arrays, records from sample_photometric.  The reference's statements in float32 numpy, in its order; a stage
    whose record value is the identity is skipped, as the reference skips a stage it did not draw.
    -> list of new (H, W, 3) float32 arrays.  The host twin of ext.train_input_u8's first five steps."""
    records = np.asarray(records, dtype=np.float32).reshape(len(imgs), 8)
    out = []
    for img, (delta, a_pre, sat, hue, a_post, p0, p1, p2) in zip(imgs, records):
        img = np.array(img, dtype=np.float32)
        if delta != 0:
            img += delta
        if a_pre != 1:
            img *= a_pre
        img = bgr2hsv_f32(img)
        if sat != 1:
            img[..., 1] *= sat
        if hue != 0:
            img[..., 0] += hue
            img[..., 0][img[..., 0] > 360] -= 360
            img[..., 0][img[..., 0] < 0] += 360
        img = hsv2bgr_f32(img)
        if a_post != 1:
            img *= a_post
        perm = [int(p0), int(p1), int(p2)]
        if perm != [0, 1, 2]:
            img = img[..., perm]
        out.append(img)
    return out


def to_batch(imgs):
    """list of (H, W, 3) float arrays -> (1, N, 3, H, W) float32 tensor (DefaultFormatBundle3D + collate)."""
    x = np.stack([np.ascontiguousarray(i.transpose(2, 0, 1)) for i in imgs], 0)
    return torch.from_numpy(x.astype(np.float32))[None]


# ----------------------------------------------------------------------------- geometry
def quaternion_rotation_matrix(q):
    """Unit quaternion (w, x, y, z) -> 3x3 rotation matrix (pyquaternion.Quaternion.rotation_matrix)."""
    w, x, y, z = (np.asarray(q, dtype=np.float64) / np.linalg.norm(q)).tolist()
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def transform_matrix(translation, rotation, inverse=False):
    """4x4 homogeneous transform from a translation and a (w, x, y, z) quaternion or 3x3 matrix
    (nuscenes.utils.geometry_utils.transform_matrix)."""
    R = np.asarray(rotation, dtype=np.float64)
    if R.shape != (3, 3):
        R = quaternion_rotation_matrix(R)
    t = np.asarray(translation, dtype=np.float64)
    tm = np.eye(4)
    if inverse:
        tm[:3, :3] = R.T
        tm[:3, 3] = R.T @ (-t)
    else:
        tm[:3, :3] = R
        tm[:3, 3] = t
    return tm


def camera_matrices(cams):
    """cams: iterable of dicts with `sensor2lidar_rotation` (3x3 matrix or quaternion),
    `sensor2lidar_translation` (3,), `cam_intrinsic` (3x3) -> (lidar2img, cam_intrinsic, lidar2cam) lists of
    4x4 arrays, built exactly as the reference does (nuscenes_occ.py:96-113)."""
    lidar2img, intrinsics, lidar2cam = [], [], []
    for cam in cams:
        rot = np.asarray(cam['sensor2lidar_rotation'], dtype=np.float64)
        if rot.shape != (3, 3):
            rot = quaternion_rotation_matrix(rot)
        lidar2cam_r = np.linalg.inv(rot)
        lidar2cam_t = np.asarray(cam['sensor2lidar_translation'], dtype=np.float64) @ lidar2cam_r.T
        rt = np.eye(4)
        rt[:3, :3] = lidar2cam_r.T
        rt[3, :3] = -lidar2cam_t
        intrinsic = np.array(cam['cam_intrinsic'], dtype=np.float32)
        viewpad = np.eye(4)
        viewpad[:intrinsic.shape[0], :intrinsic.shape[1]] = intrinsic
        lidar2img.append(viewpad @ rt.T)
        intrinsics.append(viewpad)
        lidar2cam.append(rt.T)
    return lidar2img, intrinsics, lidar2cam


def make_img_meta(cams, lidar2ego_translation, lidar2ego_rotation, img_shapes, can_bus=None,
                  prev_bev_exists=False, **extra):
    """The img_meta dict of one sample with the keys the hot path reads."""
    lidar2img, intr, l2c = camera_matrices(cams)
    meta = dict(lidar2img=lidar2img, cam_intrinsic=intr, lidar2cam=l2c,
                ego2lidar=transform_matrix(lidar2ego_translation, lidar2ego_rotation, inverse=True),
                img_shape=list(img_shapes), can_bus=np.zeros(18) if can_bus is None else np.asarray(can_bus),
                prev_bev_exists=prev_bev_exists)
    meta.update(extra)
    return meta


PSEUDO_LIDAR2EGO = np.array([[0., 1., 0., 0.94], [-1., 0., 0., 0.], [0., 0., 1., 1.84], [0., 0., 0., 1.]])


_SCENE_FRAMES = {}      # id(data_infos) -> (list object, (len, dataset_type), {scene: [frames]})


def lidar_origins(data_infos, index, dataset_type='openocc_v2', max_origins=8, xy_range=39.0):
    """Lidar origins the ray metric / the submission cast from for sample `index`: the lidar position of EVERY frame
    of the sample's scene expressed in the sample's ego frame, kept when |x|, |y| < 39 m, thinned to 8 evenly spaced
    ones (reference tools/ray_iou/ego_pose_extractor.py:84-121, driven by nuscenes_occ.py:142-166,196-224).
    data_infos: the nuScenes info dicts (`token`, `lidar2ego_translation/rotation`, `ego2global_translation/rotation`,
    `scene_token` or `occ_path`).  -> (token, float tensor (1, T, 3)) — the batch a DataLoader(batch_size=1) yields."""
    def scene_of(info):
        if dataset_type == 'openocc_v2' and 'scene_token' not in info:
            return info['occ_path'].split('openocc_v2/')[-1].split('/')[0]
        return info['scene_token']

    def ego_from_lidar(info):
        if dataset_type == 'lightwheelocc':
            return PSEUDO_LIDAR2EGO
        return transform_matrix(info['lidar2ego_translation'], info['lidar2ego_rotation'])

    def global_from_lidar(info):
        return transform_matrix(info['ego2global_translation'], info['ego2global_rotation']).dot(ego_from_lidar(info))
    info = data_infos[index]
    # scene -> frame list, built once per data_infos list (a rescan per call is O(N^2) over a dataset: ADVICE r3)
    cache = _SCENE_FRAMES.get(id(data_infos))
    if cache is None or cache[0] is not data_infos or cache[1] != (len(data_infos), dataset_type):
        by_scene = {}
        for f in data_infos:
            by_scene.setdefault(scene_of(f), []).append(f)
        cache = (data_infos, (len(data_infos), dataset_type), by_scene)
        _SCENE_FRAMES.clear()
        _SCENE_FRAMES[id(data_infos)] = cache
    frames = cache[2][scene_of(info)]
    ref_index = next(i for i, f in enumerate(frames) if f is info)
    ref_lidar_from_global = np.linalg.inv(global_from_lidar(info))
    ref_ego_from_lidar = ego_from_lidar(info)
    origins = []
    for i, frame in enumerate(frames):
        if i == ref_index:
            o = np.array([0.0, 0.0, 0.0], dtype=np.float32)
        else:
            o = np.array(ref_lidar_from_global.dot(global_from_lidar(frame))[:3, 3], dtype=np.float32)
        pad = np.ones([4])
        pad[:3] = o
        o = np.dot(ref_ego_from_lidar[:3], pad.T).T
        if np.abs(o[0]) < xy_range and np.abs(o[1]) < xy_range:
            origins.append(o)
    if len(origins) > max_origins:
        sel = np.round(np.linspace(0, len(origins) - 1, max_origins)).astype(np.int64)
        origins = [origins[i] for i in sel]
    return info['token'], torch.from_numpy(np.stack(origins))[None]


# ----------------------------------------------------------------------------- occupancy ground truth
OCC_SHAPE = (200, 200, 16)


def load_occ_gt(path, shape=OCC_SHAPE):
    """-> (semantics uint8 shape, flow float32 shape+(2,)); zeros when the file is absent, as the reference."""
    if path is not None and os.path.exists(path):
        z = np.load(path)
        return z['semantics'], z['flow']
    return np.zeros(shape, dtype=np.uint8), np.zeros(tuple(shape) + (2,), dtype=np.float32)


def save_occ_gt(path, semantics, flow):
    np.savez_compressed(path, semantics=np.asarray(semantics, dtype=np.uint8),
                        flow=np.asarray(flow, dtype=np.float32))


# ----------------------------------------------------------------------------- submission
SUBMISSION_HEADER = {
    'method': 'XXXXX (Your method name)', 'team': 'XXXXX (Your team name)', 'authors': "XXXXX (Authors)",
    'e-mail': "XXXXX (Your email)", 'institution / company': "XXXXXXXXXX (Your affiliation)",
    'country / region': "XXXXXXX (Your country/region)"}


def format_submission(samples, submission_prefix, header=None, device='cuda'):
    """samples: iterable of (token, sem_pred (200,200,16) ints, flow_pred (200,200,16,2), lidar origins
    (1, T, 3) tensor in ego metres).  Casts the 14 040 lidar rays per origin through every prediction (HIP
    DVR kernel) and writes `<prefix>/submission.gz` = gzip(pickle({... 'results': {token: {pcd_cls int8,
    pcd_dist float16, pcd_flow float16}}}), mtime=0).  -> path."""
    from .metrics import generate_lidar_rays, process_one_sample
    os.makedirs(submission_prefix, exist_ok=True)
    rays = torch.from_numpy(generate_lidar_rays())
    results = {}
    for token, sem_pred, flow_pred, origins in samples:
        sem_pred = np.reshape(np.asarray(sem_pred), OCC_SHAPE)
        flow_pred = np.reshape(np.asarray(flow_pred), OCC_SHAPE + (2,))
        pcd = process_one_sample(sem_pred, rays, origins, flow_pred, device)
        results[token] = {'pcd_cls': pcd[:, 0].astype(np.int8), 'pcd_dist': pcd[:, 1].astype(np.float16),
                          'pcd_flow': pcd[:, 2:4].astype(np.float16)}
    return write_submission(results, submission_prefix, header)


def write_submission(results, submission_prefix, header=None):
    """{token: {pcd_cls, pcd_dist, pcd_flow}} -> `<prefix>/submission.gz`, the bytes format_submission writes -> path."""
    os.makedirs(submission_prefix, exist_ok=True)
    final = dict(SUBMISSION_HEADER if header is None else header)
    final['results'] = results
    path = os.path.join(submission_prefix, 'submission.gz')
    with open(path, 'wb') as f:
        f.write(gzip.compress(pickle.dumps(final), mtime=0))
    return path


def format_submission_device(samples, submission_prefix, header=None, device='cuda', batch=8):
    """format_submission with the ray cast, the class / flow look-up and the int8 / float16 casts on the device
    (metrics.SubmissionWriter, csrc/submission_rays.hip): same sample tuples (numpy arrays or device tensors), same file.
    Samples are taken `batch` at a time, their origins padded to the batch's largest T; a batch also ends where the origins'
    float type changes, because the conversion to voxel units runs in that type (as process_one_sample's does).  -> path."""
    from .metrics import ray_metrics as rm
    from .metrics.submission_device import SubmissionWriter
    dev = torch.device(device)
    writer = SubmissionWriter(rm._pc_range, rm._voxel_size, free_id=len(rm.occ_class_names) - 1, device=dev)
    pend = []

    def flush():
        if not pend:
            return
        tmax = max(o.shape[0] for _, _, _, o in pend)
        origins = torch.zeros(len(pend), tmax, 3, dtype=pend[0][3].dtype)
        for b, (_, _, _, o) in enumerate(pend):
            origins[b, :o.shape[0]] = o
        sem = torch.stack([s for _, s, _, _ in pend])
        flow = torch.stack([f for _, _, f, _ in pend])
        writer.add([t for t, _, _, _ in pend], sem, flow, origins, origin_counts=[o.shape[0] for _, _, _, o in pend])
        pend.clear()

    for token, sem_pred, flow_pred, origins in samples:
        sem = torch.as_tensor(sem_pred)
        if sem.dtype not in (torch.uint8, torch.int64):
            sem = sem.to(torch.int64)
        sem = sem.to(dev, non_blocking=True).reshape(OCC_SHAPE)
        flow = torch.as_tensor(flow_pred).to(dev, torch.float32, non_blocking=True).reshape(OCC_SHAPE + (2,))
        org = torch.as_tensor(origins).cpu()
        if org.dtype not in (torch.float32, torch.float64):
            org = org.to(torch.float64)
        org = org.reshape(-1, 3)
        if pend and (len(pend) >= int(batch) or pend[0][3].dtype != org.dtype or pend[0][1].dtype != sem.dtype):
            flush()
        pend.append((token, sem, flow, org))
    flush()
    return writer.write(submission_prefix, header)


def merge_submission_parts(part_paths, submission_prefix, header=None, order=None):
    """Host only: the parts that the ranks of a multi-rank run saved (SubmissionWriter.save_part) -> one submission.gz.
    order: the token list of the file; default round-robin over the parts — sample i of the run is entry i // N of part
    i mod N, the sharding of occnet_amd/dist.py (shard_indices).  That sharding wraps its tail so that every rank gets the
    same count: the repeats it makes (the k-th entry after the last new token is token k again, with the same rows) are
    dropped.  Any other token held twice, a token of `order` that no part holds, or a part's token that `order` leaves out
    raises ValueError.  -> path."""
    parts = []
    for p in part_paths:
        with open(p, 'rb') as f:
            parts.append(pickle.loads(gzip.decompress(f.read())))
    lists = [list(part) for part in parts]
    n = len(lists)
    round_robin = all(len(a) - len(b) in (0, 1) for a, b in zip(lists, lists[1:]))      # the sizes such a sharding gives
    if round_robin:
        seq = [(r, lists[r][k]) for k in range(len(lists[0]) if lists else 0) for r in range(n) if k < len(lists[r])]
    else:
        seq = [(r, tok) for r in range(n) for tok in lists[r]]
    merged, found, wrapped = {}, [], 0
    for r, tok in seq:
        rows = parts[r][tok]
        if tok not in merged and not wrapped:
            merged[tok] = rows
            found.append(tok)
        elif (round_robin and wrapped < len(found) and tok == found[wrapped] and sorted(rows) == sorted(merged[tok])
              and all(np.array_equal(rows[k], merged[tok][k], equal_nan=True) and rows[k].dtype == merged[tok][k].dtype
                      for k in rows)):
            wrapped += 1
        else:
            raise ValueError(f"merge_submission_parts: token {tok!r} of {part_paths[r]} appears twice, or follows the "
                             "wrapped tail of the sharding")
    if order is None:
        if not round_robin:
            raise ValueError("merge_submission_parts: the parts' sizes are not those of a round-robin sharding "
                             f"({[len(l) for l in lists]}): pass order=")
        order = found
    order = list(order)
    if len(set(order)) != len(order):
        raise ValueError("merge_submission_parts: order names a token twice")
    missing = [t for t in order if t not in merged]
    extra = [t for t in merged if t not in set(order)]
    if missing or extra:
        raise ValueError(f"merge_submission_parts: order and parts disagree (missing {missing}, not in order {extra})")
    return write_submission({t: merged[t] for t in order}, submission_prefix, header)


def read_submission(path):
    with open(path, 'rb') as f:
        return pickle.loads(gzip.decompress(f.read()))


def score_submission(pred, gt, device='cuda', free_id=16, batch=8):
    """The score the challenge server gives a submission: the counterpart of the reference's tools/ray_iou/metric.py:compute
    on the device (metrics.SubmissionScore, csrc/submission_score.hip).  pred, gt: each the path of a submission.gz-style file
    (the ground truth's is the reference's nuscenes_infos_val_occ_pcd.gz), the dict such a file holds, or its `results` dict
    {token: {pcd_cls, pcd_dist, pcd_flow}}.  Walks the ground truth's tokens; a token without a prediction raises
    RuntimeError.  -> metric.py's `output` dict (RayIoU@1, RayIoU@2, RayIoU@4, RayIoU, mAVE, final_Occ_Score) plus iou_list
    and ave_list."""
    from .metrics.submission_score import SubmissionScore

    def results(x):
        if isinstance(x, (str, os.PathLike)):
            x = read_submission(x)
        return x['results'] if 'results' in x and 'pcd_cls' not in x['results'] else x

    score = SubmissionScore(free_id=free_id, device=device)
    score.update_results(results(pred), results(gt), batch=batch)
    return score.compute()
