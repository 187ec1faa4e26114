"""Writes tests/golden/train_input.npz: the reference's own training input pipeline run in place on small seeded frames.

    python -m tools_dev.gen_train_input_golden

oracle.refshim.install_datasets() loads the reference's transform_3d.py from where it lies; its
PhotoMetricDistortionMultiViewImage -> NormalizeMultiviewImage -> PadMultiViewImage run unmodified.  The two cv2
leaves the distortion calls through mmcv (bgr2hsv / hsv2bgr on float32) are not in the reference tree: the module's
mmcv stub gets occnet_amd.io's float32 numpy restatement of OpenCV's float path ("Training input from
uint8 frames").  The fixture holds data only: the uint8 frames, the seed, the norm settings, the reference's outputs.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'train_input.npz')
SEED = 20240611       # the first seed from 20240607 on whose six records switch every stage on and off, with deltas and hues of both signs
# the ImageNet setting rather than bevformer_base_occ.py's (std 1, to_rgb False): it also exercises 1 / std and the
# channel reversal
MEAN, STD, TO_RGB = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375], True
N, HS, WS = 6, 33, 50


def make_frames():
    """6 frames of 33 x 50: every level 0..255, grey pixels, black, white, and argmax ties in each channel pair."""
    rng = np.random.RandomState(7)
    f = rng.randint(0, 256, size=(N, HS, WS, 3)).astype(np.uint8)
    for i in range(2, N):          # 48-colour palettes: as many branches, a smaller file
        f[i] = rng.randint(0, 256, size=(48, 3)).astype(np.uint8)[rng.randint(0, 48, size=(HS, WS))]
    f[0, :, :, :] = (np.arange(HS * WS) % 256).reshape(HS, WS, 1)         # grey ramp: diff == 0, all 256 levels
    f[1, 0, :8] = [[0, 0, 0], [255, 255, 255], [200, 200, 10], [200, 10, 200], [10, 200, 200], [7, 7, 7],
                   [90, 90, 91], [91, 90, 90]]
    return f


def reference_run(t3d, frames, mean, std, to_rgb, seed):
    np.random.seed(seed)
    results = dict(img=[f.astype(np.float32) for f in frames])
    results = t3d.PhotoMetricDistortionMultiViewImage()(results)
    results = t3d.NormalizeMultiviewImage(mean=mean, std=std, to_rgb=to_rgb)(results)
    results = t3d.PadMultiViewImage(size_divisor=32)(results)
    return np.stack(results['img']).astype(np.float32)


def reference_module():
    """The reference's transform_3d module, loaded in place, with the two cv2 leaves on its mmcv stub."""
    from oracle import refshim
    from occnet_amd import io
    ns = refshim.install_datasets()
    t3d = sys.modules[ns.PadMultiViewImage.__module__]
    assert t3d.__file__ in ns.files
    t3d.mmcv.bgr2hsv = io.bgr2hsv_f32
    t3d.mmcv.hsv2bgr = io.hsv2bgr_f32
    return t3d


def main():
    t3d = reference_module()
    print('executing', t3d.__file__, 'in place:', t3d.PhotoMetricDistortionMultiViewImage.__qualname__)
    frames = make_frames()
    out = reference_run(t3d, frames, MEAN, STD, TO_RGB, SEED)
    assert out.shape == (N, 64, 64, 3) and out.dtype == np.float32
    np.savez_compressed(OUT, frames=frames, seed=np.int64(SEED), mean=np.float32(MEAN), std=np.float32(STD),
                        to_rgb=np.bool_(TO_RGB), out=out)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes; max|out|', float(np.abs(out).max()))


if __name__ == '__main__':
    main()
