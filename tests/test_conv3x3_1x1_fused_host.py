"""not-gpu: the argument checks of occ_conv3x3_conv1x1_nhwc_bf16 run before any launch, and occ_conv3x3_conv1x1_pick is a
pure function of the shape that only returns tile ids the entry point accepts (no GPU needed)."""
import ctypes

from occnet_amd import _lib

# every tile id the fused kernel is built for, by (Cmid, stride)
TILES = {(128, 1): (12,), (128, 2): (12, 13), (256, 1): (22, 23, 24), (256, 2): (22,)}


def test_entry_point_refuses_bad_arguments_without_gpu():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p, null = ctypes.cast(buf, ctypes.c_void_p), None
    f = lib.occ_conv3x3_conv1x1_nhwc_bf16
    good = [p, p, p, p, p, p, p]
    for i in range(7):                                                           # each pointer in turn
        a = list(good)
        a[i] = null
        assert f(*a, 1, 4, 4, 128, 512, 1, 12, null) == -1
    assert f(*good, 0, 4, 4, 128, 512, 1, 12, null) == -1                        # batch 0
    assert f(*good, 1, 4, 4, 128, 512, 3, 12, null) == -3                        # stride 3
    assert f(*good, 1, 4, 4, 64, 256, 1, 12, null) == -3                         # Cmid 64
    assert f(*good, 1, 4, 4, 512, 2048, 1, 22, null) == -3                       # Cmid 512
    assert f(*good, 1, 4, 4, 128, 256, 1, 12, null) == -3                        # Cout != 4 Cmid
    assert f(*good, 1, 4, 4, 256, 512, 1, 22, null) == -3
    for (cmid, s), have in TILES.items():                                        # a tile id the stride has no kernel for
        for v in (1, 2, 11, 12, 13, 14, 16, 18, 21, 22, 23, 24, 26, 34, -1):
            if v not in have:
                assert f(*good, 1, 4, 4, cmid, 4 * cmid, s, v, null) == -3, (cmid, s, v)
                assert b'no variant' in lib.occ_last_error()
    # variant 0 on a map the rule does not fuse: refused, not launched
    assert f(*good, 2, 32, 48, 128, 512, 1, 0, null) == -3


def test_pick_is_pure_and_returns_only_tiles_the_entry_point_has():
    lib = _lib.lib()
    pick = lib.occ_conv3x3_conv1x1_pick
    # the maps of test_plan_with_resident_kernels_matches_plan_on_tiled_kernels (2 x 3 x 256 x 384 input) stay on the pair
    assert pick(2, 32, 48, 128, 512, 1) == 0
    assert pick(2, 16, 24, 256, 1024, 1) == 0
    assert pick(2, 64, 96, 128, 512, 2) == 0
    assert pick(2, 32, 48, 256, 1024, 2) == 0
    # no kernel: other channel counts and strides
    for args in [(6, 116, 200, 64, 256, 1), (6, 29, 50, 512, 2048, 1), (6, 116, 200, 128, 256, 1),
                 (6, 116, 200, 128, 512, 3), (0, 116, 200, 128, 512, 1), (6, 0, 200, 128, 512, 1)]:
        assert pick(*args) == 0, args
    seen = set()
    for cmid in (128, 256):
        for s in (1, 2):
            for n in (1, 2, 6, 8, 24):
                for h, w in [(5, 7), (29, 50), (58, 100), (116, 200), (232, 400), (464, 800), (117, 199)]:
                    a = pick(n, h, w, cmid, 4 * cmid, s)
                    assert a == pick(n, h, w, cmid, 4 * cmid, s)                 # same arguments, same answer
                    assert a == 0 or a in TILES[(cmid, s)], (n, h, w, cmid, s, a)
                    if a:
                        rt = a % 10                                              # at least one tile per CU
                        ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
                        assert n * ((wo + 15) // 16) * ((ho + 2 * rt - 1) // (2 * rt)) >= 256
                    seen.add(a)
    assert 0 in seen and len(seen) > 1
