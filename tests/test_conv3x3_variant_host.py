"""not-gpu: argument checks of occ_conv3x3_nhwc_bf16_variant run before any launch (no GPU needed): a variant the
stride has no kernel for, and the shape limits of the default entry points, return OCC_E_UNSUPPORTED."""
import ctypes

from occnet_amd import _lib


def test_variant_entry_point_refuses_missing_variants_without_gpu():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p, null = ctypes.cast(buf, ctypes.c_void_p), None
    f = lib.occ_conv3x3_nhwc_bf16_variant
    assert f(null, p, p, p, 1, 4, 4, 32, 128, 1, 1, null, 14, null) == -1         # null x
    assert f(p, p, p, p, 1, 4, 4, 32, 128, 3, 1, null, 14, null) == -3            # stride 3
    assert f(p, p, p, p, 1, 4, 4, 32, 64, 1, 1, null, 14, null) == -3             # Cout % 128
    assert f(p, p, p, p, 1, 4, 4, 48, 128, 1, 1, null, 14, null) == -3            # Cin % 32
    for v in (1, 4, 11, 15, 17, 21, 26, 34, -1):                                 # no such tile at stride 1
        assert f(p, p, p, p, 1, 4, 4, 32, 256, 1, 1, null, v, null) == -3
        assert b'no variant' in lib.occ_last_error()
    for v in (14, 16, 18, 23, 24):                                               # stride 2 has 12, 13, 22 only
        assert f(p, p, p, p, 1, 4, 4, 32, 256, 2, 1, null, v, null) == -3
    for v in (22, 23, 24):                                                       # 256-channel blocks, Cout 384
        assert f(p, p, p, p, 1, 4, 4, 32, 384, 1, 1, null, v, null) == -3
