"""not-gpu: argument checks of occ_conv1x1_nhwc_bf16_variant run before any launch (no GPU needed): the codes of the
default entry point, and OCC_E_UNSUPPORTED with a "no variant" message for a variant the arguments have no kernel for."""
import ctypes

from occnet_amd import _lib


def test_variant_entry_point_checks_arguments_without_gpu():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p, null = ctypes.cast(buf, ctypes.c_void_p), None
    f = lib.occ_conv1x1_nhwc_bf16_variant
    for v in (0, 1, 2):
        assert f(null, p, p, null, p, 1, 4, 4, 128, 128, 1, 0, 0, v, null) == -1       # null x
        assert f(p, null, p, null, p, 1, 4, 4, 128, 128, 1, 0, 0, v, null) == -1       # null weight
        assert f(p, p, p, null, null, 1, 4, 4, 128, 128, 1, 0, 0, v, null) == -1       # null out
        assert f(p, p, p, null, p, 1, 4, 4, 128, 128, 0, 0, 0, v, null) == -1          # stride 0
        assert f(p, p, p, null, p, 1, 4, 4, 48, 128, 1, 0, 0, v, null) == -3           # Cin % 32
        assert b'no kernel' in lib.occ_last_error()
        assert f(p, p, p, null, p, 1, 4, 4, 128, 40, 1, 0, 0, v, null) == -3           # Cout % 32
        assert f(p, p, p, p, p, 1, 5, 4, 128, 128, 1, 0, 1, v, null) == -1             # odd size, upsampled residual
        assert f(p, p, p, null, p, 1, 4, 4, 128, 128, 1, 0, 1, v, null) == -1          # upsampled residual missing


def test_variant_entry_point_refuses_missing_variants_without_gpu():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p, null = ctypes.cast(buf, ctypes.c_void_p), None
    f = lib.occ_conv1x1_nhwc_bf16_variant

    def refused(*a):
        assert f(*a) == -3
        assert b'no variant' in lib.occ_last_error()

    for v in (3, 4, 12, 21, 23, 25, 102, 104, 202, -1, -2, -22):                            # no such kernel
        refused(p, p, p, null, p, 1, 4, 4, 128, 128, 1, 0, 0, v, null)
    for v in (2, 22, 24):
        refused(p, p, p, null, p, 1, 4, 4, 1024, 256, 1, 0, 0, v, null)                # K = 1024: the tile does not fit
        refused(p, p, p, null, p, 1, 4, 4, 2048, 256, 1, 0, 0, v, null)
        refused(p, p, p, null, p, 1, 4, 4, 64, 256, 1, 0, 0, v, null)                  # K = 64
        refused(p, p, p, null, p, 1, 4, 4, 256, 96, 1, 0, 0, v, null)                  # Cout % 128
    refused(p, p, p, null, p, 1, 4, 4, 256, 256, 1, 0, 0, 22, null)                    # 64-row tile: K = 512 only
    refused(p, p, p, null, p, 1, 4, 4, 128, 512, 1, 0, 0, 22, null)
    refused(p, p, p, null, p, 1, 4, 4, 512, 1024, 1, 0, 0, 324, null)                  # 3 column blocks, 4 passes
