"""Test infrastructure: numpy restatement of the range-scale rules of the q16 TSA value rows (OCC_TSA_VALUES=q16) — what
ext.absmax_words_f32, ext.layernorm_bound_words and occ_value_range_scale_from_amax (csrc/value_range.hip vr_write_scales /
vr_scale_of) compute.  A plain helper: no pytest code."""
import numpy as np


def bf16_words_up(x):
    """float32 bound(s) -> the bf16 pattern(s) rounded UP: (bits + 0xffff) >> 16 on the sign-stripped fp32 bits, a NaN pattern
    at most (never the sign bit)."""
    bits = np.asarray(x, np.float32).view(np.uint32).astype(np.int64) & 0x7fffffff
    return np.minimum((bits + 0xffff) >> 16, 0x7fff)


def pattern_value(p):
    """bf16 pattern(s) -> float32, as the scale kernel reads its words: bits << 16."""
    return (np.asarray(p, np.int64).astype(np.uint32) << np.uint32(16)).view(np.float32)


def ln_bound(gamma, beta):
    """max|gamma| sqrt(N - 1) (1 + 2^-8) + max|beta| in float32: the bound of a LayerNorm output over N channels
    (sum_c (x_c - mean) = 0 gives (x_c - mean)^2 <= (N - 1) var)."""
    n = np.asarray(gamma).size
    f = np.float32(float(max(n - 1, 0)) ** 0.5 * 1.00390625)
    return np.float32(np.float32(np.abs(np.asarray(gamma, np.float32)).max() * f) + np.abs(np.asarray(beta, np.float32)).max())


def range_scale(words, row_l1, bias_max):
    """-> (s, bound): bound = max|x| row_l1 (1 + 2^-8) + bias_max with max|x| the largest of the words' patterns;
    bound = m 2^e, m in [0.5, 1)  =>  s = 2^(15 - e) (exponent clamped to +-100); s = 1 for a zero, Inf or NaN bound."""
    amax = pattern_value(np.max(np.asarray(words, np.int64)) & 0xffff).astype(np.float64)
    bound = np.float32(abs(float(row_l1)) * amax * 1.00390625 + abs(float(bias_max)))
    if not (bound > 0) or not np.isfinite(bound):
        return np.float32(1.0), bound
    e = int(np.frexp(bound)[1])
    return np.ldexp(np.float32(1.0), int(np.clip(15 - e, -100, 100))), bound
