"""not-gpu: the host side of the q16 value rows of the fused TSA gather (OCC_TSA_VALUES=q16) — the range-scale rules
ext.absmax_words_f32 / ext.layernorm_bound_words / ext.tsa_value_scale rest on, restated in numpy (tests/tsa_q16_ref.py) and
held against the ATen implementations on CPU tensors, and the argument checks of the two new entry points, which come before
any launch."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from occnet_amd import _lib, ext
from occnet_amd._lib import i32, i64
from tests.tsa_q16_ref import bf16_words_up, ln_bound, pattern_value, range_scale


def _edge_values():
    """float32 edge values: bf16-exact denormals, powers of two, one ulp below a power of two, the fp16 and bf16 limits."""
    two = lambda k: np.ldexp(np.float32(1.0), k)
    below = lambda k: np.nextafter(two(k), np.float32(0.0), dtype=np.float32)
    vals = [two(-133), np.float32(3.0) * two(-133), two(-127),                  # denormals that bf16 holds exactly
            two(-126), two(-20), two(0), two(15), two(100), below(-20), below(0), below(15), below(100),
            np.float32(65504.0), np.float32(1e30)]
    return np.asarray(vals, np.float32)


def test_absmax_words_round_up_to_bf16():
    """(bits + 0xffff) >> 16 rounds the bound UP to a bf16 pattern: it decodes to at least the input and to less than
    input * (1 + 2^-7) (a bf16 ulp is 2^-7 of its binade's lower end)."""
    rng = np.random.default_rng(3)
    x = np.concatenate([np.exp(rng.uniform(np.log(1e-30), np.log(1e30), 10000)).astype(np.float32), _edge_values()])
    assert x.min() > 0
    pat = bf16_words_up(x)
    dec = pattern_value(pat).astype(np.float64)
    assert (dec >= x.astype(np.float64)).all()
    assert (dec < x.astype(np.float64) * (1.0 + 2.0 ** -7)).all()
    # the ATen implementation is this rule, element for element (8 replicated words, the maximum of a tensor)
    for v in list(_edge_values()) + list(x[:50]):
        w = ext.absmax_words_f32(torch.tensor(float(v), dtype=torch.float32))
        assert w.dtype == torch.int32 and tuple(w.shape) == (8,)
        assert w.tolist() == [int(bf16_words_up(np.float32(v)))] * 8, float(v)
    t = torch.from_numpy(x[:1000].copy()) * torch.where(torch.arange(1000) % 2 == 0, 1.0, -1.0)
    assert ext.absmax_words_f32(t).tolist() == [int(bf16_words_up(x[:1000].max()))] * 8
    # an fp32 denormal that bf16 cannot hold still rounds UP, by less than one bf16 denormal step (2^-133): the relative
    # bound above cannot hold below the normal range
    d = np.float32(1e-40)
    dd = float(pattern_value(bf16_words_up(d)))
    assert float(d) <= dd < float(d) + 2.0 ** -133
    # Inf / NaN: a non-finite pattern — occ_value_range_scale_from_amax then returns the neutral s = 1
    for bad in (float('inf'), float('nan'), -float('inf')):
        p = int(ext.absmax_words_f32(torch.tensor([1.0, bad]))[0])
        assert 0x7f80 <= p <= 0x7fff and not np.isfinite(pattern_value(np.int64(p)))
    assert int(ext.absmax_words_f32(torch.zeros(5))[0]) == 0


def _ln_rows(n, count, rng):
    """count rows of n channels: random at several amplitudes, with offsets of the size of their spread, and the extremal rows —
    one spike among zeros (|x_c - mean| = sqrt(n - 1) * std exactly), of either sign and at every few positions.  (Rows whose
    spread is many orders below their mean are left out on purpose: there a float32 LayerNorm that takes its variance from
    running moments — ATen's on the CPU — loses the variance to cancellation, 6 % at N = 2 for rows of 5 +- 1e-3, which says
    nothing about the bound.  The kernels that attach it square the very deviations they normalise: |y_c| <= sqrt(N) |gamma_c|
    + |beta_c| then holds whatever the mean's rounding, inside the bound's 2^-8 slack from N = 129 on; they run at N = 256.)"""
    rows = [rng.standard_normal((count // 4, n)) * a + o for a, o in ((1.0, 0.0), (1e-3, 1e-3), (1e3, -5e2))]
    spikes = np.zeros((count - 3 * (count // 4), n))
    pos = rng.integers(0, n, spikes.shape[0])
    spikes[np.arange(spikes.shape[0]), pos] = np.where(rng.random(spikes.shape[0]) < 0.5, 1e6, -1e6)
    spikes[::3] *= 1e-6                                     # spikes of 1.0 as well
    return np.concatenate(rows + [spikes]).astype(np.float32)


@pytest.mark.parametrize("n", [2, 8, 256])
def test_layernorm_bound_is_never_exceeded(n):
    rng = np.random.default_rng(100 + n)
    x = torch.from_numpy(_ln_rows(n, 2000, rng))
    assert x.shape == (2000, n)
    worst = 0.0
    for trial, (gs, bs) in enumerate(((1.0, 0.0), (3.0, 0.5), (0.05, 10.0))):
        ln = torch.nn.LayerNorm(n)
        with torch.no_grad():
            ln.weight.copy_(torch.from_numpy((rng.standard_normal(n) * gs).astype(np.float32)))
            ln.bias.copy_(torch.from_numpy((rng.standard_normal(n) * bs).astype(np.float32)))
            if trial == 0:
                ln.weight.fill_(1.0)                        # the spike rows then reach sqrt(n - 1) itself
        y = F.layer_norm(x, (n,), ln.weight, ln.bias, 0.0 if trial == 0 else ln.eps)
        assert y.dtype == torch.float32
        words = ext.layernorm_bound_words(ln)
        bound = float(pattern_value(np.int64(int(words[0]))))
        ref_bound = ln_bound(ln.weight.detach().numpy(), ln.bias.detach().numpy())
        assert words.tolist() == [int(bf16_words_up(np.float32(ref_bound)))] * 8
        top = float(y.detach().abs().max())
        worst = max(worst, top / bound)
        assert top <= bound, (n, trial, top, bound)
        if trial == 0:                                      # the bound is sharp: the spikes come within the slack of it
            assert top >= (n - 1) ** 0.5 * 0.999
    print(f"N={n}: largest max|LayerNorm(x)| / bound = {worst:.4f}")
    # cached on the parameters' identity, dropped by an in-place update
    again = ext.layernorm_bound_words(ln)
    assert again is ext.layernorm_bound_words(ln)
    with torch.no_grad():
        ln.weight.mul_(64.0)
    assert int(ext.layernorm_bound_words(ln)[0]) > int(again[0])


def test_scale_rule_keeps_the_rows_inside_q16():
    """(bound * row_l1 * (1 + 2^-8) + bias_max) * s <= 2^15 with s a power of two, for the restatement the GPU tests hold
    occ_value_range_scale_from_amax to; s is the largest such power of two up to the binade (> 2^14)."""
    rng = np.random.default_rng(5)
    for _ in range(2000):
        amax = np.float32(np.exp(rng.uniform(np.log(1e-20), np.log(1e20))))
        l1 = np.float32(np.exp(rng.uniform(np.log(1e-3), np.log(1e3))))
        bm = np.float32(0.0 if rng.random() < 0.3 else np.exp(rng.uniform(np.log(1e-6), np.log(1e6))))
        words = bf16_words_up(amax)
        s, bound = range_scale(words, l1, bm)
        m, e = np.frexp(np.float64(s))
        assert m == 0.5                                                     # a power of two
        full = (float(pattern_value(words)) * float(l1) * (1.0 + 2.0 ** -8) + float(bm))
        assert full * float(s) <= 2.0 ** 15 * (1.0 + 2.0 ** -22)            # (the device evaluates the bound in fp32)
        assert full * float(s) > 2.0 ** 14 * (1.0 - 2.0 ** -22)
        assert float(amax) * float(l1) + float(bm) <= float(bound) * (1.0 + 2.0 ** -22)
    assert range_scale(np.int64(0x7f80), np.float32(1.0), np.float32(0.0))[0] == 1.0        # Inf
    assert range_scale(np.int64(0x7fc0), np.float32(1.0), np.float32(0.0))[0] == 1.0        # NaN
    assert range_scale(np.int64(0), np.float32(1.0), np.float32(0.0))[0] == 1.0             # all-zero rows


def test_new_symbols_are_declared_and_exported():
    """the symbol <-> header check of tests/test_capi_host.py covers them; here: they are among the declared ones at all"""
    assert ext.TSA_VALUES in ("f32", "q16")
    names = _lib.declared_symbols()
    lib = _lib.lib()
    for n in ("occ_tsa_fused_forward_q16v", "occ_linear_bf16x3_q16rows"):
        assert n in names and hasattr(lib, n)


def _tsa(a, *, value=None, out=None, vstride=2 * 256, rows=2, so=256, sl=128, dims=(1, 2, 1, 2, 8, 32, 8)):
    """P = 8 by default: arguments that pass every check end at the shape test (-3), so nothing is ever launched on the host
    pointers — on a machine with a GPU either."""
    null = ctypes.c_void_p(0)
    pick = lambda x: a if x is None else x
    return _lib.lib().occ_tsa_fused_forward_q16v(pick(value), i64(vstride), i32(rows), a, i64(so), a, i64(sl), a, null,
                                                 pick(out), *dims, null, null)


def test_tsa_q16_argument_checks_before_any_launch():
    """Every call fails on a check in front of the launch (the pointers are host memory)."""
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 12)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a = ctypes.c_void_p(base)
    last = lambda: lib.occ_last_error()
    assert _tsa(a) == -3 and b'P=8' in last()                      # the baseline passes every argument check
    assert _tsa(a, vstride=0) == -3                                # aliased queue entries
    assert _tsa(a, value=null) == -1 and b'null' in last()
    assert _tsa(a, out=null) == -1 and b'null' in last()
    assert _tsa(a, dims=(0, 2, 1, 2, 8, 32, 8)) == -1 and b'dimension' in last()
    # padded row count: even, and bev_h*bev_w rounded up
    assert _tsa(a, rows=3, vstride=4 * 256, dims=(1, 2, 1, 3, 8, 32, 8)) == -1 and b'rounded up to even' in last()
    assert _tsa(a, rows=4, vstride=4 * 256) == -1 and b'rounded up to even' in last()
    assert _tsa(a, rows=4, vstride=4 * 256, dims=(1, 2, 1, 3, 8, 32, 8)) == -3     # 3 pixels in 4 rows
    # stride: 0 or at least one padded map, a multiple of 8 elements
    assert _tsa(a, vstride=2 * 256 - 8) == -1 and b'value stride' in last()
    assert _tsa(a, vstride=-8) == -1 and b'value stride' in last()
    assert _tsa(a, vstride=2 * 256 + 4) == -1 and b'16-byte aligned' in last()
    assert _tsa(a, value=ctypes.c_void_p(base + 8)) == -1 and b'value must be 16-byte aligned' in last()
    assert _tsa(a, value=ctypes.c_void_p(base + 2)) == -1 and b'value must be 16-byte aligned' in last()
    # both maps of a batch entry under one descriptor, below the dead-corner marker
    assert _tsa(a, rows=2048 * 1024, vstride=2048 * 1024 * 256, dims=(1, 2, 2048, 1024, 8, 32, 8)) == -1 and b'too large' in last()
    assert _tsa(a, rows=2048 * 1024, vstride=0, dims=(1, 2, 2048, 1024, 8, 32, 8)) == -3       # one aliased 1 GB map fits
    assert _tsa(a, so=255) == -1 and b'row strides' in last()
    assert _tsa(a, sl=127) == -1 and b'row strides' in last()
    assert _tsa(a, so=258) == -3 and _tsa(a, so=257) == -1 and b'even' in last()
    assert _tsa(a, out=ctypes.c_void_p(base + 8)) == -1 and b'out' in last()
    for dims, word in (((1, 2, 1, 2, 4, 32, 4), b'M=4'), ((1, 2, 1, 2, 8, 64, 4), b'D=64')):
        assert _tsa(a, vstride=2 * dims[4] * dims[5], dims=dims) == -3 and word in last()


def test_linear_q16rows_argument_checks_before_any_launch():
    lib = _lib.lib()
    null = ctypes.c_void_p(0)
    buf = (ctypes.c_float * 12)()
    a = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    last = lambda: lib.occ_last_error()
    f = lambda x=a, lda=256, K=256, out=a, M=4, N=256, groups=2: lib.occ_linear_bf16x3_q16rows(
        x, i64(lda), i32(K), a, null, null, out, i32(M), i32(N), i32(groups), null)
    assert f(x=null) == -1 and b'null' in last()
    assert f(out=null) == -1 and b'null' in last()
    assert f(M=0) == -1 and b'dimension' in last()
    assert f(groups=0) == -1 and b'dimension' in last()
    assert f(M=5) == -1 and b'split' in last()
    assert f(lda=128) == -1 and b'leading dimension' in last()
    assert f(out=ctypes.c_void_p(a.value + 8)) == -1 and b'out must be 16-byte aligned' in last()
    assert f(N=128) == -3 and b'N=128' in last()
    assert f(N=512) == -3
    assert f(K=24, lda=24) == -3 and b'K=24' in last()
    assert f(lda=258) == -3
    # the Python wrapper refuses epilogues the kernel does not have before it looks at anything else
    for kw in (dict(residual=torch.zeros(1)), dict(act='relu'), dict(ln=(None, None, 0.0))):
        with pytest.raises(_lib.OccAmdUnsupported):
            ext.linear_q16rows(None, None, None, None, 1, **kw)
    with pytest.raises(_lib.OccAmdError, match="device"):
        ext.linear_q16rows(torch.zeros(4, 256), torch.zeros(256, 256), None, None, 2)
    with pytest.raises(_lib.OccAmdError, match="value_scale"):
        ext.tsa_fused_forward(torch.zeros(2, 4, 8, 32), torch.zeros(1, 4, 128), torch.zeros(1, 4, 64),
                              torch.zeros(2, 4, 1, 2), 2, 2, 8, 4, value_scale=torch.ones(1))
