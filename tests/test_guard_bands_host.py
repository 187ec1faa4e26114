"""tests/guard_bands.py on the CPU: the helper rejects what it must (mutant "kernels" written as torch ops over CPU arenas), and
its COVERED / EXEMPT tables name every function of the C ABI exactly once."""
import importlib
import os
import re

import pytest
import torch

from tests import guard_bands as gb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("occnet_amd.h", "occnet_amd_dvr.h", "occnet_amd_visibility.h", "occnet_amd_input.h")


def _rejected(fn, *a):
    with pytest.raises(AssertionError) as e:
        fn(*a)
    return str(e.value)


def _run(fn, inputs):
    return gb.run_guarded(fn, inputs, device_type="cpu")


def _run_framed(fn, inputs):
    """The framed half alone: a mutant cannot run plainly, where its stray address has no memory behind it."""
    return gb.run_framed(fn, inputs, device_type="cpu")


def _outside(t, offset, n=1):
    """n elements of t's arena starting `offset` elements from t's first one: the view an out-of-bounds kernel address is."""
    return t.as_strided((n,), (1,), t.storage_offset() + offset)


# ---- the "kernels" -----------------------------------------------------------------------------------------------------------

def _scale_add(x, y):
    out = torch.empty_like(x)
    out.copy_(2 * x + y)
    return out


def _writes_before(x, y):
    out = _scale_add(x, y)
    _outside(out, -1).fill_(1.2345)
    return out


def _writes_after(x, y):
    out = _scale_add(x, y)
    _outside(out, out.numel()).fill_(1.2345)
    return out


def _reads_past_the_end_times_zero(x, y):
    """The clamp that is off by one: the last lane loads x[numel] and masks it with 0."""
    out = _scale_add(x, y)
    out.view(-1)[-1] += 0 * _outside(x, x.numel())[0]
    return out


def _inputs():
    g = torch.Generator().manual_seed(7)
    return [torch.randn(3, 37, generator=g), torch.randn(3, 37, generator=g)]


def test_a_correct_op_passes():
    r = _run(_scale_add, _inputs())
    gb.assert_bit_equal(r.plain, r.framed)
    gb.assert_no_new_nonfinite(r.plain, r.framed)
    assert r.n_arenas == 3                                  # two inputs, one output
    assert r.framed.data_ptr() % gb.ALIGN == 0


def test_a_store_in_front_of_the_output_is_rejected():
    msg = _rejected(_run_framed, _writes_before, _inputs())
    assert "empty_like (3, 37)" in msg and "band before" in msg and "element -1 " in msg, msg
    assert "band after" not in msg


def test_a_store_behind_the_output_is_rejected():
    msg = _rejected(_run_framed, _writes_after, _inputs())
    assert "empty_like (3, 37)" in msg and "band after" in msg and "byte +0 = element +0 " in msg, msg
    assert "band before" not in msg


def test_a_store_further_out_reports_its_offset():
    def far(x, y):
        out = _scale_add(x, y)
        _outside(out, out.numel() + 5, 2).fill_(1.2345)
        _outside(x, -9).fill_(1.2345)
        return out
    msg = _rejected(_run_framed, far, _inputs())
    assert "element +5 " in msg and "byte +20 " in msg, msg
    assert "in[0] (3, 37)" in msg and "33 byte(s) = element -9 " in msg, msg


def test_a_masked_read_past_the_end_poisons_the_result():
    plain = _scale_add(*_inputs())
    out, record, n = _run_framed(_reads_past_the_end_times_zero, _inputs())    # no band moves: only the value shows the read
    assert n == 3 and bool(torch.isfinite(plain).all()) and bool(torch.isnan(out.view(-1)[-1]))
    msg = _rejected(gb.assert_bit_equal, plain, out)
    assert "1 of 111 elements" in msg and "flat index 110" in msg, msg
    _rejected(gb.assert_no_new_nonfinite, plain, out)


def test_an_index_band_is_out_of_range():
    idx = torch.tensor([0, 2, 1, 2])
    table = torch.arange(12.0).view(3, 4)

    def gather_one_too_many(tab, index):                    # reads index[numel]
        return tab[_outside(index, 0, index.numel() + 1)]
    with pytest.raises(IndexError):
        _run_framed(gather_one_too_many, [table, gb.Poisoned(idx, 1 << 40)])


def test_zeros_keep_a_zero_interior_inside_sentinel_bands():
    gb.reset()
    with gb.guarded_allocations("cpu"):
        z = torch.zeros(5, 3, dtype=torch.int32)
        zl = torch.zeros_like(torch.ones(2, 3, 4, 5).contiguous(memory_format=torch.channels_last))
        e = torch.empty((2, 3, 4, 5), dtype=torch.bfloat16, memory_format=torch.channels_last)
        n = z.new_zeros((7,))
        ne = z.new_empty((7,), dtype=torch.float32)
    assert gb.check() == 5
    assert z.dtype == torch.int32 and int(z.abs().sum()) == 0 and int(n.abs().sum()) == 0 and float(zl.abs().sum()) == 0
    assert zl.is_contiguous(memory_format=torch.channels_last) and e.is_contiguous(memory_format=torch.channels_last)
    assert bool(torch.isnan(ne).all()) and bool(torch.isnan(e.float()).all())       # an `empty` interior is poison
    assert int(_outside(z, -1)[0]) == int.from_bytes(bytes([gb.POISON_BYTE] * 4), "little", signed=True)
    assert int(_outside(z, 15)[0]) == int(_outside(z, -1)[0])
    assert torch.empty is gb._REAL["empty"] and torch.zeros_like is gb._REAL["zeros_like"]
    assert "new_empty" not in vars(torch.Tensor) and torch.Tensor.new_zeros is gb._REAL["new_zeros"]
    # a counter that lands in the wrong word
    _outside(n, 7).add_(1)
    assert "new_zeros (7,)" in _rejected(gb.check)


def test_release_leaves_no_poison_behind():
    gb.release()
    with gb.guarded_allocations("cpu"):
        e = torch.empty(9)
    f = gb.framed(torch.ones(4))
    assert bool(torch.isnan(e).all()) and bool(torch.isnan(_outside(f, -1)[0])) and len(gb.arenas()) == 2
    gb.release()
    assert gb.arenas() == [] and gb._LIVE == []
    for t in (e, f):                                        # interior and both bands
        assert float(t.abs().sum()) == 0 and float(_outside(t, -3, 3).abs().sum()) == 0
        assert float(_outside(t, t.numel(), 3).abs().sum()) == 0


def test_allocations_on_other_devices_are_left_alone():
    gb.reset()
    with gb.guarded_allocations("cuda"):
        t = torch.empty(4)
    assert gb.arenas() == [] and t.shape == (4,)


CL = torch.channels_last


@pytest.mark.parametrize("make", [
    lambda g: torch.randn(5, 7, generator=g),
    lambda g: torch.randn(2, 8, 3, 5, generator=g).contiguous(memory_format=CL),
    lambda g: torch.randn(2, 8, 3, 5, generator=g).to(torch.bfloat16).contiguous(memory_format=CL),
    lambda g: torch.randn(3, 9, generator=g).to(torch.float16),
    lambda g: torch.randint(0, 256, (2, 3, 11, 13), generator=g, dtype=torch.uint8),
    lambda g: torch.randint(-5, 5, (17,), generator=g, dtype=torch.int64),
    lambda g: torch.randn(6, 40, generator=g)[:, 8:24],                 # a column slice: row stride > width
    lambda g: torch.randn(1, generator=g),
], ids=["f32", "f32_channels_last", "bf16_channels_last", "f16", "u8", "i64", "strided_rows", "one_element"])
def test_framed_keeps_the_tensor_and_frames_it(make):
    t = make(torch.Generator().manual_seed(3))
    gb.reset()
    f = gb.framed(t)
    (a,) = gb.arenas()
    assert f.shape == t.shape and f.dtype == t.dtype and f.stride() == t.stride() and torch.equal(f, t)
    for fmt in (torch.contiguous_format, CL) if t.dim() == 4 else (torch.contiguous_format,):
        assert f.is_contiguous(memory_format=fmt) == t.is_contiguous(memory_format=fmt)
    assert f.data_ptr() % 256 == 0
    nbytes = (1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))) * t.element_size()
    assert a.band >= 64 * 1024 and a.band >= nbytes and a.span_bytes == nbytes
    for off in (-1, nbytes // t.element_size()):
        edge = _outside(f, off)
        if t.dtype.is_floating_point:
            assert bool(torch.isnan(edge[0]))
        else:
            assert edge.view(torch.uint8).tolist() == [gb.POISON_BYTE] * t.element_size()
    assert gb.check() == 1
    f.mul_(2)                                               # the interior is the caller's to write
    assert gb.check() == 1


def test_framed_tensors_larger_than_the_least_band_get_a_band_of_their_size():
    gb.reset()
    gb.framed(torch.zeros(100_000))
    assert gb.arenas()[0].band >= 400_000


def test_framed_index_poison_and_requires_grad():
    gb.reset()
    i = gb.framed(torch.tensor([1, 2, 3]), poison=1 << 40)
    assert int(_outside(i, -1)[0]) == 1 << 40 and int(_outside(i, 3)[0]) == 1 << 40
    x = gb.framed(torch.ones(3, requires_grad=True))
    assert x.requires_grad and x.is_leaf


def test_nested_inputs_are_framed_and_results_compared_through_structures():
    def fn(d, lst, k):
        return {"s": d["a"] + lst[0], "k": k, "pair": (lst[1] * 2, None)}
    r = _run(fn, [{"a": torch.ones(4)}, [torch.ones(4), torch.arange(3)], 5])
    assert r.n_arenas == 3
    gb.assert_bit_equal(r.plain, r.framed)
    r.framed["pair"][0][1] += 1
    assert "out['pair'][0]" in _rejected(gb.assert_bit_equal, r.plain, r.framed)
    _rejected(gb.assert_bit_equal, {"a": 1}, {"a": 1})        # nothing compared is no comparison


def test_bit_equality_tells_zero_signs_apart_and_nans_alike():
    gb.assert_bit_equal(torch.tensor([float("nan"), 1.0]), torch.tensor([float("nan"), 1.0]))
    _rejected(gb.assert_bit_equal, torch.tensor([0.0]), torch.tensor([-0.0]))
    gb.assert_bit_equal(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 3.0]), defined={"out": slice(0, 1)})


def test_launch_record_requires_the_entry_point():
    rec = gb.LaunchRecord(["occ_linear_f32"])
    rec.require("occ_linear_f32")
    assert "occ_linear_bf16x3_f32" in _rejected(rec.require, "occ_linear_bf16x3_f32")


# ---- completeness -------------------------------------------------------------------------------------------------------------

def _declared():
    names = []
    for h in HEADERS:
        with open(os.path.join(ROOT, "include", h)) as f:
            src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
        names += re.findall(r"\bint (occ_\w+)\(", re.sub(r"//[^\n]*", "", src))
    return names


def test_every_c_abi_function_is_covered_or_exempt():
    names = _declared()
    assert len(names) > 80 and len(set(names)) == len(names)
    both = sorted(set(gb.COVERED) & set(gb.EXEMPT))
    assert not both, f"in both tables: {both}"
    missing = sorted(set(names) - set(gb.COVERED) - set(gb.EXEMPT))
    assert not missing, f"neither in guard_bands.COVERED nor in EXEMPT: {missing}"
    stale = sorted((set(gb.COVERED) | set(gb.EXEMPT)) - set(names))
    assert not stale, f"not declared in include/: {stale}"


def test_every_covering_test_exists():
    for name, where in sorted(gb.COVERED.items()):
        path, _, test = where.partition("::")
        assert path.startswith("tests/") and path.endswith(".py") and test.startswith("test_"), (name, where)
        mod = importlib.import_module(path[:-3].replace("/", "."))
        assert callable(getattr(mod, test, None)), f"{name}: {where} does not exist"


def test_exempt_functions_have_a_reason_and_no_stream():
    """A launcher of this ABI takes the stream as its last parameter; nothing with one may be exempt."""
    from occnet_amd import _lib
    protos = _lib.prototypes()
    for h in _lib.EXTENSION_HEADERS:
        with open(h) as f:
            protos.update(_lib.prototypes(f.read()))
    for name, reason in gb.EXEMPT.items():
        assert isinstance(reason, str) and 0 < len(reason) <= 100, name
        params = [p for _, p in protos[name][1]]
        assert "stream" not in params, f"{name} takes a stream: it launches, so it needs a test"
