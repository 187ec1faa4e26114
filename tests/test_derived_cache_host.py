"""occnet_amd/derived.py on CPU tensors (data_ptr and _version behave as on the device): the one cache protocol every
derived-weight cache uses — identity keys, pinned sources, bounded size, rebuild on a miss, the `_occ_no_cache` bypass and
the registry occnet_amd.invalidate_caches() walks."""
import gc
import weakref

import pytest
import torch

import occnet_amd
from occnet_amd import derived
from occnet_amd._lib import OccAmdUnsupported
from occnet_amd.derived import DerivedCache


def _doubling(cache, t, calls):
    def build():
        calls.append(1)
        return t.detach() * 2
    return cache.get((t,), build)


def test_second_lookup_returns_the_stored_object():
    cache, calls, t = DerivedCache("t", 4), [], torch.ones(3)
    v = _doubling(cache, t, calls)
    assert _doubling(cache, t, calls) is v and len(calls) == 1 and len(cache) == 1


def test_inplace_update_misses_and_rebuilds():
    cache, calls, t = DerivedCache("t", 4), [], torch.ones(3)
    v = _doubling(cache, t, calls)
    with torch.no_grad():
        t.add_(1.0)
    v2 = _doubling(cache, t, calls)
    assert v2 is not v and len(calls) == 2 and torch.equal(v2, torch.full((3,), 4.0))


def test_data_write_stays_stale_until_invalidate_caches():
    cache, calls, t = DerivedCache("t", 4), [], torch.ones(3)
    v = _doubling(cache, t, calls)
    t.data.mul_(5.0)                                            # invisible to _version
    assert _doubling(cache, t, calls) is v and torch.equal(v, torch.full((3,), 2.0))
    occnet_amd.invalidate_caches()
    v2 = _doubling(cache, t, calls)
    assert v2 is not v and len(calls) == 2 and torch.equal(v2, torch.full((3,), 10.0))


@pytest.mark.parametrize("how", ["evicted", "cleared"])
def test_entry_pins_its_sources(how):
    cache = DerivedCache("t", 1)
    t = torch.ones(3)
    ref = weakref.ref(t)
    cache.get((t,), lambda: 0)
    del t
    gc.collect()
    assert ref() is not None                                    # the entry holds it: its address cannot be recycled
    if how == "evicted":
        cache.get((torch.zeros(2),), lambda: 1)
    else:
        cache.clear()
    gc.collect()
    assert ref() is None


def test_capacity_evicts_the_oldest_inserted():
    cap = 4
    cache = DerivedCache("t", cap)
    ts = [torch.zeros(2) for _ in range(cap + 3)]
    for i, t in enumerate(ts):
        cache.get((t,), lambda i=i: i)
    assert len(cache) == cap
    assert [k[0] for k in cache.keys()] == [derived.ident(t) for t in ts[3:]]      # the three oldest are gone
    assert [cache.get((t,), lambda: -1) for t in ts[3:]] == [3, 4, 5, 6]            # the newest hit
    assert cache.get((ts[0],), lambda: -1) == -1 and len(cache) == cap


def test_views_of_one_storage_get_separate_entries():
    cache, base = DerivedCache("t", 8), torch.zeros(16)
    a, b = base.view(2, 8), base.view(4, 4)
    c = b.t()                                                   # same shape as b, other strides
    assert a.data_ptr() == b.data_ptr() == c.data_ptr() and a._version == b._version == c._version
    va, vb, vc = (cache.get((t,), lambda n=n: n) for n, t in (("a", a), ("b", b), ("c", c)))
    assert (va, vb, vc) == ("a", "b", "c") and len(cache) == 3
    assert cache.get((b,), lambda: "again") == "b" and cache.get((c,), lambda: "again") == "c"
    assert derived.ident(b) != derived.ident(c) and derived.ident(b)[:3] == derived.ident(c)[:3]
    assert derived.ident(b)[4] is base.device or derived.ident(b)[4] == base.device     # the device object, no string
    assert not isinstance(derived.ident(b)[4], str)
    assert derived.signature([a, None]) == (derived.ident(a), None)


def test_ident_is_kept_on_the_tensor_while_address_and_version_stand():
    t = torch.ones(2, 3)
    i0 = derived.ident(t)
    assert i0 == (t.data_ptr(), 0, t.shape, t.stride(), t.device) and derived.ident(t) is i0
    assert derived.ident(t.view(3, 2)) != i0 and derived.ident(t.detach()) == i0       # per object; equal where all five are
    with torch.no_grad():
        t.add_(1.0)
    assert derived.ident(t) == (t.data_ptr(), 1, t.shape, t.stride(), t.device)
    t.data = torch.zeros(5)                                     # another storage under the same object: the address moves
    assert derived.ident(t) == (t.data_ptr(), t._version, torch.Size([5]), (1,), t.device)


def test_none_source_is_accepted_and_distinct():
    cache, w, b = DerivedCache("t", 8), torch.ones(2, 2), torch.zeros(2)
    assert cache.get((w, None), lambda: "no bias") == "no bias"
    assert cache.get((w, b), lambda: "bias") == "bias"
    assert cache.get((w, None), lambda: "again") == "no bias" and len(cache) == 2


def test_raising_build_stores_nothing():
    cache, t, calls = DerivedCache("t", 4), torch.ones(3), []

    def bad():
        calls.append(1)
        raise OccAmdUnsupported("no")
    for _ in range(2):
        with pytest.raises(OccAmdUnsupported):
            cache.get((t,), bad)
        assert len(cache) == 0
    assert len(calls) == 2
    assert cache.get((t,), lambda: 7) == 7 and len(cache) == 1


def test_marked_source_bypasses_the_cache_in_both_directions():
    cache, calls, t = DerivedCache("t", 4), [], torch.ones(3)
    other = torch.ones(3)
    _doubling(cache, other, calls)
    keys = cache.keys()
    t._occ_no_cache = True
    v1, v2 = _doubling(cache, t, calls), _doubling(cache, t, calls)
    assert v1 is not v2 and len(calls) == 3 and cache.keys() == keys
    # ... and reads nothing either: an entry made before the mark is not served
    cached = _doubling(cache, other, calls)
    other._occ_no_cache = True
    assert _doubling(cache, other, calls) is not cached and cache.keys() == keys


def test_registered_caches_are_emptied_by_invalidate_caches():
    from occnet_amd import ext
    g, b = torch.rand(8) + 0.5, torch.rand(8)
    w = ext.layernorm_bound_words((g, b, 0.0))
    assert ext.layernorm_bound_words((g, b, 0.0)) is w
    assert ext._LN_BOUND in derived._REGISTERED and len(ext._LN_BOUND) >= 1
    occnet_amd.invalidate_caches()
    assert derived._REGISTERED and all(len(c) == 0 for c in derived._REGISTERED)
    w2 = ext.layernorm_bound_words((g, b, 0.0))
    assert w2 is not w and torch.equal(w2, w)
    owned = DerivedCache("owned", 1)                            # module-owned caches do not register
    assert owned not in derived._REGISTERED


def test_snapshot_and_restore_put_the_registered_caches_back():
    """An entry made after the snapshot leaves with restore() (and with it the pin on its sources); one made before stays."""
    cache, calls = DerivedCache("snap", 4, register=True), []
    try:
        old, new = torch.ones(3), torch.ones(5)
        v = _doubling(cache, old, calls)
        snap = derived.snapshot()
        _doubling(cache, new, calls)
        ref = weakref.ref(new)
        assert len(cache) == 2
        derived.restore(snap)
        assert len(cache) == 1 and _doubling(cache, old, calls) is v and len(calls) == 2
        del new
        gc.collect()
        assert ref() is None                                    # the cache no longer pins the later source
    finally:
        derived._REGISTERED.remove(cache)

