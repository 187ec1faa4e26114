"""The cache protocol of every tensor derived from weights (packs, stacks, folds, bounds, positional encodings), held once.

Key: ident() of each source + the site's `extra` + cache_epoch().  An in-place update autograd sees bumps `_version` and
misses; a write through `param.data` does not, so whatever writes that way bumps the epoch (occnet_amd/__init__.py).
Pin: an entry holds its sources, so no address is recycled under a live key.  Bound: `capacity` entries, the oldest-inserted
leaves first.  Miss: build() makes the value; if it raises, nothing is stored.  A source its producer marked `_occ_no_cache`
(a temporary rebuilt every call: its entry could never hit again) is built without reading or writing the cache.
Module-level caches register (invalidate_caches() empties them); single-entry ones hang on their owner module (owned()) and
are retired by the epoch alone."""
from . import cache_epoch

_REGISTERED = []


def ident(t):
    """(data_ptr, _version, shape, stride, device), None for None.  Kept on the tensor object and handed out again while address
    and version stand (two reads, not five; views are objects of their own): a keyed tensor's geometry changed in place
    (as_strided_, transpose_) bumps no _version and needs an epoch bump, as a write through `.data` does."""
    if t is None:
        return None
    memo, ptr, version = t.__dict__.get('_occ_ident'), t.data_ptr(), t._version
    if memo is None or memo[0] != ptr or memo[1] != version:
        memo = t._occ_ident = (ptr, version, t.shape, t.stride(), t.device)
    return memo


def signature(tensors):
    return tuple([ident(t) for t in tensors])


class DerivedCache:
    def __init__(self, name, capacity, register=False):
        self.name, self.capacity, self.entries = name, capacity, {}        # key -> (sources, value), insertion-ordered
        if register:
            _REGISTERED.append(self)

    def get(self, sources, build, extra=()):
        """The value derived from `sources` (tensors or None) and the hashable tuple `extra`: stored object or build()."""
        key = []
        for t in sources:
            if getattr(t, '_occ_no_cache', False):
                return build()
            key.append(ident(t))
        key = tuple(key) + extra + (cache_epoch(),)
        hit = self.entries.get(key)
        if hit is not None:
            return hit[1]
        value = build()
        if len(self.entries) >= self.capacity:
            self.entries.pop(next(iter(self.entries)))
        self.entries[key] = (tuple(sources), value)
        return value

    def keys(self):
        return list(self.entries)

    def __len__(self):
        return len(self.entries)

    def clear(self):
        self.entries.clear()


def snapshot():
    """What every registered cache holds now, for restore(): a test that runs the wrappers on tensors of its own puts the
    caches back afterwards, so that they do not go on pinning those tensors."""
    return [(cache, dict(cache.entries)) for cache in _REGISTERED]


def restore(snap):
    """Put the caches of a snapshot() back to what they held then (a cache registered since is left alone)."""
    for cache, entries in snap:
        cache.entries.clear()
        cache.entries.update(entries)


def owned(owner, attr):
    """The single-entry cache that hangs on `owner` (a module) as `attr`, made at first use; nn.Module does not register it."""
    cache = owner.__dict__.get(attr)
    if cache is None:
        cache = DerivedCache(attr, 1)
        object.__setattr__(owner, attr, cache)
    return cache
