"""occnet_amd — MI355X (gfx950) native forward hot path of OccNet / BEVFormer-occ.

Layout:
  csrc/      hand-written HIP kernels + the C ABI declared in include/occnet_amd.h
  lib/       libocc_amd.so (built in-tree by `python -m occnet_amd.build`)
  _lib.py    ctypes binding of the C ABI (fails loudly if the library is missing)
  ext.py     mirror of the reference's `mmcv._ext` operator module
  plugin/    host-side mirror of projects/mmdet3d_plugin (registry names, modules, configs)
"""
__version__ = "0.1.0"


# Tensors derived from weights are cached by one protocol, occnet_amd/derived.py: keys carry every source's
# (data_ptr, _version, shape, stride, device) and cache_epoch().  Writes through `param.data` bump no _version, so whatever
# writes that way bumps the epoch: load_state_dict on any plugin module (post hook), BEVFormerOcc.train()'s content
# fingerprint on a train -> eval transition, and an explicit occnet_amd.invalidate_caches() after EMA / manual .data surgery.
# (The folded inference backbone holds COPIES: it re-checks derived.signature() of its source parameters the first time it is
# used after the model has been in training mode.)
_CACHE_EPOCH = 0


def cache_epoch():
    return _CACHE_EPOCH


def invalidate_caches(model=None):
    """Drop every derived-weight cache; with `model` (a BEVFormerOcc) also rebuild its folded inference
    backbone from the live parameters.  Call after writing parameters through `.data`."""
    global _CACHE_EPOCH
    _CACHE_EPOCH += 1
    for cache in derived._REGISTERED:
        cache.clear()
    if model is not None and getattr(model, '_inference_backbone', None) is not None:
        model.enable_fused_backbone(**model._inference_backbone_args)


from . import derived  # noqa: E402  (it reads cache_epoch)
