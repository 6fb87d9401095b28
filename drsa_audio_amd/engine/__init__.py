"""HIP LRP engine: plan compilation (``parse.py``, ``plan.py``, ``schedule.py``) + execution (``plan.py``).

``get_engine`` caches compiled plans per (model, composite) while the model's parameters are
unchanged.  The cache holds the model and the composite only through weak references (the
engine itself keeps no strong reference to either), drops an entry as soon as its model or
composite is garbage-collected, and keeps at most ``DRSA_AMD_ENGINE_CACHE`` (default 8) entries
in LRU order; an evicted engine releases its device buffers.  So a workflow that builds a new
``HeatmapGenerator`` per pass (the reference does, cxai/xai/pixelflipping/cpf.py:161) keeps a
bounded device footprint.  A composite that maps a module to a user-written ``Hook`` (its own
``backward``) gets the autograd slow path ``HookedAutograd`` (``hooks.py``) instead of a plan.
"""
from __future__ import annotations

import os
import weakref
from collections import OrderedDict

import torch

from .hooks import HookedAutograd, has_custom_hooks
from .plan import EngineError, LRPEngine, bf16_backward_default

_MAX = max(1, int(os.environ.get("DRSA_AMD_ENGINE_CACHE", "8")))
_CACHE: "OrderedDict[tuple, _Entry]" = OrderedDict()


class _Entry:
    __slots__ = ("model_ref", "comp_ref", "fp", "eng", "finalizers")

    def __init__(self, model_ref, comp_ref, fp, eng):
        self.model_ref, self.comp_ref, self.fp, self.eng = model_ref, comp_ref, fp, eng
        self.finalizers = []


def _fingerprint(model):
    """Parameters AND buffers: the plan folds BatchNorm running statistics into the weights, so a
    train-mode forward or a buffers-only load_state_dict must recompile.  Also the DRSA projection
    matrices, which are plain tensor attributes (``Projection.U``, ``InvProjection.U_inv``,
    ``ProjectionModel.U``; cxai/model/modify_model.py:4-123) and the table of a MultiProjectionModel
    (``U_tab``): the plan caches U and P = UU^T - I, so an in-place update (``_version``) or a
    rebinding (``data_ptr``) of U, or of any entry of the table, must recompile too."""
    proj = []
    for m in model.modules():
        for attr in ("U", "U_inv"):
            t = getattr(m, attr, None)
            if isinstance(t, torch.Tensor):
                proj.append((attr, t.data_ptr(), t._version))
        # a plain attribute of the Multi* modules: read from the instance dict, since a getattr that misses costs
        # every other module of every model a walk through nn.Module.__getattr__ on each get_engine call
        t = m.__dict__.get("U_tab")
        if isinstance(t, torch.Tensor):
            proj.append(("U_tab", t.data_ptr(), t._version))
    return (tuple((p.data_ptr(), p._version) for p in model.parameters()) +
            tuple((b.data_ptr(), b._version) for b in model.buffers()) + tuple(proj))


def _rules_fingerprint(model, composite):
    """The rule the composite gives every module, with its scalar parameters (gamma, stabilizer,
    alpha, ...): the plan bakes them into prepared weight sets and constant denominators (conv and
    dense alike), so two composites that differ only in one layer's rule or in its gamma have
    different keys, and a rule edited in place on a cached composite recompiles."""
    if composite is None:
        return ()
    out = []
    for name, rule in sorted(composite.rules(model).items()):
        fields = []
        for k, v in sorted(getattr(rule, "__dict__", {}).items()):
            v = _frozen(v)
            if v is not _SKIP:
                fields.append((k, v))
        out.append((name, type(rule).__name__, tuple(fields)))
    return tuple(out)


_SKIP = object()


def _frozen(v):
    """A rule field as a hashable key part: scalars as they are, lists / tuples / sets (zero_params
    may be given as any of them) as tuples, tensors (ZBox bounds) by shape, dtype and content -- not
    by identity: an in-place edit recompiles, an equal copy does not --, anything else (callables) left out."""
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, torch.Tensor):
        t = v.detach().cpu().contiguous()
        return ("tensor", tuple(t.shape), str(t.dtype), t.reshape(-1).view(torch.uint8).numpy().tobytes())
    if isinstance(v, (list, tuple, set, frozenset)):
        items = sorted(v, key=repr) if isinstance(v, (set, frozenset)) else v
        parts = tuple(_frozen(i) for i in items)
        return _SKIP if any(p is _SKIP for p in parts) else parts
    return _SKIP


def cache_key(model, composite):
    """What a cached plan is valid for: the model's tensors, the composite's rules, the engine options."""
    return (_fingerprint(model), _rules_fingerprint(model, composite), bf16_backward_default())


def _ref(obj):
    if obj is None:
        return lambda: None
    return weakref.ref(obj)


def _evict(key) -> None:
    e = _CACHE.pop(key, None)
    if e is not None:
        for f in e.finalizers:        # one live finalizer per cached entry, never a pile-up
            f.detach()
        e.eng.release()


def get_engine(model, composite) -> LRPEngine:
    """Compiled plan for (model, composite), cached while the model's parameters are unchanged."""
    key = (id(model), id(composite))
    fp = cache_key(model, composite)   # the bf16_backward option selects different kernels
    e = _CACHE.get(key)
    if e is not None:
        if e.model_ref() is model and e.comp_ref() is composite and e.fp == fp:
            _CACHE.move_to_end(key)
            return e.eng
        _evict(key)          # stale: ids reused by new objects, or the weights changed
    rules = composite.rules(model) if composite is not None else {}
    # a composite with a user-written Hook (its own backward) cannot be compiled: autograd slow path
    eng = HookedAutograd(model, composite) if has_custom_hooks(rules) else LRPEngine(model, composite)
    entry = _Entry(_ref(model), _ref(composite), fp, eng)
    _CACHE[key] = entry
    entry.finalizers.append(weakref.finalize(model, _evict, key))
    if composite is not None:
        entry.finalizers.append(weakref.finalize(composite, _evict, key))
    while len(_CACHE) > _MAX:
        _evict(next(iter(_CACHE)))
    return eng


def cache_size() -> int:
    return len(_CACHE)


def clear_cache() -> None:
    for key in list(_CACHE):
        _evict(key)


__all__ = ["LRPEngine", "HookedAutograd", "EngineError", "get_engine", "cache_size", "clear_cache"]
