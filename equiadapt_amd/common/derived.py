"""Tensors derived from a module's parameters and buffers (folded conv + batch-norm banks, packed weights, filter spectra), kept until
a source changes -- and the one rule for "changed".

A source tensor is unchanged while it is the same object, at the same ``_version``, over the same ``data_ptr()``.  Each of the three
catches a write the other two miss: an in-place op bumps ``_version``; ``module.to()`` / ``.float()`` / ``param.data = ...`` swap the
storage under the same object at the same version; ``bn.running_mean = t`` or a loader that assigns puts another object there, whose
version may equal the old one's.  An entry keeps its source objects alive, so an ``id`` cannot come round again while it lives.
"""
from operator import is_
from typing import Any, Callable, Hashable, Sequence, Tuple

import torch


def _stamp(live) -> Tuple[list, list]:
    return [t._version for t in live], list(map(torch.Tensor.data_ptr, live))         # (on every forward: the cheapest spelling of each)


class _Entry:
    __slots__ = ("sources", "live", "stamp", "context", "parent", "value")

    def __init__(self, sources=(), context=None, parent=None):
        self.sources, self.context, self.parent = tuple(sources), context, parent
        self.live = tuple(t for t in self.sources if t is not None)
        self.stamp = _stamp(self.live)                                                 # (before the value is built from them)


class DerivedCache:
    def __init__(self):
        self._entries: dict = {}

    def get(self, slot: Hashable, sources: Sequence, build: Callable[[], Any], *context: Hashable):
        """The value of ``build()`` under `slot`, rebuilt when a source (a tensor, or None for an absent one) has changed or `context`
        (hashables beside the tensors: an input shape, a tile size) differs from the one it was built under."""
        e = self._entries.get(slot)
        if (e is not None and e.context == context and len(sources) == len(e.sources) and all(map(is_, sources, e.sources))
                and e.stamp == _stamp(e.live)):
            return e.value
        e = _Entry(sources, context)
        e.value = build()
        self._entries[slot] = e
        return e.value

    def derived(self, parent_slot: Hashable, slot: Hashable, build: Callable[[], Any]):
        """The value of ``build()`` under `slot`, something made from `parent_slot`'s value: kept while `parent_slot` holds the very
        entry this one was built beside, rebuilt once that has been rebuilt."""
        parent = self._entries[parent_slot]
        e = self._entries.get(slot)
        if e is None or e.parent is not parent:
            e = _Entry(parent=parent)
            e.value = build()
            self._entries[slot] = e
        return e.value

    def __contains__(self, slot: Hashable) -> bool:
        return slot in self._entries

    def clear(self) -> None:
        self._entries.clear()


def bn_eval_affine(bn) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scale, shift) of a batch-norm in eval mode: bn(x) = x * scale + shift per feature."""
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    return scale, bn.bias - bn.running_mean * scale


def refuse_e2cnn_state_dict(state_dict, own_prefix: str, network_name: str, advice: str, extra_markers: Sequence[str] = ()) -> None:
    """Raise on a checkpoint of the reference's e2cnn form of `network_name` instead of failing on a shape mismatch: e2cnn stores a flat
    coefficient vector per layer over its steerable basis (``...weights`` 1-D, ``...basisexpansion...`` / ``...filter`` buffers).
    extra_markers: further substrings of a key that only e2cnn writes; advice: the rest of the message."""
    for k, v in state_dict.items():
        if k.startswith(own_prefix) and ("basisexpansion" in k or k.endswith(".filter") or any(m in k for m in extra_markers)
                                         or (k.endswith(".weights") and getattr(v, "dim", lambda: 2)() == 1)):
            raise RuntimeError(f"state_dict key {k!r} comes from e2cnn's steerable-basis parameterisation (the reference's {network_name}). "
                               + advice)
