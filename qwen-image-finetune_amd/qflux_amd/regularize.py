"""Max-norm regularisation of the adapters (kohya's --scale_weight_norms: LoRANetwork.apply_max_norm_regularization) over the flat
LoRA buffer.

After an optimizer step every adapter pair whose effective weight change `scaling * B @ A` has a Frobenius norm above max_norm is
scaled back onto it, A and B by the same factor sqrt(max_norm / norm); the number of pairs scaled and the mean and maximum norm
are what people watch to see an adapter overfit.  kohya loops over the state dict, forms every [out, in] product and synchronises
twice per pair; here it is ONE launch over the flat buffer (qfx_maxnorm_apply, include/qfx.h: the norm from the two r x r Gram
matrices in fp64, every other rounding point in fp32 as written there) and nothing synchronises until stats() is asked.

adapter_pairs finds the pairs of a model, MaxNormState holds the table and the output buffers of one store layout and plugs into
the train steps (QwenLoraTrainStep(max_weight_norm=...)), MaxNorm is the object for the reference's own loop, called behind
optimizer.step().  kohya's package is not a dependency: the semantics are restated (tests/maxnorm_ref.py) and are not pinned
against the package.
"""
from __future__ import annotations

import math

import torch

from . import ops
from .modules import QfxLoraLinear

__all__ = ["adapter_pairs", "check_max_norm", "MaxNormState", "MaxNorm", "ensure_state"]

MAX_RANK = ops.MAXNORM_MAX_RANK


def check_max_norm(max_norm, what="max_weight_norm"):
    """None, or the threshold as a float: positive, inf allowed ("measure only")."""
    if max_norm is None:
        return None
    if isinstance(max_norm, bool) or not isinstance(max_norm, (int, float)):
        raise ValueError(f"{what} must be a positive float or inf, not {max_norm!r}")
    max_norm = float(max_norm)
    if math.isnan(max_norm) or not max_norm > 0:
        raise ValueError(f"{what} must be a positive float or inf, not {max_norm}")
    return max_norm


def _store_of(dit_or_store):
    return getattr(dit_or_store, "lora_store", dit_or_store)      # a model's property re-packs a stale store; a store is taken as it is


def adapter_pairs(dit_or_store):
    """The lora_A / lora_B pairs of the flat store, one per adapted linear (the conditioning head's among them), for each module's
    active adapter, in named_modules() order: a list of (module name, off_a, off_b, r, in_features, out_features, scaling)."""
    store = _store_of(dit_or_store)
    where = {id(p): off for _, p, off, _ in store.entries}
    pairs = []
    for name, m in store.model.named_modules():
        if not isinstance(m, QfxLoraLinear):
            continue
        a, b = m.A, m.B
        if id(a) not in where or id(b) not in where:
            raise ValueError(f"adapter of {name!r} is not in the flat LoRA store")
        r, nin = a.shape
        nout = b.shape[0]
        if b.shape[1] != r:
            raise ValueError(f"adapter of {name!r}: lora_A is {tuple(a.shape)}, lora_B is {tuple(b.shape)}")
        pairs.append((name, where[id(a)], where[id(b)], int(r), int(nin), int(nout), float(m.scaling[m.active_adapter])))
    return pairs


def _layout_key(store):
    """Cheap per step: the store's entries, its device and the model's active adapter (the pairs are walked on a change only)."""
    return (tuple((off, k) for _, _, off, k in store.entries), str(store.pflat.device), getattr(store.model, "_adapter_name", None))


def ensure_state(state, dit_or_store):
    """The MaxNormState for the store's current layout: rebuilt when there is none yet or the adapter set changed, as
    ema.ensure_state keys the shadows on the layout."""
    store = _store_of(dit_or_store)
    if state is None or state.key != _layout_key(store):
        state = MaxNormState(store)
    return state


class MaxNormState:
    """The descriptor table and the output buffers of one store layout.  After apply(): norms / ratios are the per-pair device
    tensors (the norm after scaling, the ratio applied; 1 where the pair was left alone), summary holds (keys_scaled, mean norm,
    max norm, 0) on the device, names[i] is the module of pair i.  Nothing here synchronises but stats()."""

    def __init__(self, dit_or_store):
        store = _store_of(dit_or_store)
        pairs = adapter_pairs(store)
        if not pairs:
            raise ValueError("max-norm regularisation: the model has no adapters")
        for name, _, _, r, _, _, _ in pairs:
            if r > MAX_RANK:
                raise NotImplementedError(f"max-norm regularisation: the adapter of {name!r} has rank {r}; ranks above {MAX_RANK} "
                                          "are not implemented")
        self.key = _layout_key(store)
        self.names = [p[0] for p in pairs]
        dev = store.pflat.device
        self.layout = ops.maxnorm_table([p[1:] for p in pairs], device=dev, n_elems=store.pflat.numel())
        self.norms = torch.zeros(len(pairs), dtype=torch.float32, device=dev)
        self.ratios = torch.ones(len(pairs), dtype=torch.float32, device=dev)
        self.summary = torch.zeros(4, dtype=torch.float32, device=dev)
        self.max_norm = None        # the threshold of the last apply()

    def apply(self, store, max_norm):
        """One launch on the current stream over store.pflat."""
        self.max_norm = float(max_norm)
        ops.maxnorm_apply(store.pflat, self.layout, self.max_norm, self.norms, self.ratios, self.summary)

    def stats(self):
        """(keys_scaled: int, mean norm: float, max norm: float) of the last apply(); synchronises."""
        k, mean, mx, _ = self.summary.tolist()
        return int(k), mean, mx


class MaxNorm:
    """For the stock loop: `reg = MaxNorm(dit, max_norm)` once, `reg.step()` behind every optimizer.step() (one launch, no host
    synchronisation), `reg.stats()` where the three numbers are logged (the only place that synchronises)."""

    def __init__(self, dit, max_norm):
        self.max_norm = check_max_norm(max_norm, "max_norm")
        if self.max_norm is None:
            raise ValueError("max_norm must be a positive float or inf, not None")
        self._target = dit
        self._state = ensure_state(None, dit)

    @torch.no_grad()
    def step(self):
        self._state = ensure_state(self._state, self._target)
        self._state.apply(_store_of(self._target), self.max_norm)

    def stats(self):
        return self._state.stats()

    norms = property(lambda self: self._state.norms)
    ratios = property(lambda self: self._state.ratios)
    names = property(lambda self: self._state.names)
