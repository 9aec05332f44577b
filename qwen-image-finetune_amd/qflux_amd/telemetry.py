"""Per-adapter training telemetry over the flat LoRA buffers: gradient, weight and update norms of every adapter tensor.

The per-tensor diagnostics a LoRA run is judged by -- each tensor's gradient norm, its weight norm, how far the last step moved it
(||dp|| / ||p||, the ~1e-3 rule of thumb) and which tensor produced the first NaN -- cost a host loop of `.norm().item()` over
every adapter view when written in Python.  Here they are two launches that bracket the optimizer's (qfx_adapter_stats,
include/qfx.h: one workgroup per tensor, sums in a fixed order, no atomics) and ONE device-to-host copy when somebody reads.

AdapterStats holds the snapshot buffer, the descriptor table and the rows of one store layout.  The train steps drive it with
`QwenLoraTrainStep(adapter_stats_every=N)`; in the stock loop it goes around optimizer.step() like qflux_amd.ema.EMAModel and
regularize.MaxNorm go behind it:

    stats = AdapterStats.from_optimizer(optimizer)
    stats.before_step(); optimizer.step(); stats.after_step()
    if step % 50 == 0: log(stats.summary())
"""
from __future__ import annotations

import math

import torch

from . import ops

__all__ = ["AdapterStats", "rows_to_dict", "summarize"]

FIELDS = ("grad_norm", "weight_norm", "update_norm", "update_ratio", "grad_absmax", "grad_nonfinite", "weight_nonfinite")


def rows_to_dict(rows, names):
    """rows: the kernel's rows (a numpy structured array with ops.STATS_ROW_FIELDS, or any sequence of mappings with them) ->
    {name: {grad_norm, weight_norm, update_norm, update_ratio, grad_absmax, grad_nonfinite, weight_nonfinite}} in table order.
    The roots and the ratio are formed in fp64; update_ratio = update_norm / weight_norm, 0 where the weight norm is 0."""
    out = {}
    for name, r in zip(names, rows):
        gn, wn, un = (math.sqrt(float(r[f])) for f in ("grad_sq", "weight_sq", "update_sq"))
        out[name] = dict(grad_norm=gn, weight_norm=wn, update_norm=un, update_ratio=un / wn if wn > 0 else 0.0,
                         grad_absmax=float(r["grad_absmax"]), grad_nonfinite=int(r["grad_nonfinite"]),
                         weight_nonfinite=int(r["weight_nonfinite"]))
    return out


def _median(v):
    v = sorted(v)
    if not v:
        return None
    h = len(v) // 2
    return v[h] if len(v) % 2 else 0.5 * (v[h - 1] + v[h])


def summarize(stats, kinds):
    """stats: what rows_to_dict returns; kinds: "A" / "B" / None per tensor, in the same order ->
    dict(grad_norm = the global gradient norm (the root of the fp64 sum of the tensors' squared norms),
         update_ratio_max_A / update_ratio_median_A / update_ratio_max_B / update_ratio_median_B over the lora_A / lora_B tensors
         (None where there is no such tensor), first_nonfinite_grad = the name of the first tensor, in table order, with a
         non-finite gradient element, or None)."""
    out = dict(grad_norm=math.sqrt(math.fsum(s["grad_norm"] ** 2 for s in stats.values())))
    for kind in ("A", "B"):
        r = [s["update_ratio"] for s, k in zip(stats.values(), kinds) if k == kind]
        out[f"update_ratio_max_{kind}"] = max(r) if r else None
        out[f"update_ratio_median_{kind}"] = _median(r)
    out["first_nonfinite_grad"] = next((n for n, s in stats.items() if s["grad_nonfinite"] > 0), None)
    return out


def _layout_key(store):
    return (tuple((off, k) for _, _, off, k in store.entries), str(store.pflat.device), getattr(store.model, "_adapter_name", None))


class AdapterStats:
    """`AdapterStats(dit_or_store)`: before_step() in front of the optimizer's launch, after_step() behind it, both on the current
    stream and without a host synchronisation; read() / summary() copy the rows to the host once per collected step and are the
    only calls that synchronise.  Reads store.pflat / store.gflat only, so every optimizer family is served alike.  The table and
    the buffers follow the store's layout (a changed adapter set rebuilds them; what was collected before is dropped)."""

    def __init__(self, dit_or_store):
        self._target = dit_or_store
        self.key = None
        self._cache = None
        self._pending = False        # before_step() ran, after_step() not yet
        self.collected = 0           # completed before_step() / after_step() pairs
        self._ensure()

    @classmethod
    def from_optimizer(cls, opt):
        """For the stock loop: `opt` is any class of qflux_amd.optim; before_step() / after_step() go around opt.step().  The
        loop has clipped already (optim.py), so before_step() takes no clip arguments there."""
        raw = getattr(opt, "_raw_store", None)
        if raw is None:
            raise ValueError("AdapterStats.from_optimizer: not a qflux_amd.optim optimizer")
        return cls(raw.model if hasattr(raw.model, "lora_store") else raw)

    def _store(self):
        return getattr(self._target, "lora_store", self._target)      # a model's property re-packs a stale store

    def _ensure(self):
        st = self._store()
        if st.pflat is None:
            raise ValueError("adapter statistics: the model has no adapters")
        key = _layout_key(st)
        if self.key != key:
            dev = st.pflat.device
            self.layout = ops.stats_table(st, dev)
            self.prev = torch.zeros_like(st.pflat)
            self.out = torch.zeros(32 * self.layout.n_entries, dtype=torch.uint8, device=dev)
            self.key, self._cache, self._pending, self.collected = key, None, False, 0
        return st

    names = property(lambda self: self.layout.names)
    kinds = property(lambda self: self.layout.kinds)

    @torch.no_grad()
    def before_step(self, gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
        """Phase 0: the gradient statistics of g * clip (the optimizer's own clip prologue on gnorm_sq / max_norm / grad_scale; the
        defaults give clip = 1) and the snapshot of the weights."""
        st = self._ensure()
        st.ensure_grads()
        ops.adapter_stats(st.pflat, st.gflat, self.prev, self.layout, self.out, 0, gnorm_sq, max_norm, grad_scale)
        self._pending, self._cache = True, None

    @torch.no_grad()
    def after_step(self):
        """Phase 1: the weight statistics and the norm of the update since before_step()."""
        if not self._pending:
            raise RuntimeError("AdapterStats.after_step() without a before_step(): there is no snapshot to measure the update against")
        st = self._store()
        if _layout_key(st) != self.key:
            raise RuntimeError("AdapterStats.after_step(): the adapter set changed since before_step()")
        ops.adapter_stats(st.pflat, None, self.prev, self.layout, self.out, 1)
        self._pending, self._cache = False, None
        self.collected += 1

    def read(self):
        """{tensor name: {grad_norm, weight_norm, update_norm, update_ratio, grad_absmax, grad_nonfinite, weight_nonfinite}} of the
        last collected step, keyed as save_lora_weights keys the tensors; None before the first one.  One device-to-host copy,
        kept until the next launch."""
        if self.collected == 0:
            return None
        if self._cache is None:
            self._cache = rows_to_dict(ops.stats_rows(self.out, self.layout.n_entries), self.layout.names)
        return self._cache

    def summary(self):
        """summarize() of read(); None before the first collected step."""
        stats = self.read()
        return None if stats is None else summarize(stats, self.layout.kinds)
