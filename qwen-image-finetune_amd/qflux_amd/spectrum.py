"""The spectrum of every adapter: the singular values of `scaling * B @ A` and what follows from them (Frobenius and spectral norm,
stable rank, effective rank, numeric rank) -- how one finds out whether r = 16 was too much or too little.

kohya-style tools take a full SVD of each [out, in] product with a host synchronisation per pair; here it is ONE launch over the
flat LoRA buffer (qfx_lora_spectrum, include/qfx.h: the two r x r Gram matrices of a pair and two small symmetric eigenproblems,
all in fp64 inside one workgroup) and ONE device -> host copy.  adapter_spectrum / spectrum_summary are the calls, SpectrumState
holds the table and the output buffers of one store layout (keyed like regularize.ensure_state).
"""
from __future__ import annotations

import math

import torch

from . import ops
from .regularize import _layout_key, _store_of, adapter_pairs

__all__ = ["SpectrumState", "ensure_state", "adapter_spectrum", "spectrum_summary", "summarize"]

MAX_RANK = ops.LORA_SVD_MAX_RANK
_LD = 64          # columns of the device sv buffer; the packed readback row is _LD + 4 doubles (sv, then info)


class SpectrumState:
    """The descriptor table and the output buffers of one store layout.  launch() is one kernel launch on the current stream and
    never synchronises; read() is the one device -> host copy."""

    def __init__(self, dit_or_store, workspace=False):
        store = _store_of(dit_or_store)
        pairs = adapter_pairs(store)
        if not pairs:
            raise ValueError("adapter spectrum: the model has no adapters")
        for name, _, _, r, _, _, _ in pairs:
            if r > MAX_RANK:
                raise NotImplementedError(f"adapter spectrum: the adapter of {name!r} has rank {r}; ranks above {MAX_RANK} "
                                          "are not implemented")
        self.key = _layout_key(store)
        self.names = [p[0] for p in pairs]
        self.ranks = [p[3] for p in pairs]
        self.scalings = [p[6] for p in pairs]
        dev = store.pflat.device
        self.layout = ops.lora_svd_table([p[1:6] for p in pairs], device=dev, n_elems=store.pflat.numel())
        self._alloc(len(pairs), dev, workspace)

    def _alloc(self, n, dev, workspace):
        self.sv = torch.zeros(n, _LD, dtype=torch.float64, device=dev)
        self.info = torch.zeros(n, 4, dtype=torch.int32, device=dev)
        self.skipped = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ws = torch.zeros(n * ops.LORA_SVD_WS_DOUBLES, dtype=torch.float64, device=dev) if workspace else None
        self.packed = torch.zeros(n + 1, _LD + 4, dtype=torch.float64, device=dev)

    @classmethod
    def for_pairs(cls, pflat, pairs, workspace=False):
        """Over a bare flat buffer: pairs = (name, off_a, off_b, r, in_features, out_features, scaling), no model needed."""
        self = cls.__new__(cls)
        for name, _, _, r, _, _, _ in pairs:
            if r > MAX_RANK:
                raise NotImplementedError(f"adapter spectrum: the adapter of {name!r} has rank {r}; ranks above {MAX_RANK} "
                                          "are not implemented")
        self.key = None
        self.names = [p[0] for p in pairs]
        self.ranks = [int(p[3]) for p in pairs]
        self.scalings = [float(p[6]) for p in pairs]
        self.layout = ops.lora_svd_table([p[1:6] for p in pairs], device=pflat.device, n_elems=pflat.numel())
        self._alloc(len(pairs), pflat.device, workspace)
        return self

    @torch.no_grad()
    def launch(self, pflat, rank_tol=ops.LORA_SVD_RANK_TOL, max_sweeps=ops.LORA_SVD_MAX_SWEEPS):
        ops.lora_spectrum(pflat, self.layout, self.sv, self.info, self.skipped, ws=self.ws, rank_tol=rank_tol, max_sweeps=max_sweeps)

    @torch.no_grad()
    def read(self):
        """-> (sv [n, 64] fp64 of B A, unscaled; info [n, 4] int64; skipped) on the host, with ONE device -> host copy."""
        n = len(self.names)
        self.packed[:n, :_LD].copy_(self.sv)
        self.packed[:n, _LD:].copy_(self.info)
        self.packed[n, 0:1].copy_(self.skipped)
        host = self.packed.cpu()
        return host[:n, :_LD].clone(), host[:n, _LD:].to(torch.int64), int(host[n, 0])


def ensure_state(state, dit_or_store, workspace=False):
    """The SpectrumState for the store's current layout: rebuilt when there is none yet or the adapter set changed."""
    store = _store_of(dit_or_store)
    if state is None or state.key != _layout_key(store) or (workspace and state.ws is None):
        state = SpectrumState(store, workspace=workspace)
    return state


def _collect(state, sv, info):
    out, meta = {}, {}
    for i, (name, r, s) in enumerate(zip(state.names, state.ranks, state.scalings)):
        out[name] = sv[i, :r] * abs(s)
        meta[name] = dict(numeric_rank=int(info[i, 0]), sweeps=(int(info[i, 1]), int(info[i, 2])), converged=bool(info[i, 3]))
    return out, meta


def adapter_spectrum(dit_or_store, state=None, rank_tol=ops.LORA_SVD_RANK_TOL, max_sweeps=ops.LORA_SVD_MAX_SWEEPS, with_info=False):
    """{module name: fp64 tensor of the singular values of scaling * B @ A, descending, length r} for each module's active adapter:
    one launch on the current stream, one device -> host copy.  with_info: also {module name: dict(numeric_rank, sweeps,
    converged)} and the number of pairs skipped for a non-finite weight."""
    store = _store_of(dit_or_store)
    state = ensure_state(state, store)
    state.launch(store.pflat, rank_tol, max_sweeps)
    sv, info, skipped = state.read()
    out, meta = _collect(state, sv, info)
    return (out, meta, skipped) if with_info else out


def summarize(sv, numeric_rank=None, converged=None):
    """One descending spectrum -> dict(fro, spectral, stable_rank, effective_rank, numeric_rank, converged).  An all-zero spectrum
    (B = 0, every adapter before its first step) has norms 0 and ranks 0."""
    s = [float(x) for x in sv]
    s1, s2 = math.fsum(s), math.fsum(x * x for x in s)
    if not s or s[0] <= 0.0:
        stable = eff = 0.0
    else:
        stable = s2 / (s[0] * s[0])
        eff = math.exp(-math.fsum((x / s1) * math.log(x / s1) for x in s if x > 0.0))
    return dict(fro=math.sqrt(s2), spectral=s[0] if s else 0.0, stable_rank=stable, effective_rank=eff,
                numeric_rank=numeric_rank, converged=converged)


def spectrum_summary(dit_or_store, state=None, rank_tol=ops.LORA_SVD_RANK_TOL, max_sweeps=ops.LORA_SVD_MAX_SWEEPS):
    """Per adapter: the Frobenius norm sqrt(sum s^2), the spectral norm, the stable rank sum s^2 / s_0^2, the effective rank
    exp(entropy of s / sum s), the numeric rank at rank_tol and the converged flag of the two eigen-solves."""
    sv, meta, _ = adapter_spectrum(dit_or_store, state, rank_tol, max_sweeps, with_info=True)
    return {name: summarize(s, meta[name]["numeric_rank"], meta[name]["converged"]) for name, s in sv.items()}
