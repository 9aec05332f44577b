"""kohya's activation-side regularisers of the adapters, fused: `network_dropout` (F.dropout on the rank-r activation
lx = lora_down(x)) and `rank_dropout` (one keep / drop draw per sample and rank, broadcast over tokens, survivors scaled by
1 / (1 - p)).  The launch plans multiply the rank-r buffers they already materialise by the factor f[token, rank] right behind
their producers (plan/emit.py, csrc/qfx_lora_dropout.hip); the mask is never stored, forward and backward regenerate it from a
counter-based generator (Philox4x32-10; include/qfx.h is the definition).  This module owns the 8 device words that drive it.

Deviation from kohya: another random stream (torch's generator there, Philox counters keyed by seed, step, sample, token and the
adapter's name here), hence other masks -- with the same distribution and the same scaling.  kohya's `module_dropout` is left out on
purpose (it skips the optimizer update of a dropped module, which the flat-state optimizers cannot express without a per-tensor
skip table), and so is peft's `lora_dropout` (a dropout on x [tokens, K]; the reference pins it to 0.0).  Adapters on the
conditioning head ([B, K] vectors, cond_hip.py) run without dropout, and the MX-FP8 trunk refuses the option (NotImplementedError).
"""
from __future__ import annotations

import zlib

import torch

from . import ops

MXFP8_REFUSAL = ("network_dropout / rank_dropout with the MX-FP8 trunk (quantize_trunk): the quantising down projections are not "
                 "covered; use the bf16 trunk")
STATE_KEY = "lora_dropout"      # the one key a train step's state_dict / checkpoint carries when the feature is on


def check_probability(p, what):
    p = 0.0 if p is None else float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{what} must satisfy 0 <= p < 1, not {p}")
    return p


def site_key(name: str) -> int:
    """The 32-bit key of an adapter in the generator's counter: crc32 of the adapted module's qualified name."""
    return zlib.crc32(name.encode()) & 0xFFFFFFFF


class LoraDropoutState:
    """The device state of the adapter dropout of one model: int32 [8] = seed_lo, seed_hi, step, active, thr_elem, thr_rank,
    scale, sample0.  `step` lives on the device (the forward program advances it, in a captured graph too); the other words are
    written from the host, each only when its value changes.  enabled: the training-mode switch (a train step's eval() / train(),
    the samplers); the masks apply while it is set AND the model is in training mode."""

    def __init__(self, device, network_dropout=0.0, rank_dropout=0.0, seed=0):
        self.network_dropout = check_probability(network_dropout, "network_dropout")
        self.rank_dropout = check_probability(rank_dropout, "rank_dropout")
        self.seed = int(seed)
        self.enabled = True
        self._host = ops.lora_dropout_state_words(self.seed, 0, 0, self.network_dropout, self.rank_dropout, 0)
        self.words = torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in self._host], dtype=torch.int32, device=device)

    def _set(self, idx, value):
        value = int(value) & 0xFFFFFFFF
        if self._host[idx] != value:
            self._host[idx] = value
            self.words[idx].fill_(value - (1 << 32) if value >= 1 << 31 else value)

    def set_active(self, on: bool):
        self._set(3, int(bool(on)))

    def set_sample0(self, sample0: int):
        self._set(7, sample0)

    @property
    def active(self) -> bool:
        return bool(self._host[3])

    def step(self) -> int:
        """The number of training forwards drawn so far (reads the device word: synchronises)."""
        return int(self.words[2].item()) & 0xFFFFFFFF

    def set_step(self, step: int):
        self._host[2] = None      # the device advances it: never trusted as a cache
        self._set(2, step)

    def host_words(self, step=None):
        """The 8 words as Python ints with the device's step (or `step`): what qfx_lora_dropout_factors_host takes."""
        w = list(self._host)
        w[2] = self.step() if step is None else int(step)
        return w

    def state_dict(self):
        return {"seed": self.seed, "step": self.step(), "network_dropout": self.network_dropout, "rank_dropout": self.rank_dropout}
