"""Schedule helpers on the host: the flow-matching timestep / sigma tables of the train step (and of the model's modulation table)
and the learning-rate multipliers of the reference's lr_scheduler configs.  No dependency on the step or the model."""
from __future__ import annotations

import math

import torch


def flowmatch_tables(num_train_timesteps: int = 1000, shift: float = 1.0):
    """FlowMatchEulerDiscreteScheduler.timesteps / .sigmas as built at construction (third-party lookup
    tables, qwen_image_edit_trainer.py:807-810,851-861; dynamic shifting => identity shift at init)."""
    ts = torch.linspace(1, num_train_timesteps, num_train_timesteps).flip(0)
    sig = ts / num_train_timesteps
    sig = shift * sig / (1 + (shift - 1) * sig)
    return sig * num_train_timesteps, sig


def get_scheduler(name: str, num_warmup_steps: int = 0, num_training_steps: int | None = None, num_cycles: float = 0.5):
    """lr multiplier(step) of diffusers.optimization.get_scheduler for the schedules the reference's configs use
    (base_trainer.py:900-916): constant, constant_with_warmup, linear, cosine.  Use: step.lr = base_lr * f(global_step)."""
    def warm(s):
        return float(s) / float(max(1, num_warmup_steps)) if s < num_warmup_steps else None

    if name == "constant":
        return lambda s: 1.0
    if name == "constant_with_warmup":
        return lambda s: (warm(s) if warm(s) is not None else 1.0)
    if name == "linear":
        return lambda s: (warm(s) if warm(s) is not None else
                          max(0.0, float(num_training_steps - s) / float(max(1, num_training_steps - num_warmup_steps))))
    if name == "cosine":
        def f(s):
            w = warm(s)
            if w is not None:
                return w
            prog = float(s - num_warmup_steps) / float(max(1, num_training_steps - num_warmup_steps))
            return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * prog)))
        return f
    raise ValueError(f"unsupported lr scheduler {name!r}")
