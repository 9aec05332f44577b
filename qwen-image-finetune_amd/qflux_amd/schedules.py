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


WEIGHTING_SCHEMES = ("none", "logit_normal", "mode", "sigma_sqrt", "cosmap")
HUBER_SCHEDULES = ("constant", "exponential")


def timestep_density(scheme: str, batch_size: int, logit_mean: float = 0.0, logit_std: float = 1.0, mode_scale: float = 1.29,
                     generator=None):
    """diffusers.training_utils.compute_density_for_timestep_sampling on the CPU: u [B] in [0, 1].  "logit_normal" and "mode" shape
    the density; "none", "sigma_sqrt" and "cosmap" draw uniformly (the last two act through loss_weighting).  "none" consumes the
    generator exactly as torch.rand(size=(B,)) does."""
    if scheme not in WEIGHTING_SCHEMES:
        raise ValueError(f"weighting_scheme is one of {WEIGHTING_SCHEMES}, not {scheme!r}")
    if scheme == "logit_normal":
        return torch.sigmoid(torch.normal(mean=logit_mean, std=logit_std, size=(batch_size,), device="cpu", generator=generator))
    u = torch.rand(size=(batch_size,), device="cpu", generator=generator)
    if scheme == "mode":
        u = 1 - u - mode_scale * (torch.cos(math.pi * u / 2) ** 2 - 1 + u)
    return u


def loss_weighting(scheme: str, sigmas: torch.Tensor) -> torch.Tensor:
    """diffusers.training_utils.compute_loss_weighting_for_sd3: the per-sample loss weight, fp32.  "sigma_sqrt": sigma^-2;
    "cosmap": 2 / (pi (1 - 2 sigma + 2 sigma^2)); every other scheme: ones."""
    sigmas = sigmas.float()
    if scheme == "sigma_sqrt":
        return sigmas ** -2.0
    if scheme == "cosmap":
        return 2 / (math.pi * (1 - 2 * sigmas + 2 * sigmas ** 2))
    return torch.ones_like(sigmas)


def huber_threshold(schedule: str, huber_c: float, timesteps: torch.Tensor) -> torch.Tensor:
    """kohya's per-sample Huber threshold, fp32 [B]: "constant": huber_c; "exponential": huber_c ** (timestep / 1000), formed in fp64
    (huber_c at t = 1000, pure noise, towards 1 at t = 0).  The "snr" schedule needs a DDPM alpha table flow matching has not."""
    if schedule not in HUBER_SCHEDULES:
        raise ValueError(f"huber_schedule is one of {HUBER_SCHEDULES}, not {schedule!r}")
    t = timesteps.double()
    if schedule == "constant":
        return torch.full_like(t, huber_c).float()
    return (huber_c ** (t / 1000)).float()


def shift_time(u: torch.Tensor, shift: float) -> torch.Tensor:
    """The time shift of flowmatch_tables applied to continuous times: shift u / (1 + (shift - 1) u); the identity at shift = 1."""
    return u if shift == 1.0 else shift * u / (1 + (shift - 1) * u)


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
