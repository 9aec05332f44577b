"""fp64 restatement of torch's single-tensor RAdam, NAdam and Adamax steps (torch/optim/radam.py, nadam.py, adamax.py:
_single_tensor_radam / _single_tensor_nadam / _single_tensor_adamax), statement for statement in numpy double, the non-capturable,
non-differentiable, maximize=False path -- the yardstick of tests/test_adamx_gpu.py; tests/test_adamx_cpu.py checks the yardstick
itself against the real torch.optim classes in fp64.  Nothing here touches the code under test.

State is a dict per tensor as torch keeps it: {"step", "exp_avg", "exp_avg_sq" | "exp_inf"[, "mu_product"]}; step and mu_product
are what torch keeps in its 0-dim tensors of the default dtype (fp32): mu_product is rounded to fp32 after every multiplication.
Every function updates param and the state in place and returns nothing, as torch's do."""
from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64


def new_state(family, param):
    """torch's lazy state initialisation (_init_group)."""
    z = np.zeros_like(np.asarray(param, F64))
    st = {"step": 0.0, "exp_avg": z.copy()}
    st["exp_inf" if family == "adamax" else "exp_avg_sq"] = z.copy()
    if family == "nadam":
        st["mu_product"] = 1.0
    return st


def _lerp_(start, end, weight):
    """Tensor.lerp_(end, weight) with a scalar weight (ATen/native/Lerp.h): start + weight (end - start) for |weight| < 0.5,
    end - (end - start)(1 - weight) otherwise."""
    diff = end - start
    start[...] = start + weight * diff if abs(weight) < 0.5 else end - diff * (1 - weight)


def radam(param, grad, st, *, lr, beta1, beta2, eps, weight_decay, decoupled_weight_decay=False):
    exp_avg, exp_avg_sq = st["exp_avg"], st["exp_avg_sq"]
    # update step
    st["step"] += 1
    step = st["step"]
    if weight_decay != 0:
        if decoupled_weight_decay:
            param *= 1 - lr * weight_decay
        else:
            grad = grad + weight_decay * param
    # Decay the first and second moment running average coefficient
    _lerp_(exp_avg, grad, 1 - beta1)
    exp_avg_sq *= beta2
    exp_avg_sq += (1 - beta2) * grad * grad
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    # correcting bias for the first moving moment
    bias_corrected_exp_avg = exp_avg / bias_correction1
    # maximum length of the approximated SMA
    rho_inf = 2 / (1 - beta2) - 1
    # compute the length of the approximated SMA
    rho_t = rho_inf - 2 * step * (beta2 ** step) / bias_correction2

    def _compute_rect():
        return ((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) ** 0.5

    def _compute_adaptive_lr():
        exp_avg_sq_sqrt = np.sqrt(exp_avg_sq)
        exp_avg_sq_sqrt += eps
        return (bias_correction2 ** 0.5) / exp_avg_sq_sqrt

    # Compute the variance rectification term and update parameters accordingly
    if rho_t > 5.0:
        param -= bias_corrected_exp_avg * lr * _compute_adaptive_lr() * _compute_rect()
    else:
        param -= bias_corrected_exp_avg * lr


def nadam(param, grad, st, *, lr, beta1, beta2, eps, weight_decay, momentum_decay=4e-3, decoupled_weight_decay=False):
    exp_avg, exp_avg_sq = st["exp_avg"], st["exp_avg_sq"]
    # update step
    st["step"] += 1
    step = st["step"]
    bias_correction2 = 1 - beta2 ** step
    if weight_decay != 0:
        if decoupled_weight_decay:
            # Perform stepweight decay
            param *= 1 - lr * weight_decay
        else:
            grad = grad + weight_decay * param
    # calculate the momentum cache \mu^{t} and \mu^{t+1}
    mu = beta1 * (1.0 - 0.5 * (0.96 ** (step * momentum_decay)))
    mu_next = beta1 * (1.0 - 0.5 * (0.96 ** ((step + 1) * momentum_decay)))
    # update mu_product (a 0-dim fp32 tensor in torch: the product is rounded to fp32)
    st["mu_product"] = float(F32(st["mu_product"]) * F32(mu))
    mu_product = st["mu_product"]
    # decay the first and second moment running average coefficient
    _lerp_(exp_avg, grad, 1 - beta1)
    exp_avg_sq *= beta2
    exp_avg_sq += (1 - beta2) * grad * grad
    denom = np.sqrt(exp_avg_sq / bias_correction2)
    mu_product_next = mu_product * mu_next
    denom += eps
    param += (-lr * (1.0 - mu) / (1.0 - mu_product)) * grad / denom
    param += ((-lr * mu_next) / (1.0 - mu_product_next)) * exp_avg / denom


def adamax(param, grad, st, *, lr, beta1, beta2, eps, weight_decay):
    exp_avg, exp_inf = st["exp_avg"], st["exp_inf"]
    # update step
    st["step"] += 1
    if weight_decay != 0:
        grad = grad + weight_decay * param
    # Update biased first moment estimate.
    _lerp_(exp_avg, grad, 1 - beta1)
    # Update the exponentially weighted infinity norm.
    exp_inf *= beta2
    np.maximum(exp_inf, np.abs(grad) + eps, out=exp_inf)
    bias_correction = 1 - beta1 ** st["step"]
    clr = lr / bias_correction
    param += -clr * exp_avg / exp_inf


STEP = {"radam": radam, "nadam": nadam, "adamax": adamax}
SECOND = {"radam": "exp_avg_sq", "nadam": "exp_avg_sq", "adamax": "exp_inf"}
TORCH = {"radam": "RAdam", "nadam": "NAdam", "adamax": "Adamax"}


def run(family, param, grads, hp, clip=1.0):
    """`len(grads)` steps from torch's initial state on a copy of `param` with the gradients grads[t] * clip: (param, state)."""
    p = np.array(param, F64)
    st = new_state(family, p)
    for g in grads:
        STEP[family](p, np.asarray(g, F64) * clip, st, **hp)
    return p, st
