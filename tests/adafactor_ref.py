"""CPU restatement of the fused Adafactor step (include/qfx.h, qfx_adafactor_step; transformers.optimization.Adafactor's arithmetic):
every fp32 operation of the kernel is one torch operation here, in the kernel's order, on tensors of `dtype` -- float32 restates the
kernel up to the order of its sums and fused multiply-adds, float64 is the yardstick both are measured against.  The host scalars
(relative step or lr, beta2_t, 1 - beta2_t, 1 - beta1) are formed in double and then cast to `dtype`, as the launch rounds them.

The transformers package is not installed where this was written: parity with the package itself is pinned only by
test_adafactor_cpu.py::test_restatement_matches_transformers, which skips without it; what is pinned without it is the hand
derivation in the same file."""
import math

import torch

DEFAULTS = dict(eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, weight_decay=0.0, scale_parameter=True,
                relative_step=True, warmup_init=False, lr=None)


def new_state(shapes, beta1=None, dtype=torch.float32):
    """Zeroed per-tensor state, transformers' names."""
    out = []
    for s in shapes:
        s = tuple(s)
        e = {"RMS": torch.zeros((), dtype=dtype)}
        if len(s) >= 2:
            e["exp_avg_sq_row"], e["exp_avg_sq_col"] = torch.zeros(s[:-1], dtype=dtype), torch.zeros(s[:-2] + s[-1:], dtype=dtype)
        else:
            e["exp_avg_sq"] = torch.zeros(s, dtype=dtype)
        if beta1 is not None:
            e["exp_avg"] = torch.zeros(s, dtype=dtype)
        out.append(e)
    return out


def host_scalars(t, lr=None, decay_rate=-0.8, relative_step=True, warmup_init=False):
    if relative_step:
        lr = min(1e-6 * t if warmup_init else 1e-2, 1.0 / math.sqrt(t))
    beta2t = 1.0 - math.pow(t, decay_rate)
    return lr, beta2t, 1.0 - beta2t


def clip_coef(gnorm_sq, max_norm, grad_scale, dtype):
    """The prologue of the fused steps: grad_scale * min(1, max_norm / (sqrt(gnorm_sq) * grad_scale + 1e-6)); gnorm_sq None or
    max_norm <= 0: grad_scale."""
    T = lambda x: torch.tensor(x, dtype=dtype)
    clip = T(grad_scale)
    if gnorm_sq is not None and max_norm > 0:
        nrm = T(gnorm_sq).sqrt() * T(grad_scale)
        c = T(max_norm) / (nrm + T(1e-6))
        clip = clip * torch.minimum(c, T(1.0))
    return clip


def step(params, grads, state, t, dtype=torch.float32, gnorm_sq=None, max_norm=0.0, grad_scale=1.0, **opts):
    """One step t (from 1) in place over lists of tensors of `dtype` (2-D or fewer dimensions); state from new_state()."""
    o = dict(DEFAULTS, **opts)
    T = lambda x: torch.tensor(x, dtype=dtype)
    lr_h, b2, omb2 = host_scalars(t, o["lr"], o["decay_rate"], o["relative_step"], o["warmup_init"])
    clip = clip_coef(gnorm_sq, max_norm, grad_scale, dtype)
    for p, g, st in zip(params, grads, state):
        gp = g.to(dtype) * clip
        if not bool(torch.isfinite(gp).all()):
            continue                                  # the whole tensor is skipped: p and its state stay
        n = p.numel()
        rms = (p * p).sum().sqrt() / T(float(n)).sqrt()
        st["RMS"] = rms
        lr = T(lr_h)
        if o["scale_parameter"]:
            lr = lr * torch.maximum(T(o["eps"][1]), rms)
        u = gp * gp + T(o["eps"][0])
        if p.dim() >= 2:
            R, C = p.shape[-2], p.shape[-1]
            row = T(b2) * st["exp_avg_sq_row"] + T(omb2) * (u.sum(-1) / T(float(C)))
            col = T(b2) * st["exp_avg_sq_col"] + T(omb2) * (u.sum(-2) / T(float(R)))
            st["exp_avg_sq_row"], st["exp_avg_sq_col"] = row, col
            rmean = row.sum(-1, keepdim=True) / T(float(R))
            rf = T(1.0) / (row / rmean).sqrt()
            cf = T(1.0) / col.sqrt()
            upd = (rf.unsqueeze(-1) * cf.unsqueeze(-2)) * gp
        else:
            v = T(b2) * st["exp_avg_sq"] + T(omb2) * u
            st["exp_avg_sq"] = v
            upd = (T(1.0) / v.sqrt()) * gp
        urms = (upd * upd).sum().sqrt() / T(float(n)).sqrt()
        den = torch.maximum(T(1.0), urms / T(o["clip_threshold"]))
        upd = (upd / den) * lr
        if o["beta1"] is not None:
            upd = T(o["beta1"]) * st["exp_avg"] + T(1.0 - o["beta1"]) * upd
            st["exp_avg"] = upd
        if o["weight_decay"] != 0:
            p.add_(p * (-(T(o["weight_decay"]) * lr)))
        p.sub_(upd)
