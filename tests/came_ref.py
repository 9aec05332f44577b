"""CPU restatement of the fused CAME step (include/qfx.h, qfx_came_step; came_pytorch.CAME's arithmetic): every fp32 operation of the
kernel is one torch operation here, in the kernel's order, on tensors of `dtype` -- float32 restates the kernel up to the order of
its sums, float64 is the yardstick both are measured against.  The host scalars (1 - beta1, 1 - beta2, 1 - beta3) are formed in
double and then cast to `dtype`, as the launch rounds them.

The came_pytorch package is not installed where this was written: parity with the package itself is pinned only by
test_came_cpu.py::test_restatement_matches_came_pytorch, which skips without it; what is pinned without it is the hand derivation
in the same file."""
import torch

from adafactor_ref import clip_coef

DEFAULTS = dict(lr=None, eps=(1e-30, 1e-16), clip_threshold=1.0, betas=(0.9, 0.999, 0.9999), weight_decay=0.0)
FACTORED = ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_res_row", "exp_avg_res_col")


def new_state(shapes, dtype=torch.float32):
    """Zeroed per-tensor state, came_pytorch's names."""
    out = []
    for s in shapes:
        s = tuple(s)
        e = {"RMS": torch.zeros((), dtype=dtype), "exp_avg": torch.zeros(s, dtype=dtype)}
        if len(s) == 2:
            e["exp_avg_sq_row"], e["exp_avg_sq_col"] = torch.zeros(s[:1], dtype=dtype), torch.zeros(s[1:], dtype=dtype)
            e["exp_avg_res_row"], e["exp_avg_res_col"] = torch.zeros(s[:1], dtype=dtype), torch.zeros(s[1:], dtype=dtype)
        else:
            e["exp_avg_sq"] = torch.zeros(s, dtype=dtype)
        out.append(e)
    return out


def step(params, grads, state, dtype=torch.float32, gnorm_sq=None, max_norm=0.0, grad_scale=1.0, **opts):
    """One step in place over lists of tensors of `dtype` (1-D or 2-D); state from new_state().  The step count does not enter the
    arithmetic.  Returns the update-clip divisor max(1, rms(upd) / clip_threshold) of every tensor (None: skipped)."""
    o = dict(DEFAULTS, **opts)
    T = lambda x: torch.tensor(x, dtype=dtype)
    lr = T(float(o["lr"]))
    (b1, b2, b3), (eps1, eps2) = (float(b) for b in o["betas"]), o["eps"]
    clip = clip_coef(gnorm_sq, max_norm, grad_scale, dtype)

    def factors(row, col, R):
        rmean = row.sum(-1, keepdim=True) / T(float(R))
        return (T(1.0) / (row / rmean).sqrt()).unsqueeze(-1) * (T(1.0) / col.sqrt()).unsqueeze(-2)

    dens = []
    for p, g, st in zip(params, grads, state):
        gp = g.to(dtype) * clip
        if not bool(torch.isfinite(gp).all()):
            dens.append(None)
            continue                                  # the whole tensor is skipped: p and its state stay
        n = p.numel()
        st["RMS"] = (p * p).sum().sqrt() / T(float(n)).sqrt()
        u = gp * gp + T(eps1)
        if p.dim() == 2:
            R, C = p.shape
            row = T(b2) * st["exp_avg_sq_row"] + T(1.0 - b2) * (u.sum(-1) / T(float(C)))
            col = T(b2) * st["exp_avg_sq_col"] + T(1.0 - b2) * (u.sum(-2) / T(float(R)))
            st["exp_avg_sq_row"], st["exp_avg_sq_col"] = row, col
            upd = factors(row, col, R) * gp
        else:
            v = T(b2) * st["exp_avg_sq"] + T(1.0 - b2) * u
            st["exp_avg_sq"] = v
            upd = (T(1.0) / v.sqrt()) * gp
        urms = (upd * upd).sum().sqrt() / T(float(n)).sqrt()
        den = torch.maximum(T(1.0), urms / T(o["clip_threshold"]))
        dens.append(float(den))
        upd = upd / den
        m = T(b1) * st["exp_avg"] + T(1.0 - b1) * upd
        st["exp_avg"] = m
        if p.dim() == 2:
            d = upd - m
            res = d * d + T(eps2)
            rrow = T(b3) * st["exp_avg_res_row"] + T(1.0 - b3) * (res.sum(-1) / T(float(C)))
            rcol = T(b3) * st["exp_avg_res_col"] + T(1.0 - b3) * (res.sum(-2) / T(float(R)))
            st["exp_avg_res_row"], st["exp_avg_res_col"] = rrow, rcol
            out = factors(rrow, rcol, R) * m
        else:
            out = m
        if o["weight_decay"] != 0:
            p.add_(p * (-(T(o["weight_decay"]) * lr)))
        p.sub_(lr * out)
    return dens
