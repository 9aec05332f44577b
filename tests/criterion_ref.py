"""Restatement of the general criterion (include/qfx.h, qfx_criterion_fwd_bwd) the criterion tests compare against, on the CPU:
an fp32 version that rounds where the kernel rounds (the gradient, for bit comparisons) and an fp64 version (for bounds)."""
import torch

KINDS = ("l2", "huber", "smooth_l1")
BF = torch.bfloat16


def _ones(t, shape, dtype):
    return torch.ones(shape, dtype=dtype) if t is None else t.detach().cpu().to(dtype).reshape(shape)


def dpred_f32(pred, target, S_t, sample_w=None, token_w=None, huber_c=None, kind="l2", inv_denom=None, gscale=1.0):
    """bf16 [B,S_all,C]: every fp32 operation of the kernel's gradient, one torch CPU op each (no fused multiply-add), the factors
    from left to right: rho'(d) * sample_w * token_w * (1/C) * inv_denom * gscale."""
    pred, target = pred.detach().cpu(), target.detach().cpu()
    B, S_all, C = pred.shape
    f = torch.float32
    d = pred[:, :S_t].to(f) - target.to(f)
    if kind == "l2":
        g = 2.0 * d
    else:
        c = _ones(huber_c, (B, 1, 1), f)
        r = torch.sqrt(d * d + c * c)
        g = ((2.0 * c) * d) / r if kind == "huber" else (2.0 * d) / r
    inv_denom = 1.0 / (B * S_t) if inv_denom is None else inv_denom
    g = g * _ones(sample_w, (B, 1, 1), f)
    g = g * _ones(token_w, (B, S_t, 1), f)
    g = g * (torch.ones((), dtype=f) / torch.tensor(float(C), dtype=f))
    g = g * torch.tensor(inv_denom, dtype=f)
    g = g * torch.tensor(gscale, dtype=f)
    out = torch.zeros(B, S_all, C, dtype=BF)
    out[:, :S_t] = g.to(BF)
    return out


def criterion_f64(pred, target, S_t, sample_w=None, token_w=None, huber_c=None, kind="l2", inv_denom=None, gscale=1.0):
    """(loss, loss_per_sample [B], dpred [B,S_all,C]) in fp64 from the formulas of the header; dpred is not rounded."""
    pred, target = pred.detach().cpu(), target.detach().cpu()
    B, S_all, C = pred.shape
    f = torch.float64
    d = pred[:, :S_t].to(f) - target.to(f)
    sw, tw = _ones(sample_w, (B,), f), _ones(token_w, (B, S_t), f)
    if kind == "l2":
        rho, drho = d * d, 2.0 * d
    else:
        c = _ones(huber_c, (B, 1, 1), f)
        r = torch.sqrt(d * d + c * c)
        q = d * d / (r + c)
        rho, drho = (2.0 * c * q, 2.0 * c * d / r) if kind == "huber" else (2.0 * q, 2.0 * d / r)
    inv_denom = 1.0 / (B * S_t) if inv_denom is None else float(torch.tensor(inv_denom, dtype=torch.float32))
    lps = B * inv_denom * (tw * rho.mean(dim=2)).sum(dim=1)
    loss = (sw * lps).mean()
    g = torch.zeros(B, S_all, C, dtype=f)
    g[:, :S_t] = drho * sw.reshape(B, 1, 1) * tw.reshape(B, S_t, 1) / C * inv_denom * float(torch.tensor(gscale, dtype=torch.float32))
    return loss, lps, g


def bf16_order(t):
    """bf16 tensor -> int32 keys that count representable values: adjacent bf16 numbers differ by 1, +0 and -0 share key 0."""
    i = t.detach().cpu().contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def bf16_steps(a, b):
    """Largest distance between two bf16 tensors, in representable values."""
    return int((bf16_order(a) - bf16_order(b)).abs().max())


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it))
