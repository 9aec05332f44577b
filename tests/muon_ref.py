"""CPU restatement of qfx_muon_step = torch.optim.Muon's step (torch/optim/_muon.py) in plain torch, with the rounding points the
kernel documents (include/qfx.h) made explicit: the momentum and the parameter update in fp32, the Newton-Schulz iteration with every
operand rounded to bf16, every product accumulated in fp32 and every result rounded to bf16 once.  tests/test_muon_cpu.py holds it
against torch.optim.Muon itself; tests/test_muon_gpu.py holds the kernel against it.

The iteration is not bit-comparable between two fp32 accumulation orders (a sum that lands near a bf16 rounding boundary goes either
way), so the yardstick for O is the reference's OWN error: `ns_f64` runs the same iteration in float64 from the same normalised bf16
input with no intermediate rounding, and `rel_err` measures torch's, the restatement's and the kernel's distance from it."""
import math

import numpy as np
import torch

F32 = np.float32
BF = torch.bfloat16
COEFFS = (3.4445, -4.7750, 2.0315)
DEFAULTS = dict(lr=1e-3, weight_decay=0.1, momentum=0.95, nesterov=True, ns_coefficients=COEFFS, eps=1e-7, ns_steps=5, adjust_lr_fn=None)


def clip_coef(gnorm_sq, max_norm, grad_scale):
    """The prologue of the fused steps, in fp32: grad_scale * min(1, max_norm / (sqrt(gnorm_sq) * grad_scale + 1e-6))."""
    clip = F32(grad_scale)
    if gnorm_sq is not None and max_norm > 0:
        nrm = np.sqrt(F32(gnorm_sq)) * F32(grad_scale)
        c = F32(max_norm) / (nrm + F32(1e-6))
        clip = clip * (c if c < F32(1.0) else F32(1.0))
    return F32(clip)


def lr_ratio(adjust_lr_fn, rows, cols):
    """torch.optim._muon._adjust_lr's factor."""
    if adjust_lr_fn is None or adjust_lr_fn == "original":
        return math.sqrt(max(1, rows / cols))
    if adjust_lr_fn == "match_rms_adamw":
        return 0.2 * math.sqrt(max(rows, cols))
    raise ValueError(f"Adjust learning rate function {adjust_lr_fn} is not supported")


def normalise(u, eps):
    """fp32 update [rows, cols] -> the bf16 X [s, n] the iteration starts from (s = the short side)."""
    x = u.to(BF)
    if x.shape[0] > x.shape[1]:
        x = x.T
    xf = x.float()
    nrm = (xf * xf).sum().sqrt().to(BF)                               # the sum of squares in fp32, the norm rounded to bf16
    den = torch.maximum(nrm, torch.tensor(eps, dtype=torch.float32).to(BF))
    return (xf / den.float()).to(BF).contiguous()


def ns_bf16(x, coeffs=COEFFS, ns_steps=5):
    """The iteration from the normalised bf16 X: operands rounded to bf16, products in fp32, results rounded to bf16."""
    a, b, c = (float(v) for v in coeffs)
    for _ in range(ns_steps):
        xf = x.float()
        g = (xf @ xf.T).to(BF)
        gf = g.float()
        h = (b * gf + c * (gf @ gf)).to(BF)
        x = (a * xf + h.float() @ xf).to(BF)
    return x


def ns_f64(x, coeffs=COEFFS, ns_steps=5):
    """The same iteration in float64 from the same bf16 X, nothing rounded on the way."""
    a, b, c = (float(v) for v in coeffs)
    x = x.double()
    for _ in range(ns_steps):
        g = x @ x.T
        x = a * x + (b * g + c * (g @ g)) @ x
    return x


def untranspose(x, shape):
    return x.T if shape[0] > shape[1] else x


def rel_err(o, o64):
    """Relative Frobenius distance; 0 for an all-zero reference that is met exactly."""
    d = (o.double() - o64.double()).norm().item()
    n = o64.double().norm().item()
    return d / n if n > 0 else (0.0 if d == 0 else float("inf"))


def step(p, g, buf, clip=1.0, **kw):
    """One step of one matrix: (p, buf) after it, O [rows, cols] in bf16 and the normalised X; None for a skipped matrix (a non-finite
    clipped gradient).  p, g, buf: fp32 [rows, cols]; nothing is modified."""
    K = dict(DEFAULTS, **kw)
    gs = g * torch.tensor(float(clip), dtype=torch.float32)
    if not torch.isfinite(gs).all():
        return None
    mu = K["momentum"]
    buf = torch.lerp(buf, gs, 1 - mu)
    u = torch.lerp(gs, buf, mu) if K["nesterov"] else buf
    x0 = normalise(u, K["eps"])
    o = untranspose(ns_bf16(x0, K["ns_coefficients"], K["ns_steps"]), p.shape)
    alr = K["lr"] * lr_ratio(K["adjust_lr_fn"], *p.shape)
    pn = (p * (1 - K["lr"] * K["weight_decay"])).add(o.float(), alpha=-alr)       # torch: param.mul_(...); param.add_(update, alpha=...)
    return pn, buf, o, x0


def ulp_diff(a, b):
    """|a - b| in units of b's fp32 spacing, elementwise."""
    a, b = a.float(), b.float()
    exp = torch.floor(torch.log2(b.abs().clamp_min(2.0 ** -126)))
    return (a - b).abs() / torch.exp2(exp - 23)


def make_matrix(shape, seed, scale=1e-2, rank1=False):
    g = torch.Generator().manual_seed(seed)
    if rank1:
        return (torch.randn(shape[0], 1, generator=g) @ torch.randn(1, shape[1], generator=g)) * scale
    return torch.randn(shape, generator=g) * scale


def flat_offsets(shapes):
    """Offsets of the matrices in a flat buffer with 64-element padded slots, as the LoRA store packs them."""
    offs, n = [], 0
    for s in shapes:
        offs.append(n)
        n += (s[0] * s[1] + 63) // 64 * 64
    return offs, n
