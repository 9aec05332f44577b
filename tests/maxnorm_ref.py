"""Max-norm regularisation of the adapters in plain torch: kohya's LoRANetwork.apply_max_norm_regularization restated with the
rounding points of include/qfx.h (qfx_maxnorm_apply), plus a literal transcription of kohya's loop to pin the restatement against.
kohya's package is not a dependency.

Per pair, A = lora_A.weight [r, in], B = lora_B.weight [out, r], s = float32(lora_alpha / r), m = max_norm > 0:
    norm_raw    = float32(|s| * ||B A||_F)       the product and its norm in fp64, rounded once
    ratio       = m / norm_raw if norm_raw > m else 1                         one fp32 divide
    q           = sqrt(ratio)                                                 one fp32 square root
    A *= q, B *= q when ratio != 1                                            one fp32 multiply per element
    scaled_norm = norm_raw * ratio                                            one fp32 multiply
A pair whose norm_raw is not finite is left alone and reported with ratio 1 and that norm.  keys_scaled counts ratio != 1, the mean
is the fp64 sum of the scaled norms in pair order over n, rounded once, the maximum an fp32 maximum that keeps a NaN."""
import torch

F32, F64 = torch.float32, torch.float64


def f32(x):
    return torch.tensor(x, dtype=F32)


def norm_raw(A, B, scale):
    """float32(|s| ||B A||_F) from the direct product in fp64; s is taken as fp32."""
    prod = B.to(F64) @ A.to(F64)
    return (abs(float(f32(scale))) * prod.pow(2).sum().sqrt()).to(F32)


def gram_norm(A, B, scale, chunk=None):
    """The same number from the two r x r Gram matrices in fp64 (the kernel's identity); chunk: sum the Gram matrices over slices
    of that many columns / rows, another summation order."""
    a, b = A.to(F64), B.to(F64)
    if chunk is None:
        ga, gb = a @ a.T, b.T @ b
    else:
        ga = sum(a[:, k:k + chunk] @ a[:, k:k + chunk].T for k in range(0, a.shape[1], chunk))
        gb = sum(b[k:k + chunk].T @ b[k:k + chunk] for k in range(0, b.shape[0], chunk))
    return (abs(float(f32(scale))) * (ga * gb).sum().clamp(min=0).sqrt()).to(F32)


def decide(nr, max_norm):
    """(ratio, q) as fp32 scalars for one fp32 norm_raw."""
    m = f32(max_norm)
    if bool(torch.isfinite(nr)) and bool(nr > m):
        ratio = m / nr
        return ratio, torch.sqrt(ratio)
    return f32(1.0), f32(1.0)


def summarize(norms, ratios):
    """(keys_scaled, mean, max) of per-pair fp32 tensors, as the summary launch forms them."""
    keys = int((ratios != 1).sum())
    mean = (norms.to(F64).sum() / norms.numel()).to(F32) if not bool(torch.isnan(norms).any()) else f32(float("nan"))
    mx = f32(float("nan")) if bool(torch.isnan(norms).any()) else norms.max()
    return keys, mean, mx


def apply(pairs, max_norm):
    """pairs: list of (A, B, scale) fp32 CPU tensors, scaled IN PLACE.  Returns (keys_scaled, mean, max, norms, ratios, raw)."""
    norms, ratios, raw = [], [], []
    for A, B, scale in pairs:
        nr = norm_raw(A, B, scale)
        ratio, q = decide(nr, max_norm)
        if bool(ratio != 1):
            A.mul_(q)
            B.mul_(q)
        raw.append(nr)
        ratios.append(ratio)
        norms.append(nr * ratio)
    norms, ratios, raw = torch.stack(norms), torch.stack(ratios), torch.stack(raw)
    return summarize(norms, ratios) + (norms, ratios, raw)


def kohya_literal(pairs, max_norm):
    """kohya's loop, line for line (lora.py, apply_max_norm_regularization), with the product and its norm in fp64 and the norm
    then taken to fp32: updown = up @ down * scale; norm = updown.norm().clamp(min=max_norm / 2); desired = clamp(norm, max=max_norm);
    ratio = desired / norm; sqrt_ratio = ratio ** 0.5; if ratio != 1: up *= sqrt_ratio, down *= sqrt_ratio;
    scalednorm = updown.norm() * ratio.  Returns (keys_scaled, mean, max) as Python numbers."""
    norms, keys_scaled = [], 0
    for down, up, scale in pairs:
        updown = (up.to(F64) @ down.to(F64)) * float(f32(scale))
        full = updown.norm().to(F32)
        norm = full.clamp(min=max_norm / 2)
        desired = torch.clamp(norm, max=max_norm)
        ratio = desired / norm
        sqrt_ratio = ratio ** 0.5
        if ratio != 1:
            keys_scaled += 1
            up.mul_(sqrt_ratio)
            down.mul_(sqrt_ratio)
        norms.append((full * ratio).item())
    return keys_scaled, sum(norms) / len(norms), max(norms)


def ulps(a, b):
    """Largest distance in fp32 units in the last place between two fp32 tensors of non-negative values; NaN matches NaN only."""
    a, b = torch.as_tensor(a, dtype=F32).reshape(-1).cpu(), torch.as_tensor(b, dtype=F32).reshape(-1).cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return float("inf")
    d = (a.view(torch.int32).to(torch.int64) - b.view(torch.int32).to(torch.int64)).abs()
    d[na] = 0
    return int(d.max()) if d.numel() else 0


def same_bits(a, b):
    return torch.equal(a.detach().cpu().contiguous().view(torch.int32), b.detach().cpu().contiguous().view(torch.int32))
