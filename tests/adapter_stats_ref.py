"""Restatement of qfx_adapter_stats (include/qfx.h) in numpy: the fp64 version is the truth, the fp32 version adds in the kernel's
order and states that order as a specification.

Per table entry (off, numel) over the flat buffers p, g, prev:
  phase 0   g' = float32(g * clip);  grad_sq = sum g'^2, grad_absmax = max |g'|, grad_nonfinite = #(g' not finite);  prev = p
  phase 1   weight_sq = sum p^2, weight_nonfinite = #(p not finite), update_sq = sum (p - prev)^2
A non-finite element (g'; p; p - prev) adds nothing to its sum and is passed over by the maximum.

The truth takes the fp32 values the kernel is given -- g' as the rounded fp32 product (its rounding is not the sum's), p, prev --
widens them and does the rest in fp64: squares, sums and the difference p - prev.

The kernel's order (ordered_sumsq): lane L of 256 adds the squares of the elements i = L (mod 256) in index order, one fp32
multiply and one fp32 add each; the 64 lanes of each of the four waves are folded by an xor-shuffle tree, offsets 32, 16, ..., 1
(every lane adds its partner's value to its own); the four wave sums are added as (w0 + w1) + (w2 + w3).

bound(): every term is non-negative, so each passes through at most ceil(numel / 256) + 11 fp32 additions (the lane chain, six
shuffle levels, the fold of four waves) and one rounded square:  |sum - sum64| <= (ceil(numel / 256) + 12) 2^-24 sum64; the
update's difference is rounded before it is squared, which adds 2 to the factor.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
LANES, WAVE = 256, 64


def clip_factor(gnorm_sq, max_norm, grad_scale):
    """opt_clip (csrc/qfx_optim.h) in fp32, operation by operation: grad_scale * min(1, max_norm / (sqrt(gnorm_sq) grad_scale + 1e-6)),
    grad_scale alone without a norm or with max_norm <= 0."""
    clip = F32(grad_scale)
    if gnorm_sq is not None and max_norm > 0:
        nrm = F32(np.sqrt(F32(gnorm_sq)) * F32(grad_scale))
        c = F32(F32(max_norm) / F32(nrm + F32(1e-6)))
        clip = F32(clip * (c if c < F32(1.0) else F32(1.0)))
    return clip


def clipped(g, clip):
    """g' = g * clip, one fp32 multiply per element."""
    with np.errstate(all="ignore"):
        return (np.asarray(g, F32) * F32(clip)).astype(F32)


def _finite_or_zero(x):
    return np.where(np.isfinite(x), x, x.dtype.type(0))


def ordered_sumsq(x):
    """The kernel's sum of squares of the fp32 vector x (non-finite elements count as 0), bit for bit."""
    x = _finite_or_zero(np.asarray(x, F32))
    n = x.size
    rows = -(-n // LANES)
    pad = np.zeros(max(rows, 1) * LANES, F32)
    pad[:n] = x                                     # a lane without an element at some index adds nothing: +0 changes no bit
    acc = np.zeros(LANES, F32)
    with np.errstate(over="ignore"):
        for r in pad.reshape(-1, LANES):            # index order down every lane's chain
            acc = (acc + (r * r).astype(F32)).astype(F32)
        w = acc.reshape(4, WAVE).copy()
        lane = np.arange(WAVE)
        for o in (32, 16, 8, 4, 2, 1):
            w = (w + w[:, lane ^ o]).astype(F32)
        ws = w[:, 0]
        return F32(F32(ws[0] + ws[1]) + F32(ws[2] + ws[3]))


def sumsq64(x):
    """fp64 sum of squares of the finite elements of x (x widened first)."""
    x = _finite_or_zero(np.asarray(x).astype(F64))
    return float(np.sum(x * x))


def bound(numel, sum64, update=False):
    return (math.ceil(numel / LANES) + 12 + (2 if update else 0)) * 2.0 ** -24 * sum64


def phase0(g, off, numel, clip, ordered=False):
    """-> dict(grad_sq, grad_absmax, grad_nonfinite) of one entry; zeros for an entry the kernel skips."""
    if numel <= 0 or off < 0:
        return dict(grad_sq=0.0, grad_absmax=0.0, grad_nonfinite=0)
    gc = clipped(g[off:off + numel], clip)
    ok = np.isfinite(gc)
    return dict(grad_sq=float(ordered_sumsq(gc)) if ordered else sumsq64(gc),
                grad_absmax=float(np.abs(gc[ok]).max()) if ok.any() else 0.0, grad_nonfinite=int((~ok).sum()))


def phase1(p, prev, off, numel, ordered=False):
    """-> dict(weight_sq, update_sq, weight_nonfinite) of one entry."""
    if numel <= 0 or off < 0:
        return dict(weight_sq=0.0, update_sq=0.0, weight_nonfinite=0)
    a, b = np.asarray(p[off:off + numel], F32), np.asarray(prev[off:off + numel], F32)
    with np.errstate(all="ignore"):
        if ordered:
            w, u = float(ordered_sumsq(a)), float(ordered_sumsq((a - b).astype(F32)))
        else:
            w, u = sumsq64(a), sumsq64(a.astype(F64) - b.astype(F64))
    return dict(weight_sq=w, update_sq=u, weight_nonfinite=int((~np.isfinite(a)).sum()))


def make_tensor(numel, seed, scale=1.0):
    """Deterministic fp32 test data with a spread of magnitudes (so that the order of a sum shows in its last bits)."""
    rng = np.random.default_rng(1000 + seed)
    return (rng.standard_normal(numel) * np.exp(rng.uniform(-3.0, 3.0, numel)) * scale).astype(F32)
