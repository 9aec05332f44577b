"""CPU restatement (torch only) of the row kernels of csrc/qfx_elem.hip and of the conditioning-head kernels of csrc/qfx_cond.hip,
the yardstick of tests/test_rowkernel_gpu.py.  Every function applies the bf16 rounding points the kernel comments and include/qfx.h
state (`q` below) and returns, per output, the pair

    (value, scale)      scale: same shape, the largest magnitude among the intermediates rounded to bf16 on that element's path.

One flipped rounding of an intermediate moves an output by one bf16 ulp OF THAT INTERMEDIATE, so errors are counted in bf16 ulps
of `scale` (err_ulps).  Arguments shared by all restatements:

    dt    torch.float64 (the reference) or torch.float32 (the same arithmetic in the kernels' precision),
    flip  reductions run over the reversed axis (a second summation order),
    rnd   False switches every rounding point off (the plain formula, for the autograd checks of tests/test_rowkernel_ref_cpu.py).

fp32 + flip against fp64 is the reference's OWN noise: tests/test_rowkernel_ref_cpu.py measures it on the case lists below (the
ones the GPU tests run) and asserts 2 x floor <= BARS[output]; the bars are never taken from what the kernels give.

exact_case data: integers in [-2, 2] and integers in [-2, 2] times 2^-4 (2^-2 for the adapter scales of the conditioning head),
so that every partial sum of the contractions named by the EXACT_MAX_* constants is exactly representable in fp32 and an fp32
kernel must give the fp64 sum bit for bit whatever the order of its atomics."""
from __future__ import annotations

import torch

from skinny_ref import BF, CANARY_BF16, CANARY_F32, bits, canary_bf16, canary_f32   # noqa: F401  (re-exported)

F64, F32 = torch.float64, torch.float32
EPS = 1e-6

# ---------------------------------------------------------------------------------------------- exactness premise of exact_case
# the longest contractions the GPU tests may run on exact_case data; tests/test_rowkernel_ref_cpu.py proves the premise at these
# lengths (worst-case magnitude x granularity < 2^24, and fp32 sums in three orders), tests/test_rowkernel_gpu.py asserts them
EXACT_MAX_ROWS = 64          # mod_grad: rows of one sample (terms |.| <= 4, multiples of 2^-4)
EXACT_MAX_GEMV_K = 4096      # mod_gemv: K (terms <= 4 * 2^-4-multiples, plus a bias <= 2)
EXACT_MAX_GEMV_T = 3 * 130   # mod_gemv_t: nmat * N (terms <= 4, multiples of 2^-4, plus an initial fill <= 2)
EXACT_MAX_COND = dict(B=8, r=64, K=3072, N=1000, na=3)      # conditioning head, adapter scales in {0.25, 0.5, 1}

# ---------------------------------------------------------------------------------------------- bars, in bf16 ulps of `scale`
# BARS[output] = 2 x the floor measured by tests/test_rowkernel_ref_cpu.py::test_bars_are_twice_the_reference_noise (fp32 sums in
# reversed order against fp64, on the case lists of this file, FLOOR_DRAWS draws of each), rounded up to the next whole ulp.  The
# measured floor stands in the comment.  The smallest bar is one ulp: every output here ends in a rounding (bf16, or fp32 for the
# sums), a value within fp32 noise of a tie rounds either way, and a floor of 0 only says that no draw met such a value.
BARS = {
    "ln_fwd.y": 2,              # floor 1.00
    "ln_bwd.dx": 2,             # floor 1.00
    "ln_bwd.dyg": 4,            # floor 2.00   (a flipped dx times a gate just below a power of two)
    "mod_grad.dshift": 1,       # floor 3.8e-5   (an fp32 sum of bf16 values: no rounded intermediate, order noise only)
    "mod_grad.dscale": 2,       # floor 0.79
    "mod_grad.dgate": 1,        # floor 9.2e-5
    "rmsnorm.y": 2,             # floor 1.00
    "mod_gemv.out": 1,          # floor 0.031
    "mod_gemv_t.out": 1,        # floor 7.4e-5
    "qk_fwd.out": 1,            # floor 0.0078
    "qk_bwd.out": 2,            # floor 1.00
    "mse.loss": 1,              # floor 2.5e-5
    "mse.dpred": 2,             # floor 1.00
    "mse_tw.loss": 1,           # floor 2.0e-5
    "mse_tw.dpred": 1,          # floor 0   (no flip observed: the minimum)
    "flowmatch.packed": 1,      # floor 0
    "flowmatch.target": 1,      # floor 0   (bit-equal on exact_case data)
    "timestep.out": 1,          # floor 0.50
    "silu_bwd.dx": 1,           # floor 0
    "cond.u": 1,                # floor 5.3e-4
    "cond.y": 2,                # floor 1.00
    "cond.dA": 1,               # floor 6.6e-4
    "cond.dB": 1,               # floor 1.6e-4
    "cond.du": 1,               # floor 5.3e-4
    "cond.dx": 1,               # floor 7.8e-5
}


def q_bf16(t):
    """Round to bf16 (nearest even), stay in the working dtype."""
    return t.float().to(BF).to(t.dtype)


def _q(rnd):
    return q_bf16 if rnd else (lambda t: t)


def ulp_bf16(s):
    """Spacing of bf16 at magnitude |s| (fp64): 2^(floor(log2 |s|) - 7); zero counts as the smallest normal."""
    _, e = torch.frexp(s.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(s, dtype=F64), e - 8)


def err_ulps(got, ref, scale):
    """Worst |got - ref| in bf16 ulps of scale.  A non-finite `got` (an unwritten canary) is infinitely wrong."""
    g = got.double()
    if not torch.isfinite(g).all():
        return float("inf")
    return ((g - ref.double()).abs() / ulp_bf16(scale)).max().item() if g.numel() else 0.0


def _amax(*ts):
    out = ts[0].abs()
    for t in ts[1:]:
        out = torch.maximum(out, t.abs())
    return out.double()


def rsum(t, dim, flip=False, keepdim=False):
    return (t.flip(dim) if flip else t).sum(dim, keepdim=keepdim)


def _eps(eps, dt):
    return torch.tensor(eps, dtype=F32).to(dt)          # the kernels take eps as a float


def _f32c(v, dt):
    return torch.tensor(v, dtype=F32).to(dt)


def _stats(X, eps, dt, flip):
    D = X.shape[-1]
    mean = rsum(X, -1, flip, True) / D
    d = X - mean
    rstd = torch.rsqrt(rsum(d * d, -1, flip, True) / D + _eps(eps, dt))
    return d, rstd


# ---------------------------------------------------------------------------------------------- LayerNorm + modulate
def ln_fwd(x, shift, scale, rpb, eps=EPS, dt=F64, flip=False, rnd=True):
    """x [rows, D]; shift, scale [B or 1, D] (row 0 for every sample when there is one row: mod_bstride = 0)."""
    q = _q(rnd)
    d, rstd = _stats(x.to(dt), eps, dt, flip)
    b = torch.arange(x.shape[0]) // rpb if shift.shape[0] > 1 else torch.zeros(x.shape[0], dtype=torch.int64)
    ln = q(d * rstd)
    t1 = q(1.0 + scale.to(dt)[b])
    p = q(ln * t1)
    y = q(p + shift.to(dt)[b])
    return {"y": (y, _amax(ln, t1, p, y))}


def ln_bwd(dy, x, scale, rpb, dres=None, gate=None, mask=None, eps=EPS, dt=F64, flip=False, rnd=True):
    """dx = bf16(dres + bf16(LN_bwd(g))), g = bf16(dy * bf16(1 + scale)); dyg = bf16(gate * dx); masked rows exact zeros."""
    q = _q(rnd)
    D = x.shape[1]
    d, rstd = _stats(x.to(dt), eps, dt, flip)
    bs = torch.arange(x.shape[0]) // rpb
    b = bs if scale.shape[0] > 1 else torch.zeros_like(bs)
    xh = d * rstd
    g = q(dy.to(dt) * q(1.0 + scale.to(dt)[b]))
    c1 = rsum(g, 1, flip, True) / D
    c2 = rsum(g * xh, 1, flip, True) / D
    dd = q((g - c1 - xh * c2) * rstd)
    dx = q(dres.to(dt) + dd) if dres is not None else dd
    sc = _amax(g, dd, dx)
    keep = torch.ones(x.shape[0], 1, dtype=dt) if mask is None else (mask != 0).to(dt)[:, None]
    dx = dx * keep
    out = {"dx": (dx, sc)}
    if gate is not None:
        gt = gate.to(dt)[bs if gate.shape[0] > 1 else torch.zeros_like(bs)]
        dyg = q(gt * dx)
        out["dyg"] = (dyg, torch.maximum(dyg.abs().double(), gt.abs().double() * sc))
    return out


def mod_grad(dy, x, rpb, dxo=None, y=None, mask=None, eps=EPS, dt=F64, flip=False, rnd=True):
    """Per sample b (rows b*rpb .. of the [rows, D] operands, the last sample may be short):
    dshift = sum dy, dscale = sum dy * bf16(LN(x)), dgate = sum dxo * y; rows with mask 0 drop out.  Values [B, D]."""
    q = _q(rnd)
    rows = x.shape[0]
    d, rstd = _stats(x.to(dt), eps, dt, flip)
    ln = q(d * rstd)
    keep = torch.ones(rows, 1, dtype=dt) if mask is None else (mask != 0).to(dt)[:, None]
    terms = {"dshift": dy.to(dt) * keep, "dscale": dy.to(dt) * ln * keep}
    if dxo is not None:
        terms["dgate"] = dxo.to(dt) * y.to(dt) * keep
    B = (rows + rpb - 1) // rpb
    out = {}
    for k, t in terms.items():
        val = torch.stack([rsum(t[b * rpb:min((b + 1) * rpb, rows)], 0, flip) for b in range(B)])
        sc = torch.stack([t[b * rpb:min((b + 1) * rpb, rows)].abs().amax(0) for b in range(B)])
        out[k] = (val, sc.double())
    return out


def rmsnorm(x, w, eps=EPS, dt=F64, flip=False, rnd=True):
    q = _q(rnd)
    X = x.to(dt)
    rstd = torch.rsqrt(rsum(X * X, 1, flip, True) / X.shape[1] + _eps(eps, dt))
    xn = q(X * rstd)
    y = q(xn * w.to(dt))
    return {"y": (y, _amax(xn, y))}


# ---------------------------------------------------------------------------------------------- modulation GEMV and its transpose
def silu(t):
    return t / (1.0 + torch.exp(-t))


def mod_gemv(temb, Ws, biases, apply_silu, dt=F64, flip=False, rnd=True):
    """out[mat, b, n] = bf16(sum_k act(temb)[b, k] W_mat[n, k] + bias_mat[n]), act = bf16(silu(.)) or identity."""
    q = _q(rnd)
    t = temb.to(dt)
    act = q(silu(t)) if apply_silu else t
    vals, scs = [], []
    for i, W in enumerate(Ws):
        prod = act[:, None, :] * W.to(dt)[None]                  # [B, N, K]
        acc = rsum(prod, 2, flip)
        if biases is not None:
            acc = acc + biases[i].to(dt)[None]
        o = q(acc)
        vals.append(o)
        scs.append(torch.maximum(o.abs().double(), prod.abs().amax(2).double()))
    return {"out": (torch.stack(vals), torch.stack(scs))}


def mod_gemv_t(dy, Ws, out0, dt=F64, flip=False):
    """out[b, k] = out0[b, k] + sum_mat sum_n dy[mat, b, n] W_mat[n, k]   (fp32 in the kernel, no rounding point)."""
    g = dy.to(dt)
    acc = torch.zeros(dy.shape[1], Ws[0].shape[1], dtype=dt)
    sc = torch.zeros(dy.shape[1], Ws[0].shape[1], dtype=F64)
    order = range(len(Ws) - 1, -1, -1) if flip else range(len(Ws))
    for i in order:
        prod = g[i][:, :, None] * Ws[i].to(dt)[None]              # [B, N, K]
        acc = acc + rsum(prod, 1, flip)
        sc = torch.maximum(sc, prod.abs().amax(1).double())
    return {"out": (out0.to(dt) + acc, torch.maximum(sc, out0.abs().double()))}


# ---------------------------------------------------------------------------------------------- QK RMSNorm + RoPE
def _qk_w(ws, S, T, dt):
    """[S, 2, 1, dh]: (wq, wk) of the text rows s < T, of the image rows beyond.  ws = (wq_txt, wk_txt, wq_img, wk_img)."""
    txt = torch.stack([ws[0], ws[1]]).to(dt)
    img = torch.stack([ws[2], ws[3]]).to(dt)
    sel = (torch.arange(S) < T)[:, None, None]
    return torch.where(sel, txt[None], img[None])[:, :, None, :]


def _qk_view(qkv, H, dh):
    B, S = qkv.shape[:2]
    return qkv[..., :2 * H * dh].reshape(B, S, 2, H, dh)


def _pair_scale(*ts):
    m = _amax(*ts)
    m = torch.maximum(m[..., 0::2], m[..., 1::2])
    return torch.stack([m, m], -1).flatten(-2)


def qk_fwd(qkv, rope, ws, T, H, dh, flags=0, eps=EPS, dt=F64, flip=False, rnd=True):
    """qkv [B, S, 3 H dh]; rope [1 or B, S, dh/2, 2] fp32 (cos, sin).  Returns the q|k sections [B, S, 2, H, dh]."""
    q = _q(rnd)
    x = _qk_view(qkv, H, dh).to(dt)
    S = x.shape[1]
    rstd = torch.rsqrt(rsum(x * x, -1, flip, True) / dh + _eps(eps, dt))
    w = _qk_w(ws, S, T, dt)
    if flags & 1:
        xn = x * rstd
        t = q(xn * w)
        mids = (t,)
    else:
        xn = q(x * rstd)
        t = q(xn * w)
        mids = (xn, t)
    c, sn = rope.to(dt)[:, :, None, None, :, 0], rope.to(dt)[:, :, None, None, :, 1]
    t0, t1 = t[..., 0::2], t[..., 1::2]
    o = q(torch.stack([t0 * c - t1 * sn, t0 * sn + t1 * c], -1).flatten(-2))
    return {"out": (o, _pair_scale(*mids, o))}


def qk_bwd(dqkv, saved, rope, ws, T, H, dh, flags=0, eps=EPS, dt=F64, flip=False, rnd=True):
    """dqkv [B, S, 3 H dh] (gradient of the rotated q, k), saved [B, S, 2 H dh] the pre-norm q, k -> d(pre-norm) [B, S, 2, H, dh]."""
    q = _q(rnd)
    dy = _qk_view(dqkv, H, dh).to(dt)
    x = _qk_view(saved, H, dh).to(dt)
    S = x.shape[1]
    rstd = torch.rsqrt(rsum(x * x, -1, flip, True) / dh + _eps(eps, dt))
    w = _qk_w(ws, S, T, dt)
    c, sn = rope.to(dt)[:, :, None, None, :, 0], rope.to(dt)[:, :, None, None, :, 1]
    y0, y1 = dy[..., 0::2], dy[..., 1::2]
    d = q(torch.stack([y0 * c + y1 * sn, -y0 * sn + y1 * c], -1).flatten(-2))      # dy * conj(f)
    dn = d * w if (flags & 1) else q(d * w)
    xh = x * rstd
    dot = rsum(dn * xh, -1, flip, True) / dh
    o = q((dn - xh * dot) * rstd)
    return {"out": (o, torch.maximum(_pair_scale(d), _amax(dn, o)))}


# ---------------------------------------------------------------------------------------------- criterion, flow-match, small ones
def _inv(dt, *factors):
    v = torch.tensor(1.0, dtype=F32)
    p = torch.tensor(float(factors[0]), dtype=F32)
    for f in factors[1:]:
        p = p * torch.tensor(float(f), dtype=F32)
    return (v / p).to(dt)


def mse(pred, target, S_t, gscale, dt=F64, flip=False, rnd=True):
    """pred [B, S_all, C], target [B, S_t, C]: loss = mean (pred - target)^2 over the rows s < S_t, dpred = bf16(2 d inv gscale)."""
    q = _q(rnd)
    B, S_all, Cc = pred.shape
    inv = _inv(dt, B, S_t, Cc) if rnd else 1.0 / (B * S_t * Cc)
    d = pred.to(dt)[:, :S_t] - target.to(dt)
    loss = rsum((d * d).flatten(), 0, flip) * inv
    g = torch.zeros(B, S_all, Cc, dtype=dt)
    g[:, :S_t] = q(2.0 * d * inv * _f32c(gscale, dt))
    return {"loss": (loss, loss.abs().double()), "dpred": (g, g.abs().double())}


def mse_tw(pred, target, tw, S_t, inv_denom, gscale, dt=F64, flip=False, rnd=True):
    """loss = sum_{b,s} tw[b,s] mean_c d^2 * inv_denom; dpred = bf16(2 tw d / C inv_denom gscale)."""
    q = _q(rnd)
    B, S_all, Cc = pred.shape
    invc = _inv(dt, Cc) if rnd else 1.0 / Cc
    idn = _f32c(inv_denom, dt)
    d = pred.to(dt)[:, :S_t] - target.to(dt)
    w = tw.to(dt)[:, :, None]
    loss = rsum((w * d * d * invc).flatten(), 0, flip) * idn
    g = torch.zeros(B, S_all, Cc, dtype=dt)
    g[:, :S_t] = q(2.0 * w * d * invc * idn * _f32c(gscale, dt))
    return {"loss": (loss, loss.abs().double()), "dpred": (g, g.abs().double())}


def flowmatch(x0, noise, ctrl, sigma, mode, dt=F64):
    """x0 [B, S_t, C] bf16 (mode 0) or fp16 (mode 1), noise bf16, ctrl [B, S_c, C] or None, sigma [B] bf16."""
    q = q_bf16
    sg = sigma.to(dt)[:, None, None]
    n, a = noise.to(dt), x0.to(dt)
    if mode == 0:
        m1, m2 = q(q(1.0 - sg) * a), q(sg * n)
        xt = q(m1 + m2)
        tgt = q(n - a)
    else:
        m1, m2 = q(1.0 - sg) * a, q(sg * n)
        xt = q(m1 + m2)
        tgt = q(n - q(a))
    sc = _amax(m1, m2, xt)
    if ctrl is not None and ctrl.shape[1]:
        xt = torch.cat([xt, ctrl.to(dt)], 1)
        sc = torch.cat([sc, ctrl.abs().double()], 1)
    return {"packed": (xt, sc), "target": (tgt, tgt.abs().double())}


def add3(a, b, c=None, dt=F64):
    v = q_bf16(a.to(dt) + b.to(dt))
    if c is not None:
        v = q_bf16(v + c.to(dt))
    return {"out": (v, v.abs().double())}


def timestep_embed(t, dim, scale, pre_scale, dt=F64):
    """out[b] = bf16([cos | sin](scale * (tv * f_j))), tv = bf16(t) or bf16(bf16(t) * pre_scale), f_j = exp(-ln(1e4) j / (dim/2))."""
    half = dim // 2
    tv = q_bf16(t.to(dt))
    if pre_scale != 1.0:
        tv = q_bf16(tv * _f32c(pre_scale, dt))
    f = torch.exp(_f32c(-9.210340371976184, dt) * torch.arange(half, dtype=dt) / half)
    e = _f32c(scale, dt) * (tv[:, None] * f[None])
    o = q_bf16(torch.cat([torch.cos(e), torch.sin(e)], 1))
    return {"out": (o, torch.ones_like(o, dtype=F64))}        # the amplitude of cos / sin: the last rounding happens below 1


def silu_bwd(ds, x, dt=F64, rnd=True):
    """dx = bf16(bf16(ds) * silu'(x)), silu'(x) = s (1 + x (1 - s)), s = sigmoid(x)."""
    q = _q(rnd)
    t = x.to(dt)
    s = 1.0 / (1.0 + torch.exp(-t))
    dsb = q(ds.to(dt))
    o = q(dsb * (s * (1.0 + t * (1.0 - s))))
    return {"dx": (o, _amax(dsb, o))}


# ---------------------------------------------------------------------------------------------- conditioning head (qfx_cond.hip)
def cond_act(x, apply_silu, dt=F64, rnd=True):
    t = x.to(dt)
    return _q(rnd)(silu(t)) if apply_silu else t


def cond_fwd(x, A, Bm, s, y0, apply_silu, dt=F64, flip=False, rnd=True):
    """x [B, K] bf16; A [na, r, K], Bm [na, N, r], s [na] fp32; y0 [na, B, N] bf16 (the base outputs).
    u = A act(x) (stored fp32), y = bf16(y0 + s * (Bm u))."""
    q = _q(rnd)
    act = cond_act(x, apply_silu, dt, rnd)
    pu = act[None, :, None, :] * A.to(dt)[:, None]                      # [na, B, r, K]
    u = rsum(pu, 3, flip)
    if dt == F32 or not rnd:
        us = u
    else:
        us = u.float().to(dt)                                          # the kernel hands u over as fp32
    su = torch.maximum(pu.abs().amax(3), u.abs()).double()
    py = Bm.to(dt)[:, None] * us[:, :, None, :]                         # [na, B, N, r]
    lo = rsum(py, 3, flip) * s.to(dt)[:, None, None]
    y = q(y0.to(dt) + lo)
    sy = torch.maximum(_amax(y, y0.to(dt), lo), (py.abs().amax(3) * s.to(dt).abs()[:, None, None]).double())
    return {"u": (u, su), "y": (y, sy)}


def cond_bwd(x, A, Bm, s, u, g, apply_silu, dA0, dB0, du0, dx0, dt=F64, flip=False, rnd=True):
    """g [na, B, N] bf16, u [na, B, r] (what the forward left); the four outputs accumulate onto dA0 [na, r, K], dB0 [na, N, r],
    du0 [na, B, r] (the caller's zeroed scratch in the library's use) and dx0 [B, K] or None:
    ga = s g;  dB += ga^T u;  du += ga Bm;  dA += du^T act(x);  dx += sum_a du A."""
    act = cond_act(x, apply_silu, dt, rnd)
    ga = g.to(dt) * s.to(dt)[:, None, None]
    U = u.to(dt)
    pB = ga[:, :, :, None] * U[:, :, None, :]                           # [na, B, N, r]
    dB = dB0.to(dt) + rsum(pB, 1, flip)
    pu = ga[:, :, :, None] * Bm.to(dt)[:, None]                         # [na, B, N, r]
    du = du0.to(dt) + rsum(pu, 2, flip)
    pA = du[:, :, :, None] * act[None, :, None, :]                      # [na, B, r, K]
    dA = dA0.to(dt) + rsum(pA, 1, flip)
    out = {"dB": (dB, torch.maximum(pB.abs().amax(1), dB0.abs().to(dt)).double()),
           "du": (du, torch.maximum(pu.abs().amax(2), du0.abs().to(dt)).double()),
           "dA": (dA, torch.maximum(pA.abs().amax(1), dA0.abs().to(dt)).double())}
    if dx0 is not None:
        px = du[:, :, :, None] * A.to(dt)[:, None]                      # [na, B, r, K]
        acc = rsum(rsum(px, 2, flip), 0, flip)
        out["dx"] = (dx0.to(dt) + acc, torch.maximum(px.abs().amax(2).amax(0), dx0.abs().to(dt)).double())
    return out


# ---------------------------------------------------------------------------------------------- whole-buffer images
def flat_image(val, numel, dtype=BF):
    """A flat output buffer of `numel` elements: `val` (row-major) in front, the canary behind."""
    img = canary_bf16(numel) if dtype == BF else canary_f32(numel)
    v = val.to(dtype).contiguous().flatten()
    assert v.numel() <= numel
    img[:v.numel()] = v
    return img


def strided_image(val, rows, ld, dtype=BF, fill=None):
    """[rows, ld] buffer holding val [r, c] in its top-left corner; `fill` (a finite value) or the canary elsewhere."""
    if fill is None:
        img = canary_bf16(rows, ld) if dtype == BF else canary_f32(rows, ld)
    else:
        img = torch.full((rows, ld), fill, dtype=dtype)
    assert val.shape[0] <= rows and val.shape[1] <= ld
    img[:val.shape[0], :val.shape[1]] = val.to(dtype)
    return img


def transpose_heads_image(x, S, S_pad, HD, rows_extra=3):
    """x [B, S, >= HD] -> [B * HD + rows_extra, S_pad]: x^T per sample, zeros in the pad columns, canary rows behind."""
    B = x.shape[0]
    img = canary_bf16(B * HD + rows_extra, S_pad)
    body = torch.zeros(B, HD, S_pad, dtype=BF)
    body[:, :, :S] = x[:, :, :HD].transpose(1, 2)
    img[:B * HD] = body.reshape(B * HD, S_pad)
    return img


# ---------------------------------------------------------------------------------------------- data
_DRAW = [0]          # which independent draw of every case's data: 0 in the GPU tests, 0 .. n-1 when the noise floors are measured


def _gen(seed):
    return torch.Generator().manual_seed(seed + 100003 * _DRAW[0])


def randn_bf(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def ints(g, *shape, scale=1.0, dtype=BF):
    return (torch.randint(-2, 3, shape, generator=g).float() * scale).to(dtype)


def rand_case(seed, **shapes):
    """Gaussian bf16 tensors, one per keyword (value: shape, or (shape, scale))."""
    g = _gen(seed)
    out = {}
    for k, v in shapes.items():
        shape, sc = (v if isinstance(v[0], (tuple, list)) else (v, 1.0))
        out[k] = randn_bf(g, *shape, scale=sc)
    return out


def exact_case(seed, **shapes):
    """Integers in [-2, 2] per keyword (value: shape, or (shape, scale) with scale a power of two, 2^-4 for second factors)."""
    g = _gen(seed)
    out = {}
    for k, v in shapes.items():
        shape, sc = (v if isinstance(v[0], (tuple, list)) else (v, 1.0))
        out[k] = ints(g, *shape, scale=sc)
    return out


def case_data(kind, seed, **shapes):
    return (exact_case if kind == "exact" else rand_case)(seed, **shapes)


# ---------------------------------------------------------------------------------------------- the case lists of the GPU tests
def roundup(a, b):
    return (a + b - 1) // b * b


RPB = 3                                              # rows per sample of the LayerNorm cases: samples change inside a 4-row block
LN_D = (8, 264, 512, 520, 1536, 3072, 3080, 3584, 4096)
LN_ROWS = (1, 4, 5, 7)
LN_STRIDES = ("shared", "tight", "six")             # mod_bstride 0, D, 6 D
# (D, rows, stride): every D with two row counts, every row count and stride with small and large D
LN_FWD_CASES = [(D, LN_ROWS[(i + j) % 4], LN_STRIDES[(i + 2 * j) % 3]) for i, D in enumerate(LN_D) for j in (0, 1)]
LN_FWD_BATCHES = [((3072, 4), (256, 5)), ((3072, 8), (256, 4), (520, 7)), ((3072, 4), (256, 8), (520, 4), (4096, 5))]
LN_BWD_D = (8, 520, 3072, 3080, 3584, 4096)          # <6>: 8, 520, 3072;  <8>: 3080, 3584, 4096
# (D, rows, dres, dyg, gate stride, masked rows)
LN_BWD_CASES = [(D, (5, 7, 8, 9)[(i + j) % 4], (i + j) % 2 == 0, (i + 2 * j) % 3 != 0, ("shared", "six")[(i // 2 + j) % 2], ((0, 3), (4,), (3, 4), ())[(i + 3 * j) % 4])
                for i, D in enumerate(LN_BWD_D) for j in (0, 1)]
LN_BWD_BATCH = ((3072, 8), (3584, 7))
MG_D = (512, 520, 1032, 2048, 2056, 3072, 3080, 4096)      # <1> <2> <3> <4> <6> (5 -> 6) <6> <8> (7 -> 8) <8>
MG_RPB = (1, 8, 9, 17)
# (D, rpb, B, short last sample, gate, mask, wide strides)
MG_CASES = [(D, MG_RPB[(i + j) % 4], (1, 3)[(i + j) % 2], j == 1 and i % 2 == 0, (i + j) % 3 != 0, (i + j) % 4 == 1, (i + j) % 2 == 1)
            for i, D in enumerate(MG_D) for j in (0, 1)]
MG_BATCHES = [(3080, ((8, 1), (9, 3), (17, 2), (1, 3))), (520, ((17, 3), (8, 1)))]      # (D, ((rpb, B), ...)): grid.y sized by another problem
RMS_CASES = [(8, 1), (8, 5), (520, 5), (3584, 1), (4096, 5), (520, 1)]
GEMV_B, GEMV_K, GEMV_N = (1, 3, 8), (8, 256, 520, 4096), (1, 15, 16, 17, 130)
# (B, K, N, nmat, silu, bias)
GEMV_CASES = [(GEMV_B[(i + j) % 3], K, GEMV_N[(2 * i + j) % 5], (1, 3)[(i + j) % 2], (i + j) % 2 == 0, (i + j) % 3 != 2)
              for i, K in enumerate(GEMV_K) for j in range(5)] + [(8, 4096, 17, 1, False, True), (8, 4096, 1, 1, True, False)]
GEMVT_K, GEMVT_B, GEMVT_N = (8, 520, 1024, 1536, 2048, 3072), (1, 2, 3, 8), (1, 3, 4, 5, 130)
# (B, K, N, nmat):  K <= 1024 <*,2>, <= 2048 <*,4>, beyond <*,6>;  B odd ends in the one-sample form <1,*>
GEMVT_CASES = [(GEMVT_B[(i + j) % 4], K, GEMVT_N[(i + 2 * j) % 5], (1, 3)[(i + j) % 2]) for i, K in enumerate(GEMVT_K) for j in range(4)]
# (dh, B, S, T, H, flags, per-sample rope, saved)
QK_CASES = [(64, 2, 5, 2, 3, 0, True, True), (128, 2, 5, 2, 3, 1, True, True), (64, 3, 7, 0, 1, 1, False, True), (128, 3, 7, 7, 1, 0, True, False),
            (64, 1, 3, 3, 5, 0, False, False), (128, 1, 9, 0, 2, 0, False, True)]
COND_B, COND_R, COND_K, COND_N = (1, 3, 8), (1, 16, 64), (8, 300, 3072), (1, 255, 256, 257, 1000)
# (B, r, K, N, na, silu, wide ld, dx)
COND_CASES = [(COND_B[(i + j) % 3], COND_R[(i + 2 * j) % 3], COND_K[j], N, (1, 3)[(i + j) % 2], (i + j) % 2 == 1, j == 0, (i + j) % 3 != 0)
              for i, N in enumerate(COND_N) for j in (0, 1, 2)] + [(8, 64, 3072, 1000, 3, False, True, True)]
MSE_CASES = [(2, 5, 3, 4, 0), (2, 5, 3, 8, 1), (2, 5, 3, 8, 0), (3, 4, 4, 16, 0)]        # (B, S_all, S_t, C, target offset in elements)
GRID_STRIDE_N = (2048 * 256 + 77, 1024 * 256 + 77)      # cast_f32_bf16, silu_bwd: just past what their capped grids cover in one trip


def mod_views(buf_or_rows, D, stride, which):
    """The [B or 1, D] view of modulation vector `which` (0 shift, 1 scale, 2 gate) inside a [B, 6 D] table for the three
    stride kinds; returns (view, mod_bstride)."""
    t = buf_or_rows
    if stride == "shared":
        return t[:1, which * D:(which + 1) * D], 0
    if stride == "tight":
        return t[:, which * D:(which + 1) * D].contiguous(), D
    return t[:, which * D:(which + 1) * D], 6 * D


# ---------------------------------------------------------------------------------------------- families: inputs + reference per case
# make(case, kind) -> dict of CPU tensors (generated once per case, never modified); ref(inp, case, dt, flip) -> {output: (value, scale)}.
# The CPU noise floors and the GPU tests both walk FAMILIES, so the bars are measured on the very cases the kernels are held to.
FILL = dict(dshift=1.5, dscale=-0.5, dgate=0.25, gemv_t=1.5, dA=0.5, dB=-1.5, du=0.25, dx=2.0)   # finite, non-zero, exact initial values


def ln_fwd_make(case, kind="rand"):
    D, rows, _ = case
    B = (rows + RPB - 1) // RPB
    return case_data(kind, 1000 + D + rows, x=(rows, D), mod=((B, 6 * D), 0.5))


def ln_fwd_ref(inp, case, dt=F64, flip=False):
    D, _, stride = case
    return ln_fwd(inp["x"], mod_views(inp["mod"], D, stride, 0)[0], mod_views(inp["mod"], D, stride, 1)[0], RPB, dt=dt, flip=flip)


def ln_bwd_make(case, kind="rand"):
    D, rows = case[:2]
    B = (rows + RPB - 1) // RPB
    d = case_data(kind, 2000 + D + rows, x=(rows, D), dy=(rows, D), dres=(rows, D), mod=((B, 6 * D), 0.5))
    d["mask"] = torch.ones(rows)
    for r in case[5]:
        if r < rows:
            d["mask"][r] = 0.0
    return d


def ln_bwd_ref(inp, case, dt=F64, flip=False):
    D, rows, dres, dyg, gstride, masked = case
    return ln_bwd(inp["dy"], inp["x"], mod_views(inp["mod"], D, "six", 1)[0], RPB, dres=inp["dres"] if dres else None,
                  gate=mod_views(inp["mod"], D, gstride, 2)[0] if dyg else None, mask=inp["mask"] if masked else None, dt=dt, flip=flip)


def mg_rows(case):
    D, rpb, B, short = case[:4]
    return B * rpb - (max(1, rpb // 2) if short and rpb > 1 else 0)


def mg_lds(case):
    D, wide = case[0], case[6]
    return (D + 8, D + 16, D + 24, D + 8, 3 * D + 8) if wide else (D, D, D, D, D)     # ld_dy, ld_x, ld_dxo, ld_y, out_bstride


def mg_make(case, kind="rand"):
    D, rpb, B, short, gate, mask, wide = case
    rows = mg_rows(case)
    ld = mg_lds(case)
    d = case_data(kind, 3000 + D + rpb + B, dy=(rows, ld[0]), x=(rows, ld[1]), dxo=(rows, ld[2]), y=((rows, ld[3]), 2.0 ** -4 if kind == "exact" else 1.0))
    d["mask"] = torch.ones(rows)
    if mask:
        d["mask"][0] = 0.0
        d["mask"][rows - 1] = 0.0
        d["mask"][rows // 2] = 0.0
    return d


def mg_ref(inp, case, dt=F64, flip=False):
    D, rpb, B, short, gate, mask, wide = case
    return mod_grad(inp["dy"][:, :D], inp["x"][:, :D], rpb, dxo=inp["dxo"][:, :D] if gate else None, y=inp["y"][:, :D] if gate else None,
                    mask=inp["mask"] if mask else None, dt=dt, flip=flip)


def rms_make(case, kind="rand"):
    D, rows = case
    return case_data(kind, 4000 + D + rows, x=(rows, D), w=(D,))


def rms_ref(inp, case, dt=F64, flip=False):
    return rmsnorm(inp["x"], inp["w"], dt=dt, flip=flip)


def gemv_make(case, kind="rand"):
    B, K, N, nmat, _, bias = case
    g = _gen(5000 + B + K + N)
    if kind == "exact":
        d = dict(temb=ints(g, B, K), Ws=[ints(g, N, K, scale=2.0 ** -4) for _ in range(nmat)], bias=[ints(g, N) for _ in range(nmat)])
    else:
        d = dict(temb=randn_bf(g, B, K), Ws=[randn_bf(g, N, K, scale=0.05) for _ in range(nmat)], bias=[randn_bf(g, N) for _ in range(nmat)])
    if not bias:
        d["bias"] = None
    return d


def gemv_ref(inp, case, dt=F64, flip=False):
    return mod_gemv(inp["temb"], inp["Ws"], inp["bias"], case[4], dt=dt, flip=flip)


def gemvt_make(case, kind="rand"):
    B, K, N, nmat = case
    g = _gen(6000 + B + K + N)
    if kind == "exact":
        d = dict(dy=ints(g, nmat, B, N), Ws=[ints(g, N, K, scale=2.0 ** -4) for _ in range(nmat)])
    else:
        d = dict(dy=randn_bf(g, nmat, B, N), Ws=[randn_bf(g, N, K, scale=0.05) for _ in range(nmat)])
    d["out0"] = torch.full((B, K), FILL["gemv_t"])
    return d


def gemvt_ref(inp, case, dt=F64, flip=False):
    return mod_gemv_t(inp["dy"], inp["Ws"], inp["out0"], dt=dt, flip=flip)


def qk_make(case, kind="rand"):
    dh, B, S, T, H, flags, per_sample, saved = case
    g = _gen(7000 + dh + B + S + H)
    ang = torch.rand(B if per_sample else 1, S, dh // 2, generator=g) * 6.28
    return dict(qkv=randn_bf(g, B, S, 3 * H * dh), dqkv=randn_bf(g, B, S, 3 * H * dh), rope=torch.stack([torch.cos(ang), torch.sin(ang)], -1).contiguous(),
                ws=[(1.0 + 0.1 * torch.randn(dh, generator=g)).to(BF) for _ in range(4)])


def qk_fwd_ref(inp, case, dt=F64, flip=False):
    dh, B, S, T, H, flags = case[:6]
    return qk_fwd(inp["qkv"], inp["rope"], inp["ws"], T, H, dh, flags, dt=dt, flip=flip)


def qk_bwd_ref(inp, case, dt=F64, flip=False):
    dh, B, S, T, H, flags = case[:6]
    return qk_bwd(inp["dqkv"], inp["qkv"][..., :2 * H * dh], inp["rope"], inp["ws"], T, H, dh, flags, dt=dt, flip=flip)


MSE_GSCALE, MSE_INV_DENOM = 0.75, 1.0 / 5.5


def mse_make(case, kind="rand"):
    B, S_all, S_t, Cc, off = case
    g = _gen(8000 + B + S_all + Cc + off)
    return dict(pred=randn_bf(g, B, S_all, Cc), target=randn_bf(g, B, S_t, Cc), tw=torch.rand(B, S_t, generator=g) * 2.0)


def mse_ref(inp, case, dt=F64, flip=False):
    return mse(inp["pred"], inp["target"], case[2], MSE_GSCALE, dt=dt, flip=flip)


def mse_tw_ref(inp, case, dt=F64, flip=False):
    return mse_tw(inp["pred"], inp["target"], inp["tw"], case[2], MSE_INV_DENOM, MSE_GSCALE, dt=dt, flip=flip)


FM_CASES = [(2, 5, 0, 16, 1), (3, 4, 3, 8, 1), (2, 3, 2, 16, 0)]       # (B, S_t, S_c, C, mode)


def fm_make(case, kind="rand"):
    B, S_t, S_c, Cc, mode = case
    g = _gen(9000 + B + S_t + S_c)
    if kind == "exact":
        x0 = ints(g, B, S_t, Cc, dtype=torch.float16 if mode else BF)
        d = dict(x0=x0, noise=ints(g, B, S_t, Cc), sigma=torch.tensor([0.25, 0.5, 0.75][:B]).to(BF))
    else:
        x0 = torch.randn(B, S_t, Cc, generator=g).to(torch.float16 if mode else BF)
        d = dict(x0=x0, noise=randn_bf(g, B, S_t, Cc), sigma=torch.rand(B, generator=g).to(BF))
    d["ctrl"] = randn_bf(g, B, S_c, Cc) if S_c else None
    return d


def fm_ref(inp, case, dt=F64, flip=False):
    return flowmatch(inp["x0"], inp["noise"], inp["ctrl"], inp["sigma"], case[4], dt=dt)


TS_CASES = [(3, 256, 1000.0, 1.0), (2, 64, 1.0, 1000.0), (8, 10, 1.0, 1000.0)]      # (B, dim, scale, pre_scale)


def ts_make(case, kind="rand"):
    return dict(t=torch.rand(case[0], generator=_gen(9500 + case[1])))


def ts_ref(inp, case, dt=F64, flip=False):
    return timestep_embed(inp["t"], case[1], case[2], case[3], dt=dt)


SILU_BWD_N = (1000, GRID_STRIDE_N[1])


def sb_make(case, kind="rand"):
    g = _gen(9700 + case % 1000)
    return dict(ds=torch.randn(case, generator=g), x=randn_bf(g, case, scale=2.0))


def sb_ref(inp, case, dt=F64, flip=False):
    return silu_bwd(inp["ds"], inp["x"], dt=dt)


COND_SCALES = {"rand": (0.5, 2.0, 1.0), "exact": (0.5, 1.0, 0.25)}


def cond_make(case, kind="rand"):
    B, r, K, N, na, apply_silu, wide, dx = case
    g = _gen(10000 + B + r + K + N)
    if kind == "exact":
        d = dict(x=ints(g, B, K), A=ints(g, na, r, K, dtype=F32), Bm=ints(g, na, N, r, dtype=F32), y0=ints(g, na, B, N), g=ints(g, na, B, N))
    else:
        d = dict(x=randn_bf(g, B, K), A=torch.randn(na, r, K, generator=g) * 0.05, Bm=torch.randn(na, N, r, generator=g) * 0.05,
                 y0=randn_bf(g, na, B, N), g=randn_bf(g, na, B, N))
    d["s"] = torch.tensor(COND_SCALES[kind][:na])
    d["u"] = cond_fwd(d["x"], d["A"], d["Bm"], d["s"], d["y0"], apply_silu, dt=F32)["u"][0].float()    # what a forward leaves for the backward
    return d


def cond_fwd_ref(inp, case, dt=F64, flip=False):
    return cond_fwd(inp["x"], inp["A"], inp["Bm"], inp["s"], inp["y0"], case[5], dt=dt, flip=flip)


def cond_bwd_ref(inp, case, dt=F64, flip=False, u=None):
    B, r, K, N, na, apply_silu, wide, dx = case
    full = lambda v, *s: torch.full(s, v)      # noqa: E731
    return cond_bwd(inp["x"], inp["A"], inp["Bm"], inp["s"], inp["u"] if u is None else u, inp["g"], apply_silu, full(FILL["dA"], na, r, K),
                    full(FILL["dB"], na, N, r), full(FILL["du"], na, B, r), full(FILL["dx"], B, K) if dx else None, dt=dt, flip=flip)


# family -> (prefix of its BARS keys, cases, kinds, make, ref)
FAMILIES = {
    "ln_fwd": ("ln_fwd", LN_FWD_CASES, ("rand",), ln_fwd_make, ln_fwd_ref),
    "ln_bwd": ("ln_bwd", LN_BWD_CASES, ("rand",), ln_bwd_make, ln_bwd_ref),
    "mod_grad": ("mod_grad", MG_CASES, ("rand", "exact"), mg_make, mg_ref),
    "rmsnorm": ("rmsnorm", RMS_CASES, ("rand",), rms_make, rms_ref),
    "mod_gemv": ("mod_gemv", GEMV_CASES, ("rand", "exact"), gemv_make, gemv_ref),
    "mod_gemv_t": ("mod_gemv_t", GEMVT_CASES, ("rand", "exact"), gemvt_make, gemvt_ref),
    "qk_fwd": ("qk_fwd", QK_CASES, ("rand",), qk_make, qk_fwd_ref),
    "qk_bwd": ("qk_bwd", QK_CASES, ("rand",), qk_make, qk_bwd_ref),
    "mse": ("mse", MSE_CASES, ("rand",), mse_make, mse_ref),
    "mse_tw": ("mse_tw", MSE_CASES, ("rand",), mse_make, mse_tw_ref),
    "flowmatch": ("flowmatch", FM_CASES, ("rand", "exact"), fm_make, fm_ref),
    "timestep": ("timestep", TS_CASES, ("rand",), ts_make, ts_ref),
    "silu_bwd": ("silu_bwd", SILU_BWD_N, ("rand",), sb_make, sb_ref),
    "cond_fwd": ("cond", COND_CASES, ("rand", "exact"), cond_make, cond_fwd_ref),
    "cond_bwd": ("cond", COND_CASES, ("rand", "exact"), cond_make, cond_bwd_ref),
}


def exact_outputs(family, case, kind):
    """The outputs that must be BIT-EQUAL to the fp64 value on this case (exact_case data, no inexact activation on the path)."""
    if kind != "exact":
        return ()
    if family == "mod_grad":
        return ("dshift", "dgate")
    if family == "mod_gemv":
        return () if case[4] else ("out",)
    if family == "mod_gemv_t":
        return ("out",)
    if family == "flowmatch":
        return ("target",)
    if family == "cond_fwd":
        return () if case[5] else ("u", "y")
    if family == "cond_bwd":
        return ("du",) if case[5] else ("dA", "dB", "du", "dx")      # with SiLU, u and act(x) are no integers: only ga Bm stays exact
    return ()


FLOOR_DRAWS = 4


def measure_floors(families=None, draws=FLOOR_DRAWS):
    """{BARS key: worst error of the fp32, reversed-order restatement against the fp64 one, in bf16 ulps of scale} over every case
    of every family -- the reference's own noise (nothing here runs the code under test).  A flipped rounding is a rare event
    (about 2^-16 per rounding point and element), so every case is drawn `draws` times: draw 0 is the data of the GPU tests."""
    floors = {}
    try:
        for draw in range(draws):
            _DRAW[0] = draw
            for fam, (prefix, cases, kinds, make, ref) in FAMILIES.items():
                if families is not None and fam not in families:
                    continue
                for case in cases:
                    for kind in kinds:
                        inp = make(case, kind)
                        r64, r32 = ref(inp, case), ref(inp, case, F32, True)
                        for k, (v, sc) in r64.items():
                            key = f"{prefix}.{k}"
                            floors[key] = max(floors.get(key, 0.0), err_ulps(r32[k][0], v, sc))
    finally:
        _DRAW[0] = 0
    return floors
