"""CPU restatement of csrc/qfx_optim.hip -- the clip prologue, qfx_sumsq / qfx_sumsq_det, qfx_adamw_step(_grouped), qfx_sgd_step(_grouped)
and qfx_prodigy_step -- the yardstick of tests/test_optim_gpu.py; tests/test_optim_ref_cpu.py checks the yardstick itself against
torch.optim, oracle/prodigy.py and exact rationals.  numpy on the CPU, nothing here touches the code under test.

Three tiers:
  * fp64 (`*_f64`): the header's arithmetic in double on the fp32 images of the scalars, lr / bc1 and 1 / sqrt(bc2) formed once as the
    kernel forms them.  Every output comes as (value, scale): scale is the sum of the magnitudes of the addends that form the value,
    and errors are counted in fp32 ulps of scale (err_ulps), so a cancelled sum is not held to the ulp of its small result; p's
    scale carries the scale of m's addends through the update, so a cancelled m is not held to the ulp of its small value either.
  * fp32 bit oracle (`adamw_f32`, `sgd_f32`): adamw_elem and sgd_elem pin their contraction (contract(off), explicit fmaf), the
    library is built without fast-math, so / and sqrtf are correctly rounded: one numpy fp32 operation per kernel operation and an
    exact fmaf (fma32: error-free sum, round-to-odd in double, one rounding to fp32) give the kernel's BITS whenever the clip
    coefficient itself is pinned -- no norm, max_norm <= 0, or a grad_scale that is a power of two (sqrt(gnorm_sq) * grad_scale is
    then exact and fusing it with the + 1e-6 changes nothing).
  * fp32 floor (`prodigy_*` with f32=True, clip_f32(fused=...)): qfx_optim.hip is built with the compiler's default contraction,
    so Prodigy's element updates and the prologue may fuse.  Every product and sum rounded is one legal form, not a bit oracle: its
    own error against the fp64 tier is the FLOOR, and BARS = twice that (measured by test_optim_ref_cpu.py, written below).
The two sums are restated in fp64 with a derived bound (sum_bound): non-negative terms, relative error <= (1 + u)^(depth + 1) - 1,
u = 2^-24, depth = the longest chain of additions a term passes through; the + 1 is the rounding of g * g, so the bound holds whether
or not acc += g * g fuses."""
from __future__ import annotations

import math

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
EPS6 = float(F32(1e-6))                  # the prologue's 1e-6f


def f32img(x):
    return float(F32(x))


# ---------------------------------------------------------------- exact fmaf
def fma32(a, b, c):
    """fmaf on fp32 operands, one rounding.  a * b is exact in double (48 bits); the sum with c is formed error-free (TwoSum) and
    rounded to odd in double, which a final round-to-nearest to 24 bits cannot tell from the exact sum (53 >= 24 + 2).  fp64
    a * b + c rounded to fp32 rounds twice and misses near ties."""
    a64, b64, c64 = np.broadcast_arrays(*(np.asarray(x, F32).astype(F64) for x in (a, b, c)))
    p = a64 * b64
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)
    s = np.ascontiguousarray(s)
    even = (s.view(np.int64) & 1) == 0
    nxt = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & even, nxt, s).astype(F32)


# ---------------------------------------------------------------- errors in ulps of a scale
def ulp32(scale):
    _, e = np.frexp(np.maximum(np.abs(np.asarray(scale, F64)), 2.0 ** -126))
    return np.ldexp(1.0, e - 24)


def err_ulps(got, ref, scale):
    """Worst |got - ref| in fp32 ulps of scale; a non-finite `got` is infinitely wrong."""
    g = np.asarray(got, F64)
    if g.size == 0:
        return 0.0
    if not np.isfinite(g).all():
        return float("inf")
    return float((np.abs(g - ref) / ulp32(scale)).max())


# ---------------------------------------------------------------- the clip prologue (opt_clip, csrc/qfx_optim.h)
def clip_f64(gnorm_sq, max_norm, grad_scale):
    """gnorm_sq: the fp32 value in memory, or None for a NULL pointer."""
    gs = f32img(grad_scale)
    if gnorm_sq is None or not f32img(max_norm) > 0:
        return gs
    c = f32img(max_norm) / (math.sqrt(f32img(gnorm_sq)) * gs + EPS6)
    return gs * (c if c < 1.0 else 1.0)


def clip_f32(gnorm_sq, max_norm, grad_scale, fused=False):
    """The prologue's fp32 operations one by one; fused: sqrt(gnorm_sq) * grad_scale + 1e-6 as one FMA (the other legal form)."""
    gs = F32(grad_scale)
    if gnorm_sq is None or not F32(max_norm) > 0:
        return gs
    r = np.sqrt(F32(gnorm_sq))
    den = fma32(r, gs, F32(EPS6))[()] if fused else F32(r * gs) + F32(EPS6)
    c = F32(max_norm) / F32(den)
    return F32(gs * (c if c < F32(1.0) else F32(1.0)))


def bias_corr(beta, t):
    """What ops.adamw_step hands the C ABI: 1 - beta^t in double, rounded to the fp32 argument."""
    return f32img(1.0 - f32img(beta) ** t)


# ---------------------------------------------------------------- AdamW
def adamw_f64(p, g, m, v, clip, lr, b1, b2, eps, wd, bc1, bc2, mut=None):
    """{"p", "m", "v"} -> (value, scale) in fp64.  Scalars are used as given (the GPU tests pass fp32 images, the torch comparison
    passes doubles).  mut: one of the deliberate mistakes test_optim_ref_cpu.py must see separated."""
    p, g, m, v = (np.asarray(x, F64) for x in (p, g, m, v))
    step, rs2 = lr / bc1, 1.0 / math.sqrt(bc2)
    if mut == "no_eps":
        eps = 0.0
    if mut == "no_wd":
        wd = 0.0
    gi = g * clip
    decay = 1.0 - lr * wd
    pi = p if mut == "decay_after" else p * decay
    mi = (1.0 - b1) * gi + b1 * m
    vi = b2 * v + (1.0 - b2) * gi * (1.0 if mut == "v_linear" else gi)
    den = rs2 * np.sqrt(np.abs(vi)) + eps
    upd = (step * mi) / den
    pn = pi - upd
    if mut == "decay_after":
        pn = pn * decay
    ms = np.abs((1.0 - b1) * gi) + np.abs(b1 * m)       # the update carries the scale of m's addends, not of their cancelled sum
    return {"p": (pn, np.abs(pi) + np.abs(step) * ms / den), "m": (mi, ms), "v": (vi, np.abs(vi))}


def adamw_f32(p, g, m, v, clip, lr, b1, b2, eps, wd, bc1, bc2):
    """adamw_elem's bits: (p, m, v) fp32."""
    p, g, m, v = (np.asarray(x, F32) for x in (p, g, m, v))
    clip, lr, b1, b2, eps, wd, bc1, bc2 = (F32(x) for x in (clip, lr, b1, b2, eps, wd, bc1, bc2))
    one = F32(1.0)
    step, rs2 = lr / bc1, one / np.sqrt(bc2)
    with np.errstate(invalid="ignore", divide="ignore"):
        gi = g * clip
        pi = p * fma32(-lr, wd, one)
        mi = fma32(one - b1, gi, b1 * m)
        vi = b2 * v + ((one - b2) * gi) * gi
        pn = pi - (step * mi) / fma32(rs2, np.sqrt(vi), eps)
    return pn.astype(F32), mi.astype(F32), vi.astype(F32)


# ---------------------------------------------------------------- SGD
def sgd_f64(p, g, buf, clip, lr, mom, damp, wd, nesterov, first, mut=None):
    """{"p", "buf"} -> (value, scale); "buf" only when mom != 0."""
    p, g = np.asarray(p, F64), np.asarray(g, F64)
    keep = 1.0 - damp
    if mut == "ignore_first":
        first = False
    if mut == "clip_after_decay":
        gi = (g + wd * p) * clip
    else:
        gi = g * clip + wd * p
    sc = np.abs(g * clip) + np.abs(wd * p)
    out = {}
    if mom != 0:
        b = np.asarray(buf, F64)
        if first:
            bi, bs = (keep * gi if mut == "damp_on_first" else gi), sc
        else:
            bi, bs = keep * gi + mom * b, np.abs(keep) * sc + np.abs(mom * b)
        out["buf"] = (bi, bs)
        if nesterov and mut != "no_nesterov_sum":
            gi, sc = gi + mom * bi, sc + np.abs(mom) * bs
        else:
            gi, sc = bi, bs
    out["p"] = (p - lr * gi, np.abs(p) + np.abs(lr) * sc)
    return out


def sgd_f32(p, g, buf, clip, lr, mom, damp, wd, nesterov, first):
    """sgd_elem's bits: (p, buf) fp32; buf is None when mom == 0."""
    p, g = np.asarray(p, F32), np.asarray(g, F32)
    clip, lr, mom, damp, wd = (F32(x) for x in (clip, lr, mom, damp, wd))
    keep = F32(1.0) - damp
    with np.errstate(invalid="ignore"):
        gi = g * clip
        if wd != 0:
            gi = wd * p + gi
        bi = None
        if mom != 0:
            bi = gi if first else keep * gi + mom * np.asarray(buf, F32)
            gi = fma32(mom, bi, gi) if nesterov else bi
            bi = bi.astype(F32)
        pn = fma32(-lr, gi, p)
    return pn, bi


# ---------------------------------------------------------------- Prodigy (the four kernels of qfx_prodigy_step)
PRODIGY_DEFAULTS = dict(lr=1.0, b1=0.9, b2=0.999, beta3=0.0, eps=1e-8, wd=0.0, d0=1e-6, d_coef=1.0, growth=float("inf"), use_bc=0,
                        safeguard=0)


def prodigy_hp(**kw):
    """The scalars as the launcher sees them: fp32 struct fields widened to double."""
    h = dict(PRODIGY_DEFAULTS, **kw)
    return {k: (f32img(x) if isinstance(x, float) else x) for k, x in h.items()}


def prodigy_state(d0, **kw):
    """qfx_prodigy_init_state: d = d_max = d_hat = d0, everything else 0."""
    d0 = float(d0)
    return dict(dict(d=d0, d_max=d0, num=0.0, den=0.0, d_hat=d0, k=0.0), **kw)


def prodigy_beta3(h, mut=None):
    if h["beta3"] > 0:
        return h["beta3"]
    return h["b2"] if mut == "beta3_is_beta2" else math.sqrt(h["b2"])


def prodigy_begin(st, h):
    """prodigy_begin_kernel: dlr = d lr bias_correction with the d of the previous step, in Python floats."""
    k = st["k"]
    bc = math.sqrt(1.0 - math.pow(h["b2"], k + 1.0)) / (1.0 - math.pow(h["b1"], k + 1.0)) if h["use_bc"] else 1.0
    return st["d"] * h["lr"] * bc


def prodigy_ema(p, g, m, v, s, p0, st, h, clip, f32=False, mut=None, round_scalars=True):
    """prodigy_ema_kernel.  {"m", "v", "s"} -> (value, scale), plus acc_num = <g', p0 - p> and acc_den = |s|_1 in fp64.
    f32: every product and sum rounded to fp32 (values only, scale None).  round_scalars=False: the package's unrounded doubles
    (for the comparison with oracle/prodigy.py)."""
    d, d0, dlr = st["d"], h["d0"], prodigy_begin(st, h)
    b3 = prodigy_beta3(h, mut)
    rs = f32img if round_scalars else float
    safeguard = h["safeguard"] if mut != "safeguard_swapped" else not h["safeguard"]
    am, av = rs(d * (1.0 - h["b1"])), rs(d * d * (1.0 - h["b2"]))
    a_s = rs((d / d0) * d if safeguard else (d / d0) * dlr)
    b1, b2, b3 = h["b1"], h["b2"], rs(b3)
    T = F32 if f32 else F64
    p, g, m, v, s, p0 = (np.asarray(x, T) for x in (p, g, m, v, s, p0))
    clip, am, av, a_s, b1, b2, b3 = (T(x) for x in (clip, am, av, a_s, b1, b2, b3))
    gi = g * clip
    num = (gi * (p0 - p)).astype(F64).sum()
    mn, vn, sn = m * b1 + gi * am, v * b2 + (av * gi) * gi, s * b3 + gi * a_s
    den = np.abs(sn).astype(F64).sum()
    if f32:
        return {"m": (mn, None), "v": (vn, None), "s": (sn, None)}, float(num), float(den)
    return {"m": (mn, np.abs(m * b1) + np.abs(gi * am)), "v": (vn, np.abs(vn)), "s": (sn, np.abs(s * b3) + np.abs(gi * a_s))}, float(num), float(den)


def prodigy_d(st, h, acc_num, acc_den, mut=None):
    """prodigy_d_kernel in Python floats: the new scalar state, or None when den == 0 (the package returns before storing anything:
    d, k and p keep their values)."""
    if acc_den == 0.0:
        return None
    b3, d, d0 = prodigy_beta3(h, mut), st["d"], h["d0"]
    num = st["num"] * b3 + (d / d0) * prodigy_begin(st, h) * acc_num
    d_hat = h["d_coef"] * num / acc_den
    if F32(d) == F32(d0):       # decided in float: the state holds the caller's double d0, the step's struct its float image
        d = max(d, d_hat)
    d_max = max(st["d_max"], d_hat)
    d = min(d_max, d * h["growth"])
    return dict(d=d, d_max=d_max, num=num, den=acc_den, d_hat=d_hat, k=st["k"] + 1.0)


def prodigy_apply(p, m, v, d_new, dlr, h, f32=False, mut=None, round_scalars=True, m_scale=None):
    """prodigy_apply_kernel on the NEW m, v with the new d in d eps and the step's dlr.  "p" -> (value, scale); m_scale: the scale of
    m's addends, which the update carries (a cancelled m is not held to the ulp of its small value)."""
    rs = f32img if round_scalars else float
    T = F32 if f32 else F64
    deps = T(rs(h["eps"] if mut == "eps_not_scaled" else d_new * h["eps"]))
    adec, astep = T(rs(-h["wd"] * dlr)), T(rs(-dlr))
    p, m, v = (np.asarray(x, T) for x in (p, m, v))
    pi, sc = p, np.abs(p)
    if h["wd"] != 0:
        pi, sc = p + p * adec, sc + np.abs(p * adec)
    with np.errstate(invalid="ignore", divide="ignore"):
        upd = astep * (m / (np.sqrt(v) + deps))
        if not f32:
            sc = sc + np.abs(astep) * (np.abs(m) if m_scale is None else m_scale) / (np.sqrt(v) + deps)
    return {"p": (pi + upd, None if f32 else sc)}


def prodigy_step(p, g, m, v, s, p0, st, h, clip, f32=False, mut=None, den=None, round_scalars=True):
    """One whole qfx_prodigy_step.  den: evaluate the scalar kernel on this |s|_1 instead of the restatement's own (the GPU test hands
    in the device's fp32-summed value, held to its own bound, so that the double arithmetic behind it is compared to 1e-12).
    Returns (outputs, new state or None for a skipped / lr == 0 step, acc_num, acc_den)."""
    if h["lr"] == 0.0:
        return {}, None, 0.0, 0.0
    out, acc_num, acc_den = prodigy_ema(p, g, m, v, s, p0, st, h, clip, f32, mut, round_scalars)
    new = prodigy_d(st, h, acc_num, acc_den if den is None else den, mut)
    if new is not None:
        out.update(prodigy_apply(p, out["m"][0], out["v"][0], new["d"], prodigy_begin(st, h), h, f32, mut, round_scalars, out["m"][1]))
    return out, new, acc_num, acc_den


def prodigy_den_bound(s_scale, trips):
    """|device d_denom - sum |s_ref|| allowed: every s_i is formed by three roundings on addends of total magnitude scale_i (g', the two
    products; then the sum) -> (1 + u)^3 - 1 of scale_i whichever products fuse; the fp32 part of the sum is the per-thread trips and
    the 6 butterfly levels (non-negative terms), the four waves and the workgroups are added in double."""
    tot = float(np.asarray(s_scale, F64).sum())
    return ((1 + U) ** 3 - 1) * tot + ((1 + U) ** (trips + 6 + 1) - 1) * tot


# ---------------------------------------------------------------- the two sums
def flat_grid(work, cap):
    return min((work + 255) // 256, cap)


def sumsq_f64(g):
    return float((np.asarray(g, F64) ** 2).sum())


def sumsq_depth(n, det, nslots=2048):
    """Longest chain of fp32 additions of qfx_sumsq (det=False: 2048 blocks at most) / qfx_sumsq_det (det=True: nslots at most)."""
    blocks = flat_grid(n, nslots if det else 2048)
    trips = -(-n // (blocks * 256))
    if det:     # per-thread trips, 6 butterfly levels, 2 levels of the four-wave fold; the fold kernel the same over `blocks` partials
        return trips + 6 + 2 + -(-blocks // 256) + 6 + 2
    return trips + 6 + 3 + blocks      # red[0] + red[1] + red[2] + red[3] left to right; blocks - 1 atomics among them, 1 into out


def sum_bound(depth):
    """Relative error of a sum of non-negative terms whose longest chain has `depth` additions, the term's own product included."""
    return (1 + U) ** (depth + 1) - 1


# ---------------------------------------------------------------- data
def _rng(seed):
    return np.random.default_rng(seed)


def pad_slots(n):
    """Zero slots behind tensors, as LoraStore leaves them: for n >= 255 a gap inside and the tail."""
    return [(100, 128), (n - 20, n)] if n >= 255 else []


def rand_data(n, seed=0, pad=True):
    """fp32 p, g, m, v, buf, s, p0 of n elements.  Magnitudes are spread over decades per element (|g| from 1e-7 to 1, |p| from 1e-4
    to 1, independently) so that every term of every update dominates somewhere: eps = 1e-8 is felt where sqrt(v) ~ 1e-7, the decay
    where |p| >> lr, the order of decay and update where |p| << lr.  v > 0 everywhere outside the pad slots."""
    r = _rng(seed)
    gm = 10.0 ** r.integers(-7, 1, n)
    pm = 10.0 ** r.integers(-4, 1, n)
    d = dict(g=r.standard_normal(n) * gm, p=r.standard_normal(n) * pm, m=r.standard_normal(n) * gm * 0.3,
             v=(r.standard_normal(n) * gm) ** 2 + (1e-3 * gm) ** 2, buf=r.standard_normal(n) * gm * 2.0)
    d["p0"] = d["p"] + r.standard_normal(n) * pm * 0.1
    d["s"] = r.standard_normal(n) * gm * 1e-6          # Prodigy's s ~ d g
    d = {k: x.astype(F32) for k, x in d.items()}
    if pad:
        for a, b in pad_slots(n):
            for x in d.values():
                x[a:b] = 0.0
    return d


def prodigy_rescale(d, dd):
    """Prodigy's moments live at d g and d^2 g^2: bring rand_data's m, v, s to the scale of the distance estimate dd."""
    out = dict(d)
    out["m"] = (d["m"].astype(F64) * dd).astype(F32)
    out["v"] = (d["v"].astype(F64) * dd * dd).astype(F32)
    out["s"] = (d["s"].astype(F64) * (dd / 1e-6)).astype(F32)
    return out


def select_data(n, seed=0):
    """Small integers times powers of two: g = k / 16 (|k| <= 2), p and p0 = j / 64 (|j| <= 1) -- every g^2 and every g (p0 - p) is
    at most 16 units of 2^-10, so every partial sum of either over up to 2^19 + 3 elements is an integer below 2^24 of these units:
    exact in fp32 in ANY order (and under fusion, and times a power-of-two clip).  The two norms and Prodigy's numerator compare
    exactly."""
    r = _rng(1000 + seed)
    assert n <= (1 << 19) + 3
    g = r.integers(-2, 3, n) / 16.0
    p = r.integers(-1, 2, n) / 64.0
    p0 = r.integers(-1, 2, n) / 64.0
    d = rand_data(n, seed, pad=False)
    d.update(g=g.astype(F32), p=p.astype(F32), p0=p0.astype(F32))
    return d


# ---------------------------------------------------------------- cases
LENGTHS_SMALL = [1, 3, 255, 257, 1027]
N_STEP_TRIP2 = (1 << 20) + 3          # second grid-stride trip of the 4096-block step kernels
N_SUM_TRIP2 = (1 << 19) + 3           # second trip of the 2048-block sum and Prodigy kernels
N_GROUPED_VEC_TRIP2 = 4 * (1 << 20) + 67      # second trip of the grouped 16-byte form
STEPS = [1, 2, 1000]

ADAMW_HP = {
    "default": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2),
    "wd0": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0),
    "beta1_0": dict(lr=1e-3, b1=0.0, b2=0.999, eps=1e-8, wd=1e-2),
    "eps0": dict(lr=1e-3, b1=0.9, b2=0.999, eps=0.0, wd=1e-2),          # v > 0 in rand_data outside the pad slots
    "eps_large": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-3, wd=1e-2),
}
ADAMW_LORAPLUS = [dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2), dict(lr=1.6e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.0)]
SGD_HP = {
    "default": dict(lr=0.05, mom=0.9, damp=0.0, wd=1e-4, nesterov=0),
    "nesterov": dict(lr=0.05, mom=0.9, damp=0.0, wd=1e-4, nesterov=1),
    "dampening": dict(lr=0.05, mom=0.8, damp=0.1, wd=1e-4, nesterov=0),
    "wd0": dict(lr=0.05, mom=0.9, damp=0.0, wd=0.0, nesterov=0),
    "mom0": dict(lr=0.05, mom=0.0, damp=0.0, wd=1e-4, nesterov=0),
}
SGD_LORAPLUS = [dict(lr=0.05, mom=0.9, damp=0.0, wd=1e-4, nesterov=1), dict(lr=0.8, mom=0.0, damp=0.0, wd=0.0, nesterov=0)]
# name -> (pass gnorm_sq, max_norm as a share of ||g|| grad_scale (<= 0: that value itself), grad_scale, bit-exact)
CLIPS = {
    "null_norm": (False, 0.25, 1.0, True),
    "max_norm_0": (True, 0.0, 0.5, True),
    "max_norm_neg": (True, -1.0, 1.0, True),
    "clip_gs1": (True, 0.25, 1.0, True),
    "clip_gs_half": (True, 0.25, 0.5, True),
    "clip_gs_third": (True, 0.25, 1.0 / 3.0, False),
}


def clip_args(name, g):
    """(gnorm_sq fp32 value or None, max_norm, grad_scale, exact) of a CLIPS line on gradient g; gnorm_sq is the fp32 image of the
    fp64 sum -- both sides are handed the same number."""
    use, share, gs, exact = CLIPS[name]
    gsq = f32img(sumsq_f64(g))
    mx = f32img(share * math.sqrt(gsq) * f32img(gs)) if share > 0 else share
    if use and share > 0:
        assert gsq > 0 and clip_f64(gsq, mx, gs) < 0.3 * f32img(gs)        # the clip is active
    return (gsq if use else None), mx, f32img(gs), exact


PRODIGY_CASES = {      # hyperparameters over PRODIGY_DEFAULTS
    "default": dict(),
    "bias_corr": dict(use_bc=1),
    "safeguard": dict(safeguard=1, use_bc=1),
    "beta3": dict(beta3=0.99),
    "decay": dict(wd=0.01, use_bc=1),
    "growth": dict(growth=1.02),
    "lr_half": dict(lr=0.5, safeguard=1),
}



def prodigy_inputs(name, n=1027, seed=3, dd=3e-4):
    """Mid-run state of a PRODIGY_CASES line: d = d_max = dd, k = 7, moments at the scale of dd."""
    h = prodigy_hp(**PRODIGY_CASES[name])
    d = prodigy_rescale(case_data(n, seed), dd)
    st = prodigy_state(h["d0"], d=dd, d_max=dd, num=1e-2, den=1e-5, d_hat=dd, k=7.0)
    return h, d, st


def prodigy_element_cases():
    """(case, clip, n, seed) of the element-state comparison: every case and clip at 1027, the short lengths (one thread, a partial
    wave, a block and a bit) with cases and clips in rotation, and the second grid-stride trip."""
    clips = ("null_norm", "clip_gs_half", "clip_gs_third")
    out = [(name, cn, 1027, 3) for name in PRODIGY_CASES for cn in clips]
    out += [(name, clips[(i + n) % 3], n, n + i) for n in LENGTHS_SMALL[:-1] for i, name in enumerate(PRODIGY_CASES)]
    return out + [("decay", "clip_gs_half", N_SUM_TRIP2, 3)]


PRODIGY_D0 = 1e-6           # as every caller holds it: a double; qfx_prodigy_init_state stores it, the step sees its float image


def prodigy_scalar_states():
    """(name, hyperparameters, scalar state) that take prodigy_d_kernel through each branch on select_prodigy data: d == d0 raised to
    d_hat uncapped (the "fresh" states are what qfx_prodigy_init_state(1e-6) writes: the double 1e-6, not its float image), the
    growth cap binding and absent, d_max kept."""
    dd = 3e-4
    mid = lambda **kw: prodigy_state(PRODIGY_D0, **dict(dict(d=dd, d_max=dd, num=1e-9, den=1e-5, d_hat=dd, k=7.0), **kw))      # noqa: E731
    fresh = lambda: prodigy_state(PRODIGY_D0)      # noqa: E731
    return [("fresh_growth2", dict(growth=2.0), fresh()), ("fresh_growth1.02", dict(growth=1.02), fresh()),
            ("fresh_bc", dict(use_bc=1, safeguard=1), fresh()),
            ("cap", dict(growth=1.02, use_bc=1), mid()), ("free", dict(beta3=0.99, wd=0.01), mid()),
            ("dmax_kept", dict(growth=1.02, safeguard=1), mid(d_max=1e6))]


def prodigy_scalar_cases():
    """(name, hyperparameters, state, n): every state at every length of the sum and Prodigy kernels."""
    return [(name, kw, dict(st), n) for n in LENGTHS_SMALL + [N_SUM_TRIP2] for name, kw, st in prodigy_scalar_states()]


def select_prodigy(n, dd):
    """select_data with p = 0 and p0 = sign(g) / 64: <g, p0 - p> > 0 and every product exact; moments at the scale of dd."""
    d = prodigy_rescale(select_data(n), dd)
    d["p0"], d["p"] = (np.sign(d["g"]) / 64.0).astype(F32), np.zeros(n, F32)
    return d


# BARS[line][output]: fp32 ulps of scale, twice the floors test_optim_ref_cpu.py::test_bars_are_twice_the_floors measures (the fp32
# restatement against the fp64 one over every case above, both forms of the unpinned prologue); never taken from a kernel's output.
FLOORS = {
    "adamw": {"p": 3.29, "m": 1.40, "v": 1.58},
    "sgd": {"p": 2.10, "buf": 2.20},
    "prodigy": {"p": 3.82, "m": 1.66, "v": 1.81, "s": 2.76},
}
BARS = {line: {k: 2.0 * x for k, x in fl.items()} for line, fl in FLOORS.items()}
MUTANT_MARGIN = 4.0          # every mutant misses the fp64 reference by at least this many bars
SCALAR_RTOL = 1e-12          # Prodigy's double scalars


# ---------------------------------------------------------------- what the CPU and the GPU tests share
def adamw_args(hp, t):
    """The twelve scalars of qfx_adamw_step at step t as the C ABI receives them (fp32 images); clip is filled in by the caller."""
    a = {k: f32img(x) for k, x in hp.items()}
    return dict(a, bc1=bias_corr(hp["b1"], t), bc2=bias_corr(hp["b2"], t))


def sgd_args(hp):
    return {k: (f32img(x) if isinstance(x, float) else x) for k, x in hp.items()}


def case_data(n, seed, hp_name=""):
    """eps = 0 divides 0 by 0 in a zero slot (as torch does): that line runs without pad slots."""
    return rand_data(n, seed, pad=hp_name != "eps0")


def clips_of(name, g):
    """(fp64 clip, [fp32 clip in each legal form of the prologue], exact, (gnorm_sq, max_norm, grad_scale))."""
    gsq, mx, gs, exact = clip_args(name, g)
    forms = [clip_f32(gsq, mx, gs), clip_f32(gsq, mx, gs, fused=True)]
    assert not exact or forms[0] == forms[1]
    return clip_f64(gsq, mx, gs), forms, exact, (gsq, mx, gs)
