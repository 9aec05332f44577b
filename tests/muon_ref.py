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


# ---- one product at a time, exactly (tests/test_muon_cpu.py, tests/test_muon_gpu.py) --------------------------------------------
# ns_coefficients isolates a product in one iteration: (0, 1, 0) gives X1 = bf16(G X0), (0, 0, 1) gives bf16(bf16(G G) X0), (a, 0, 0)
# gives a X0.  On a matrix in {0, +1, -1} with 4^j non-zeros the norm is 2^j and X0 is in {0, +-2^-j}: every term of every sum is an
# integer multiple of one power of two, and while the sum of the terms' magnitudes stays below 2^24 of those units every partial sum in
# ANY order is an fp32 number.  Such a product has one value, whatever the association order: a kernel must meet it bit for bit.
PROBES = {"gram": (0, 1, 0), "gg": (0, 0, 1), "ax": (1, 0, 0), "ax_half": (0.5, 0, 0)}


def short_image(m):
    """The [s, n] image of a [rows, cols] matrix, the short side on the rows."""
    return m.T if m.shape[0] > m.shape[1] else m


def max_design_j(shape):
    """The largest j with 4^j <= rows * cols."""
    j = 0
    while 4 ** (j + 1) <= shape[0] * shape[1]:
        j += 1
    return j


def sign_design(shape, seed, nonzeros=None):
    """fp32 [rows, cols] in {0, +1, -1} with exactly 4^j non-zeros at random positions with random signs; j the largest that fits, or
    the one of `nonzeros` (= 4^j) where given.  Every row and every column holds a non-zero: the seed is advanced until they do."""
    k = shape[0] * shape[1]
    nz = 4 ** max_design_j(shape) if nonzeros is None else int(nonzeros)
    j = round(math.log(nz, 4))
    if 4 ** j != nz or not 0 < nz <= k:
        raise ValueError(f"sign_design: {nz} non-zeros in {shape}")
    for attempt in range(4096):
        g = torch.Generator().manual_seed(seed + 7919 * attempt)
        flat = torch.zeros(k)
        pos = torch.randperm(k, generator=g)[:nz]
        flat[pos] = torch.randint(0, 2, (nz,), generator=g).float() * 2 - 1
        m = flat.view(shape)
        if bool((m != 0).any(0).all()) and bool((m != 0).any(1).all()):
            return m
    raise ValueError(f"sign_design: no seed near {seed} fills every row and column of {shape} with {nz} non-zeros")


def _unit(a):
    """The lowest set bit over the non-zero elements of a, as a power of two; every element is an integer multiple of it."""
    v = a.double().abs().numpy().ravel()
    v = v[v != 0]
    if v.size == 0:
        return None
    m, e = np.frexp(v)
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = np.log2((mi & -mi).astype(np.float64)) + e - 53
    return 2.0 ** float(low.min())


def exact_ok(A, B):
    """Sufficient for A @ B to be exact in fp32 in every summation order: with uA, uB the lowest set bits of A and B every term is an
    integer multiple of uA uB, and max over outputs of sum_k |a_ik b_kj| / (uA uB) < 2^24 keeps every partial sum within 24 bits."""
    ua, ub = _unit(A), _unit(B)
    if ua is None or ub is None:
        return True
    mag = (A.double().abs() @ B.double().abs()).max().item() / (ua * ub)
    return mag < 2.0 ** 24 and ua * ub >= 2.0 ** -100 and mag * ua * ub < 2.0 ** 100       # and nothing near the ends of fp32's range


def _drop_last_gram_chunk(n):
    return (n + 31) // 32 * 32 - 32


def ns_staged(x, coeffs=COEFFS, ns_steps=1, f64=True, mutant=None):
    """The iteration stage by stage with the kernel's rounding points: G, H and X to bf16, the fp32 results b G + c (G G) and
    a X + H X formed from separately rounded fp32 products and one fp32 addition (no contraction).  f64: the three matrix products are
    accumulated in float64 and rounded to fp32 where the kernel holds an fp32 accumulator; otherwise torch's fp32 matmul.
    mutant: None, or one of the three kernel faults of MUTANTS.  Returns (X, the exact_ok verdict of every product formed)."""
    a, b, c = (torch.tensor(float(v), dtype=torch.float32) for v in coeffs)
    mm = (lambda p, q: (p.double() @ q.double()).float()) if f64 else (lambda p, q: p @ q)
    s, n = x.shape
    ok = {}
    for it in range(ns_steps):
        xf = x.float()
        xg = xf[:, :_drop_last_gram_chunk(n)] if mutant == "gram_chunk" else xf
        ok[f"xxT{it}"] = exact_ok(xg, xg.T)
        g = mm(xg, xg.T).to(BF)
        if mutant == "g_element":
            g[s // 2, s // 2] = 0
        gf = g.float()
        ok[f"gg{it}"] = exact_ok(gf, gf)
        h = (b * gf + c * mm(gf, gf)).to(BF)
        hf = h.float()
        ok[f"hx{it}"] = exact_ok(hf, xf)
        acc = mm(hf, xf)
        if mutant == "hx_strip":
            c0 = (n - 1) // 16 * 16
            acc[:, c0:c0 + 16] = 0
        x = (a * xf + acc).to(BF)
    return x, ok


def probe_exact(x0, coeffs):
    """One iteration from x0 in float64 with the kernel's rounding points, and whether each of its three products was exact."""
    return ns_staged(x0, coeffs, 1, f64=True)


def _mutant(kind):
    def run(x0, coeffs=COEFFS, ns_steps=1):
        return ns_staged(x0, coeffs, ns_steps, f64=False, mutant=kind)[0]
    return run


# What a kernel fault would compute: the Gram product without its last 32-column chunk in every iteration; G with its middle diagonal
# element cleared; the last 16-column strip of H X never added.  Only to show on the CPU that a comparison sees them.
MUTANTS = {"gram_chunk": _mutant("gram_chunk"), "g_element": _mutant("g_element"), "hx_strip": _mutant("hx_strip")}


def bf16_ulps(a, b):
    """|a - b| elementwise in steps of the bf16 grid (sign-magnitude order of the bit patterns), int32."""
    def key(t):
        v = t.to(BF).contiguous().view(torch.int16).to(torch.int32)
        mag = v & 0x7FFF
        return torch.where(v < 0, -mag, mag)
    return (key(a) - key(b)).abs()


def norm_margin(u):
    """Relative distance of the float64 norm of bf16(u) from the nearest bf16 rounding boundary, and that norm."""
    nrm = float(u.to(BF).double().pow(2).sum().sqrt())
    m, e = math.frexp(nrm)                                 # m in [0.5, 1): bf16 values at multiples of 2^-8, boundaries half way
    f = m * 256.0
    d = abs(f - math.floor(f) - 0.5) / 256.0
    return d / m, nrm
