"""CPU restatement of qfx_scaled_adamw_step (include/qfx.h, whose listing is the specification; the authors' package of
"Riemannian Preconditioned LoRA" was not at hand) -- the yardstick of tests/test_scaled_adamw_gpu.py; tests/test_scaled_adamw_cpu.py
checks the yardstick itself.  torch and numpy on the CPU, nothing here touches the code under test.

Per pair A [r, in], B [out, r]: gA = c g_A, gB = c g_B in fp32; G_B = B^T B + reg I and G_A = A A^T + reg I in fp64 from the widened
fp32 weights, every sum sequential in index order; P = G^-1 by torch.linalg.cholesky and torch.cholesky_solve in fp64; g^A =
fp32(P_B gA), g^B = fp32(gB P_A), each an fp64 sum over the r terms in index order, rounded once; then optim_ref.adamw_f32 -- the bits
of adamw_elem -- on g^ with clip 1.  reg is the fp32 image of the argument, as the kernel receives it.

`reverse=True` runs every fp64 sum (the two Gram matrices and the two products with P) in the opposite index order.  It exists to
measure the reference's own order noise: the largest distance between the two orders is the floor, and the GPU test's bar is twice
that (the project's rule for bars).  Distances are counted as optim_ref counts them, in fp32 ulps of each quantity's scale -- the sum
of the magnitudes of the addends that form it (optim_ref.adamw_f64), so that a cancelled first moment is not held to the ulp of its
small value."""
from __future__ import annotations

import numpy as np
import torch

import optim_ref as OR

F32, F64 = np.float32, np.float64
REG = 1e-6
QUANTITIES = ("p", "m", "v")


def osum(terms, reverse=False):
    """Sequential fp64 sum along the last axis in index order (reverse: from the last index down)."""
    n = terms.shape[-1]
    acc = torch.zeros(terms.shape[:-1], dtype=torch.float64)
    for k in (range(n - 1, -1, -1) if reverse else range(n)):
        acc = acc + terms[..., k]
    return acc


def gram(x, reg, reverse=False):
    """x [r, n] fp32 -> x x^T + reg I in fp64 (every product of two widened fp32 values is exact)."""
    x = torch.as_tensor(np.asarray(x, F32)).double()
    g = osum(x[:, None, :] * x[None, :, :], reverse)
    return g + float(F32(reg)) * torch.eye(x.shape[0], dtype=torch.float64)


def inverse(g):
    """G^-1 of an SPD fp64 matrix: Cholesky, then the two triangular solves on the identity.  None when the factorisation fails."""
    L, info = torch.linalg.cholesky_ex(g)
    if int(info) != 0 or not bool(torch.isfinite(L).all()):
        return None
    return torch.cholesky_solve(torch.eye(g.shape[0], dtype=torch.float64), L)


def preconditioned(A, B, gA, gB, reg=REG, reverse=False):
    """(g^A, g^B) fp32 of the listing from the clipped fp32 gradients, or None when a factorisation fails."""
    PB = inverse(gram(np.asarray(B, F32).T, reg, reverse))
    PA = inverse(gram(A, reg, reverse))
    if PA is None or PB is None:
        return None
    ga = torch.as_tensor(np.asarray(gA, F32)).double()
    gb = torch.as_tensor(np.asarray(gB, F32)).double()
    hA = osum(PB[:, None, :] * ga.T[None, :, :], reverse)        # [i, k, j]: P_B[i][j] gA[j][k]
    hB = osum(gb[:, None, :] * PA.T[None, :, :], reverse)        # [o, i, j]: gB[o][j] P_A[j][i]
    return hA.numpy().astype(F32), hB.numpy().astype(F32)


def hyper(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2):
    """fp32 images, as the tests of the other fp32 optimizers pass them: the wrapper forms 1 - beta^t from the double it is given,
    optim_ref.bias_corr from the fp32 image the kernel sees, and the two agree only for a beta that is its own image."""
    return {k: OR.f32img(x) for k, x in dict(lr=lr, b1=b1, b2=b2, eps=eps, wd=wd).items()}


def tensor_args(hp, t, lr_ratio=1.0, wd=None):
    """The scalars of one tensor's AdamW as the kernel holds them: fp32 images, lr_X = lr * lr_ratio_X in fp32."""
    a = OR.adamw_args(dict(hp, wd=hp["wd"] if wd is None else wd), t)
    a["lr"] = float(F32(a["lr"]) * F32(lr_ratio))
    return a


def pair_step(state, pair, hp, t, clip=1.0, reg=REG, precondition=True, reverse=False, scales=None):
    """One step of one pair in place on the flat fp32 arrays state = {"p", "g", "m", "v"}.  pair: (off_a, off_b, r, in, out, lr_ratio_a,
    lr_ratio_b, wd_a, wd_b).  Returns False when the pair is skipped (a non-finite g, a failed factorisation) and nothing was
    written.  scales: dict of flat fp64 arrays that receive the scale of every new p, m, v (optim_ref.adamw_f64)."""
    off_a, off_b, r, nin, nout, ra, rb, wa, wb = pair
    sa, sb = slice(off_a, off_a + r * nin), slice(off_b, off_b + nout * r)
    g = state["g"]
    if not (np.isfinite(g[sa]).all() and np.isfinite(g[sb]).all()):
        return False
    c = F32(clip)
    gA, gB = (g[sa] * c).astype(F32).reshape(r, nin), (g[sb] * c).astype(F32).reshape(nout, r)
    if precondition:
        h = preconditioned(state["p"][sa].reshape(r, nin), state["p"][sb].reshape(nout, r), gA, gB, reg, reverse)
        if h is None:
            return False
        gA, gB = h
    for s, gh, ratio, wd in ((sa, gA, ra, wa), (sb, gB, rb, wb)):
        a = tensor_args(hp, t, ratio, wd)
        old = (state["p"][s].copy(), state["m"][s].copy(), state["v"][s].copy())
        if scales is not None:
            f = OR.adamw_f64(old[0], gh.reshape(-1), old[1], old[2], 1.0, **a)
            for q in QUANTITIES:
                scales[q][s] = f[q][1]
        state["p"][s], state["m"][s], state["v"][s] = OR.adamw_f32(old[0], gh.reshape(-1), old[1], old[2], 1.0, **a)
    return True


def step(state, pairs, hp, t, clip=1.0, reg=REG, precondition=True, reverse=False, scales=None):
    """One launch: every pair of the table; returns the number of pairs skipped."""
    return sum(not pair_step(state, p, hp, t, clip, reg, precondition, reverse, scales) for p in pairs)


# ---------------------------------------------------------------- the GPU tests' data (shared with the CPU tests that measure the bar)
SHAPES = [(4, 32, 96), (16, 64, 33), (64, 96, 64), (1, 32, 1)]        # (r, in, out)
STEPS = 3


def pack(shapes, lead=3, gap=5, ratios=(1.0, 1.0), wds=(float(F32(1e-2)), float(F32(1e-2)))):
    """Pairs of `shapes` in one flat buffer, A then B of each, `gap` elements between tensors and `lead` in front: with the odd
    sizes among the shapes some offsets are 16-byte aligned and most are not.  Returns (pairs, n_elems)."""
    pairs, at = [], lead
    for r, nin, nout in shapes:
        off_a = at
        at += r * nin + gap
        off_b = at
        at += nout * r + gap
        pairs.append((off_a, off_b, r, nin, nout, ratios[0], ratios[1], wds[0], wds[1]))
    return pairs, at


def gaussian_state(pairs, n, seed=0, steps=STEPS):
    """Gaussian A, B (std 0.2: products of order one at these widths) and one Gaussian gradient per step (std 1e-2); moments zero;
    the slots between the tensors hold a sentinel that no launch may change."""
    rng = np.random.default_rng(seed)
    p = np.full(n, 7.0, F32)
    for off_a, off_b, r, nin, nout, *_ in pairs:
        p[off_a:off_a + r * nin] = (rng.standard_normal(r * nin) * 0.2).astype(F32)
        p[off_b:off_b + nout * r] = (rng.standard_normal(nout * r) * 0.2).astype(F32)
    grads = [(rng.standard_normal(n) * 1e-2).astype(F32) for _ in range(steps)]
    return dict(p=p, g=grads[0].copy(), m=np.zeros(n, F32), v=np.zeros(n, F32)), grads


def fresh_lora_state(pairs, n, seed=1, steps=STEPS):
    """What a fresh LoRA produces: B = 0 exactly and with it g_A = 0 (the gradient of A is B^T times something)."""
    st, grads = gaussian_state(pairs, n, seed, steps)
    for off_a, off_b, r, nin, nout, *_ in pairs:
        st["p"][off_b:off_b + nout * r] = 0.0
        for g in grads:
            g[off_a:off_a + r * nin] = 0.0
    st["g"] = grads[0].copy()
    return st, grads


RANK_DEFICIENT = dict(shape=(8, 64, 40), reg=1e-4)


def rank_deficient_state(seed=2, steps=STEPS):
    """A with two equal rows (r = 8): A A^T is singular and reg = 1e-4 alone makes G_A invertible (condition number about 1e5)."""
    pairs, n = pack([RANK_DEFICIENT["shape"]])
    st, grads = gaussian_state(pairs, n, seed, steps)
    off_a, _, r, nin, *_ = pairs[0]
    st["p"][off_a + 5 * nin:off_a + 6 * nin] = st["p"][off_a + 2 * nin:off_a + 3 * nin]
    return pairs, n, st, grads


def run(st, grads, pairs, hp, clip=1.0, reg=REG, precondition=True, reverse=False, want_scales=False):
    """STEPS steps from a copy of st on the given gradients; returns (state, scales of the last step or None, pairs skipped)."""
    st = {k: v.copy() for k, v in st.items()}
    scales = {q: np.zeros(st["p"].shape, F64) for q in QUANTITIES} if want_scales else None
    skipped = 0
    for t, g in enumerate(grads, 1):
        st["g"] = g.copy()
        skipped += step(st, pairs, hp, t, clip, reg, precondition, reverse, scales)
    return st, scales, skipped


def order_noise(st, grads, pairs, hp, reg=REG):
    """{quantity: the largest distance, in fp32 ulps of the quantity's scale, between the forward and the reversed order} after the
    run's steps."""
    fwd, scales, _ = run(st, grads, pairs, hp, reg=reg, want_scales=True)
    rev, _, _ = run(st, grads, pairs, hp, reg=reg, reverse=True)
    return {q: distance(rev[q], fwd[q], scales[q], pairs) for q in QUANTITIES}


def covered(pairs, n):
    mask = np.zeros(n, bool)
    for off_a, off_b, r, nin, nout, *_ in pairs:
        mask[off_a:off_a + r * nin] = True
        mask[off_b:off_b + nout * r] = True
    return mask


def distance(got, ref, scale, pairs):
    """Worst |got - ref| over the tensors of `pairs` in fp32 ulps of scale (optim_ref.err_ulps)."""
    mask = covered(pairs, len(ref))
    return OR.err_ulps(np.asarray(got, F64)[mask], np.asarray(ref, F64)[mask], scale[mask])


# The floors tests/test_scaled_adamw_cpu.py::test_bar_is_twice_the_references_own_order_noise measures on gaussian_state over
# pack(SHAPES) (and confirms on rank_deficient_state and fresh_lora_state): fp32 ulps of scale after three steps, forward against
# reversed sums.  Measured: 0 for all three -- the two orders move P by at most 2.4e-12 relative (the r = 64 pair, condition number
# 4e4), five orders below half an fp32 ulp, and not one of the 38k elements of g^ rounds the other way.  Twice 0 is 0: the kernel
# is held to the restatement's bits.
FLOORS = {"p": 0.0, "m": 0.0, "v": 0.0}
BARS = {q: 2.0 * x for q, x in FLOORS.items()}
