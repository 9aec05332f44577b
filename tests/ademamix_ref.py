"""Numpy restatement of the AdEMAMix specification of include/qfx.h (qfx_ademamix_step / qfx_ademamix8bit_step), the yardstick of
csrc/qfx_ademamix.hip.  The listing in the header is the specification: it restates what bitsandbytes' 32-bit AdEMAMix kernel is
understood to compute (Pagliardini et al. 2024: Adam plus a slow gradient average m2 that enters the numerator with weight alpha;
decoupled multiplicative decay after the update; eps outside the corrected root) and was written without a copy of the package, so
parity with the package itself is unpinned; what is pinned is this statement.

  schedules(t)  alpha_t = alpha if t_alpha is None else min(t alpha / t_alpha, alpha)
                beta3_t = beta3 if t_beta3 is None else min(exp(ln b1 ln b3 / ((1 - s) ln b3 + s ln b1)), beta3),  s = t / t_beta3
  per element   g' = g clip;  m1 = m1 b1 + (1 - b1) g';  m2 = m2 beta3_t + (1 - beta3_t) g';  nu = nu b2 + ((1 - b2) g') g'
                p = p - lr ((m1 / (1 - b1^t) + alpha_t m2) / (sqrt(nu) / sqrt(1 - b2^t) + eps));  p = p (1 - lr wd) when wd > 0
                an element whose g' is not finite keeps p and its three states.

step64 evaluates it in double.  step32 rounds exactly as the kernel does: every scalar of the row is formed in double and rounded to
fp32 once (`row`), every operation of the listing is one numpy fp32 operation.  AdEMAMix8bitRef is the blockwise 8-bit form on
tests/bnb8_ref.py's quantiser: state1 holds m1 and m2 as two planes of signed-map codes with an absmax per plane and block, state2
is nu on the unsigned map; tensors below min_8bit_size keep fp32 states; the update uses the fp32 states, not their re-quantised
images.  adamw64 is bnb-style AdamW in double (decay after the update): AdEMAMix with alpha = 0."""
from __future__ import annotations

import math

import numpy as np
import torch

import bnb8_ref as B

F32, F64 = np.float32, np.float64
BETAS = (0.9, 0.999, 0.9999)
STATES = ("m1", "m2", "nu")


def alpha_t(t, alpha, t_alpha=None):
    return alpha if t_alpha is None else min(t * alpha / t_alpha, alpha)


def beta3_t(t, beta1, beta3, t_beta3=None):
    if t_beta3 is None:
        return beta3
    s = t / t_beta3
    l1, l3 = math.log(beta1), math.log(beta3)
    return min(math.exp(l1 * l3 / ((1 - s) * l3 + s * l1)), beta3)


def row(hp, t):
    """The scalars of step t (from 1) in double; hp: lr, betas (triple), eps, weight_decay, alpha, t_alpha, t_beta3."""
    b1, b2, b3 = hp["betas"]
    b3t = beta3_t(t, b1, b3, hp.get("t_beta3"))
    return dict(lr=hp["lr"], beta1=b1, beta2=b2, eps=hp["eps"], weight_decay=hp["weight_decay"], omb1=1 - b1, omb2=1 - b2, beta3_t=b3t,
                omb3=1 - b3t, alpha_t=alpha_t(t, hp.get("alpha", 5.0), hp.get("t_alpha")), bc1=1 - b1 ** t, sbc2=math.sqrt(1 - b2 ** t),
                decay=1 - hp["lr"] * hp["weight_decay"])


def row32(hp, t):
    """row rounded to the kernel's floats."""
    return {k: F32(v) for k, v in row(hp, t).items()}


def new_state(p, dtype=F64):
    return {k: np.zeros(np.shape(p), dtype) for k in STATES}


def _step(p, gs, st, K):
    """The listing, in the dtype of its inputs (numpy rounds every fp32 operation once; nothing is fused)."""
    with np.errstate(all="ignore"):
        fin = np.isfinite(gs)
        m1 = st["m1"] * K["beta1"] + K["omb1"] * gs
        m2 = st["m2"] * K["beta3_t"] + K["omb3"] * gs
        nu = st["nu"] * K["beta2"] + (K["omb2"] * gs) * gs
        pn = p - K["lr"] * ((m1 / K["bc1"] + K["alpha_t"] * m2) / (np.sqrt(nu) / K["sbc2"] + K["eps"]))
        if K["weight_decay"] > 0:
            pn = pn * K["decay"]
    st["m1"], st["m2"], st["nu"] = np.where(fin, m1, st["m1"]), np.where(fin, m2, st["m2"]), np.where(fin, nu, st["nu"])
    return np.where(fin, pn, p)


def step64(p, gs, st, hp, t):
    """One step in double: p, gs = g * clip (double) and the states are float64 arrays; returns the new p, updates st."""
    assert p.dtype == F64 and gs.dtype == F64
    return _step(p, gs, st, row(hp, t))


def step32(p, g, clip, st, hp, t):
    """One step as the kernel rounds it: p, g and the states float32, clip the fp32 coefficient; g' = g * clip is the first rounding."""
    assert p.dtype == F32 and g.dtype == F32 and all(st[k].dtype == F32 for k in STATES)
    with np.errstate(all="ignore"):
        gs = g * F32(clip)
    out = _step(p, gs, st, row32(hp, t))
    assert out.dtype == F32 and all(st[k].dtype == F32 for k in STATES)
    return out


def run64(p, grads, clips, hp):
    pp, st = np.array(p, F64), new_state(p, F64)
    for t, (g, c) in enumerate(zip(grads, clips), 1):
        pp = step64(pp, np.asarray(g, F64) * float(c), st, hp, t)
    return dict(st, p=pp)


def run32(p, grads, clips, hp):
    pp, st = np.array(p, F32), new_state(p, F32)
    for t, (g, c) in enumerate(zip(grads, clips), 1):
        pp = step32(pp, np.asarray(g, F32), c, st, hp, t)
    return dict(st, p=pp)


def adamw64(p, grads, lr, beta1, beta2, eps, weight_decay):
    """bnb-style AdamW in double: p -= lr (m / (1 - b1^t)) / (sqrt(v) / sqrt(1 - b2^t) + eps), then p *= 1 - lr wd."""
    p = np.array(p, F64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t, g in enumerate(grads, 1):
        g = np.asarray(g, F64)
        m = m * beta1 + (1 - beta1) * g
        v = v * beta2 + ((1 - beta2) * g) * g
        p = p - lr * ((m / (1 - beta1 ** t)) / (np.sqrt(v) / math.sqrt(1 - beta2 ** t) + eps))
        if weight_decay > 0:
            p = p * (1 - lr * weight_decay)
    return p, m, v


# ---------------------------------------------------------------- blockwise 8-bit
def _encode_signed(m, qmap1, bs):
    c, _, a, _ = B.encode(m, torch.zeros_like(m), qmap1, qmap1, bs)
    return c, a


class AdEMAMix8bitRef:
    """The 8-bit form over a list of fp32 CPU tensors (updated in place); per-parameter state in the file layout of
    optim_state.AdEMAMixBlockwiseState: state1 [2, *shape] (uint8 codes or fp32), absmax1 [2, blocks], state2, absmax2, qmap1, qmap2.
    `last` keeps, per 8-bit tensor, the fp32 states of the step just taken and the decoded ones it started from (diagnostics)."""

    def __init__(self, params, hp, min_8bit_size=4096, blocksize=256):
        self.params, self.hp, self.min_8bit_size, self.blocksize = params, hp, min_8bit_size, blocksize
        self.qmap1, self.qmap2 = B.create_dynamic_map(True), B.create_dynamic_map(False)
        self.state = [{} for _ in params]
        self.last = [None for _ in params]
        self.t = 0

    def _init(self, p, st):
        if p.numel() < self.min_8bit_size:
            st["state1"] = torch.zeros((2,) + tuple(p.shape), dtype=torch.float32)
            st["state2"] = torch.zeros_like(p, dtype=torch.float32)
        else:
            nb = (p.numel() + self.blocksize - 1) // self.blocksize
            st["state1"] = torch.zeros((2,) + tuple(p.shape), dtype=torch.uint8)
            st["state2"] = torch.zeros_like(p, dtype=torch.uint8)
            st["qmap1"], st["qmap2"] = self.qmap1.clone(), self.qmap2.clone()
            st["absmax1"] = torch.zeros(2, nb, dtype=torch.float32)
            st["absmax2"] = torch.zeros(nb, dtype=torch.float32)

    def decoded(self, i):
        """The fp32 states tensor i's next step starts from, as numpy."""
        p, st, bs = self.params[i], self.state[i], self.blocksize
        if not st:
            self._init(p, st)
        if st["state1"].dtype != torch.uint8:
            s1 = st["state1"].reshape(2, -1)
            return {"m1": s1[0].numpy().copy(), "m2": s1[1].numpy().copy(), "nu": st["state2"].reshape(-1).numpy().copy()}
        c = st["state1"].reshape(2, -1)
        return {"m1": B.dequant(c[0], st["qmap1"], st["absmax1"][0], bs).numpy(), "m2": B.dequant(c[1], st["qmap1"], st["absmax1"][1], bs).numpy(),
                "nu": B.dequant(st["state2"], st["qmap2"], st["absmax2"], bs).numpy()}

    def step(self, grads, clip=1.0, hps=None):
        """hps: one hp dict per tensor (parameter groups); None: self.hp for all."""
        self.t += 1
        for i, (p, g) in enumerate(zip(self.params, grads)):
            st, bs = self.state[i], self.blocksize
            before = self.decoded(i)
            s = {k: v.copy() for k, v in before.items()}
            pn = step32(p.reshape(-1).numpy().copy(), g.reshape(-1).numpy().astype(F32), clip, s, self.hp if hps is None else hps[i], self.t)
            if st["state1"].dtype != torch.uint8:
                st["state1"] = torch.from_numpy(np.stack([s["m1"], s["m2"]])).view((2,) + tuple(p.shape)).clone()
                st["state2"] = torch.from_numpy(s["nu"]).view(p.shape).clone()
            else:
                m1, m2, nu = (torch.from_numpy(s[k]) for k in STATES)
                c1, a1 = _encode_signed(m1, st["qmap1"], bs)
                c1b, a1b = _encode_signed(m2, st["qmap1"], bs)
                _, c2, _, a2 = B.encode(torch.zeros_like(nu), nu, st["qmap1"], st["qmap2"], bs)
                st["state1"] = torch.stack([c1, c1b]).view((2,) + tuple(p.shape))
                st["state2"] = c2.view(p.shape)
                st["absmax1"], st["absmax2"] = torch.stack([a1, a1b]), a2
                self.last[i] = {"before": before, "after": s}
            p.copy_(torch.from_numpy(pn).view(p.shape))

    def state_dict(self):
        return {i: dict({k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}, step=self.t) for i, st in enumerate(self.state) if st}
