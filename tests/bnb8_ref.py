"""CPU restatement of bitsandbytes' blockwise 8-bit Adam (Adam8bit / AdamW8bit), the yardstick of the fused qfx_adam8bit_step.

Restated from the published algorithm -- Dettmers et al., "8-bit Optimizers via Block-wise Quantization" (ICLR 2022) -- and
bitsandbytes 0.45's functional.create_dynamic_map, optim.optimizer.Optimizer2State and the CUDA kernels kOptimizer32bit2State /
kOptimizer8bit2StateBlockwise (ADAM branch) with their quantize_2D.  The package is not installed anywhere this project is tested, so
parity with the package itself is unpinned; what is pinned is this statement:

  * code books: create_dynamic_map(signed, max_exponent_bits=7, total_bits=8), 256 sorted fp32 values each (qmap1 signed, qmap2
    unsigned);
  * clip = grad_scale * min(1, max_norm / (sqrt(gnorm_sq) * grad_scale + 1e-6)) in fp32 (the fused AdamW step's prologue), g' = g clip;
  * 8-bit tensor (numel >= min_8bit_size), blocks of `blocksize` consecutive elements, the last one short:
      m = qmap1[c1] absmax1[blk], v = qmap2[c2] absmax2[blk];  m = m b1 + (1-b1) g';  v = v b2 + ((1-b2) g') g'
    fp32 tensor: m = m b1 + (1-b1) g';  v = v b2 + (1-b2) (g' g')
    p = p + step_size (m / (sqrt(v) + eps_hat)), step_size = -lr sqrt(1-b2^t)/(1-b1^t), eps_hat = eps sqrt(1-b2^t) (double, then
    fp32); p = p (1 - lr wd) when wd > 0 -- decoupled, after the update, with the fp32 (not re-quantised) moments;
  * an element whose g' is not finite keeps p and its moments (bnb's kernels skip the parameter update there; its 8-bit kernel would
    fold the value into the block's moments, this statement keeps one bad element from poisoning its block);
  * absmax = max |m| (|v|) over the block; code = number of fp32 midpoints (q[k] + q[k+1]) / 2 below m / absmax, i.e. the nearest
    code with a tie going to the LOWER one (bnb's quantize_2D decides ties by its search path); state1 then keeps its sign (bnb: a code
    whose value has the other sign bit than m moves one index towards m); a block with absmax 0 stores the code of 0.0.
Every fp32 operation is one torch op on fp32 tensors (one rounding each), in the kernel's order."""
from __future__ import annotations

import math

import numpy as np
import torch

F32 = np.float32


def create_dynamic_map(signed=True, max_exponent_bits=7, total_bits=8):
    data = []
    non_sign_bits = total_bits - 1
    additional_items = 2 ** (non_sign_bits - max_exponent_bits) - 1
    assert additional_items == 0
    for i in range(max_exponent_bits):
        fraction_items = int(2 ** (i + non_sign_bits - max_exponent_bits) + 1 if signed
                             else 2 ** (i + non_sign_bits - max_exponent_bits + 1) + 1)
        boundaries = torch.linspace(0.1, 1, fraction_items, dtype=torch.float32)
        means = (boundaries[:-1] + boundaries[1:]) / 2.0
        data += ((10 ** (-(max_exponent_bits - 1) + i)) * means).tolist()
        if signed:
            data += (-(10 ** (-(max_exponent_bits - 1) + i)) * means).tolist()
    data.append(0)
    data.append(1.0)
    assert len(data) == 2 ** total_bits
    data.sort()
    return torch.tensor(data, dtype=torch.float32)


def midpoints(qmap):
    return (qmap[:-1] + qmap[1:]) / 2.0


def quantize(x, qmap):
    """Nearest code by the fp32 midpoints, ties to the lower code (int64 codes)."""
    return torch.searchsorted(midpoints(qmap), x.contiguous(), side="left")


def keep_sign(codes, m, qmap1):
    """bnb's state1 rule after quantising: a code whose value has the other sign bit than the moment moves one index towards it."""
    flip = torch.signbit(qmap1[codes]) != torch.signbit(m)
    step = torch.where(m > 0, 1, -1)
    return torch.where(flip, (codes + step).clamp(0, 255), codes)


def clip_coef(gnorm_sq, max_norm, grad_scale):
    clip = F32(grad_scale)
    if gnorm_sq is not None and max_norm > 0:
        nrm = np.sqrt(F32(gnorm_sq)) * F32(grad_scale)
        c = F32(max_norm) / (nrm + F32(1e-6))
        clip = clip * (c if c < F32(1.0) else F32(1.0))
    return F32(clip)


def step_scalars(lr, b1, b2, eps, wd, t):
    lr32, b1_32, b2_32, eps32, wd32 = (float(F32(x)) for x in (lr, b1, b2, eps, wd))
    c1 = 1.0 - math.pow(b1_32, t)
    c2 = math.sqrt(1.0 - math.pow(b2_32, t))
    t32 = lambda x: torch.tensor(x, dtype=torch.float32)   # noqa: E731
    return dict(b1=t32(b1_32), b2=t32(b2_32), omb1=t32(F32(1.0) - F32(b1_32)), omb2=t32(F32(1.0) - F32(b2_32)),
                step_size=t32(F32(-lr32 * c2 / c1)), eps_hat=t32(F32(eps32 * c2)), decay=t32(F32(1.0) - F32(lr32) * F32(wd32)),
                wd=wd32 > 0)


def _update(p, gs, m, v, K, fp32_form):
    fin = torch.isfinite(gs)
    m2 = m * K["b1"] + K["omb1"] * gs
    v2 = v * K["b2"] + K["omb2"] * (gs * gs) if fp32_form else v * K["b2"] + (K["omb2"] * gs) * gs
    p2 = p + K["step_size"] * (m2 / (torch.sqrt(v2) + K["eps_hat"]))
    if K["wd"]:
        p2 = p2 * K["decay"]
    return torch.where(fin, p2, p), torch.where(fin, m2, m), torch.where(fin, v2, v)


def blocks_absmax(x, bs):
    n = x.numel()
    nb = (n + bs - 1) // bs
    pad = torch.zeros(nb * bs, dtype=x.dtype)
    pad[:n] = x.abs()
    return pad.view(nb, bs).amax(1)


def dequant(codes, qmap, absmax, bs):
    blk = torch.arange(codes.numel()) // bs
    return qmap[codes.reshape(-1).long()] * absmax[blk]


def encode(m, v, qmap1, qmap2, bs):
    """fp32 moments of one tensor -> (codes1 uint8, codes2 uint8, absmax1, absmax2)."""
    a1, a2 = blocks_absmax(m, bs), blocks_absmax(v, bs)
    blk = torch.arange(m.numel()) // bs
    d1, d2 = a1[blk], a2[blk]
    z1, z2 = d1 > 0, d2 > 0
    x1 = torch.where(z1, m / torch.where(z1, d1, torch.ones_like(d1)), torch.zeros_like(m))
    x2 = torch.where(z2, v / torch.where(z2, d2, torch.ones_like(d2)), torch.zeros_like(v))
    c1 = quantize(x1, qmap1)
    c1 = torch.where(z1, keep_sign(c1, m, qmap1), c1)
    c2 = quantize(x2, qmap2)
    return c1.to(torch.uint8), c2.to(torch.uint8), a1, a2


class Adam8bitRef:
    """bnb's Optimizer2State over a list of fp32 CPU tensors (updated in place), state in bnb's per-parameter layout."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, min_8bit_size=4096, blocksize=256):
        self.params = params
        self.group = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        self.min_8bit_size, self.blocksize = min_8bit_size, blocksize
        self.qmap1, self.qmap2 = create_dynamic_map(True), create_dynamic_map(False)
        self.state = [{} for _ in params]

    def _init(self, p, st):
        st["step"] = 0
        if p.numel() < self.min_8bit_size:
            st["state1"] = torch.zeros_like(p, dtype=torch.float32)
            st["state2"] = torch.zeros_like(p, dtype=torch.float32)
        else:
            nb = (p.numel() + self.blocksize - 1) // self.blocksize
            st["state1"] = torch.zeros_like(p, dtype=torch.uint8)
            st["state2"] = torch.zeros_like(p, dtype=torch.uint8)
            st["qmap1"], st["qmap2"] = self.qmap1.clone(), self.qmap2.clone()
            st["absmax1"] = torch.zeros(nb, dtype=torch.float32)
            st["absmax2"] = torch.zeros(nb, dtype=torch.float32)

    def step(self, grads, gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
        G = self.group
        clip = torch.tensor(clip_coef(gnorm_sq, max_norm, grad_scale))
        for p, g, st in zip(self.params, grads, self.state):
            if not st:
                self._init(p, st)
            st["step"] += 1
            K = step_scalars(G["lr"], G["betas"][0], G["betas"][1], G["eps"], G["weight_decay"], st["step"])
            gs = g.reshape(-1).float() * clip
            pf = p.reshape(-1)
            if st["state1"].dtype != torch.uint8:
                pn, m, v = _update(pf, gs, st["state1"].reshape(-1), st["state2"].reshape(-1), K, True)
                st["state1"], st["state2"] = m.view(p.shape).clone(), v.view(p.shape).clone()
            else:
                bs = blocksize_of(st, p.numel())
                m = dequant(st["state1"], st["qmap1"], st["absmax1"], bs)
                v = dequant(st["state2"], st["qmap2"], st["absmax2"], bs)
                pn, m, v = _update(pf, gs, m, v, K, False)
                c1, c2, a1, a2 = encode(m, v, st["qmap1"], st["qmap2"], bs)
                st["state1"], st["state2"] = c1.view(p.shape), c2.view(p.shape)
                st["absmax1"], st["absmax2"] = a1, a2
                st["_m"], st["_v"] = m, v            # the fp32 moments of this step (test diagnostics; not part of bnb's state)
            p.copy_(pn.view(p.shape))

    def state_dict(self):
        state = {i: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items() if not k.startswith("_")}
                 for i, st in enumerate(self.state) if st}
        return {"state": state, "param_groups": [dict(self.group, params=list(range(len(self.params))))]}


def blocksize_of(st, numel):
    for bs in (256, 2048):
        if st["absmax1"].numel() == (numel + bs - 1) // bs:
            return bs
    raise ValueError("no block size fits")
