"""CPU restatement of Lion with an fp32 moment and with bitsandbytes' blockwise 8-bit moment, the yardstick of the fused qfx_lion_step
and qfx_lion8bit_step.

Restated from the published algorithm -- Chen et al., "Symbolic Discovery of Optimization Algorithms" (2023) -- from
lion_pytorch.Lion.step and from bitsandbytes' optim.optimizer.Optimizer1State with the CUDA kernels kOptimizer32bit1State /
kOptimizerStatic8bit1StateBlockwise (LION branch).  Neither package is installed anywhere this project is tested, so parity with
the packages themselves is unpinned; what is pinned is this statement:

  * clip = grad_scale * min(1, max_norm / (sqrt(gnorm_sq) * grad_scale + 1e-6)) in fp32 (the fused AdamW step's prologue), g' = g clip;
  * 1 - b1, 1 - b2 and decay = 1 - lr wd are formed in fp32 from the fp32 images of lr, b1, b2, wd (bnb8_ref.step_scalars' way);
  * c = m b1 + (1 - b1) g'           two products and one sum, each rounded: never an FMA;
    p = p decay                      only when wd > 0: decoupled, BEFORE the update;
    p = p - lr sgn(c)                sgn(0) = 0, sgn(+-x) = +-1;
    m = m b2 + (1 - b2) g'           the same un-contracted form;
  * an element whose g' is not finite keeps p and m; the step count does not enter the arithmetic;
  * 8-bit tensor (numel >= min_8bit_size), blocks of `blocksize` consecutive elements, the last one short: m = qmap1[c1] absmax1[blk]
    is decoded, updated as above and stored as bnb8_ref stores state1 (absmax = max |m|, nearest code by the fp32 midpoints with ties
    to the lower code, then the keep-the-sign rule; a block with absmax 0 stores the code of 0.0).  The parameter update uses the
    fp32 m.  A tensor below min_8bit_size keeps an fp32 moment.  There is no second state.
Every fp32 operation is one torch op on fp32 tensors (one rounding each), in the kernels' order."""
from __future__ import annotations

import numpy as np
import torch

from bnb8_ref import UNDECIDED_CAP as B8_UNDECIDED_CAP
from bnb8_ref import blocks_absmax, clip_coef, create_dynamic_map, dequant, keep_sign, quantize

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)


def step_scalars(lr, b1, b2, wd):
    lr32, b1_32, b2_32, wd32 = (float(F32(x)) for x in (lr, b1, b2, wd))
    t32 = lambda x: torch.tensor(x, dtype=torch.float32)   # noqa: E731
    return dict(lr=t32(lr32), b1=t32(b1_32), b2=t32(b2_32), omb1=t32(F32(1.0) - F32(b1_32)), omb2=t32(F32(1.0) - F32(b2_32)),
                decay=t32(F32(1.0) - F32(lr32) * F32(wd32)), wd=wd32 > 0)


def update(p, gs, m, K):
    """(p, m, und) after one step of fp32 vectors p, m with the clipped gradient gs.  `und` marks the elements where this statement
    itself calls the sign of c undecided: |c| <= 4 eps32 (|m b1| + |(1 - b1) g'|) -- a last-bit difference in g' (the clip
    coefficient is formed once on the host here, once on the device there) can turn it.  Where both products are exactly zero
    (a zero gradient over a zero moment) c is exactly zero for any clip: that element is decided, sgn(0) = 0."""
    fin = torch.isfinite(gs)
    a = m * K["b1"]
    b = K["omb1"] * gs
    c = a + b
    p2 = p * K["decay"] if K["wd"] else p
    p2 = p2 - K["lr"] * torch.sign(c)
    m2 = m * K["b2"] + K["omb2"] * gs
    mag = a.abs() + b.abs()
    und = fin & (mag > 0) & (c.abs() <= 4.0 * EPS32 * mag)
    return torch.where(fin, p2, p), torch.where(fin, m2, m), und


def encode(m, qmap1, bs):
    """fp32 moment of one tensor -> (codes uint8, absmax)."""
    a1 = blocks_absmax(m, bs)
    d1 = a1[torch.arange(m.numel()) // bs]
    z1 = d1 > 0
    x1 = torch.where(z1, m / torch.where(z1, d1, torch.ones_like(d1)), torch.zeros_like(m))
    c1 = quantize(x1, qmap1)
    c1 = torch.where(z1, keep_sign(c1, m, qmap1), c1)
    return c1.to(torch.uint8), a1


def blocksize_of(st, numel):
    for bs in (256, 2048):
        if st["absmax1"].numel() == (numel + bs - 1) // bs:
            return bs
    raise ValueError("no block size fits")


class LionRef:
    """Lion over a list of fp32 CPU tensors (updated in place).  min_8bit_size=None: every moment in fp32, state in lion_pytorch's
    layout ({"exp_avg"}); otherwise bnb's Optimizer1State layout ({"step", "state1"[, "qmap1", "absmax1"]})."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0, min_8bit_size=None, blocksize=256):
        self.params = params
        self.group = dict(lr=lr, betas=tuple(betas), weight_decay=weight_decay)
        self.min_8bit_size, self.blocksize = min_8bit_size, blocksize
        self.qmap1 = create_dynamic_map(True)
        self.state = [{} for _ in params]
        self.undecided = [None for _ in params]       # per tensor, of the last step (test diagnostics)
        self.m64 = [None for _ in params]             # per 8-bit tensor, the float64 twin of the last step's moment (test diagnostics)

    def _init(self, p, st):
        if self.min_8bit_size is None:
            st["exp_avg"] = torch.zeros_like(p, dtype=torch.float32)
            return
        st["step"] = 0
        if p.numel() < self.min_8bit_size:
            st["state1"] = torch.zeros_like(p, dtype=torch.float32)
        else:
            st["state1"] = torch.zeros_like(p, dtype=torch.uint8)
            st["qmap1"] = self.qmap1.clone()
            st["absmax1"] = torch.zeros((p.numel() + self.blocksize - 1) // self.blocksize, dtype=torch.float32)

    def step(self, grads, gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
        G = self.group
        clip = torch.tensor(clip_coef(gnorm_sq, max_norm, grad_scale))
        K = step_scalars(G["lr"], G["betas"][0], G["betas"][1], G["weight_decay"])
        for i, (p, g, st) in enumerate(zip(self.params, grads, self.state)):
            if not st:
                self._init(p, st)
            gs = g.reshape(-1).float() * clip
            pf = p.reshape(-1)
            if "exp_avg" in st:
                pn, m, und = update(pf, gs, st["exp_avg"].reshape(-1), K)
                st["exp_avg"] = m.view(p.shape).clone()
            elif st["state1"].dtype != torch.uint8:
                st["step"] += 1
                pn, m, und = update(pf, gs, st["state1"].reshape(-1), K)
                st["state1"] = m.view(p.shape).clone()
            else:
                st["step"] += 1
                bs = blocksize_of(st, p.numel())
                m = dequant(st["state1"], st["qmap1"], st["absmax1"], bs)
                self.m64[i] = update(pf.double(), gs.double(), m.double(), K)[1]      # the float64 twin (bnb8_ref.tied_blocks)
                pn, m, und = update(pf, gs, m, K)
                c1, a1 = encode(m, st["qmap1"], bs)
                st["state1"], st["absmax1"] = c1.view(p.shape), a1
                st["_m"] = m                         # the fp32 moment of this step (test diagnostics; not part of bnb's state)
            self.undecided[i] = und
            p.copy_(pn.view(p.shape))

    def state_dict(self):
        state = {i: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items() if not k.startswith("_")}
                 for i, st in enumerate(self.state) if st}
        return {"state": state, "param_groups": [dict(self.group, params=list(range(len(self.params))))]}


# ---- the inputs tests/test_lion_cpu.py (the near-cancellation census) and tests/test_lion_gpu.py (the kernels) share: a LoraStore-like
# flat buffer with tensors below 4096 elements, lengths that are no multiple of either block size, 64-element slots
SIZES = [1000, 4096, 5000, 300, 9000, 20000, 64, 4100]
STEPS = 5
KW = dict(lr=1e-3, betas=(0.9, 0.99), max_norm=1.0, grad_scale=0.5)
UNDECIDED_CAP = B8_UNDECIDED_CAP          # share of the compared elements per step that may be undecided (1e-4, all three families)


def flat_offsets(sizes):
    offs, off = [], 0
    for k in sizes:
        offs.append(off)
        off += (k + 63) // 64 * 64
    return offs, off


def make_params(sizes=SIZES, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(k, generator=g) * 0.1 for k in sizes]


def make_grads(sizes, it, bs):
    g = torch.Generator().manual_seed(100 + it)
    out = [torch.randn(k, generator=g) * (10.0 ** (i % 3 - 1)) for i, k in enumerate(sizes)]
    if sizes != SIZES:
        return out
    out[4][:bs] = 0.0                                   # an all-zero block over zero state: sgn(0) = 0, absmax 0, the code of 0.0
    if it == 2:
        out[2][17] = float("nan")                       # 8-bit tensors
        out[5][3000] = float("inf")
    if it == 3:
        out[0][5] = float("-inf")                       # a small (fp32-moment) tensor
    return out


def gnorm_sq(grads):
    """Sum of squares of the finite gradient elements (what the test hands both sides as the clip's norm)."""
    return float(sum(torch.nan_to_num(g.double(), nan=0.0, posinf=0.0, neginf=0.0).pow(2).sum() for g in grads))


def run_reference(bs, weight_decay):
    """STEPS steps of the restatement on SIZES; bs=None: every moment fp32 (lion_pytorch's layout), else bnb's layout with that block
    size and min_8bit_size 4096.  Returns one record per step: the gradients, gnorm_sq, deep copies of parameters and state before
    and after the step, and the undecided masks.  Computed once per (bs, weight_decay) and never modified by its users."""
    key = (bs, weight_decay)
    if key not in _RUNS:
        opt = LionRef(make_params(), lr=KW["lr"], betas=KW["betas"], weight_decay=weight_decay,
                      min_8bit_size=None if bs is None else 4096, blocksize=bs or 256)
        snap = lambda: ([p.clone() for p in opt.params],   # noqa: E731
                        [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()} for st in opt.state])
        recs = []
        for it in range(STEPS):
            grads = make_grads(SIZES, it, bs or 256)
            gsq = gnorm_sq(grads)
            assert gsq * KW["grad_scale"] ** 2 > 1.0                    # the clip is active
            before = snap()
            opt.step([g.clone() for g in grads], gnorm_sq=gsq, max_norm=KW["max_norm"], grad_scale=KW["grad_scale"])
            recs.append(dict(grads=grads, gsq=gsq, before=before, after=snap(), undecided=[u.clone() for u in opt.undecided],
                             m64=[None if t is None else t.clone() for t in opt.m64]))
        _RUNS[key] = recs
    return _RUNS[key]


_RUNS = {}
