"""CPU restatement of Schedule-Free AdamW, the yardstick of the fused qfx_sfadamw_step and qfx_sf_swap (include/qfx.h).

Restated from the published method -- Defazio et al., "The Road Less Scheduled" (2024) -- and from the arithmetic of
schedulefree.AdamWScheduleFree.step / .eval / .train.  The package is not installed where this was written: parity with the
package itself is pinned only by test_schedulefree_cpu.py::test_restatement_matches_the_package, which skips without it; what is
pinned without it are the paper's invariants in the same file.

Per group and step k (from 0), in Python doubles as the package forms them (host_scalars):
    sched = (k + 1) / warmup_steps if k < warmup_steps else 1;  bc2 = 1 - beta2^(k + 1);  lr_t = lr sched;  lr_max = max(lr_t, lr_max)
    weight = (k + 1)^r lr_max^weight_lr_power;  weight_sum += weight;  ckp1 = weight / weight_sum (0 when weight_sum == 0)
    ylr = lr_t (beta1 (1 - ckp1) - 1)
Per element on tensors of `dtype` (update): every operation is one torch operation, so float32 restates the kernel rounding by
rounding and float64 is the yardstick both are measured against (the tolerance rule, tolerance()).  Scalars are cast to `dtype`
where they meet a tensor, as torch casts a Python scalar:
    g' = g clip                                  clip = grad_scale min(1, max_norm / (sqrt(gnorm_sq) grad_scale + 1e-6)), the fused AdamW's
    v  = v beta2 + ((1 - beta2) g') g'
    gn = g' / (sqrt(v / bc2) + eps)
    gn = gn + weight_decay y                     only when weight_decay != 0
    y  = lerp(y, z, ckp1);  y = y + ylr gn;  z = z - lr_t gn
with z = y and v = 0 on the first step, lerp(a, b, w) = a + w (b - a) for |w| < 0.5, else b - (b - a)(1 - w) (torch.lerp), and no
non-finite guard.  beta2 enters as its fp32 image in BOTH precisions and 1 - beta2 is formed from that image: the C ABI carries
beta2 as a float, and 1 - beta2 amplifies its rounding a thousandfold (the fused AdamW step forms 1 - beta2 the same way).  For a
beta2 that fp32 represents exactly this is the package's arithmetic to the bit.
eval(): y -> x = lerp(y, z, 1 - 1 / beta1);  train(): x -> y = lerp(x, z, 1 - beta1);  each a no-op in its own mode; step() in eval
mode raises.  train_mode starts True here (the package's releases differ: call train() before the first step with any of them)."""
from __future__ import annotations

import math

import numpy as np
import torch

F32 = np.float32
DEFAULTS = dict(lr=0.0025, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, warmup_steps=0, r=0.0, weight_lr_power=2.0)
PARAM_KEYS = {"z", "exp_avg_sq"}
GROUP_KEYS = {"lr", "betas", "eps", "weight_decay", "warmup_steps", "r", "weight_lr_power", "k", "train_mode", "weight_sum", "lr_max",
              "scheduled_lr", "foreach"}


def cast(x, dtype):
    """A Python scalar as it meets a tensor of `dtype`."""
    return float(F32(x)) if dtype == torch.float32 else float(x)


def host_scalars(group):
    """Advance the group's running scalars by one step (k itself is advanced by the caller) -> (lr_t, bc2, ckp1, ylr)."""
    k, warmup = group["k"], group["warmup_steps"]
    sched = (k + 1) / warmup if k < warmup else 1.0
    bc2 = 1 - group["betas"][1] ** (k + 1)
    lr_t = group["lr"] * sched
    group["scheduled_lr"] = lr_t
    lr_max = group["lr_max"] = max(lr_t, group["lr_max"])
    weight = ((k + 1) ** group["r"]) * (lr_max ** group["weight_lr_power"])
    weight_sum = group["weight_sum"] = group["weight_sum"] + weight
    ckp1 = weight / weight_sum if weight_sum != 0 else 0.0
    return lr_t, bc2, ckp1, lr_t * (group["betas"][0] * (1 - ckp1) - 1)


def clip_coef(gnorm_sq, max_norm, grad_scale, dtype):
    """qfx_adamw_step's clip prologue: in fp32 as the kernel rounds it, or in double."""
    if dtype == torch.float32:
        clip = F32(grad_scale)
        if gnorm_sq is not None and max_norm > 0:
            c = F32(max_norm) / (np.sqrt(F32(gnorm_sq)) * F32(grad_scale) + F32(1e-6))
            clip = clip * (c if c < F32(1.0) else F32(1.0))
        return float(F32(clip))
    clip = float(grad_scale)
    if gnorm_sq is not None and max_norm > 0:
        clip *= min(1.0, max_norm / (math.sqrt(float(F32(gnorm_sq))) * grad_scale + 1e-6))
    return clip


def lerp(a, b, w):
    """torch.lerp's formula with a scalar weight, one torch operation per rounding."""
    dt = a.dtype
    w = cast(w, dt)
    d = b - a
    return a + w * d if abs(w) < 0.5 else b - d * cast(1.0 - w, dt)


def update(y, gs, z, v, beta2, eps, weight_decay, lr_t, bc2, ckp1, ylr):
    """(y, z, v) after one step on the clipped gradient gs; z = None: the first step."""
    dt = y.dtype
    b2 = float(F32(beta2))                       # the fp32 image in both precisions
    if z is None:
        z, v = y.clone(), torch.zeros_like(y)
    v = v * b2 + ((1.0 - b2) * gs) * gs
    gn = gs / ((v / cast(bc2, dt)).sqrt() + cast(eps, dt))
    if weight_decay != 0:
        gn = gn + cast(weight_decay, dt) * y
    y = lerp(y, z, ckp1)
    y = y + cast(ylr, dt) * gn
    z = z - cast(lr_t, dt) * gn
    return y, z, v


class SFRef:
    """Schedule-Free AdamW over a list of CPU tensors of one dtype (float32 or float64), updated in place; state and group in the
    package's layout."""

    def __init__(self, params, **kw):
        unknown = set(kw) - set(DEFAULTS)
        if unknown:
            raise TypeError(f"unexpected keywords {sorted(unknown)}")
        self.params = params
        self.group = dict(DEFAULTS, **kw)
        self.group["betas"] = tuple(self.group["betas"])
        self.group.update(k=0, train_mode=True, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0, foreach=True)
        self.state = [{} for _ in params]

    def step(self, grads, gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
        G = self.group
        if not G["train_mode"]:
            raise RuntimeError("step() in eval mode: call train() first")
        lr_t, bc2, ckp1, ylr = host_scalars(G)
        for p, g, st in zip(self.params, grads, self.state):
            gs = g.to(p.dtype) * clip_coef(gnorm_sq, max_norm, grad_scale, p.dtype)
            y, z, v = update(p, gs, st.get("z"), st.get("exp_avg_sq"), G["betas"][1], G["eps"], G["weight_decay"], lr_t, bc2, ckp1, ylr)
            p.copy_(y)
            st["z"], st["exp_avg_sq"] = z, v
        G["k"] += 1

    def _swap(self, train):
        G = self.group
        if G["train_mode"] == train:
            return
        b1 = G["betas"][0]
        for p, st in zip(self.params, self.state):
            if "z" in st:
                p.copy_(lerp(p, st["z"], 1 - b1 if train else 1 - 1 / b1))
        G["train_mode"] = train

    def eval(self):
        self._swap(False)

    def train(self):
        self._swap(True)

    def state_dict(self):
        state = {i: {k: v.clone() for k, v in st.items()} for i, st in enumerate(self.state) if st}
        return {"state": state, "param_groups": [dict(self.group, params=list(range(len(self.params))))]}


def tolerance(ref32, ref64):
    """The tolerance rule of one buffer: (bound, the fp32 restatement's own largest error against the fp64 run).  The kernel's
    largest absolute error against the fp64 run may be at most 4 times that error -- the factor covers the different rounding of
    division and square root between the CPU and the device, nothing more -- plus one fp32 ulp of the buffer's largest magnitude."""
    own = (ref32.double() - ref64).abs().max().item()
    ulp = float(np.spacing(F32(ref64.abs().max().item())))
    return 4.0 * own + ulp, own


def check(name, got, ref32, ref64, where=""):
    """Assert the tolerance rule for one buffer; both measured errors go into the message and are printed."""
    bound, own = tolerance(ref32, ref64)
    err = (got.double().cpu() - ref64).abs().max().item()
    msg = f"{where} {name}: kernel error {err:.3e} against fp64, fp32 restatement's own error {own:.3e}, bound {bound:.3e}"
    print(msg)
    assert torch.isfinite(got).all() and err <= bound, msg


# ---- the inputs the kernel tests share
def make_inputs(n, steps, seed=3):
    """y [n], `steps` gradients whose scale alternates so that the clip (max_norm 1, grad_scale 0.5) is active on the even steps
    and inactive on the odd ones, and each gradient's sum of squares as the fp32 value both sides are handed."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(n, generator=g) * 0.1
    grads = [torch.randn(n, generator=g) * (1.0 if it % 2 == 0 else 0.5 / math.sqrt(n)) for it in range(steps)]
    gsq = [float(F32(float(t.double().pow(2).sum()))) for t in grads]
    return y, grads, gsq


def run(y, grads, gsq, dtype, max_norm=1.0, grad_scale=0.5, **kw):
    """The restatement over the given steps in `dtype` -> one (y, z, v) snapshot per step."""
    p = y.to(dtype).clone()
    opt = SFRef([p], **kw)
    out = []
    for g, s in zip(grads, gsq):
        opt.step([g], gnorm_sq=s, max_norm=max_norm, grad_scale=grad_scale)
        out.append((p.clone(), opt.state[0]["z"].clone(), opt.state[0]["exp_avg_sq"].clone()))
    return out
