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


def sqrt_rn(x):
    """The correctly rounded square root, as the kernel's sqrtf is.  torch.sqrt on fp32 CPU tensors is a vectorised approximation
    that misses the correctly rounded value on part of its inputs -- how many, and which, depends on the machine; numpy's is the
    hardware instruction."""
    with np.errstate(all="ignore"):
        return torch.from_numpy(np.sqrt(x.detach().numpy()))


def _update(p, gs, m, v, K, fp32_form):
    fin = torch.isfinite(gs)
    m2 = m * K["b1"] + K["omb1"] * gs
    v2 = v * K["b2"] + K["omb2"] * (gs * gs) if fp32_form else v * K["b2"] + (K["omb2"] * gs) * gs
    p2 = p + K["step_size"] * (m2 / (sqrt_rn(v2) + K["eps_hat"]))
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
                _, st["_m64"], st["_v64"] = _update(pf.double(), gs.double(), m.double(), v.double(), K, False)     # the float64 twins
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


# ---------------------------------------------------------------- the exact comparison rule of the blockwise 8-bit kernels
# (shared by tests/lion_ref.py and tests/ademamix_ref.py).  A kernel is held to the fp32 restatement bit for bit wherever that is a
# statement about the kernel: the parameters, the block maxima and the fp32 moments of small tensors.  A stored code is the outcome
# of a comparison x > mid, and there the rule says which elements the comparison decides.
#
# Between the fp32 moment m and that comparison lie two rounded operations:
#   x^   = fl(m / mx)                   one division:         x^   = x   (1 + d1),  x = m / mx exactly
#   mid^ = fl(q[k] + q[k + 1]) / 2      one midpoint average: mid^ = mid (1 + d2),  the halving is exact
# Correctly rounded, |d1|, |d2| <= u = 2^-24.  x^ > mid^ and x > mid can differ only when |x - mid| <= |d1| |x| + |d2| |mid|.  The
# rule grants each operation a whole ulp (2u = EPS32: a division that is faithfully, not correctly, rounded), so an element is
# DECIDED when its margin min_k |x - mid_k| > EPS32 (|x| + |mid_k|), margin and midpoints evaluated in float64 (2^-53: nothing
# beside u).  The bound is relative and vanishes at zero with the quantities themselves.  The sign repair of a signed state is a
# further boundary at x = 0; it is taken on the sign BIT of m, which no operation rounds, so |x| > EPS32 |x| decides every m != 0,
# and m = +-0 is decided as well: 0 / mx is exact.  A block with maximum 0 performs no division: decided.
# A block is UNDECIDED, all its elements with it, when its maximum is tied: the float64 twin of the update (the same statement
# evaluated in double from the same decoded state) holds an element within TIE_ULPS fp32 ulp of the block's float64 maximum whose
# fp32 magnitude is not the block's fp32 maximum -- the two rounded apart, and one more rounding somewhere could name the other.
EPS32 = float(np.finfo(np.float32).eps)
TIE_ULPS = 4.0
UNDECIDED_CAP = 1e-4          # share of the compared elements per step that may be undecided (lion_ref.UNDECIDED_CAP is this)


def code_margin(m, mx, qmap, signed):
    """(margin, bound) in float64 per element: the distance of m / mx from the nearest boundary (a code midpoint; for a signed
    state also 0, the sign repair) and the rule's bound at that boundary.  mx: the block maximum per element, > 0."""
    x = m.double() / mx.double()
    q = qmap.double()
    mid = (q[:-1] + q[1:]) / 2.0
    k = torch.searchsorted(mid, x.contiguous(), side="left")
    margin = torch.full_like(x, float("inf"))
    bound = torch.zeros_like(x)
    for kk in ((k - 1).clamp(0, 254), k.clamp(0, 254)):
        b = mid[kk]
        d, lim = (x - b).abs(), EPS32 * (x.abs() + b.abs())
        closer = d - lim < margin - bound
        margin, bound = torch.where(closer, d, margin), torch.where(closer, lim, bound)
    if signed:
        d, lim = x.abs(), EPS32 * x.abs()
        closer = (d - lim < margin - bound) & (m != 0)
        margin, bound = torch.where(closer, d, margin), torch.where(closer, lim, bound)
    return margin, bound


def tied_blocks(m, m64, blk, n_blocks):
    """bool[n_blocks]: the blocks whose maximum is tied (see above).  m: the fp32 moments, m64: their float64 twins, blk: the block
    of every element."""
    a32, a64 = m.abs(), m64.abs()
    top32 = torch.zeros(n_blocks, dtype=a32.dtype).scatter_reduce_(0, blk, a32, "amax")
    top64 = torch.zeros(n_blocks, dtype=a64.dtype).scatter_reduce_(0, blk, a64, "amax")
    other = torch.where(a32 == top32[blk], torch.zeros_like(a64), a64)
    rival = torch.zeros(n_blocks, dtype=a64.dtype).scatter_reduce_(0, blk, other, "amax")
    return (rival > 0) & (rival >= top64 * (1.0 - TIE_ULPS * EPS32))


def undecided_codes(m, m64, blk, n_blocks, qmap, signed):
    """bool per element: True where the rule lets the stored code differ by one step.  Also returns the fp32 block maxima."""
    mx = torch.zeros(n_blocks, dtype=torch.float32).scatter_reduce_(0, blk, m.abs(), "amax")
    d = mx[blk]
    live = d > 0
    margin, bound = code_margin(m, torch.where(live, d, torch.ones_like(d)), qmap, signed)
    und = live & ~(margin > bound)
    return und | tied_blocks(m, m64, blk, n_blocks)[blk], mx


def sign_repaired(m, mx_elem, qmap1):
    """bool per element: the restatement takes the keep-the-sign branch of a signed state there."""
    live = mx_elem > 0
    x = torch.where(live, m / torch.where(live, mx_elem, torch.ones_like(mx_elem)), torch.zeros_like(m))
    return live & (torch.signbit(qmap1[quantize(x, qmap1)]) != torch.signbit(m))


def same_bits(a, b):
    a, b = (t.reshape(-1).clone(memory_format=torch.contiguous_format) for t in (a, b))      # (a one-element view keeps its parent's stride: clone, not contiguous)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def ulp_diff(a, b):
    """Largest distance of two fp32 tensors in units in the last place (finite values; 0 where the bits are equal)."""
    ia, ib = (t.contiguous().view(torch.int32).long() for t in (a, b))
    ia, ib = (torch.where(t < 0, -(t & 0x7FFFFFFF), t) for t in (ia, ib))
    return int((ia - ib).abs().max()) if a.numel() else 0


def check_codes(got, want, und, where):
    """The rule on one buffer of codes: identical on decided elements, within one step elsewhere.  Returns (decided mismatches,
    undecided elements that differ)."""
    got, want = got.reshape(-1).long(), want.reshape(-1).long()
    diff = got != want
    bad = int((diff & ~und).sum())
    assert bad == 0, (where, f"{bad} decided codes differ", torch.nonzero(diff & ~und).flatten()[:8].tolist())
    assert not diff.any() or int((got - want).abs().max()) <= 1, (where, "an undecided code is more than one step off")
    return bad, int(diff.sum())


# ---------------------------------------------------------------- the inputs tests/test_adam8bit_gpu.py (the kernel) and
# tests/test_blockwise8_cpu.py (the undecided census of the same steps, without a device) share
SIZES = [1000, 4096, 5000, 300, 9000, 20000, 64, 4100]      # a LoraStore-like flat buffer: tensors below 4096 elements, lengths that
KW = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_norm=1.0, grad_scale=0.5)      # are no multiple of a block size


def file_cases(bs):
    """(sizes, min_8bit_size, seed of the parameters, steps) of the two restatement tests of test_adam8bit_gpu.py: SIZES, and 259
    elements (8-bit, the last block short), exactly one block and 5 elements (fp32 moments) at min_8bit_size 256."""
    return {"sizes": (SIZES, 4096, 1, 5), "clipped": ([256 + 3, bs, 5], 256, 3, 3)}


def flat_offsets(sizes):
    offs, off = [], 0
    for k in sizes:
        offs.append(off)
        off += (k + 63) // 64 * 64
    return offs, off


def make_params(sizes, seed):
    torch.manual_seed(seed)
    return [torch.randn(k) * 0.1 for k in sizes]


def make_grads(sizes, it, bs):
    g = torch.Generator().manual_seed(100 + it)
    out = [torch.randn(k, generator=g) * (10.0 ** (i % 3 - 1)) for i, k in enumerate(sizes)]
    if sizes != SIZES:
        return out
    out[4][:bs] = 0.0                                   # an all-zero block (with zero state: absmax 0, the code of 0.0)
    if it == 2:
        out[2][17] = float("nan")
        out[5][3000] = float("inf")
    if it == 3:
        out[0][5] = float("-inf")                       # a small (fp32-moment) tensor
    return out


def gnorm_sq(grads):
    """Sum of squares of the finite gradient elements (what the tests hand both sides as the clip's norm)."""
    return float(sum(torch.nan_to_num(g.double(), nan=0.0, posinf=0.0, neginf=0.0).pow(2).sum() for g in grads))


def file_reference(which, bs):
    """The restatement and the gradients of one of file_cases: (opt, [(grads, gnorm_sq)]); the caller steps opt."""
    sizes, min8, seed, steps = file_cases(bs)[which]
    opt = Adam8bitRef(make_params(sizes, seed), lr=KW["lr"], betas=KW["betas"], eps=KW["eps"], weight_decay=KW["weight_decay"],
                      min_8bit_size=min8, blocksize=bs)
    steps = [(g, gnorm_sq(g)) for g in (make_grads(sizes, it, bs) for it in range(steps))]
    return opt, steps


def census(opt, bs):
    """(codes, undecided codes) of the step opt just took, by the rule above."""
    tot = n_und = 0
    for p, st in zip(opt.params, opt.state):
        if st["state1"].dtype != torch.uint8:
            continue
        blk = torch.arange(p.numel()) // bs
        for mk, qk, sg in (("_m", "qmap1", True), ("_v", "qmap2", False)):
            n_und += int(undecided_codes(st[mk], st[mk + "64"], blk, st["absmax1"].numel(), st[qk], sg)[0].sum())
            tot += p.numel()
    return tot, n_und
