"""One step of the three blockwise 8-bit families (Adam, Lion, AdEMAMix) from ANY given state, restated over the whole flat buffer at
once, and the inputs tests/test_blockwise8_cpu.py and tests/test_blockwise8_gpu.py share.

The arithmetic is not restated here: the element updates are bnb8_ref._update, lion_ref.update and ademamix_ref._step / step32, the
quantiser is bnb8_ref's, and the comparison rule (decided / undecided codes, tied block maxima) is bnb8_ref's.  What this module
adds is the layout: a host image (`Flat`) of exactly the buffers a launch gets -- p, g, one code plane, one absmax array and one
fp32 moment array per state -- with canary words wherever the block table names no element, so that comparing the whole buffers
bit for bit checks the step and every canary together.  States per family: adam (m signed, v unsigned), lion (m signed), ademamix
(m1 signed, m2 signed, nu unsigned)."""
from __future__ import annotations

import math

import numpy as np
import torch

import ademamix_ref as AR
import bnb8_ref as B
import lion_ref as LR

F32, F64 = np.float32, np.float64
GUARD, CANARY, CANARY8 = 64, 12345.0, 77
FAMILIES = ("adam", "lion", "ademamix")
PLANES = {"adam": (True, False), "lion": (True,), "ademamix": (True, True, False)}      # per state: on the signed map?
QMAP = {True: B.create_dynamic_map(True), False: B.create_dynamic_map(False)}
ZERO_CODE = {sg: int(torch.searchsorted(QMAP[sg], torch.tensor(0.0))) for sg in (True, False)}      # 127 / 0
TINY = float(np.finfo(np.float32).tiny)

# three rows per family: the plain entry takes row 0, the grouped entry all three
HPS = {
    "adam": [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01), dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0),
             dict(lr=5e-4, betas=(0.95, 0.98), eps=1e-8, weight_decay=0.02)],
    "lion": [dict(lr=1e-3, betas=(0.9, 0.99), weight_decay=0.01), dict(lr=2e-3, betas=(0.8, 0.95), weight_decay=0.0),
             dict(lr=5e-4, betas=(0.95, 0.98), weight_decay=0.02)],
    "ademamix": [dict(lr=0.01, betas=AR.BETAS, eps=1e-8, weight_decay=0.01, alpha=5.0, t_alpha=3, t_beta3=4),
                 dict(lr=0.02, betas=(0.8, 0.99, 0.999), eps=1e-6, weight_decay=0.0, alpha=2.0, t_alpha=None, t_beta3=None),
                 dict(lr=0.005, betas=(0.95, 0.98, 0.9995), eps=1e-8, weight_decay=0.02, alpha=8.0, t_alpha=2, t_beta3=None)],
}


class Flat:
    """Host image of one launch's buffers: p, g fp32[n]; codes uint8[P, n]; the block maxima and the fp32 moments as raw 1-D arrays
    (absmax_raw, m32_raw) of GUARD canary words followed by P planes of n_absmax + GUARD (n_fp32 + GUARD) words each.  `absmax` and
    `m32` are the [P, plane] views behind the front canaries -- what a launch is handed -- so every plane has canary words before
    and behind it, and comparing the raw arrays compares them all."""

    def __init__(self, p, g, codes, absmax_raw, m32_raw):
        self.p, self.g, self.codes, self.absmax_raw, self.m32_raw = p, g, codes, absmax_raw, m32_raw
        P = codes.shape[0]
        self.absmax, self.m32 = absmax_raw[GUARD:].view(P, -1), m32_raw[GUARD:].view(P, -1)

    def clone(self):
        return Flat(*(t.clone() for t in self.buffers()))

    def buffers(self):
        return self.p, self.g, self.codes, self.absmax_raw, self.m32_raw


class Index:
    """Per element of every tensor of a block table (ops.Adam8bitLayout), in table order: its position in the flat buffers, its mode,
    its absmax slot (8-bit) or its place in the fp32 moments, and its tensor."""

    def __init__(self, lay):
        bs = lay.blocksize
        pos, eight, blk, sidx, tid = [], [], [], [], []
        for i, (off, k, e8, a0, nb, s0) in enumerate(lay.tensors):
            r = np.arange(k, dtype=np.int64)
            pos.append(off + r)
            eight.append(np.full(k, bool(e8)))
            blk.append(a0 + r // bs if e8 else np.zeros(k, np.int64))
            sidx.append(np.zeros(k, np.int64) if e8 else s0 + r)
            tid.append(np.full(k, i, np.int64))
        self.pos, self.eight, self.blk, self.sidx, self.tid = (torch.from_numpy(np.concatenate(x)) for x in (pos, eight, blk, sidx, tid))
        self.n_tensors = len(lay.tensors)


def place(sizes, align=None):
    """[(offset, numel)] and the buffer length: the first tensor behind GUARD canary words, at least one canary word between two
    tensors, every offset a multiple of 4 (what the block-table builder accepts); align[i]: the offset of tensor i modulo 64."""
    off, entries = GUARD, []
    for i, k in enumerate(sizes):
        off = (off + 3) // 4 * 4
        if align is not None:
            off += (align[i] - off) % 64
        entries.append((off, k))
        off += k + 1
    return entries, (off + GUARD + 63) // 64 * 64


def new_flat(fam, lay, n):
    P = len(PLANES[fam])
    return Flat(torch.full((n,), CANARY), torch.full((n,), CANARY), torch.full((P, n), CANARY8, dtype=torch.uint8),
                torch.full((GUARD + P * (lay.n_absmax + GUARD),), CANARY), torch.full((GUARD + P * (lay.n_fp32 + GUARD),), CANARY))


def clip_of(clipargs):
    gsq, max_norm, grad_scale = clipargs
    return B.clip_coef(gsq, max_norm, grad_scale)


def _update(fam, p, g, clip, olds, eight, hp, t):
    """The family's element update on fp32 vectors -> (p, [states], [float64 twins of the states], undecided-parameter mask or None,
    for Lion the three parameters sgn(c) = -1, 0, +1 would give or None)."""
    gs = g * torch.tensor(clip)
    d = [o.double() for o in olds]
    if fam == "adam":
        K = B.step_scalars(hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], hp["weight_decay"], t)
        p8, m8, v8 = B._update(p, gs, olds[0], olds[1], K, False)
        p3, m3, v3 = B._update(p, gs, olds[0], olds[1], K, True)            # the fp32 tensors associate the g'^2 term the other way
        _, m64, v64 = B._update(p.double(), gs.double(), d[0], d[1], K, False)
        return torch.where(eight, p8, p3), [torch.where(eight, m8, m3), torch.where(eight, v8, v3)], [m64, v64], None, None
    if fam == "lion":
        K = LR.step_scalars(hp["lr"], hp["betas"][0], hp["betas"][1], hp["weight_decay"])
        pn, m, und = LR.update(p, gs, olds[0], K)
        pd = p * K["decay"] if K["wd"] else p
        return pn, [m], [LR.update(p.double(), gs.double(), d[0], K)[1]], und, torch.stack([pd - K["lr"] * sg for sg in (-1.0, 0.0, 1.0)])
    st = {k: o.numpy().copy() for k, o in zip(AR.STATES, olds)}
    pn = AR.step32(p.numpy().copy(), g.numpy().copy(), clip, st, hp, t)
    s64 = {k: o.numpy() for k, o in zip(AR.STATES, d)}
    with np.errstate(all="ignore"):
        AR._step(p.double().numpy(), gs.double().numpy(), s64, AR.row32(hp, t))
    return torch.from_numpy(pn), [torch.from_numpy(st[k]) for k in AR.STATES], [torch.from_numpy(s64[k]) for k in AR.STATES], None, None


def step_ref(fam, S, X, hps, t, clipargs, assign=None):
    """One step of the restatement from the state S (not modified) -> (the new Flat, info).  hps: the family's rows; assign: the row
    of every tensor (None: row 0 for all) -- the restatement runs once per row over that row's tensors.  info: per state the flat mask
    of undecided codes (`und`), the flat mask of parameters whose sign Lion calls undecided (`p_und`), and the counts the tests
    record: code elements compared, undecided ones, sign repairs taken, codes 0 / 255 written; `p_alts`: for Lion the parameters the
    three signs of c would give, [3, n] (what an undecided element may hold)."""
    out, n = S.clone(), S.p.numel()
    signed = PLANES[fam]
    info = dict(und=[torch.zeros(n, dtype=torch.bool) for _ in signed], p_und=torch.zeros(n, dtype=torch.bool), codes=0, undecided=0,
                repaired=0, code0=0, code255=0, elements=int(X.pos.numel()), p_alts=None)
    clip = clip_of(clipargs)
    rows = [0] * X.n_tensors if assign is None else list(assign)
    for gi in sorted(set(rows)):
        sel = torch.tensor([r == gi for r in rows])[X.tid]
        pos, eight, blk, sidx = X.pos[sel], X.eight[sel], X.blk[sel], X.sidx[sel]
        olds = [torch.where(eight, QMAP[sg][S.codes[j][pos].long()] * S.absmax[j][blk], S.m32[j][sidx]) for j, sg in enumerate(signed)]
        pn, news, twins, p_und, alts = _update(fam, S.p[pos], S.g[pos], clip, olds, eight, hps[gi], t)
        out.p[pos] = pn
        if p_und is not None:
            info["p_und"][pos] = p_und
            if info["p_alts"] is None:
                info["p_alts"] = out.p.repeat(3, 1)
            info["p_alts"][:, pos] = alts
        e, nb = eight, S.absmax.shape[1]
        for j, sg in enumerate(signed):
            m, q = news[j], QMAP[sg]
            out.m32[j][sidx[~e]] = m[~e]
            if not bool(e.any()):
                continue
            und, mx = B.undecided_codes(m[e], twins[j][e], blk[e], nb, q, sg)
            touched = torch.unique(blk[e])
            out.absmax[j][touched] = mx[touched]
            d = mx[blk[e]]
            live = d > 0
            x = torch.where(live, m[e] / torch.where(live, d, torch.ones_like(d)), torch.zeros_like(d))
            c = B.quantize(x, q)
            if sg:
                info["repaired"] += int(B.sign_repaired(m[e], d, q).sum())
                c = torch.where(live, B.keep_sign(c, m[e], q), c)
            out.codes[j][pos[e]] = c.to(torch.uint8)
            info["und"][j][pos[e]] = und
            info["codes"] += int(e.sum())
            info["undecided"] += int(und.sum())
            info["code0"] += int((c == 0).sum())
            info["code255"] += int((c == 255).sum())
    info["undecided"] += int(info["p_und"].sum())
    return out, info


def compare(fam, got, want, info, where):
    """The exact rule on the whole buffers (canaries included): p, g, the block maxima and the fp32 moments bit for bit, decided codes
    identical, undecided ones within one step.  Lion's p where the restatement calls the sign of c undecided must still carry the
    bits one of the three signs gives.  Returns the figures, printed before anything is asserted."""
    keep = ~info["p_und"]
    rec = dict(elements=info["elements"], codes=info["codes"], undecided=info["undecided"],
               undecided_share=info["undecided"] / max(1, info["codes"] if fam != "lion" else info["codes"] + info["elements"]),
               p_ulp=B.ulp_diff(got.p[keep], want.p[keep]), absmax_ulp=B.ulp_diff(got.absmax_raw, want.absmax_raw),
               m32_ulp=B.ulp_diff(got.m32_raw, want.m32_raw), sign_repairs=info["repaired"])
    diffs = [(got.codes[j] != want.codes[j]) for j in range(len(PLANES[fam]))]
    rec["decided_mismatches"] = sum(int((d & ~u).sum()) for d, u in zip(diffs, info["und"]))
    rec["undecided_that_differ"] = sum(int((d & u).sum()) for d, u in zip(diffs, info["und"]))
    print(where, rec)
    assert B.same_bits(got.g, want.g), (where, "g was written")
    assert B.same_bits(got.p[keep], want.p[keep]), (where, "parameters", rec["p_ulp"])
    if bool(info["p_und"].any()):
        u = info["p_und"]
        hit = (got.p[u].view(torch.int32).unsqueeze(0) == info["p_alts"][:, u].contiguous().view(torch.int32)).any(0)
        assert bool(hit.all()), (where, "an undecided parameter holds none of the three signs' values")
    assert B.same_bits(got.absmax_raw, want.absmax_raw), (where, "block maxima", rec["absmax_ulp"])
    assert B.same_bits(got.m32_raw, want.m32_raw), (where, "fp32 moments", rec["m32_ulp"])
    for j in range(len(PLANES[fam])):
        B.check_codes(got.codes[j], want.codes[j], info["und"][j], (where, "state", j))
    assert rec["undecided_share"] <= B.UNDECIDED_CAP, (where, rec["undecided_share"])
    return rec


# ---------------------------------------------------------------- the inputs
SMALL = [1, 2, 3, 4, 5, 7, 8, 9, 17, 33, 63, 64, 65]      # fp32-mode lengths of the stride layouts (all below min_8bit_size 256)
TAIL_J = (1, 2, 3, 4, 5, 7, 8, 9)


def stride_sizes(bs):
    """Many short tensors, min_8bit_size 256, more table entries than two sweeps of the launch (about 4200 at blocksize 2048, about
    16500 at 256) below a million elements.  2048: period (8-bit 257.., 8-bit 256.., fp32): one entry each.  256: period (8-bit 257:
    a full entry and a 1-element entry, then five fp32 tensors).  The periods (3 and 7 entries) do not divide the sweep, so one
    workgroup (wave) meets both modes on consecutive trips, in both orders (test_blockwise8_cpu.py counts them)."""
    sizes, entries, i = [], 0, 0
    while entries < (4200 if bs == 2048 else 16500):
        if bs == 2048:
            sizes += [257 + i % 11, 256 + (i * 7) % 40, SMALL[i % len(SMALL)] + (190 if i % 5 == 0 else 0)]
            entries += 3
        else:
            sizes += [257] + [SMALL[(5 * i + j) % len(SMALL)] for j in range(5)]
            entries += 7
        i += 1
    return sizes


def tail_sizes(bs):
    """k bs + j for j in TAIL_J and k in {0, 1}, bs - 1 and bs - 5, twice: with the alignments of _case every offset class modulo 64
    that the builder accepts (the multiples of 4) carries some of them."""
    one = [k * bs + j for k in (0, 1) for j in TAIL_J] + [bs - 1, bs - 5]
    return one + one


def _lay(entries, bs, min8):
    from qflux_amd import ops
    return ops.adam8bit_block_table(entries, bs, min8)


class Case:
    """One layout with its step count and clip: `state(fam)` builds the Flat the step starts from (a fresh copy each call)."""

    def __init__(self, name, bs, sizes, min8, t, clip, fill, align=None):
        self.name, self.bs, self.sizes, self.min8, self.t, self.clip, self.fill = name, bs, sizes, min8, t, clip, fill
        self.entries, self.n = place(sizes, align)
        self.lay = _lay(self.entries, bs, min8)
        self.X = Index(self.lay)
        self._states, self._refs, self._clip = {}, {}, {}

    def state(self, fam):
        if fam not in self._states:
            S = new_flat(fam, self.lay, self.n)
            self.fill(self, fam, S, torch.Generator().manual_seed(1000 + len(self.name) + self.bs))
            if self.clip:      # the clip at work: the norm of the finite elements, max_norm 1, grad_scale 1/2
                gsq = float(torch.nan_to_num(S.g[self.X.pos].double(), nan=0.0, posinf=0.0, neginf=0.0).pow(2).sum())
                assert gsq * 0.25 > 1.0
                self._clip[fam] = (float(F32(gsq)), 1.0, 0.5)
            else:
                self._clip[fam] = (None, 0.0, 1.0)
            self._states[fam] = S
        return self._states[fam].clone()

    def clipargs_of(self, fam):
        """(gnorm_sq, max_norm, grad_scale) of this family's gradients: what the restatement and the launch are both handed."""
        self.state(fam)
        return self._clip[fam]

    def reference(self, fam, grouped=False):
        """(new Flat, info) of the restatement's step, computed once per family and entry and never modified by its users."""
        key = (fam, grouped)
        if key not in self._refs:
            S = self.state(fam)
            self._refs[key] = step_ref(fam, S, self.X, HPS[fam], self.t, self.clipargs_of(fam), self.assign() if grouped else None)
        return self._refs[key]

    def assign(self):
        return [(i + i // 3) % 3 for i in range(len(self.sizes))]

    def trips(self):
        from qflux_amd import ops
        per_sweep = ops.grouped_sweep_elems(self.bs) // self.bs
        return math.ceil(self.lay.n_blocks / per_sweep), per_sweep


def _one_top_per_block(blk, signed, gen):
    """Codes as a step could have written them: exactly one element of every block, at a random place, carries the block's largest
    magnitude -- code 255 (1.0) over codes uniform in 0..254, or, in every other block of a signed state, code 0 (-0.993, the
    magnitude of code 254) over codes uniform in 1..253.  Without such an element, or with several, the largest old moments of a
    block are equal, a gradient too small to separate them leaves the block maximum tied by bnb8_ref's rule, and whole tied blocks
    would spend the undecided cap on the input instead of on the kernel.  blk: ascending block ids."""
    n = blk.numel()
    if not n:
        return torch.zeros(0, dtype=torch.uint8)
    ids, inv, counts = torch.unique_consecutive(blk, return_inverse=True, return_counts=True)
    neg = (torch.arange(ids.numel()) % 2 == 1) if signed else torch.zeros(ids.numel(), dtype=torch.bool)
    u = torch.rand(n, generator=gen, dtype=torch.float64)
    codes = torch.where(neg[inv], 1 + (u * 253).long().clamp(max=252), (u * 255).long().clamp(max=254))
    start = torch.cumsum(counts, 0) - counts
    at = start + torch.minimum((torch.rand(ids.numel(), generator=gen, dtype=torch.float64) * counts).long(), counts - 1)
    codes[at] = torch.where(neg, 0, 255)
    return codes.to(torch.uint8)


def _fill_random(c, fam, S, gen, amax=(1e-3, 1.0), gscale=0.5):
    """Uniform codes (_one_top_per_block), log-uniform block maxima, small fp32 moments, gradients of mixed sign at the scale of the block's first-state
    maximum (fp32 tensors: 0.1)."""
    X, nab = c.X, c.lay.n_absmax
    N = X.pos.numel()
    S.p[X.pos] = torch.randn(N, generator=gen) * 0.1
    lo, hi = math.log10(amax[0]), math.log10(amax[1])
    for j, sg in enumerate(PLANES[fam]):
        S.codes[j][X.pos[X.eight]] = _one_top_per_block(X.blk[X.eight], sg, gen)
        S.absmax[j][:nab] = (10.0 ** (lo + (hi - lo) * torch.rand(nab, generator=gen, dtype=torch.float64))).float().clamp(amax[0], amax[1])
        r = torch.randn(int((~X.eight).sum()), generator=gen) * 0.01
        S.m32[j][X.sidx[~X.eight]] = r if sg else r * r
    scale = torch.where(X.eight, S.absmax[0][X.blk] * gscale, torch.full((N,), 0.1))
    S.g[X.pos] = torch.randn(N, generator=gen) * scale


def _fill_extreme(c, fam, S, gen):
    """Arbitrary reachable and extreme states: uniform codes; block maxima log-uniform between the smallest normal fp32 and 1e4, both
    ends present; in tensor 0 a block of all code 0, one of all code 255, one of all the code of 0.0 and one with maximum 0 under
    non-zero codes; gradients of mixed sign at half the block's first-state maximum, so many moments cross zero; and in every other
    block eight elements that hold the code of 0.0 and get a tiny negative gradient: their new first moment is a negative number
    whose nearest code is +0.0 -- the sign repair.  The three uniform blocks start from equal moments: their maxima are 1 (0.1 for the
    unsigned state) and their gradients large (200 sigma), so that the new moments are apart and the block maximum is not tied."""
    _fill_random(c, fam, S, gen, amax=(TINY, 1e4))
    X, bs = c.X, c.bs
    off0, a0 = c.entries[0][0], c.lay.tensors[0][3]
    for j, sg in enumerate(PLANES[fam]):
        for b, code in enumerate((0, 255, ZERO_CODE[sg])):
            S.codes[j][off0 + b * bs:off0 + (b + 1) * bs] = code
        S.absmax[j][a0 + 3] = 0.0
        S.absmax[j][a0 + 4], S.absmax[j][a0 + 5] = TINY, 1e4
    e = X.eight
    scale = S.absmax[0][X.blk[e]]
    S.g[X.pos[e]] = torch.randn(int(e.sum()), generator=gen) * torch.where(scale > 0, scale * 0.5, torch.full_like(scale, 1e-3))
    for j, sg in enumerate(PLANES[fam]):
        S.absmax[j][a0:a0 + 3] = 1.0 if sg else 0.1
    S.g[off0:off0 + 3 * bs] = torch.randn(3 * bs, generator=gen) * 200.0
    for off, k, _, ta0, nb, _ in c.lay.tensors:
        for b in range(nb):
            if (off == off0 and b < 4) or min(bs, k - b * bs) < 16:
                continue
            s = slice(off + b * bs + 1, off + b * bs + 9)
            for j, sg in enumerate(PLANES[fam]):
                if sg:
                    S.codes[j][s] = ZERO_CODE[True]
            S.g[s] = -S.absmax[0][ta0 + b] * 1e-6 * (0.1 + torch.rand(8, generator=gen))


SKIP_AT = 37      # element of the block that holds the old maximum and gets the non-finite gradient


def _fill_skips(c, fam, S, gen):
    """Elements the step must skip: in tensor 0 (8-bit) block 0 gets a NaN, block 1 a +inf and block 2 a -inf gradient, each on the
    one element whose old moments are the block's largest (code 255 over codes kept below |1|, small gradients everywhere): its old
    moment must still be the new block maximum.  Tensor 1 (fp32 moments) gets a NaN and a -inf."""
    _fill_random(c, fam, S, gen, gscale=0.01)
    off0 = c.entries[0][0]
    for b, bad in enumerate((float("nan"), float("inf"), float("-inf"))):
        s = slice(off0 + b * c.bs, off0 + (b + 1) * c.bs)
        for j in range(len(PLANES[fam])):
            S.codes[j][s] = torch.randint(20, 236, (c.bs,), generator=gen, dtype=torch.uint8)
            S.codes[j][off0 + b * c.bs + SKIP_AT] = 255
        S.g[off0 + b * c.bs + SKIP_AT] = bad
    off1 = c.entries[1][0]
    S.g[off1 + 5], S.g[off1 + 50] = float("nan"), float("-inf")


def _fill_zero(c, fam, S, gen):
    """Step 1 from bnb's initial state: every code 0, every maximum 0, zero fp32 moments; block 1 of tensor 0 has zero gradients."""
    X = c.X
    _fill_random(c, fam, S, gen)
    S.codes[:, X.pos[X.eight]] = 0
    S.absmax[:, :c.lay.n_absmax] = 0.0
    S.m32[:, X.sidx[~X.eight]] = 0.0
    S.g[X.pos] = torch.randn(X.pos.numel(), generator=gen) * 0.3
    off0 = c.entries[0][0]
    S.g[off0 + c.bs:off0 + 2 * c.bs] = 0.0


_CASES = {}
CASE_NAMES = ("stride", "extreme", "tails8", "tails32", "skips", "zero")


def case(name, bs):
    """The shared inputs, built once: stride (min_8bit_size 256, the clip at work), extreme, tails8 / tails32 (every tensor 8-bit /
    every tensor fp32, offsets through every multiple of 4 modulo 64), skips, zero (step 1)."""
    if (name, bs) not in _CASES:
        tails = tail_sizes(bs)
        rot = [4 * ((5 * i) % 16) for i in range(len(tails))]
        _CASES[name, bs] = {
            "stride": lambda: Case("stride", bs, stride_sizes(bs), 256, 3, True, _fill_random),
            "extreme": lambda: Case("extreme", bs, [24 * bs + 17, 12 * bs, bs + 1], 256, 3, False, _fill_extreme),
            "tails8": lambda: Case("tails8", bs, tails, 1, 2, True, _fill_random, rot),
            "tails32": lambda: Case("tails32", bs, tails, 10 ** 9, 2, True, _fill_random, rot),
            "skips": lambda: Case("skips", bs, [3 * bs + 17, 100, bs], 256, 2, False, _fill_skips),
            "zero": lambda: Case("zero", bs, [2 * bs + 9, 70, bs + 3], 256, 1, True, _fill_zero),
        }[name]()
    return _CASES[name, bs]
