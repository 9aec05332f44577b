"""GPU: csrc/qfx_ademamix.hip (qfx_ademamix_step, qfx_ademamix8bit_step and its grouped entry through ops) against the restatement
tests/ademamix_ref.py, and the two families in the fused train step.

Accuracy bar (the project's practice, tests/test_adamx_gpu.py): for every case and every output (p, m1, m2, nu), with e = the largest
absolute error against the fp64 restatement, e_kernel <= 2 e_ref32, where e_ref32 is the error of the fp32 restatement -- the
listing of include/qfx.h with one numpy fp32 operation per operation -- on the same inputs.  The number of elements whose bits differ
from the fp32 restatement's is recorded beside it.  On exactly representable data the kernel gives the fp32 restatement's bits.  A
grouped launch gives every tensor the bits a one-group launch with its row gives it; a launch repeated gives the same bits; an
element with a non-finite g' keeps p and its states; canaries around every buffer hold and g is not written.
8-bit: codes and absmax equal the 8-bit restatement's exactly; were a code to differ, the test counts and prints them and accepts
only a neighbouring code at a midpoint tie of the fp32 value.  p equals the 8-bit restatement's bit for bit, and is held to the
same 2x bar, per step, against the fp64 update from the same decoded states.
Every figure is printed before it is judged and dumped as ademamix_parity_gpu.json (kept as profiles/ademamix_parity.json)."""
import numpy as np
import pytest
import torch

import ademamix_ref as R
import optim_ref as OR
import test_ademamix_cpu as CPU
from parity_util import QWEN_BARS, _observe, build_pair, tiny_embeddings
from test_adamx_gpu import CLIPS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
GUARD, CANARY = 64, 12345.0
OUT = ("p",) + R.STATES
STEPS = 5
SCHED = dict(t_alpha=3, t_beta3=4)      # both schedules ramp and then saturate inside the five steps
_STATS = {"what": "tests/test_ademamix_gpu.py: per case the largest absolute error of the kernel and of the fp32 restatement against the "
                  "fp64 restatement (p, m1, m2, nu), and the elements whose bits differ from the fp32 restatement's; 8-bit: the codes "
                  "that differ from the 8-bit restatement's per step", "records": []}


def _lib():
    from qflux_amd import _lib
    return _lib


def _record(rec):
    print(rec)
    _STATS["records"].append(rec)
    _observe(None, None, dump=("ademamix_parity_gpu.json", _STATS))


class Buf:
    """n floats on the device between two canaries, at a 16-byte boundary (shift 0) or one float past it (shift 1)."""

    def __init__(self, host, shift=0):
        host = np.asarray(host, F32)
        self.n, self.lo = host.size, GUARD + shift
        raw = np.full(self.lo + self.n + GUARD, CANARY, F32)
        raw[self.lo:self.lo + self.n] = host
        self.whole = torch.from_numpy(raw).to(DEV)
        self.t = self.whole[self.lo:self.lo + self.n]
        assert (self.t.data_ptr() % 16 == 0) == (shift == 0)

    def get(self):
        r = self.whole.cpu().numpy()
        assert (r[:self.lo] == CANARY).all() and (r[self.lo + self.n:] == CANARY).all(), "canary overwritten"
        return r[self.lo:self.lo + self.n].copy()


def data(n, seed, steps, pads=()):
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(n) * 0.5).astype(F32)
    g = [(rng.standard_normal(n) * (0.1 + 0.05 * t)).astype(F32) for t in range(steps)]
    for a, b in pads:      # LoraStore's padding behind a tensor: zeros in every buffer
        p[a:b] = 0
        for x in g:
            x[a:b] = 0
    return p, g


def clip_of(name, g):
    """(fp64 coefficient, fp32 coefficient as the kernel forms it without contraction, the launch's arguments)."""
    gsq, mx, gs = CLIPS[name]
    if gsq is not None:
        gsq = float(F32(np.sum(np.asarray(g, F64) ** 2)))
    return OR.clip_f64(gsq, mx, gs), F32(OR.clip_f32(gsq, mx, gs)), (gsq, mx, gs)


def hp_of(wd=0.0, **kw):
    return dict(dict(lr=0.01, betas=R.BETAS, eps=1e-8, weight_decay=wd, alpha=5.0, **SCHED), **kw)


def kernel_run(p, grads, rows, clipname, tile_map=None, shift=0, start=None, t0=0):
    """len(grads) launches from zero states (or `start`: a dict of p / m1 / m2 / nu) at step counts t0 + 1 ...: the four buffers as numpy."""
    from qflux_amd import ops
    init = dict({k: np.zeros_like(p) for k in R.STATES}, p=p) if start is None else start
    B = {k: Buf(init[k], shift) for k in OUT}
    tg = None if tile_map is None else torch.from_numpy(np.asarray(tile_map, np.uint8)).to(DEV)
    for t, g in enumerate(grads, t0 + 1):
        G = Buf(g, shift)
        _, _, (gsq, mx, gs) = clip_of(clipname, g)
        gn = None if gsq is None else torch.tensor([gsq], dtype=torch.float32, device=DEV)
        ops.ademamix_step(B["p"].t, G.t, B["m1"].t, B["m2"].t, B["nu"].t, rows, t, tile_group=tg, gnorm_sq=gn, max_norm=mx, grad_scale=gs)
        torch.cuda.synchronize()
        assert np.array_equal(G.get().view(np.uint32), np.asarray(g, F32).view(np.uint32)), "g was written"
    return {k: B[k].get() for k in OUT}


def refs(p, grads, hp, clipname):
    """(fp64 restatement, fp32 restatement) on the same inputs."""
    return (R.run64(p, grads, [clip_of(clipname, g)[0] for g in grads], hp), R.run32(p, grads, [clip_of(clipname, g)[1] for g in grads], hp))


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def judge(case, got, r64, r32, mask=None):
    rec = {"case": case}
    sel = slice(None) if mask is None else mask
    for k in OUT:
        ek = float(np.abs(got[k].astype(F64) - r64[k])[sel].max())
        er = float(np.abs(r32[k].astype(F64) - r64[k])[sel].max())
        rec[k] = {"e_kernel": ek, "e_ref32": er, "bits_differ": int((got[k].view(np.uint32) != r32[k].view(np.uint32))[sel].sum())}
    _record(rec)
    for k in OUT:
        assert np.isfinite(got[k]).all() and rec[k]["e_kernel"] <= 2 * rec[k]["e_ref32"], (case, k, rec[k])


# ---------------------------------------------------------------- fp32: sizes, alignment, clip, schedules
@pytest.mark.parametrize("shift", [0, 1])
def test_one_group_every_size_decay_and_clip(shift):
    """n in {1, 63, 64, 65, 257, 4099} at a 16-byte boundary and one float past it (the scalar form), weight decay 0 / 0.01 and the clip
    off / active with grad_scale 1/3 / grad_scale 1/2 in rotation (all six pairs occur), five steps through both schedules."""
    for i, n in enumerate((1, 63, 64, 65, 257, 4099)):
        hp, cn = hp_of(wd=(0.0, 0.01)[(i + shift) % 2]), list(CLIPS)[(i + 2 * shift) % 3]
        p, grads = data(n, 100 + i, STEPS)
        r64, r32 = refs(p, grads, hp, cn)
        got = kernel_run(p, grads, [hp], cn, shift=shift)
        judge((n, shift, cn, hp["weight_decay"]), got, r64, r32)
        if n == 4099:      # the same launches again: the same bits; and the other access form gives these bits too
            again, other = kernel_run(p, grads, [hp], cn, shift=shift), kernel_run(p, grads, [hp], cn, shift=1 - shift)
            for k in OUT:
                assert same_bits(got[k], again[k]), (k, "not deterministic")
                assert same_bits(got[k], other[k]), (k, "scalar != 16-byte form")


def test_the_stride_loop_runs_twice():
    """n = one grid sweep of the 16-byte form + 67: the last 67 elements are the second trip (and its scalar tail)."""
    from qflux_amd import ops
    n = ops.grouped_sweep_elems(0) + 67
    hp = hp_of(wd=0.01)
    p, grads = data(n, 7, 2)
    r64, r32 = refs(p, grads, hp, "active_third")
    got = kernel_run(p, grads, [hp], "active_third")
    tail = np.zeros(n, bool)
    tail[-67 - 64:] = True
    judge((n, "second trip"), got, r64, r32, mask=tail)
    judge((n, "whole"), got, r64, r32)


@pytest.mark.parametrize("betas,exact", [((0.5, 0.5, 0.5), False), ((0.5, 0.75, 0.5), True)])
def test_exact_case_gives_the_fp32_restatements_bits(betas, exact):
    """Powers of two, one step: with every beta 0.5 the one inexact scalar is sqrt(1 - 0.5); with beta2 = 0.75 (sqrt(0.25) = 0.5) every
    operation is exact and fp64 and fp32 restatement are the same numbers.  Either way the kernel gives the fp32 restatement's bits."""
    rng = np.random.default_rng(11)
    n = 300
    p = (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-2, 3, n)).astype(F32)
    g = (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-6, 2, n)).astype(F32)
    for wd in (0.0, 0.5):
        hp = dict(lr=2.0 ** -4, betas=betas, eps=0.0, weight_decay=wd, alpha=2.0, t_alpha=None, t_beta3=None)
        r64, r32 = refs(p, [g], hp, "off")
        if exact:
            for k in OUT:
                assert np.array_equal(r32[k].astype(F64), r64[k]), k
            assert np.array_equal(r32["p"], ((p - 2.0 ** -3 * np.sign(g)) * (1 - 2.0 ** -4 * wd)).astype(F32))
        for shift in (0, 1):
            got = kernel_run(p, [g], [hp], "off", shift=shift)
            for k in OUT:
                assert same_bits(got[k], r32[k]), (betas, wd, shift, k)


@pytest.mark.parametrize("n", [64 * 4 + 3, 4096 * 1024 + 64 + 3])
def test_exact_case_with_a_quad_body_a_tail_and_a_second_trip(n):
    """The all-exact case above at a length with a 16-byte body and an n % 4 tail (also one float past a 16-byte boundary: the scalar
    form), and at one where 4096 workgroups of 256 quads leave a second trip of the stride loop with such a tail behind it."""
    rng = np.random.default_rng(12)
    p = (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-2, 3, n)).astype(F32)
    g = (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-6, 2, n)).astype(F32)
    hp = dict(lr=2.0 ** -4, betas=(0.5, 0.75, 0.5), eps=0.0, weight_decay=0.5, alpha=2.0, t_alpha=None, t_beta3=None)
    r64, r32 = refs(p, [g], hp, "off")
    for shift in (0, 1) if n < 1024 else (0,):
        got = kernel_run(p, [g], [hp], "off", shift=shift)
        for k in OUT:
            assert np.array_equal(r32[k].astype(F64), r64[k]) and same_bits(got[k], r32[k]), (n, shift, k)


# ---------------------------------------------------------------- fp32: parameter groups
def layout64():
    """Tensors of odd sizes at multiples of 64 filling exactly 64 tiles: [(off, numel)], 4096, the pad slots."""
    sizes = [37, 64, 65, 130, 200, 7, 128, 1, 63, 257, 90, 64, 33, 191, 5, 129, 70, 300, 2, 66, 500, 320, 513]
    entries, off = [], 0
    for k in sizes:
        entries.append((off, k))
        off += (k + 63) // 64 * 64
    assert off == 64 * 64
    return entries, off, [(o + k, (o + k + 63) // 64 * 64) for o, k in entries]


def test_three_groups_over_a_64_tile_map_with_an_out_of_range_byte():
    from qflux_amd import ops
    entries, n, pads = layout64()
    assign = [i % 3 for i in range(len(entries))]
    good = ops.tile_group_map(entries, assign, 3, numel=n).numpy()
    assert good.size == 64
    bad = good.copy()
    last = np.flatnonzero(good == 2)
    bad[last[0]], bad[last[-1]] = 3, 255      # past n_groups: the last row
    rows = [hp_of(wd=0.0), hp_of(wd=0.01, lr=0.02, betas=(0.8, 0.99, 0.999), alpha=2.0, t_alpha=None),
            hp_of(wd=0.02, lr=0.005, betas=(0.95, 0.98, 0.9995), eps=1e-6, t_beta3=None)]
    elem = np.repeat(good, 64)[:n].astype(np.int64)
    p, grads = data(n, 33, STEPS, pads)
    cn = "active_third"
    got = {s: kernel_run(p, grads, rows, cn, tile_map=bad, shift=s) for s in (0, 1)}
    want = kernel_run(p, grads, rows, cn, tile_map=good)
    for k in OUT:
        assert same_bits(got[0][k], got[1][k]), (k, "scalar != 16-byte form")
        assert same_bits(got[0][k], want[k]), (k, "an entry past n_groups did not take the last row")
    for a, b in pads:
        assert not got[0]["p"][a:b].view(np.uint32).any()      # the padding of the parameters stays +0
    for gi, hp in enumerate(rows):
        mask = elem == gi
        single = kernel_run(p, grads, [hp], cn)      # one group, NULL map, this group's row
        for k in OUT:
            assert same_bits(got[0][k][mask], single[k][mask]), (gi, k)
        r64, r32 = refs(p, grads, hp, cn)
        judge(("groups", gi), got[0], r64, r32, mask=mask)


def test_a_non_finite_gradient_element_keeps_its_parameter_and_states():
    n = 300
    hp = hp_of(wd=0.01)
    p, grads = data(n, 41, 3)
    before = kernel_run(p, grads[:2], [hp], "off")
    g_bad, g_zero = grads[2].copy(), grads[2].copy()
    where = [0, 5, 63, 64, 130, 299]
    g_bad[where] = [np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf]
    g_zero[where] = 0
    for shift in (0, 1):
        got = kernel_run(before["p"], [g_bad], [hp], "off", shift=shift, start=before, t0=2)
        ref = kernel_run(before["p"], [g_zero], [hp], "off", shift=shift, start=before, t0=2)
        keep = np.zeros(n, bool)
        keep[where] = True
        for k in OUT:
            assert same_bits(got[k][keep], before[k][keep]), (shift, k, "a skipped element moved")
            assert same_bits(got[k][~keep], ref[k][~keep]), (shift, k, "a neighbour was not stepped as usual")
            assert (got[k][~keep] != before[k][~keep]).any() and np.isfinite(got[k]).all()


def test_refusals_happen_before_any_launch():
    """QFX_EINVAL for every case of include/qfx.h; the pointers handed over are not memory, so a launch would have faulted -- and the
    device still computes afterwards."""
    CPU.check_refusals(_lib())
    torch.cuda.synchronize()
    assert float(torch.ones(4, device=DEV).sum()) == 4.0


# ---------------------------------------------------------------- blockwise 8-bit
MIN8 = 200
SIZES8 = [255, 256, 257, 2049, 4099, 100]      # the last one is below MIN8: fp32 states


def flat_offsets(sizes):
    offs, off = [], 0
    for k in sizes:
        offs.append(off)
        off += (k + 63) // 64 * 64
    return offs, off


class Dev8:
    """The device buffers of the 8-bit step between canaries; the states start as bnb's initial ones (codes 0, absmax 0)."""

    def __init__(self, sizes, bs, params):
        from qflux_amd import ops
        self.offs, n = flat_offsets(sizes)
        self.n, self.sizes = n, sizes
        self.lay = ops.adam8bit_block_table(list(zip(self.offs, sizes)), bs, MIN8, device=DEV)
        flat = np.zeros(n, F32)
        for off, p in zip(self.offs, params):
            flat[off:off + p.numel()] = p.numpy()
        self.P, self.V32 = Buf(flat), Buf(np.zeros(max(4, self.lay.n_fp32), F32))
        self.M32 = Buf(np.zeros(2 * max(4, self.lay.n_fp32), F32))
        self.A1, self.A2 = Buf(np.zeros(2 * max(1, self.lay.n_absmax), F32)), Buf(np.zeros(max(1, self.lay.n_absmax), F32))
        self.plane = (n + 15) // 16 * 16
        self.q1 = torch.full((2 * self.plane + 2 * GUARD,), 77, dtype=torch.uint8, device=DEV)
        self.q2 = torch.full((n + 2 * GUARD,), 77, dtype=torch.uint8, device=DEV)
        self.q1[GUARD:-GUARD] = 0
        self.q2[GUARD:-GUARD] = 0
        self.qm1, self.qm2 = R.B.create_dynamic_map(True).to(DEV), R.B.create_dynamic_map(False).to(DEV)

    def step(self, grads, rows, t, clipname, block_group=None):
        from qflux_amd import ops
        flat = np.zeros(self.n, F32)
        for off, g in zip(self.offs, grads):
            flat[off:off + g.numel()] = g.numpy()
        G = Buf(flat)
        _, _, (gsq, mx, gs) = clip_of(clipname, flat)
        gn = None if gsq is None else torch.tensor([gsq], dtype=torch.float32, device=DEV)
        ops.ademamix8bit_step(self.P.t, G.t, self.q1[GUARD:-GUARD].view(2, self.plane), self.q2[GUARD:-GUARD], self.A1.t.view(2, -1), self.A2.t,
                              self.M32.t.view(2, -1), self.V32.t, self.lay, self.qm1, self.qm2, rows, t, block_group=block_group, gnorm_sq=gn,
                              max_norm=mx, grad_scale=gs)
        torch.cuda.synchronize()
        assert same_bits(G.get(), flat), "g was written"
        return flat

    def get(self):
        """Per tensor the file-layout state and p, as CPU tensors; every canary checked."""
        q1, q2 = self.q1.cpu(), self.q2.cpu()
        assert (q1[:GUARD] == 77).all() and (q1[-GUARD:] == 77).all() and (q2[:GUARD] == 77).all() and (q2[-GUARD:] == 77).all(), "canary overwritten"
        q1, q2 = q1[GUARD:-GUARD].view(2, -1), q2[GUARD:-GUARD]
        p, a1, a2 = torch.from_numpy(self.P.get()), torch.from_numpy(self.A1.get()).view(2, -1), torch.from_numpy(self.A2.get())
        m32, v32 = torch.from_numpy(self.M32.get()).view(2, -1), torch.from_numpy(self.V32.get())
        out = []
        for off, k, eight, a0, nb, s0 in self.lay.tensors:
            if eight:
                out.append(dict(p=p[off:off + k], state1=q1[:, off:off + k], state2=q2[off:off + k], absmax1=a1[:, a0:a0 + nb], absmax2=a2[a0:a0 + nb]))
            else:
                out.append(dict(p=p[off:off + k], state1=m32[:, s0:s0 + k], state2=v32[s0:s0 + k]))
        return out


def bits(t):
    return t.contiguous().view(torch.uint8)


def make8(bs, seed=3):
    """Parameters and three steps of gradients for SIZES8: block 0 of the 4099-element tensor has zero gradients throughout (its
    absmax stays 0); in the 2049-element tensor elements 0 and 1 carry the block's largest gradient at step 1 and -0.95 of it at
    step 2 -- the fast average (beta1 = 0.9) changes sign there, the slow one (beta3 = 0.9999) does not."""
    gen = torch.Generator().manual_seed(seed)
    params = [torch.randn(k, generator=gen) * 0.5 for k in SIZES8]
    grads = [[torch.randn(k, generator=gen) * (0.1 + 0.05 * t) for k in SIZES8] for t in range(3)]
    for g in grads:
        g[4][:bs] = 0
    grads[0][3][:2] = torch.tensor([8.0, -8.0])
    grads[1][3][:2] = torch.tensor([-7.6, 7.6])
    return params, grads


def codes_agree(case, got, want, x, qmap, stats):
    """Codes equal; a code that differs is counted and must be the neighbouring code at a midpoint tie of the fp32 value x."""
    got, want = got.reshape(-1).long(), want.reshape(-1).long()
    diff = torch.nonzero(got != want).flatten()
    stats["codes"] += got.numel()
    stats["differ"] += diff.numel()
    if diff.numel():
        print(case, f"{diff.numel()} of {got.numel()} codes differ from the restatement's")
        mid = R.B.midpoints(qmap)
        for i in diff.tolist():
            lo = min(int(got[i]), int(want[i]))
            assert abs(int(got[i]) - int(want[i])) == 1 and float(x[i]) == float(mid[lo]), (case, i, int(got[i]), int(want[i]), float(x[i]))


@pytest.mark.parametrize("bs", [256, 2048])
def test_8bit_codes_absmax_and_parameters_match_the_restatement(bs):
    hp = dict(lr=0.01, betas=R.BETAS, eps=1e-8, weight_decay=0.01, alpha=5.0, t_alpha=3, t_beta3=None)
    params, grads = make8(bs)
    ref = R.AdEMAMix8bitRef([p.clone() for p in params], hp, min_8bit_size=MIN8, blocksize=bs)
    d = Dev8(SIZES8, bs, params)
    assert [t[2] for t in d.lay.tensors] == [True] * 5 + [False]
    zero = int(torch.searchsorted(ref.qmap1, torch.tensor(0.0)))
    for t, g in enumerate(grads, 1):
        cn = "off" if t < 3 else "active_third"      # one coefficient through steps 1 and 2: the sign scenario of make8 is stated in g
        p_before = [p.clone() for p in ref.params]
        flat = d.step(g, [hp], t, cn)
        c64, c32, _ = clip_of(cn, flat)
        ref.step(g, clip=c32)
        got, stats = d.get(), {"codes": 0, "differ": 0}
        ek = er = 0.0
        for i, (o, st) in enumerate(zip(got, ref.state)):
            case = (bs, t, SIZES8[i])
            if st["state1"].dtype != torch.uint8:
                assert torch.equal(bits(o["state1"]), bits(st["state1"])) and torch.equal(bits(o["state2"]), bits(st["state2"])), case
                assert torch.equal(bits(o["p"]), bits(ref.params[i])), case
                continue
            last = ref.last[i]
            assert torch.equal(bits(o["p"]), bits(ref.params[i])), case      # the update reads only the decoded old state: the fp32 restatement's bits
            assert torch.equal(bits(o["absmax1"]), bits(st["absmax1"])), case
            assert torch.equal(bits(o["absmax2"]), bits(st["absmax2"])), case
            blk = torch.arange(SIZES8[i]) // bs
            for plane, k in enumerate(("m1", "m2")):
                am = st["absmax1"][plane][blk]
                x = torch.where(am > 0, torch.from_numpy(last["after"][k]) / torch.where(am > 0, am, torch.ones_like(am)), torch.zeros_like(am))
                codes_agree(case + (k,), o["state1"][plane], st["state1"][plane], x, ref.qmap1, stats)
            am = st["absmax2"][blk]
            x = torch.where(am > 0, torch.from_numpy(last["after"]["nu"]) / torch.where(am > 0, am, torch.ones_like(am)), torch.zeros_like(am))
            codes_agree(case + ("nu",), o["state2"], st["state2"], x, ref.qmap2, stats)
            # p against the fp64 update from the same decoded states
            s64 = {k: v.astype(F64) for k, v in last["before"].items()}
            p64 = R.step64(p_before[i].numpy().astype(F64), g[i].numpy().astype(F64) * c64, s64, hp, t)
            ek = max(ek, float(np.abs(o["p"].numpy().astype(F64) - p64).max()))
            er = max(er, float(np.abs(ref.params[i].numpy().astype(F64) - p64).max()))
            if i == 4:      # the all-zero block: absmax 0, the code of 0.0 in both planes, code 0 (= 0.0) for nu, p only decayed
                assert (st["absmax1"][:, 0] == 0).all() and st["absmax2"][0] == 0
                assert (o["state1"][:, :bs] == zero).all() and (o["state2"][:bs] == 0).all()
                assert torch.equal(o["p"][:bs], ref.params[i][:bs])
            if i == 3 and t == 2:      # the sign of m1 flipped, that of m2 did not, and the stored codes carry those signs
                b, a = last["before"], last["after"]
                assert (np.sign(a["m1"][:2]) == -np.sign(b["m1"][:2])).all() and (np.sign(a["m2"][:2]) == np.sign(b["m2"][:2])).all()
                for plane, k in enumerate(("m1", "m2")):
                    assert (torch.sign(ref.qmap1[o["state1"][plane][:2].long()]).numpy() == np.sign(a[k][:2])).all(), k
        _record({"case": ("8bit", bs, t, cn), "codes": stats["codes"], "codes_differ": stats["differ"], "p": {"e_kernel": ek, "e_ref32": er}})
        assert ek <= 2 * er, (bs, t, ek, er)


@pytest.mark.parametrize("bs", [256, 2048])
def test_8bit_grouped_launch_equals_the_per_tensor_launches(bs):
    from qflux_amd import ops
    rows = [dict(lr=0.01, betas=R.BETAS, eps=1e-8, weight_decay=0.0, alpha=5.0, t_alpha=3, t_beta3=4),
            dict(lr=0.02, betas=(0.8, 0.99, 0.999), eps=1e-6, weight_decay=0.01, alpha=2.0, t_alpha=None, t_beta3=None),
            dict(lr=0.005, betas=(0.95, 0.98, 0.9995), eps=1e-8, weight_decay=0.02, alpha=8.0, t_alpha=2, t_beta3=None)]
    assign = [i % 3 for i in range(len(SIZES8))]
    params, grads = make8(bs, seed=9)
    grouped = Dev8(SIZES8, bs, params)
    again = Dev8(SIZES8, bs, params)
    bmap = ops.block_group_map(grouped.lay, assign, 3, device=DEV)
    singles = [Dev8(SIZES8, bs, params) for _ in rows]
    for t, g in enumerate(grads, 1):
        grouped.step(g, rows, t, "active_third", block_group=bmap)
        again.step(g, rows, t, "active_third", block_group=bmap)
        for d, r in zip(singles, rows):
            d.step(g, [r], t, "active_third")      # the ungrouped entry with this group's row
    got, rep, ones = grouped.get(), again.get(), [d.get() for d in singles]
    for i, o in enumerate(got):
        for k, v in o.items():
            assert torch.equal(bits(v), bits(ones[assign[i]][i][k])), (bs, i, k)
            assert torch.equal(bits(v), bits(rep[i][k])), (bs, i, k, "not deterministic")
    assert not torch.equal(ones[0][1]["p"], ones[1][1]["p"])      # the rows do differ


# ---------------------------------------------------------------- through the train step
_TWINS = {}


def _twins():
    from common import TINY
    if not _TWINS:
        _TWINS["models"] = [build_pair(dict(TINY), device=DEV, seed=2)[1] for _ in range(2)]
        _TWINS["start"] = _TWINS["models"][0].lora_store.pflat.detach().clone()
    for m in _TWINS["models"]:
        with torch.no_grad():
            m.lora_store.pflat.copy_(_TWINS["start"])
            m.lora_store.gflat.zero_()
    return _TWINS["models"]


def test_fused_train_steps_follow_the_fp32_restatement_on_autograd_gradients():
    """Three fused train steps (forward, backward, clip, the AdEMAMix launch) against the same model on the autograd path, whose
    gradients -- after clip_grad_norm_ -- are stepped by the fp32 restatement on the host.  Held to parity_util.QWEN_BARS: every
    loss within QWEN_BARS[0] relative, the loss bar of the fused-vs-autograd step parity.  QWEN_BARS' gradient bar says nothing
    about the weights: an Adam-type update divides by |g|, so the relative error of a small gradient passes into the update
    undamped.  Beside the losses the sibling tests' measure is asserted (tests/test_adamx_gpu.py): the cosine of the two total
    updates above 0.9; their relative distance is printed and recorded."""
    from qflux_amd.trainer import QwenLoraTrainStep
    a, b = _twins()
    start = _TWINS["start"]
    lr, steps, wd = 1e-4, 3, 0.01
    args = dict(alpha=5.0, t_alpha=3, t_beta3=4)
    hp = dict(lr=lr, betas=R.BETAS, eps=1e-8, weight_decay=wd, **args)
    pool = [tiny_embeddings(seed=500 + i) for i in range(steps)]
    fused = QwenLoraTrainStep(a, lr=lr, weight_decay=wd, max_grad_norm=1.0, optimizer="ademamix", optimizer_args=args)
    helper = QwenLoraTrainStep(b)
    params = [p for n, p in b.named_parameters() if "lora_" in n]
    hp_state = [R.new_state(p.detach().cpu().numpy().reshape(-1), F32) for p in params]
    la, lb = [], []
    for t, (emb, noise, u) in enumerate(pool, 1):
        la.append(fused.train_step(emb, noise=noise, u=u).item())
        loss = helper.compute_loss(emb, noise=noise, u=u)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        with torch.no_grad():
            for p, st in zip(params, hp_state):
                new = R.step32(p.detach().cpu().numpy().reshape(-1).astype(F32), p.grad.detach().cpu().numpy().reshape(-1).astype(F32), F32(1), st, hp, t)
                p.copy_(torch.from_numpy(new).view(p.shape).to(p.device))
                p.grad = None
        lb.append(loss.item())
    du_a, du_b = (a.lora_store.pflat.detach() - start).flatten(), (b.lora_store.pflat.detach() - start).flatten()
    rel = [abs(x - y) / abs(y) for x, y in zip(la, lb)]
    cos = float(torch.dot(du_a, du_b) / (du_a.norm() * du_b.norm() + 1e-30))
    dist = float((du_a - du_b).norm() / du_b.norm())
    _record({"case": ("ademamix", "train step"), "loss_rel": rel, "update_cosine": cos, "update_rel_distance": dist})
    assert max(rel) < QWEN_BARS[0], rel
    assert cos > 0.9 and float(du_a.abs().max()) > 0, cos
    assert fused.global_step == steps and set(next(iter(fused.state_dict()["state"].values()))) == CPU.KEYS32


@pytest.mark.parametrize("family,args", [("ademamix", {}), ("ademamix8bit_blockwise", {"min_8bit_size": 64})])
def test_checkpoint_resume_is_bit_for_bit(family, args, tmp_path):
    """Two steps, save_checkpoint, a fresh step object, load_checkpoint, one more step == three uninterrupted steps, bit for bit: the
    states and the step count both schedules hang on come back."""
    from qflux_amd.trainer import QwenLoraTrainStep
    a, a2 = _twins()
    args = dict(args, alpha=4.0, t_alpha=3, t_beta3=4)
    pool = [tiny_embeddings(seed=520 + i) for i in range(3)]
    run = QwenLoraTrainStep(a, lr=2e-3, max_grad_norm=1.0, optimizer=family, optimizer_args=dict(args))
    for it, (emb, noise, u) in enumerate(pool):
        run.train_step(emb, noise=noise, u=u)
        if it == 1:
            run.save_checkpoint(str(tmp_path / "ck"))
            mid = a.lora_store.pflat.detach().clone()
    want = a.lora_store.pflat.detach().clone()
    want_bufs = [t.detach().clone() for _, t in run.opt_state.buffers()]
    with torch.no_grad():
        a2.lora_store.pflat.copy_(mid)
    resumed = QwenLoraTrainStep(a2, lr=123.0, max_grad_norm=1.0, optimizer=family,
                                optimizer_args={"min_8bit_size": 64} if "min_8bit_size" in args else None)
    resumed.load_checkpoint(str(tmp_path / "ck"))
    assert resumed.global_step == 2 and resumed.lr == 2e-3 and resumed.betas == R.BETAS and resumed.weight_decay == 0.01
    assert all(resumed.optimizer_args[k] == v for k, v in args.items())
    emb, noise, u = pool[-1]
    resumed.train_step(emb, noise=noise, u=u)
    assert torch.equal(a2.lora_store.pflat.detach(), want) and not torch.equal(want, mid)
    if family == "ademamix":
        for x, (n, y) in zip(want_bufs, resumed.opt_state.buffers()):
            assert torch.equal(x, y), n
    keys = {frozenset(e) for e in resumed.state_dict()["state"].values()}
    if family == "ademamix":
        assert keys == {frozenset(CPU.KEYS32)}
    else:
        assert frozenset(CPU.KEYS8) in keys and keys <= {frozenset(CPU.KEYS8), frozenset({"step", "state1", "state2"})}


@pytest.mark.parametrize("family", ["ademamix", "ademamix8bit_blockwise"])
def test_loraplus_groups_and_ema_compose(family):
    """loraplus_lr_ratio=4 and ema_decay=0.9 beside the AdEMAMix step: lora_A is stepped with the one-group run's bits (its row is the
    one-group row), lora_B moves differently (four times the rate), and the EMA shadow is updated behind the step."""
    from qflux_amd.trainer import QwenLoraTrainStep
    a, b = _twins()
    start = _TWINS["start"]
    args = dict(t_alpha=3, t_beta3=4, **({"min_8bit_size": 64} if family.endswith("blockwise") else {}))
    pool = [tiny_embeddings(seed=540 + i) for i in range(2)]
    plus = QwenLoraTrainStep(a, lr=1e-3, max_grad_norm=1.0, optimizer=family, optimizer_args=dict(args), loraplus_lr_ratio=4.0, ema_decay=0.9)
    one = QwenLoraTrainStep(b, lr=1e-3, max_grad_norm=1.0, optimizer=family, optimizer_args=dict(args))
    emb, noise, u = pool[0]
    plus.train_step(emb, noise=noise, u=u)
    one.train_step(emb, noise=noise, u=u)
    st = a.lora_store
    for name, p, off, k in st.entries:
        x, y, s = st.pflat[off:off + k], b.lora_store.pflat[off:off + k], start[off:off + k]
        if "lora_A" in name:
            assert torch.equal(x, y), name
        elif float((y - s).abs().max()) > 0:
            assert not torch.equal(x, y), name
    assert len(plus.state_dict()["param_groups"]) == 2 and plus.ema is not None
    first = st.pflat.detach().clone()
    # diffusers' decay of the first update is 0: the shadow is s - 1 * (s - p), the stepped weights to two fp32 roundings of |s|, |p| <= max
    big = float(torch.maximum(first.abs().max(), start.abs().max()))
    assert float((plus.ema.shadows[0] - first).abs().max()) <= 4 * 2.0 ** -24 * big and not torch.equal(plus.ema.shadows[0], start)
    emb, noise, u = pool[1]
    loss = plus.train_step(emb, noise=noise, u=u)
    assert torch.isfinite(loss) and torch.isfinite(st.pflat).all() and plus.global_step == 2
    shadow = plus.ema.shadows[0].detach()      # second update: decay min(0.9, 2 / 11), strictly between the two sets of weights
    assert torch.isfinite(shadow).all() and not torch.equal(shadow, first) and not torch.equal(shadow, st.pflat.detach())
