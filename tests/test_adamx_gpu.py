"""GPU: csrc/qfx_adamx.hip (qfx_adamx_step through ops.adamx_step) against the fp64 restatement tests/adamx_ref.py, and the three
families in the fused train step against the real torch.optim classes on the autograd path.

Accuracy bar (the project's practice, tools/muon_bench.py): for every case and every output (p, exp_avg, the second state), with
e = the largest absolute error against the fp64 restatement, e_kernel <= 2 e_torch, where e_torch is the error of torch's own fp32
CPU step (the real torch.optim class, single-tensor path) on the same inputs -- the gradient it is handed is the fp32 product
g * clip the kernel forms first, the restatement gets g * clip in double.  Where one step is exact arithmetic (test_adamx_cpu's
exact_case) the kernel gives torch's fp32 bits.  A grouped launch gives every tensor the bits a one-group launch with its row
gives it; a launch repeated gives the same bits; canaries around every buffer hold and g is not written.
Every figure is printed before it is judged and dumped as adamx_parity_gpu.json (kept in profiles/adam_variants.json)."""
import numpy as np
import pytest
import torch

import adamx_ref as R
import optim_ref as OR
import test_adamx_cpu as CPU
from parity_util import QWEN_BARS, _observe, build_pair, tiny_embeddings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
GUARD, CANARY = 64, 12345.0
_STATS = {"what": "tests/test_adamx_gpu.py: per case the largest absolute error of the kernel and of torch's fp32 CPU step against the "
                  "fp64 restatement (p, exp_avg, second state), and the elements whose bits differ from torch's", "records": []}

HP = {
    "radam": [dict(weight_decay=0.0), dict(weight_decay=0.01), dict(weight_decay=0.01, decoupled_weight_decay=True)],
    "nadam": [dict(weight_decay=0.0), dict(weight_decay=0.01, momentum_decay=0.0), dict(weight_decay=0.01, decoupled_weight_decay=True)],
    "adamax": [dict(weight_decay=0.0), dict(weight_decay=0.01)],
}
STEPS = {"radam": 8, "nadam": 4, "adamax": 3}      # RAdam: rho_t > 5 from step 6 on; NAdam: mu_product has compounded
# (gnorm_sq or None, max_norm, grad_scale): the clip off, active with grad_scale 1/3, grad_scale alone
CLIPS = {"off": (None, 0.0, 1.0), "active_third": ("norm", 0.5, 1.0 / 3.0), "scale_half": (None, 0.0, 0.5)}


def _lib():
    from qflux_amd import _lib
    return _lib


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


def kernel_run(family, p, grads, rows, clipname, tile_map=None, shift=0, n_groups=None):
    """len(grads) launches from torch's initial state: {"p", "exp_avg", "second"} as numpy; rows: one hp dict per group."""
    from qflux_amd import ops
    B = {"p": Buf(p, shift), "m": Buf(np.zeros_like(p), shift), "s": Buf(np.zeros_like(p), shift)}
    tg = None if tile_map is None else torch.from_numpy(np.asarray(tile_map, np.uint8)).to(DEV)
    groups = [dict(lr=r["lr"], betas=(r["beta1"], r["beta2"]), eps=r["eps"], weight_decay=r["weight_decay"],
                   **{k: r[k] for k in ("decoupled_weight_decay", "momentum_decay") if k in r}) for r in rows]
    mus = [torch.tensor(1.0) for _ in groups]
    for t, g in enumerate(grads, 1):
        G = Buf(g, shift)
        _, _, (gsq, mx, gs) = clip_of(clipname, g)
        gn = None if gsq is None else torch.tensor([gsq], dtype=torch.float32, device=DEV)
        ops.adamx_step(family, B["p"].t, G.t, B["m"].t, B["s"].t, groups[:n_groups] if n_groups else groups, t, tile_group=tg,
                       mu_products=mus, gnorm_sq=gn, max_norm=mx, grad_scale=gs)
        torch.cuda.synchronize()
        assert np.array_equal(G.get().view(np.uint32), np.asarray(g, F32).view(np.uint32)), "g was written"
    return {"p": B["p"].get(), "exp_avg": B["m"].get(), "second": B["s"].get()}


def refs(family, p, grads, hp, clipname):
    """(fp64 restatement, torch's fp32 CPU step) on the same inputs, each {"p", "exp_avg", "second"}."""
    c64 = [clip_of(clipname, g)[0] for g in grads]
    c32 = [clip_of(clipname, g)[1] for g in grads]
    pp = np.array(p, F64)
    st = R.new_state(family, pp)
    for g, c in zip(grads, c64):
        R.STEP[family](pp, np.asarray(g, F64) * c, st, **hp)
    r64 = {"p": pp, "exp_avg": st["exp_avg"], "second": st[R.SECOND[family]]}
    tp, ts = CPU.torch_run(family, np.asarray(p, F32), [(np.asarray(g, F32) * c).astype(F32) for g, c in zip(grads, c32)], hp, torch.float32)
    return r64, {"p": tp, "exp_avg": ts["exp_avg"], "second": ts[R.SECOND[family]]}


def judge(case, got, r64, r32, mask=None):
    rec = {"case": case}
    for k in ("p", "exp_avg", "second"):
        sel = slice(None) if mask is None else mask
        ek = float(np.abs(got[k].astype(F64) - r64[k])[sel].max())
        et = float(np.abs(r32[k].astype(F64) - r64[k])[sel].max())
        rec[k] = {"e_kernel": ek, "e_torch": et, "bits_differ": int((got[k].view(np.uint32) != r32[k].view(np.uint32))[sel].sum())}
    print(rec)
    _STATS["records"].append(rec)
    _observe(None, None, dump=("adamx_parity_gpu.json", _STATS))
    for k in ("p", "exp_avg", "second"):
        assert np.isfinite(got[k]).all() and rec[k]["e_kernel"] <= 2 * rec[k]["e_torch"], (case, k, rec[k])


def hp_of(family, i, beta2=0.999, lr=0.01):
    return dict(lr=lr, beta1=0.9, beta2=beta2, eps=1e-8, **HP[family][i % len(HP[family])])


# ---------------------------------------------------------------- one group: sizes, alignment, clip, steps
@pytest.mark.parametrize("family", list(HP))
def test_one_group_every_size_option_and_clip(family):
    """n in {1, 63, 64, 65, 4099} at a 16-byte boundary, 4099 one float past it (the scalar form), every option of the family and the
    clip off / active with grad_scale 1/3 / grad_scale 1/2 in rotation, over the family's step count; RAdam a second time with
    beta2 = 0.9.  The map is NULL: one group."""
    cases = [(n, 0) for n in (1, 63, 64, 65, 4099)] + [(4099, 1)]
    for b2 in (0.999, 0.9) if family == "radam" else (0.999,):
        for i, (n, shift) in enumerate(cases):
            hp, cn = hp_of(family, i, b2), list(CLIPS)[i % 3]
            p, grads = data(n, 100 + i, STEPS[family])
            r64, r32 = refs(family, p, grads, hp, cn)
            got = kernel_run(family, p, grads, [hp], cn, shift=shift)
            judge((family, n, shift, b2, cn, HP[family][i % len(HP[family])]), got, r64, r32)
            if n == 4099:      # the same launch again: the same bits; and the scalar form gives the 16-byte form's bits
                again = kernel_run(family, p, grads, [hp], cn, shift=shift)
                other = kernel_run(family, p, grads, [hp], cn, shift=1 - shift)
                for k in got:
                    assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), (family, k, "not deterministic")
                    assert np.array_equal(got[k].view(np.uint32), other[k].view(np.uint32)), (family, k, "scalar != 16-byte form")


@pytest.mark.parametrize("family", list(HP))
def test_the_stride_loop_runs_twice(family):
    """n = one grid sweep of the 16-byte form + 67: the last 67 elements are the second trip (and its scalar tail)."""
    from qflux_amd import ops
    n = ops.grouped_sweep_elems(0) + 67
    hp = hp_of(family, 1)
    p, grads = data(n, 7, 2)
    r64, r32 = refs(family, p, grads, hp, "active_third")
    got = kernel_run(family, p, grads, [hp], "active_third")
    tail = np.zeros(n, bool)
    tail[-67 - 64:] = True
    judge((family, n, "second trip"), got, r64, r32, mask=tail)
    judge((family, n, "whole"), got, r64, r32)


@pytest.mark.parametrize("family,option", [(f, o) for f in HP for o in range(3)])
def test_exact_step_gives_torchs_fp32_bits(family, option):
    p, grads, hp = CPU.exact_case(family, option=option)
    want_p, want = CPU.torch_run(family, p.astype(F32), [g.astype(F32) for g in grads], hp, torch.float32)
    exact_p, exact = R.run(family, p, grads, hp)
    for shift in (0, 1):
        got = kernel_run(family, p, grads, [hp], "off", shift=shift)
        for k, w, x in (("p", want_p, exact_p), ("exp_avg", want["exp_avg"], exact["exp_avg"]),
                        ("second", want[R.SECOND[family]], exact[R.SECOND[family]])):
            assert np.array_equal(got[k].view(np.uint32), np.asarray(w, F32).view(np.uint32)), (family, option, shift, k)
            assert np.array_equal(got[k].astype(F64), x), (family, option, shift, k)


@pytest.mark.parametrize("family", list(HP))
@pytest.mark.parametrize("n", [64 * 4 + 3, 4096 * 1024 + 64 + 3])
def test_exact_step_with_a_quad_body_a_tail_and_a_second_trip(family, n):
    """The exact case at a length with a 16-byte body and an n % 4 tail (also one float past a 16-byte boundary: the scalar form), and
    at one where 4096 workgroups of 256 quads leave a second trip of the stride loop with such a tail behind it: torch's fp32 bits."""
    p, grads, hp = CPU.exact_case(family, n=n, option=1)
    want_p, want = CPU.torch_run(family, p.astype(F32), [g.astype(F32) for g in grads], hp, torch.float32)
    for shift in (0, 1) if n < 1024 else (0,):
        got = kernel_run(family, p, grads, [hp], "off", shift=shift)
        for k, w in (("p", want_p), ("exp_avg", want["exp_avg"]), ("second", want[R.SECOND[family]])):
            assert np.array_equal(got[k].view(np.uint32), np.asarray(w, F32).view(np.uint32)), (family, n, shift, k)


# ---------------------------------------------------------------- parameter groups
def layout(n_tensors):
    """Tensors of odd sizes at multiples of 64, as LoraStore lays them out: [(off, numel)], the padded extent, the pad slots."""
    sizes = [37, 64, 65, 130, 200, 7, 128, 1, 63, 257, 90, 64, 33, 191, 5, 129, 70, 300, 2, 66][:n_tensors]
    entries, off = [], 0
    for k in sizes:
        entries.append((off, k))
        off += (k + 63) // 64 * 64
    return entries, off, [(o + k, (o + k + 63) // 64 * 64) for o, k in entries]


@pytest.mark.parametrize("family", list(HP))
@pytest.mark.parametrize("n_groups", [1, 2, 16])
def test_groups_step_every_tensor_with_its_row(family, n_groups):
    from qflux_amd import ops
    entries, n, pads = layout(20)
    assign = [i % n_groups for i in range(len(entries))]
    tmap = ops.tile_group_map(entries, assign, n_groups, numel=n).numpy()
    elem = np.repeat(tmap, 64)[:n].astype(np.int64)
    rows = [dict(hp_of(family, k, lr=0.01 * (1 + k)), beta1=0.9 - 0.02 * k, beta2=0.999 - 0.01 * k, eps=1e-8 * (1 + k)) for k in range(n_groups)]
    p, grads = data(n, 31 + n_groups, STEPS[family], pads)
    cn = "active_third"
    got = {s: kernel_run(family, p, grads, rows, cn, tile_map=tmap, shift=s) for s in (0, 1)}
    for k in got[0]:
        assert np.array_equal(got[0][k].view(np.uint32), got[1][k].view(np.uint32)), (family, k, "scalar != 16-byte form")
        for a, b in pads:
            assert not got[0]["p"][a:b].view(np.uint32).any()      # the padding of the parameters stays +0
    for gi, hp in enumerate(rows):
        mask = elem == gi
        single = kernel_run(family, p, grads, [hp], cn)      # one group, NULL map, this group's scalars
        for k in single:
            assert np.array_equal(got[0][k][mask].view(np.uint32), single[k][mask].view(np.uint32)), (family, n_groups, gi, k)
        if gi in (0, n_groups - 1):
            r64, r32 = refs(family, p, grads, hp, cn)
            judge((family, "groups", n_groups, gi), got[0], r64, r32, mask=mask)


@pytest.mark.parametrize("family", list(HP))
def test_a_map_entry_past_n_groups_takes_the_last_row(family):
    from qflux_amd import ops
    entries, n, pads = layout(8)
    assign = [i % 2 for i in range(len(entries))]
    good = ops.tile_group_map(entries, assign, 2, numel=n).numpy()
    bad = good.copy()
    ones = np.flatnonzero(good == 1)
    bad[ones[0]], bad[ones[-1]] = 2, 255
    rows = [hp_of(family, 0), dict(hp_of(family, 1, lr=0.04), beta1=0.8)]
    p, grads = data(n, 9, 2, pads)
    for shift in (0, 1):
        want = kernel_run(family, p, grads, rows, "off", tile_map=good, shift=shift)
        got = kernel_run(family, p, grads, rows, "off", tile_map=bad, shift=shift)
        for k in got:
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (family, shift, k)


def test_refusals_happen_before_any_launch():
    """QFX_EINVAL for every case of include/qfx.h; the pointers handed over are not memory, so a launch would have faulted -- and the
    device still computes afterwards."""
    CPU.check_refusals(_lib())
    torch.cuda.synchronize()
    assert float(torch.ones(4, device=DEV).sum()) == 4.0


# ---------------------------------------------------------------- the fused train step against the real torch.optim classes
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


@pytest.mark.parametrize("family,kw", [("radam", dict(weight_decay=0.01, decoupled_weight_decay=True)), ("nadam", dict(momentum_decay=0.01))])
def test_fused_train_steps_agree_with_the_autograd_path_under_the_real_class_and_resume_bit_for_bit(family, kw):
    """Three fused train steps (forward, backward, clip, the family's launch) against the same model on the autograd path stepped by
    the real torch.optim class after clip_grad_norm_.  The bars are the ones the fused AdamW class is held to against stock
    torch.optim.AdamW in the reference's loop (tests/test_optim_classes_gpu.py, from parity_util.QWEN_BARS): every loss within
    4 QWEN_BARS[0] relative, the cosine of the two total updates above 0.9; the adapter weights' relative distance is printed.
    Then: two steps, state_dict, a fresh step object that loads it, one more step == three uninterrupted steps, bit for bit."""
    from qflux_amd.trainer import QwenLoraTrainStep
    a, b = _twins()
    start = _TWINS["start"]
    lr, steps = 3e-3, 3
    args = {k: v for k, v in kw.items() if k != "weight_decay"}
    wd = kw.get("weight_decay", 0.0)
    pool = [tiny_embeddings(seed=400 + i) for i in range(steps)]
    fused = QwenLoraTrainStep(a, lr=lr, weight_decay=wd, max_grad_norm=1.0, optimizer=family, optimizer_args=args)
    helper = QwenLoraTrainStep(b)
    params = [p for n, p in b.named_parameters() if "lora_" in n]
    stock = getattr(torch.optim, R.TORCH[family])(params, lr=lr, weight_decay=wd, foreach=False, **args)
    la, lb, mid = [], [], None
    for it, (emb, noise, u) in enumerate(pool):
        la.append(fused.train_step(emb, noise=noise, u=u).item())
        loss = helper.compute_loss(emb, noise=noise, u=u)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        stock.step()
        stock.zero_grad()
        lb.append(loss.item())
        if it == steps - 2:
            mid = (fused.state_dict(), a.lora_store.pflat.detach().clone())
    want = a.lora_store.pflat.detach().clone()
    du_a, du_b = (want - start).flatten(), (b.lora_store.pflat.detach() - start).flatten()
    rel = [abs(x - y) / abs(y) for x, y in zip(la, lb)]
    cos = float(torch.dot(du_a, du_b) / (du_a.norm() * du_b.norm() + 1e-30))
    dist = float((du_a - du_b).norm() / du_b.norm())
    print(family, "fused vs torch.optim on the autograd path: loss rel", rel, "update cosine", cos, "relative distance of the updates", dist)
    _STATS["records"].append({"case": (family, "train step"), "loss_rel": rel, "update_cosine": cos, "update_rel_distance": dist})
    _observe(None, None, dump=("adamx_parity_gpu.json", _STATS))
    assert max(rel) < QWEN_BARS[0] * 4, rel
    assert cos > 0.9 and float(du_a.abs().max()) > 0, cos
    assert set(next(iter(mid[0]["state"].values()))) == CPU.KEYS[family]
    # resume
    a2, _ = _twins()
    with torch.no_grad():
        a2.lora_store.pflat.copy_(mid[1])
    resumed = QwenLoraTrainStep(a2, lr=123.0, max_grad_norm=1.0, optimizer=family)
    resumed.load_state_dict(mid[0])
    assert resumed.global_step == steps - 1 and resumed.lr == lr and all(resumed.optimizer_args[k] == v for k, v in args.items())
    emb, noise, u = pool[-1]
    resumed.train_step(emb, noise=noise, u=u)
    assert torch.equal(a2.lora_store.pflat.detach(), want)
