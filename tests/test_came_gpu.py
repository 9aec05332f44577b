"""GPU: qfx_came_step against the restatement tests/came_ref.py, 3 steps from zero state with fresh random gradients, one flat buffer
holding [16, 3072] and [3072, 16] (the two real adapter shapes), [64, 320] and [12288, 16] (the long side crosses more than one
streaming trip, and is on the rows), [4, 40] and [40, 4] (smaller than one wave), [1, 7] (one row: mean(row) over one element),
[3, 129] (odd: no 16-byte alignment holds) and [130] (unfactored).  Two packings: "unaligned" (offsets that are multiples of
nothing: every access is a 4-byte one) and "aligned" (every tensor on a 16-byte boundary: the 16-byte accesses run wherever cols is a
multiple of 4); the two must give the same bits, since the order of every sum is fixed by the shape alone.

Metric, per tensor and per quantity (p, RMS, exp_avg, the four factored statistics or exp_avg_sq): max |kernel - ref64| / max |ref64|
with ref64 the restatement in float64.  Bar: tests/test_adafactor_gpu.py's, unchanged -- 8 x the same metric of the float32
restatement against ref64 on the same inputs (the kernel's sums run in another order than torch's), never tighter than 2^-23.
profiles/came.json records the observed figures and the bars under "parity".
Also: two runs give the same bits, a non-finite gradient skips its tensor alone, a checkpoint written by save_checkpoint resumes
bit identically, optimizer="came" in QwenLoraTrainStep / FluxKontextTrainStep equals qflux_amd.optim.CAME stepping a twin model
through the same gradients, and EMA and max-norm run behind the CAME step."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import came_ref as R  # noqa: E402
import ema_ref as E  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(16, 3072), (3072, 16), (64, 320), (12288, 16), (4, 40), (40, 4), (1, 7), (3, 129), (130,)]
STEPS = 3
FLOOR = 2.0 ** -23
LR = 1e-3
CONFIGS = {
    "defaults": dict(),
    "decay": dict(weight_decay=0.01),
    "clip": dict(clip_threshold=0.5, grad_mult=4.0),       # gradients scaled up: the update clip engages at every step (asserted)
    "gnorm": dict(max_norm=None, grad_scale=0.5),          # max_norm: half the smallest scaled gradient norm, active at every step
    "no_momentum": dict(betas=(0.0, 0.9, 0.9)),
}
NOT_OPTS = ("max_norm", "grad_scale", "grad_mult")
STATS = ("row", "col", "rrow", "rcol", "v", "rms", "m")
_CACHE = {}


def _numel(s):
    n = 1
    for d in s:
        n *= d
    return n


def layout(packing="unaligned"):
    """(offset, shape) of every tensor.  unaligned: 3 unused elements after each one from offset 5 on, so no offset is a multiple of
    4 (asserted); aligned: every offset is the next multiple of 4."""
    out, off = [], 5 if packing == "unaligned" else 0
    for s in SHAPES:
        if packing == "unaligned" and off % 4 == 0:
            off += 1
        out.append((off, s))
        off += _numel(s) + 3
        if packing == "aligned":
            off = (off + 3) // 4 * 4
    assert all((o % 4 == 0) == (packing == "aligned") for o, _ in out)
    return out, off


def data():
    """Per-tensor parameters and STEPS gradients, built once and never written; flat() packs them."""
    if "data" not in _CACHE:
        g = torch.Generator().manual_seed(2025)
        ps = [torch.randn(s, generator=g) * 0.1 for s in SHAPES]
        grads = [[torch.randn(s, generator=g) * 1e-2 * (1 + t) for s in SHAPES] for t in range(STEPS)]
        _CACHE["data"] = (ps, grads)
    return _CACHE["data"]


def flat(tensors, packing, fill=0.0):
    ents, n = layout(packing)
    f = torch.full((n,), fill)
    for (off, s), t in zip(ents, tensors):
        f[off:off + _numel(s)] = t.reshape(-1)
    return f


def grads_of(cfg, grads=None):
    grads = data()[1] if grads is None else grads
    k = cfg.get("grad_mult", 1.0)
    return [[g * k for g in step] for step in grads]


def resolved(name):
    cfg = dict(CONFIGS[name])
    if "max_norm" in cfg:
        norms = [torch.cat([g.reshape(-1) for g in step]).double().norm() * cfg["grad_scale"] for step in grads_of(cfg)]
        cfg["max_norm"] = 0.5 * min(float(x) for x in norms)
    return cfg


def run_kernel(cfg, grads, packing="unaligned", steps=None):
    """-> dict of CPU tensors p and STATS, the fp32 gnorm_sq values the launches read (None without a global clip), the layout."""
    from qflux_amd import ops
    ents, n = layout(packing)
    opts = {k: v for k, v in cfg.items() if k not in NOT_OPTS}
    lay = ops.came_table(ents, device=DEV)
    p = flat(data()[0], packing, fill=7.0).to(DEV)                  # 7.0 in the padding: nothing outside the tensors may move
    z = lambda k: torch.zeros(max(1, k), device=DEV)
    st = dict(row=z(lay.n_row), col=z(lay.n_col), rrow=z(lay.n_row), rcol=z(lay.n_col), v=z(lay.n_v), rms=z(lay.n_tensors), m=z(n))
    nsq, parts, norms = torch.zeros((), device=DEV), torch.zeros(1024, device=DEV), []
    clip = cfg.get("max_norm", 0.0) > 0
    for g in grads[:steps]:
        gh = flat(g, packing)
        gd = gh.to(DEV)
        if clip:
            ops.sumsq_det(gd, nsq, parts)
            norms.append(nsq.item())
        ops.came_step(p, gd, st["row"], st["col"], st["rrow"], st["rcol"], st["v"], st["m"], st["rms"], lay, LR,
                      gnorm_sq=nsq if clip else None, max_norm=cfg.get("max_norm", 0.0), grad_scale=cfg.get("grad_scale", 1.0), **opts)
        assert torch.equal(gd.cpu().view(torch.int32), gh.view(torch.int32))          # the gradient is read only (bits: it may hold nan)
    out = {k: v.cpu() for k, v in st.items()}
    out["p"] = p.cpu()
    return out, (norms if clip else None), lay


def run_ref(cfg, grads, norms, dtype):
    """-> parameters, state, and the update-clip divisor of every tensor at every step."""
    opts = {k: v for k, v in cfg.items() if k not in NOT_OPTS}
    ps = [p.to(dtype).clone() for p in data()[0]]
    st, dens = R.new_state(SHAPES, dtype=dtype), []
    for t, g in enumerate(grads):
        dens.append(R.step(ps, g, st, dtype=dtype, lr=LR, gnorm_sq=None if norms is None else norms[t], max_norm=cfg.get("max_norm", 0.0),
                           grad_scale=cfg.get("grad_scale", 1.0), **opts))
    return ps, st, dens


def per_tensor(out, lay):
    """The kernel's flat buffers cut into the restatement's per-tensor pieces: [(name, tensor)] per entry."""
    res = []
    for i, (off, rows, cols, factored, r0, c0, v0) in enumerate(lay.tensors):
        n, shape = rows * cols, SHAPES[i]
        e = [("p", out["p"][off:off + n].view(shape)), ("RMS", out["rms"][i]), ("exp_avg", out["m"][off:off + n].view(shape))]
        if factored:
            e += [("exp_avg_sq_row", out["row"][r0:r0 + rows]), ("exp_avg_sq_col", out["col"][c0:c0 + cols]),
                  ("exp_avg_res_row", out["rrow"][r0:r0 + rows]), ("exp_avg_res_col", out["rcol"][c0:c0 + cols])]
        else:
            e += [("exp_avg_sq", out["v"][v0:v0 + n].view(shape))]
        res.append(e)
    return res


def metric(a, ref64):
    return ((a.double() - ref64).abs().max() / ref64.abs().max()).item()


def kernel_run(name, packing="unaligned"):
    if ("k", name, packing) not in _CACHE:
        cfg = resolved(name)
        _CACHE[("k", name, packing)] = run_kernel(cfg, grads_of(cfg), packing)
    return _CACHE[("k", name, packing)]


def compare(name, packing="unaligned"):
    """-> [(shape, quantity, kernel's metric, the fp32 restatement's own, bar)] for every tensor and quantity, and the run."""
    cfg = resolved(name)
    grads = grads_of(cfg)
    out, norms, lay = kernel_run(name, packing)
    p32, s32, _ = run_ref(cfg, grads, norms, torch.float32)
    p64, s64, dens = run_ref(cfg, grads, norms, torch.float64)
    rows = []
    for i, pieces in enumerate(per_tensor(out, lay)):
        for key, got in pieces:
            r32, r64 = (p32[i], p64[i]) if key == "p" else (s32[i][key], s64[i][key])
            assert torch.isfinite(got).all() and r64.abs().max() > 0, (SHAPES[i], key)
            own, mine = metric(r32, r64), metric(got, r64)
            rows.append((SHAPES[i], key, mine, own, max(8 * own, FLOOR)))
    return rows, (cfg, out, norms, lay, dens)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_kernel_matches_the_restatement(name):
    rows, (cfg, out, norms, lay, dens) = compare(name)
    worst = []
    for shape, key, mine, own, bar in rows:
        print(f"came {name} {shape} {key}: kernel {mine:.2e} fp32 restatement {own:.2e} bar {bar:.2e}")
        if mine > bar:
            worst.append((shape, key, mine, bar))
    assert not worst, worst
    start = flat(data()[0], "unaligned", fill=7.0)
    assert metric(out["p"], start.double()) > 1e-4                # the parameters moved by more than any bar
    pad = torch.ones_like(start, dtype=torch.bool)
    for off, s in layout()[0]:
        pad[off:off + _numel(s)] = False
    assert torch.equal(out["p"][pad], start[pad]) and not out["m"][pad].any()      # nothing outside the tensors is written
    assert all(d is not None and d >= 1.0 for step in dens for d in step)
    if name == "clip":
        assert all(d > 1.0 for step in dens for d in step)        # the update clip engaged on every tensor at every step
    if name == "gnorm":
        assert all((n ** 0.5) * cfg["grad_scale"] > 1.9 * cfg["max_norm"] for n in norms)


@pytest.mark.parametrize("name", ["decay", "gnorm"])
def test_aligned_packing_gives_the_bits_of_the_unaligned_one(name):
    """The 16-byte accesses (aligned packing, cols a multiple of 4) and the 4-byte ones add in the same order."""
    a, _, la = kernel_run(name, "aligned")
    b, _, lb = kernel_run(name, "unaligned")
    assert all(x[0] % 4 == 0 for x in la.tensors) and not any(x[0] % 4 == 0 for x in lb.tensors)
    for i, (pa, pb) in enumerate(zip(per_tensor(a, la), per_tensor(b, lb))):
        for (key, x), (_, y) in zip(pa, pb):
            assert torch.equal(x, y), (SHAPES[i], key)


def test_two_runs_give_identical_bits():
    for name, packing in (("decay", "unaligned"), ("gnorm", "aligned")):
        cfg = resolved(name)
        a, b = kernel_run(name, packing)[0], run_kernel(cfg, grads_of(cfg), packing)[0]
        for k in a:
            assert torch.equal(a[k], b[k]), (name, k)


def test_non_finite_gradient_skips_its_tensor_alone():
    """+inf, nan, -inf in the [4, 40] tensor's gradient, a different element at every step, clip off (max_norm = 0, no gnorm_sq):
    that tensor keeps its parameters, its five statistics, m and rms bit for bit (zero state), every other tensor equals the run
    without them (which matches the restatement: test_kernel_matches_the_restatement)."""
    clean, _, lay = kernel_run("defaults")
    bad_i = SHAPES.index((4, 40))
    grads = [[g.clone() for g in step] for step in data()[1]]
    for s, step in enumerate(grads):
        step[bad_i].view(-1)[17 * s + 3] = (float("inf"), float("nan"), float("-inf"))[s % 3]
    out, _, _ = run_kernel(resolved("defaults"), grads)
    a, b = per_tensor(out, lay), per_tensor(clean, lay)
    for i in range(len(SHAPES)):
        for (key, x), (_, y) in zip(a[i], b[i]):
            if i != bad_i:
                assert torch.equal(x, y), (SHAPES[i], key)
            elif key == "p":
                assert torch.equal(x, data()[0][bad_i])
            else:
                assert not x.any(), key
    assert b[bad_i][1][1] > 0 and not torch.equal(b[bad_i][0][1], a[bad_i][0][1])      # the clean run did step that tensor


TARGETS = ("to_k", "to_q", "to_v", "to_out.0", "img_mlp.net.2")


def _pair(seed=2):
    from common import TINY
    from parity_util import build_pair
    return build_pair(dict(TINY), device=DEV, targets=TARGETS, seed=seed)[1]


def _same_state(sa, sb):
    for (n, x), (_, y) in zip(sa.opt_state.buffers(), sb.opt_state.buffers()):
        assert E.same_bits(x, y), n
    assert [n for n, _ in sa.opt_state.buffers()] == list(STATS)


def test_checkpoint_round_trip_is_bit_identical(tmp_path):
    """3 straight steps == 2 steps, save_checkpoint, load_checkpoint into a fresh step on a fresh model, 1 step."""
    from parity_util import tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    from qflux_amd.trainer.optim_state import CameState
    kw = dict(lr=2e-3, weight_decay=1e-2, optimizer="came")
    batches = [tiny_embeddings(seed=5 + i) for i in range(3)]
    a, b, c = _pair(), _pair(), _pair()
    sa, sb = QwenLoraTrainStep(a, **kw), QwenLoraTrainStep(b, **kw)
    start = a.lora_store.pflat.detach().clone()
    for e, nz, u in batches:
        sa.train_step(e, noise=nz, u=u)
    for e, nz, u in batches[:2]:
        sb.train_step(e, noise=nz, u=u)
    ck = str(tmp_path / "ck")
    sb.save_checkpoint(ck)
    sd = torch.load(os.path.join(ck, "optimizer.bin"), map_location="cpu", weights_only=False)
    assert all(set(e) == set(CameState.FACTORED_KEYS) and e["step"] == 2 for e in sd["state"].values()) and len(sd["state"]) == len(b.lora_store.entries)
    assert sd["param_groups"][0]["betas"] == (0.9, 0.999, 0.9999) and sd["param_groups"][0]["eps"] == (1e-30, 1e-16)
    sc = QwenLoraTrainStep(c, lr=0.5, betas=(0.5, 0.5, 0.5), optimizer="came", optimizer_args={"clip_threshold": 3.0})
    sc.load_checkpoint(ck, adapter_name="lora_edit")
    assert sc.global_step == 2 and sc.lr == 2e-3 and sc.betas == (0.9, 0.999, 0.9999) and sc.optimizer_args["clip_threshold"] == 1.0
    e, nz, u = batches[2]
    sc.train_step(e, noise=nz, u=u)
    assert E.same_bits(a.lora_store.pflat, c.lora_store.pflat) and not E.same_bits(a.lora_store.pflat, start)
    _same_state(sa, sc)
    assert bool(sa.opt_state.rrow.all()) and bool(sa.opt_state.rms[:len(a.lora_store.entries)].all())


def _lora_params(m):
    return [p for n, p in m.named_parameters() if "lora_" in n]


def _assert_train_step_equals_the_class(step, helper, opt, batches):
    """`step` runs train_step on its model; the twin model gets the same fused forward/backward through `helper` and is stepped by
    the torch.optim class `opt`, as the drop-in loop steps it: equal weights in, equal gradient bits, and then equal weights out."""
    a, b = step.dit.lora_store, helper.dit.lora_store
    assert torch.equal(a.pflat, b.pflat)
    start = a.pflat.detach().clone()
    for emb, extra in batches:
        loss = step.train_step(emb, **extra)
        helper.forward_backward(emb, **extra)
        opt.step()
        opt.zero_grad()                       # set_to_none; the next access to lora_store re-attaches zeroed views
        helper.zero_grad()
        assert torch.isfinite(loss).all()
        assert torch.equal(a.pflat, b.pflat)
    assert torch.isfinite(a.pflat).all() and not torch.equal(a.pflat, start)
    for (n, x), (_, y) in zip(step.opt_state.buffers(), opt._opt_state.buffers()):
        assert torch.equal(x, y), n
    assert step.state_dict()["state"][0]["step"] == len(batches) == opt.state_dict()["state"][0]["step"]


def test_qwen_train_step_equals_the_optim_class_on_a_twin():
    from common import TINY
    from parity_util import build_pair, tiny_embeddings
    from qflux_amd import optim as O
    from qflux_amd.trainer import QwenLoraTrainStep
    a, b = (build_pair(dict(TINY), device=DEV, seed=2)[1] for _ in range(2))
    step = QwenLoraTrainStep(a, lr=2e-3, weight_decay=1e-2, max_grad_norm=0, optimizer="came")
    helper = QwenLoraTrainStep(b, max_grad_norm=0)
    opt = O.CAME(_lora_params(b), lr=2e-3, weight_decay=1e-2)
    batches = []
    for i in range(2):
        e, nz, u = tiny_embeddings(seed=5 + i)
        batches.append((e, dict(noise=nz, u=u)))
    _assert_train_step_equals_the_class(step, helper, opt, batches)


def _flux_model():
    from common import FLUX_TINY
    from qflux_amd.models import FluxTransformer2DModel
    from qflux_amd.modules import LoraConfig
    cfg = dict(FLUX_TINY, joint_attention_dim=64, guidance_embeds=True)
    with torch.device(DEV):
        m = FluxTransformer2DModel(**cfg)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_((torch.randn(p.shape, generator=g) * (0.5 / p.shape[-1] ** 0.5 if p.ndim == 2 else 0.05) + (1.0 if "norm_" in n and p.ndim == 1 else 0.0)).to(p.dtype))
    m.add_adapter(LoraConfig(r=4, lora_alpha=8), "a", generator=g)
    return m, g


def test_flux_train_step_equals_the_optim_class_on_a_twin():
    from oracle import flux_dit as FO
    from qflux_amd import optim as O
    from qflux_amd.trainer import FluxKontextTrainStep
    (a, g), (b, _) = _flux_model(), _flux_model()
    step = FluxKontextTrainStep(a, lr=1e-3, betas=(0.8, 0.99, 0.999), max_grad_norm=0, optimizer="came", optimizer_args={"clip_threshold": 0.5})
    helper = FluxKontextTrainStep(b, max_grad_norm=0)
    opt = O.CAME(_lora_params(b), lr=1e-3, betas=(0.8, 0.99, 0.999), clip_threshold=0.5)
    ctl = FO.prepare_latent_image_ids(4, 6); ctl[:, 0] = 1
    emb = dict(image_latents=torch.randn(2, 24, 64, generator=g).half(), control_latents=torch.randn(2, 24, 64, generator=g).half(),
               control_ids=ctl, text_ids=torch.zeros(7, 3), latent_hw=(4, 6),
               pooled_prompt_embeds=torch.randn(2, 16, generator=g).half(), prompt_embeds=torch.randn(2, 7, 64, generator=g).half())
    batches = [(emb, dict(noise=torch.randn(2, 24, 64, generator=g), t=torch.tensor([0.3, 0.8]))) for _ in range(2)]
    _assert_train_step_equals_the_class(step, helper, opt, batches)


def test_ema_and_max_norm_run_behind_the_came_step():
    """ema_decay=0.9 and max_weight_norm=1.0 behind optimizer="came": the shadow is the hand formula (tests/ema_ref.py) on the weights
    CAME (and then the clamp) produced, and no adapter pair is left above the threshold."""
    from parity_util import tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    a = _pair()
    step = QwenLoraTrainStep(a, lr=2e-3, optimizer="came", ema_decay=0.9, max_weight_norm=1.0)
    ref = E.Ema([a.lora_store.pflat.detach().clone()], 0.9)
    e, nz, u = tiny_embeddings(seed=5)
    for it in range(3):
        step.train_step(e, noise=nz, u=u)
        ref.step([a.lora_store.pflat])
    assert E.same_bits(step.ema.shadows[0], ref.shadow[0]) and not E.same_bits(step.ema.shadows[0], a.lora_store.pflat)
    norms = step.last_weight_norms.norms.cpu()
    assert bool(torch.isfinite(norms).all()) and 0 < float(norms.max()) <= 1.0 * (1 + 1e-6)
