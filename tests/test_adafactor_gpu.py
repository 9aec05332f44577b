"""GPU: qfx_adafactor_step against the restatement tests/adafactor_ref.py, 5 steps with fresh random gradients, one flat buffer holding
[1, 32] (a single row), [3, 40] (columns no multiple of the wave), [130, 5] (many short rows), [64, 1031] (more than one sweep per
thread), [16, 3072] and [3072, 16] (the two real adapter shapes) and [7] (unfactored), at offsets that are multiples of nothing.

Metric, per tensor and per quantity (p, row, col, v, m, RMS): max |kernel - ref64| / max |ref64| with ref64 the restatement in float64.
Bar: 8 x the same metric of the float32 restatement against ref64 on the same inputs (the kernel's sums run in another order than
torch's: 8 x leaves room for a tree-order sum against a sequential one over at most 3072 terms), never tighter than 2^-23.
The float32 restatement's own figures on these inputs (computed on the CPU; maximum over the tensors, per configuration):
    defaults     p 1.5e-07  row 1.4e-07  col 1.6e-07  v 6.4e-08  RMS 5.2e-08
    external_lr  p 2.8e-07  row 1.4e-07  col 1.6e-07  v 6.4e-08  m 2.0e-07  RMS 6.3e-08
    warmup       p 1.4e-07  row 1.4e-07  col 1.6e-07  v 6.4e-08  RMS 6.4e-08
    clip         p 1.4e-07  row 1.9e-07  col 1.6e-07  v 3.5e-08  RMS 9.4e-08
(for "clip" with torch's fp32 sum of squares standing in for the device's gnorm_sq).
Also: two runs give the same bits, a non-finite gradient skips its tensor alone, a checkpoint in transformers' layout resumes bit
identically, and optimizer="adafactor" in QwenLoraTrainStep / FluxKontextTrainStep equals qflux_amd.optim.Adafactor stepping a twin
model through the same gradients."""
import types

import pytest
import torch

import adafactor_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 32), (3, 40), (130, 5), (64, 1031), (16, 3072), (3072, 16), (7,)]
STEPS = 5
FLOOR = 2.0 ** -23
CONFIGS = {
    "defaults": dict(),
    "external_lr": dict(lr=1e-3, relative_step=False, beta1=0.9, weight_decay=1e-2),
    "warmup": dict(warmup_init=True),
    "clip": dict(max_norm=None, grad_scale=0.25),          # max_norm: half the smallest scaled gradient norm, active at every step
}
_CACHE = {}


def _numel(s):
    n = 1
    for d in s:
        n *= d
    return n


def layout():
    """(offset, shape) of every tensor: 3 unused elements after each one, so no offset is aligned to anything."""
    out, off = [], 5
    for s in SHAPES:
        out.append((off, s))
        off += _numel(s) + 3
    return out, off


def data():
    """Flat parameters and STEPS flat gradients (zero in the padding), built once and never written."""
    if "data" not in _CACHE:
        ents, n = layout()
        g = torch.Generator().manual_seed(2024)
        p = torch.randn(n, generator=g) * 0.1
        grads = []
        for s in range(STEPS):
            f = torch.zeros(n)
            for off, shape in ents:
                f[off:off + _numel(shape)] = torch.randn(_numel(shape), generator=g) * 1e-2 * (1 + s)
            grads.append(f)
        _CACHE["data"] = (p, grads)
    return _CACHE["data"]


def resolved(name, grads=None):
    cfg = dict(CONFIGS[name])
    if "max_norm" in cfg:
        grads = data()[1] if grads is None else grads
        cfg["max_norm"] = 0.5 * min(float((g.double() * cfg["grad_scale"]).norm()) for g in grads)
    return cfg


def run_kernel(cfg, grads, p0=None, steps=None, state=None, t0=0):
    """-> dict of CPU tensors p, row, col, v, m, rms and the fp32 gnorm_sq values the launches read (None without a clip)."""
    from qflux_amd import ops
    ents, n = layout()
    opts = {k: v for k, v in cfg.items() if k not in ("max_norm", "grad_scale")}
    lay = ops.adafactor_table(ents, device=DEV)
    p = (data()[0] if p0 is None else p0).clone().to(DEV)
    if state is None:
        z = lambda k: torch.zeros(max(1, k), device=DEV)
        state = dict(row=z(lay.n_row), col=z(lay.n_col), v=z(lay.n_v), rms=z(lay.n_tensors),
                     m=torch.zeros(n, device=DEV) if opts.get("beta1") is not None else None)
    else:
        state = {k: (None if v is None else v.clone().to(DEV)) for k, v in state.items() if k != "p"}
    nsq, parts, norms = torch.zeros((), device=DEV), torch.zeros(1024, device=DEV), []
    clip = cfg.get("max_norm", 0.0) > 0
    for s, g in enumerate(grads[:steps]):
        gd = g.to(DEV)
        if clip:
            ops.sumsq_det(gd, nsq, parts)
            norms.append(nsq.item())
        ops.adafactor_step(p, gd, state["row"], state["col"], state["v"], state["m"], state["rms"], lay, t0 + s + 1,
                           gnorm_sq=nsq if clip else None, max_norm=cfg.get("max_norm", 0.0), grad_scale=cfg.get("grad_scale", 1.0), **opts)
        assert torch.equal(gd.cpu().view(torch.int32), g.view(torch.int32))          # the gradient is read only (bits: it may hold nan)
    out = {k: (None if v is None else v.cpu()) for k, v in state.items()}
    out["p"] = p.cpu()
    return out, (norms if clip else None), lay


def run_ref(cfg, grads, norms, dtype):
    ents, _ = layout()
    opts = {k: v for k, v in cfg.items() if k not in ("max_norm", "grad_scale")}
    p0 = data()[0]
    ps = [p0[off:off + _numel(s)].view(s).to(dtype).clone() for off, s in ents]
    st = R.new_state(SHAPES, beta1=opts.get("beta1"), dtype=dtype)
    for t, g in enumerate(grads):
        gs = [g[off:off + _numel(s)].view(s) for off, s in ents]
        R.step(ps, gs, st, t + 1, dtype=dtype, gnorm_sq=None if norms is None else norms[t], max_norm=cfg.get("max_norm", 0.0),
               grad_scale=cfg.get("grad_scale", 1.0), **opts)
    return ps, st


def per_tensor(out, lay):
    """The kernel's flat buffers cut into the restatement's per-tensor pieces: [(name, tensor)] per entry."""
    res = []
    for i, (off, rows, cols, factored, r0, c0, v0) in enumerate(lay.tensors):
        n, shape = rows * cols, SHAPES[i]
        e = [("p", out["p"][off:off + n].view(shape)), ("RMS", out["rms"][i])]
        if factored:
            e += [("exp_avg_sq_row", out["row"][r0:r0 + rows]), ("exp_avg_sq_col", out["col"][c0:c0 + cols])]
        else:
            e += [("exp_avg_sq", out["v"][v0:v0 + n].view(shape))]
        if out["m"] is not None:
            e += [("exp_avg", out["m"][off:off + n].view(shape))]
        res.append(e)
    return res


def metric(a, ref64):
    return ((a.double() - ref64).abs().max() / ref64.abs().max()).item()


def kernel_run(name):
    if ("k", name) not in _CACHE:
        _CACHE[("k", name)] = run_kernel(resolved(name), data()[1])
    return _CACHE[("k", name)]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_kernel_matches_the_restatement(name):
    cfg, grads = resolved(name), data()[1]
    out, norms, lay = kernel_run(name)
    p32, s32 = run_ref(cfg, grads, norms, torch.float32)
    p64, s64 = run_ref(cfg, grads, norms, torch.float64)
    worst = []
    for i, pieces in enumerate(per_tensor(out, lay)):
        for key, got in pieces:
            r32, r64 = (p32[i], p64[i]) if key == "p" else (s32[i][key], s64[i][key])
            assert torch.isfinite(got).all() and r64.abs().max() > 0
            own, mine = metric(r32, r64), metric(got, r64)
            bar = max(8 * own, FLOOR)
            print(f"adafactor {name} {SHAPES[i]} {key}: kernel {mine:.2e} fp32 restatement {own:.2e} bar {bar:.2e}")
            if mine > bar:
                worst.append((SHAPES[i], key, mine, bar))
    assert not worst, worst
    moved = metric(out["p"], data()[0].double())
    assert moved > (1e-4 if name != "warmup" else 10 * FLOOR)      # the parameters moved by more than any bar (warm-up: lr = 1e-6 t)
    pad = torch.ones_like(out["p"], dtype=torch.bool)
    for off, s in layout()[0]:
        pad[off:off + _numel(s)] = False
    assert torch.equal(out["p"][pad], data()[0][pad])     # nothing outside the tensors is written
    if name == "clip":
        assert all((n ** 0.5) * cfg["grad_scale"] > 1.9 * cfg["max_norm"] for n in norms)


def test_two_runs_give_identical_bits():
    for name in ("external_lr", "clip"):
        a, b = kernel_run(name)[0], run_kernel(resolved(name), data()[1])[0]
        for k in a:
            assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), (name, k)


def test_non_finite_gradient_skips_its_tensor_alone():
    """+inf, nan, -inf in the [3, 40] tensor's gradient, a different element at every step, clip off (max_norm = 0, no gnorm_sq):
    that tensor keeps its parameters and its zero state bit for bit, every other tensor equals the run without them."""
    clean, _, lay = kernel_run("defaults")
    off, n = lay.tensors[1][0], 120
    grads = [g.clone() for g in data()[1]]
    for s, g in enumerate(grads):
        g[off + 17 * s + 3] = (float("inf"), float("nan"), float("-inf"))[s % 3]
    out, _, _ = run_kernel(resolved("defaults"), grads)
    a, b = per_tensor(out, lay), per_tensor(clean, lay)
    for i in range(len(SHAPES)):
        for (key, x), (_, y) in zip(a[i], b[i]):
            if i != 1:
                assert torch.equal(x, y), (SHAPES[i], key)
            elif key == "p":
                assert torch.equal(x, data()[0][off:off + n].view(3, 40))
            else:
                assert not x.any(), key
    assert b[1][1][1] > 0 and not torch.equal(b[1][0][1], a[1][0][1])      # the clean run did step that tensor


def _store(p, g):
    ents, _ = layout()
    return types.SimpleNamespace(pflat=p, gflat=g, entries=[(f"t{i}", p[off:off + _numel(s)].view(s), off, _numel(s))
                                                             for i, (off, s) in enumerate(ents)])


def test_checkpoint_round_trip_is_bit_identical(tmp_path):
    """2 steps, state_dict() -> file -> fresh state -> load_state_dict, 2 more steps == 4 uninterrupted steps."""
    from qflux_amd.trainer import optim_state as OS
    p0, grads = data()
    _, fam, cls, wd, args = OS.resolve_family("adafactor", 1e-2, {"beta1": 0.9, "relative_step": False})
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)

    def steps(store, state, t0, k):
        for s in range(t0, t0 + k):
            store.gflat.copy_(grads[s])
            state.step(store, hyper["lr"], hyper["betas"], hyper["eps"], hyper["weight_decay"], s + 1, None, 0.0, 1.0, args)
    a = _store(p0.clone().to(DEV), torch.zeros_like(p0, device=DEV))
    sa = cls(a, args)
    steps(a, sa, 0, 4)
    b = _store(p0.clone().to(DEV), torch.zeros_like(p0, device=DEV))
    sb = cls(b, args)
    steps(b, sb, 0, 2)
    torch.save(OS.state_dict(cls, sb, b, 2, args, **hyper), str(tmp_path / "optimizer.bin"))
    sd = torch.load(str(tmp_path / "optimizer.bin"), map_location="cpu", weights_only=False)
    assert set(sd["state"][0]) == {"step", "RMS", "exp_avg_sq_row", "exp_avg_sq_col", "exp_avg"}
    assert set(sd["state"][6]) == {"step", "RMS", "exp_avg_sq", "exp_avg"} and sd["state"][6]["exp_avg_sq"].shape == (7,)
    args2 = OS.resolve_family("adafactor", None, None)[4]
    hyper2 = dict(lr=None, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    sc, t = OS.load_state_dict(cls, b, sd, args2, hyper2)
    assert t == 2 and args2 == args and hyper2 == hyper and sc is not sb
    args, hyper = args2, hyper2
    steps(b, sc, 2, 2)
    assert torch.equal(a.pflat, b.pflat) and not torch.equal(a.pflat.cpu(), p0)
    for (n, x), (_, y) in zip(sa.buffers(), sc.buffers()):
        assert torch.equal(x, y), n
    assert [n for n, _ in sc.buffers()] == ["row", "col", "v", "rms", "m"]


def _lora_params(m):
    return [p for n, p in m.named_parameters() if "lora_" in n]


def _assert_train_step_equals_the_class(step, helper, opt, batches, **kw):
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
    args = {"beta1": 0.9}
    step = QwenLoraTrainStep(a, lr=None, weight_decay=1e-2, max_grad_norm=0, optimizer="adafactor", optimizer_args=args)
    helper = QwenLoraTrainStep(b, max_grad_norm=0)
    opt = O.Adafactor(_lora_params(b), beta1=0.9, weight_decay=1e-2)
    batches = []
    for i in range(3):
        e, nz, u = tiny_embeddings(seed=5 + i)
        batches.append((e, dict(noise=nz, u=u)))
    _assert_train_step_equals_the_class(step, helper, opt, batches)
    with pytest.raises(ValueError, match="relative_step"):
        step.lr = 1e-3                     # a scheduler writing an lr into a relative-step run is refused at the step, not ignored
        step.optimizer_step()


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
    step = FluxKontextTrainStep(a, lr=1e-3, max_grad_norm=0, optimizer="adafactor", optimizer_args={"relative_step": False})
    helper = FluxKontextTrainStep(b, max_grad_norm=0)
    opt = O.Adafactor(_lora_params(b), lr=1e-3, relative_step=False)
    ctl = FO.prepare_latent_image_ids(4, 6); ctl[:, 0] = 1
    emb = dict(image_latents=torch.randn(2, 24, 64, generator=g).half(), control_latents=torch.randn(2, 24, 64, generator=g).half(),
               control_ids=ctl, text_ids=torch.zeros(7, 3), latent_hw=(4, 6),
               pooled_prompt_embeds=torch.randn(2, 16, generator=g).half(), prompt_embeds=torch.randn(2, 7, 64, generator=g).half())
    extra = dict(noise=torch.randn(2, 24, 64, generator=g), t=torch.tensor([0.3, 0.8]))
    _assert_train_step_equals_the_class(step, helper, opt, [(emb, extra)])
