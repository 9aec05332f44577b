"""GPU: the fused Schedule-Free AdamW step and mode swap (qfx_sfadamw_step, qfx_sf_swap) against their CPU restatement
(tests/schedulefree_ref.py), their determinism, the trainer / sampler / checkpoint path with optimizer="adamw_schedulefree", and
the torch.optim class in the stock loop.

Every numeric comparison follows one rule (schedulefree_ref.tolerance): the restatement runs in fp64 and in fp32 on the same
inputs; the kernel's largest absolute error against the fp64 run may be at most 4 times the fp32 restatement's own largest error
against it, per buffer, plus one fp32 ulp of the buffer's largest magnitude.  Both measured errors are printed and are part of the
assertion message."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import schedulefree_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TARGETS = ("to_k", "to_q", "to_v", "to_out.0", "img_mlp.net.2")
KW = dict(lr=0.0025, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, warmup_steps=3, r=0.5, weight_lr_power=2.0)
GUARD = 12345.0


def _kernel_run(y, grads, gsq, kw, shift=0, max_norm=1.0, grad_scale=0.5):
    """qfx_sfadamw_step over the steps from `first`, on slices that start `shift` elements into larger allocations; returns one
    (y, z, v) CPU snapshot per step and the allocations (guard checks)."""
    from qflux_amd import ops
    n = y.numel()
    bufs = [torch.full((n + 8,), GUARD, device=DEV) for _ in range(4)]
    p, g, z, v = (b[shift:shift + n] for b in bufs)
    p.copy_(y.to(DEV))
    lr_max, wsum, out = -1.0, 0.0, []
    for k, (gr, s) in enumerate(zip(grads, gsq)):
        g.copy_(gr.to(DEV))
        lr_t, bc2, ckp1, lr_max, wsum = ops.sfadamw_schedule(k, kw["lr"], kw["betas"][1], kw["warmup_steps"], kw["r"], kw["weight_lr_power"],
                                                             lr_max, wsum)
        ops.sfadamw_step(p, g, z, v, lr_t, kw["betas"][0], kw["betas"][1], kw["eps"], kw["weight_decay"], bc2, ckp1, first=k == 0,
                         gnorm_sq=torch.tensor(s, dtype=torch.float32, device=DEV), max_norm=max_norm, grad_scale=grad_scale)
        torch.cuda.synchronize()
        out.append((p.cpu(), z.cpu(), v.cpu()))
    return out, bufs


_REF = {}


def _ref(n, steps):
    """The shared inputs and the restatement's fp64 / fp32 runs for one length, computed once and never modified."""
    if (n, steps) not in _REF:
        y, grads, gsq = R.make_inputs(n, steps)
        _REF[n, steps] = (y, grads, gsq, R.run(y, grads, gsq, torch.float64, **KW), R.run(y, grads, gsq, torch.float32, **KW))
    return _REF[n, steps]


def test_step_kernel_matches_restatement_over_six_steps():
    y, grads, gsq, r64, r32 = _ref(4099, 6)
    active = [s ** 0.5 * 0.5 > 1.0 for s in gsq]
    assert any(active) and not all(active)                               # the clip acts on some steps and not on others
    got, _ = _kernel_run(y, grads, gsq, KW)
    for it in range(6):
        for i, name in enumerate(("y", "z", "v")):
            R.check(name, got[it][i], r32[it][i], r64[it][i], f"n=4099 step {it} (clip {'on' if active[it] else 'off'})")
    assert not torch.equal(got[-1][0], got[-1][1])                       # y and z did part


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 255, 1027, 4099])
def test_lengths_and_alignment(n, shift):
    """16-byte path with its n % 4 tail (shift 0) and the scalar path of views off a 16-byte boundary (shift 1), the first step and
    a later one; the guard elements before and after every slice keep their bits."""
    y, grads, gsq, r64, r32 = _ref(n, 2)
    got, bufs = _kernel_run(y, grads, gsq, KW, shift=shift)
    for it in range(2):
        for i, name in enumerate(("y", "z", "v")):
            R.check(name, got[it][i], r32[it][i], r64[it][i], f"n={n} shift={shift} step {it}")
    for b in bufs:
        assert bool((b[:shift] == GUARD).all()) and bool((b[shift + n:] == GUARD).all()), (n, shift)


def test_clip_active_at_every_step_aligned_and_offset_view():
    """max_norm a quarter of the smallest scaled gradient norm, so the clip acts at both steps, at the smallest length with a 16-byte
    body and a scalar tail: the aligned run and the view one element in (the scalar instantiation) give the same bits and meet the
    restatement as every other case does."""
    n = 4 * 256 + 3
    y, grads, gsq = R.make_inputs(n, 2)
    max_norm = 0.25 * min(s ** 0.5 * 0.5 for s in gsq)
    r64, r32 = (R.run(y, grads, gsq, dt, max_norm=max_norm, **KW) for dt in (torch.float64, torch.float32))
    runs = [_kernel_run(y, grads, gsq, KW, shift=shift, max_norm=max_norm)[0] for shift in (0, 1)]
    for it in range(2):
        for i, name in enumerate(("y", "z", "v")):
            R.check(name, runs[0][it][i], r32[it][i], r64[it][i], f"n={n} clipped step {it}")
            assert torch.equal(runs[0][it][i], runs[1][it][i]), (it, name)


def test_second_trip_of_the_16_byte_form_in_the_step_and_the_swap():
    """n = 2048 workgroups x 256 quads + 64 + 3: the stride loop of the 16-byte form runs a second time, with an n % 4 tail behind it,
    in the first step (z and v written only), a later one and the swap to the averaged point."""
    from qflux_amd import ops
    n = 2048 * 1024 + 64 + 3
    y, grads, gsq, r64, r32 = _ref(n, 2)
    got, bufs = _kernel_run(y, grads, gsq, KW)
    for it in range(2):
        for i, name in enumerate(("y", "z", "v")):
            R.check(name, got[it][i], r32[it][i], r64[it][i], f"n={n} step {it}")
            R.check(name, got[it][i][-131:], r32[it][i][-131:], r64[it][i][-131:], f"n={n} step {it}, second trip")
    for b in bufs:
        assert bool((b[n:] == GUARD).all())
    yk, zk = got[1][0], got[1][1]
    p, zd = yk.to(DEV), zk.to(DEV)
    we = 1 - 1 / KW["betas"][0]
    ops.sf_swap(p, zd, KW["betas"][0], to_eval=True)
    x64, x32 = torch.lerp(yk.double(), zk.double(), we), torch.lerp(yk, zk, we)
    R.check("x", p.cpu(), x32, x64, f"eval n={n}")
    R.check("x", p.cpu()[-131:], x32[-131:], x64[-131:], f"eval n={n}, second trip")
    assert torch.equal(zd.cpu(), zk) and not torch.equal(p.cpu()[-131:], yk[-131:])


@pytest.mark.parametrize("beta1", [0.9, 0.4])
def test_swap_matches_torch_lerp_and_round_trips(beta1):
    """beta1 = 0.9: weights -0.111.. and 0.1, the |w| < 0.5 branch; beta1 = 0.4: -1.5 and 0.6, the other one."""
    from qflux_amd import ops
    g = torch.Generator().manual_seed(11)
    for n, shift in ((4099, 0), (1027, 1)):
        y, z = torch.randn(n, generator=g) * 0.1, torch.randn(n, generator=g) * 0.1
        bufs = [torch.full((n + 8,), GUARD, device=DEV) for _ in range(2)]
        p, zd = (b[shift:shift + n] for b in bufs)
        p.copy_(y.to(DEV)); zd.copy_(z.to(DEV))
        we, wt = 1 - 1 / beta1, 1 - beta1
        assert (abs(we) < 0.5) == (beta1 == 0.9) and (abs(wt) < 0.5) == (beta1 == 0.9)
        ops.sf_swap(p, zd, beta1, to_eval=True)
        x64, x32 = torch.lerp(y.double(), z.double(), we), torch.lerp(y, z, we)
        R.check("x", p.cpu(), x32, x64, f"eval beta1={beta1} n={n}")
        assert not torch.equal(p.cpu(), y)
        ops.sf_swap(p, zd, beta1, to_eval=False)
        # the round trip against the fp64 round trip (which returns y up to fp64 rounding), the fp32 one being torch.lerp twice
        R.check("y", p.cpu(), torch.lerp(x32, z, wt), torch.lerp(x64, z.double(), wt), f"round trip beta1={beta1} n={n}")
        assert torch.equal(zd.cpu(), z)
        for b in bufs:
            assert bool((b[:shift] == GUARD).all()) and bool((b[shift + n:] == GUARD).all())


def test_kernels_are_deterministic():
    from qflux_amd import ops
    n = 600003                                                           # more workgroups than the grid cap admits: the stride loop runs
    y, grads, gsq = R.make_inputs(n, 3, seed=5)
    runs = []
    for _ in range(2):
        got, _ = _kernel_run(y, grads, gsq, KW)
        p, z = got[-1][0].to(DEV), got[-1][1].to(DEV)
        ops.sf_swap(p, z, 0.9, to_eval=True)
        torch.cuda.synchronize()
        runs.append([t for snap in got for t in snap] + [p.cpu()])
    assert len(runs[0]) == 10 and all(torch.equal(a, b) for a, b in zip(*runs))
    assert not torch.equal(runs[0][-1], runs[0][-4])                     # the swap moved the parameters


def _pair(seed=2):
    from common import TINY
    from parity_util import build_pair
    _, m = build_pair(dict(TINY), device=DEV, targets=TARGETS, seed=seed)
    return m


def test_trainer_learns_saves_x_in_the_documented_layout_and_resumes_bit_identically(tmp_path):
    from parity_util import tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    a = _pair()
    sa = QwenLoraTrainStep(a, lr=1e-3, optimizer="adamw_schedulefree", optimizer_args={"warmup_steps": 2})
    assert sa.weight_decay == 0.0 and sa.betas == (0.9, 0.999)
    e, nz, u = tiny_embeddings(seed=5)
    losses = [sa.train_step(e, noise=nz, u=u).item() for _ in range(12)]
    print(f"adamw_schedulefree: losses {losses}")
    assert losses[-1] < losses[0], losses
    y = a.lora_store.pflat.detach().cpu().clone()
    z = sa.opt_state.z.detach().cpu().clone()
    ck = str(tmp_path / "ck")
    sa.save_checkpoint(ck)
    assert sa.train_mode is True
    # optimizer.bin: the package's layout, written in train mode
    sd = torch.load(os.path.join(ck, "optimizer.bin"), map_location="cpu", weights_only=False)
    for i, (_, p, off, k) in enumerate(a.lora_store.entries):
        s = sd["state"][i]
        assert set(s) == R.PARAM_KEYS and all(s[n].dtype == torch.float32 and s[n].shape == p.shape for n in s)
        assert torch.equal(s["z"].reshape(-1), z[off:off + k])
    g0 = sd["param_groups"][0]
    assert set(g0) == R.GROUP_KEYS | {"params"} and sd["global_step"] == 12
    assert (g0["k"], g0["train_mode"], g0["warmup_steps"], g0["lr"], tuple(g0["betas"])) == (12, True, 2, 1e-3, (0.9, 0.999))
    assert g0["lr_max"] == 1e-3 and g0["scheduled_lr"] == 1e-3 and g0["weight_sum"] > 0
    # the weights file holds x = lerp(y, z, 1 - 1 / beta1), not y
    b = _pair()
    b.load_lora_adapter(ck, adapter_name="lora_edit")
    x_file = b.lora_store.pflat.detach().cpu().clone()
    w = 1 - 1 / 0.9
    R.check("x", x_file, R.lerp(y, z, w), R.lerp(y.double(), z.double(), w), "saved safetensors")
    assert not torch.equal(x_file, y) and (x_file - y).abs().max() > 10 * R.tolerance(R.lerp(y, z, w), R.lerp(y.double(), z.double(), w))[0]
    # the run that wrote the folder goes on; the run resumed from it equals it bit for bit
    for _ in range(3):
        sa.train_step(e, noise=nz, u=u)
    want = a.lora_store.pflat.detach().cpu().clone()
    sb = QwenLoraTrainStep(b, lr=0.5, betas=(0.5, 0.5), optimizer="adamw_schedulefree")
    sb.load_checkpoint(ck, adapter_name="lora_edit")
    assert sb.global_step == 12 and sb.lr == 1e-3 and sb.betas == (0.9, 0.999) and sb.train_mode is True
    assert sb.optimizer_args["warmup_steps"] == 2 and sb.opt_state.k == 12
    for _ in range(3):
        sb.train_step(e, noise=nz, u=u)
    assert torch.equal(b.lora_store.pflat.detach().cpu(), want)


def test_mode_handling_and_sampling_from_x():
    from parity_util import tiny_embeddings
    from qflux_amd.sampling import QwenSampler
    from qflux_amd.trainer import QwenLoraTrainStep
    m = _pair()
    step = QwenLoraTrainStep(m, lr=5e-3, optimizer="adamw_schedulefree")
    e, nz, u = tiny_embeddings(seed=5)
    for _ in range(4):
        step.train_step(e, noise=nz, u=u)
    y = m.lora_store.pflat.detach().clone()
    with step.eval_mode():
        assert step.train_mode is False and not torch.equal(m.lora_store.pflat, y)
        with pytest.raises(RuntimeError, match=r"train\(\) first"):
            step.optimizer_step()
        with pytest.raises(RuntimeError, match=r"train\(\) first"):
            step.train_step(e, noise=nz, u=u)
    assert step.train_mode is True and step.global_step == 4 and step.opt_state.k == 4
    back = m.lora_store.pflat.detach().clone()
    bound, _ = R.tolerance(y.cpu(), y.double().cpu())                    # one fp32 ulp of the largest magnitude: the round trip rounds
    assert (back - y).abs().max().item() <= 4 * bound
    step.zero_grad()
    loss = step.train_step(e, noise=nz, u=u)                             # training continues
    assert torch.isfinite(loss).all() and step.global_step == 5 and not torch.equal(m.lora_store.pflat, back)
    # sampling from x differs from sampling from y: the swap reaches the launch programs
    emb = dict(e, latents=nz.clone(), num_inference_steps=2, true_cfg_scale=1.0)
    before = m.lora_store.pflat.detach().clone()
    from_y = QwenSampler(m).sample(emb)
    from_x = QwenSampler(m).sample(emb, train_step=step)
    assert torch.isfinite(from_x.float()).all() and from_x.shape == from_y.shape and not torch.equal(from_x, from_y)
    assert torch.equal(QwenSampler(m).sample(emb), from_y) and step.train_mode is True
    assert (m.lora_store.pflat - before).abs().max().item() <= 4 * bound
    # every other family: the argument changes nothing
    other = QwenLoraTrainStep(m, lr=1e-3)
    assert torch.equal(QwenSampler(m).sample(emb, train_step=other), QwenSampler(m).sample(emb))


def test_flux_step_runs_with_the_family():
    from common import FLUX_TINY
    from oracle import flux_dit as FO
    from qflux_amd.models import FluxTransformer2DModel
    from qflux_amd.modules import LoraConfig
    from qflux_amd.trainer import FluxKontextTrainStep
    cfg = dict(FLUX_TINY, joint_attention_dim=64, guidance_embeds=True)
    with torch.device(DEV):
        m = FluxTransformer2DModel(**cfg)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_((torch.randn(p.shape, generator=g) * (0.5 / p.shape[-1] ** 0.5 if p.ndim == 2 else 0.05) + (1.0 if "norm_" in n and p.ndim == 1 else 0.0)).to(p.dtype))
    m.add_adapter(LoraConfig(r=4, lora_alpha=8), "a", generator=g)
    step = FluxKontextTrainStep(m, lr=1e-3, optimizer="adamw_schedulefree", optimizer_args={"warmup_steps": 1})
    ctl = FO.prepare_latent_image_ids(4, 6); ctl[:, 0] = 1
    emb = dict(image_latents=torch.randn(2, 24, 64, generator=g).half(), control_latents=torch.randn(2, 24, 64, generator=g).half(),
               control_ids=ctl, text_ids=torch.zeros(7, 3), latent_hw=(4, 6),
               pooled_prompt_embeds=torch.randn(2, 16, generator=g).half(), prompt_embeds=torch.randn(2, 7, 64, generator=g).half())
    for it in range(2):
        before = m.lora_store.pflat.detach().clone()
        loss = step.train_step(emb, noise=torch.randn(2, 24, 64, generator=g), t=torch.tensor([0.3, 0.8]))
        assert torch.isfinite(loss).all() and not torch.equal(before, m.lora_store.pflat) and torch.isfinite(m.lora_store.pflat).all()
    sd = step.state_dict()
    assert sd["param_groups"][0]["k"] == 2 and set(sd["state"][0]) == R.PARAM_KEYS and step.betas == (0.9, 0.999)
    y = m.lora_store.pflat.detach().clone()
    with step.eval_mode():
        assert not torch.equal(m.lora_store.pflat, y)


def test_class_steps_bit_identically_to_the_train_step_and_exchanges_checkpoints():
    from common import TINY
    from parity_util import build_pair
    from qflux_amd import optim as O
    from qflux_amd.trainer import QwenLoraTrainStep
    a, b = (build_pair(dict(TINY), device=DEV, targets=TARGETS, seed=2)[1] for _ in range(2))
    sa, sb = a.lora_store, b.lora_store
    start = sa.pflat.detach().clone()
    assert torch.equal(start, sb.pflat)
    kw = dict(lr=1e-3, weight_decay=0.01, warmup_steps=2, r=0.5)
    args = {"warmup_steps": 2, "r": 0.5}
    params = [p for n, p in a.named_parameters() if "lora_" in n]
    opt = O.AdamWScheduleFree(params, **kw)
    opt.train()
    step = QwenLoraTrainStep(b, lr=kw["lr"], weight_decay=kw["weight_decay"], max_grad_norm=0, optimizer="adamw_schedulefree", optimizer_args=args)

    def grad(it):
        g = (torch.randn(sa.gflat.shape, generator=torch.Generator().manual_seed(50 + it)) * 1e-2).to(DEV)
        for m in (a, b):
            m.lora_store.gflat.copy_(g)
    for it in range(3):
        grad(it)
        opt.step()
        step.optimizer_step()
        opt.zero_grad()                       # set_to_none: the next step() re-attaches the flat views
        step.zero_grad()
    assert not torch.equal(sa.pflat, start) and torch.equal(sa.pflat, sb.pflat)
    x, y = opt._opt_state.buffers(), step.opt_state.buffers()
    assert [n for n, _ in x] == [n for n, _ in y] == ["z", "v", "sched"] and all(torch.equal(s, t) for (_, s), (_, t) in zip(x, y))
    # the class's file resumes a fresh train step, which then steps like the class that never stopped
    sd = opt.state_dict()
    assert sd["global_step"] == 3 and sd["param_groups"][0]["k"] == 3 and list(sd["state"]) == list(step.state_dict()["state"])
    step2 = QwenLoraTrainStep(b, lr=0.5, max_grad_norm=0, optimizer="adamw_schedulefree")
    step2.load_state_dict(sd)
    assert step2.lr == kw["lr"] and step2.global_step == 3 and step2.optimizer_args == dict(warmup_steps=2, r=0.5, weight_lr_power=2.0)
    grad(3)
    opt.step()
    step2.optimizer_step()
    assert torch.equal(sa.pflat, sb.pflat)
    # and the other way: the train step's file resumes a fresh class
    opt2 = O.AdamWScheduleFree(params, lr=0.5)
    opt2.load_state_dict(step2.state_dict())
    assert opt2.param_groups[0]["lr"] == kw["lr"] and opt2.param_groups[0]["warmup_steps"] == 2 and opt2._opt_state.k == 4
    grad(4)
    opt2.step()
    step2.optimizer_step()
    assert torch.equal(sa.pflat, sb.pflat)
    # both do the same eval round trip: still the same bits, and both refuse to step in between
    opt2.eval(); step2.eval()
    assert torch.equal(sa.pflat, sb.pflat)
    with pytest.raises(RuntimeError, match=r"train\(\) first"):
        opt2.step()
    opt2.train(); step2.train()
    assert torch.equal(sa.pflat, sb.pflat)
