"""GPU: qfx_scaled_adamw_step (Riemannian-preconditioned AdamW for LoRA pairs) through the C ABI against tests/scaled_adamw_ref.py and
against qfx_adamw_step, and the family through both train steps, the torch.optim class, checkpoints and a captured graph.  The pairs
of scaled_adamw_ref.SHAPES are packed in one flat buffer with odd gaps, so that some tensors take the 16-byte path and most the
scalar one; every kernel test runs three steps."""
import math

import numpy as np
import pytest
import torch

import optim_ref as OR
import scaled_adamw_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
HP = R.hyper()
# The bar of every comparison with the restatement, in fp32 ulps of each quantity's scale: twice the restatement's own order noise
# (forward against reversed fp64 sums on these very inputs, three steps), measured by
# tests/test_scaled_adamw_cpu.py::test_bar_is_twice_the_references_own_order_noise: p 0.0, m 0.0, v 0.0 -- no element of g^ rounds
# the other way -- so the bar is 0: the restatement's bits.
ORDER_NOISE_BAR = {"p": 2 * 0.0, "m": 2 * 0.0, "v": 2 * 0.0}
assert ORDER_NOISE_BAR == R.BARS


def _ops():
    from qflux_amd import ops
    return ops


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def kernel_run(st, grads, pairs, hp=HP, clip=None, reg=R.REG, precondition=True, n_elems=None):
    """Three launches from a copy of st; clip: None or (gnorm_sq, max_norm, grad_scale).  Returns ({p, m, v} numpy, [skipped per step])."""
    ops = _ops()
    p, m, v = dev(st["p"]), dev(st["m"]), dev(st["v"])
    lay = ops.scaled_adamw_table(pairs, device=DEV, n_elems=p.numel() if n_elems is None else n_elems)
    skipped = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    gn = None if clip is None or clip[0] is None else torch.tensor(clip[0], dtype=torch.float32, device=DEV)
    out = []
    for t, g in enumerate(grads, 1):
        ops.scaled_adamw_step(p, dev(g), m, v, lay, skipped, hp["lr"], hp["b1"], hp["b2"], hp["eps"], t, reg=reg, precondition=precondition,
                              gnorm_sq=gn, max_norm=0.0 if clip is None else clip[1], grad_scale=1.0 if clip is None else clip[2])
        out.append(int(skipped.item()))
    return dict(p=p.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy()), out


def adamw_run(st, grads, hp, clip, wd=None):
    ops = _ops()
    p, m, v = dev(st["p"]), dev(st["m"]), dev(st["v"])
    gn = None if clip is None or clip[0] is None else torch.tensor(clip[0], dtype=torch.float32, device=DEV)
    for t, g in enumerate(grads, 1):
        ops.adamw_step(p, dev(g), m, v, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"] if wd is None else wd, t, gnorm_sq=gn,
                       max_norm=0.0 if clip is None else clip[1], grad_scale=1.0 if clip is None else clip[2])
    return dict(p=p.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy())


def same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def within_bar(got, ref, scales, pairs, what):
    for q in R.QUANTITIES:
        d = R.distance(got[q], ref[q], scales[q], pairs)
        print(f"SCALED_ADAMW {what} {q}: {d:.3f} ulps of scale (bar {ORDER_NOISE_BAR[q]})")
    for q in R.QUANTITIES:
        assert R.distance(got[q], ref[q], scales[q], pairs) <= ORDER_NOISE_BAR[q], (what, q)
        assert np.isfinite(got[q]).all()


def gaps_untouched(got, st, pairs):
    mask = R.covered(pairs, len(st["p"]))
    return all(same_bits(got[q][~mask], st[q][~mask]) for q in R.QUANTITIES) and not mask.all()


@pytest.fixture(scope="module")
def gauss():
    pairs, n = R.pack(R.SHAPES)
    st, grads = R.gaussian_state(pairs, n)
    ref, scales, skipped = R.run(st, grads, pairs, HP, want_scales=True)
    assert skipped == 0
    return pairs, n, st, grads, ref, scales


# ---------------------------------------------------------------- 1. precondition = 0 is qfx_adamw_step
@pytest.mark.parametrize("clipname", ["null_norm", "clip_gs1", "clip_gs_half", "clip_gs_third"])
def test_without_the_preconditioner_the_launch_is_qfx_adamw_step_bit_for_bit(gauss, clipname):
    pairs, n, st, grads, _, _ = gauss
    clip = OR.clip_args(clipname, grads[0])[:3]
    got, skipped = kernel_run(st, grads, pairs, clip=clip, precondition=False)
    want = adamw_run(st, grads, HP, clip)
    mask = R.covered(pairs, n)
    assert skipped == [0, 0, 0] and gaps_untouched(got, st, pairs)
    for q in R.QUANTITIES:
        assert same_bits(got[q][mask], want[q][mask]), q
    assert not same_bits(got["p"][mask], st["p"][mask])


# ---------------------------------------------------------------- 2. the listing
def test_gaussian_pairs_match_the_restatement_within_its_own_order_noise(gauss):
    pairs, n, st, grads, ref, scales = gauss
    got, skipped = kernel_run(st, grads, pairs)
    assert skipped == [0, 0, 0] and gaps_untouched(got, st, pairs)
    within_bar(got, ref, scales, pairs, "gaussian")
    plain = adamw_run(st, grads, HP, None)
    mask = R.covered(pairs, n)
    assert not same_bits(got["p"][mask], plain["p"][mask])         # the preconditioner does something


def test_clipped_gradient_is_scaled_before_the_preconditioner(gauss):
    pairs, n, st, grads, _, _ = gauss
    gsq, mx, gs, exact = OR.clip_args("clip_gs_half", grads[0])
    assert exact
    c = float(OR.clip_f32(gsq, mx, gs))
    got, _ = kernel_run(st, grads, pairs, clip=(gsq, mx, gs))
    ref, scales, _ = R.run(st, grads, pairs, HP, clip=c, want_scales=True)
    within_bar(got, ref, scales, pairs, "clipped")


# ---------------------------------------------------------------- 3. a fresh LoRA
def test_fresh_lora_decays_a_exactly_and_steps_b():
    pairs, n = R.pack(R.SHAPES)
    st, grads = R.fresh_lora_state(pairs, n)
    got, skipped = kernel_run(st, grads, pairs)
    ref, scales, _ = R.run(st, grads, pairs, HP, want_scales=True)
    decay = OR.fma32(-F32(HP["lr"]), F32(HP["wd"]), F32(1.0))
    assert skipped == [0, 0, 0]
    for off_a, off_b, r, nin, nout, *_ in pairs:
        a = st["p"][off_a:off_a + r * nin]
        for _ in range(R.STEPS):
            a = a * decay
        sa = slice(off_a, off_a + r * nin)
        assert same_bits(got["p"][sa], a) and not got["m"][sa].any() and not got["v"][sa].any()
        assert got["p"][off_b:off_b + nout * r].any()
    within_bar(got, ref, scales, pairs, "fresh")


# ---------------------------------------------------------------- 4. rank-deficient Gram matrix
def test_rank_deficient_gram_stays_finite_and_within_the_bar():
    pairs, n, st, grads = R.rank_deficient_state()
    reg = R.RANK_DEFICIENT["reg"]
    got, skipped = kernel_run(st, grads, pairs, reg=reg)
    ref, scales, rs = R.run(st, grads, pairs, HP, reg=reg, want_scales=True)
    assert skipped == [0, 0, 0] and rs == 0
    within_bar(got, ref, scales, pairs, "rank-deficient")


# ---------------------------------------------------------------- 5. the skip rule
def test_a_nan_gradient_leaves_its_pair_and_only_its_pair(gauss):
    pairs, n, st, grads, _, _ = gauss
    bad = [g.copy() for g in grads]
    victim = pairs[2]
    for g in bad:
        g[victim[0] + 17] = np.nan
    got, skipped = kernel_run(st, bad, pairs)
    others = [p for p in pairs if p is not victim]
    want, _ = kernel_run(st, bad, others, n_elems=n)
    assert skipped == [1, 1, 1]
    vm, om = R.covered([victim], n), R.covered(others, n)
    for q in R.QUANTITIES:
        assert same_bits(got[q][vm], st[q][vm]), q
        assert same_bits(got[q][om], want[q][om]), q
    assert not same_bits(got["p"][om], st["p"][om])
    # the B half counts too, and so does the plain mode
    bad = [g.copy() for g in grads]
    bad[1][pairs[0][1] + 1] = np.inf
    got, skipped = kernel_run(st, bad, pairs, precondition=False)
    assert skipped == [0, 1, 0]


# ---------------------------------------------------------------- 6. same inputs, same bits
def test_two_launches_from_the_same_state_give_the_same_bits(gauss):
    pairs, n, st, grads, _, _ = gauss
    a, _ = kernel_run(st, grads, pairs)
    b, _ = kernel_run(st, grads, pairs)
    assert all(same_bits(a[q], b[q]) for q in R.QUANTITIES)


# ---------------------------------------------------------------- 7. per-tensor fields
def test_per_tensor_lr_ratio_and_weight_decay_equal_two_scalar_launches(gauss):
    _, n, st, grads, _, _ = gauss
    mixed, _ = R.pack(R.SHAPES, ratios=(1.0, 4.0), wds=(HP["wd"], 0.0))
    base, _ = R.pack(R.SHAPES)
    hp_b = dict(HP, lr=4 * HP["lr"])
    # the Gram matrices come from the weights of BOTH tensors: after step 1 the runs differ in the partner, so compare step 1
    one = [grads[0]]
    got, _ = kernel_run(st, one, mixed)
    as_a, _ = kernel_run(st, one, base)                                                # every tensor with lora_A's fields
    as_b, _ = kernel_run(st, one, R.pack(R.SHAPES, wds=(0.0, 0.0))[0], hp=hp_b)        # every tensor with lora_B's, as scalars
    for off_a, off_b, r, nin, nout, *_ in mixed:
        sa, sb = slice(off_a, off_a + r * nin), slice(off_b, off_b + nout * r)
        for q in R.QUANTITIES:
            assert same_bits(got[q][sa], as_a[q][sa]) and same_bits(got[q][sb], as_b[q][sb]), q
        assert not same_bits(got["p"][sb], as_a["p"][sb])
    # three steps against the restatement with the same fields
    got, _ = kernel_run(st, grads, mixed)
    ref, scales, _ = R.run(st, grads, mixed, HP, want_scales=True)
    within_bar(got, ref, scales, mixed, "per-tensor")


def test_refusals_of_the_wrapper():
    ops = _ops()
    pairs, n = R.pack(R.SHAPES[:1])
    lay = ops.scaled_adamw_table(pairs, device=DEV)
    z = torch.zeros(n, device=DEV)
    sk = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="reg"):
        ops.scaled_adamw_step(z, z, z, z, lay, sk, 1e-3, 0.9, 0.999, 1e-8, 1, reg=0.0)
    with pytest.raises(ValueError, match="elements"):
        ops.scaled_adamw_step(z[:10].contiguous(), z, z, z, lay, sk, 1e-3, 0.9, 0.999, 1e-8, 1)
    with pytest.raises(ValueError, match="skipped"):
        ops.scaled_adamw_step(z, z, z, z, lay, None, 1e-3, 0.9, 0.999, 1e-8, 1)


# ---------------------------------------------------------------- through the train steps
_TWINS = {}


def _twins():
    from common import TINY
    from parity_util import build_pair
    if not _TWINS:
        _TWINS["models"] = [build_pair(dict(TINY), device=DEV, seed=2)[1] for _ in range(2)]
        _TWINS["start"] = _TWINS["models"][0].lora_store.pflat.detach().clone()
    for m in _TWINS["models"]:
        with torch.no_grad():
            m.lora_store.pflat.copy_(_TWINS["start"])
            m.lora_store.gflat.zero_()
    return _TWINS["models"]


def _start_b(model, seed=9):
    """A fresh adapter has B = 0; give every lora_B values so that both preconditioners are at work from the first step."""
    g = torch.Generator().manual_seed(seed)
    st = model.lora_store
    with torch.no_grad():
        for name, p, off, k in st.entries:
            if ".lora_B." in name:
                st.pflat[off:off + k].copy_((torch.randn(k, generator=g) * 0.05).to(DEV))


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
    return m


def _flux_batch():
    from oracle import flux_dit as FO
    g = torch.Generator().manual_seed(4)
    ctl = FO.prepare_latent_image_ids(4, 6); ctl[:, 0] = 1
    emb = dict(image_latents=torch.randn(2, 24, 64, generator=g).half(), control_latents=torch.randn(2, 24, 64, generator=g).half(),
               control_ids=ctl, text_ids=torch.zeros(7, 3), latent_hw=(4, 6),
               pooled_prompt_embeds=torch.randn(2, 16, generator=g).half(), prompt_embeds=torch.randn(2, 7, 64, generator=g).half())
    return emb, torch.randn(2, 24, 64, generator=g), torch.tensor([0.3, 0.8])


def _stock_loop_equals_the_fused_step(a, b, step, passes):
    """Model a: the fused train step.  Model b: the stock loop's optimizer, qflux_amd.optim.ScaledAdamW over the LoRA+ groups, fed
    the gradient the fused step took (the stock loop has clipped before step(): the fused step runs without clipping here)."""
    from qflux_amd import optim as O
    sa, sb = a.lora_store, b.lora_store
    with torch.no_grad():
        sb.pflat.copy_(sa.pflat)
    start = sa.pflat.detach().clone()
    opt = O.ScaledAdamW(O.loraplus_param_groups(b, step.lr, 4.0, weight_decay=step.weight_decay), weight_decay=step.weight_decay)
    for run in passes:
        run()
        b.lora_store.gflat.copy_(sa.gflat)
        step.optimizer_step()
        opt.step()
        step.zero_grad()
        opt.zero_grad()
    assert torch.equal(sa.pflat, sb.pflat) and not torch.equal(sa.pflat, start)
    assert torch.equal(step.opt_state.m, opt._opt_state.m) and torch.equal(step.opt_state.v, opt._opt_state.v)
    assert int(step.opt_state.skipped.item()) == 0 and int(opt.skipped.item()) == 0
    assert [len(g["params"]) for g in opt.state_dict()["param_groups"]] == [len(g["params"]) for g in step.state_dict()["param_groups"]]
    return start


def test_qwen_train_step_with_loraplus_equals_the_stock_loop_bit_for_bit():
    from parity_util import tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    a, b = _twins()
    _start_b(a)
    step = QwenLoraTrainStep(a, lr=1e-3, max_grad_norm=0, optimizer="scaled_adamw", loraplus_lr_ratio=4)
    pool = [tiny_embeddings(seed=600 + i) for i in range(3)]
    start = _stock_loop_equals_the_fused_step(a, b, step, [lambda e=e, nz=nz, u=u: step.forward_backward(e, noise=nz, u=u) for e, nz, u in pool])
    assert step.global_step == 3
    # lora_B moved at four times lora_A's rate: Adam's first step is lr in every element with a gradient
    st = a.lora_store
    for name, p, off, k in st.entries:
        d = (st.pflat[off:off + k] - start[off:off + k]).abs().max().item()
        assert d > 0, name


def test_flux_train_step_with_loraplus_equals_the_stock_loop_bit_for_bit():
    from qflux_amd.trainer import FluxKontextTrainStep
    a, b = _flux_model(), _flux_model()
    _start_b(a)
    step = FluxKontextTrainStep(a, lr=1e-3, max_grad_norm=0, optimizer="scaled_adamw", loraplus_lr_ratio=4)
    emb, noise, t = _flux_batch()
    _stock_loop_equals_the_fused_step(a, b, step, [lambda: step.forward_backward(emb, noise=noise, t=t)])


def test_checkpoint_after_step_two_resumes_step_three_bit_for_bit(tmp_path):
    from parity_util import tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    a, a2 = _twins()
    _start_b(a)
    pool = [tiny_embeddings(seed=620 + i) for i in range(3)]
    args = dict(reg=1e-5, precondition=True)
    run = QwenLoraTrainStep(a, lr=2e-3, max_grad_norm=1.0, optimizer="scaled_adamw", optimizer_args=dict(args), loraplus_lr_ratio=4)
    for it, (emb, noise, u) in enumerate(pool):
        run.train_step(emb, noise=noise, u=u)
        if it == 1:
            run.save_checkpoint(str(tmp_path / "ck"))
            mid = a.lora_store.pflat.detach().clone()
    want = a.lora_store.pflat.detach().clone()
    with torch.no_grad():
        a2.lora_store.pflat.copy_(mid)
    resumed = QwenLoraTrainStep(a2, lr=123.0, max_grad_norm=1.0, optimizer="scaled_adamw", loraplus_lr_ratio=4)
    resumed.load_checkpoint(str(tmp_path / "ck"))
    assert resumed.global_step == 2 and resumed.optimizer_args == args
    assert [g["lr"] for g in resumed.state_dict()["param_groups"]] == [2e-3, 8e-3]      # the groups' rates are the file's
    emb, noise, u = pool[-1]
    resumed.train_step(emb, noise=noise, u=u)
    assert torch.equal(a2.lora_store.pflat.detach(), want) and not torch.equal(want, mid)
    for (n, x), (_, y) in zip(run.opt_state.buffers(), resumed.opt_state.buffers()):
        assert torch.equal(x, y), n
    sd = resumed.state_dict()
    assert {frozenset(e) for e in sd["state"].values()} == {frozenset({"step", "exp_avg", "exp_avg_sq"})}
    assert [g["reg"] for g in sd["param_groups"]] == [1e-5, 1e-5] and math.isclose(sd["param_groups"][1]["lr"] / sd["param_groups"][0]["lr"], 4.0)


def test_ema_max_norm_and_adapter_stats_ride_along():
    """The three options read only the flat buffers: one accumulated step with all of them beside the family."""
    from parity_util import tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    a, _ = _twins()
    _start_b(a)
    before = a.lora_store.pflat.detach().clone()
    step = QwenLoraTrainStep(a, lr=1e-3, optimizer="scaled_adamw", ema_decay=0.9, max_weight_norm=1e-3, adapter_stats_every=1)
    (e, nz, u), (e2, _, _) = tiny_embeddings(seed=640), tiny_embeddings(seed=641)
    loss = step.train_step(e, noise=nz, u=u, micro_batches=[e2])
    st = a.lora_store
    assert torch.isfinite(loss) and torch.isfinite(st.pflat).all() and not torch.equal(st.pflat, before)
    assert step.weight_norm_stats()[0] > 0 and not torch.equal(step.ema.shadows[0], before)
    stats = step.last_adapter_stats
    assert stats and all(v["grad_nonfinite"] == 0 for v in stats.values()) and int(step.opt_state.skipped.item()) == 0


def test_captured_graph_replay_equals_the_eager_step():
    from parity_util import tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    a, b = _twins()
    _start_b(a)
    with torch.no_grad():
        b.lora_store.pflat.copy_(a.lora_store.pflat)
    kw = dict(lr=1e-3, optimizer="scaled_adamw", loraplus_lr_ratio=4)
    sa, sb = QwenLoraTrainStep(a, **kw), QwenLoraTrainStep(b, **kw)
    batches = [tiny_embeddings(seed=s) for s in (11, 12, 13)]
    gstep = sb.capture_graph(batches[0][0])
    assert sb.global_step == 0
    for e, nz, u in batches:
        la = sa.train_step(e, noise=nz, u=u).item()
        lb = gstep(e, noise=nz, u=u).item()
        assert abs(la - lb) <= 1e-6 * abs(la), (la, lb)      # the loss sum is an fp32 atomic reduction (tests/test_model_gpu.py)
    # the bar of tests/test_model_gpu.py for the attention-only adapter set (the backward's fp32 atomics move the gradient by 1e-6;
    # nothing of the optimizer's differs between the two): taken over at a tenth of that test's learning rate, which leaves a
    # factor of ten for what the preconditioner adds (the condition numbers of these rank-4 Gram matrices are of order one)
    rel = ((a.lora_store.pflat - b.lora_store.pflat).abs().max() / a.lora_store.pflat.abs().max()).item()
    assert rel < 1e-6 and sb.global_step == 3, rel
