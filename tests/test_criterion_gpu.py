"""GPU: the general criterion kernel (qfx_criterion_fwd_bwd) against tests/criterion_ref.py, and the train steps' objective options
(timestep densities, loss weighting, Huber forms, per-sample losses, the captured graph) on the tiny models of parity_util.

Bounds.  The gradient is a handful of correctly rounded fp32 operations (the library is built with hipcc's default correctly rounded
fp32 divide and square root, without FMA contraction), so L2 equals the fp32 restatement bit for bit; the Huber forms are held to
"equal or adjacent in bf16" to the fp64 restatement: the fp32 arithmetic error of a few 2^-24 is far below half a bf16 ulp (2^-9).
The loss sums S_t * C non-negative terms: relative S_t * C * 2^-24 to the fp64 value holds for any summation order."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import criterion_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16

# (B, S_all, S_t, C, misaligned pred view)
SHAPES = {
    "one_vector": (1, 1, 1, 8, False),
    "rows_past_S_t": (2, 70, 37, 64, False),
    "odd_rows_many_chunks": (3, 257, 257, 64, False),
    "scalar_C12": (2, 19, 5, 12, False),
    "C1": (1, 5, 5, 1, False),
    "misaligned_pred": (2, 70, 37, 64, True),
    "headline_tokens": (2, 4352, 4096, 64, False),      # 272 (sample, chunk) items on at most 256 workgroups: the stride loop runs
}
CANARY = 12345.678


@functools.lru_cache(maxsize=None)
def _case(shape, kind, weighted):
    """Inputs (CPU) and the two restatements of one case, computed once and left unchanged."""
    B, S_all, S_t, Cc, _ = SHAPES[shape]
    g = torch.Generator().manual_seed(1000 + 7 * sorted(SHAPES).index(shape) + R.KINDS.index(kind))
    pred = torch.randn(B, S_all, Cc, generator=g).to(BF)
    target = torch.randn(B, S_t, Cc, generator=g).to(BF)
    sw = tw = hc = None
    if weighted:
        sw = torch.rand(B, generator=g) * 2.5 + 0.5
        tw = torch.rand(B, S_t, generator=g) * 2.0
        tw[torch.rand(B, S_t, generator=g) < 0.25] = 0.0
        tw[0, 0] = 1.5
    if kind != "l2":
        hc = 10.0 ** (torch.rand(B, generator=g) * 3.0 - 2.0)      # 0.01 .. 10: |d| both far above and far below c
    inv_denom = 1.0 / (float(tw.sum()) + 1e-12) if weighted else 1.0 / (B * S_t)
    gscale = 0.37 if weighted else 1.0
    kw = dict(sample_w=sw, token_w=tw, huber_c=hc, kind=kind, inv_denom=inv_denom, gscale=gscale)
    return dict(pred=pred, target=target, kw=kw, d32=R.dpred_f32(pred, target, S_t, **kw), f64=R.criterion_f64(pred, target, S_t, **kw))


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _launch(shape, case):
    """One raw launch with canaries around loss_per_sample, the loss and the workspace: (loss, lps, dpred, guards intact)."""
    from qflux_amd import _lib as L
    from qflux_amd import ops
    B, S_all, S_t, Cc, misaligned = SHAPES[shape]
    kw = case["kw"]
    if misaligned:      # pred starts one bf16 element past a 16-byte boundary: the kernel must take its scalar path
        buf = torch.empty(B * S_all * Cc + 8, dtype=BF, device=DEV)
        pred = buf[1:1 + B * S_all * Cc].view(B, S_all, Cc)
        pred.copy_(case["pred"])
        assert pred.data_ptr() % 16 == 2
    else:
        pred = _dev(case["pred"])
    target, sw, tw, hc = _dev(case["target"]), _dev(kw["sample_w"]), _dev(kw["token_w"]), _dev(kw["huber_c"])
    nws = L.lib.qfx_criterion_workspace_bytes(B, S_t, Cc) // 8
    out = torch.full((8 + B + 8 + 1 + 8,), CANARY, dtype=torch.float32, device=DEV)       # guard | lps | guard | loss | guard
    ws = torch.full((8 + nws + 8,), CANARY, dtype=torch.float64, device=DEV)
    dpred = torch.empty(B, S_all, Cc, dtype=BF, device=DEV)
    a = L.CriterionArgs()
    a.pred, a.target, a.sample_w, a.token_w, a.huber_c = pred.data_ptr(), target.data_ptr(), ops._p(sw), ops._p(tw), ops._p(hc)
    a.loss_per_sample, a.loss = out[8:].data_ptr(), out[8 + B + 8:].data_ptr()
    a.dpred, a.workspace, a.workspace_bytes = dpred.data_ptr(), ws[8:].data_ptr(), nws * 8
    a.B, a.S_all, a.S_t, a.C, a.kind, a.inv_denom, a.gscale = B, S_all, S_t, Cc, ops.LOSS_KINDS[kw["kind"]], kw["inv_denom"], kw["gscale"]
    L.check(L.lib.qfx_criterion_fwd_bwd(C.byref(a), ops.stream_ptr()), "qfx_criterion_fwd_bwd")
    torch.cuda.synchronize()
    out, ws = out.cpu(), ws.cpu()
    guards = torch.cat([out[:8], out[8 + B:8 + B + 8], out[8 + B + 9:]])
    intact = bool((guards == np.float32(CANARY)).all()) and bool((torch.cat([ws[:8], ws[8 + nws:]]) == CANARY).all())
    assert not bool((ws[8:8 + nws] == CANARY).any())      # every partial of the query's size is written
    return out[8 + B + 8].clone(), out[8:8 + B].clone(), dpred.cpu(), intact


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_against_the_restatements(shape, kind, weighted):
    B, S_all, S_t, Cc, _ = SHAPES[shape]
    case = _case(shape, kind, weighted)
    loss, lps, dpred, intact = _launch(shape, case)
    loss64, lps64, g64 = case["f64"]
    steps32, steps64 = R.bf16_steps(dpred, case["d32"]), R.bf16_steps(dpred, g64.to(BF))
    bound = S_t * Cc * 2.0 ** -24
    rel_loss = abs(float(loss) - float(loss64)) / abs(float(loss64))
    rel_lps = float(((lps.double() - lps64).abs() / lps64.abs().clamp_min(1e-300)).max())
    sw = case["kw"]["sample_w"]
    again = ((torch.ones(B) if sw is None else sw) * lps).sum() / torch.tensor(float(B))
    ulps = abs(float(loss) - float(again)) / float(np.spacing(np.float32(abs(float(again)))))
    print(f"CRITERION {shape} {kind} weighted={weighted}: dpred bf16 steps vs fp32 {steps32} vs fp64 {steps64}; loss rel {rel_loss:.3e} "
          f"per-sample rel {rel_lps:.3e} bound {bound:.3e}; loss vs fp32 mean of per-sample {ulps:.2f} ulp")
    assert intact, "a canary beside loss_per_sample, the loss or the workspace was overwritten"
    assert torch.isfinite(dpred.float()).all() and torch.isfinite(lps).all()
    if kind == "l2":
        assert R.same_bits(dpred, case["d32"])
    assert steps64 <= 1
    assert rel_loss <= bound and rel_lps <= bound
    assert ulps <= 2.0
    if S_all > S_t:
        assert bool((dpred[:, S_t:].view(torch.int16) == 0).all())
    loss2, lps2, dpred2, _ = _launch(shape, case)
    assert R.same_bits(loss, loss2) and R.same_bits(lps, lps2) and R.same_bits(dpred, dpred2)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_unit_weights_l2_agrees_with_the_mse_kernel(shape):
    """Unit weights and L2 through the wrapper against ops.mse_loss_fwd_bwd: the losses within the same bound of each other, dpred bit
    for bit at C = 64, where 1/C is a power of two and every other extra factor is exactly 1 (adjacent at most elsewhere: the older
    kernel rounds 1/(B S_t C) once, this one 1/C and 1/(B S_t))."""
    from qflux_amd import ops
    B, S_all, S_t, Cc, misaligned = SHAPES[shape]
    case = _case(shape, "l2", False)
    pred, target = _dev(case["pred"]), _dev(case["target"])
    loss_old, dpred_old = ops.mse_loss_fwd_bwd(pred, target, S_t)
    loss, lps, dpred = ops.criterion_fwd_bwd(pred, target, S_t)
    loss_nograd, _, none = ops.criterion_fwd_bwd(pred, target, S_t, want_grad=False)
    bound = S_t * Cc * 2.0 ** -24
    ref = float(case["f64"][0])
    print(f"CRITERION-vs-MSE {shape}: new {float(loss):.9g} old {float(loss_old):.9g} fp64 {ref:.12g}")
    assert abs(float(loss) - float(loss_old)) <= bound * abs(float(loss_old)) and abs(float(loss) - ref) <= bound * ref
    assert none is None and R.same_bits(loss, loss_nograd) and lps.shape == (B,)
    if Cc == 64:
        assert R.same_bits(dpred, dpred_old)
    else:
        assert R.bf16_steps(dpred, dpred_old) <= 1


# ---------------------------------------------------------------------------------------------------------------- the train steps
def _lora_grads(model):
    return {n: p.grad.detach().float().cpu().clone() for n, p in model.named_parameters() if "lora" in n}


def _fused_vs_autograd(step, model, emb, noise, key, val):
    """(fused loss, autograd loss, worst adapter-gradient difference relative to the tensor's maximum, per-sample losses)."""
    lf = step.forward_backward(emb, noise, **{key: val})
    per_sample = step.last_sample_losses
    gf = _lora_grads(model)
    step.zero_grad()
    la = step.compute_loss(emb, noise, **{key: val})
    la.backward()
    ga = _lora_grads(model)
    step.zero_grad()
    worst = max(((gf[n] - ga[n]).abs().max() / ga[n].abs().max()).item() for n in ga if ga[n].abs().max() > 0)
    assert sum(int(ga[n].abs().max() > 0) for n in ga) > 0
    return lf, la, worst, per_sample


@pytest.mark.parametrize("opts", [dict(weighting_scheme="cosmap", loss_type="l2"),
                                  dict(weighting_scheme="logit_normal", loss_type="huber", huber_c=0.1, huber_schedule="exponential")],
                         ids=["cosmap_l2", "logit_normal_huber_exponential"])
def test_qwen_step_fused_matches_its_autograd_objective(opts):
    """The bars of test_mask_edit_criterion_step_matches_oracle for the same comparison: loss 5e-3, worst adapter gradient 5e-2."""
    from common import TINY
    from parity_util import build_pair, tiny_embeddings
    from qflux_amd.schedules import huber_threshold, loss_weighting
    from qflux_amd.trainer import QwenLoraTrainStep
    _, hip = build_pair(dict(TINY), device=DEV)
    emb, noise, u = tiny_embeddings()
    step = QwenLoraTrainStep(hip, **opts)
    lf, la, worst, per_sample = _fused_vs_autograd(step, hip, emb, noise, "u", u)
    # the plain-MSE step on the same inputs: the options really change the objective
    plain = QwenLoraTrainStep(hip).forward_backward(emb, noise, u=u)
    step.zero_grad()
    print("criterion options", opts, "fused/autograd/plain", lf.item(), la.item(), plain.item(), "grad worst", worst)
    assert abs(lf.item() - la.item()) / abs(la.item()) < 5e-3 and worst < 5e-2
    if opts["loss_type"] == "huber":      # c = 0.1 ** (t / 1000) is 0.51 and 0.14 here, |d| is of order 1: far from d^2
        assert abs(lf.item() - plain.item()) / abs(plain.item()) > 5e-2
    else:
        assert not torch.equal(step._step_objective[0].cpu(), torch.ones(2))
    # last_sample_losses: [B] on the device, and the loss is its weighted mean
    ts, sig = step.sample_timesteps(2, u)
    sw = loss_weighting(step.weighting_scheme, sig)
    assert per_sample.shape == (2,) and per_sample.is_cuda and per_sample.dtype == torch.float32
    again = (sw * per_sample.cpu()).sum() / 2
    assert abs(float(again) - lf.item()) <= 2 * float(np.spacing(np.float32(lf.item())))
    if opts["loss_type"] == "huber":
        assert torch.equal(step._step_objective[1].cpu(), huber_threshold("exponential", 0.1, ts)) and step._step_objective[0] is None


def _flux_pair():
    from common import FLUX_TINY, fill_weights
    from oracle import flux_dit as FO
    from oracle import qwen_dit as O
    from qflux_amd.models import FluxTransformer2DModel
    from qflux_amd.modules import LoraConfig
    cfg = dict(FLUX_TINY)
    if cfg["joint_attention_dim"] % 64:
        cfg["joint_attention_dim"] = 64
    targets = ("to_k", "to_q", "to_v", "to_out.0")
    oracle = FO.OracleFluxDiT(**cfg)
    O.add_lora(oracle, r=4, lora_alpha=8, adapter_name="lora_edit", target_modules=targets)
    fill_weights(oracle, seed=5)
    for n, p in oracle.named_parameters():
        if "lora" not in n:
            p.data = p.data.to(BF)
    with torch.device(DEV):
        hip = FluxTransformer2DModel(**cfg)
    hip.add_adapter(LoraConfig(r=4, lora_alpha=8, target_modules=list(targets)), "lora_edit")
    hip.load_state_dict(oracle.state_dict(), strict=True)
    g = torch.Generator().manual_seed(31)
    h, w, T, B = 4, 6, 7, 2
    ctl_ids = FO.prepare_latent_image_ids(h, w)
    ctl_ids[:, 0] = 1
    emb = dict(image_latents=torch.randn(B, h * w, 64, generator=g).half(), control_latents=torch.randn(B, h * w, 64, generator=g).half(),
               control_ids=ctl_ids, text_ids=torch.zeros(T, 3), latent_hw=(h, w),
               pooled_prompt_embeds=torch.randn(B, cfg["pooled_projection_dim"], generator=g).half(),
               prompt_embeds=torch.randn(B, T, cfg["joint_attention_dim"], generator=g).half())
    noise = torch.randn(B, h * w, 64, generator=g).to(BF)
    return hip, emb, noise, torch.tensor([0.7109, 0.1611]).to(BF)


def test_flux_step_with_sigma_sqrt_weighting():
    from qflux_amd.schedules import loss_weighting
    from qflux_amd.trainer import FluxKontextTrainStep
    hip, emb, noise, t = _flux_pair()
    step = FluxKontextTrainStep(hip, weighting_scheme="sigma_sqrt")
    lf, la, worst, per_sample = _fused_vs_autograd(step, hip, emb, noise, "t", t)
    sw = loss_weighting("sigma_sqrt", t.float())
    print("flux sigma_sqrt fused/autograd", lf.item(), la.item(), "grad worst", worst, "weights", sw.tolist())
    assert abs(lf.item() - la.item()) / abs(la.item()) < 5e-3 and worst < 5e-2
    assert torch.equal(step._step_objective[0].cpu(), sw) and per_sample.shape == (2,)
    assert abs(float((sw * per_sample.cpu()).sum() / 2) - lf.item()) <= 2 * float(np.spacing(np.float32(lf.item())))
    # without an injected t the step draws through the density on the CPU generator and still runs
    torch.manual_seed(3)
    loss = step.forward_backward(emb, noise)
    step.zero_grad()
    assert torch.isfinite(loss) and step.last_sample_losses.shape == (2,)


def test_flux_multires_step_with_cosmap_and_smooth_l1():
    """The ragged batch of tests/test_flux_gpu.py through the general criterion: token weights (the padding mask), per-sample weights
    and thresholds from each sample's own t; fused against the step's autograd objective, same bars."""
    from qflux_amd.schedules import loss_weighting
    from qflux_amd.trainer import FluxKontextTrainStep
    from test_flux_gpu import _multires_case
    hip = _flux_pair()[0]
    samples, txt = _multires_case()
    step = FluxKontextTrainStep(hip, weighting_scheme="cosmap", loss_type="smooth_l1", huber_c=0.3)
    lf = step.forward_backward_multires(samples, txt)
    per_sample, sw = step.last_sample_losses, step._step_objective[0].cpu()
    gf = _lora_grads(hip)
    step.zero_grad()
    la = step.compute_loss_multires(samples, txt)
    la.backward()
    ga = _lora_grads(hip)
    step.zero_grad()
    worst = max(((gf[n] - ga[n]).abs().max() / ga[n].abs().max()).item() for n in ga if ga[n].abs().max() > 0)
    print("flux multires cosmap + smooth_l1 fused/autograd", lf.item(), la.item(), "grad worst", worst)
    assert abs(lf.item() - la.item()) / abs(la.item()) < 5e-3 and worst < 5e-2
    assert torch.equal(sw, loss_weighting("cosmap", torch.stack([s["t"] for s in samples]).float()))
    assert torch.equal(step._step_objective[1].cpu(), torch.full((3,), 0.3)) and per_sample.shape == (3,)


def test_captured_graph_with_cosmap_replays_the_eager_bits():
    """capture_graph stages sample_w in a static buffer: two replays with different u give the loss, per-sample-loss and (through the
    optimizer step they feed) gradient bits of two eager fused steps.  The eager model's flat buffers are first allocated AFTER the
    capture: a workspace the graph holds by address but the step does not keep alive would be handed to them and overwritten."""
    from common import TINY
    from parity_util import build_pair, tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    _, a = build_pair(dict(TINY), device=DEV)
    _, b = build_pair(dict(TINY), device=DEV)
    sa, sb = QwenLoraTrainStep(a, lr=1e-2, weighting_scheme="cosmap"), QwenLoraTrainStep(b, lr=1e-2, weighting_scheme="cosmap")
    emb, noise, u = tiny_embeddings()
    gstep = sb.capture_graph(emb)
    start = a.lora_store.pflat.clone()
    assert R.same_bits(start, b.lora_store.pflat)
    for k, uk in enumerate((u, torch.tensor([0.05, 0.977]))):
        la = sa.train_step(emb, noise=noise, u=uk)
        pa = sa.last_sample_losses.clone()
        lb = gstep(emb, noise=noise, u=uk)
        assert R.same_bits(la, lb), (k, la.item(), lb.item())
        assert R.same_bits(pa, sb.last_sample_losses) and sb.last_sample_losses.shape == (2,)
        assert R.same_bits(a.lora_store.pflat, b.lora_store.pflat), k
    assert not R.same_bits(start, a.lora_store.pflat)


def test_default_keywords_give_the_default_steps_bits():
    from common import TINY
    from parity_util import build_pair, tiny_embeddings
    from qflux_amd.trainer import QwenLoraTrainStep
    _, hip = build_pair(dict(TINY), device=DEV)
    emb, noise, u = tiny_embeddings(B=1)      # one sample: the MSE kernel's atomic loss sum is a single addend's, so reproducible
    spelled = dict(weighting_scheme="none", logit_mean=0.0, logit_std=1.0, mode_scale=1.29, timestep_shift=1.0, loss_type="l2",
                   huber_c=0.1, huber_schedule="constant")
    out = []
    for kw in ({}, spelled):
        step = QwenLoraTrainStep(hip, **kw)
        loss = step.forward_backward(emb, noise, u=u)
        assert step.last_sample_losses is None and step._step_objective is None
        out.append((loss.clone(), hip.lora_store.gflat.clone()))
        step.zero_grad()
    assert R.same_bits(out[0][0], out[1][0]) and R.same_bits(out[0][1], out[1][1]) and float(out[0][1].abs().max()) > 0
