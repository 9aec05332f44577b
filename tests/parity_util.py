"""Shared parity drivers (used by tests/ and __graft_entry__.smoke()): HIP path vs the CPU oracle."""
from __future__ import annotations

import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "qwen-image-finetune_amd"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

BF = torch.bfloat16
# Step-parity bars of the tiny-model drivers (HIP path vs the bf16 oracle): 2x the maxima observed over the whole -m gpu suite of
# round 4 (profiles/r04_parity_observed.json: Qwen, 23 runs: loss 1.8e-4, prediction 7.4e-3, worst gradient 1.44e-2 of the tensor
# maximum; FLUX, 18 runs: 2.7e-3, 1.13e-2, 3.75e-2), never looser than the round-3 bars (2e-2, 2e-2, 4e-2).  The FLUX gradient bar (4e-2) is
# where the tiny bf16 graph's OWN reduction-order noise sits (3.8e-2, profiles/r06_flux_bar_noise.json): run_flux_step_parity evaluates
# the oracle a second time on the GPU and lets a tensor exceed the bar only up to twice that self-noise on the same tensor.
QWEN_BARS = (4e-4, 1.5e-2, 3e-2)     # loss, prediction, gradient
FLUX_BARS = (6e-3, 2e-2, 4e-2)
LOSS_BAR, PRED_BAR, GRAD_BAR = FLUX_BARS      # (the looser set: for callers that do not say which model)


_OBSERVED = {}


def _observe(kind, res, dump=None):
    """Running maxima of what the step-parity drivers measured in this process (gpurun_out/parity_observed.json): the bars below are
    ratcheted to ~2x these.
    dump = (file name, table): only write that table as JSON into the same directory, created if absent (kernel tests that keep
    their own figures)."""
    import json
    d = os.path.join(ROOT, "gpurun_out")
    if dump is not None:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, dump[0]), "w") as f:
            json.dump(dump[1], f, indent=1)
        return
    path = os.path.join(d, "parity_observed.json")
    if not _OBSERVED and os.path.exists(path):      # several processes (pytest, smoke) add to one file
        try:
            _OBSERVED.update(json.load(open(path)))
        except Exception:  # noqa: BLE001
            pass
    o = _OBSERVED.setdefault(kind, dict(n=0, loss_rel=0.0, pred_rel=0.0, grad_rel_worst=0.0))
    o["n"] += 1
    for k in ("loss_rel", "pred_rel", "grad_rel_worst"):
        if k in res and res[k] is not None:
            o[k] = max(o[k], float(res[k]))
    if os.path.isdir(d):
        with open(path, "w") as f:
            json.dump(_OBSERVED, f, indent=1)


def relmax(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _grad_tol_factor(name: str) -> float:
    """LoRA-gradient bar: 4e-2 of the tensor's maximum (bf16 graph vs bf16 graph).  The adapters of the timestep / guidance /
    text EMBEDDERS sit behind the longest bf16 chain of the model -- d(temb) is the sum of every block's d(modulation) pushed back
    through its 6D x D matrix, each a bf16 tensor in the oracle's autograd and an fp32 column sum here -- and get 2x that bar."""
    return 2.0 if "time_text_embed" in name else 1.0


def build_pair(cfg, r=4, lora_alpha=8, adapter="lora_edit", seed=2, device="cuda:0", targets=("to_k", "to_q", "to_v", "to_out.0")):
    """Oracle (bf16 base weights, fp32 adapters: the reference's training dtype layout) and the HIP model
    loaded from the oracle's state dict (exercises the state-dict name compatibility)."""
    from common import fill_weights
    from oracle import qwen_dit as O
    from qflux_amd.models import QwenImageTransformer2DModel
    from qflux_amd.modules import LoraConfig

    oracle = O.OracleQwenDiT(**cfg)
    O.add_lora(oracle, r=r, lora_alpha=lora_alpha, adapter_name=adapter, target_modules=targets)
    fill_weights(oracle, seed=seed)
    for n, p in oracle.named_parameters():
        if "lora" not in n:
            p.data = p.data.to(BF)
    with torch.device(device):
        hip = QwenImageTransformer2DModel(**cfg)
    hip.add_adapter(LoraConfig(r=r, lora_alpha=lora_alpha, target_modules=(targets if isinstance(targets, str) else list(targets))), adapter)
    missing, unexpected = hip.load_state_dict(oracle.state_dict(), strict=True)
    assert not missing and not unexpected
    return oracle, hip


def tiny_embeddings(B=2, shapes=((1, 4, 6), (1, 4, 6)), T=5, Jd=512, seed=11):
    g = torch.Generator().manual_seed(seed)
    S_t = shapes[0][0] * shapes[0][1] * shapes[0][2]
    S_c = sum(f * h * w for f, h, w in shapes[1:])
    emb = dict(image_latents=torch.randn(B, S_t, 64, generator=g).half().float(),
               control_latents=torch.randn(B, S_c, 64, generator=g).half().float(),
               prompt_embeds=(torch.randn(B, T, Jd, generator=g) * 4).half().float(),
               prompt_embeds_mask=torch.ones(B, T, dtype=torch.int64),
               img_shapes=[[tuple(s) for s in shapes]] * B)
    noise = torch.randn(B, S_t, 64, generator=g)
    u = torch.tensor([0.7109, 0.1611, 0.5, 0.93][:B])
    return emb, noise, u


def run_tiny_step_parity(device="cuda:0", verbose=False, cfg=None, shapes=((1, 4, 6), (1, 4, 6)), T=5, B=2, r=4,
                         targets=("to_k", "to_q", "to_v", "to_out.0"), fused=True):
    from common import TINY
    from oracle import qwen_dit as O
    from qflux_amd.trainer import QwenLoraTrainStep

    cfg = dict(TINY if cfg is None else cfg)
    oracle, hip = build_pair(cfg, r=r, device=device, targets=targets)
    emb, noise, u = tiny_embeddings(B=B, shapes=shapes, T=T, Jd=cfg["joint_attention_dim"])
    loss_o, pred_o = O.qwen_compute_loss(oracle, emb, noise, u, BF, return_pred=True)
    loss_o.backward()
    step = QwenLoraTrainStep(hip)
    res = {}
    if fused:
        loss_h = step.forward_backward(emb, noise=noise, u=u)
        plan = list(hip._plans.values())[0]
        pred_h = plan.A["out"].view(B, -1, plan.A["out"].shape[-1])[:, : pred_o.shape[1]]
    else:
        loss_h = step.compute_loss(emb, noise=noise, u=u)
        loss_h.backward()
        pred_h = None
    torch.cuda.synchronize()
    res["loss_oracle"], res["loss_hip"] = loss_o.item(), loss_h.item()
    res["loss_rel"] = abs(loss_h.item() - loss_o.item()) / abs(loss_o.item())
    if pred_h is not None:
        res["pred_rel"] = relmax(pred_h, pred_o)
    og = {n: p.grad for n, p in oracle.named_parameters() if "lora" in n}
    worst = 0.0
    worst_name = None
    nz = 0
    dead = 0
    for n, p in hip.named_parameters():
        if "lora" in n:
            if og[n] is None:  # dead compute in the reference (last block's text tail): our grad must be exactly zero
                assert p.grad.abs().max().item() == 0.0, n
                dead += 1
                continue
            e = relmax(p.grad, og[n]) / _grad_tol_factor(n)
            nz += int((p.grad.abs().max().item() > 0) == (og[n].abs().max().item() > 0))
            if e > worst:
                worst, worst_name = e, n
    res["grad_rel_worst"], res["grad_worst_name"], res["grads_nonzero"] = worst, worst_name, nz
    _observe("qwen_tiny_step", res)
    res["ok"] = bool(res["loss_rel"] < QWEN_BARS[0] and res.get("pred_rel", 0.0) < QWEN_BARS[1] and worst < QWEN_BARS[2] and nz == len(og) - dead)
    if verbose:
        print(res)
    return res


def run_flux_step_parity(device="cuda:0", verbose=False, cfg=None, hw=(4, 6), T=7, B=2, r=4, guidance=True, fused=True,
                         targets=("to_k", "to_q", "to_v", "to_out.0")):
    """FLUX-Kontext LoRA step: HIP path vs the bf16 oracle (1 target + 1 control image of the same size)."""
    from common import FLUX_TINY, fill_weights
    from oracle import flux_dit as FO
    from oracle import qwen_dit as O
    from qflux_amd.models import FluxTransformer2DModel
    from qflux_amd.modules import LoraConfig
    from qflux_amd.trainer import FluxKontextTrainStep

    cfg = dict(FLUX_TINY if cfg is None else cfg)
    cfg["guidance_embeds"] = guidance
    if cfg["joint_attention_dim"] % 64:
        cfg["joint_attention_dim"] = 64      # the GEMM contracts in 64-wide K tiles
    oracle = FO.OracleFluxDiT(**cfg)
    O.add_lora(oracle, r=r, lora_alpha=2 * r, adapter_name="lora_edit", target_modules=targets)
    fill_weights(oracle, seed=5)
    for n, p in oracle.named_parameters():
        if "lora" not in n:
            p.data = p.data.to(BF)
    with torch.device(device):
        hip = FluxTransformer2DModel(**cfg)
    hip.add_adapter(LoraConfig(r=r, lora_alpha=2 * r, target_modules=(targets if isinstance(targets, str) else list(targets))), "lora_edit")
    missing, unexpected = hip.load_state_dict(oracle.state_dict(), strict=True)
    assert not missing and not unexpected
    g = torch.Generator().manual_seed(31)
    h, w = hw
    S_t = h * w
    ctl_ids = FO.prepare_latent_image_ids(h, w)
    ctl_ids[:, 0] = 1
    emb = dict(image_latents=torch.randn(B, S_t, 64, generator=g).half(), control_latents=torch.randn(B, S_t, 64, generator=g).half(),
               control_ids=ctl_ids, text_ids=torch.zeros(T, 3), latent_hw=(h, w),
               pooled_prompt_embeds=torch.randn(B, cfg["pooled_projection_dim"], generator=g).half(),
               prompt_embeds=torch.randn(B, T, cfg["joint_attention_dim"], generator=g).half())
    noise = torch.randn(B, S_t, 64, generator=g).to(BF)
    t = torch.tensor([0.7109, 0.1611, 0.43, 0.9][:B]).to(BF)
    emb_o = dict(emb, control_latents=emb["control_latents"].to(BF))
    loss_o, pred_o = FO.flux_compute_loss(oracle, emb_o, noise, t, BF, return_pred=True)
    loss_o.float().backward()
    # Round 6 (profiles/r06_flux_bar_noise.json): the tiny FLUX bf16 graph differs from ITSELF by up to 3.8e-2 of a
    # gradient tensor's maximum when only the reduction order changes (torch CPU kernels vs rocBLAS on the GPU; 8 weight seeds) -- the
    # 4e-2 gradient bar sits at the eager graph's own noise, and the HIP path's worst tensor (3.9e-2) is the oracle's own worst tensor.
    # So the same oracle step is ALSO evaluated on the GPU and a tensor may exceed the bar only as far as twice the oracle's self-noise
    # on that very tensor.
    import copy
    oracle_g = copy.deepcopy(oracle).to(device)
    for p_ in oracle_g.parameters():
        p_.grad = None
    emb_g = {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in emb_o.items()}
    FO.flux_compute_loss(oracle_g, emb_g, noise.to(device), t.to(device), BF).float().backward()
    self_noise = {n: relmax(p_.grad, dict(oracle.named_parameters())[n].grad) for n, p_ in oracle_g.named_parameters()
                  if "lora" in n and p_.grad is not None and dict(oracle.named_parameters())[n].grad is not None}
    step = FluxKontextTrainStep(hip)
    res = {}
    if fused:
        loss_h = step.forward_backward(emb, noise=noise, t=t)
        plan = list(hip._plans.values())[0]
        pred_h = plan.A["out"].view(B, -1, plan.A["out"].shape[-1])[:, :S_t]
        res["pred_rel"] = relmax(pred_h, pred_o)
    else:
        loss_h = step.compute_loss(emb, noise=noise, t=t)
        plan = list(hip._plans.values())[0]
        res["pred_rel"] = relmax(plan.A["out"].view(B, -1, plan.A["out"].shape[-1])[:, :S_t], pred_o)
        loss_h.backward()
    torch.cuda.synchronize()
    res["loss_oracle"], res["loss_hip"] = loss_o.item(), loss_h.item()
    res["loss_rel"] = abs(loss_h.item() - loss_o.item()) / abs(loss_o.item())
    og = {n: p.grad for n, p in oracle.named_parameters() if "lora" in n}
    worst, worst_name, bad, worst_norm = 0.0, None, 0, 0.0
    for n, p in hip.named_parameters():
        if "lora" in n:
            if og[n] is None:
                assert p.grad.abs().max().item() == 0.0, n
                continue
            e = relmax(p.grad, og[n]) / _grad_tol_factor(n)
            bad += int((p.grad.abs().max().item() > 0) != (og[n].abs().max().item() > 0))
            if e > worst:
                worst, worst_name = e, n
            # normalised: 1.0 = the bar, or twice the eager graph's own noise on this tensor where that is larger
            worst_norm = max(worst_norm, e / max(FLUX_BARS[2], 2.0 * self_noise.get(n, 0.0) / _grad_tol_factor(n)))
    res["grad_rel_worst"], res["grad_worst_name"], res["n_lora"] = worst, worst_name, len(og)
    res["grad_rel_worst_over_allowed"] = worst_norm
    res["oracle_self_noise_worst"] = max(self_noise.values()) if self_noise else 0.0
    _observe("flux_tiny_step", res)
    res["ok"] = bool(res["loss_rel"] < FLUX_BARS[0] and res.get("pred_rel", 0.0) < FLUX_BARS[1] and worst_norm < 1.0 and bad == 0)
    if verbose:
        print(res)
    return res


def assert_step_bit_reproducible(plan, run_step, gflat, zero_grad, what=""):
    """Two identical fused steps, each started from a ZEROED arena: every arena tensor must come out bit-identical (position-weighted
    check-sums over all raw bytes).  The flat LoRA gradient is bit-identical as well since round 6 (chunk partials summed in chunk
    order instead of fp32 atomics); the scalar loss (one fp32 atomic per block of the criterion) is held to 1e-6.  `run_step()` -> loss tensor; `gflat` the flat gradient buffer."""
    tens, seen = [], set()

    def flat(prefix, obj):
        if isinstance(obj, torch.Tensor):
            key = (obj.data_ptr(), obj.numel(), obj.dtype)
            if obj.numel() and key not in seen:
                seen.add(key)
                tens.append((prefix, obj))
        elif isinstance(obj, dict):
            for k, v in obj.items():
                flat(f"{prefix}.{k}", v)
        elif isinstance(obj, (list, tuple)):
            for i, v in enumerate(obj):
                flat(f"{prefix}[{i}]", v)
    flat("A", plan.A)

    def checksum(t):
        """Position-weighted check-sum over EVERY raw byte (int64 words times odd position weights, wrapping; the size % 8 tail bytes
        weighted separately): a permutation of words or a change in the trailing bytes changes it, unlike a plain sum."""
        raw = (t if t.is_contiguous() else t.contiguous()).view(torch.uint8).view(-1)
        n8 = raw.numel() // 8
        acc = 0
        CH = 1 << 24
        words = raw[: n8 * 8].view(torch.int64)
        for c0 in range(0, n8, CH):
            wv = words[c0:c0 + CH]
            pos = torch.arange(c0, c0 + wv.numel(), device=wv.device, dtype=torch.int64)
            acc = (acc + int((wv * (pos * 0x9E3779B1 + 1)).sum().item())) & 0xFFFFFFFFFFFFFFFF
        tail = raw[n8 * 8:]
        if tail.numel():
            acc = (acc + int((tail.to(torch.int64) * torch.arange(1, tail.numel() + 1, device=tail.device)).sum().item()) * 0x10001) & 0xFFFFFFFFFFFFFFFF
        return acc

    def one():
        for _, t in tens:
            t.zero_()
        loss = run_step().item()
        torch.cuda.synchronize()
        sums = [checksum(t) for _, t in tens]
        g = gflat.clone()
        zero_grad()
        return loss, sums, g
    l1, s1, g1 = one()
    l2, s2, g2 = one()
    bad = [tens[i][0] for i in range(len(tens)) if s1[i] != s2[i]]
    assert abs(l1 - l2) <= 1e-6 * abs(l1) and not bad, (what, l1, l2, bad[:6])
    # round 6: the weight-gradient launches add their token chunks in a fixed order (qfx_lora_grad_args.ws): the flat gradient is bit-identical too
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)), (what, ((g1 - g2).abs().max() / g1.abs().max()).item())
    return len(tens)
