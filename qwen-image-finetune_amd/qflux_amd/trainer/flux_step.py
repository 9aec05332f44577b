"""Cached-embedding LoRA training step for FLUX-Kontext on MI355X.

Mirrors FluxKontextLoraTrainer._compute_loss_shared_mode (src/qflux/trainer/flux_kontext_trainer.py:494-577):
noise ~ N(0,1) bf16, t ~ U(0,1) bf16 (both injectable, :515-521), x_t = (1-t) x0 + t noise, latent ids built per
step (:871-883), concat with the control latents / ids, guidance = 1 when the model has guidance embeddings,
model call, slice, target = noise - x0, MSE.  Same two ways to drive it as QwenLoraTrainStep.
"""
from __future__ import annotations

import torch

from .. import ops
from ..schedules import shift_time, timestep_density
from .qwen_step import BF, QwenLoraTrainStep


def prepare_latent_image_ids(height: int, width: int) -> torch.Tensor:
    ids = torch.zeros(height, width, 3)
    ids[..., 1] = ids[..., 1] + torch.arange(height)[:, None]
    ids[..., 2] = ids[..., 2] + torch.arange(width)[None, :]
    return ids.reshape(height * width, 3)


class FluxKontextTrainStep(QwenLoraTrainStep):
    def _draw_t(self, n, dev, t=None):
        """(t [n] in the weight dtype on the device, float(t) on the CPU or None).  With every objective option at its default: the
        reference's device draw, nothing comes back to the host.  Otherwise u from the step's density on the CPU generator, shifted;
        an injected t is final.  The CPU copy (a device-to-host copy for an injected device tensor) feeds weighting and threshold."""
        dt = self.weight_dtype
        if t is None and self.weighting_scheme == "none" and self.timestep_shift == 1.0 and not self._general_objective:
            return torch.rand((n,), device=dev, dtype=dt), None
        if t is None:
            u = timestep_density(self.weighting_scheme, n, self.logit_mean, self.logit_std, self.mode_scale)
            t = shift_time(u, self.timestep_shift).to(dt)
        else:
            t = t.to(dt)
        return t.to(dev), (t.float().cpu() if self._general_objective else None)

    def _prepare_flux(self, embeddings, noise=None, t=None):
        dev = self.dit.device
        x0 = embeddings["image_latents"].to(dev, non_blocking=True)
        if x0.dtype != torch.float16:   # the embedding cache stores fp16 (cache_manager.py:78); keep its rounding behaviour
            x0 = x0.to(torch.float16)
        ctrl = embeddings["control_latents"].to(dev, non_blocking=True).to(self.weight_dtype)
        pe = embeddings["prompt_embeds"].to(dev, non_blocking=True).to(self.weight_dtype)
        pooled = embeddings["pooled_prompt_embeds"].to(dev, non_blocking=True).to(self.weight_dtype)
        B = x0.shape[0]
        noise = torch.randn(x0.shape, device=dev, dtype=self.weight_dtype) if noise is None else noise.to(dev).to(self.weight_dtype)
        t, t_host = self._draw_t(B, dev, t)
        self._step_objective = None if t_host is None else self._stage_objective(t_host * 1000, t_host, dev)
        packed, target = ops.flowmatch_prepare(x0.contiguous(), noise.contiguous(), ctrl.contiguous(), t.contiguous(), mode=1)
        h, w = embeddings["latent_hw"]
        img_ids = torch.cat([prepare_latent_image_ids(h, w), embeddings["control_ids"].float().cpu()], dim=0)
        txt_ids = embeddings["text_ids"].float().cpu()
        guidance = torch.ones((B,), device=dev, dtype=self.weight_dtype) if self.dit.config.guidance_embeds else None
        return packed, target, pe, pooled, t, guidance, img_ids, txt_ids, x0.shape[1]

    def compute_loss(self, embeddings, noise=None, t=None):
        packed, target, pe, pooled, t, guidance, img_ids, txt_ids, S_t = self._prepare_flux(embeddings, noise, t)
        pred = self.dit(hidden_states=packed, timestep=t, guidance=guidance, pooled_projections=pooled, encoder_hidden_states=pe,
                        txt_ids=txt_ids, img_ids=img_ids, joint_attention_kwargs={}, return_dict=False)[0]
        pred = pred[:, :S_t]
        if self._step_objective is not None:
            tok_w = self._token_weights(embeddings, target.shape[0], S_t, pred.device) if self.criterion == "mask_edit" else None
            return self._general_loss(pred, target, tok_w, 1.0 / (target.shape[0] * S_t))
        el = (pred.float() - target.float()) ** 2
        if self.criterion == "mask_edit":      # forward_loss(..., edit_mask=embeddings["edit_mask"]) (flux_kontext_trainer.py:570-574)
            el = el * self._token_weights(embeddings, target.shape[0], S_t, el.device).unsqueeze(-1)
        return torch.mean(el.reshape(target.shape[0], -1), dim=1).mean()

    def forward_backward(self, embeddings, noise=None, t=None, grad_scale=1.0, sync=True):
        """Same contract as QwenLoraTrainStep.forward_backward (criterion "mse" | "mask_edit", sync=False = no_sync micro-step)."""
        packed, target, pe, pooled, t, guidance, img_ids, txt_ids, S_t = self._prepare_flux(embeddings, noise, t)
        plan = self.dit.get_plan(packed.shape[0], packed.shape[1], pe.shape[1], img_ids, txt_ids)
        return self._fused_pass(plan, (packed, pooled, guidance), pe, t, target, S_t, grad_scale, sync, embeddings)

    def train_step(self, embeddings, noise=None, t=None, micro_batches=None):
        """QwenLoraTrainStep.train_step with FLUX's keyword t (the flow-matching times, injectable like noise)."""
        return super().train_step(embeddings, noise, t, micro_batches)

    def compute_loss_multires(self, samples, txt):
        """Autograd path: AttentionMaskMseLoss(reduction='mean') on the masked prediction (attention_mask_loss.py:146-226)."""
        b = _build_multires_batch(self, samples, txt)
        pred = self.dit(hidden_states=b["inp"], timestep=b["timestep"], guidance=b["guidance"], pooled_projections=b["pooled"],
                        encoder_hidden_states=b["pe"], txt_ids=b["txt_ids"], img_ids=b["ids"], attention_mask=b["mask"],
                        joint_attention_kwargs={}, return_dict=False)[0][:, : b["n_t_max"]]
        if self._step_objective is not None:
            return self._general_loss(pred, b["target"], b["tok_w"], 1.0 / (b["n_valid"] + 1e-12))
        el = (pred.float() - b["target"].float()) ** 2
        tok = (el * b["tok_w"].unsqueeze(-1)).mean(dim=2)
        return tok.sum() / (b["n_valid"] + 1e-12)

    def forward_backward_multires(self, samples, txt, grad_scale=1.0, sync=True):
        b = _build_multires_batch(self, samples, txt)
        B, S_i, T = b["inp"].shape[0], b["inp"].shape[1], b["pe"].shape[1]
        valid = b["mask"][:, T:].sum(dim=1).tolist()
        plan = self.dit.get_plan_multires(B, S_i, T, b["ids"], valid)
        return self._fused_pass(plan, (b["inp"], b["pooled"], b["guidance"]), b["pe"], b["timestep"], b["target"], b["n_t_max"], grad_scale,
                                sync, tok_w=b["tok_w"].contiguous(), inv_denom=1.0 / (b["n_valid"] + 1e-12))


def _build_multires_batch(step, samples, txt):
    """Host/device plumbing of _compute_loss_multi_resolution_mode (flux_kontext_trainer.py:579-760): per-sample ids,
    x_t, right-padding to the batch maximum, masks.  samples[i]: image_latents [n_t,64], control_latents [n_c,64],
    hw, control_hw [(h,w),...], optional noise / t."""
    dev, dt = step.dit.device, step.weight_dtype
    B = len(samples)
    seqs, ids, n_t = [], [], []
    noises, ts, ts_host = [], [], []
    for smp in samples:
        x0 = smp["image_latents"].to(dev)
        ctrl = smp["control_latents"].to(dev)
        noise = smp["noise"].to(dev).to(dt) if "noise" in smp else torch.randn(x0.shape, device=dev, dtype=dt)
        t, t_host = step._draw_t(1, dev, smp["t"].reshape(1) if "t" in smp else None)
        ts_host.append(t_host)
        t_ = t.unsqueeze(1)
        x_t = (1.0 - t_) * x0 + t_ * noise                      # bf16 * cache dtype promotes like the reference
        seqs.append(torch.cat([x_t.to(dt), ctrl.to(dt)], dim=0))
        h, w = smp["hw"]
        parts = [prepare_latent_image_ids(h, w)]
        for j, (ch, cw) in enumerate(smp["control_hw"]):
            ci = prepare_latent_image_ids(ch, cw)
            ci[..., 0] = j + 1
            parts.append(ci)
        ids.append(torch.cat(parts, dim=0))
        assert ids[-1].shape[0] == seqs[-1].shape[0]
        n_t.append(x0.shape[0]); noises.append(noise); ts.append(t)
    S_max, n_t_max = max(s.shape[0] for s in seqs), max(n_t)
    T = txt["text_ids"].shape[0]
    inp = torch.zeros(B, S_max, 64, device=dev, dtype=dt)
    idb = torch.zeros(B, S_max, 3)
    full = torch.ones(B, T + S_max, dtype=torch.bool)
    tok_w = torch.zeros(B, n_t_max)
    target = torch.zeros(B, n_t_max, 64, device=dev, dtype=dt)
    for i in range(B):
        L = seqs[i].shape[0]
        inp[i, :L] = seqs[i]
        idb[i, :L] = ids[i]
        full[i, T + L:] = False
        tok_w[i, : n_t[i]] = 1.0
        target[i, : n_t[i]] = noises[i] - samples[i]["image_latents"].to(dev).to(dt)
    timestep = torch.cat(ts)
    t_host = torch.cat(ts_host) if step._general_objective else None
    step._step_objective = None if t_host is None else step._stage_objective(t_host * 1000, t_host, dev)
    guidance = torch.ones((B,), device=dev, dtype=dt) if step.dit.config.guidance_embeds else None
    pe = txt["prompt_embeds"].to(dev).to(dt)
    pooled = txt["pooled_prompt_embeds"].to(dev).to(dt)
    return dict(inp=inp, ids=idb, mask=full, tok_w=tok_w.to(dev), target=target, timestep=timestep, guidance=guidance, pe=pe,
                pooled=pooled, txt_ids=txt["text_ids"].float().cpu(), n_t_max=n_t_max, n_valid=float(sum(n_t)))
