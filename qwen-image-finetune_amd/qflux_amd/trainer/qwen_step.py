"""The cached-embedding LoRA training step for Qwen-Image-Edit on MI355X.

Mirrors the reference's step (names and argument meaning):
  QwenImageEditTrainer._compute_loss      src/qflux/trainer/qwen_image_edit_trainer.py:777-849
  BaseTrainer.train_epoch (one iteration) src/qflux/trainer/base_trainer.py:508-561
  BaseTrainer.clip_gradients              :449-455   (global-norm clip, here over the trainable params only)
  DDP of the LoRA container               :384-393   (here: ONE explicit RCCL all-reduce of the flat LoRA gradient)

Two ways to drive it:
  * drop-in: `loss = step.compute_loss(embeddings)` returns an autograd scalar built on `self.dit(...)`;
    `loss.backward()`, any torch optimizer over the LoRA parameters.
  * fused (bench / production): `step.train_step(embeddings)` = prepare -> DiT forward program -> criterion
    kernel (loss + dpred) -> DiT backward program -> all-reduce -> fused clip+AdamW; no autograd graph, no
    host synchronisation anywhere in the step.

Beside the step: the bucketed gradient exchange is dp.LoraGradSync (step.sync), the YAML -> keyword mapping is
trainer/optim_config.py, the timestep tables and lr schedules are qflux_amd/schedules.py.
"""
from __future__ import annotations

import contextlib
import os
import re

import torch
import torch.distributed as dist

from .. import dropout as DR
from .. import ema as E
from .. import regularize as RG
from .. import telemetry as TM
from .. import ops
from ..dp import LoraGradSync, check_replicas, init_distributed_from_env  # noqa: F401  (the last: bench.py and tools/ import it from here)
from ..schedules import HUBER_SCHEDULES, WEIGHTING_SCHEMES, flowmatch_tables, huber_threshold, loss_weighting, timestep_density
from . import adam8bit as A8
from . import optim_state as OS
from .optim_state import resolve_family

BF = torch.bfloat16


def map_mask_to_latent(image_mask: torch.Tensor) -> torch.Tensor:
    """[B,H,W] pixel-space edit mask -> [B, (H/16)(W/16)] packed-latent token mask: 8x8 average pool (VAE stride), then
    the maximum over each 2x2 packing patch (src/qflux/losses/edit_mask_loss.py:7-36).  Host-side plumbing."""
    B, H, W = image_mask.shape
    lh, lw = H // 8, W // 8
    m = torch.nn.functional.avg_pool2d(image_mask.float().unsqueeze(1), kernel_size=8, stride=8).squeeze(1)
    m = m.reshape(B, lh // 2, 2, lw // 2, 2).permute(0, 1, 3, 2, 4).reshape(B, lh // 2, lw // 2, 4)
    return m.max(dim=-1)[0].reshape(B, (lh // 2) * (lw // 2))


class QwenLoraTrainStep:
    def __init__(self, dit, lr=1e-4, betas=None, eps=1e-8, weight_decay=None, max_grad_norm=1.0,
                 weight_dtype=BF, process_group=None, criterion="mse", forground_weight=2.0, background_weight=1.0,
                 bucket_mb=24.0, optimizer="adamw", optimizer_args=None, param_groups=None, loraplus_lr_ratio=None, ema_decay=None,
                 ema_args=None, weighting_scheme="none", logit_mean=0.0, logit_std=1.0, mode_scale=1.29, timestep_shift=1.0,
                 loss_type="l2", huber_c=0.1, huber_schedule="constant", max_weight_norm=None, network_dropout=None, rank_dropout=None,
                 dropout_seed=0, adapter_stats_every=0):
        """optimizer / optimizer_args / weight_decay / betas: the optimizer family, the extra init_args of its class and the defaults
        that None stands for -- every family is described at optim_state.resolve_family, which reads them.  With Prodigy `lr` is the
        schedule multiplier the reference sets to 1.0; with Adafactor lr must be None with relative_step (the default) and a float
        without it; with CAME betas is the package's triple and lr must be > 0.
        param_groups: parameter groups by name -- a list of dicts, each a "match" regex (re.search on the adapter parameter's name)
        plus any of lr, weight_decay, betas, eps; the first matching rule wins, unmatched parameters form the default group with
        this constructor's values (the last group).  The families with grouped kernels (optim_state: AdamW / Adam, SGD, Lion, RAdam,
        NAdam, Adamax, AdEMAMix, the blockwise 8-bit ones) step all groups in their one launch; every other family refuses a second group.  An lr schedule
        written to `self.lr` scales every group's lr by the same factor self.lr / (the constructor's lr), as torch's schedulers do
        with the groups' initial_lr.  loraplus_lr_ratio: shorthand for the two LoRA+ groups of
        qflux_amd.optim.loraplus_param_groups -- lora_A at lr, lora_B at lr * ratio.
        ema_decay: None, a float or 1..4 floats -- exponential moving averages of the adapter weights (qflux_amd.ema: diffusers'
        EMAModel), one shadow per decay, updated in one launch behind every optimizer step; ema_args: EMAModel's min_decay,
        update_after_step, use_ema_warmup, inv_gamma, power.  eval(ema=k) / eval_mode(ema=k) put shadow k into the adapter weights
        (sampling with train_step=... uses shadow 0), save_checkpoint writes them beside the trained weights.  Refused with
        optimizer="adamw_schedulefree", whose x is an average already and wants the same eval swap.  None: nothing is allocated or
        launched.
        criterion: "mse" = MseLoss (losses/mse_loss.py:46-83); "mask_edit" = MaskEditLoss(forground_weight,
        background_weight) (losses/edit_mask_loss.py:39-90), fed by embeddings["edit_mask"] [B,S_t] (all-ones when absent).
        weighting_scheme: diffusers' one knob over the timestep density and the loss weighting (schedules.timestep_density /
        loss_weighting): "none" | "logit_normal" (logit_mean, logit_std) | "mode" (mode_scale) shape where the timesteps fall,
        "sigma_sqrt" | "cosmap" draw uniformly and weight every sample's loss by its sigma.  timestep_shift: the time shift
        shift s / (1 + (shift - 1) s) of the sigma table (Qwen: flowmatch_tables(shift=), the modulation table is keyed on the same
        timesteps) or of the drawn t (FLUX).  loss_type: "l2" | "huber" | "smooth_l1" (kohya's pseudo-Huber forms, include/qfx.h)
        with the threshold huber_c, per sample huber_c ** (timestep / 1000) under huber_schedule="exponential".  An injected u / t
        is taken as the final value: density and shift are skipped, weighting and threshold follow from it.  With unit weights
        and "l2" (every default) the step launches the two MSE kernels as before and last_sample_losses is None; otherwise the
        general criterion kernel, after which last_sample_losses holds the per-sample losses ([B] on the device, no host sync).
        max_weight_norm: None, a positive float or inf -- kohya's --scale_weight_norms (qflux_amd.regularize): behind every
        optimizer step, in one launch and before the EMA update, every adapter pair whose ||scaling B A||_F exceeds the value is
        scaled back onto it (inf: measured only).  last_weight_norms then holds the per-pair norms, ratios and the summary on the
        device (no host sync), weight_norm_stats() reads (keys_scaled, mean norm, max norm).  Refused with
        optimizer="adamw_schedulefree": the clamp would scale y and leave z, which breaks the average.  None: nothing is allocated
        or launched.
        network_dropout / rank_dropout / dropout_seed: kohya's dropout on the adapters' rank-r activation lx = lora_down(x) and its
        per-sample rank dropout (qflux_amd.dropout), 0 <= p < 1, forwarded to dit.set_lora_dropout when either is given (None, None:
        the model's setting stays).  Active while the step is in training mode (the default); eval() / eval_mode() and the samplers
        switch the masks off, train() on again -- nn.Dropout's rule, through one device word, so a captured graph follows without
        being captured again.  Every training forward (each micro-batch) draws new masks; with a process group rank k draws the
        masks of samples k * B ... .  state_dict() / save_checkpoint carry {seed, step, network_dropout, rank_dropout} under the key
        "lora_dropout" only while the feature is on, and loading restores them: a resumed run draws the masks the uninterrupted run
        would have drawn.  Not with the MX-FP8 trunk (NotImplementedError); adapters on the conditioning head run without dropout.
        Both 0: the plans emit exactly the launches they emit without the option.
        adapter_stats_every: 0 (off, the default: nothing is allocated or launched) or N > 0 -- per-adapter telemetry
        (qflux_amd.telemetry): on every optimizer step whose number is a multiple of N two launches bracket the optimizer's and
        leave, for every adapter tensor, the norm of the clipped gradient the optimizer stepped with, the weight norm, the norm of
        the update, ||update|| / ||weight||, the gradient's largest magnitude and the non-finite counts on the device.
        last_adapter_stats reads them (the only host synchronisation; None before the first collected step),
        adapter_stats_summary() condenses them.  The weights train bit-identically with and without it.  Every optimizer family is
        served: only the flat weight and gradient buffers are read.  Measured in front of the max-norm clamp and the EMA update.
        Not with capture_graph (the every-N gate is host control flow)."""
        if criterion not in ("mse", "mask_edit"):
            raise ValueError(f"unknown criterion {criterion!r}")
        self.optimizer_alias, self.optimizer, self._opt_cls, weight_decay, self.optimizer_args = resolve_family(optimizer, weight_decay,
                                                                                                                optimizer_args)
        if self.optimizer == "adafactor":
            self._opt_cls.validate(self.optimizer_args, lr)
        if self.optimizer == "came":        # lr > 0 and a betas triple, as the package's constructor asks
            self._opt_cls.validate(self.optimizer_args, lr, OS.default_betas("came") if betas is None else tuple(betas))
        if weighting_scheme not in WEIGHTING_SCHEMES:
            raise ValueError(f"weighting_scheme is one of {WEIGHTING_SCHEMES}, not {weighting_scheme!r}")
        if loss_type not in ops.LOSS_KINDS:
            raise ValueError(f"loss_type is one of {tuple(ops.LOSS_KINDS)}, not {loss_type!r}")
        if huber_schedule not in HUBER_SCHEDULES:
            raise ValueError(f"huber_schedule is one of {HUBER_SCHEDULES}, not {huber_schedule!r}")
        if not 0 < huber_c < float("inf"):
            raise ValueError(f"huber_c must be positive and finite, not {huber_c}")
        if not 0 < timestep_shift < float("inf"):
            raise ValueError(f"timestep_shift must be positive and finite, not {timestep_shift}")
        self.weighting_scheme, self.logit_mean, self.logit_std, self.mode_scale = weighting_scheme, logit_mean, logit_std, mode_scale
        self.timestep_shift, self.loss_type, self.huber_c, self.huber_schedule = float(timestep_shift), loss_type, float(huber_c), huber_schedule
        # the general criterion kernel is launched only where the objective needs it: per-sample weights or a Huber form
        self._general_objective = weighting_scheme in ("sigma_sqrt", "cosmap") or loss_type != "l2"
        self._step_objective = None       # (sample_w, huber_c) of the batch last prepared, on the device; None on the MSE path
        self.last_sample_losses = None    # [B] device fp32 after a fused pass through the general criterion
        self.ema_decays, self.ema_args = E.check_config(ema_decay, ema_args)
        if self.ema_decays is not None and self.optimizer == "adamw_schedulefree":
            raise ValueError("ema_decay with optimizer='adamw_schedulefree': the schedule-free x is the averaged point already, and both "
                             "want the eval swap of the adapter weights")
        self.ema = None             # qflux_amd.ema.EmaState, from the first step, eval() or load_checkpoint on (ema_decay given)
        self.max_weight_norm = RG.check_max_norm(max_weight_norm)
        if self.max_weight_norm is not None and self.optimizer == "adamw_schedulefree":
            raise ValueError("max_weight_norm with optimizer='adamw_schedulefree': scaling y and not z breaks the schedule-free average")
        self.last_weight_norms = None     # qflux_amd.regularize.MaxNormState, from the first step on (max_weight_norm given)
        if isinstance(adapter_stats_every, bool) or not isinstance(adapter_stats_every, int) or adapter_stats_every < 0:
            raise ValueError(f"adapter_stats_every must be an int >= 0, not {adapter_stats_every!r}")
        self.adapter_stats_every = adapter_stats_every
        self._adapter_stats = None        # qflux_amd.telemetry.AdapterStats, from the first collected step on
        self.blockwise = optimizer in A8.BLOCKWISE
        self.opt_state = None       # the family's optim_state object, from the first step or load_state_dict on
        self.criterion, self.fg, self.bg = criterion, float(forground_weight), float(background_weight)
        self.dit = dit
        if network_dropout is not None or rank_dropout is not None:
            pe, pr = DR.check_probability(network_dropout, "network_dropout"), DR.check_probability(rank_dropout, "rank_dropout")
            dit.set_lora_dropout(pe, pr, dropout_seed)
        betas = OS.default_betas(self.optimizer) if betas is None else tuple(betas)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        if loraplus_lr_ratio is not None:
            if param_groups is not None:
                raise ValueError("give either param_groups or loraplus_lr_ratio")
            if not loraplus_lr_ratio > 0:
                raise ValueError(f"loraplus_lr_ratio must be positive, not {loraplus_lr_ratio}")
            param_groups = [{"match": r"lora_A", "lr": lr}, {"match": r"lora_B", "lr": lr * loraplus_lr_ratio}]
        self._base_lr = lr
        self.group_rules = self._check_rules(param_groups)
        self._grouping = None       # (adapter names, rows, members) of the store layout the rules were last applied to
        self.max_grad_norm = max_grad_norm
        self.weight_dtype = weight_dtype
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        self.timesteps_tbl, self.sigmas_tbl = flowmatch_tables(shift=self.timestep_shift)
        # frozen conditioning head: the AdaLN modulation vectors of every training timestep, computed once here so that no step pays
        # for it (dit.ensure_modulation_table; QFX_MOD_TABLE=0 / QFX_MOD_TABLE_GB; nothing happens with adapters on the head)
        if getattr(dit, "_MOD_TABLE", False):
            dit.set_modulation_keys(self.timesteps_tbl / 1000)
            dit.ensure_modulation_table()
        self.global_step = 0
        self._gnorm = self._gparts = None
        # data-parallel exchange overlapped with the backward: the flat gradient is all-reduced in buckets of whole DiT
        # blocks as soon as their backward segment has been enqueued (the gradient of block i is final when its segment ends).
        # An exchange object of this step's own, apart from dit._dp (the drop-in path's: group and bucket size may differ).
        # QFX_DP_FORCE=1: run the bucketed exchange on a ONE-rank process group too (the collectives are then identities) -- lets a
        # one-GPU box execute the real RCCL code path: communicator, RCCL's stream, async handles, ordering against the main and
        # the side gradient stream (tests/test_dp_gpu.py)
        self.sync = LoraGradSync(dit, process_group, bucket_mb,
                                 force=os.environ.get("QFX_DP_FORCE", "0") == "1" and dist.is_available() and dist.is_initialized())
        self._synced = False      # rank 0's adapter / optimizer state is broadcast before the first step (broadcast_state)
        self._synced_version = None

    @property
    def bucket_bytes(self):
        """The exchange's bucket size (bench.py reports it)."""
        return self.sync.bucket_bytes

    def _ensure_synced(self):
        """Rank 0's adapter + optimizer state reaches every rank before the first step AND again whenever the model's adapter set
        was re-injected or re-loaded since (dit._adapter_gen moves on add_adapter / load_lora_adapter / load_state_dict ONLY): a
        re-loaded adapter must not depend on every rank having produced identical weights.  Purely local actions that rebuild the
        plans (.to(), set_adapter, merge / unmerge, quantize_trunk: dit._version) do NOT trigger the collective -- a rank-0-only
        validation or merge would otherwise leave the ranks with mismatched collectives and hang the job; call
        resync() on every rank after such an action if the adapter weights themselves were changed by it."""
        ver = getattr(self.dit, "_adapter_gen", 0)
        if not self._synced or self._synced_version != ver:
            self._synced, self._synced_version = True, ver
            if self.world > 1:
                self.dit.lora_store
                self.broadcast_state()

    def resync(self):
        """Explicit collective resync (every rank must call it): rank 0's adapter + optimizer state to all ranks at the next step."""
        self._synced = False

    # ------------------------------------------------------------------ sampling (CPU RNG like the reference)
    def sample_timesteps(self, batch_size, u=None):
        if u is None:    # compute_density_for_timestep_sampling; "none" is torch.rand(size=(batch_size,), device="cpu")
            u = timestep_density(self.weighting_scheme, batch_size, self.logit_mean, self.logit_std, self.mode_scale)
        idx = (u * 1000).long().clamp_(0, 999)      # sigmoid rounds to 1.0 in fp32 far out in the tail
        return self.timesteps_tbl[idx], self.sigmas_tbl[idx]

    def _stage_objective(self, timesteps, sigmas, dev):
        """The per-sample inputs of the general criterion from the batch's timesteps (0..1000) and sigmas (CPU [B]), uploaded
        non-blocking: (sample_w or None for unit weights, huber_c or None for l2); None when the MSE kernels serve the objective."""
        if not self._general_objective:
            return None
        sw = hc = None
        if self.weighting_scheme in ("sigma_sqrt", "cosmap"):
            sw = loss_weighting(self.weighting_scheme, sigmas).contiguous().to(dev, non_blocking=True)
        if self.loss_type != "l2":
            hc = huber_threshold(self.huber_schedule, self.huber_c, timesteps).contiguous().to(dev, non_blocking=True)
        return sw, hc

    def _prepare(self, embeddings, noise=None, u=None):
        dev = self.dit.device
        x0 = embeddings["image_latents"].to(self.weight_dtype).to(dev, non_blocking=True)
        ctrl = embeddings["control_latents"].to(self.weight_dtype).to(dev, non_blocking=True)
        pe = embeddings["prompt_embeds"].to(self.weight_dtype).to(dev, non_blocking=True)
        B = x0.shape[0]
        if noise is None:
            noise = torch.randn_like(x0, device=dev, dtype=self.weight_dtype)
        else:
            noise = noise.to(self.weight_dtype).to(dev)
        timesteps, sigmas = self.sample_timesteps(B, u)
        sig = sigmas.to(self.weight_dtype).to(dev, non_blocking=True)
        self._step_objective = self._stage_objective(timesteps, sigmas, dev)
        packed, target = ops.flowmatch_prepare(x0.contiguous(), noise.contiguous(), ctrl.contiguous(), sig)
        t_in = (timesteps / 1000).to(dev, non_blocking=True)
        return packed, target, pe, t_in, x0.shape[1]

    def _ensure_mod_table(self):
        """The modulation table again after the model dropped it (load_state_dict, merge / unmerge, a move): one attribute test when
        it is in place or decided against."""
        if getattr(self.dit, "_MOD_TABLE", False):
            self.dit.ensure_modulation_table()

    # ------------------------------------------------------------------ drop-in (autograd) path
    def compute_loss(self, embeddings, noise=None, u=None):
        packed, target, pe, t_in, S_t = self._prepare(embeddings, noise, u)
        mask = embeddings["prompt_embeds_mask"]
        txt_seq_lens = [pe.shape[1]] * pe.shape[0] if mask is None else mask.sum(dim=1).tolist()
        pred = self.dit(hidden_states=packed, timestep=t_in, guidance=None, encoder_hidden_states_mask=mask,
                        encoder_hidden_states=pe, img_shapes=embeddings["img_shapes"], txt_seq_lens=txt_seq_lens,
                        return_dict=False)[0]
        pred = pred[:, :S_t]
        if self._step_objective is not None:
            tok_w = self._token_weights(embeddings, target.shape[0], S_t, pred.device) if self.criterion == "mask_edit" else None
            return self._general_loss(pred, target, tok_w, 1.0 / (target.shape[0] * S_t))
        el = (pred.float() - target.float()) ** 2            # MseLoss with weighting = 1 (mse_loss.py:71-81)
        if self.criterion == "mask_edit":                      # MaskEditLoss, reduction="mean" (edit_mask_loss.py:62-86)
            el = el * self._token_weights(embeddings, target.shape[0], S_t, el.device).unsqueeze(-1)
        return torch.mean(el.reshape(target.shape[0], -1), dim=1).mean()

    def _general_loss(self, pred, target, tok_w, inv_denom):
        """The objective of qfx_criterion_fwd_bwd in torch, for the autograd paths: pred [B,S_t,C], the batch's staged
        (sample_w, huber_c), tok_w [B,S_t] or None."""
        sw, hc = self._step_objective
        d = pred.float() - target.float()
        if self.loss_type == "l2":
            rho = d ** 2
        else:
            c = hc.reshape(-1, 1, 1)
            r = torch.sqrt(d ** 2 + c ** 2)
            rho = (2 * c if self.loss_type == "huber" else 2.0) * (d ** 2 / (r + c))
        tok = rho.mean(dim=2)
        if tok_w is not None:
            tok = tok * tok_w
        per_sample = target.shape[0] * inv_denom * tok.sum(dim=1)
        return (per_sample if sw is None else sw * per_sample).mean()

    def _token_weights(self, embeddings, B, S_t, dev):
        m = embeddings.get("edit_mask")
        m = torch.ones(B, S_t) if m is None else m.float()
        return (m * self.fg + (1.0 - m) * self.bg).to(dev).contiguous()

    # ------------------------------------------------------------------ fused path
    def forward_backward(self, embeddings, noise=None, u=None, grad_scale=1.0, sync=True):
        """loss (device fp32 scalar); LoRA grads ACCUMULATE into the flat gradient buffer.
        sync=False = accelerator.accumulate()/no_sync micro-step (base_trainer.py:518): no gradient exchange is started; pass
        sync=True on the last micro-step of the window (the buckets then carry the accumulated sums)."""
        packed, target, pe, t_in, S_t = self._prepare(embeddings, noise, u)
        self._ensure_mod_table()
        plan = self.dit.get_plan(packed.shape[0], packed.shape[1], pe.shape[1], embeddings["img_shapes"], None)
        return self._fused_pass(plan, packed, pe, t_in, target, S_t, grad_scale, sync, embeddings)

    def _fused_pass(self, plan, inputs, pe, t, target, n_tok, grad_scale, sync, embeddings=None, tok_w=None, inv_denom=None):
        """The device part of every fused forward_backward: forward program, loss kernel, backward program.  The loss is the MSE
        over the first n_tok predicted tokens; token-weighted with tok_w / inv_denom when given, or with the mask_edit criterion's
        weights (embeddings["edit_mask"]).  With per-sample weights or a Huber form staged by the batch's preparation
        (_step_objective) the general criterion kernel computes it and leaves last_sample_losses.  sync: the bucketed gradient exchange
        runs behind the backward."""
        self.dit.lora_store  # make sure the flat buffers / grads are attached
        self._refuse_in_ema_eval(E.EVAL_GRAD)
        self._ensure_synced()
        self._stage_dropout(target.shape[0])
        pred = plan.run_forward(inputs, pe, t)
        if tok_w is None and self.criterion == "mask_edit":
            B = target.shape[0]
            tok_w, inv_denom = self._token_weights(embeddings, B, n_tok, pred.device), 1.0 / (B * n_tok)
        self.last_sample_losses = None
        if self._step_objective is not None:
            sw, hc = self._step_objective
            loss, self.last_sample_losses, dpred = ops.criterion_fwd_bwd(pred, target, n_tok, sample_w=sw, token_w=tok_w, huber_c=hc,
                                                                         kind=self.loss_type, inv_denom=inv_denom, gscale=grad_scale)
        elif tok_w is None:
            loss, dpred = ops.mse_loss_fwd_bwd(pred, target, n_tok, gscale=grad_scale)
        else:
            loss, dpred = ops.mse_token_weighted_fwd_bwd(pred, target, tok_w, n_tok, inv_denom, gscale=grad_scale)
        self._mark_unexchanged()       # local gradients are added below: whatever exchange a drop-in backward did before is stale
        plan.run_backward(dpred, on_segment=self.sync.hook() if ((self.world > 1 or self.sync.force) and sync) else None)
        return loss

    # ------------------------------------------------------------------ dropout on the adapters' rank-r activation
    def _stage_dropout(self, batch, write_active=False):
        """Before a forward: this replica's first global sample index (rank * batch) into the dropout state; write_active: also the
        `active` word (a captured graph's forward program cannot: plan._sync_dropout)."""
        st = getattr(self.dit, "_dropout", None)
        if st is None:
            return
        rank = dist.get_rank(self.group) if self.world > 1 else 0
        st.set_sample0(rank * batch)
        if write_active:
            st.set_active(st.enabled and self.dit.training)

    def _set_dropout_mode(self, train):
        st = getattr(self.dit, "_dropout", None)
        if st is not None:
            st.enabled = bool(train)

    # ------------------------------------------------------------------ hipGraph replay of the DiT part of the step
    def capture_graph(self, embeddings):
        """Capture [LoRA operand refresh, forward program, loss, backward program] -- every launch of the step except the
        flow-match preparation (host RNG) and the 3 optimizer launches (host-side step count / lr) -- into ONE hipGraph for the
        shape of `embeddings`, side-stream gradient launches and their fork / join events included.  Returns
        step(embeddings, noise=None, u=None) -> loss, a full optimisation step that replays the graph: the ~1.45k ctypes calls
        of the Python replay become one hipGraphLaunch.  Inputs are staged through static buffers; all arena pointers are baked
        in, so the graph is valid until the plan is rebuilt (adapter set / quantisation / shape change -> capture again).
        Data-parallel: the gradient exchange runs as one all-reduce after the graph (the bucketed overlap needs the eager
        replay)."""
        if self.criterion == "mask_edit":
            raise NotImplementedError("capture_graph: the mask_edit criterion takes per-step token weights; use train_step")
        if self.adapter_stats_every > 0:
            raise NotImplementedError("capture_graph with adapter_stats_every > 0: collecting on every N-th step is host control "
                                      "flow; use train_step, or set adapter_stats_every=0")
        dit = self.dit
        packed, target, pe, t_in, S_t = self._prepare(embeddings)
        self._ensure_mod_table()
        plan = dit.get_plan(packed.shape[0], packed.shape[1], pe.shape[1], embeddings["img_shapes"], None)
        dit.lora_store
        self._ensure_synced()      # outside the capture: a job driven only by the captured step still starts from rank 0's state
        version = dit._version
        static = [torch.empty_like(t) for t in (packed, target, pe, t_in)]
        for d, s_ in zip(static, (packed, target, pe, t_in)):
            d.copy_(s_)
        # the general criterion's per-step inputs, staged like the four above; its workspace is the graph's own
        obj_static = None if self._step_objective is None else [None if t is None else t.clone() for t in self._step_objective]
        ws = None if obj_static is None else ops.criterion_workspace(target.shape[0], S_t, target.shape[2], target.device)

        def body():
            pred = plan.run_forward(static[0], static[2], static[3])
            if obj_static is None:
                loss, dpred = ops.mse_loss_fwd_bwd(pred, static[1], S_t)
                per_sample = None
            else:
                loss, per_sample, dpred = ops.criterion_fwd_bwd(pred, static[1], S_t, sample_w=obj_static[0], huber_c=obj_static[1],
                                                                kind=self.loss_type, workspace=ws)
            plan.run_backward(dpred)
            return loss, per_sample

        drop = getattr(dit, "_dropout", None)
        drop_step = None if drop is None else drop.step()      # the warm-up pass below draws masks: its step is given back
        self._stage_dropout(packed.shape[0], write_active=True)
        warm = torch.cuda.Stream(device=dit.device)     # one eager pass on a non-default stream (lazy module loads, pool warm-up)
        warm.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(warm):
            body()
        torch.cuda.current_stream().wait_stream(warm)
        self.zero_grad()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss_static, per_sample_static = body()
        self.zero_grad()
        if drop is not None:
            drop.set_step(drop_step)
        shapes = [tuple(t.shape) for t in static]

        def step(emb, noise=None, u=None):
            if dit._version != version or not any(p is plan for p in dit._plans.values()):
                raise RuntimeError("capture_graph: the plan this graph was captured on is gone (adapters / quantisation changed "
                                   "or it was evicted); capture again")
            self._refuse_in_ema_eval(E.EVAL_GRAD)
            ins = self._prepare(emb, noise, u)
            if [tuple(t.shape) for t in ins[:4]] != shapes:
                raise ValueError("capture_graph: batch shape differs from the captured one")
            for d, s_ in zip(static, ins[:4]):
                d.copy_(s_)
            for d, s_ in zip(obj_static or (), self._step_objective or ()):
                if d is not None:
                    d.copy_(s_)
            self._ensure_synced()
            self._mark_unexchanged()
            self._stage_dropout(shapes[0][0], write_active=True)
            graph.replay()
            self.sync.disarm()
            self.optimizer_step(grad_scale=self.allreduce_grads())
            self.zero_grad()
            self.last_sample_losses = None if per_sample_static is None else per_sample_static.clone()
            return loss_static.clone()      # the graph overwrites loss_static on every replay

        step.graph = graph
        step.criterion_workspace = ws      # the graph holds its address: it lives as long as the step does
        return step

    # ------------------------------------------------------------------ gradient exchange (the buckets: dp.LoraGradSync)
    def allreduce_grads(self):
        """Returns the factor the optimizer applies to the summed gradient (1/world)."""
        if self.world > 1 or self.sync.force:
            if self.sync.armed:
                self.sync.finish(average=False)
            else:   # no bucketed backward of THIS object ran (drop-in autograd path, or the hipGraph replay)
                dp = getattr(self.dit, "_dp", None)
                if dp is not None and dp.exchanged:
                    # dit.enable_data_parallel(): the LAST loss.backward() since zero_grad already exchanged (overlapped) and averaged
                    # the accumulated gradient (dp.py sets the flag in finish(); merely being enabled proves nothing -- the captured
                    # graph replays plan.run_backward directly and never passes through the autograd node's exchange)
                    return 1.0
                dist.all_reduce(self.dit.lora_store.gflat, op=dist.ReduceOp.SUM, group=self.group)
            return 1.0 / self.world
        return 1.0

    # ------------------------------------------------------------------ parameter groups
    _RULE_FIELDS = ("lr", "weight_decay", "betas", "eps")

    def _check_rules(self, rules):
        if rules is None:
            return None
        out = []
        for k, r in enumerate(rules):
            unknown = set(r) - {"match", *self._RULE_FIELDS}
            if "match" not in r or unknown:
                raise ValueError(f"param_groups[{k}]: a rule is a dict with a 'match' regex and any of {self._RULE_FIELDS}" +
                                 (f", not {sorted(unknown)}" if unknown else ""))
            self._opt_cls.check_rule_fields(k, r)
            out.append(dict(r, match=re.compile(r["match"]), **({"betas": tuple(r["betas"])} if "betas" in r else {})))
        self._opt_cls.check_groups(len(out))      # a second group is refused here by the families without grouped kernels
        return out

    def param_groups_of(self, store):
        """(rows, members) of the rules over the store's adapter names: one row dict (lr, betas, eps, weight_decay) and one tuple of
        store-entry indices per non-empty group -- the rules' groups in rule order, then the default group.  (None, None) without
        rules or when everything lands in one group."""
        if self.group_rules is None:
            return None, None
        names = tuple(n for n, _, _, _ in store.entries)
        if self._grouping is None or self._grouping[0] != names:
            base = dict(lr=self._base_lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)
            buckets = [[] for _ in range(len(self.group_rules) + 1)]
            for i, n in enumerate(names):
                buckets[next((k for k, r in enumerate(self.group_rules) if r["match"].search(n)), len(self.group_rules))].append(i)
            rows = [dict(base, **{f: r[f] for f in self._RULE_FIELDS if f in r}) for r in self.group_rules] + [base]
            for k, (r, b) in enumerate(zip(self.group_rules, buckets)):
                if not b:
                    raise ValueError(f"param_groups[{k}]: {r['match'].pattern!r} matches no adapter parameter")
            keep = [k for k, b in enumerate(buckets) if b]
            self._opt_cls.check_groups(len(keep))
            self._grouping = (names, [rows[k] for k in keep], tuple(tuple(buckets[k]) for k in keep))
        _, rows, members = self._grouping
        return (rows, members) if len(rows) > 1 else (None, None)

    def _scheduled_rows(self, rows, initial=False):
        """The groups' rows with the schedule's factor self.lr / (constructor lr) on every lr; initial: with the unscheduled lr as
        torch's schedulers keep it in a group, "initial_lr" (a checkpoint restores the factor from it)."""
        if rows is None:
            return None
        f = self.lr / self._base_lr if self.lr != self._base_lr else 1.0
        return [dict(r, lr=r["lr"] * f if f != 1.0 else r["lr"], **({"initial_lr": r["lr"]} if initial else {})) for r in rows]

    def _ensure_opt_state(self):
        st = self.dit.lora_store
        _, members = self.param_groups_of(st)
        self.opt_state = OS.ensure_state(self._opt_cls, self.opt_state, st, self.optimizer_args, members)
        return st

    # ------------------------------------------------------------------ train / eval form of the adapter weights
    @property
    def train_mode(self):
        """False while the adapter weights hold the averaged point x of a schedule-free optimizer or an EMA shadow (eval()); True
        otherwise."""
        if self.ema is not None and self.ema.active is not None:
            return False
        return self.opt_state is None or self.opt_state.train_mode

    def _ensure_ema(self):
        """The EMA state for the store's current layout (ema_decay given): created as copies of the adapter weights as they are now."""
        self.ema = E.ensure_state(self.ema, self.dit.lora_store, self.ema_decays, self.ema_args)
        return self.ema

    def _refuse_in_ema_eval(self, message):
        if self.ema is not None and self.ema.active is not None:
            raise RuntimeError(message.format(k=self.ema.active))

    def _swap(self, train):
        if self.optimizer == "adamw_schedulefree":
            self._ensure_opt_state()
            self.opt_state.swap(self.dit.lora_store, self.betas[0], train)

    def eval(self, ema=0):
        """optimizer="adamw_schedulefree": the adapter weights (lora_store.pflat, which every plan reads its LoRA operands from at
        each pass: no plan is rebuilt) go from y to the averaged x that is sampled from and saved -- the package's optimizer.eval().
        With ema_decay: EMA shadow `ema` is exchanged with the adapter weights.  Nothing happens in eval mode already (the same
        shadow), and for every other family without EMA."""
        self._set_dropout_mode(False)
        if self.ema_decays is not None:
            self._ensure_ema().swap_in(self.dit.lora_store, ema)
        else:
            self._swap(False)

    def train(self):
        """Back from x to y (the package's optimizer.train()), or the trained weights back in place of the EMA shadow, bit for bit;
        nothing happens in train mode already, and for every other family without EMA."""
        self._set_dropout_mode(True)
        if self.ema_decays is not None:
            if self.ema is not None:
                self.ema.swap_out(self.dit.lora_store)
        else:
            self._swap(True)

    @contextlib.contextmanager
    def eval_mode(self, ema=0):
        """`with step.eval_mode():` -- eval() on entry, train() on exit if the step was in train mode before."""
        was = self.train_mode
        drop = getattr(self.dit, "_dropout", None)
        drop_was = drop.enabled if drop is not None else True
        self.eval(ema)
        try:
            yield self
        finally:
            if was:
                self.train()
            self._set_dropout_mode(drop_was)

    def optimizer_step(self, grad_scale=1.0):
        self._refuse_in_ema_eval(E.EVAL_STEP)
        if not self.train_mode:
            raise RuntimeError(self.opt_state.EVAL_STEP)
        st = self._ensure_opt_state()
        if self.ema_decays is not None:
            self._ensure_ema()      # before the first step: the shadows start from the weights that step starts from
        self.global_step += 1
        if self._gnorm is None or self._gnorm.device != st.pflat.device:
            self._gnorm = torch.zeros((), dtype=torch.float32, device=st.pflat.device)
            self._gparts = torch.zeros(1024, dtype=torch.float32, device=st.pflat.device)
        ops.sumsq_det(st.gflat, self._gnorm, self._gparts)     # fixed reduction order: every replica computes the same clip coefficient
        rows, _ = self.param_groups_of(st)
        collect = self.adapter_stats_every > 0 and self.global_step % self.adapter_stats_every == 0
        if collect:      # around the optimizer's launch, same stream: the gradient it steps with, the update it makes
            if self._adapter_stats is None:
                self._adapter_stats = TM.AdapterStats(self.dit)
            self._adapter_stats.before_step(self._gnorm, self.max_grad_norm, grad_scale)
        self.opt_state.step(st, self.lr, self.betas, self.eps, self.weight_decay, self.global_step, self._gnorm, self.max_grad_norm,
                            grad_scale, self.optimizer_args, **({"groups": self._scheduled_rows(rows)} if rows else {}))
        if collect:
            self._adapter_stats.after_step()
        if self.max_weight_norm is not None:      # behind the optimizer, before the EMA: the shadows average the clamped weights
            self.last_weight_norms = RG.ensure_state(self.last_weight_norms, st)
            self.last_weight_norms.apply(st, self.max_weight_norm)
        if self.ema is not None:
            self.ema.update(st)     # same stream, outside a captured graph like the optimizer launches

    def weight_norm_stats(self):
        """(keys_scaled, mean norm, max norm) of the last optimizer step's max-norm launch (max_weight_norm given); synchronises.
        None before the first step and without max_weight_norm."""
        return None if self.last_weight_norms is None else self.last_weight_norms.stats()

    def adapter_spectrum(self, **kw):
        """qflux_amd.spectrum.adapter_spectrum of the model: {module name: the singular values of scaling * B @ A}.  One launch on
        the current stream OUTSIDE the captured step graph and one device-to-host copy; its buffers are allocated on the first
        call and kept for the store layout (FluxKontextTrainStep inherits it)."""
        from .. import spectrum as SP
        self._spectrum_state = SP.ensure_state(getattr(self, "_spectrum_state", None), self.dit)
        return SP.adapter_spectrum(self.dit, state=self._spectrum_state, **kw)

    @property
    def last_adapter_stats(self):
        """{adapter tensor name: {grad_norm, weight_norm, update_norm, update_ratio, grad_absmax, grad_nonfinite, weight_nonfinite}}
        of the last step that collected (adapter_stats_every), keyed as save_lora_weights keys the tensors; reads on access (one
        device-to-host copy, the only synchronisation of the feature).  None before the first collected step and with the option off."""
        return None if self._adapter_stats is None else self._adapter_stats.read()

    def adapter_stats_summary(self):
        """telemetry.summarize of the last collected step: the global gradient norm, the maximum and median update ratio over the
        lora_A and over the lora_B tensors, the first tensor with a non-finite gradient.  None where last_adapter_stats is."""
        return None if self._adapter_stats is None else self._adapter_stats.summary()

    @property
    def _m(self):
        """AdamW's / Prodigy's fp32 exp_avg over the flat buffer (read-only; None before the first step and for the 8-bit state)."""
        return getattr(self.opt_state, "m", None)

    @property
    def _v(self):
        """exp_avg_sq, as _m."""
        return getattr(self.opt_state, "v", None)

    def _mark_unexchanged(self):
        dp = getattr(self.dit, "_dp", None)
        if dp is not None:
            dp.exchanged = False

    def zero_grad(self):
        self.dit.lora_store.gflat.zero_()
        self._mark_unexchanged()

    # ------------------------------------------------------------------ optimizer / resume state (base_trainer.py:827-875,944-1002)
    def state_dict(self):
        """{"state": {i: per-parameter state}, "param_groups": [...]} with one entry per LoRA parameter in named_parameters() order
        (what accelerate's optimizer.bin holds for the reference), in the optimizer's own layout: torch.optim.AdamW's, prodigyopt's
        or bitsandbytes' (optim_state)."""
        st = self.dit.lora_store
        rows, members = self.param_groups_of(st)
        sd = OS.state_dict(self._opt_cls, self.opt_state, st, self.global_step, self.optimizer_args, self.lr, self.betas,
                           self.eps, self.weight_decay, groups=self._scheduled_rows(rows, initial=True), members=members)
        drop = getattr(self.dit, "_dropout", None)
        if drop is not None:      # only while the feature is on: no new key otherwise
            sd[DR.STATE_KEY] = drop.state_dict()
        return sd

    def load_state_dict(self, sd):
        """With param_groups the file must hold the same groups (torch's ValueError otherwise): every group takes the file's betas,
        eps and weight_decay, and its lr as the unscheduled one -- the file's "initial_lr" where it has one (the schedule's factor
        lr / initial_lr then comes back into self.lr), else its lr (factor 1)."""
        st = self.dit.lora_store
        if DR.STATE_KEY in sd:      # seed, probabilities and the count of training forwards: the masks continue where the file left
            d = sd[DR.STATE_KEY]
            sd = {k: v for k, v in sd.items() if k != DR.STATE_KEY}
            drop = self.dit.set_lora_dropout(d["network_dropout"], d["rank_dropout"], d["seed"])
            if drop is not None:
                drop.set_step(d["step"])
        rows, members = self.param_groups_of(st)
        hyper = dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)
        file_rows = None if rows is None else [dict(r, initial_lr=None) for r in rows]
        self.opt_state, self.global_step = OS.load_state_dict(self._opt_cls, st, sd, self.optimizer_args, hyper, groups=file_rows,
                                                              members=members)
        if rows is None:
            self.lr, self.betas, self.eps, self.weight_decay = hyper["lr"], hyper["betas"], hyper["eps"], hyper["weight_decay"]
            return
        for r, f in zip(rows, file_rows):
            r.update(betas=f["betas"], eps=f["eps"], weight_decay=f["weight_decay"], lr=f["initial_lr"] if f["initial_lr"] else f["lr"])
        f = file_rows[0]
        self.lr = self._base_lr * (f["lr"] / f["initial_lr"]) if f["initial_lr"] and f["lr"] != f["initial_lr"] else self._base_lr

    def save_checkpoint(self, save_dir, extra_state=None):
        """checkpoint-<e>-<step> folder of the reference (base_trainer.py:827-875): pytorch_lora_weights.safetensors (diffusers
        key style) + optimizer.bin + state.json.  With a schedule-free optimizer the weights file holds the averaged x (what an
        inference pipeline must load): the weights are swapped to eval for it and back, and optimizer.bin is written after that, in
        the mode the step was in.  The round trip y -> x -> y rounds (the package's own does); the run goes on from the
        swapped-back y, and so does a run resumed from the folder.
        With ema_decay the weights file holds the trained weights (resume is exact), pytorch_lora_weights_ema.safetensors holds
        shadow 0 and _ema1 ... the others, each written by the same writer with the shadow swapped in (any LoRA loader reads them),
        and ema.bin is torch.save of EmaState.state_dict(); the step ends in the form it was in.
        After a PiSSA initialisation state.json also carries "pissa": its (niter, oversample, seed) -- the residual trunk itself
        is not stored, load_checkpoint rebuilds it bit for bit from the original weights."""
        import json
        os.makedirs(save_dir, exist_ok=True)
        pissa = getattr(self.dit, "_pissa", None)
        if pissa is not None:
            extra_state = dict(extra_state or {}, pissa={k: pissa[k] for k in ("niter", "oversample", "seed")})
        if self.ema_decays is not None:
            self._save_ema(save_dir)
        else:
            with self.eval_mode():
                self.dit.save_lora_weights(save_dir)
        torch.save(self.state_dict(), os.path.join(save_dir, "optimizer.bin"))
        with open(os.path.join(save_dir, "state.json"), "w") as f:
            json.dump(dict({"global_step": self.global_step, "lr": self.lr}, **(extra_state or {})), f, indent=2)

    def _save_ema(self, save_dir):
        from ..lora_io import WEIGHT_NAME
        st, ema = self.dit.lora_store, self._ensure_ema()
        was = ema.active
        stem, ext = os.path.splitext(WEIGHT_NAME)
        for k in range(len(ema.shadows)):
            ema.swap_in(st, k)
            os.replace(self.dit.save_lora_weights(save_dir), os.path.join(save_dir, f"{stem}_ema{k or ''}{ext}"))
        ema.swap_out(st)
        self.dit.save_lora_weights(save_dir)
        torch.save(ema.state_dict(st), os.path.join(save_dir, "ema.bin"))
        if was is not None:
            ema.swap_in(st, was)

    def _load_ema(self, save_dir):
        """Fresh shadows from the weights now in place, then ema.bin's over them where the folder has one."""
        import warnings
        self.ema = None
        ema, path = self._ensure_ema(), os.path.join(save_dir, "ema.bin")
        if os.path.exists(path):
            ema.load_state_dict(self.dit.lora_store, torch.load(path, map_location="cpu", weights_only=False))
            self.ema_decays, self.ema_args = ema.decays, ema.args      # the file's settings, as load_state_dict takes the optimizer's
        else:
            warnings.warn(f"{save_dir} has no ema.bin: the EMA shadows start as copies of the loaded weights, with no update counted")

    def load_checkpoint(self, save_dir, adapter_name=None):
        """adapter_name: inject/overwrite that adapter from the saved weights first (None = the adapter is already in place).
        Schedule-free: the step ends in train mode.  Weights read from the folder are the averaged x whatever optimizer.bin says
        (save_checkpoint writes them in eval mode); weights already in place are x when the file says train_mode=False.  Either
        way y is reconstructed from x and the file's z with train()'s lerp -- the same launch on the same bits as the swap back in
        save_checkpoint, so the resumed run continues like the run that wrote the folder.
        A folder written after a PiSSA initialisation names its (niter, oversample, seed): a model that still holds the ORIGINAL
        weights is initialised with them first (the same residual trunk, bit for bit), then the trained A, B are loaded over
        A0, B0 -- so such a folder needs adapter_name, and a model whose adapters exist with the run's rank and lora_alpha."""
        import json
        with open(os.path.join(save_dir, "state.json")) as f:
            pissa = json.load(f).get("pissa")
        if pissa is not None:
            have = getattr(self.dit, "_pissa", None)
            if have is None:
                if adapter_name is None:
                    raise ValueError(f"{save_dir} was trained from a PiSSA initialisation {pissa}: pass adapter_name, so that the trained "
                                     "weights are loaded after the residual trunk has been rebuilt")
                self.dit.pissa_init_(**pissa)
            elif any(have[k] != pissa[k] for k in pissa):
                raise ValueError(f"{save_dir} was trained from the PiSSA initialisation {pissa}, the model holds another one")
        if adapter_name is not None:
            self.dit.load_lora_adapter(save_dir, adapter_name=adapter_name)
        self.load_state_dict(torch.load(os.path.join(save_dir, "optimizer.bin"), map_location="cpu", weights_only=False))
        if self.optimizer == "adamw_schedulefree" and self.opt_state is not None:
            if adapter_name is not None:
                self.opt_state.train_mode = False
            self.train()
        if self.ema_decays is not None:      # an ema.bin in the folder is ignored without ema_decay
            self._load_ema(save_dir)
        self.broadcast_state()       # every replica continues from rank 0's copy of the checkpoint
        with open(os.path.join(save_dir, "state.json")) as f:
            return json.load(f)

    # ------------------------------------------------------------------ replica consistency (main.py:58, base_trainer.py:384-393)
    def _state_buffers(self):
        """Every flat buffer that must be identical on all ranks: adapter weights, then the optimizer state's (None where this rank
        has no state: the list has the same length on every rank), then the EMA shadows ema0 ... when ema_decay is given."""
        opt = self.opt_state.buffers() if self.opt_state is not None else [(n, None) for n in self._opt_cls.names(self.optimizer_args)]
        ema = []
        if self.ema_decays is not None:
            ema = self.ema.buffers() if self.ema is not None else [(n, None) for n in E.EmaState.names(self.ema_decays)]
        return [("lora", self.dit.lora_store.pflat)] + opt + ema

    def broadcast_state(self, src: int = 0):
        """Rank `src`'s adapter weights (+ optimizer state, + step count) to every rank: what DDP's constructor does for the
        reference's LoRA container (base_trainer.py:384-393; the reference otherwise relies on equal seeds, main.py:58).  Called
        once before the first step and after load_checkpoint / load_lora_adapter: a resumed or re-injected adapter set must not
        depend on every rank having read identical files.  Whether rank `src` has optimizer state, its step count and the layout
        ints of its state (optim_state LAYOUT_ARGS) are agreed on first."""
        if self.world <= 1:
            return
        st, cls = self.dit.lora_store, self._opt_cls
        head = torch.tensor([int(self.opt_state is not None), self.global_step] + [int(self.optimizer_args[n]) for n in cls.LAYOUT_ARGS] +
                            ([self._ensure_ema().optimization_step] if self.ema_decays is not None else []),
                            dtype=torch.int64, device=st.pflat.device)
        dist.broadcast(head, src=src, group=self.group)
        have, self.global_step, *ints = head.tolist()
        if self.ema_decays is not None:      # the shadows exist on every rank from here on and travel with the buffers below
            self.ema.optimization_step = ints.pop()
        # the buffer list is derived from the AGREED header on every rank (same collectives in the same order everywhere): state
        # rank `src` has is created where missing, state it lacks is dropped locally (a rank that had stepped before must not carry
        # moments the others do not have)
        if have:
            self.optimizer_args.update(zip(cls.LAYOUT_ARGS, ints))
            self.opt_state = OS.ensure_state(cls, self.opt_state, st, self.optimizer_args, self.param_groups_of(st)[1])
        else:
            self.opt_state = None
        for _, t in self._state_buffers():
            if t is not None:
                dist.broadcast(t, src=src, group=self.group)
        if self.opt_state is not None:
            self.opt_state.sync_host()

    def check_replicas(self, what: str = "adapter weights"):
        """Raises if the adapter weights (and optimizer buffers) differ between ranks: two order-sensitive fp64 checksums per
        buffer, gathered and compared on every rank.  Cheap (one small all-gather); call it after loading state and periodically."""
        return self.world <= 1 or check_replicas(self._state_buffers(), self.world, self.group, what)

    def train_step(self, embeddings, noise=None, u=None, micro_batches=None):
        """One full optimisation step; returns the (device) loss.  micro_batches: optional list of further embedding dicts
        accumulated before the step (gradient_accumulation_steps = 1 + len(micro_batches); mean over micro-steps)."""
        extra = list(micro_batches or [])
        k = 1 + len(extra)
        loss = self.forward_backward(embeddings, noise, u, sync=not extra)
        for j, mb in enumerate(extra):
            loss = loss + self.forward_backward(mb, sync=(j == len(extra) - 1))
        scale = self.allreduce_grads() / k
        self.optimizer_step(grad_scale=scale)
        self.zero_grad()
        return loss / k if k > 1 else loss

    def gather_loss(self, loss):
        """accelerator.gather(loss).mean() (base_trainer.py:539)."""
        if self.world > 1:
            out = [torch.zeros_like(loss) for _ in range(self.world)]
            dist.all_gather(out, loss, group=self.group)
            return torch.stack(out).mean()
        return loss
