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
"""
from __future__ import annotations

import contextlib
import os

import torch
import torch.distributed as dist

from .. import ops
from . import adam8bit as A8
from . import optim_state as OS
from .optim_state import resolve_family

BF = torch.bfloat16


def flowmatch_tables(num_train_timesteps: int = 1000, shift: float = 1.0):
    """FlowMatchEulerDiscreteScheduler.timesteps / .sigmas as built at construction (third-party lookup
    tables, qwen_image_edit_trainer.py:807-810,851-861; dynamic shifting => identity shift at init)."""
    ts = torch.linspace(1, num_train_timesteps, num_train_timesteps).flip(0)
    sig = ts / num_train_timesteps
    sig = shift * sig / (1 + (shift - 1) * sig)
    return sig * num_train_timesteps, sig


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
                 bucket_mb=24.0, optimizer="adamw", optimizer_args=None):
        """optimizer: "adamw" (torch.optim.AdamW semantics, lr/betas/eps/weight_decay above) or "prodigy" (prodigyopt.Prodigy, the
        reference's parameter-free choice: configs/face_seg_flux_kontext_fp16_prodigy.yaml:41-47); optimizer_args = the extra
        init_args of that class (use_bias_correction, safeguard_warmup, beta3, decouple, d0, d_coef, growth_rate).  With Prodigy
        `lr` is the schedule multiplier the reference sets to 1.0.
        "adam8bit_blockwise" / "adamw8bit_blockwise": bitsandbytes.optim.Adam8bit / AdamW8bit with their blockwise 8-bit moments and
        state layout (trainer/adam8bit.py; weight decay decoupled, defaults 0 / 1e-2); optimizer_args: min_8bit_size (4096), blocksize
        (256 or 2048).
        "sgd": torch.optim.SGD, the fourth optimizer the reference documents (docs/guide/training.md:768-826: momentum 0.9, weight_decay
        1e-4; weight decay in the L2 form, default 0); optimizer_args: momentum (0), dampening (0), nesterov (False); betas / eps unused.
        "adafactor": transformers.optimization.Adafactor (factored second moments per adapter matrix, update clipping; weight decay
        scaled by the step's learning rate, default 0); optimizer_args: eps ((1e-30, 1e-3)), clip_threshold (1.0), decay_rate (-0.8),
        beta1 (None), scale_parameter (True), relative_step (True), warmup_init (False).  lr must be None with relative_step (the
        default) and a float without it; betas / eps unused.
        "lion": lion_pytorch.Lion / bitsandbytes.optim.Lion (one fp32 moment, the update is lr times the sign of the interpolated
        moment; weight decay decoupled, before the update, default 0); no optimizer_args; eps unused.  "lion8bit_blockwise":
        bitsandbytes.optim.Lion8bit / PagedLion8bit with the moment in blockwise 8-bit codes and bnb's one-state layout;
        optimizer_args: min_8bit_size (4096), blocksize (256 or 2048).
        "muon": torch.optim.Muon (per adapter matrix: Nesterov momentum, then five Newton-Schulz iterations in bf16 on the matrix
        units orthogonalise the update; weight decay decoupled, default the class's 0.1); optimizer_args: momentum (0.95), nesterov
        (True), ns_coefficients ((3.4445, -4.7750, 2.0315)), ns_steps (5), adjust_lr_fn (None = "original", or "match_rms_adamw") and
        eps (1e-7: Muon's own, the floor of the update's norm, not this constructor's Adam eps); betas / eps unused.
        "adamw_schedulefree": schedulefree.AdamWScheduleFree (Defazio et al. 2024: Adam's second moment, no first moment and no
        schedule -- the gradient is taken at y, an interpolation between the base sequence z and the running average x; made for a
        constant lr; weight decay in the L2 form on y, default 0; the package's lr is 0.0025); optimizer_args: warmup_steps (0: the
        optimizer's own linear warm-up), r (0.0) and weight_lr_power (2.0): the averaging weight of step k is (k + 1)^r lr_max^power.
        The adapter weights hold y while training: eval() / train() / eval_mode() swap them to x and back, save_checkpoint writes x,
        and the samplers take train_step= to sample from x.
        betas=None (the default) means the optimizer class's own default: (0.9, 0.99) for the two Lion families, (0.9, 0.999) --
        torch.optim.AdamW's, this constructor's default before Lion -- for every other one; betas given explicitly are never
        reinterpreted.
        criterion: "mse" = MseLoss (losses/mse_loss.py:46-83); "mask_edit" = MaskEditLoss(forground_weight,
        background_weight) (losses/edit_mask_loss.py:39-90), fed by embeddings["edit_mask"] [B,S_t] (all-ones when absent)."""
        if criterion not in ("mse", "mask_edit"):
            raise ValueError(f"unknown criterion {criterion!r}")
        self.optimizer_alias, self.optimizer, self._opt_cls, weight_decay, self.optimizer_args = resolve_family(optimizer, weight_decay,
                                                                                                                optimizer_args)
        if self.optimizer == "adafactor":
            self._opt_cls.validate(self.optimizer_args, lr)
        self.blockwise = optimizer in A8.BLOCKWISE
        self.opt_state = None       # the family's optim_state object, from the first step or load_state_dict on
        self.criterion, self.fg, self.bg = criterion, float(forground_weight), float(background_weight)
        self.dit = dit
        betas = OS.default_betas(self.optimizer) if betas is None else tuple(betas)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.max_grad_norm = max_grad_norm
        self.weight_dtype = weight_dtype
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_available() and dist.is_initialized() else 1
        self.timesteps_tbl, self.sigmas_tbl = flowmatch_tables()
        # frozen conditioning head: the AdaLN modulation vectors of every training timestep, computed once here so that no step pays
        # for it (dit.ensure_modulation_table; QFX_MOD_TABLE=0 / QFX_MOD_TABLE_GB; nothing happens with adapters on the head)
        if getattr(dit, "_MOD_TABLE", False):
            dit.set_modulation_keys(self.timesteps_tbl / 1000)
            dit.ensure_modulation_table()
        self.global_step = 0
        self._gnorm = self._gparts = None
        # data-parallel exchange overlapped with the backward: the flat gradient is all-reduced in buckets of whole DiT
        # blocks as soon as their backward segment has been enqueued (the gradient of block i is final when its segment ends)
        self.bucket_bytes = int(bucket_mb * (1 << 20))
        self._pending = []
        self._finish_buckets = None
        self._reduced = False
        self._synced = False      # rank 0's adapter / optimizer state is broadcast before the first step (broadcast_state)
        self._synced_version = None
        # QFX_DP_FORCE=1: run the bucketed exchange on a ONE-rank process group too (the collectives are then identities) -- lets a
        # one-GPU box execute the real RCCL code path: communicator, RCCL's stream, async handles, ordering against the main and
        # the side gradient stream (tests/test_dp_gpu.py)
        self._force_dp = os.environ.get("QFX_DP_FORCE", "0") == "1" and dist.is_available() and dist.is_initialized()

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
        if u is None:
            u = torch.rand(size=(batch_size,), device="cpu")  # compute_density_for_timestep_sampling("none")
        idx = (u * 1000).long()
        return self.timesteps_tbl[idx], self.sigmas_tbl[idx]

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
        el = (pred.float() - target.float()) ** 2            # MseLoss with weighting = 1 (mse_loss.py:71-81)
        if self.criterion == "mask_edit":                      # MaskEditLoss, reduction="mean" (edit_mask_loss.py:62-86)
            el = el * self._token_weights(embeddings, target.shape[0], S_t, el.device).unsqueeze(-1)
        return torch.mean(el.reshape(target.shape[0], -1), dim=1).mean()

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
        weights (embeddings["edit_mask"]).  sync: the bucketed gradient exchange runs behind the backward."""
        self.dit.lora_store  # make sure the flat buffers / grads are attached
        self._ensure_synced()
        pred = plan.run_forward(inputs, pe, t)
        if tok_w is None and self.criterion == "mask_edit":
            B = target.shape[0]
            tok_w, inv_denom = self._token_weights(embeddings, B, n_tok, pred.device), 1.0 / (B * n_tok)
        if tok_w is None:
            loss, dpred = ops.mse_loss_fwd_bwd(pred, target, n_tok, gscale=grad_scale)
        else:
            loss, dpred = ops.mse_token_weighted_fwd_bwd(pred, target, tok_w, n_tok, inv_denom, gscale=grad_scale)
        self._mark_unexchanged()       # local gradients are added below: whatever exchange a drop-in backward did before is stale
        plan.run_backward(dpred, on_segment=self._bucket_hook() if ((self.world > 1 or self._force_dp) and sync) else None)
        return loss

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

        def body():
            pred = plan.run_forward(static[0], static[2], static[3])
            loss, dpred = ops.mse_loss_fwd_bwd(pred, static[1], S_t)
            plan.run_backward(dpred)
            return loss

        warm = torch.cuda.Stream(device=dit.device)     # one eager pass on a non-default stream (lazy module loads, pool warm-up)
        warm.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(warm):
            body()
        torch.cuda.current_stream().wait_stream(warm)
        self.zero_grad()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss_static = body()
        self.zero_grad()
        shapes = [tuple(t.shape) for t in static]

        def step(emb, noise=None, u=None):
            if dit._version != version or not any(p is plan for p in dit._plans.values()):
                raise RuntimeError("capture_graph: the plan this graph was captured on is gone (adapters / quantisation changed "
                                   "or it was evicted); capture again")
            ins = self._prepare(emb, noise, u)
            if [tuple(t.shape) for t in ins[:4]] != shapes:
                raise ValueError("capture_graph: batch shape differs from the captured one")
            for d, s_ in zip(static, ins[:4]):
                d.copy_(s_)
            self._ensure_synced()
            self._mark_unexchanged()
            graph.replay()
            self._finish_buckets = None
            self.optimizer_step(grad_scale=self.allreduce_grads())
            self.zero_grad()
            return loss_static.clone()      # the graph overwrites loss_static on every replay

        step.graph = graph
        return step

    # ------------------------------------------------------------------ bucketed all-reduce behind the backward
    def _bucket_hook(self):
        st = self.dit.lora_store
        ents = st.entries
        todo = set(range(len(ents)))
        acc = []          # entry indices final but not yet reduced
        self._pending, self._reduced = [], False

        def flush(force=False):
            nbytes = sum(((ents[i][3] + 63) // 64 * 64) * 4 for i in acc)
            if not acc or (not force and nbytes < self.bucket_bytes):
                return
            for lo, hi in _contiguous_runs(sorted(acc), ents):
                self._pending.append(dist.all_reduce(st.gflat[lo:hi], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
            acc.clear()

        # adapters of the conditioning head (AdaLN modulation linears img_mod.1 / txt_mod.1, FLUX norm*.linear, the embedders) live
        # under the block prefixes too, but their gradients are written by the LAST call of the backward program (the head's own
        # backward, fed by the d(modulation) column sums of every block): they are never final at a block mark and go out with
        # finish(), after the whole program
        cond_sfx = tuple(getattr(self.dit, "_COND_SUFFIXES", ()))
        late = {i for i in todo if cond_sfx and ents[i][0].split(".lora_")[0].endswith(cond_sfx)}

        def hook(prefix):
            done = [i for i in todo if i not in late and ents[i][0].startswith(prefix)]
            todo.difference_update(done)
            acc.extend(done)
            flush()

        def finish():
            acc.extend(sorted(todo))   # adapters outside the marked blocks, if any
            todo.clear()
            flush(force=True)

        self._finish_buckets = finish
        return hook

    def allreduce_grads(self):
        """Returns the factor the optimizer applies to the summed gradient (1/world)."""
        if self.world > 1 or self._force_dp:
            fin = self._finish_buckets
            if fin is not None:
                fin()
                self._finish_buckets = None
                for w in self._pending:
                    w.wait()
                self._pending = []
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

    def _ensure_opt_state(self):
        st = self.dit.lora_store
        if self.opt_state is None or self.opt_state.key != self._opt_cls.layout_key(st, self.optimizer_args):
            self.opt_state = self._opt_cls(st, self.optimizer_args)      # zeroed state of the current layout
        return st

    # ------------------------------------------------------------------ train / eval form of the adapter weights
    @property
    def train_mode(self):
        """False while the adapter weights hold the averaged point x of a schedule-free optimizer (eval()); True otherwise, always
        for every other family."""
        return self.opt_state is None or self.opt_state.train_mode

    def _swap(self, train):
        if self.optimizer == "adamw_schedulefree":
            self._ensure_opt_state()
            self.opt_state.swap(self.dit.lora_store, self.betas[0], train)

    def eval(self):
        """optimizer="adamw_schedulefree": the adapter weights (lora_store.pflat, which every plan reads its LoRA operands from at
        each pass: no plan is rebuilt) go from y to the averaged x that is sampled from and saved -- the package's optimizer.eval().
        Nothing happens in eval mode already, and for every other family."""
        self._swap(False)

    def train(self):
        """Back from x to y (the package's optimizer.train()); nothing happens in train mode already, and for every other family."""
        self._swap(True)

    @contextlib.contextmanager
    def eval_mode(self):
        """`with step.eval_mode():` -- eval() on entry, train() on exit if the step was in train mode before."""
        was = self.train_mode
        self.eval()
        try:
            yield self
        finally:
            if was:
                self.train()

    def optimizer_step(self, grad_scale=1.0):
        if not self.train_mode:
            raise RuntimeError(self.opt_state.EVAL_STEP)
        st = self._ensure_opt_state()
        self.global_step += 1
        if self._gnorm is None or self._gnorm.device != st.pflat.device:
            self._gnorm = torch.zeros((), dtype=torch.float32, device=st.pflat.device)
            self._gparts = torch.zeros(1024, dtype=torch.float32, device=st.pflat.device)
        ops.sumsq_det(st.gflat, self._gnorm, self._gparts)     # fixed reduction order: every replica computes the same clip coefficient
        self.opt_state.step(st, self.lr, self.betas, self.eps, self.weight_decay, self.global_step, self._gnorm, self.max_grad_norm,
                            grad_scale, self.optimizer_args)

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
        return OS.state_dict(self._opt_cls, self.opt_state, self.dit.lora_store, self.global_step, self.optimizer_args, self.lr, self.betas,
                             self.eps, self.weight_decay)

    def load_state_dict(self, sd):
        hyper = dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)
        self.opt_state, self.global_step = OS.load_state_dict(self._opt_cls, self.dit.lora_store, sd, self.optimizer_args, hyper)
        self.lr, self.betas, self.eps, self.weight_decay = hyper["lr"], hyper["betas"], hyper["eps"], hyper["weight_decay"]

    def save_checkpoint(self, save_dir, extra_state=None):
        """checkpoint-<e>-<step> folder of the reference (base_trainer.py:827-875): pytorch_lora_weights.safetensors (diffusers
        key style) + optimizer.bin + state.json.  With a schedule-free optimizer the weights file holds the averaged x (what an
        inference pipeline must load): the weights are swapped to eval for it and back, and optimizer.bin is written after that, in
        the mode the step was in.  The round trip y -> x -> y rounds (the package's own does); the run goes on from the
        swapped-back y, and so does a run resumed from the folder."""
        import json
        os.makedirs(save_dir, exist_ok=True)
        with self.eval_mode():
            self.dit.save_lora_weights(save_dir)
        torch.save(self.state_dict(), os.path.join(save_dir, "optimizer.bin"))
        with open(os.path.join(save_dir, "state.json"), "w") as f:
            json.dump(dict({"global_step": self.global_step, "lr": self.lr}, **(extra_state or {})), f, indent=2)

    def load_checkpoint(self, save_dir, adapter_name=None):
        """adapter_name: inject/overwrite that adapter from the saved weights first (None = the adapter is already in place).
        Schedule-free: the step ends in train mode.  Weights read from the folder are the averaged x whatever optimizer.bin says
        (save_checkpoint writes them in eval mode); weights already in place are x when the file says train_mode=False.  Either
        way y is reconstructed from x and the file's z with train()'s lerp -- the same launch on the same bits as the swap back in
        save_checkpoint, so the resumed run continues like the run that wrote the folder."""
        import json
        if adapter_name is not None:
            self.dit.load_lora_adapter(save_dir, adapter_name=adapter_name)
        self.load_state_dict(torch.load(os.path.join(save_dir, "optimizer.bin"), map_location="cpu", weights_only=False))
        if self.optimizer == "adamw_schedulefree" and self.opt_state is not None:
            if adapter_name is not None:
                self.opt_state.train_mode = False
            self.train()
        self.broadcast_state()       # every replica continues from rank 0's copy of the checkpoint
        with open(os.path.join(save_dir, "state.json")) as f:
            return json.load(f)

    # ------------------------------------------------------------------ replica consistency (main.py:58, base_trainer.py:384-393)
    def _state_buffers(self):
        """Every flat buffer that must be identical on all ranks: adapter weights, then the optimizer state's (None where this rank
        has no state: the list has the same length on every rank)."""
        opt = self.opt_state.buffers() if self.opt_state is not None else [(n, None) for n in self._opt_cls.names(self.optimizer_args)]
        return [("lora", self.dit.lora_store.pflat)] + opt

    def broadcast_state(self, src: int = 0):
        """Rank `src`'s adapter weights (+ optimizer state, + step count) to every rank: what DDP's constructor does for the
        reference's LoRA container (base_trainer.py:384-393; the reference otherwise relies on equal seeds, main.py:58).  Called
        once before the first step and after load_checkpoint / load_lora_adapter: a resumed or re-injected adapter set must not
        depend on every rank having read identical files.  Whether rank `src` has optimizer state, its step count and the layout
        ints of its state (optim_state LAYOUT_ARGS) are agreed on first."""
        if self.world <= 1:
            return
        st, cls = self.dit.lora_store, self._opt_cls
        head = torch.tensor([int(self.opt_state is not None), self.global_step] + [int(self.optimizer_args[n]) for n in cls.LAYOUT_ARGS],
                            dtype=torch.int64, device=st.pflat.device)
        dist.broadcast(head, src=src, group=self.group)
        have, self.global_step, *ints = head.tolist()
        # the buffer list is derived from the AGREED header on every rank (same collectives in the same order everywhere): state
        # rank `src` has is created where missing, state it lacks is dropped locally (a rank that had stepped before must not carry
        # moments the others do not have)
        if have:
            self.optimizer_args.update(zip(cls.LAYOUT_ARGS, ints))
            if self.opt_state is None or self.opt_state.key != cls.layout_key(st, self.optimizer_args):
                self.opt_state = cls(st, self.optimizer_args)
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
        if self.world <= 1:
            return True
        dev = self.dit.lora_store.pflat.device
        sums = []
        for _, t in self._state_buffers():      # fixed layout: a buffer a rank lacks is part of the verdict
            if t is None:
                sums += [torch.zeros((), dtype=torch.float64, device=dev)] * 3
                continue
            d = t.detach().double().flatten()
            w = torch.arange(1, d.numel() + 1, device=d.device, dtype=torch.float64) % 8191
            sums += [torch.ones((), dtype=torch.float64, device=dev), d.sum(), (d * w).sum()]
        mine = torch.stack(sums)
        out = [torch.zeros_like(mine) for _ in range(self.world)]
        dist.all_gather(out, mine, group=self.group)
        for r, o in enumerate(out):
            if not torch.equal(o, out[0]):
                raise RuntimeError(f"data-parallel replicas diverged ({what}): rank {r} differs from rank 0 "
                                   f"(checksums {o.tolist()} vs {out[0].tolist()}); call broadcast_state() after loading state")
        return True

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


# qflux_amd.optim class -> (the class it stands in for, the state_bits it implies)
_OWN_CLASSES = {"qflux_amd.optim.AdamW": ("torch.optim.AdamW", 32), "qflux_amd.optim.Adam": ("torch.optim.Adam", 32),
                "qflux_amd.optim.Adam8bit": ("bitsandbytes.optim.Adam8bit", 8), "qflux_amd.optim.AdamW8bit": ("bitsandbytes.optim.AdamW8bit", 8),
                "qflux_amd.optim.Prodigy": ("prodigyopt.Prodigy", 0), "qflux_amd.optim.SGD": ("qflux_amd.optim.SGD", 0),
                "qflux_amd.optim.Adafactor": ("transformers.optimization.Adafactor", 0),
                "qflux_amd.optim.Muon": ("torch.optim.Muon", 0),
                "qflux_amd.optim.AdamWScheduleFree": ("schedulefree.AdamWScheduleFree", 0),
                "qflux_amd.optim.Lion8bit": ("bitsandbytes.optim.Lion8bit", 8),
                "qflux_amd.optim.PagedLion8bit": ("bitsandbytes.optim.PagedLion8bit", 8)}
_ADAFACTOR = ("transformers.optimization.Adafactor", "transformers.Adafactor")
_MUON = ("torch.optim.Muon",)
_SCHEDULEFREE = ("schedulefree.AdamWScheduleFree",)
_LION = ("lion_pytorch.Lion", "bitsandbytes.optim.Lion", "bitsandbytes.optim.Lion32bit")
_BNB_LION_8BIT = ("bitsandbytes.optim.Lion8bit", "bitsandbytes.optim.PagedLion8bit")
_BNB_8BIT = ("bitsandbytes.optim.Adam8bit", "bitsandbytes.optim.PagedAdam8bit", "bitsandbytes.optim.AdamW8bit",
             "bitsandbytes.optim.PagedAdamW8bit")


def optimizer_kwargs_from_config(class_path: str, init_args: dict | None = None, state_bits: int = 32) -> dict:
    """The reference's YAML `optimizer: {class_path, init_args}` (BaseTrainer.configure_optimizers, base_trainer.py:884-909) ->
    keyword arguments of QwenLoraTrainStep / FluxKontextTrainStep.
        torch.optim.AdamW                      -> optimizer="adamw"   (lr, betas, eps, weight_decay)
        bitsandbytes.optim.Adam8bit / Adam     -> optimizer="adam8bit": Adam with FP32 moments (see __init__; 8-bit states buy nothing
        bitsandbytes.optim.AdamW8bit / AdamW   -> optimizer="adamw"     next to 288 GB of HBM)
        prodigyopt.Prodigy                     -> optimizer="prodigy" + optimizer_args
    state_bits=8 maps the four 8-bit bnb classes (Adam8bit, PagedAdam8bit, AdamW8bit, PagedAdamW8bit) to the blockwise 8-bit optimizer
    with bnb's state layout instead: "adam8bit_blockwise" (weight decay default 0) / "adamw8bit_blockwise" (default 1e-2), min_8bit_size
    honoured; percentile_clipping != 100, max_unorm != 0, block_wise=False, skip_zeros=True and amsgrad=True are refused; is_paged only
    moves memory (same math).  state_bits=32 is the mapping above.
    The torch.optim classes of qflux_amd.optim (the drop-in loop's optimizers) map to the family each of them runs, whatever state_bits
    says: AdamW -> "adamw", Adam -> "adam", Adam8bit / AdamW8bit -> "adam8bit_blockwise" / "adamw8bit_blockwise" (the class is named for
    its state), Prodigy -> "prodigy", SGD -> "sgd" + optimizer_args (momentum, dampening, nesterov; maximize is refused).
    torch.optim.SGD itself is not mapped.
        transformers.optimization.Adafactor / transformers.Adafactor / qflux_amd.optim.Adafactor -> optimizer="adafactor" + optimizer_args
    (eps pair, clip_threshold, decay_rate, beta1, scale_parameter, relative_step, warmup_init); lr is None with relative_step (the
    package's default) and the package's refusals apply: lr with relative_step, warmup_init without it, no lr without it.
        lion_pytorch.Lion / bitsandbytes.optim.Lion / Lion32bit -> optimizer="lion" (lr, betas, weight_decay;
    betas left out = the class's (0.9, 0.99), weight decay default 0); lion_pytorch's use_triton and decoupled_weight_decay=False are
    accepted (where the arithmetic runs; the plain decoupled form), decoupled_weight_decay=True and cautious_factor != 1 are refused.
        bitsandbytes.optim.Lion8bit / PagedLion8bit -> "lion" (fp32 moment) with state_bits=32, "lion8bit_blockwise" (bnb's one-state
    8-bit layout, min_8bit_size honoured) with state_bits=8 -- the Adam8bit rule, with the same init_args refused;
    qflux_amd.optim.Lion8bit / PagedLion8bit always map to the blockwise form.  The path qflux_amd.optim.Lion itself is NOT mapped
    here and keeps raising (tests/test_optim_classes_cpu.py pins that refusal): the class exists and steps "lion", a config for the
    fused train step names lion_pytorch.Lion, whose keywords it takes.
        torch.optim.Muon / qflux_amd.optim.Muon -> optimizer="muon" + optimizer_args (momentum, nesterov, ns_coefficients, eps,
    ns_steps, adjust_lr_fn); weight decay left out is the class's 0.1; ns_steps >= 100 and an unknown adjust_lr_fn are refused with
    torch's messages.
        schedulefree.AdamWScheduleFree / qflux_amd.optim.AdamWScheduleFree -> optimizer="adamw_schedulefree" + optimizer_args
    (warmup_steps, r, weight_lr_power); lr and weight decay left out are the class's 0.0025 and 0; foreach is dropped.  Keep the
    reference's lr_scheduler at `constant`: the warm-up is the optimizer's own warmup_steps.
    Unknown classes raise: silently training with a different optimizer is worse than stopping."""
    if state_bits not in (8, 32):
        raise ValueError(f"state_bits must be 8 or 32, not {state_bits!r}")
    a = dict(init_args or {})
    name = class_path.rsplit(".", 1)[-1]
    given = class_path
    if class_path in _OWN_CLASSES:
        class_path, bits = _OWN_CLASSES[class_path]
        state_bits = bits or state_bits
    out = {}
    if class_path in _ADAFACTOR:
        # lr may be None (relative_step) and eps is the package's pair: both are read here, the package's own refusals apply
        out["optimizer"] = "adafactor"
        if "betas" in a:
            raise NotImplementedError(f"unsupported optimizer init_args for {given}: ['betas']")
        lr = a.pop("lr", None)
        out["lr"] = None if lr is None else float(lr)
        out["optimizer_args"] = {k: a.pop(k) for k in list(a) if k in OS.AdafactorState.DEFAULTS}
        if "eps" in out["optimizer_args"]:
            out["optimizer_args"]["eps"] = tuple(float(e) for e in out["optimizer_args"]["eps"])
        OS.AdafactorState.validate(dict(OS.AdafactorState.DEFAULTS, **out["optimizer_args"]), out["lr"])
    if class_path in _MUON:
        # eps is Muon's own (the norm's floor), one of the family's optimizer_args next to the Newton-Schulz settings
        out["optimizer"] = "muon"
        if "betas" in a:
            raise NotImplementedError(f"unsupported optimizer init_args for {given}: ['betas']")
        out["optimizer_args"] = {k: a.pop(k) for k in list(a) if k in OS.MuonState.DEFAULTS}
        OS.MuonState.validate(dict(OS.MuonState.DEFAULTS, **out["optimizer_args"]))
        if "ns_coefficients" in out["optimizer_args"]:
            out["optimizer_args"]["ns_coefficients"] = tuple(float(c) for c in out["optimizer_args"]["ns_coefficients"])
    for k in ("lr", "eps", "weight_decay"):
        if k in a:
            out[k] = float(a.pop(k))
    if "betas" in a:
        out["betas"] = tuple(float(b) for b in a.pop("betas"))
    if state_bits == 8 and class_path in _BNB_8BIT + _BNB_LION_8BIT:
        adamw = "AdamW" in name
        out["optimizer"] = "lion8bit_blockwise" if class_path in _BNB_LION_8BIT else "adamw8bit_blockwise" if adamw else "adam8bit_blockwise"
        out.setdefault("weight_decay", 0.01 if adamw else 0.0)
        refused = {"percentile_clipping": (100, "percentile clipping"), "max_unorm": (0.0, "update-norm clipping (max_unorm)"),
                   "block_wise": (True, "non-blockwise 8-bit state"), "skip_zeros": (False, "skip_zeros"), "amsgrad": (False, "amsgrad")}
        for k, (ok, what) in refused.items():
            if k in a and a.pop(k) != ok:
                raise NotImplementedError(f"{given}: {what} is not implemented by the blockwise 8-bit step ({k} must be {ok!r})")
        if "min_8bit_size" in a:
            out["optimizer_args"] = {"min_8bit_size": int(a.pop("min_8bit_size"))}
        a.pop("is_paged", None)        # paged memory: where the state lives, not what is computed
        a.pop("optim_bits", None)      # the 8-bit classes pass 8 whatever this says
    elif class_path in ("torch.optim.AdamW", "bitsandbytes.optim.AdamW8bit", "bitsandbytes.optim.AdamW", "bitsandbytes.optim.PagedAdamW8bit"):
        out["optimizer"] = "adamw"
    elif class_path in ("torch.optim.Adam", "bitsandbytes.optim.Adam8bit", "bitsandbytes.optim.Adam", "bitsandbytes.optim.PagedAdam8bit"):
        out["optimizer"] = "adam8bit" if "8bit" in name else "adam"
        out.setdefault("weight_decay", 0.0)
    elif class_path in _LION + _BNB_LION_8BIT:
        out["optimizer"] = "lion"
        out.setdefault("weight_decay", 0.0)
        if a.pop("decoupled_weight_decay", False):
            raise NotImplementedError(f"{given}: decoupled_weight_decay=True (weight decay scaled by lr / the initial lr) is not implemented")
        if float(a.pop("cautious_factor", 1.0)) != 1.0:
            raise NotImplementedError(f"{given}: the cautious variant (cautious_factor != 1) is not implemented")
        a.pop("use_triton", None)      # where lion_pytorch runs the same arithmetic
    elif given == "qflux_amd.optim.SGD":
        out["optimizer"] = "sgd"
        if a.pop("maximize", False):
            raise NotImplementedError(f"{given}: maximize=True is not implemented")
        out["optimizer_args"] = {k: a.pop(k) for k in list(a) if k in ("momentum", "dampening", "nesterov")}
        a.pop("differentiable", None)
    elif class_path in _ADAFACTOR + _MUON:
        pass
    elif class_path in _SCHEDULEFREE:
        out["optimizer"] = "adamw_schedulefree"
        out.setdefault("lr", 0.0025)
        out.setdefault("weight_decay", 0.0)
        out["optimizer_args"] = {k: a.pop(k) for k in list(a) if k in OS.ScheduleFreeAdamWState.DEFAULTS}
        OS.ScheduleFreeAdamWState.validate(dict(OS.ScheduleFreeAdamWState.DEFAULTS, **out["optimizer_args"]))
    elif class_path == "prodigyopt.Prodigy":
        out["optimizer"] = "prodigy"
        out["optimizer_args"] = {k: a.pop(k) for k in list(a) if k in ("beta3", "decouple", "use_bias_correction", "safeguard_warmup", "d0",
                                                                       "d_coef", "growth_rate")}
    else:
        raise NotImplementedError(f"optimizer {class_path!r} has no fused counterpart (use the drop-in path with the torch optimizer)")
    for k in ("min_8bit_size", "percentile_clipping", "block_wise", "optim_bits", "is_paged", "amsgrad", "foreach", "fused"):
        a.pop(k, None)       # knobs of the 8-bit state / torch dispatch: no meaning for the fused fp32 step
    if a:
        raise NotImplementedError(f"unsupported optimizer init_args for {given}: {sorted(a)}")
    return out


def get_scheduler(name: str, num_warmup_steps: int = 0, num_training_steps: int | None = None, num_cycles: float = 0.5):
    """lr multiplier(step) of diffusers.optimization.get_scheduler for the schedules the reference's configs use
    (base_trainer.py:900-916): constant, constant_with_warmup, linear, cosine.  Use: step.lr = base_lr * f(global_step)."""
    import math

    def warm(s):
        return float(s) / float(max(1, num_warmup_steps)) if s < num_warmup_steps else None

    if name == "constant":
        return lambda s: 1.0
    if name == "constant_with_warmup":
        return lambda s: (warm(s) if warm(s) is not None else 1.0)
    if name == "linear":
        return lambda s: (warm(s) if warm(s) is not None else
                          max(0.0, float(num_training_steps - s) / float(max(1, num_training_steps - num_warmup_steps))))
    if name == "cosine":
        def f(s):
            w = warm(s)
            if w is not None:
                return w
            prog = float(s - num_warmup_steps) / float(max(1, num_training_steps - num_warmup_steps))
            return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * prog)))
        return f
    raise ValueError(f"unsupported lr scheduler {name!r}")


def _contiguous_runs(idx, ents):
    """Entry indices -> [lo, hi) element ranges of the flat buffer, merged where adjacent (64-element padded slots)."""
    runs = []
    for i in idx:
        lo = ents[i][2]
        hi = lo + (ents[i][3] + 63) // 64 * 64
        if runs and runs[-1][1] == lo:
            runs[-1][1] = hi
        else:
            runs.append([lo, hi])
    return [(a, b) for a, b in runs]


def init_distributed_from_env():
    """One process per GPU; backend "nccl" is RCCL on ROCm.  Returns (rank, local_rank, world).
    Test hooks: QFX_DIST_BACKEND=gloo and QFX_SHARE_GPU=1 let several ranks share device 0 (RCCL refuses duplicate devices), so
    the multi-rank code path can be exercised on a one-GPU box."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("QFX_SHARE_GPU") == "1":
        local = 0
    if torch.cuda.is_available():
        torch.cuda.set_device(local)   # before the process group: RCCL binds to the current device
    if (world > 1 or os.environ.get("QFX_BENCH_INIT_PG") == "1") and not dist.is_initialized():     # (one-rank group: tools/rccl_one_rank.py)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("QFX_DIST_BACKEND", "nccl" if torch.cuda.is_available() else "gloo")
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, local, world
