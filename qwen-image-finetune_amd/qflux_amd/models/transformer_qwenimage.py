"""MI355X-native drop-in for the reference's QwenImageTransformer2DModel
(src/qflux/models/transformer_qwenimage.py:497-672) on the LoRA-training hot path.

Same constructor arguments, state-dict keys, forward signature and return value; `add_adapter`
reproduces peft's naming (X.base_layer / X.lora_A.<name> / X.lora_B.<name>).  The forward and the
backward of the whole DiT are ONE autograd node: for a given shape signature a *launch program*
(flat list of libqfx C-ABI calls with pre-built argument structs over a persistent HBM arena) is
built once and replayed every step -- no per-op autograd graph, no gradient checkpointing (288 GB),
frozen base weights never get a dW, LoRA dA/dB accumulate straight into the flat gradient buffer.

Numerics follow the reference's bf16 eager graph at every rounding point (see csrc/*.hip).
"""
from __future__ import annotations

import contextlib
import os

import torch
import torch.distributed as dist
import torch.nn as nn

from .. import _lib as L
from .. import dropout as DR
from .. import levers
from ..dp import DataParallelMixin
from ..plan_cache import PlanCache, ladder
from ..modules import (LoraConfig, LoraStore, QfxLinear, QfxLoraLinear, QfxRMSNorm, init_lora_, match_target)
from ..plan.prog import _ceil
from ..plan.qwen import _QwenDiTFn, _QwenPlan
from ..rope import QwenEmbedRope, normalize_img_shapes
from ..schedules import flowmatch_tables

lib = L.lib
BF = torch.bfloat16
F32 = torch.float32


# ----------------------------------------------------------------------------------------------
# holder modules (names == reference state-dict keys)
# ----------------------------------------------------------------------------------------------
class _GELUProj(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = QfxLinear(dim_in, dim_out)


class QfxFeedForward(nn.Module):
    def __init__(self, dim, mult=4):
        super().__init__()
        self.net = nn.ModuleList([_GELUProj(dim, dim * mult), nn.Identity(), QfxLinear(dim * mult, dim)])


class QfxAttention(nn.Module):
    def __init__(self, dim, heads, dim_head, eps=1e-6):
        super().__init__()
        inner = heads * dim_head
        self.heads = heads
        for n in ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj"):
            setattr(self, n, QfxLinear(dim, inner))
        self.to_out = nn.ModuleList([QfxLinear(inner, dim), nn.Identity()])
        self.to_add_out = QfxLinear(inner, dim)
        for n in ("norm_q", "norm_k", "norm_added_q", "norm_added_k"):
            setattr(self, n, QfxRMSNorm(dim_head, eps))


class QwenImageTransformerBlock(nn.Module):
    def __init__(self, dim, num_attention_heads, attention_head_dim, eps=1e-6):
        super().__init__()
        self.img_mod = nn.Sequential(nn.Identity(), QfxLinear(dim, 6 * dim))   # index 1 == the Linear (index 0 is SiLU)
        self.attn = QfxAttention(dim, num_attention_heads, attention_head_dim, eps)
        self.img_mlp = QfxFeedForward(dim)
        self.txt_mod = nn.Sequential(nn.Identity(), QfxLinear(dim, 6 * dim))
        self.txt_mlp = QfxFeedForward(dim)


class _TimestepEmbedder(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.linear_1 = QfxLinear(256, dim)
        self.linear_2 = QfxLinear(dim, dim)


class _TimeTextEmbed(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.timestep_embedder = _TimestepEmbedder(dim)


class _AdaLNOut(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.linear = QfxLinear(dim, 2 * dim)


class _Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


# ----------------------------------------------------------------------------------------------
# prepared device-side weights
# ----------------------------------------------------------------------------------------------
class _LoraW:
    __slots__ = ("mod", "r", "Rp", "Kext", "scale", "A_hi", "A_lo", "Bt_hi", "Bt_lo", "We", "WeT", "gA", "gB", "A_hl", "Bt_hl", "hl_dh", "A_fr", "fr_row0", "fr_nf")


class _LinW:
    __slots__ = ("W", "b", "WT", "lora", "N", "K", "mod")

    def __init__(self, mod, need_T: bool):
        self.mod = mod
        base = mod.base_layer if isinstance(mod, QfxLoraLinear) else mod
        self.W = base.weight.data
        assert self.W.is_contiguous() and self.W.dtype == BF
        self.b = base.bias.data if base.bias is not None else None
        self.N, self.K = self.W.shape
        self.WT = self.W.t().contiguous() if need_T else None
        self.lora = None


# ----------------------------------------------------------------------------------------------
class QwenImageTransformer2DModel(DataParallelMixin, nn.Module):
    """See module docstring.  Reference: transformer_qwenimage.py:497-672."""

    _supports_gradient_checkpointing = True

    def __init__(self, patch_size: int = 2, in_channels: int = 64, out_channels: int | None = 16, num_layers: int = 60,
                 attention_head_dim: int = 128, num_attention_heads: int = 24, joint_attention_dim: int = 3584,
                 guidance_embeds: bool = False, axes_dims_rope=(16, 56, 56)):
        super().__init__()
        if attention_head_dim not in (64, 128):
            raise ValueError("qflux_amd attention kernels support head dims 64 and 128")
        self.config = _Cfg(patch_size=patch_size, in_channels=in_channels, out_channels=out_channels, num_layers=num_layers,
                           attention_head_dim=attention_head_dim, num_attention_heads=num_attention_heads,
                           joint_attention_dim=joint_attention_dim, guidance_embeds=guidance_embeds,
                           axes_dims_rope=tuple(axes_dims_rope))
        self.out_channels = out_channels or in_channels
        self.inner_dim = num_attention_heads * attention_head_dim
        D = self.inner_dim
        self.pos_embed = QwenEmbedRope(theta=10000, axes_dim=list(axes_dims_rope), scale_rope=True)   # :546 (no parameters)
        self.time_text_embed = _TimeTextEmbed(D)
        self.txt_norm = QfxRMSNorm(joint_attention_dim, eps=1e-6)
        self.img_in = QfxLinear(in_channels, D)
        self.txt_in = QfxLinear(joint_attention_dim, D)
        self.transformer_blocks = nn.ModuleList(
            [QwenImageTransformerBlock(D, num_attention_heads, attention_head_dim) for _ in range(num_layers)])
        self.norm_out = _AdaLNOut(D)
        self.proj_out = QfxLinear(D, patch_size * patch_size * self.out_channels)
        self._init_state()

    def _init_state(self):      # (the FLUX constructor calls it too)
        self.gradient_checkpointing = False
        self._lora = LoraStore(self)
        self._adapter_name = None
        self._prepared = None      # prepared weights
        self._lora_prep = None     # packed-operand buffers + descriptors
        self._plans = PlanCache()
        self._quant = None         # low-precision trunk mode (quantize_trunk) ...
        self._wq_cache = {}        # ... and the quantised copies of the frozen weights, shared by the model's plans
        self._version = 0
        self._adapter_gen = 0      # bumped ONLY by add_adapter / load_lora_adapter / load_state_dict: what a data-parallel resync keys on
        self._mod_keys = None      # timestep keys of the modulation table (None: the flow-match training timesteps / 1000)
        self._mod_table = None     # None: not decided; False: decided against; dict(keys, mods, out): see ensure_modulation_table
        self._dropout = None       # dropout.LoraDropoutState while network_dropout / rank_dropout are on (set_lora_dropout)
        self._pissa = None         # dict(A0, B0, niter, oversample, seed) once the base weights are PiSSA residuals (pissa_init_)

    # ------------------------------------------------------------------ reference-surface methods
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder: str | None = None, torch_dtype=BF, device_map=None,
                        variant: str | None = None, use_safetensors: bool = True, **unused):
        """diffusers ModelMixin.from_pretrained for a LOCAL checkpoint folder (the reference's loader calls it with
        subfolder="transformer", torch_dtype=weight_dtype, device_map="cpu": src/qflux/models/load_model.py:34-47,
        flux_kontext_loader.py:145-181): `config.json` -> constructor arguments (unknown keys ignored), weights from
        `diffusion_pytorch_model[.<variant>].safetensors` or its sharded form (`...safetensors.index.json` -> weight_map).
        Hub ids are not resolved here (no network on the training nodes: pass the snapshot directory).  Extra keyword
        arguments of the reference's call sites (attn_implementation, ...) are accepted and ignored."""
        import inspect
        import json
        from safetensors import safe_open
        root = str(pretrained_model_name_or_path)
        if subfolder:
            root = os.path.join(root, subfolder)
        if not os.path.isdir(root):
            raise FileNotFoundError(f"{root}: from_pretrained needs a local checkpoint directory (hub ids are not resolved offline)")
        if not use_safetensors:
            raise NotImplementedError("only safetensors checkpoints are read")
        with open(os.path.join(root, "config.json")) as f:
            cfg = json.load(f)
        accepted = set(inspect.signature(cls.__init__).parameters) - {"self"}
        kwargs = {k: (tuple(v) if isinstance(v, list) else v) for k, v in cfg.items() if k in accepted}
        dtype = torch_dtype or BF
        if dtype != BF:
            raise NotImplementedError("the MI355X path keeps the frozen trunk in bf16 (weight_dtype of the reference's configs)")
        device = torch.device("cpu")
        if isinstance(device_map, (str, torch.device)) and str(device_map) not in ("cpu", "auto"):
            device = torch.device(device_map)
        with torch.device(device):
            model = cls(**kwargs)
        stem = "diffusion_pytorch_model" + (f".{variant}" if variant else "")
        index = os.path.join(root, stem + ".safetensors.index.json")
        if os.path.exists(index):
            with open(index) as f:
                files = sorted(set(json.load(f)["weight_map"].values()))
        else:
            files = [stem + ".safetensors"]
        own = dict(model.named_parameters())
        seen = set()
        with torch.no_grad():
            for fn in files:
                with safe_open(os.path.join(root, fn), framework="pt", device=str(device)) as sf:
                    for key in sf.keys():
                        if key not in own:
                            raise KeyError(f"unexpected key {key!r} in {fn}")
                        t = sf.get_tensor(key)
                        if tuple(t.shape) != tuple(own[key].shape):
                            raise ValueError(f"{key}: checkpoint shape {tuple(t.shape)} != model shape {tuple(own[key].shape)}")
                        own[key].copy_(t.to(own[key].dtype))
                        seen.add(key)
        missing = sorted(set(own) - seen)
        if missing:
            raise KeyError(f"{len(missing)} parameters missing from the checkpoint, e.g. {missing[:3]}")
        model._invalidate()
        return model

    @property
    def device(self):
        return self.norm_out.linear.weight.device if isinstance(self.norm_out.linear, QfxLinear) else next(self.parameters()).device

    @property
    def dtype(self):
        return BF      # the frozen trunk is bf16 (adapters are fp32)

    def enable_gradient_checkpointing(self):
        """Accepted for API parity (base_trainer.py:324-325); a no-op: activations stay resident in HBM."""
        self.gradient_checkpointing = True

    def _invalidate(self):
        self._prepared = None
        self._mod_table = None     # rows computed from the prepared frozen weights
        self._lora_prep = None
        self._plans = PlanCache()
        self._wq_cache = {}
        self._version += 1

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        if self._dropout is not None:
            self._dropout.words = fn(self._dropout.words)
        self._invalidate()
        return r

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self._invalidate()
        self._adapter_gen += 1
        return r

    def add_adapter(self, adapter_config, adapter_name: str = "default", generator: torch.Generator | None = None):
        """peft add_adapter look-alike (base_trainer.py:939): wrap matching Linears, freeze all but 'lora' params.
        init_lora_weights="pissa" / "pissa_niter_N" (N <= 4) then runs pissa_init_ with 2 resp. N power iterations: the model
        must be on the GPU (for a model moved later: any other init here, then model.pissa_init_(...) on the device)."""
        cfg = adapter_config
        from ..pissa import check_config, parse_init
        pissa_niter = parse_init(cfg.init_lora_weights)      # a ValueError for a bad spelling, before anything is wrapped
        if pissa_niter is not None:
            check_config(cfg.r, cfg.lora_alpha, "add_adapter")
            if self._pissa is not None:
                raise ValueError("add_adapter: the base weights are PiSSA residuals already")
            if not self.device.type == "cuda":
                raise RuntimeError(f"add_adapter: init_lora_weights={cfg.init_lora_weights!r} factorises the weights on the GPU and the "
                                   f"model is on {self.device}: move it first, or add the adapter with another init and call "
                                   "model.pissa_init_(...) on the device")
        names = [n for n, m in self.named_modules() if isinstance(m, QfxLinear) and ".base_layer" not in n
                 and not n.endswith("base_layer") and match_target(n, cfg.target_modules)]
        for n in names:
            if not self._lora_supported(n):
                raise NotImplementedError(
                    f"LoRA target '{n}': the fused path covers the attention projections, the feed-forward linears, the embedders "
                    f"and the output projection (FLUX: also the single-block proj_mlp / proj_out) and the conditioning head "
                    f"(timestep / guidance / text embedders, AdaLN modulation linears)")
        for n in names:
            parent_name, _, child = n.rpartition(".")
            parent = self.get_submodule(parent_name)
            base = parent[int(child)] if child.isdigit() else getattr(parent, child)
            wrapped = QfxLoraLinear(base, cfg.r, cfg.lora_alpha, adapter_name)
            init_lora_(wrapped, cfg.init_lora_weights, generator)
            if child.isdigit():
                parent[int(child)] = wrapped
            else:
                setattr(parent, child, wrapped)
        prev_name, prev_cfg = self._adapter_name, (getattr(self, "peft_config", None) or {}).get(adapter_name)
        self._adapter_name = adapter_name
        for pn, p in self.named_parameters():
            p.requires_grad_("lora" in pn)
        # diffusers' PeftAdapterMixin.add_adapter keeps the config under `peft_config[adapter_name]`: peft's
        # get_peft_model_state_dict(model, adapter_name=...) -- what BaseTrainer.save_lora calls on the unwrapped DiT
        # (base_trainer.py:870-872) -- reads `.peft_type`, `.bias`, `.use_dora`, `.target_modules` ... from it and then filters
        # model.state_dict() by "lora_" + adapter name.  A real peft.LoraConfig passes through untouched; the stand-in
        # (modules.LoraConfig) carries the same fields.
        if not isinstance(getattr(self, "peft_config", None), dict):
            self.peft_config = {}
        self.peft_config[adapter_name] = cfg
        self._hf_peft_config_loaded = True
        self._invalidate()
        self._adapter_gen += 1
        self._lora.tag()
        if pissa_niter is not None:
            try:
                self.pissa_init_(niter=pissa_niter)
            except Exception:      # (a non-finite weight, ...): no plain LoRA is left behind -- the linears wrapped above are unwrapped again
                for n in names:
                    parent_name, _, child = n.rpartition(".")
                    parent = self.get_submodule(parent_name)
                    if child.isdigit():
                        parent[int(child)] = parent[int(child)].base_layer
                    else:
                        setattr(parent, child, getattr(parent, child).base_layer)
                self._adapter_name = prev_name
                if prev_cfg is None:
                    del self.peft_config[adapter_name]
                else:
                    self.peft_config[adapter_name] = prev_cfg
                self._invalidate()
                self._lora.tag()
                raise
        # The reference wraps its LoRA container in DDP right after this call (base_trainer.py:384-393); the kernels write dA / dB
        # straight into the flat gradient buffer, so the model exchanges them itself.  Under an initialised multi-rank process
        # group that happens without an extra line in the trainer (no-op otherwise; call enable_data_parallel(...) again to
        # choose a process group / bucket size).
        # Opt-out: QFX_AUTO_DP=0 (a trainer that wraps / exchanges the LoRA gradients itself).
        if (self._dp is None and os.environ.get("QFX_AUTO_DP", "1") != "0" and dist.is_available() and dist.is_initialized()
                and dist.get_world_size() > 1):
            self.enable_data_parallel()
        return names

    _LORA_SUFFIXES = ("attn.to_q", "attn.to_k", "attn.to_v", "attn.to_out.0", "attn.add_q_proj", "attn.add_k_proj",
                      "attn.add_v_proj", "attn.to_add_out",
                      "img_mlp.net.0.proj", "img_mlp.net.2", "txt_mlp.net.0.proj", "txt_mlp.net.2",      # Qwen feed-forwards
                      "ff.net.0.proj", "ff.net.2", "ff_context.net.0.proj", "ff_context.net.2")           # FLUX double blocks

    # embedders / output projection: plain GEMM sites outside the blocks (K-extension + the two rank-r gradient launches)
    _HEAD_SITES = {"img_in": "img_in", "txt_in": "txt_in", "proj_out": "proj_out"}      # module name -> key in the prepared weights

    # conditioning head (M = batch rows): timestep embedder, AdaLN modulation linears -- cond_hip.py when adapted
    _COND_SUFFIXES = ("timestep_embedder.linear_1", "timestep_embedder.linear_2", "img_mod.1", "txt_mod.1", "norm_out.linear")

    def _lora_supported(self, name: str) -> bool:
        if name in self._HEAD_SITES or name.endswith(self._COND_SUFFIXES):
            return True
        return name.startswith("transformer_blocks.") and name.endswith(self._LORA_SUFFIXES)

    def _cond_modules(self):
        te = self.time_text_embed.timestep_embedder
        mods = [te.linear_1, te.linear_2, self.norm_out.linear]
        for blk in self.transformer_blocks:
            mods += [blk.img_mod[1], blk.txt_mod[1]]
        return mods

    @property
    def cond_lora(self) -> bool:
        """True when a linear of the conditioning head carries an adapter (the head is then emitted by cond_hip.CondHeadHip)."""
        return any(isinstance(m, QfxLoraLinear) for m in self._cond_modules())

    def set_adapter(self, adapter_name):
        """PeftAdapterMixin.set_adapter (base_trainer.py:940-941): make `adapter_name` the active adapter of every wrapped linear.
        Plans bake adapter pointers, rank and scaling in at build time, so a change of the active adapter drops them."""
        if isinstance(adapter_name, (list, tuple)):
            if len(adapter_name) != 1:
                raise NotImplementedError("one active adapter at a time")
            adapter_name = adapter_name[0]
        wrapped = [m for m in self.modules() if isinstance(m, QfxLoraLinear)]
        if wrapped and not any(adapter_name in m.lora_A for m in wrapped):
            raise ValueError(f"Adapter {adapter_name!r} not found (known: {sorted({k for m in wrapped for k in m.lora_A})})")
        changed = self._adapter_name != adapter_name
        for m in wrapped:
            if adapter_name in m.lora_A and m.active_adapter != adapter_name:
                m.active_adapter, changed = adapter_name, True
        self._adapter_name = adapter_name
        if changed:
            self._invalidate()

    def merge_adapter(self):
        """PeftAdapterMixin.merge_adapter as BaseTrainer.merge_lora calls it (base_trainer.py:413-416): fold every adapter into its
        base weight; the LoRA segment of the GEMMs then carries a zero scale (forward == merged base layer alone)."""
        for m in self.modules():
            if isinstance(m, QfxLoraLinear):
                m.merge()
        self._merged = True
        self._invalidate()

    def unmerge_adapter(self):
        for m in self.modules():
            if isinstance(m, QfxLoraLinear):
                m.unmerge()
        self._merged = False
        self._invalidate()

    def save_lora_weights(self, save_folder, style="diffusers", convert_pissa=False, rank=None):
        """pytorch_lora_weights.safetensors as BaseTrainer.save_lora writes it (base_trainer.py:858-875).  convert_pissa: after a
        PiSSA initialisation, the rank-2r pair that applies to the ORIGINAL base weights (pissa.pissa_to_lora; rank=k resizes it)
        where the default writes the residual-basis A, B a resumed run loads."""
        from ..lora_io import save_lora_weights
        return save_lora_weights(self, save_folder, style, convert_pissa=convert_pissa, rank=rank)

    def pissa_init_(self, niter=2, oversample=8, seed=0, group_bytes=2 << 30):
        """PiSSA initialisation of the adapters in place (qflux_amd.pissa.pissa_init_): the model is on the GPU."""
        from ..pissa import pissa_init_
        return pissa_init_(self, niter=niter, oversample=oversample, seed=seed, group_bytes=group_bytes)

    def load_lora_adapter(self, path, adapter_name="default", lora_alpha=None):
        """DIFFUSERS- or PEFT-style LoRA file/folder (base_trainer.py:977-999)."""
        from ..lora_io import load_lora_adapter
        names = load_lora_adapter(self, path, adapter_name, lora_alpha)
        self._invalidate()
        self._adapter_gen += 1
        self._lora.tag()
        return names

    def quantize_trunk(self, mode: str | None = "mxfp8"):
        """Low-precision trunk switch (the reference's `model.quantize: true`, base_trainer.py:617-621,919-927 ->
        quantize_model_to_fp8): "mxfp8" runs the forward GEMMs of the block linears on the block-scaled FP8 MFMA
        (OCP MX-FP8: e4m3 elements, E8M0 scale per 32 K elements; weights quantised once, activations per launch);
        "mxfp8-fb" also the dX GEMMs of the backward (dY and the transposed weight copy quantised along the contraction);
        None restores the bf16 trunk.  Adapters, biases, norms, attention, the rank-r gradient kernels stay bf16 / fp32."""
        if mode not in (None, "mxfp8", "mxfp8-fb"):
            raise ValueError(f"unknown trunk quantisation {mode!r} (supported: 'mxfp8' = forward GEMMs, 'mxfp8-fb' = forward + dX GEMMs)")
        if mode is not None and self._dropout is not None:
            raise NotImplementedError(DR.MXFP8_REFUSAL)
        self._quant = mode
        self._wq_cache = {}
        self._plans = PlanCache()
        self._version += 1
        return self

    # ------------------------------------------------------------------ dropout on the adapters' rank-r activation
    def set_lora_dropout(self, network_dropout=0.0, rank_dropout=0.0, seed=0):
        """kohya's `network_dropout` (F.dropout on lx = lora_down(x)) and `rank_dropout` (one draw per sample and rank, survivors
        scaled by 1 / (1 - p)) on every adapter of the blocks, the embedders and the output projection (qflux_amd.dropout).  The
        model owns the device state (seed, the count of training forwards, thresholds); masks apply while the model is in training
        mode and the state is enabled, and are the same in the forward and the backward pass.  Both probabilities 0 switches the
        feature off: the plans then emit exactly the launches they emit without it (on / off is part of the plan-cache key, the
        probabilities are not: they live in the state).  Out of scope: the MX-FP8 trunk together with dropout raises
        NotImplementedError; adapters on the conditioning head ([B, K] vectors, cond_hip.py) run without dropout.  Returns the
        state (None when off)."""
        pe, pr = DR.check_probability(network_dropout, "network_dropout"), DR.check_probability(rank_dropout, "rank_dropout")
        if pe == 0.0 and pr == 0.0:
            if self._dropout is not None:      # (plans built with the feature off are keyed apart and stay valid)
                self._dropout = None
                self._plans = PlanCache()
                self._version += 1
            return None
        if self._quant is not None:
            raise NotImplementedError(DR.MXFP8_REFUSAL)
        old = self._dropout
        self._dropout = DR.LoraDropoutState(self.device, pe, pr, seed)
        if old is not None:      # plans bake the state's address in (those built with the feature off are keyed apart)
            self._dropout.enabled = old.enabled
            self._plans = PlanCache()
            self._version += 1
        return self._dropout

    @property
    def lora_dropout(self):
        """The dropout.LoraDropoutState of set_lora_dropout, None while the feature is off."""
        return self._dropout

    @contextlib.contextmanager
    def lora_dropout_off(self):
        """No masks inside the context (the samplers run under it), whatever the mode; the switch is restored on exit."""
        st = self._dropout
        was = st.enabled if st is not None else None
        if st is not None:
            st.enabled = False
        try:
            yield
        finally:
            if st is not None:
                st.enabled = was

    # ------------------------------------------------------------------ modulation table (frozen conditioning head)
    _MOD_TABLE = True     # (the FLUX head also depends on guidance and pooled text: no table there)

    @staticmethod
    def modulation_table_bytes(n_keys: int, num_layers: int, dim: int) -> int:
        """bf16 rows of one key: [2 * num_layers][6 * dim] modulation vectors + [2 * dim] of norm_out."""
        return n_keys * (2 * num_layers * 6 * dim + 2 * dim) * 2

    @staticmethod
    def modulation_table_levers(env=None):
        """(QFX_MOD_TABLE: on unless "0", QFX_MOD_TABLE_GB: size cap in GB, default 8)."""
        env = os.environ if env is None else env
        cap = float(env.get("QFX_MOD_TABLE_GB", "8"))
        if not cap >= 0:
            raise ValueError(f"QFX_MOD_TABLE_GB={env.get('QFX_MOD_TABLE_GB')!r}: a non-negative number of GB")
        return env.get("QFX_MOD_TABLE", "1") != "0", cap

    def _modulation_keys(self):
        if self._mod_keys is None:
            return (flowmatch_tables()[0] / 1000).to(F32).contiguous()
        return self._mod_keys

    def set_modulation_keys(self, keys):
        """The timesteps (as the forward receives them: sigma-scaled, fp32) the modulation table holds rows for.  Other keys than
        the current ones drop an existing table."""
        keys = torch.as_tensor(keys).detach().to("cpu", F32).reshape(-1).contiguous().clone()
        if keys.numel() < 1:
            raise ValueError("set_modulation_keys: at least one key")
        if not torch.equal(keys.view(torch.int32), self._modulation_keys().view(torch.int32)):
            self.drop_modulation_table()
        self._mod_keys = keys

    def drop_modulation_table(self):
        """Free the table; plans that fetch from it are dropped with it.  The next training use builds it again."""
        if self._mod_table:
            self._plans = PlanCache()
            self._version += 1
        self._mod_table = None

    @property
    def modulation_table(self):
        """dict(keys [n] fp32, mods [n, 2L, 6D], out [n, 2D]) when the table exists, else None."""
        return self._mod_table or None

    def ensure_modulation_table(self) -> bool:
        """Build the per-timestep table of the AdaLN modulation vectors if it is allowed and missing; True when it exists.
        The conditioning head (timestep embedding -> linear_1 -> silu -> linear_2 -> silu -> every img_mod / txt_mod, norm_out.linear)
        is a function of the timestep alone, and without adapters on it its weights never change: the 13.6 GB weight stream of the
        big qfx_mod_gemv launch is replaced by a row copy (qfx_mod_table_fetch).  Rows come from the same launches the step
        runs, in batches of 8 keys (a row of qfx_mod_gemv does not depend on the batch it was computed in), so a hit is bit-identical
        to the computed path.  Training entry points call this; inference never builds a table but uses one that exists."""
        if self._mod_table is not None:
            return bool(self._mod_table)
        self._mod_table = False
        if not self._MOD_TABLE or self.device.type != "cuda" or self.cond_lora:
            return False
        on, cap_gb = self.modulation_table_levers()
        keys = self._modulation_keys()
        Lyr, D = self.config.num_layers, self.inner_dim
        if not on or self.modulation_table_bytes(keys.numel(), Lyr, D) > cap_gb * 1e9:
            return False
        P = self._prepare()
        dev, n = self.device, keys.numel()
        kd = keys.to(dev)
        mods_t = torch.empty(n, 2 * Lyr, 6 * D, dtype=BF, device=dev)
        out_t = torch.empty(n, 2 * D, dtype=BF, device=dev)
        tproj, t1, temb = (torch.empty(8, w, dtype=BF, device=dev) for w in (256, D, D))
        mods, mo = torch.empty(2 * Lyr * 8 * 6 * D, dtype=BF, device=dev), torch.empty(8 * 2 * D, dtype=BF, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        for i0 in range(0, n, 8):
            B = min(8, n - i0)
            for rc in (lib.qfx_timestep_embed(kd[i0:].data_ptr(), B, 256, 1000.0, 1.0, tproj.data_ptr(), st),
                       lib.qfx_mod_gemv(tproj.data_ptr(), B, 256, P["t1_Wp"].data_ptr(), P["t1_bp"].data_ptr(), 1, D, 0, t1.data_ptr(), st),
                       lib.qfx_mod_gemv(t1.data_ptr(), B, D, P["t2_Wp"].data_ptr(), P["t2_bp"].data_ptr(), 1, D, 1, temb.data_ptr(), st),
                       lib.qfx_mod_gemv(temb.data_ptr(), B, D, P["mod_W"].data_ptr(), P["mod_b"].data_ptr(), 2 * Lyr, 6 * D, 1,
                                        mods.data_ptr(), st),
                       lib.qfx_mod_gemv(temb.data_ptr(), B, D, P["norm_out_Wp"].data_ptr(), P["norm_out_bp"].data_ptr(), 1, 2 * D, 1,
                                        mo.data_ptr(), st)):
                L.check(rc, "modulation table build")
            mods_t[i0:i0 + B].copy_(mods[:2 * Lyr * B * 6 * D].view(2 * Lyr, B, 6 * D).transpose(0, 1))
            out_t[i0:i0 + B].copy_(mo[:B * 2 * D].view(B, 2 * D))
        self._mod_table = dict(keys=kd, mods=mods_t, out=out_t)
        self._plans = PlanCache()      # plans built before the table existed compute the vectors
        self._version += 1
        return True

    def lora_parameters(self):
        return [p for n, p in self.named_parameters() if "lora_" in n]

    @property
    def lora_store(self) -> LoraStore:
        self._ensure_lora_store()
        return self._lora

    # ------------------------------------------------------------------ preparation
    def _ensure_lora_store(self):
        if not self._lora.is_consistent(self.device):
            self._lora.rebuild(self.device)
            self._lora_prep = None
            self._plans = PlanCache()
        self._lora.ensure_grads()

    def _prepare(self):
        """Contiguous bf16 weights + resident transposed copies for the dX GEMMs (2x weight memory, by design)."""
        if self._prepared is not None:
            return self._prepared
        assert self.device.type == "cuda", "qflux_amd runs on the GPU only (no CPU fallback)"
        P = {"blocks": []}
        for blk in self.transformer_blocks:
            P["blocks"].append(self._prepare_double(blk.attn, blk.img_mlp, blk.txt_mlp, blk.img_mod[1], blk.txt_mod[1]))
        P["img_in"] = _LinW(self.img_in, False)
        P["txt_in"] = _LinW(self.txt_in, False)
        P["t1"] = _LinW(self.time_text_embed.timestep_embedder.linear_1, False)
        P["t2"] = _LinW(self.time_text_embed.timestep_embedder.linear_2, False)
        P["norm_out"] = _LinW(self.norm_out.linear, False)
        P["proj_out"] = _LinW(self.proj_out, True)
        dev = self.device
        mods = [w[s + ".mod"] for w in P["blocks"] for s in ("img", "txt")]
        P["mod_W"] = torch.tensor([m.W.data_ptr() for m in mods], dtype=torch.int64, device=dev)
        P["mod_b"] = torch.tensor([m.b.data_ptr() for m in mods], dtype=torch.int64, device=dev)
        for key in ("t1", "t2", "norm_out"):
            P[key + "_Wp"] = torch.tensor([P[key].W.data_ptr()], dtype=torch.int64, device=dev)
            P[key + "_bp"] = torch.tensor([P[key].b.data_ptr()], dtype=torch.int64, device=dev)
        self._prepared = P
        return P

    @staticmethod
    def _prepare_double(a, img_mlp, txt_mlp, img_mod, txt_mod):
        """Prepared weights of one double-stream block (the Qwen block; the FLUX double block under its own module names)."""
        w = {}
        for s, names in (("img", ("to_q", "to_k", "to_v")), ("txt", ("add_q_proj", "add_k_proj", "add_v_proj"))):
            qkv = [_LinW(getattr(a, n), False) for n in names]
            w[s + ".qkv"] = qkv
            w[s + ".qkvT"] = torch.cat([l.W for l in qkv], dim=0).t().contiguous()       # [D, 3D]
        w["img.o"] = _LinW(a.to_out[0], True)
        w["txt.o"] = _LinW(a.to_add_out, True)
        for s, mlp in (("img", img_mlp), ("txt", txt_mlp)):
            w[s + ".fc1"] = _LinW(mlp.net[0].proj, True)
            w[s + ".fc2"] = _LinW(mlp.net[2], True)
        w["img.mod"] = _LinW(img_mod, False)
        w["txt.mod"] = _LinW(txt_mod, False)
        w["norms"] = (a.norm_added_q.weight.data, a.norm_added_k.weight.data, a.norm_q.weight.data, a.norm_k.weight.data)
        return w

    def _prepare_lora(self):
        """Packed bf16 operand buffers for every adapter (+ the device descriptor array for qfx_lora_pack)."""
        if self._lora_prep is not None:
            return self._lora_prep
        P = self._prepare()
        self._ensure_lora_store()
        lv = levers.read()
        descs = []
        max_dim = 1
        for w, blk in zip(P["blocks"], self.transformer_blocks):
            max_dim = max(max_dim, self._prep_double_lora(w, blk.attn, descs, lv))
        return self._finish_lora_prep(descs, max(max_dim, self._prep_head_lora(P, descs)))

    def _finish_lora_prep(self, descs, max_dim):
        prep = dict(n=len(descs), max_dim=max_dim, descs=None)
        if descs:
            arr = (L.LoraPackArgs * len(descs))(*descs)
            prep["descs"] = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device)
        self._lora_prep = prep
        return prep

    def _prep_site_lora(self, lw, descs, hl=None):
        """Operand buffers of ONE adapted linear that is not part of a q/k/v group (own A_hi/A_lo and WeT)."""
        m = lw.mod
        if not isinstance(m, QfxLoraLinear):
            lw.lora = None
            return 1
        if m.in_features % 32:
            raise NotImplementedError(f"LoRA on a linear with in_features={m.in_features}: the rank-r kernels contract in 32-wide steps")
        dev = self.device
        r = m.r[m.active_adapter]
        Rp, Kext = _ceil(r, 16), _ceil(3 * _ceil(r, 16), 64)
        K = m.in_features
        lw.lora = self._make_lora(m, Rp, Kext, torch.zeros(Rp, K, dtype=BF, device=dev), torch.zeros(Rp, K, dtype=BF, device=dev),
                                  torch.zeros(K, Kext, dtype=BF, device=dev), dev, hl=hl)
        descs.append(self._pack_desc(lw.lora))
        return max(lw.N, K)

    def _prep_head_lora(self, P, descs):
        return max(self._prep_site_lora(P[key], descs) for key in self._HEAD_SITES.values())

    def _prep_qkv_lora(self, w, prefix, mods, descs, lv, WeT=None, hl=None):
        """LoRA operand buffers of a q/k/v projection group sharing one input: concatenated A_hi/A_lo [3Rp,D] (one fused
        down-projection) and WeT [D, 3*Kext] (one K-extension of the dX GEMM).  WeT may be a column slice of a bigger B2."""
        dev, D = self.device, self.inner_dim
        lmods = [m for m in mods if isinstance(m, QfxLoraLinear)]
        w[prefix + "qkv_lora"] = None
        if not lmods:
            return 1
        r = lmods[0].r[lmods[0].active_adapter]
        Rp, Kext = _ceil(r, 16), _ceil(3 * _ceil(r, 16), 64)
        A_hi = torch.zeros(3 * Rp, D, dtype=BF, device=dev)
        A_lo = torch.zeros_like(A_hi)
        if WeT is None:
            WeT = torch.zeros(D, 3 * Kext, dtype=BF, device=dev)
        else:
            WeT = WeT(Kext)
        # the same rows in MFMA-fragment order for the fused LayerNorm + down projection (qfx_ln_down_args.W_fr): [hi image | lo image]
        A_fr = torch.zeros(2 * 3 * Rp * D, dtype=BF, device=dev) if (D % 32 == 0 and lv.ln_down_frag) else None
        w[prefix + "qkv_lora"] = dict(Rp=Rp, Kext=Kext, A_hi=A_hi, A_lo=A_lo, A_fr=A_fr, WeT=WeT, present=[isinstance(m, QfxLoraLinear) for m in mods])
        md = 1
        for sec, (m, lw) in enumerate(zip(mods, w[prefix + "qkv"])):
            if not isinstance(m, QfxLoraLinear):
                continue
            lo = self._make_lora(m, Rp, Kext, A_hi[sec * Rp:(sec + 1) * Rp], A_lo[sec * Rp:(sec + 1) * Rp],
                                 WeT[:, sec * Kext:(sec + 1) * Kext], dev, hl=hl)
            lo.A_fr, lo.fr_row0, lo.fr_nf = A_fr, sec * Rp, 3 * Rp // 16
            lw.lora = lo
            descs.append(self._pack_desc(lo))
            md = max(md, lw.N, lw.K)
        return md

    def _prep_double_lora(self, w, a, descs, lv):
        md = 1
        # head-fragment weight images for the attention epilogues' rank-r projections (qfx_head_lora, ABI 6)
        hl = lv.fuse_head_lora and self.config.attention_head_dim % 32 == 0
        for s, names in (("img", ("to_q", "to_k", "to_v")), ("txt", ("add_q_proj", "add_k_proj", "add_v_proj"))):
            md = max(md, self._prep_qkv_lora(w, s + ".", [getattr(a, n) for n in names], descs, lv, hl="Bt" if hl else None))
        for key in ("img.o", "txt.o", "img.fc1", "img.fc2", "txt.fc1", "txt.fc2"):
            md = max(md, self._prep_site_lora(w[key], descs, hl="A" if (hl and key.endswith(".o")) else None))
        return md

    def _make_lora(self, m: QfxLoraLinear, Rp, Kext, A_hi, A_lo, WeT, dev, hl=None):
        lo = _LoraW()
        name = m.active_adapter
        lo.mod, lo.r, lo.Rp, lo.Kext, lo.scale = m, m.r[name], Rp, Kext, m.scaling[name]
        N, K = m.out_features, m.in_features
        lo.A_hi, lo.A_lo, lo.WeT = A_hi, A_lo, WeT
        lo.Bt_hi = torch.zeros(Rp, N, dtype=BF, device=dev)
        lo.Bt_lo = torch.zeros(Rp, N, dtype=BF, device=dev)
        lo.We = torch.zeros(N, Kext, dtype=BF, device=dev)
        lo.A_hl = torch.zeros(2 * Rp * K, dtype=BF, device=dev) if hl == "A" else None
        lo.Bt_hl = torch.zeros(2 * Rp * N, dtype=BF, device=dev) if hl == "Bt" else None
        lo.hl_dh = self.config.attention_head_dim
        lo.A_fr, lo.fr_row0, lo.fr_nf = None, 0, 0
        st = self._lora
        oa, ob = st.offset_of(m.A), st.offset_of(m.B)
        lo.gA = st.gflat[oa:oa + m.A.numel()]
        lo.gB = st.gflat[ob:ob + m.B.numel()]
        return lo

    @staticmethod
    def _pack_desc(lo: _LoraW):
        d = L.LoraPackArgs()
        m = lo.mod
        d.A, d.B, d.r, d.K, d.N = m.A.data_ptr(), m.B.data_ptr(), lo.r, m.in_features, m.out_features
        d.scale = 0.0 if m.merged else lo.scale      # merged adapter: the base weight already holds scale * B A
        d.A_hi, d.A_lo, d.ld_a = lo.A_hi.data_ptr(), lo.A_lo.data_ptr(), lo.A_hi.stride(0)
        d.Bt_hi, d.Bt_lo, d.ld_bt = lo.Bt_hi.data_ptr(), lo.Bt_lo.data_ptr(), lo.Bt_hi.stride(0)
        d.We, d.ld_we = lo.We.data_ptr(), lo.We.stride(0)
        d.WeT, d.ld_wet = lo.WeT.data_ptr(), lo.WeT.stride(0)
        d.Rp, d.Kext = lo.Rp, lo.Kext
        d.A_hl = lo.A_hl.data_ptr() if lo.A_hl is not None else None
        d.Bt_hl = lo.Bt_hl.data_ptr() if lo.Bt_hl is not None else None
        d.hl_dh = lo.hl_dh
        d.A_fr = lo.A_fr.data_ptr() if lo.A_fr is not None else None
        d.fr_row0, d.fr_nf = lo.fr_row0, lo.fr_nf
        return d

    def refresh_lora_operands(self):
        """Re-split the fp32 adapter weights into the bf16 hi/lo MFMA operands (one launch for all adapters)."""
        prep = self._prepare_lora()
        if prep["n"]:
            rc = lib.qfx_lora_pack(prep["descs"].data_ptr(), prep["n"], prep["max_dim"], torch.cuda.current_stream().cuda_stream)
            L.check(rc, "qfx_lora_pack")

    # ------------------------------------------------------------------ forward
    @contextlib.contextmanager
    def cache_context(self, name: str):
        """diffusers CacheMixin.cache_context("cond"|"uncond") (qwen_image_edit_trainer.py:1237,1255): no feature caches exist
        here, the context is accepted for call-site compatibility."""
        yield

    def forward(self, hidden_states, encoder_hidden_states=None, encoder_hidden_states_mask=None, timestep=None,
                img_shapes=None, txt_seq_lens=None, guidance=None, attention_kwargs=None, return_dict=True, attention_mask=None):
        """attention_mask: optional bool [B, T+S_max] padding mask of the multi-resolution model (transformer_qwen_custom.py:384-396);
        with it, or with per-sample img_shapes that differ, the masked / per-sample-RoPE launch program runs."""
        if encoder_hidden_states is None:
            raise ValueError("QwenImageTransformer2DModel requires encoder_hidden_states (text stream)")
        if guidance is not None:
            raise NotImplementedError("guidance embeddings are not part of the Qwen-Image-Edit training path")
        B, S_i, T = hidden_states.shape[0], hidden_states.shape[1], encoder_hidden_states.shape[1]
        batched = isinstance(img_shapes, list) and len(img_shapes) > 0 and isinstance(img_shapes[0], list)
        ragged = batched and not all(sh == img_shapes[0] for sh in img_shapes)
        if self.training and torch.is_grad_enabled():
            self.ensure_modulation_table()      # the drop-in module's first training-mode forward builds it
        if attention_mask is not None or ragged:
            if attention_mask is not None:
                if attention_mask.dim() != 2:
                    raise ValueError("attention_mask must have shape (batch, total_sequence_length).")
                if attention_mask.shape[1] < T + S_i:
                    raise ValueError(f"attention_mask length {attention_mask.shape[1]} is smaller than expected sequence length {T + S_i}.")
            plan = self.get_plan_multires(B, S_i, T, img_shapes, txt_seq_lens, attention_mask)
        else:
            plan = self.get_plan(B, S_i, T, img_shapes, txt_seq_lens)
        out = _QwenDiTFn.apply(self, plan, hidden_states, encoder_hidden_states, timestep, *self.lora_parameters())
        return (out,) if not return_dict else _Cfg(sample=out)

    def get_plan(self, B, S_i, T, img_shapes, txt_seq_lens):
        shapes = normalize_img_shapes(img_shapes)
        if sum(f * h * w for f, h, w in shapes) != S_i:
            raise ValueError(f"img_shapes {shapes} do not cover the {S_i} image tokens")
        if txt_seq_lens is not None and max(txt_seq_lens) != T:
            raise ValueError("max(txt_seq_lens) must equal the text sequence length (reference RoPE broadcast)")
        self._prepare()
        self._prepare_lora()
        key = (B, S_i, T, shapes, self._version, self._dropout is not None)
        return self._plans.get_or_build(key, lambda: _QwenPlan(self, B, S_i, T, shapes))

    def get_plan_multires(self, B, S_i, T, img_shapes, txt_seq_lens, attention_mask):
        """One plan per LADDER size of the padded shape (B, ladder(S_max), T) in an LRU-bounded cache (plan_cache.py): the rows
        between S_max and the ladder size are further padded rows of the masked program.  The per-batch contents (per-sample
        RoPE, key mask, row masks) are refreshed on every call."""
        self._prepare()
        self._prepare_lora()
        S_plan = ladder(S_i)
        key = ("multires", B, S_plan, T, self._version, self._dropout is not None)
        plan = self._plans.get_or_build(key, lambda: _QwenPlan(self, B, S_plan, T, None, multires=True))
        plan.set_multires(img_shapes, txt_seq_lens, attention_mask, S_in=S_i)
        return plan
