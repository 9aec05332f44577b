"""MI355X-native drop-in for FluxTransformer2DModel on the LoRA-training hot path
(reference: src/qflux/models/transformer_flux.py:557-828; blocks :385-523; attention processor :102-166;
FluxPosEmbed :526-554).  Same constructor arguments, diffusers state-dict keys and forward signature.

Built on the same launch-program machinery as the Qwen model (plan/flux.py describes the programs).
RoPE: real cos/sin from ids (float64 on the host, cached) == the complex rotation the kernels already apply;
q/k norms are torch.nn.RMSNorm (single rounding): norm_flags = 1.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import levers
from ..plan.flux import _FluxPlan, flux_joint_rope  # noqa: F401  (flux_joint_rope: this module's public helper)
from ..plan.prog import _ceil
from ..plan.qwen import _QwenDiTFn
from ..plan_cache import ladder
from ..modules import QfxLinear, QfxRMSNorm
from .transformer_qwenimage import (BF, QfxAttention, QfxFeedForward, QwenImageTransformer2DModel, _AdaLNOut, _Cfg, _LinW,
                                    _TimestepEmbedder)


class _NormLinear(nn.Module):
    """AdaLayerNormZero / -Single holder: only `.linear` carries parameters."""

    def __init__(self, dim, n):
        super().__init__()
        self.linear = QfxLinear(dim, n * dim)


class FluxTransformerBlock(nn.Module):
    def __init__(self, dim, heads, dim_head):
        super().__init__()
        self.norm1 = _NormLinear(dim, 6)
        self.norm1_context = _NormLinear(dim, 6)
        self.attn = QfxAttention(dim, heads, dim_head, eps=1e-6)
        self.ff = QfxFeedForward(dim)
        self.ff_context = QfxFeedForward(dim)


class _SingleAttn(nn.Module):
    def __init__(self, dim, heads, dim_head):
        super().__init__()
        self.heads = heads
        for n in ("to_q", "to_k", "to_v"):
            setattr(self, n, QfxLinear(dim, heads * dim_head))
        self.norm_q = QfxRMSNorm(dim_head, 1e-6)
        self.norm_k = QfxRMSNorm(dim_head, 1e-6)


class FluxSingleTransformerBlock(nn.Module):
    def __init__(self, dim, heads, dim_head, mlp_ratio=4.0):
        super().__init__()
        self.norm = _NormLinear(dim, 3)
        self.proj_mlp = QfxLinear(dim, int(dim * mlp_ratio))
        self.proj_out = QfxLinear(dim + int(dim * mlp_ratio), dim)
        self.attn = _SingleAttn(dim, heads, dim_head)


class _TextProj(nn.Module):
    def __init__(self, pooled, dim):
        super().__init__()
        self.linear_1 = QfxLinear(pooled, dim)
        self.linear_2 = QfxLinear(dim, dim)


class _CombinedEmb(nn.Module):
    def __init__(self, dim, pooled, guidance):
        super().__init__()
        self.timestep_embedder = _TimestepEmbedder(dim)
        if guidance:
            self.guidance_embedder = _TimestepEmbedder(dim)
        self.text_embedder = _TextProj(pooled, dim)


class FluxTransformer2DModel(QwenImageTransformer2DModel):
    """See module docstring."""

    def __init__(self, patch_size: int = 1, in_channels: int = 64, out_channels: int | None = None, num_layers: int = 19,
                 num_single_layers: int = 38, attention_head_dim: int = 128, num_attention_heads: int = 24,
                 joint_attention_dim: int = 4096, pooled_projection_dim: int = 768, guidance_embeds: bool = False,
                 axes_dims_rope=(16, 56, 56)):
        nn.Module.__init__(self)
        if attention_head_dim not in (64, 128):
            raise ValueError("qflux_amd attention kernels support head dims 64 and 128")
        self.config = _Cfg(patch_size=patch_size, in_channels=in_channels, out_channels=out_channels, num_layers=num_layers,
                           num_single_layers=num_single_layers, attention_head_dim=attention_head_dim,
                           num_attention_heads=num_attention_heads, joint_attention_dim=joint_attention_dim,
                           pooled_projection_dim=pooled_projection_dim, guidance_embeds=guidance_embeds,
                           axes_dims_rope=tuple(axes_dims_rope))
        self.out_channels = out_channels or in_channels
        self.inner_dim = D = num_attention_heads * attention_head_dim
        self.time_text_embed = _CombinedEmb(D, pooled_projection_dim, guidance_embeds)
        self.context_embedder = QfxLinear(joint_attention_dim, D)
        self.x_embedder = QfxLinear(in_channels, D)
        self.transformer_blocks = nn.ModuleList([FluxTransformerBlock(D, num_attention_heads, attention_head_dim) for _ in range(num_layers)])
        self.single_transformer_blocks = nn.ModuleList(
            [FluxSingleTransformerBlock(D, num_attention_heads, attention_head_dim) for _ in range(num_single_layers)])
        self.norm_out = _AdaLNOut(D)
        self.proj_out = QfxLinear(D, patch_size * patch_size * self.out_channels)
        self._init_state()
        self._rope_cache = {}

    _HEAD_SITES = {"x_embedder": "x_in", "context_embedder": "c_in", "proj_out": "proj_out"}
    _MOD_TABLE = False    # temb also depends on guidance and the pooled text: no per-timestep modulation table

    _COND_SUFFIXES = ("timestep_embedder.linear_1", "timestep_embedder.linear_2", "guidance_embedder.linear_1", "guidance_embedder.linear_2",
                      "text_embedder.linear_1", "text_embedder.linear_2", "norm1.linear", "norm1_context.linear", "norm.linear",
                      "norm_out.linear")

    def _cond_modules(self):
        te = self.time_text_embed
        mods = [te.timestep_embedder.linear_1, te.timestep_embedder.linear_2, te.text_embedder.linear_1, te.text_embedder.linear_2,
                self.norm_out.linear]
        if self.config.guidance_embeds:
            mods += [te.guidance_embedder.linear_1, te.guidance_embedder.linear_2]
        for blk in self.transformer_blocks:
            mods += [blk.norm1.linear, blk.norm1_context.linear]
        mods += [blk.norm.linear for blk in self.single_transformer_blocks]
        return mods

    def _lora_supported(self, name: str) -> bool:
        if name in self._HEAD_SITES or name.endswith(self._COND_SUFFIXES):
            return True
        if name.startswith("transformer_blocks."):
            return name.endswith(self._LORA_SUFFIXES)
        return name.startswith("single_transformer_blocks.") and name.endswith(("attn.to_q", "attn.to_k", "attn.to_v", "proj_mlp", "proj_out"))

    # ------------------------------------------------------------------ preparation
    def _prepare(self):
        if self._prepared is not None:
            return self._prepared
        assert self.device.type == "cuda", "qflux_amd runs on the GPU only (no CPU fallback)"
        dev = self.device
        P = {"blocks": [], "singles": []}
        for blk in self.transformer_blocks:
            P["blocks"].append(self._prepare_double(blk.attn, blk.ff, blk.ff_context, blk.norm1.linear, blk.norm1_context.linear))
        for blk in self.single_transformer_blocks:
            a = blk.attn
            w = {"qkv": [_LinW(getattr(a, n), False) for n in ("to_q", "to_k", "to_v")]}
            w["qkvT"] = torch.cat([l.W for l in w["qkv"]], dim=0).t().contiguous()       # [D, 3D]
            w["mlp"] = _LinW(blk.proj_mlp, True)                                           # WT [D, 4D]
            w["out"] = _LinW(blk.proj_out, True)                                           # W [D, 5D], WT [5D, D]
            w["mod"] = _LinW(blk.norm.linear, False)
            w["norms"] = (a.norm_q.weight.data, a.norm_k.weight.data)
            w["B2"] = w["mlp"].WT                                                          # replaced by [WmlpT | WeT] when LoRA'd
            P["singles"].append(w)
        te = self.time_text_embed
        lin = {"x_in": self.x_embedder, "c_in": self.context_embedder, "t1": te.timestep_embedder.linear_1,
               "t2": te.timestep_embedder.linear_2, "p1": te.text_embedder.linear_1, "p2": te.text_embedder.linear_2,
               "norm_out": self.norm_out.linear}
        if self.config.guidance_embeds:
            lin["g1"], lin["g2"] = te.guidance_embedder.linear_1, te.guidance_embedder.linear_2
        for k, m in lin.items():
            P[k] = _LinW(m, False)
            P[k + "_Wp"] = torch.tensor([P[k].W.data_ptr()], dtype=torch.int64, device=dev)
            P[k + "_bp"] = torch.tensor([P[k].b.data_ptr()], dtype=torch.int64, device=dev)
        P["proj_out"] = _LinW(self.proj_out, True)
        Jd = self.config.joint_attention_dim
        if Jd % 64:   # the GEMM contracts in 64-wide K tiles: zero-pad the context embedder's K once
            Jp = _ceil(Jd, 64)
            wpad = torch.zeros(self.inner_dim, Jp, dtype=BF, device=dev)
            wpad[:, :Jd].copy_(P["c_in"].W)
            P["c_in"].W, P["c_in"].K = wpad, Jp
        mods = [w[s + ".mod"] for w in P["blocks"] for s in ("img", "txt")]
        P["mod_W"] = torch.tensor([m.W.data_ptr() for m in mods], dtype=torch.int64, device=dev)
        P["mod_b"] = torch.tensor([m.b.data_ptr() for m in mods], dtype=torch.int64, device=dev)
        P["smod_W"] = torch.tensor([w["mod"].W.data_ptr() for w in P["singles"]] or [0], dtype=torch.int64, device=dev)
        P["smod_b"] = torch.tensor([w["mod"].b.data_ptr() for w in P["singles"]] or [0], dtype=torch.int64, device=dev)
        self._prepared = P
        return P

    def _prepare_lora(self):
        if self._lora_prep is not None:
            return self._lora_prep
        P = self._prepare()
        self._ensure_lora_store()
        lv = levers.read()
        dev, D = self.device, self.inner_dim
        descs = []
        max_dim = 1
        for w, blk in zip(P["blocks"], self.transformer_blocks):
            max_dim = max(max_dim, self._prep_double_lora(w, blk.attn, descs, lv))
        for w, blk in zip(P["singles"], self.single_transformer_blocks):
            a = blk.attn

            # adapters on proj_mlp / proj_out (configs/face_seg_flux_kontext_fp16.yaml:11) are stand-alone sites; proj_mlp's
            # backward K-extension joins segment 2 of the block's dX GEMM: [W_mlp^T | WeT(q) WeT(k) WeT(v) | WeT(mlp)]
            max_dim = max(max_dim, self._prep_site_lora(w["mlp"], descs), self._prep_site_lora(w["out"], descs))
            kx_mlp = w["mlp"].lora.Kext if w["mlp"].lora is not None else 0

            def make_wet(Kext, w=w, kx_mlp=kx_mlp):
                # dX B operand of the single block: [W_mlp^T | WeT(q) WeT(k) WeT(v)] so the LoRA K-extension rides in segment 2
                b2 = torch.zeros(D, 4 * D + 3 * Kext + kx_mlp, dtype=BF, device=dev)
                b2[:, : 4 * D].copy_(w["mlp"].WT)
                w["B2"] = b2
                return b2[:, 4 * D: 4 * D + 3 * Kext]

            max_dim = max(max_dim, self._prep_qkv_lora(w, "", [a.to_q, a.to_k, a.to_v], descs, lv, WeT=make_wet))
            if kx_mlp:
                if w["qkv_lora"] is None:
                    make_wet(0)
                # the packed WeT of proj_mlp must live inside B2: re-point the adapter's WeT (and its pack descriptor) there
                lo = w["mlp"].lora
                kq = 3 * w["qkv_lora"]["Kext"] if w["qkv_lora"] is not None else 0
                lo.WeT = w["B2"][:, 4 * D + kq: 4 * D + kq + kx_mlp]
                for d_ in descs:
                    if d_.A == lo.mod.A.data_ptr():
                        d_.WeT, d_.ld_wet = lo.WeT.data_ptr(), lo.WeT.stride(0)
        return self._finish_lora_prep(descs, max(max_dim, self._prep_head_lora(P, descs)))

    # ------------------------------------------------------------------ forward
    def forward(self, hidden_states, encoder_hidden_states=None, pooled_projections=None, timestep=None, img_ids=None, txt_ids=None,
                guidance=None, joint_attention_kwargs=None, controlnet_block_samples=None, controlnet_single_block_samples=None,
                return_dict=True, controlnet_blocks_repeat=False, attention_mask=None):
        if controlnet_block_samples is not None or controlnet_single_block_samples is not None:
            raise NotImplementedError("controlnet residuals are not part of the LoRA training path")
        if self.config.guidance_embeds and guidance is None:
            raise ValueError("guidance_embeds=True requires `guidance`")
        B, S_i, T = hidden_states.shape[0], hidden_states.shape[1], encoder_hidden_states.shape[1]
        if attention_mask is not None:
            m = attention_mask if attention_mask.dtype == torch.bool else attention_mask > 0
            if m.dim() != 2 or m.shape[1] < T + S_i:
                raise ValueError("attention_mask must have shape (batch, total_sequence_length).")
            if not bool(m.all()):
                plan = self.get_plan_multires(B, S_i, T, img_ids, m[:, T:T + S_i].sum(dim=1).tolist())
            else:
                attention_mask = None
        if attention_mask is None:
            plan = self.get_plan(B, S_i, T, img_ids[0] if img_ids.ndim == 3 else img_ids, txt_ids)
        out = _QwenDiTFn.apply(self, plan, (hidden_states, pooled_projections, guidance), encoder_hidden_states, timestep,
                               *self.lora_parameters())
        return (out,) if not return_dict else _Cfg(sample=out)

    def get_plan(self, B, S_i, T, img_ids, txt_ids):
        if img_ids.ndim == 3:
            img_ids = img_ids[0]
        if txt_ids.ndim == 3:
            txt_ids = txt_ids[0]
        if img_ids.shape[0] != S_i or txt_ids.shape[0] != T:
            raise ValueError("img_ids / txt_ids do not match the sequence lengths")
        ids = torch.cat((txt_ids.float().cpu(), img_ids.float().cpu()), dim=0)
        rkey = (tuple(ids.shape), hash(ids.numpy().tobytes()))
        self._prepare()
        self._prepare_lora()
        key = (B, S_i, T, rkey, self._version, self._dropout is not None)
        return self._plans.get_or_build(key, lambda: _FluxPlan(self, B, S_i, T, ids))

    def get_plan_multires(self, B, S_i, T, img_ids, valid_lens):
        """Multi-resolution plan: one per LADDER size of the padded shape, in an LRU-bounded cache (plan_cache.py); rows between the
        batch maximum and the ladder size are further padded rows.  RoPE / masks are refreshed every call."""
        if img_ids.ndim == 2:
            img_ids = img_ids.unsqueeze(0).expand(B, -1, -1)
        self._prepare()
        self._prepare_lora()
        S_plan = ladder(S_i)
        key = (B, S_plan, T, "multires", self._version, self._dropout is not None)
        plan = self._plans.get_or_build(key, lambda: _FluxPlan(self, B, S_plan, T, None, multires=True))
        plan.set_multires(img_ids, valid_lens)
        return plan
