"""The FLUX launch plan: the double-stream blocks reuse the Qwen emitters (AdaLayerNormZero == modulation GEMV + ln_modulate with
the same (shift, scale, gate) x2 chunk order); the single-stream blocks run on the joint [text|image] buffer:
    ln_modulate -> grouped q/k/v GEMM (+LoRA K-ext) + proj_mlp GEMM (GELU epilogue) -> qk_norm_rope -> attention ->
    proj_out as a two-segment GEMM  [attn | gelu(mlp)] @ W_out^T  (no concat buffer), epilogue x + gate*y
and backward mirrors it with ONE dX GEMM over K = 3D (dq|dk|dv) + 4D (d mlp) + LoRA extension."""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib as L
from ..cond_hip import CondHeadHip
from .emit import _flush_batch, _gargs, _kext, _ln_fwd_args, emit_attn_backward
from .prog import _Prog, _ceil, _ptr
from .qwen import F32, STREAMS, _QwenPlan

lib = L.lib


def flux_joint_rope(ids: torch.Tensor, axes_dim, theta: float = 10000.0) -> torch.Tensor:
    """FluxPosEmbed (transformer_flux.py:533-554) in the kernels' layout [S, dh/2, 2] (cos, sin), float64 math."""
    pos = ids.detach().float().cpu()
    parts = []
    for i, d in enumerate(axes_dim):
        freqs = 1.0 / (theta ** (torch.arange(0, d, 2, dtype=torch.float64) / d))
        ang = torch.outer(pos[:, i].to(torch.float64), freqs)
        parts.append(torch.stack([ang.cos(), ang.sin()], dim=-1))
    return torch.cat(parts, dim=1).float().contiguous()


class _FluxPlan(_QwenPlan):
    NORM_FLAGS = 1  # torch.nn.RMSNorm rounding

    def __init__(self, model, B, S_i, T, ids, multires=False):
        self._setup(model, B, S_i, T)
        self.multires = multires
        cfg = model.config
        D, S, H, dh, S_pad = self.D, self.S, self.H, self.dh, self.S_pad
        buf, rows = self.buf, self.rows
        Ld, Ls = cfg.num_layers, cfg.num_single_layers
        Cin, Cout, Jd, Pd = cfg.in_channels, model.proj_out.out_features, cfg.joint_attention_dim, cfg.pooled_projection_dim
        P = model._prepared
        A = self.A
        if multires:
            self.rmask["joint"] = self._alloc_multires(rm_joint=B * S)      # row mask of the joint [text | image] rows (single blocks)
        else:
            self.rope = flux_joint_rope(ids, cfg.axes_dims_rope).to(model.device)
            assert self.rope.shape == (S, dh // 2, 2)
        A["in_img"] = buf(B * S_i, Cin); A["in_txt"] = buf(B * T, P["c_in"].K, zero=True); A["pooled"] = buf(B, Pd)
        A["t"] = buf(B, dtype=F32); A["gd"] = buf(B, dtype=F32)
        for k in ("tproj", "gproj"):
            A[k] = buf(B, 256)
        for k in ("t1", "t2", "g1", "g2", "p1", "p2", "temb"):
            A[k] = buf(1, B, D)
        A["X"] = {s: [buf(rows[s], D) for _ in range(Ld + 1)] for s in STREAMS}
        A["J"] = [buf(B * S, D) for _ in range(Ls + 1)]
        A["mods"] = buf(max(2 * Ld, 1), B, 6 * D); A["smods"] = buf(max(Ls, 1), B, 3 * D); A["mod_out"] = buf(1, B, 2 * D)
        A["xn_out"] = buf(B * S_i, D); A["out"] = buf(B * S_i, Cout)
        A["dpred"] = buf(B * S_i, Cout); A["dxn"] = buf(B * S_i, D)
        A["blk"] = [self._alloc_double_block(w) for w in P["blocks"]]
        self._alloc_double_scratch(P["blocks"])
        # single-stream blocks
        mpj = _ceil(B * S, 128)
        A["sblk"] = []
        kext_s, rp_s = 0, 0
        kext_m = 0
        for w in P["singles"]:
            b = dict(qkv=buf(B, S, 3 * D), sqk=buf(B, S, 2 * D), lse=buf(B, H, S_pad, dtype=F32, zero=True), h=buf(B * S, 4 * D))
            if w["out"].lora is not None or self.model._quant:
                # adapter on proj_out: its input [attn | gelu(mlp)] is kept as ONE row-major buffer (attention and the GELU epilogue
                # write straight into its two column ranges), so that u = cat A^T and dA = v^T cat are single rank-r launches.
                # MX-FP8 trunk: the same layout makes proj_out ONE contraction over K = 5D, which the block-scaled kernel takes
                # (its two-segment form -- different operands per segment -- exists in bf16 only)
                b["cat"] = buf(B * S, 5 * D)
                b["ao"] = b["cat"][:, :D]
            else:
                b["ao"] = buf(B * S, D)
            grp = w["qkv_lora"]
            if grp is not None or w["mlp"].lora is not None:
                b["xm"] = buf(B * S, D)
            if grp is not None:
                b["Uqkv"] = (buf(3 * grp["Rp"], mpj, zero=True), buf(3 * grp["Rp"], mpj, zero=True))
                kext_s, rp_s = max(kext_s, grp["Kext"]), max(rp_s, grp["Rp"])
            b["site_mlp"] = self._site_alloc(w["mlp"], B * S)
            b["site_out"] = self._site_alloc(w["out"], B * S)
            if w["mlp"].lora is not None:
                kext_m = max(kext_m, w["mlp"].lora.Kext)
            A["sblk"].append(b)
        A["xm_j"] = buf(B * S, D); A["g_j"] = buf(B * S, 4 * D)
        A["A2"] = buf(B * S, 4 * D + 3 * kext_s + kext_m, zero=True)   # [d(mlp pre-act) | LoRA v ext (q,k,v) | LoRA v ext (proj_mlp)] : A operand, segment 2 of the dX GEMM
        self.cond = model.cond_lora
        if self.cond:
            A["dmods"] = buf(max(2 * Ld, 1), B, 6 * D, dtype=F32, zero=True)
            A["dsmods"] = buf(max(Ls, 1), B, 3 * D, dtype=F32, zero=True)
            A["dmod_out"] = buf(1, B, 2 * D, dtype=F32, zero=True)
            te = model.time_text_embed
            chains = [(te.timestep_embedder.linear_1, te.timestep_embedder.linear_2, A["tproj"], A["t1"], A["t2"])]
            if cfg.guidance_embeds:
                chains.append((te.guidance_embedder.linear_1, te.guidance_embedder.linear_2, A["gproj"], A["g1"], A["g2"]))
            chains.append((te.text_embedder.linear_1, te.text_embedder.linear_2, A["pooled"], A["p1"], A["p2"]))
            banks = []
            if Ld:
                banks.append(([m for blk in model.transformer_blocks for m in (blk.norm1.linear, blk.norm1_context.linear)],
                              A["mods"], A["dmods"]))
            if Ls:
                banks.append(([blk.norm.linear for blk in model.single_transformer_blocks], A["smods"], A["dsmods"]))
            banks.append(([model.norm_out.linear], A["mod_out"], A["dmod_out"]))
            self.cond_head = CondHeadHip(model, B, D, chains=chains, temb=A["temb"], banks=banks, buf=buf)
            for bb in A["blk"]:
                bb["y1"] = {s: buf(rows[s], D) for s in STREAMS}
                bb["y2"] = {s: buf(rows[s], D) for s in STREAMS}
            for bb in A["sblk"]:
                bb["y"] = buf(B * S, D)
        A["site"] = {"x_in": self._site_alloc(P["x_in"], rows["img"]), "c_in": self._site_alloc(P["c_in"], rows["txt"]),
                     "proj_out": self._site_alloc(P["proj_out"], rows["img"])}
        self.in_grad = P["x_in"].lora is not None or P["c_in"].lora is not None
        self.full_bwd = self.in_grad or self.cond
        if self.full_bwd and Ld == 0:
            raise NotImplementedError("LoRA on the embedders / conditioning head of a FLUX model without double-stream blocks")
        if kext_s:
            A["ext3_j"] = buf(B * S, 3 * kext_s, zero=True)
            A["Vt_j"] = (buf(3 * rp_s, mpj, zero=True), buf(3 * rp_s, mpj, zero=True))
        A["dJ"] = [buf(B * S, D, zero=True), buf(B * S, D, zero=True)]
        A["dyg_j"] = buf(B * S, D, zero=True)
        A["dxm_j"] = buf(B * S, D)
        self.kext_s = kext_s
        self.fwd = _Prog()
        self.bwd = _Prog()
        self._build_forward(P)
        self._build_backward(P)

    # ------------------------------------------------------------------ forward
    def _gemv(self, p, P, key, x, K, N, silu, out):
        p.c(lib.qfx_mod_gemv, _ptr(x), self.B, K, _ptr(P[key + "_Wp"]), _ptr(P[key + "_bp"]), 1, N, silu, _ptr(out))

    def _cond_hip(self, p, P):
        A, B, D = self.A, self.B, self.D
        cfg = self.model.config
        Ld, Ls = cfg.num_layers, cfg.num_single_layers
        self._gemv(p, P, "t1", A["tproj"], 256, D, 0, A["t1"])
        self._gemv(p, P, "t2", A["t1"], D, D, 1, A["t2"])
        self._gemv(p, P, "p1", A["pooled"], cfg.pooled_projection_dim, D, 0, A["p1"])
        self._gemv(p, P, "p2", A["p1"], D, D, 1, A["p2"])
        n = B * D
        if cfg.guidance_embeds:
            p.c(lib.qfx_timestep_embed, _ptr(A["gd"]), B, 256, 1.0, 1000.0, _ptr(A["gproj"]))
            self._gemv(p, P, "g1", A["gproj"], 256, D, 0, A["g1"])
            self._gemv(p, P, "g2", A["g1"], D, D, 1, A["g2"])
            p.c(lib.qfx_add3_bf16, _ptr(A["t2"]), _ptr(A["g2"]), _ptr(A["p2"]), _ptr(A["temb"]), n)
        else:
            p.c(lib.qfx_add3_bf16, _ptr(A["t2"]), _ptr(A["p2"]), None, _ptr(A["temb"]), n)
        if Ld:
            p.c(lib.qfx_mod_gemv, _ptr(A["temb"]), B, D, _ptr(P["mod_W"]), _ptr(P["mod_b"]), 2 * Ld, 6 * D, 1, _ptr(A["mods"]))
        if Ls:
            p.c(lib.qfx_mod_gemv, _ptr(A["temb"]), B, D, _ptr(P["smod_W"]), _ptr(P["smod_b"]), Ls, 3 * D, 1, _ptr(A["smods"]))
        self._gemv(p, P, "norm_out", A["temb"], D, 2 * D, 1, A["mod_out"])

    def _build_forward(self, P):
        A, B, D, S, T, S_i = self.A, self.B, self.D, self.S, self.T, self.S_i
        p = self.fwd
        cfg = self.model.config
        Ld, Ls = cfg.num_layers, cfg.num_single_layers
        rows, rpb, off = self.rows, self.rpb, self.off
        eps = 1e-6
        self._emit_dropout_advance(p)
        # ---- temb = time_emb(+ guidance_emb) + pooled text emb   (CombinedTimestep(Guidance)TextProjEmbeddings)
        p.c(lib.qfx_timestep_embed, _ptr(A["t"]), B, 256, 1.0, 1000.0, _ptr(A["tproj"]))
        if self.cond:   # adapters on the conditioning head: base GEMVs + the banks' rank-r launches (cond_hip.py)
            if cfg.guidance_embeds:
                p.c(lib.qfx_timestep_embed, _ptr(A["gd"]), B, 256, 1.0, 1000.0, _ptr(A["gproj"]))
            self.cond_head.emit_forward(p)
        else:
            self._cond_hip(p, P)
        # ---- embedders; with no double blocks the embeddings go straight into the joint buffer
        if Ld == 0 and Ls == 0:
            raise NotImplementedError("FLUX model without any transformer block")
        first_out = {s: ((A["X"][s][0], (0, 0)) if Ld else (A["J"][0], (S, off[s]))) for s in STREAMS}
        site = A["site"]
        kw = self._adapter_fwd(p, P["x_in"], A["in_img"], cfg.in_channels, rows["img"], site["x_in"].U, site["x_in"].ext)
        self._gemm(p, A1=A["in_img"], lda1=cfg.in_channels, B1=P["x_in"].W, K1=cfg.in_channels, M=rows["img"], N=D,
                   C_=first_out["img"][0], ldc=D, bias=P["x_in"].b, rpb=rpb["img"], c_map=first_out["img"][1], row_mask=self.rmask["img"], **kw)
        kw = self._adapter_fwd(p, P["c_in"], A["in_txt"], P["c_in"].K, rows["txt"], site["c_in"].U, site["c_in"].ext)
        self._gemm(p, A1=A["in_txt"], lda1=P["c_in"].K, B1=P["c_in"].W, K1=P["c_in"].K, M=rows["txt"], N=D,
                   C_=first_out["txt"][0], ldc=D, bias=P["c_in"].b, rpb=rpb["txt"], c_map=first_out["txt"][1], **kw)
        self.attn_args, self.attn_hl_qkv = [], []
        for i in range(Ld):
            mods = {"img": A["mods"][2 * i], "txt": A["mods"][2 * i + 1]}
            to_joint = (i + 1 == Ld) and Ls > 0
            x_out = {s: ((A["J"][0], (S, off[s])) if to_joint else (A["X"][s][i + 1], (0, 0))) for s in STREAMS}
            self._emit_double_fwd(p, P["blocks"][i], A["blk"][i], mods, {s: A["X"][s][i] for s in STREAMS}, x_out,
                                  last=(i + 1 == Ld and Ls == 0), norm_flags=self.NORM_FLAGS)
        self.sattn_args = []
        for i in range(Ls):
            self._emit_single_fwd(p, P["singles"][i], A["sblk"][i], A["smods"][i], A["J"][i], A["J"][i + 1])
        # ---- norm_out + proj_out on the image rows of the joint buffer (per sample: contiguous row ranges)
        if Ls:
            mo, JL = A["mod_out"][0], A["J"][Ls]
            for b in range(B):
                p.c(lib.qfx_ln_modulate_fwd, _ptr(JL[b * S + T:]), _ptr(mo[b:b + 1, D:2 * D]), _ptr(mo[b:b + 1, 0:D]), 2 * D,
                    _ptr(A["xn_out"][b * S_i:]), S_i, D, S_i, eps)
        else:
            self._norm_out_fwd(p, A["X"]["img"][Ld])
        self._proj_out_fwd(p, P["proj_out"])

    def _emit_single_fwd(self, p, w, bb, mod, x, x_next):
        """FluxSingleTransformerBlock.forward (transformer_flux.py:407-436) on the joint buffer; mod [B,3D] = shift|scale|gate."""
        A, B, D, S, H, dh, T = self.A, self.B, self.D, self.S, self.H, self.dh, self.T
        eps = 1e-6
        M = B * S
        grp = w["qkv_lora"]
        xm = bb.get("xm", A["xm_j"])
        q2 = bb["qkv"].view(M, 3 * D)
        sqk2 = bb["sqk"].view(M, 2 * D)
        e3 = A.get("ext3_j")
        fused = grp is not None and self._ln_down(p, [(_ln_fwd_args(x, mod[:, 0:D], mod[:, D:2 * D], 3 * D, xm, M, D, S, eps),
                                                       dict(self._qkv_down_kw(grp, bb["Uqkv"], e3, w["qkv"]), W_fr=grp.get("A_fr")))])
        if not fused:
            p.c(lib.qfx_ln_modulate_fwd, _ptr(x), _ptr(mod[:, 0:D]), _ptr(mod[:, D:2 * D]), 3 * D, _ptr(xm), M, D, S, eps)
        groups = []
        for sec, (lw, kw) in enumerate(zip(w["qkv"], self._qkv_adapters_fwd(p, w["qkv"], grp, xm, M, bb.get("Uqkv"), e3, fused))):
            c_, ldc = (sqk2[:, sec * D:], 2 * D) if sec < 2 else (q2[:, 2 * D:], 3 * D)    # q,k: see the Qwen double block
            groups.append(_gargs(A1=xm, lda1=D, B1=lw.W, K1=D, M=M, N=D, C_=c_, ldc=ldc, bias=lw.b, **kw))
        self._gemm_group(p, groups)
        ml, wo = w["mlp"], w["out"]
        cat = bb.get("cat")                       # [M, 5D] = [attn | gelu(mlp)] when proj_out carries an adapter
        gact, ldg = (cat[:, D:], 5 * D) if cat is not None else (A["g_j"], 4 * D)
        kw = self._adapter_fwd(p, ml, xm, D, M, bb["site_mlp"].U, bb["site_mlp"].ext)
        self._gemm(p, A1=xm, lda1=D, B1=ml.W, K1=D, M=M, N=4 * D, C_=bb["h"], ldc=4 * D, bias=ml.b, epi=L.EPI_GELU, C2=gact, ldc2=ldg, **kw)
        nq, nk = w["norms"]
        p.c(lib.qfx_qk_norm_rope_fwd, _ptr(bb["qkv"]), _ptr(bb["sqk"]), _ptr(self.rope), _ptr(nq), _ptr(nk), _ptr(nq), _ptr(nk),
            B, S, T, H, dh, eps, self.NORM_FLAGS | 2, self.rope_bs)
        a = self._attn_args(bb["qkv"], bb["sqk"], bb["ao"], bb["ao"].stride(0), bb["lse"], A["dqkv"], (nq, nk, nq, nk), self.NORM_FLAGS, eps)
        self.sattn_args.append(a)
        p.c(lib.qfx_attn_fwd, C.byref(a))
        if cat is not None:
            # adapted proj_out: ONE contraction over the kept [attn | gelu(mlp)] buffer + the LoRA K-extension (base rounded first)
            kw = self._adapter_fwd(p, wo, cat, 5 * D, M, bb["site_out"].U, bb["site_out"].ext)
            if "y" in bb:
                kw.update(C2=bb["y"], ldc2=D)
            self._gemm(p, A1=cat, lda1=5 * D, B1=wo.W, ldb1=5 * D, K1=5 * D, M=M, N=D, C_=x_next, ldc=D, bias=wo.b, epi=L.EPI_GATE_RES,
                       aux=x, ldaux=D, gate=mod[:, 2 * D:3 * D], gate_bs=3 * D, rpb=S, row_mask=self.rmask["joint"], **kw)
            return
        # proj_out([attn | gelu(mlp)]) as a two-segment contraction, epilogue x + gate * y
        kw = dict(C2=bb["y"], ldc2=D) if "y" in bb else {}
        self._gemm(p, A1=bb["ao"].view(M, D), lda1=D, B1=wo.W, ldb1=5 * D, K1=D, **_kext(A["g_j"], 4 * D, wo.W[:, D:], 4 * D),
                   M=M, N=D, C_=x_next, ldc=D, bias=wo.b, epi=L.EPI_GATE_RES, aux=x, ldaux=D, gate=mod[:, 2 * D:3 * D],
                   gate_bs=3 * D, rpb=S, seg2_plain=1, row_mask=self.rmask["joint"], **kw)

    # ------------------------------------------------------------------ backward
    def _build_backward(self, P):
        A, B, D, S, H, dh, T, S_i = self.A, self.B, self.D, self.S, self.H, self.dh, self.T, self.S_i
        p = self.bwd
        cfg = self.model.config
        Ld, Ls = cfg.num_layers, cfg.num_single_layers
        rows, rpb, off = self.rows, self.rpb, self.off
        eps = 1e-6
        self._proj_out_bwd(p, P["proj_out"], masked=False)
        mo = A["mod_out"][0]
        cur = dcur = 0   # (dcur: single block 0 writes the per-stream gradients into A["dX"][s][0] / A["dyg2"][s])
        if self.cond:
            for k in ("dmods", "dsmods", "dmod_out"):
                p.py(A[k].zero_)
            dmo = A["dmod_out"][0]
        if Ls:
            # tail LayerNorm backward per sample into the joint gradient; text rows of d(joint) are zero (dead text tail)
            dJ, dyg = A["dJ"][cur], A["dyg_j"]
            gl = A["smods"][Ls - 1]
            p.py(dJ.view(B, S, D)[:, :T].zero_)
            p.py(dyg.view(B, S, D)[:, :T].zero_)
            for b in range(B):
                r0 = b * S + T
                if self.cond:
                    self._mod_grad(p, dy=A["dxn"][b * S_i:], x=A["J"][Ls][r0:], rows=S_i, rpb=S_i, dshift=dmo[b:b + 1, D:2 * D],
                                   dscale=dmo[b:b + 1, 0:D], out_bs=2 * D,
                                   row_mask=self.rmask["img"][b * S_i:] if self.rmask["img"] is not None else None)
                p.c(lib.qfx_ln_modulate_bwd, _ptr(A["dxn"][b * S_i:]), _ptr(A["J"][Ls][r0:]), _ptr(mo[b:b + 1, 0:D]), 2 * D, None,
                    _ptr(gl[b:b + 1, 2 * D:3 * D]), 3 * D, _ptr(dJ[r0:]), _ptr(dyg[r0:]), S_i, D, S_i, eps,
                    _ptr(self.rmask["img"][b * S_i:]) if self.rmask["img"] is not None else None)
            for i in range(Ls - 1, -1, -1):
                nxt = cur ^ 1
                self._emit_single_bwd(p, P["singles"][i], A["sblk"][i], self.sattn_args[i], A["smods"][i], A["J"][i],
                                      dJ_out=A["dJ"][cur], dJ_in=A["dJ"][nxt], i=i, Ld=Ld)
                p.mark(f"single_transformer_blocks.{i}.")
                cur = nxt
            if Ld == 0:
                return
        else:
            self._norm_out_bwd(p, A["X"]["img"][Ld], A["mods"][2 * (Ld - 1)][:, 5 * D:6 * D], A["dX"]["img"][dcur])
        for i in range(Ld - 1, -1, -1):
            nxt = dcur ^ 1
            mods = {"img": A["mods"][2 * i], "txt": A["mods"][2 * i + 1]}
            gate_prev = None if i == 0 else {"img": A["mods"][2 * (i - 1)][:, 5 * D:6 * D], "txt": A["mods"][2 * (i - 1) + 1][:, 5 * D:6 * D]}
            self._emit_double_bwd(p, P["blocks"][i], A["blk"][i], self.attn_args[i], self.attn_hl_qkv[i], mods, {s: A["X"][s][i] for s in STREAMS},
                                  dx2={s: A["dX"][s][dcur] for s in STREAMS}, out_dx={s: A["dX"][s][nxt] for s in STREAMS},
                                  gate_prev=gate_prev, last=(i + 1 == Ld and Ls == 0), first=(i == 0 and not self.full_bwd),
                                  norm_flags=self.NORM_FLAGS,
                                  dmods=({"img": A["dmods"][2 * i], "txt": A["dmods"][2 * i + 1]} if self.cond else None))
            p.mark(f"transformer_blocks.{i}.")
            dcur = nxt
        if self.in_grad:   # the embedders' adapters: d(block-0 input) = A["dX"][s][dcur]; their own inputs carry no gradient
            site = A["site"]
            for key, s, x, ldx in (("x_in", "img", A["in_img"], cfg.in_channels), ("c_in", "txt", A["in_txt"], P["c_in"].K)):
                self._adapter_bwd(p, P[key], A["dX"][s][dcur], D, rows[s], x, ldx, site[key].U, site[key].V, site[key].extb)
        if self.cond:
            self.cond_head.emit_backward(p)

    def _emit_single_bwd(self, p, w, bb, a, mod, x, dJ_out, dJ_in, i, Ld):
        """In: dJ_out = d(block output) [B*S,D], A["dyg_j"] = gate*dJ_out.  Out: dJ_in and A["dyg_j"] = gate_prev*dJ_in
        (or, for the first single block, the per-stream gradients of the last double block)."""
        A, B, D, S, H, dh, T, S_i = self.A, self.B, self.D, self.S, self.H, self.dh, self.T, self.S_i
        rows, rpb, off = self.rows, self.rpb, self.off
        eps = 1e-6
        M = B * S
        wo, ml = w["out"], w["mlp"]
        grp = w["qkv_lora"]
        ldA2 = A["A2"].stride(0)
        dao2 = A["dao"].view(M, D)
        dq2 = A["dqkv"].view(M, 3 * D)
        # d[attn | mlp] = (gate*dx) W_out : attention part -> dO, mlp part through gelu' -> A2[:, :4D]   (+ proj_out's adapter)
        kwa, kwm = {}, {}
        # the block's weight-gradient problems (up to 8) go out as batched launches right before the LayerNorm backward overwrites
        # dyg_j -- their operands (dyg_j, dqkv, A2, v^T scratch, the block's kept buffers) stay intact until then; one launch each
        # they were 8 x 38 latency-bound launches on the main stream (the FLUX programs keep their gradients there)
        gl = []
        if wo.lora is not None:
            sb = bb["site_out"]
            kwo = self._adapter_bwd(p, wo, A["dyg_j"], D, M, bb["cat"], 5 * D, sb.U, sb.V, sb.extb, dB=gl, dA=gl)
            kwa = dict(kwo, B2=wo.lora.WeT[:D])
            kwm = dict(kwo, B2=wo.lora.WeT[D:])
        self._gemm(p, A1=A["dyg_j"], lda1=D, B1=wo.WT, K1=D, M=M, N=D, C_=dao2, ldc=D, **kwa)
        self._gemm(p, A1=A["dyg_j"], lda1=D, B1=wo.WT[D:], K1=D, M=M, N=4 * D, C_=A["A2"], ldc=ldA2, epi=L.EPI_DGELU, aux=bb["h"],
                   ldaux=4 * D, **kwm)
        emit_attn_backward(p, a, A, self.lv.attn_bwd)      # two-pass pair, or the one-pass kernel (QFX_ATTN_BWD)
        if not a.qk_saved:
            nq, nk = w["norms"]
            p.c(lib.qfx_qk_norm_rope_bwd, _ptr(A["dqkv"]), _ptr(bb["sqk"]), _ptr(self.rope), _ptr(nq), _ptr(nk), _ptr(nq), _ptr(nk),
                B, S, T, H, dh, eps, self.NORM_FLAGS, self.rope_bs)
        K2 = 4 * D
        if grp is not None:
            dl = []     # the q / k / v down projections of dqkv: one launch
            self._qkv_adapters_bwd(p, w["qkv"], grp, dq2, M, bb["xm"], bb["Uqkv"], A["Vt_j"], A["A2"][:, 4 * D:], down=dl, grads=gl)
            _flush_batch(p, dl, L.LoraDownArgs, lib.qfx_lora_down_batch)
            self._flush_dropout(p)
            K2 = 4 * D + 3 * grp["Kext"]
        if ml.lora is not None:
            # proj_mlp's adapter: v = d(mlp pre-act) (sB)^T goes into the last K-extension columns of A2; dB / dA as for any site
            sb = bb["site_mlp"]
            self._adapter_bwd(p, ml, A["A2"], ldA2, M, bb["xm"], D, sb.U, sb.V, A["A2"][:, K2:], dB=gl, dA=gl)
            K2 += ml.lora.Kext
        # d(norm_x) = [dq|dk|dv] Wqkv + [d mlp | LoRA v] [W_mlp ; A]
        if self.model._quant == "mxfp8-fb" and D % 128 == 0 and D >= 1024:
            # low-precision trunk: the four frozen contractions as one MX-FP8 GEMM over K = 3D + 4D, adapters as its bf16 K-extension
            self.fp8._gemm_mxfp8_cat(p, [(dq2, 3 * D, 3 * D, w["qkvT"]), (A["A2"], ldA2, 4 * D, w["B2"])], M=M, N=D, C_=A["dxm_j"], ldc=D,
                                     ext=_kext(A["A2"][:, 4 * D:], ldA2, w["B2"][:, 4 * D:], K2 - 4 * D))
        else:
            self._gemm(p, A1=dq2, lda1=3 * D, B1=w["qkvT"], K1=3 * D, **_kext(A["A2"], ldA2, w["B2"], K2), M=M, N=D, C_=A["dxm_j"],
                       ldc=D, seg2_plain=1)
        if self.cond:   # d(shift, scale, gate) of the single block's AdaLayerNormZeroSingle
            dm = A["dsmods"][i]
            self._mod_grad(p, dy=A["dxm_j"], x=x, rows=M, rpb=S, dshift=dm[:, 0:D], dscale=dm[:, D:2 * D], dgate=dm[:, 2 * D:3 * D],
                           dxo=dJ_out, y=bb["y"], out_bs=3 * D, row_mask=self.rmask["joint"])
        _flush_batch(p, gl, L.LoraGradArgs, lib.qfx_lora_grad_batch)
        if i > 0:
            gp = A["smods"][i - 1][:, 2 * D:3 * D]
            p.c(lib.qfx_ln_modulate_bwd, _ptr(A["dxm_j"]), _ptr(x), _ptr(mod[:, D:2 * D]), 3 * D, _ptr(dJ_out), _ptr(gp), 3 * D,
                _ptr(dJ_in), _ptr(A["dyg_j"]), M, D, S, eps, _ptr(self.rmask["joint"]))
        elif Ld > 0:
            # hand the gradient over to the last double block: per (sample, stream) row ranges of the joint buffer
            mods_prev = {"img": A["mods"][2 * (Ld - 1)], "txt": A["mods"][2 * (Ld - 1) + 1]}
            for b in range(B):
                for s in ("txt", "img"):
                    r0, n, c0 = b * S + off[s], rpb[s], b * rpb[s]
                    gp = mods_prev[s][b:b + 1, 5 * D:6 * D]
                    p.c(lib.qfx_ln_modulate_bwd, _ptr(A["dxm_j"][r0:]), _ptr(x[r0:]), _ptr(mod[b:b + 1, D:2 * D]), 3 * D,
                        _ptr(dJ_out[r0:]), _ptr(gp), 6 * D, _ptr(A["dX"][s][0][c0:]), _ptr(A["dyg2"][s][c0:]), n, D, n, eps,
                        _ptr(self.rmask[s][c0:]) if self.rmask[s] is not None else None)

    def set_multires(self, img_ids_b: torch.Tensor, valid_lens):
        """Per-step dynamic state of the multi-resolution path (transformer_flux_custom.py:499-616): per-sample RoPE with
        identity rotation on padding, additive key mask (0 / -inf), row masks of the padded image tokens."""
        cfg = self.model.config
        B, S, T, S_i = self.B, self.S, self.T, self.S_i
        dev = self.model.device
        rope = torch.zeros(B, S, self.dh // 2, 2)
        rope[..., 0] = 1.0
        km = torch.zeros(B, S)
        rm = torch.zeros(B, S_i)
        txt = torch.zeros(T, 3)
        for b in range(B):
            n = int(valid_lens[b])
            ids = torch.cat([txt, img_ids_b[b, :n].float().cpu()], dim=0)
            rope[b, : T + n] = flux_joint_rope(ids, cfg.axes_dims_rope)
            km[b, T + n:] = float("-inf")
            rm[b, :n] = 1.0
        A = self.A
        A["rope_b"].copy_(rope.to(dev, non_blocking=True))
        A["kmask"].copy_(km.to(dev, non_blocking=True))
        A["rm_img"].copy_(rm.reshape(-1).to(dev, non_blocking=True))
        rj = torch.ones(B, S)
        rj[:, T:] = rm
        A["rm_joint"].copy_(rj.reshape(-1).to(dev, non_blocking=True))

    # ------------------------------------------------------------------ execution
    def run_forward(self, inputs, encoder_hidden_states, timestep):
        hidden_states, pooled, guidance = inputs
        A = self.A
        self._copy_rows(A["in_img"].view(self.B, self.S_i, -1), hidden_states)
        A["in_txt"].view(self.B, self.T, -1)[:, :, : encoder_hidden_states.shape[-1]].copy_(encoder_hidden_states)
        A["pooled"].copy_(pooled)
        A["t"].copy_(timestep.reshape(self.B).to(F32))
        if guidance is not None:
            A["gd"].copy_(guidance.reshape(self.B).to(F32))
        self.model.refresh_lora_operands()
        self._sync_dropout()
        self.fwd.run()
        return A["out"].view(self.B, self.S_i, -1)
