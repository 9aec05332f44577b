"""The Qwen launch plan: for one shape signature a persistent HBM arena plus the forward and the backward launch program
(flat lists of libqfx C-ABI calls with pre-built argument structs), built once from the model's prepared weights and replayed
every step; and the autograd node that runs a plan.  The FLUX plan (flux.py) subclasses it for the shared double-stream blocks."""
from __future__ import annotations

import ctypes as C
import math
from collections import namedtuple

import torch

from .. import _lib as L
from .. import dropout as DR
from .. import levers, ops
from ..cond_hip import CondHeadHip
from ..rope import normalize_img_shapes, qwen_joint_rope
from .emit import (_down_args, _emit_or_defer, _flush_batch, _flush_dropout, _flush_head_reduce, _flush_ln, _flush_mod_grad, _gargs, _grad_args,
                   _head_reduce_args, _kext, _ln_bwd_args, _ln_fwd_args, _mod_grad_args, emit_attn_backward)
from .fp8 import _Fp8Trunk
from .prog import _Prog, _ceil, _ptr

lib = L.lib
BF = torch.bfloat16
F32 = torch.float32
STREAMS = ("img", "txt")
_NONE = dict.fromkeys(STREAMS)      # stands in for the per-stream rank-r scratch of a plan without adapters

# Private rank-r buffers of one stand-alone adapted linear: K-extension images of the forward (ext) and backward (extb) GEMM,
# transposed hi/lo splits of u = x A^T (kept for dB) and v = dy (sB)^T (for dA).  All None for a linear without an adapter.
_Site = namedtuple("_Site", "ext extb U V", defaults=(None,) * 4)


class _QwenPlan:
    """Launch programs (forward, backward) + persistent arena for one shape signature."""

    side_grads = False        # see _init_side_grads (plans that do not call it keep every launch on the main stream)
    _side_q = ()

    def __init__(self, model, B: int, S_i: int, T: int, shapes, multires: bool = False):
        self._setup(model, B, S_i, T)
        cfg = model.config
        D, S = self.D, self.S
        buf = self.buf
        rows = self.rows
        Lyr = cfg.num_layers
        Cin, Cout, Jd = cfg.in_channels, model.proj_out.out_features, cfg.joint_attention_dim
        P = model._prepared
        A = self.A
        self.multires = multires
        self.rm_txt0 = None
        if multires:
            self.rm_txt0 = self._alloc_multires(rm_txt0=B * T)      # row mask of the padded text tokens (applied once, after txt_in)
        else:
            self.rope = qwen_joint_rope(shapes, T, cfg.axes_dims_rope).to(model.device)
            assert self.rope.shape == (S, self.dh // 2, 2)
        A["in_img"] = buf(B * S_i, Cin); A["in_txt"] = buf(B * T, Jd); A["t"] = buf(B, dtype=F32)
        A["tproj"] = buf(B, 256); A["t1"] = buf(1, B, D); A["temb"] = buf(1, B, D)
        A["txt_n"] = buf(B * T, Jd)
        A["X"] = {s: [buf(rows[s], D) for _ in range(Lyr + 1)] for s in ("img", "txt")}
        A["mods"] = buf(2 * Lyr, B, 6 * D); A["mod_out"] = buf(1, B, 2 * D)
        A["xn_out"] = buf(B * S_i, D); A["out"] = buf(B * S_i, Cout)
        A["dpred"] = buf(B * S_i, Cout); A["dxn"] = buf(B * S_i, D)
        A["blk"] = [self._alloc_double_block(w) for w in P["blocks"]]
        self._alloc_double_scratch(P["blocks"])
        self.cond = model.cond_lora
        if self.cond:
            A["dmods"] = buf(2 * Lyr, B, 6 * D, dtype=F32, zero=True)
            A["dmod_out"] = buf(1, B, 2 * D, dtype=F32, zero=True)
            te = model.time_text_embed.timestep_embedder
            self.cond_head = CondHeadHip(
                model, B, D, chains=[(te.linear_1, te.linear_2, A["tproj"], A["t1"], A["temb"])], temb=A["temb"],
                banks=[([m for blk in model.transformer_blocks for m in (blk.img_mod[1], blk.txt_mod[1])], A["mods"], A["dmods"]),
                       ([model.norm_out.linear], A["mod_out"], A["dmod_out"])], buf=buf)
            for bb in A["blk"]:    # pre-gate outputs of the two gated linears of a block (d gate = sum_rows dx_out * y)
                bb["y1"] = {s: buf(rows[s], D) for s in ("img", "txt")}
                bb["y2"] = {s: buf(rows[s], D) for s in ("img", "txt")}
        A["site"] = {"img_in": self._site_alloc(P["img_in"], rows["img"]), "txt_in": self._site_alloc(P["txt_in"], rows["txt"]),
                     "proj_out": self._site_alloc(P["proj_out"], rows["img"])}
        self.in_grad = P["img_in"].lora is not None or P["txt_in"].lora is not None   # the gradient must reach the block-0 inputs
        self.full_bwd = self.in_grad or self.cond      # block 0 runs its complete backward (d xm1 feeds d shift1 / d scale1)
        if multires and P["txt_in"].lora is not None:
            raise NotImplementedError("LoRA on txt_in with the multi-resolution Qwen model (the reference has no training caller for it)")
        self.fwd = _Prog()
        self.bwd = _Prog()
        self._init_side_grads(P["blocks"], type(self) is _QwenPlan)
        self._build_forward(P)
        self._build_backward(P)

    def _init_side_grads(self, blocks, allowed):
        """LoRA weight gradients are leaves of the backward: the batched lora_grad launch of block i goes to a low-priority side
        stream and overlaps the first two GEMMs of block i-1 (persistent 240-block grids leave 16 CUs idle); the main stream joins
        it right before block i-1 first overwrites one of its operands (dyg1).  With feed-forward adapters dh and their v^T scratch
        alternate by block parity too, the join sits at the top of the block (dh is the first thing a block's backward overwrites),
        and the launches that read dyg2 stay on the main stream.  QFX_SIDE_GRADS=0 keeps everything on the main stream."""
        ff = any(w[s + k].lora is not None for w in blocks for s in ("img", "txt") for k in (".fc1", ".fc2"))
        self._ff_side = bool(ff)      # feed-forward adapters: dh / v^T(fc1, fc2) join the parity-alternated scratch, the join moves to the block top
        self.side_grads = bool(allowed and self.has_lora and self.lv.side_grads
                               and (not ff or self.lv.side_grads_ff))
        self._side_q = []              # (event, prefix) of the blocks whose gradient launches are in flight on the side stream
        if self.side_grads:
            dev = self.model.device
            # an ordinary low-priority stream: a CU-masked queue slowed the whole step (profiles/HISTORY.md, profiles/r01_cu_mask_probe.json)
            self.bwd.side = ops.side_stream(dev)
            self._ev_fork = torch.cuda.Event()
            # the scratch operands of those launches (dyg1, dqkv, v^T) alternate between two copies by block parity, so a launch
            # has a whole block of main-stream work to hide under (on the 16 idle CUs it runs ~5x longer than alone)
            A = self.A
            for name in ("dyg1", "dqkv", "Vt", "VtO") + (("dh", "VtF1", "VtF2") if ff else ()):
                src = A[name]
                if isinstance(src, dict):
                    A[name + "#1"] = {s: (tuple(torch.zeros_like(t) for t in v) if isinstance(v, tuple) else torch.zeros_like(v))
                                      for s, v in src.items()}
                else:
                    A[name + "#1"] = torch.zeros_like(src)

    def _fuse_qk_bwd(self, a, sqk, norms, norm_flags, eps):
        """Backward of the QK RMSNorm + RoPE in the epilogues of qfx_attn_bwd_dq / _dkv (one pass over dqkv and a launch less per
        block; QFX_FUSE_QKNORM_BWD=0 keeps the separate qfx_qk_norm_rope_bwd launch)."""
        if not self.lv.fuse_qknorm_bwd:
            return
        nq_t, nk_t, nq_i, nk_i = norms
        a.qk_saved, a.ld_saved = _ptr(sqk), 2 * self.D
        a.rope, a.rope_bstride = _ptr(self.rope), self.rope_bs
        a.wq_txt, a.wk_txt, a.wq_img, a.wk_img = _ptr(nq_t), _ptr(nk_t), _ptr(nq_i), _ptr(nk_i)
        a.T, a.norm_flags, a.norm_eps = self.T, norm_flags & 1, eps

    def _head_lora_slots(self, a, w, live):
        """Fill the qfx_head_lora slots of a block's attention arguments (forward slot 0: out-projection adapter; backward slots
        1-3: q / k / v adapters, which need the fused QK-norm backward).  Returns {stream: H} for the streams whose out-projection
        down projection now rides in qfx_attn_fwd, and {stream: Rp} for the streams whose q / k / v down projections ride in the
        attention backward."""
        # the fused projections pick the text / image adapter by `row >= a.T`: set it HERE, not only in _fuse_qk_bwd (which returns
        # early under QFX_FUSE_QKNORM_BWD=0 and used to leave T = 0: every text row then took the image adapter -- ADVICE r4)
        a.T = self.T
        if not self.head_lora:
            return {}, {}
        A, B, S, H = self.A, self.B, self.S, self.H
        out, out_qkv = {}, {}
        los = {s: w[s + ".o"].lora for s in live}
        rps = {lo.Rp for lo in los.values() if lo is not None}
        if len(rps) == 1:
            Rp = rps.pop()
            hl = a.hl[0]
            hl.part, hl.part_hstride, hl.ld_part, hl.c0, hl.R = _ptr(A["hl_o"]), B * S * A["hl_o"].shape[2], A["hl_o"].shape[2], 0, Rp
            for si, s in enumerate(("img", "txt")):
                lo = los.get(s)
                if lo is not None and lo.A_hl is not None:
                    hl.w_pk[si] = _ptr(lo.A_hl)
                    out[s] = H
        if a.qk_saved:
            grp = {s: w[s + ".qkv_lora"] for s in ("img", "txt")}
            full = {s: g for s, g in grp.items() if g is not None and all(
                w[s + ".qkv"][sec].lora is not None and w[s + ".qkv"][sec].lora.Bt_hl is not None for sec in range(3))}
            rps = {g["Rp"] for g in full.values()}
            if len(rps) == 1:
                Rp = rps.pop()
                ld = A["hl_qkv"].shape[2]
                for sec in range(3):
                    hl = a.hl[1 + sec]
                    hl.part, hl.part_hstride, hl.ld_part, hl.c0, hl.R = _ptr(A["hl_qkv"]), B * S * ld, ld, sec * Rp, Rp
                    for si, s in enumerate(("img", "txt")):
                        if s in full:
                            lo = w[s + ".qkv"][sec].lora
                            hl.w_pk[si] = _ptr(lo.Bt_hl)
                out_qkv = {s: Rp for s in full}
        return out, out_qkv

    def _sb(self, name, par):
        """Scratch buffer `name` of block parity `par` (second copies exist only with side-stream gradient launches)."""
        return self.A[name + f"#{par}"] if (par and self.side_grads) else self.A.get(name)   # v^T scratch exists only with adapters

    def _side_fork(self):
        self._ev_fork.record(torch.cuda.current_stream())
        self._ev_fork.wait(self.bwd.side)

    def _side_join(self, p, keep=0):
        """Emit the joins with the oldest in-flight side-stream gradient launches until at most `keep` stay in flight, each
        followed by the mark that its block's gradients are final."""
        while len(self._side_q) > keep:
            ev, prefix = self._side_q.pop(0)
            p.py(lambda ev=ev: ev.wait(torch.cuda.current_stream()))
            if prefix is not None:
                p.mark(prefix)

    def _setup(self, model, B, S_i, T):
        self.model = model
        cfg = model.config
        dev = model.device
        self.B, self.S_i, self.T = B, S_i, T
        self.H, self.dh = cfg.num_attention_heads, cfg.attention_head_dim
        self.D = self.H * self.dh
        self.S = T + S_i
        self.S_pad = _ceil(self.S, 64)
        if B > 8:
            raise NotImplementedError("per-GPU batch > 8 (modulation GEMV holds <= 8 rows in LDS)")

        def buf(*shape, dtype=BF, zero=False):
            return (torch.zeros if zero else torch.empty)(*shape, dtype=dtype, device=dev)

        self.buf = buf
        self.rows = {"img": B * S_i, "txt": B * T}
        self.rpb = {"img": S_i, "txt": T}
        self.off = {"img": T, "txt": 0}
        self.A = {}
        self.lv = levers.read()   # the one look at the environment: every lever this plan consults
        self.fp8 = _Fp8Trunk(self)
        # dropout on the adapters' rank-r activation (model.set_lora_dropout): the device state, None = off (nothing below emits)
        self.dropout = model._dropout
        self._dq = []             # dropout problems of deferred producers, flushed behind the producers' own flush
        if self.dropout is not None:
            if model._quant is not None:
                raise NotImplementedError(DR.MXFP8_REFUSAL)
            self._mod_names = {id(m): n for n, m in model.named_modules()}
        self.head_lora = False    # set by _alloc_double_scratch
        self.rope_bs = 0          # per-sample RoPE stride (multi-resolution plans set it)
        self.rmask = {"img": None, "txt": None, "joint": None}   # fp32 row masks of padded tokens (multi-resolution)
        self.kmask = None         # additive fp32 key mask [B,S] (multi-resolution)

    def _alloc_multires(self, **extra):
        """Per-batch contents of a multi-resolution plan, filled by set_multires(): per-sample RoPE (identity on unrotated rows),
        additive key mask, row mask of the padded image tokens (every block) and one further fp32 row mask `name=rows`, returned."""
        A, buf, B, S = self.A, self.buf, self.B, self.S
        A["rope_b"] = buf(B, S, self.dh // 2, 2, dtype=F32)
        A["kmask"] = buf(B, S, dtype=F32, zero=True)
        A["rm_img"] = buf(B * self.S_i, dtype=F32)
        self.rope, self.rope_bs = A["rope_b"], S * (self.dh // 2) * 2
        self.kmask = A["kmask"]
        self.rmask["img"] = A["rm_img"]
        (name, n), = extra.items()
        A[name] = buf(n, dtype=F32)
        return A[name]

    def _alloc_double_block(self, w):
        """Per-block saved activations of a double-stream block."""
        buf, rows, B, S, D, H, S_pad = self.buf, self.rows, self.B, self.S, self.D, self.H, self.S_pad
        b = dict(qkv=buf(B, S, 3 * D), sqk=buf(B, S, 2 * D), ao=buf(B, S, D), lse=buf(B, H, S_pad, dtype=F32, zero=True),
                 x1={s: buf(rows[s], D) for s in ("img", "txt")}, h={s: buf(rows[s], 4 * D) for s in ("img", "txt")})
        for s in ("img", "txt"):
            grp = w[s + ".qkv_lora"]
            mp = _ceil(rows[s], 128)
            if grp is not None:
                b["xm1." + s] = buf(rows[s], D)
                b["Uqkv." + s] = (buf(3 * grp["Rp"], mp, zero=True), buf(3 * grp["Rp"], mp, zero=True))   # u^T hi/lo
            if w[s + ".o"].lora is not None:
                rp_o = w[s + ".o"].lora.Rp
                b["Uo." + s] = (buf(rp_o, mp, zero=True), buf(rp_o, mp, zero=True))
            # feed-forward adapters: their inputs (LN2 output / GELU output) are scratch otherwise and must be kept for dA
            for key, kept, width, u in ((".fc1", "xm2.", D, "Uf1."), (".fc2", "g.", 4 * D, "Uf2.")):
                if w[s + key].lora is not None:
                    rp = w[s + key].lora.Rp
                    b[kept + s] = buf(rows[s], width)
                    b[u + s] = (buf(rp, mp, zero=True), buf(rp, mp, zero=True))
        return b

    def _alloc_double_scratch(self, blocks):
        """Scratch shared by all double-stream blocks (forward + backward)."""
        buf, rows, B, S, D, H, dh, S_pad, A = self.buf, self.rows, self.B, self.S, self.D, self.H, self.dh, self.S_pad, self.A
        A["xm"] = {s: buf(rows[s], D) for s in ("img", "txt")}
        A["g"] = {s: buf(rows[s], 4 * D) for s in ("img", "txt")}
        kext_max = 0
        rp_max = 0
        for w in blocks:   # LoRA scratch (pad columns stay zero forever)
            for s in ("img", "txt"):
                if w[s + ".qkv_lora"] is not None:
                    kext_max = max(kext_max, w[s + ".qkv_lora"]["Kext"]); rp_max = max(rp_max, w[s + ".qkv_lora"]["Rp"])
                for key in (".o", ".fc1", ".fc2"):
                    if w[s + key].lora is not None:
                        kext_max = max(kext_max, w[s + key].lora.Kext); rp_max = max(rp_max, w[s + key].lora.Rp)
        self.has_lora = kext_max > 0
        if self.has_lora:
            A["ext3"] = {s: buf(rows[s], 3 * kext_max, zero=True) for s in ("img", "txt")}
            A["ext1"] = {s: buf(rows[s], kext_max, zero=True) for s in ("img", "txt")}
            for name in ("VtO", "VtF1", "VtF2"):   # one v^T scratch per adapter site: the deferred dA launches read them at block end
                A[name] = {s: (buf(rp_max, _ceil(rows[s], 128), zero=True), buf(rp_max, _ceil(rows[s], 128), zero=True))
                           for s in ("img", "txt")}
            A["Vt"] = {s: (buf(3 * rp_max, _ceil(rows[s], 128), zero=True), buf(3 * rp_max, _ceil(rows[s], 128), zero=True))
                       for s in ("img", "txt")}   # v^T hi/lo scratch (pad columns stay zero)
        # Round 4 (ABI 6): the rank-r down projections whose input an attention kernel holds in registers -- u = ao A_o^T in the
        # forward, v = d(pre-norm q | k) , dV times (sB)^T in the backward -- ride in that kernel's epilogue as per-head partial sums
        # (qfx_head_lora) and a small reduce launch writes what qfx_lora_down wrote: 2 of the 3 qfx_lora_down launches per block go.
        # Needs T % 16 == 0 (a 16-row fragment is all text or all image), rank <= 32, the bf16 trunk (the MX-FP8 trunk's down
        # projections also quantise their input), and -- backward -- the QK-norm backward fused into the same epilogues.
        self.head_lora = (self.has_lora and self.lv.fuse_head_lora and self.T % 16 == 0 and 0 < rp_max <= 32
                          and self.model._quant is None)
        if self.head_lora:
            A["hl_o"] = buf(H, B * S, rp_max, dtype=F32, zero=True)
            A["hl_qkv"] = buf(H, B * S, 3 * rp_max, dtype=F32, zero=True)
        A["dX"] = {s: [buf(rows[s], D), buf(rows[s], D)] for s in ("img", "txt")}
        A["dyg2"] = {s: buf(rows[s], D) for s in ("img", "txt")}
        A["dyg1"] = {s: buf(rows[s], D) for s in ("img", "txt")}
        A["dx1"] = {s: buf(rows[s], D) for s in ("img", "txt")}
        A["dh"] = {s: buf(rows[s], 4 * D) for s in ("img", "txt")}
        A["dxm"] = {s: buf(rows[s], D) for s in ("img", "txt")}
        A["dao"] = buf(B, S, D, zero=True)
        A["dsum"] = buf(B, H, S_pad, dtype=F32, zero=True)
        A["dqkv"] = buf(B, S, 3 * D)

    def _gemm(self, prog, **kw):
        self._gemm_group(prog, [_gargs(**kw)])

    def _gemm_group(self, prog, groups):
        """One grid for several independent GEMMs with the same epilogue (image+text streams, q/k/v)."""
        if self.fp8.takes(prog, groups):
            self.fp8._gemm_group_mxfp8(prog, groups)
        else:
            self.fp8.check_bf16(groups)
            if len(groups) == 1:
                prog.keep.append(groups[0].args)
                prog.c(lib.qfx_gemm_bf16, C.byref(groups[0].args))
            else:
                arr = (L.GemmArgs * len(groups))(*(op.args for op in groups))
                prog.keep.append(arr)
                prog.c(lib.qfx_gemm_grouped, arr, len(groups))
        self.fp8.next_group()

    def _down(self, prog, *, defer=None, site=None, **kw):
        """site: the dropout keys of the producer's adapters (_site_keys), one per group of its output columns."""
        _emit_or_defer(prog, _down_args(**kw), lib.qfx_lora_down, defer)
        if self.dropout is not None and kw.get("Ut") is not None:
            q = self._dq if defer is not None else []
            self._drop_add(ext=kw.get("ext"), ld_ext=kw.get("ld_ext", 0), Ut=kw["Ut"], M=kw["M"], R=kw["R"], group_R=kw.get("group_R"),
                           group_stride=kw.get("group_stride", 0), sites=site, queue=q)
            if defer is None:      # a launch of its own: so is its dropout
                self._flush_dropout(prog, q)

    # ------------------------------------------------------------------ dropout on the rank-r activation (qflux_amd.dropout)
    def _site_keys(self, *lws):
        """The generator keys of the adapters of the prepared linears `lws` (0 for one without adapter); None with dropout off."""
        if self.dropout is None:
            return None
        return tuple(0 if lw.lora is None else DR.site_key(self._mod_names[id(lw.mod)]) for lw in lws)

    def _drop_add(self, *, ext, ld_ext, Ut, M, R, sites, group_R=None, group_stride=0, queue=None):
        """Collect the dropout problem of one rank-r producer call: its transposed split Ut and K-extension image ext (the fields
        of the producer's own arguments) are multiplied in place by f[token, rank] in the next _flush_dropout.  M rows = B samples of
        M / B tokens each, forward and backward alike, so both passes regenerate the same mask."""
        if self.dropout is None:
            return
        a = ops.lora_dropout_args(Ut=Ut, M=M, R=R, rows_per_batch=M // self.B, sites=sites, ext=ext, ld_ext=ld_ext,
                                  group_R=group_R, group_stride=group_stride)
        (self._dq if queue is None else queue).append(a)

    def _flush_dropout(self, prog, queue=None):
        if self.dropout is not None:
            _flush_dropout(prog, self._dq if queue is None else queue, self.dropout)

    def _emit_dropout_advance(self, prog):
        """First call of a forward program: the state's step moves on the device, so eager and captured replays advance alike."""
        if self.dropout is not None:
            prog.c(lib.qfx_lora_dropout_advance, _ptr(self.dropout.words))

    def _sync_dropout(self):
        """Before a forward program runs: the state's `active` word follows the training-mode switch (nn.Dropout's rule).  Not
        while a graph is being captured: the write would be replayed; the captured step sets the word before it replays."""
        st = self.dropout
        if st is not None and not torch.cuda.is_current_stream_capturing():
            st.set_active(st.enabled and self.model.training)

    def _ln_down(self, prog, entries):
        """LayerNorm+modulate of up to two streams with the LoRA down projection of the adapted ones fused in (qfx_ln_down_fwd).
        entries: [(LnFwdArgs, None | dict(W_hi, W_lo, ldw, R, Ut, ext, ld_ext, group_R, group_stride))].  Returns False when the
        shape is outside the fused kernel's range (caller falls back to the two separate launches)."""
        D = entries[0][0].D
        rs = {d["R"] for _, d in entries if d is not None}
        # (streams without adapters take the same kernel as plain LayerNorm rows, so that a zero adapter reproduces the frozen
        # model bit for bit: one LayerNorm arithmetic per site, adapted or not)
        if not self.lv.fuse_ln_down or len(rs) > 1 or (rs and max(rs) > 48) or D % 256 or D > 3072 or len(entries) > 2:
            return False
        arr = (L.LnDownArgs * len(entries))()
        for i, (ln, d) in enumerate(entries):
            C.memmove(C.byref(arr[i].ln), C.byref(ln), C.sizeof(L.LnFwdArgs))
            if d is not None:
                a = arr[i]
                a.W_hi, a.W_lo, a.ldw, a.R = _ptr(d["W_hi"]), _ptr(d["W_lo"]), d["ldw"], d["R"]
                a.W_fr = _ptr(d.get("W_fr"))
                a.ext, a.ld_ext = _ptr(d["ext"]), d["ld_ext"]
                a.Ut_hi, a.Ut_lo, a.ld_ut = _ptr(d["Ut"][0]), _ptr(d["Ut"][1]), d["Ut"][0].stride(0)
                a.group_R, a.group_stride = d.get("group_R", d["R"]), d.get("group_stride", 0)
        prog.keep.append(arr)
        prog.c(lib.qfx_ln_down_fwd, arr, len(entries))
        if self.dropout is not None:
            q = []
            for ln, d in entries:
                if d is not None:
                    self._drop_add(ext=d["ext"], ld_ext=d["ld_ext"], Ut=d["Ut"], M=ln.rows, R=d["R"], group_R=d.get("group_R"),
                                   group_stride=d.get("group_stride", 0), sites=d["site"], queue=q)
            self._flush_dropout(prog, q)
        return True

    def _grad(self, prog, *, defer=None, **kw):
        _emit_or_defer(prog, _grad_args(prog, self.lv.grad_det, **kw), lib.qfx_lora_grad, defer)

    def _mod_grad(self, prog, *, defer=None, **kw):
        """defer: list collecting the problem for ONE batched launch (_flush_mod_grad) -- the image and text stream of a block."""
        _emit_or_defer(prog, _mod_grad_args(self.D, **kw), lib.qfx_mod_grad, defer)

    # ------------------------------------------------------------------ adapted linears
    def _site_alloc(self, lw, M):
        """The private rank-r buffers (_Site) of one stand-alone adapted linear with M input rows: embedders, output projection ..."""
        if lw.lora is None:
            return _Site()
        lo, buf, mp = lw.lora, self.buf, _ceil(M, 128)
        return _Site(ext=buf(M, lo.Kext, zero=True), extb=buf(M, lo.Kext, zero=True),
                     U=(buf(lo.Rp, mp, zero=True), buf(lo.Rp, mp, zero=True)), V=(buf(lo.Rp, mp, zero=True), buf(lo.Rp, mp, zero=True)))

    def _adapter_fwd(self, p, lw, X, ldx, M, U, ext, *, defer=None, rmap=(None, (0, 0)), xq=None):
        """Forward of the adapter of linear `lw` (none: nothing, {}): u = x A^T (fp32-accurate) into the hi/lo pair U (kept for dB)
        and the K-extension image `ext`; returns the K-extension keywords of the linear's GEMM.  defer: list that collects the down
        projection for a batched launch by the caller; rmap = (rows per sample, (joint rows per sample, offset)) when X is a stream's
        rows of a joint buffer; xq: see _down_args."""
        lo = lw.lora
        if lo is None:
            return {}
        self._down(p, X=X, ldx=ldx, M=M, K=lo.A_hi.shape[1], W_hi=lo.A_hi, W_lo=lo.A_lo, ldw=lo.A_hi.stride(0), R=lo.Rp, Ut=U,
                   ext=ext, ld_ext=ext.stride(0), rpb=rmap[0], x_map=rmap[1], xq=xq, defer=defer, site=self._site_keys(lw))
        return _kext(ext, ext.stride(0), lo.We, lo.Kext)

    def _adapter_bwd(self, p, lw, dY, ldy, M, Xin, ldxin, U, V, ext, *, down=None, dB=None, dA=None, rmap=(None, (0, 0))):
        """Backward of the adapter of linear `lw` (none: nothing, {}): v = dy (sB)^T into the first Rp rows of the hi/lo pair V and
        the K-extension image `ext`, dB += dy^T u, dA += v^T x; returns the K-extension keywords of the linear's dX GEMM.  down / dB /
        dA: lists that collect the down projection and the two weight-gradient problems for batched launches by the caller (who keeps
        dY, Xin, U and V intact until it flushes).  rmap: as in _adapter_fwd, for the adapter's input Xin."""
        lo = lw.lora
        if lo is None:
            return {}
        K, Vt = lo.A_hi.shape[1], (V[0][:lo.Rp], V[1][:lo.Rp])
        self._down(p, X=dY, ldx=ldy, M=M, K=lw.N, W_hi=lo.Bt_hi, W_lo=lo.Bt_lo, ldw=lo.Bt_hi.stride(0), R=lo.Rp, Ut=Vt,
                   ext=ext, ld_ext=ext.stride(0), defer=down, site=self._site_keys(lw))
        self._grad(p, Vt=U, R=lo.Rp, r_valid=lo.r, X=dY, ldx=ldy, M=M, K=lw.N, G=lo.gB, g_sr=1, g_sc=lo.r, out_scale=lo.scale, defer=dB)
        self._grad(p, Vt=Vt, R=lo.Rp, r_valid=lo.r, X=Xin, ldx=ldxin, M=M, K=K, G=lo.gA, g_sr=K, g_sc=1, rpb=rmap[0], x_map=rmap[1],
                   defer=dA)
        return _kext(ext, ext.stride(0), lo.WeT, lo.Kext)

    def _qkv_adapters_fwd(self, p, qkv, grp, xm, M, U, ext3, fused):
        """Forward of the grouped q/k/v adapters (grp; None: nothing) on the LayerNorm output xm [M, D]: one down projection for the
        three (unless the LayerNorm launch carried it: fused); returns the K-extension keywords of the three projections."""
        if grp is None:
            return [{}, {}, {}]
        if not fused:
            self._down(p, X=xm, ldx=self.D, M=M, K=self.D, **self._qkv_down_kw(grp, U, ext3, qkv))
        return [{} if lw.lora is None else _kext(ext3[:, sec * grp["Kext"]:], ext3.stride(0), lw.lora.We, lw.lora.Kext)
                for sec, lw in enumerate(qkv)]

    def _qkv_down_kw(self, grp, U, ext3, qkv):
        """Weight and output keywords of the q/k/v group's down projection (qfx_lora_down; with W_fr: qfx_ln_down_fwd); site: the
        dropout keys of the three prepared linears qkv."""
        return dict(W_hi=grp["A_hi"], W_lo=grp["A_lo"], ldw=self.D, R=3 * grp["Rp"], Ut=U, ext=ext3, ld_ext=ext3.stride(0),
                    group_R=grp["Rp"], group_stride=grp["Kext"], site=self._site_keys(*qkv))

    def _qkv_adapters_bwd(self, p, qkv, grp, dq2, M, xm, U, V, ext, *, down, grads, rmap=(None, (0, 0)), pq=None, reduced=False):
        """Backward of the grouped q/k/v adapters on dq2 [*, 3D] = d(q | k | v): per adapted section v = d(section) (sB)^T into its
        rows of the hi/lo pair V and its columns of `ext` (collected in `down`; not when the attention epilogues and a head reduce
        have produced them: reduced) and dB; then dA over xm [M, D], the group's input: one pass for the three when all are adapted,
        else one per section.  The weight-gradient problems join `grads`.  rmap: as in _adapter_fwd, for dq2; pq: dq2's MX-FP8
        image (bytes, scales) that the down projections write on their way.  Returns the K-extension keywords of the group's dX GEMM."""
        D, Rp, Kext = self.D, grp["Rp"], grp["Kext"]
        (Vth, Vtl), (Uth, Utl) = V, U
        los = [lw.lora for lw in qkv]
        for sec, lo in enumerate(los):
            if lo is None:
                continue
            sl = slice(sec * Rp, (sec + 1) * Rp)
            if not reduced:
                self._down(p, X=dq2[:, sec * D:], ldx=3 * D, M=M, K=D, W_hi=lo.Bt_hi, W_lo=lo.Bt_lo, ldw=lo.Bt_hi.stride(0), R=Rp,
                           Ut=(Vth[sl], Vtl[sl]), ext=ext[:, sec * Kext:], ld_ext=ext.stride(0), rpb=rmap[0], x_map=rmap[1], defer=down,
                           site=self._site_keys(qkv[sec]), xq=None if pq is None else (_ptr(pq[0]) + sec * D, _ptr(pq[1]), 3 * D, M, sec * D // 32))
            self._grad(p, Vt=(Uth[sl], Utl[sl]), R=Rp, r_valid=lo.r, X=dq2[:, sec * D:], ldx=3 * D, M=M, K=D, G=lo.gB, g_sr=1,
                       g_sc=lo.r, rpb=rmap[0], x_map=rmap[1], out_scale=lo.scale, defer=grads)
        if all(lo is not None for lo in los):   # one pass over xm for dA of q, k and v
            self._grad(p, Vt=(Vth[:3 * Rp], Vtl[:3 * Rp]), R=3 * Rp, r_valid=los[0].r, group_R=Rp, X=xm, ldx=D, M=M, K=D,
                       G=[lo.gA for lo in los], g_sr=D, g_sc=1, defer=grads)
        else:
            for sec, lo in enumerate(los):
                if lo is not None:
                    sl = slice(sec * Rp, (sec + 1) * Rp)
                    self._grad(p, Vt=(Vth[sl], Vtl[sl]), R=Rp, r_valid=lo.r, X=xm, ldx=D, M=M, K=D, G=lo.gA, g_sr=D, g_sc=1, defer=grads)
        return _kext(ext, ext.stride(0), grp["WeT"], 3 * Kext)

    def _attn_args(self, qkv, sqk, ao, ldo, lse, dqkv, norms, norm_flags, eps):
        """The qfx_attn_args of one block, forward and backward fields (the backward program reuses the struct): q/k/v and their
        gradients as column sections of the joint [B*S, 3D] buffers qkv / dqkv, output ao (row stride ldo), saved pre-norm q|k sqk."""
        B, S, D = self.B, self.S, self.D
        a = L.AttnArgs()
        a.B, a.S, a.S_pad, a.H, a.dh, a.scale = B, S, self.S_pad, self.H, self.dh, 1.0 / math.sqrt(self.dh)
        q2 = qkv.view(B * S, 3 * D)
        a.Q, a.K, a.V = _ptr(q2[:, 0:]), _ptr(q2[:, D:]), _ptr(q2[:, 2 * D:])
        a.ldq = a.ldk = a.ldv = 3 * D
        a.O, a.ldo, a.lse2 = _ptr(ao), ldo, _ptr(lse)   # no transposed copies: the kernels use LDS transpose reads
        a.key_mask = _ptr(self.kmask)
        a.dsum = _ptr(self.A["dsum"])
        a.dO, a.lddo = _ptr(self.A["dao"]), D
        dq2 = dqkv.view(B * S, 3 * D)
        a.dQ, a.dK, a.dV = _ptr(dq2[:, 0:]), _ptr(dq2[:, D:]), _ptr(dq2[:, 2 * D:])
        a.lddq = a.lddk = a.lddv = 3 * D
        self._fuse_qk_bwd(a, sqk, norms, norm_flags, eps)
        return a

    # ------------------------------------------------------------------ forward program
    def _build_forward(self, P):
        A, B, D = self.A, self.B, self.D
        p = self.fwd
        model = self.model
        cfg = model.config
        Lyr = cfg.num_layers
        Jd = cfg.joint_attention_dim
        rows = self.rows
        eps = 1e-6
        self._emit_dropout_advance(p)
        # head: timestep embedding -> temb ; img_in ; txt_norm + txt_in ; all modulation vectors in one GEMV launch
        p.c(lib.qfx_timestep_embed, _ptr(A["t"]), B, 256, 1000.0, 1.0, _ptr(A["tproj"]))
        if self.cond:   # adapters on the conditioning head: base GEMVs + the banks' rank-r launches (cond_hip.py)
            self.cond_head.emit_forward(p)
        elif model.modulation_table is not None:
            # frozen head + a per-timestep table of its outputs (model.ensure_modulation_table): the fetch serves mods / mod_out when
            # every sample's timestep is a key and raises the hit cell, on which the four GEMVs return at once; an off-table
            # timestep leaves the cell at 0 and they run as ever.  Decided on the device: the program stays a static launch list.
            tb = self.mod_table = model.modulation_table      # (keeps the rows alive as long as this plan)
            A["mod_hit"] = self.buf(1, dtype=torch.int32, zero=True)
            hit = _ptr(A["mod_hit"])
            p.c(lib.qfx_mod_table_fetch, _ptr(A["t"]), B, _ptr(tb["keys"]), tb["keys"].numel(), _ptr(tb["mods"]), tb["mods"].stride(0),
                2 * Lyr, 6 * D, _ptr(tb["out"]), tb["out"].stride(0), 2 * D, _ptr(A["mods"]), _ptr(A["mod_out"]), hit)
            p.c(lib.qfx_mod_gemv_unless, _ptr(A["tproj"]), B, 256, _ptr(P["t1_Wp"]), _ptr(P["t1_bp"]), 1, D, 0, _ptr(A["t1"]), hit)
            p.c(lib.qfx_mod_gemv_unless, _ptr(A["t1"]), B, D, _ptr(P["t2_Wp"]), _ptr(P["t2_bp"]), 1, D, 1, _ptr(A["temb"]), hit)
            p.c(lib.qfx_mod_gemv_unless, _ptr(A["temb"]), B, D, _ptr(P["mod_W"]), _ptr(P["mod_b"]), 2 * Lyr, 6 * D, 1, _ptr(A["mods"]), hit)
            p.c(lib.qfx_mod_gemv_unless, _ptr(A["temb"]), B, D, _ptr(P["norm_out_Wp"]), _ptr(P["norm_out_bp"]), 1, 2 * D, 1,
                _ptr(A["mod_out"]), hit)
        else:
            p.c(lib.qfx_mod_gemv, _ptr(A["tproj"]), B, 256, _ptr(P["t1_Wp"]), _ptr(P["t1_bp"]), 1, D, 0, _ptr(A["t1"]))
            p.c(lib.qfx_mod_gemv, _ptr(A["t1"]), B, D, _ptr(P["t2_Wp"]), _ptr(P["t2_bp"]), 1, D, 1, _ptr(A["temb"]))
            p.c(lib.qfx_mod_gemv, _ptr(A["temb"]), B, D, _ptr(P["mod_W"]), _ptr(P["mod_b"]), 2 * Lyr, 6 * D, 1, _ptr(A["mods"]))
            p.c(lib.qfx_mod_gemv, _ptr(A["temb"]), B, D, _ptr(P["norm_out_Wp"]), _ptr(P["norm_out_bp"]), 1, 2 * D, 1, _ptr(A["mod_out"]))
        site = A["site"]
        kw = self._adapter_fwd(p, P["img_in"], A["in_img"], cfg.in_channels, rows["img"], site["img_in"].U, site["img_in"].ext)
        self._gemm(p, A1=A["in_img"], lda1=cfg.in_channels, B1=P["img_in"].W, K1=cfg.in_channels, M=rows["img"], N=D,
                   C_=A["X"]["img"][0], ldc=D, bias=P["img_in"].b, row_mask=self.rmask["img"], **kw)
        p.c(lib.qfx_rmsnorm_fwd, _ptr(A["in_txt"]), _ptr(model.txt_norm.weight.data), _ptr(A["txt_n"]), rows["txt"], Jd, eps)
        kw = self._adapter_fwd(p, P["txt_in"], A["txt_n"], Jd, rows["txt"], site["txt_in"].U, site["txt_in"].ext)
        self._gemm(p, A1=A["txt_n"], lda1=Jd, B1=P["txt_in"].W, K1=Jd, M=rows["txt"], N=D, C_=A["X"]["txt"][0], ldc=D,
                   bias=P["txt_in"].b, row_mask=self.rm_txt0, **kw)
        self.attn_args, self.attn_hl_qkv = [], []   # per block: qfx_attn_args, {stream: Rp} of the q/k/v projections fused in its backward
        for i in range(Lyr):
            mods = {"img": A["mods"][2 * i], "txt": A["mods"][2 * i + 1]}   # [B, 6D]: shift1 scale1 gate1 shift2 scale2 gate2
            self._emit_double_fwd(p, P["blocks"][i], A["blk"][i], mods, {s: A["X"][s][i] for s in ("img", "txt")},
                                  {s: (A["X"][s][i + 1], (0, 0)) for s in ("img", "txt")}, last=(i == Lyr - 1), norm_flags=0, par=i % 2)
        self._norm_out_fwd(p, A["X"]["img"][Lyr])
        self._proj_out_fwd(p, P["proj_out"])

    def _norm_out_fwd(self, p, x):
        """norm_out (AdaLayerNormContinuous) on the image stream x [B*S_i, D] -> A["xn_out"]."""
        A, D = self.A, self.D
        mo = A["mod_out"][0]  # [B, 2D]: scale | shift  (AdaLayerNormContinuous chunk order)
        p.c(lib.qfx_ln_modulate_fwd, _ptr(x), _ptr(mo[:, D:2 * D]), _ptr(mo[:, 0:D]), 2 * D, _ptr(A["xn_out"]),
            self.rows["img"], D, self.rpb["img"], 1e-6)

    def _proj_out_fwd(self, p, po):
        """proj_out (+ its adapter): A["xn_out"] -> A["out"], padded image rows masked."""
        A, D, M = self.A, self.D, self.rows["img"]
        kw = self._adapter_fwd(p, po, A["xn_out"], D, M, A["site"]["proj_out"].U, A["site"]["proj_out"].ext)
        self._gemm(p, A1=A["xn_out"], lda1=D, B1=po.W, K1=D, M=M, N=po.N, C_=A["out"], ldc=po.N, bias=po.b,
                   row_mask=self.rmask["img"], **kw)

    def _proj_out_bwd(self, p, po, masked):
        """proj_out dX (+ its adapter): A["dpred"] -> A["dxn"].  masked: the backward of the output masked_fill, no gradient enters
        through padded rows (the Qwen program passes the row mask here, the FLUX program does not)."""
        A, D, M = self.A, self.D, self.rows["img"]
        sb = A["site"]["proj_out"]
        kw = self._adapter_bwd(p, po, A["dpred"], po.N, M, A["xn_out"], D, sb.U, sb.V, sb.extb)
        self._gemm(p, A1=A["dpred"], lda1=po.N, B1=po.WT, K1=po.N, M=M, N=D, C_=A["dxn"], ldc=D,
                   row_mask=self.rmask["img"] if masked else None, **kw)

    def _norm_out_bwd(self, p, x, gate, dx):
        """norm_out backward on the image stream (+ d scale / d shift with a conditioning-head adapter): A["dxn"] -> dx = d(x) and
        A["dyg2"]["img"] = gate * dx for the last double block, whose gate2 = gate [B, D] of a [B, 6D] bank."""
        A, D, rows, rpb = self.A, self.D, self.rows["img"], self.rpb["img"]
        mo = A["mod_out"][0]
        if self.cond:
            dmo = A["dmod_out"][0]       # [B, 2D] = d scale | d shift (AdaLayerNormContinuous chunk order)
            self._mod_grad(p, dy=A["dxn"], x=x, rows=rows, rpb=rpb, dshift=dmo[:, D:2 * D], dscale=dmo[:, 0:D], out_bs=2 * D,
                           row_mask=self.rmask["img"])
        p.c(lib.qfx_ln_modulate_bwd, _ptr(A["dxn"]), _ptr(x), _ptr(mo[:, 0:D]), 2 * D, None, _ptr(gate), 6 * D, _ptr(dx),
            _ptr(A["dyg2"]["img"]), rows, D, rpb, 1e-6, None)

    def _emit_double_fwd(self, p, w, bb, mods, x_in, x_out, last, norm_flags, par=0):
        """One double-stream block (reference: transformer_qwenimage.py:425-494; FLUX: transformer_flux.py:467-523).
        x_in[s]: [rows_s, D] block input; x_out[s] = (tensor, c_map): where the block output goes (possibly a joint buffer)."""
        A, B, D, S, H, dh, T = self.A, self.B, self.D, self.S, self.H, self.dh, self.T
        rows, rpb, off = self.rows, self.rpb, self.off
        eps = 1e-6
        e1, e3 = A.get("ext1", _NONE), A.get("ext3", _NONE)
        qkv = bb["qkv"]
        q2 = qkv.view(B * S, 3 * D)
        sqk2 = bb["sqk"].view(B * S, 2 * D)
        ao2 = bb["ao"].view(B * S, D)
        # ---- LN1 + modulate, LoRA down-projections, then ONE grouped launch for the 6 q/k/v projections
        groups = []
        lnl = []
        ents = []
        xm1 = {s: (bb["xm1." + s] if w[s + ".qkv_lora"] is not None else A["xm"][s]) for s in STREAMS}
        for s in STREAMS:
            mod = mods[s]
            grp = w[s + ".qkv_lora"]
            ln = _ln_fwd_args(x_in[s], mod[:, 0:D], mod[:, D:2 * D], 6 * D, xm1[s], rows[s], D, rpb[s], eps)
            pq_ = self.fp8._preq_out(p, xm1[s], D, rows[s], D, s)    # MX-FP8 trunk: the q/k/v GEMMs take xm1 quantised by its producer
            if pq_ is not None:
                ln.yq, ln.ys, ln.ldyq, ln.ys_rows = _ptr(pq_[0]), _ptr(pq_[1]), D, rows[s]
            lnl.append(ln)
            ents.append((ln, None if grp is None else dict(self._qkv_down_kw(grp, bb["Uqkv." + s], e3[s], w[s + ".qkv"]), W_fr=grp.get("A_fr"))))
        # LayerNorm+modulate and the q/k/v down projection of its output in ONE pass over the row block (qfx_ln_down_fwd)
        fused = self._ln_down(p, ents)
        if not fused:
            _flush_ln(p, lnl, L.LnFwdArgs, lib.qfx_ln_modulate_fwd_batch)
        for s in STREAMS:
            kws = self._qkv_adapters_fwd(p, w[s + ".qkv"], w[s + ".qkv_lora"], xm1[s], rows[s], bb.get("Uqkv." + s), e3[s], fused)
            for sec, (lw, kw) in enumerate(zip(w[s + ".qkv"], kws)):
                # q and k go straight into the block's saved pre-norm copy (what the backward of the QK norm needs); the
                # norm+RoPE pass reads them there and writes the joint buffer (out-of-place mode: no copy pass)
                c_, ldc = (sqk2[:, sec * D:], 2 * D) if sec < 2 else (q2[:, 2 * D:], 3 * D)
                groups.append(_gargs(A1=xm1[s], lda1=D, B1=lw.W, K1=D, M=rows[s], N=D, C_=c_, ldc=ldc,
                                     bias=lw.b, rpb=rpb[s], c_map=(S, off[s]), **kw))
        self._gemm_group(p, groups)
        nq_t, nk_t, nq_i, nk_i = w["norms"]
        p.c(lib.qfx_qk_norm_rope_fwd, _ptr(qkv), _ptr(bb["sqk"]), _ptr(self.rope), _ptr(nq_t), _ptr(nk_t), _ptr(nq_i), _ptr(nk_i),
            B, S, T, H, dh, eps, norm_flags | 2, self.rope_bs)
        a = self._attn_args(qkv, bb["sqk"], bb["ao"], D, bb["lse"], self._sb("dqkv", par), w["norms"], norm_flags, eps)
        # the text stream of the last block never reaches the output (:661-663): dead compute, skipped
        live = [s for s in STREAMS if not (last and s == "txt")]
        hl_o, hl_qkv = self._head_lora_slots(a, w, live)
        self.attn_args.append(a)
        self.attn_hl_qkv.append(hl_qkv)
        p.c(lib.qfx_attn_fwd, C.byref(a))
        groups = []
        dfo = []
        dho = []
        for s in live:
            lw = w[s + ".o"]
            lo = lw.lora
            if lo is not None and s in hl_o:
                # u = ao A_o^T left the attention epilogue as per-head partial sums: reduce + pack (what qfx_lora_down wrote)
                dho.append(_head_reduce_args(A["hl_o"], hl_o[s], lo.Rp, rows[s], rpb[s], S, off[s], e1[s], bb["Uo." + s], lo.Rp, 0))
                self._drop_add(ext=e1[s], ld_ext=e1[s].stride(0), Ut=bb["Uo." + s], M=rows[s], R=lo.Rp, sites=self._site_keys(lw))
                kw = _kext(e1[s], e1[s].stride(0), lo.We, lo.Kext)
            else:
                # MX-FP8 trunk: the down projection reads every attention-output row of this stream anyway and leaves its
                # MX-FP8 image for the out-projection GEMM
                pq_ = None if lo is None else self.fp8._preq_out(p, ao2, D, rows[s], D, "ao." + s, a_map=(S, off[s]))
                kw = self._adapter_fwd(p, lw, ao2, D, rows[s], bb.get("Uo." + s), e1[s], defer=dfo, rmap=(rpb[s], (S, off[s])),
                                       xq=None if pq_ is None else (_ptr(pq_[0]), _ptr(pq_[1]), D, rows[s], 0))
            if "y1" in bb:
                kw.update(C2=bb["y1"][s], ldc2=D)
            groups.append(_gargs(A1=ao2, lda1=D, B1=lw.W, K1=D, M=rows[s], N=D, C_=bb["x1"][s], ldc=D, bias=lw.b,
                                 epi=L.EPI_GATE_RES, aux=x_in[s], ldaux=D, gate=mods[s][:, 2 * D:3 * D], gate_bs=6 * D,
                                 rpb=rpb[s], a_map=(S, off[s]), **kw))
        _flush_batch(p, dfo, L.LoraDownArgs, lib.qfx_lora_down_batch)
        _flush_head_reduce(p, dho)
        self._flush_dropout(p)
        self._gemm_group(p, groups)
        groups = []
        # feed-forward (+ LoRA on net.0.proj / net.2: the adapter's input is then kept per block instead of in scratch)
        xm2 = {s: (bb["xm2." + s] if w[s + ".fc1"].lora is not None else A["xm"][s]) for s in live}
        gact = {s: (bb["g." + s] if w[s + ".fc2"].lora is not None else A["g"][s]) for s in live}
        lnl = [_ln_fwd_args(bb["x1"][s], mods[s][:, 3 * D:4 * D], mods[s][:, 4 * D:5 * D], 6 * D, xm2[s], rows[s], D, rpb[s], eps)
               for s in live]
        for ln, s in zip(lnl, live):
            pq_ = self.fp8._preq_out(p, xm2[s], D, rows[s], D, s)    # ... and fc1 takes xm2
            if pq_ is not None:
                ln.yq, ln.ys, ln.ldyq, ln.ys_rows = _ptr(pq_[0]), _ptr(pq_[1]), D, rows[s]
        _flush_ln(p, lnl, L.LnFwdArgs, lib.qfx_ln_modulate_fwd_batch)
        dfw = []      # the image- and text-stream down projections of one site go out as ONE batched launch
        for s in live:
            f1 = w[s + ".fc1"]
            kw = self._adapter_fwd(p, f1, xm2[s], D, rows[s], bb.get("Uf1." + s), e1[s], defer=dfw)
            groups.append(_gargs(A1=xm2[s], lda1=D, B1=f1.W, K1=D, M=rows[s], N=4 * D, C_=bb["h"][s], ldc=4 * D,
                                 bias=f1.b, epi=L.EPI_GELU, C2=gact[s], ldc2=4 * D,
                                 nxt=(gact[s], 4 * D, w[s + ".fc2"].lora is not None), **kw))   # gelu(h) feeds fc2 (and its adapter's dA, if any)
        _flush_batch(p, dfw, L.LoraDownArgs, lib.qfx_lora_down_batch)
        self._flush_dropout(p)
        self._gemm_group(p, groups)
        groups = []
        for s in live:
            f2 = w[s + ".fc2"]
            kw = self._adapter_fwd(p, f2, gact[s], 4 * D, rows[s], bb.get("Uf2." + s), e1[s], defer=dfw)
            if "y2" in bb:
                kw.update(C2=bb["y2"][s], ldc2=D)
            groups.append(_gargs(A1=gact[s], lda1=4 * D, B1=f2.W, K1=4 * D, M=rows[s], N=D, C_=x_out[s][0], ldc=D,
                                 bias=f2.b, epi=L.EPI_GATE_RES, aux=bb["x1"][s], ldaux=D, gate=mods[s][:, 5 * D:6 * D],
                                 gate_bs=6 * D, rpb=rpb[s], c_map=x_out[s][1], aux_unmapped=1, row_mask=self.rmask[s], **kw))
        _flush_batch(p, dfw, L.LoraDownArgs, lib.qfx_lora_down_batch)
        self._flush_dropout(p)
        self._gemm_group(p, groups)

    # ------------------------------------------------------------------ backward program
    def _build_backward(self, P):
        A, D = self.A, self.D
        p = self.bwd
        cfg = self.model.config
        Lyr = cfg.num_layers
        rows, site = self.rows, A["site"]
        # tail: proj_out dX (+ its adapter), norm_out LN backward (+ gate2 of the last block folded in)
        self._proj_out_bwd(p, P["proj_out"], masked=True)
        cur = 0
        if self.cond:
            p.py(A["dmods"].zero_)
            p.py(A["dmod_out"].zero_)
        self._norm_out_bwd(p, A["X"]["img"][Lyr], A["mods"][2 * (Lyr - 1)][:, 5 * D:6 * D], A["dX"]["img"][cur])
        for i in range(Lyr - 1, -1, -1):
            nxt = cur ^ 1
            mods = {"img": A["mods"][2 * i], "txt": A["mods"][2 * i + 1]}
            gate_prev = None if i == 0 else {"img": A["mods"][2 * (i - 1)][:, 5 * D:6 * D], "txt": A["mods"][2 * (i - 1) + 1][:, 5 * D:6 * D]}
            self._emit_double_bwd(p, P["blocks"][i], A["blk"][i], self.attn_args[i], self.attn_hl_qkv[i], mods, {s: A["X"][s][i] for s in ("img", "txt")},
                                  dx2={s: A["dX"][s][cur] for s in ("img", "txt")}, out_dx={s: A["dX"][s][nxt] for s in ("img", "txt")},
                                  gate_prev=gate_prev, last=(i == Lyr - 1), first=(i == 0 and not self.full_bwd), norm_flags=0,
                                  prefix=f"transformer_blocks.{i}.", par=i % 2,
                                  dmods=({"img": A["dmods"][2 * i], "txt": A["dmods"][2 * i + 1]} if self.cond else None))
            if not self.side_grads:
                p.mark(f"transformer_blocks.{i}.")
            cur = nxt
        self._side_join(p)
        # head: the embedders' adapters (their inputs carry no gradient: rank-r launches only); d(block-0 input) = A["dX"][s][cur]
        if self.in_grad:
            for key, s, x, ldx in (("img_in", "img", A["in_img"], cfg.in_channels), ("txt_in", "txt", A["txt_n"], cfg.joint_attention_dim)):
                self._adapter_bwd(p, P[key], A["dX"][s][cur], D, rows[s], x, ldx, site[key].U, site[key].V, site[key].extb)
        if self.cond:
            self.cond_head.emit_backward(p)

    def _emit_double_bwd(self, p, w, bb, a, hl_qkv, mods, x_in, dx2, out_dx, gate_prev, last, first, norm_flags, prefix=None, par=0, dmods=None):
        """Backward of one double-stream block.  In: dx2[s] = d(block output), A["dyg2"][s] = gate2*dx2 (emitted by whoever
        produced dx2).  Out: out_dx[s] = d(block input) and A["dyg2"][s] = gate_prev*out_dx (for the previous block)."""
        A, B, D, S, H, dh, T = self.A, self.B, self.D, self.S, self.H, self.dh, self.T
        rows, rpb, off = self.rows, self.rpb, self.off
        eps = 1e-6
        dao2 = A["dao"].view(B * S, D)
        dqkv, dyg1 = self._sb("dqkv", par), self._sb("dyg1", par)
        VtO, VtQ = self._sb("VtO", par) or _NONE, self._sb("Vt", par) or _NONE
        ff_side = self.side_grads and self._ff_side
        dh_ = self._sb("dh", par) if ff_side else A["dh"]
        VtF1, VtF2 = ((self._sb(name, par) if ff_side else A.get(name)) or _NONE for name in ("VtF1", "VtF2"))
        e1, e3 = A.get("ext1", _NONE), A.get("ext3", _NONE)
        if ff_side:
            self._side_join(p, keep=1)      # the launch of block i+2 read this parity's dh: overwritten by this block's first GEMM
        dq2 = dqkv.view(B * S, 3 * D)
        i = 0 if first else 1
        # LoRA weight gradients are leaves: every qfx_lora_grad of the block is deferred to ONE batched launch per rank at the
        # end of the block (their X operands -- dyg1, ao, dqkv, xm1, dh, the kept feed-forward inputs -- stay intact until the next block's backward
        # starts; the one exception, dyg2, is flushed early)
        gl = []
        ao2 = bb["ao"].view(B * S, D)
        live = [s for s in STREAMS if not (last and s == "txt")]
        if last:
            # no gradient reaches the last block's text tail: d(attn out) of the text rows is zero
            p.py(A["dao"][:, :T].zero_)
        # ---- MLP backward: dh = (gate2*dx2) W2 * gelu'(h) ; dxm2 = dh W1   (both streams per launch)
        ge = []   # gradients whose X operand (dyg2) is overwritten before the end of the block: flushed right after the MLP
        groups = []
        dbw = []      # both streams' v = dY B of a site in ONE batched launch
        for s in live:
            f2 = w[s + ".fc2"]
            kw = self._adapter_bwd(p, f2, A["dyg2"][s], D, rows[s], bb.get("g." + s), 4 * D, bb.get("Uf2." + s), VtF2[s], e1[s],
                                   down=dbw, dB=ge, dA=gl)
            groups.append(_gargs(A1=A["dyg2"][s], lda1=D, B1=f2.WT, K1=D, M=rows[s], N=4 * D, C_=dh_[s],
                                 ldc=4 * D, epi=L.EPI_DGELU, aux=bb["h"][s], ldaux=4 * D,
                                 nxt=(dh_[s], 4 * D, w[s + ".fc1"].lora is not None), **kw))   # dh feeds fc1's dX GEMM (and its adapter's v / dB)
        _flush_batch(p, dbw, L.LoraDownArgs, lib.qfx_lora_down_batch)
        self._flush_dropout(p)
        self._gemm_group(p, groups)
        groups = []
        for s in live:
            f1 = w[s + ".fc1"]
            kw = self._adapter_bwd(p, f1, dh_[s], 4 * D, rows[s], bb.get("xm2." + s), D, bb.get("Uf1." + s), VtF1[s], e1[s],
                                   down=dbw, dB=gl, dA=gl)
            groups.append(_gargs(A1=dh_[s], lda1=4 * D, B1=f1.WT, K1=4 * D, M=rows[s], N=D, C_=A["dxm"][s], ldc=D, **kw))
        _flush_batch(p, dbw, L.LoraDownArgs, lib.qfx_lora_down_batch)
        self._flush_dropout(p)
        self._gemm_group(p, groups)
        _flush_batch(p, ge, L.LoraGradArgs, lib.qfx_lora_grad_batch)
        if dmods is not None:   # d(shift2, scale2, gate2): dy = d(xm2) (fc1 dX output), LN input x1, gate side dx2 * y2
            mg = []
            for s in live:
                dm = dmods[s]
                self._mod_grad(p, dy=A["dxm"][s], x=bb["x1"][s], rows=rows[s], rpb=rpb[s], dshift=dm[:, 3 * D:4 * D],
                               dscale=dm[:, 4 * D:5 * D], dgate=dm[:, 5 * D:6 * D], dxo=dx2[s], y=bb["y2"][s], out_bs=6 * D,
                               row_mask=self.rmask[s], defer=mg)
            _flush_mod_grad(p, mg)
        self._side_join(p, keep=1)   # the launch of block i+2 read this parity's dyg1 / dqkv / v^T scratch: overwritten from here on
        groups = []
        lnl = [_ln_bwd_args(A["dxm"][s], bb["x1"][s], mods[s][:, 4 * D:5 * D], 6 * D, dx2[s], mods[s][:, 2 * D:3 * D], 6 * D,
                            A["dx1"][s], dyg1[s], rows[s], D, rpb[s], eps, None) for s in live]
        for ln, s in zip(lnl, live):
            pq_ = self.fp8._preq_out(p, dyg1[s], D, rows[s], D, s)   # "mxfp8-fb": the out-projection dX GEMM takes gate1*dx quantised
            if pq_ is not None:
                ln.dygq, ln.dygs, ln.lddygq, ln.dygs_rows = _ptr(pq_[0]), _ptr(pq_[1]), D, rows[s]
        _flush_ln(p, lnl, L.LnBwdArgs, lib.qfx_ln_modulate_bwd_batch)
        dbo = []
        for s in live:
            # attention out-projection backward (+ LoRA)
            lw = w[s + ".o"]
            kw = self._adapter_bwd(p, lw, dyg1[s], D, rows[s], ao2, D, bb.get("Uo." + s), VtO[s], e1[s], down=dbo, dB=gl, dA=gl,
                                   rmap=(rpb[s], (S, off[s])))
            groups.append(_gargs(A1=dyg1[s], lda1=D, B1=lw.WT, K1=lw.N, M=rows[s], N=lw.K, C_=dao2, ldc=D, rpb=rpb[s],
                                 c_map=(S, off[s]), **kw))
        _flush_batch(p, dbo, L.LoraDownArgs, lib.qfx_lora_down_batch)
        self._flush_dropout(p)
        self._gemm_group(p, groups)
        # ---- attention backward
        emit_attn_backward(p, a, A, self.lv.attn_bwd)      # two-pass pair, or the one-pass kernel (QFX_ATTN_BWD)
        if not a.qk_saved:      # (else: the backward of the QK norm + RoPE runs in the epilogues of the two kernels above)
            nq_t, nk_t, nq_i, nk_i = w["norms"]
            p.c(lib.qfx_qk_norm_rope_bwd, _ptr(dqkv), _ptr(bb["sqk"]), _ptr(self.rope), _ptr(nq_t), _ptr(nk_t), _ptr(nq_i),
                _ptr(nk_i), B, S, T, H, dh, eps, norm_flags, self.rope_bs)
        # ---- q/k/v projection backward (+ LoRA), both streams in one launch
        groups = []
        dl = []   # the q/k/v down projections of both streams: one batched launch
        dhq = []  # ... or, fused into the attention epilogues, their reduce + pack halves
        for s in STREAMS:
            grp = w[s + ".qkv_lora"]
            kw = {}
            if grp is not None:
                Rp = grp["Rp"]
                # "mxfp8-fb": the three down projections together read every element of this stream's dqkv rows and leave
                # its MX-FP8 image (q, k, v column sections of one operand) for the qkv dX GEMM
                pq_ = None
                if i > 0 and all(lw.lora is not None for lw in w[s + ".qkv"]):
                    pq_ = self.fp8._preq_out(p, dq2, 3 * D, rows[s], 3 * D, "dqkv." + s, a_map=(S, off[s]))
                if s in hl_qkv:     # v = d(pre-norm q | k), dV times (sB)^T left the attention epilogues as per-head partial sums
                    dhq.append(_head_reduce_args(A["hl_qkv"], H, 3 * Rp, rows[s], rpb[s], S, off[s], e3[s],
                                                 (VtQ[s][0][:3 * Rp], VtQ[s][1][:3 * Rp]), Rp, grp["Kext"]))
                    self._drop_add(ext=e3[s], ld_ext=e3[s].stride(0), Ut=(VtQ[s][0][:3 * Rp], VtQ[s][1][:3 * Rp]), M=rows[s], R=3 * Rp,
                                   group_R=Rp, group_stride=grp["Kext"], sites=self._site_keys(*w[s + ".qkv"]))
                kw = self._qkv_adapters_bwd(p, w[s + ".qkv"], grp, dq2, rows[s], bb["xm1." + s], bb["Uqkv." + s], VtQ[s], e3[s],
                                            down=dl, grads=gl, rmap=(rpb[s], (S, off[s])), pq=pq_, reduced=s in hl_qkv)
            if i > 0:   # nothing upstream of block 0 needs a gradient (frozen embedders, inputs without grad)
                groups.append(_gargs(A1=dq2, lda1=3 * D, B1=w[s + ".qkvT"], K1=3 * D, M=rows[s], N=D, C_=A["dxm"][s], ldc=D,
                                     rpb=rpb[s], a_map=(S, off[s]), **kw))
        _flush_batch(p, dl, L.LoraDownArgs, lib.qfx_lora_down_batch)
        _flush_head_reduce(p, dhq)
        self._flush_dropout(p)
        if i > 0:
            self._gemm_group(p, groups)
            if dmods is not None:   # d(shift1, scale1, gate1): dy = d(xm1) (q/k/v dX output), LN input x_in, gate side dx1 * y1
                mg = []
                for s in STREAMS:
                    dm = dmods[s]
                    dead = last and s == "txt"     # no out-projection / residual gradient on the last block's text tail
                    self._mod_grad(p, dy=A["dxm"][s], x=x_in[s], rows=rows[s], rpb=rpb[s], dshift=dm[:, 0:D], dscale=dm[:, D:2 * D],
                                   dgate=None if dead else dm[:, 2 * D:3 * D], dxo=None if dead else A["dx1"][s],
                                   y=None if dead else bb["y1"][s], out_bs=6 * D, row_mask=self.rmask[s], defer=mg)
                _flush_mod_grad(p, mg)
            lnl = []
            for s in STREAMS:
                dres = None if (last and s == "txt") else A["dx1"][s]
                gp = gate_prev[s] if gate_prev is not None else None
                lnl.append(_ln_bwd_args(A["dxm"][s], x_in[s], mods[s][:, D:2 * D], 6 * D, dres, gp,
                                        (gp.stride(0) if gp is not None else 0), out_dx[s],
                                        A["dyg2"][s] if gp is not None else None, rows[s], D, rpb[s], eps, self.rmask[s]))
                pq_ = self.fp8._preq_out(p, A["dyg2"][s] if gp is not None else None, D, rows[s], D, s)   # the previous block's fc2-dX operand
                if pq_ is not None:
                    lnl[-1].dygq, lnl[-1].dygs, lnl[-1].lddygq, lnl[-1].dygs_rows = _ptr(pq_[0]), _ptr(pq_[1]), D, rows[s]
            _flush_ln(p, lnl, L.LnBwdArgs, lib.qfx_ln_modulate_bwd_batch)
        if self.side_grads and gl:
            self._emit_side(p, gl, prefix)
        else:
            _flush_batch(p, gl, L.LoraGradArgs, lib.qfx_lora_grad_batch)

    def _emit_side(self, p, gl, prefix):
        """Fork, the block's batched gradient launches on the side stream, the event its join will wait for."""
        p.py(self._side_fork)
        _flush_batch(p, gl, L.LoraGradArgs, lib.qfx_lora_grad_batch, side=True)
        ev = torch.cuda.Event()
        p.py(lambda ev=ev: ev.record(self.bwd.side))
        self._side_q.append((ev, prefix))

    def set_multires(self, img_shapes, txt_seq_lens, attention_mask, S_in=None):
        """Per-batch tables of the multi-resolution path (host-side plumbing of transformer_qwen_custom.py:72-150,175-228,
        444-512).  Per sample the joint table [text rows | image rows] starts at joint row 0, i.e. the image rows follow the
        sample's OWN text length (the reference's placement); every other row keeps the identity rotation."""
        cfg = self.model.config
        B, S, T, S_i = self.B, self.S, self.T, self.S_i
        dev = self.model.device
        batched = isinstance(img_shapes, list) and len(img_shapes) > 0 and isinstance(img_shapes[0], list)
        per = [normalize_img_shapes(sh) for sh in img_shapes] if batched else [normalize_img_shapes(img_shapes)] * B
        lens = list(txt_seq_lens) if isinstance(txt_seq_lens, (list, tuple)) else [int(txt_seq_lens)] * B
        rope = torch.zeros(B, S, self.dh // 2, 2)
        rope[..., 0] = 1.0
        if all(sh == per[0] for sh in per):      # shared RoPE: first sample's shapes, max text length (custom forward :462-470)
            tbl = qwen_joint_rope(per[0], max(lens), cfg.axes_dims_rope)
            if max(lens) != T:
                raise ValueError("max(txt_seq_lens) must equal the text sequence length (reference RoPE broadcast)")
            rope[:, : tbl.shape[0]] = tbl
        else:
            for b in range(B):
                tbl = qwen_joint_rope(per[b], int(lens[b]), cfg.axes_dims_rope)
                if tbl.shape[0] > S:
                    raise ValueError(f"sample {b}: text + image tokens ({tbl.shape[0]}) exceed the padded joint length {S}")
                rope[b, : tbl.shape[0]] = tbl
        km = torch.zeros(B, S)
        rm_i = torch.ones(B, S_i)
        rm_t = torch.ones(B, T)
        S_in = S_i if S_in is None else S_in          # image rows the caller hands over; rows S_in..S_i are ladder padding
        if attention_mask is not None or S_in < S_i:
            m = torch.zeros(B, S, dtype=torch.bool)
            if attention_mask is not None:
                am = attention_mask if attention_mask.dtype == torch.bool else attention_mask > 0
                m[:, : T + S_in] = am[:, : T + S_in].cpu()
            else:
                m[:, : T + S_in] = True
            km.masked_fill_(~m, float("-inf"))
            rm_i = m[:, T:].float()
            rm_t = m[:, :T].float()
        A = self.A
        A["rope_b"].copy_(rope.to(dev, non_blocking=True))
        A["kmask"].copy_(km.to(dev, non_blocking=True))
        A["rm_img"].copy_(rm_i.reshape(-1).to(dev, non_blocking=True))
        A["rm_txt0"].copy_(rm_t.reshape(-1).to(dev, non_blocking=True))

    # ------------------------------------------------------------------ execution
    def run_forward(self, hidden_states, encoder_hidden_states, timestep):
        A = self.A
        self._copy_rows(A["in_img"].view(self.B, self.S_i, -1), hidden_states)
        A["in_txt"].view(self.B, self.T, -1).copy_(encoder_hidden_states)
        A["t"].copy_(timestep.reshape(self.B).to(F32))
        self.model.refresh_lora_operands()
        self._sync_dropout()
        self.fwd.run()
        return A["out"].view(self.B, self.S_i, -1)

    @staticmethod
    def _copy_rows(dst, src):
        """dst [B, S_plan, C] <- src [B, S_in <= S_plan, C]; the ladder-padding rows (masked everywhere) are zeroed."""
        n = src.shape[1]
        if n == dst.shape[1]:
            dst.copy_(src)
        else:
            dst[:, :n].copy_(src)
            dst[:, n:].zero_()

    def run_backward(self, dpred, on_segment=None):
        """on_segment(prefixes): called after each marked segment of the backward program with the parameter-name prefixes
        whose LoRA gradients just became final (data-parallel bucketed all-reduce hooks in here)."""
        if getattr(self.model, "_merged", False):
            raise RuntimeError("adapters are merged into the base weights (merge_adapter): call unmerge_adapter() before training")
        self._copy_rows(self.A["dpred"].view(self.B, self.S_i, -1), dpred)
        self.model._lora.ensure_grads()
        if on_segment is None:
            self.bwd.run()
            return
        pos = 0
        for idx, prefix in self.bwd.marks:
            self.bwd.run(pos, idx)
            pos = idx
            on_segment(prefix)
        self.bwd.run(pos, None)


class _QwenDiTFn(torch.autograd.Function):
    """Whole-DiT autograd node.  LoRA parameters are inputs only so that autograd schedules the node;
    their gradients are accumulated by the kernels directly into the flat .grad buffer (returns None)."""

    @staticmethod
    def forward(ctx, model, plan, hidden_states, encoder_hidden_states, timestep, *lora_params):
        ctx.plan = plan
        out = plan.run_forward(hidden_states, encoder_hidden_states, timestep)
        n = (hidden_states[0] if isinstance(hidden_states, tuple) else hidden_states).shape[1]
        return out[:, :n].clone()      # a ladder plan carries more rows than the caller handed over

    @staticmethod
    def backward(ctx, grad_out):
        ctx.plan.model._dp_backward(ctx.plan, grad_out.contiguous())     # + the data-parallel exchange when enabled (dp.py)
        return (None,) * len(ctx.needs_input_grad)
