"""The MX-FP8 trunk of a plan (model.quantize_trunk): which GEMM groups run on the block-scaled FP8 MFMA, their quantisation
launches and scratch, and the hand-over of operands that a producer's epilogue already quantised to the GEMM group that follows."""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib as L
from .. import ops
from .emit import _gargs
from .prog import _ptr

lib = L.lib


class _Fp8Trunk:
    """One per plan.  `scratch`: quantised-operand buffers by slot; `preq`: operands that left their producer already quantised,
    {(address, row stride, a_map, M): (bytes, scales, MX-FP8 only)}, valid until the next GEMM group is emitted; `produced`: what
    the group being emitted quantises in its epilogues for the group after it.  The quantised copies of the frozen weights live on
    the model (`_wq_cache`: shared by its plans, dropped with them)."""

    def __init__(self, plan):
        self.plan = plan
        self.scratch = {}
        self.preq = {}
        self.produced = []

    def _slot(self, slot, M, K):
        if slot not in self.scratch:
            self.scratch[slot] = (self.plan.buf(M, K, dtype=torch.uint8), self.plan.buf(K // 128, M, 4, dtype=torch.uint8))
        return self.scratch[slot]

    def takes(self, prog, groups):
        q, plan = self.plan.model._quant, self.plan
        return bool(q) and (prog is plan.fwd or (q == "mxfp8-fb" and prog is plan.bwd)) and all(self._fp8_ok(op) for op in groups)

    def next_group(self):
        """A GEMM group has been emitted: on-the-fly quantised operands are for the group that follows their producer."""
        self.preq.clear()
        self.preq.update(self.produced)
        self.produced = []

    def check_bf16(self, groups):
        """An operand that left its producer as MX-FP8 only (no bf16 copy) must not reach a bf16 GEMM."""
        for op in groups:
            A1, lda1, a_map = op.src[:3]
            ent = self.preq.get((A1.data_ptr(), lda1, a_map, op.args.M)) if isinstance(A1, torch.Tensor) else None
            if ent is not None and ent[2]:
                raise RuntimeError("internal: an operand that exists only as MX-FP8 is consumed by a bf16 GEMM")

    def _preq_out(self, prog, out, ld, M, N, tag, keep_bf16=True, a_map=(0, 0)):
        """Scratch (fp8 bytes [M, N], tile-major scales [N/128, M, 4]) for the MX-FP8 image of `out` that its PRODUCER writes on
        the fly; registered so that the MX-FP8 GEMM group that comes next skips its quantisation pass for this operand (the
        registration lives until that next group).  None when the trunk is not quantised in this direction / shape."""
        q = self.plan.model._quant
        if (not q or (prog is self.plan.bwd and q != "mxfp8-fb") or N % 128 or N < 1024 or out is None
                or not self.plan.lv.fp8_fused_quant):
            return None
        oq, osc = self._slot(("pre", M, N, tag), M, N)
        self.preq[(out.data_ptr(), ld, tuple(a_map), M)] = (oq, osc, not keep_bf16)
        return oq, osc

    @staticmethod
    def _fp8_ok(op):
        g, B1 = op.args, op.src[4]
        # a weight [N, K1] or the first N rows of a taller contiguous one (the FLUX single block's proj_out^T is contracted in two row
        # ranges): MX blocks run along K, so a row range quantises to the same bytes as the rows of the whole matrix
        return (isinstance(B1, torch.Tensor) and B1.dim() == 2 and B1.is_contiguous() and g.K1 % 128 == 0 and g.K1 >= 1024
                and g.N >= 1024 and B1.shape[1] == g.K1 and B1.shape[0] >= g.N and g.ldb1 == g.K1 and not g.seg2_plain)

    def _gemm_group_mxfp8(self, prog, groups):
        """Forward GEMMs of the block linears on the block-scaled FP8 MFMA (model.quantize = "mxfp8", the MI355X analogue of
        the reference's quantized trunk, src/qflux/models/quantize.py): the frozen weight is quantised ONCE (cached on the model),
        the activation operand once per distinct input of the group; bias, bf16 mid-rounding, the bf16 LoRA K-extension and the
        epilogue are unchanged.  The backward stays on the bf16 operands (dX = dY W in bf16, adapters on the bf16 activations)."""
        cache = self.plan.model._wq_cache
        quantised = {}
        fp8 = []
        tiles = sum(((op.args.M + 255) // 256) * ((op.args.N + 127) // 128) for op in groups)
        persistent = tiles >= 160 and len(groups) <= 6
        for gi_, (g, (A1, lda1, a_map, rpb, B1), nxt) in enumerate(groups):
            key = (B1.data_ptr(), (g.N, g.K1))
            if key not in cache:
                cache[key] = ops.quant_mxfp8(B1[:g.N])
            wq, ws = cache[key]
            akey = (A1.data_ptr(), lda1, a_map, g.M)
            if akey in self.preq:
                quantised[akey] = self.preq[akey][:2]
            if akey not in quantised:
                xq, xs = self._slot((g.M, g.K1, len(quantised)), g.M, g.K1)
                qa = L.QuantArgs()
                qa.X, qa.ldx, qa.M, qa.K = _ptr(A1), lda1, g.M, g.K1
                qa.Q, qa.ldq, qa.S, qa.lds = _ptr(xq), g.K1, _ptr(xs), 0
                qa.rows_per_batch, qa.x_batch_rows, qa.x_row_off = rpb, a_map[0], a_map[1]
                prog.keep.append(qa)
                prog.c(lib.qfx_quant_mxfp8, C.byref(qa))
                quantised[akey] = (xq, xs)
            xq, xs = quantised[akey]
            f = L.GemmFp8Args()
            C.memmove(C.byref(f.g), C.byref(g), C.sizeof(L.GemmArgs))
            f.g.A1, f.g.lda1, f.g.a_batch_rows, f.g.a_row_off = _ptr(xq), g.K1, 0, 0
            f.g.B1, f.g.ldb1 = _ptr(wq), g.K1
            f.sa, f.ldsa, f.sb, f.ldsb = _ptr(xs), 0, _ptr(ws), 0
            # quantising epilogue: gelu(h) (forward fc1 -> fc2) / dh (backward fc2-dX -> fc1-dX) leave the producer as MX-FP8 when the
            # consumer is an MX-FP8 GEMM too; the stand-alone quantisation pass of that operand (60 MB read per block) disappears,
            # and so does the bf16 copy when nothing else reads it (`nxt` = (tensor, row stride, bf16 copy still needed))
            if (nxt is not None and persistent and g.N % 128 == 0 and g.N >= 1024 and g.c_batch_rows == 0
                    and self.plan.lv.fp8_fused_quant):
                out, ld_out, keep_bf16 = nxt
                oq, osc = self._slot(("pre", g.M, g.N, gi_), g.M, g.N)
                f.cq, f.cs, f.ldcq, f.cq_rows, f.cq_only = _ptr(oq), _ptr(osc), g.N, g.M, 0 if keep_bf16 else 1
                self.produced.append(((out.data_ptr(), ld_out, (0, 0), g.M), (oq, osc, not keep_bf16)))
            fp8.append(f)
            prog.keep.append((wq, ws))
        # one persistent grid for the whole group (image + text stream, q/k/v) when it is large enough, else one launch each
        if persistent:
            arr = (L.GemmFp8Args * len(fp8))(*fp8)
            prog.keep.append(arr)
            prog.c(lib.qfx_gemm_mxfp8_grouped, arr, len(fp8))
        else:
            for f in fp8:
                prog.keep.append(f)
                prog.c(lib.qfx_gemm_mxfp8, C.byref(f))

    def _gemm_mxfp8_cat(self, prog, parts, *, M, N, C_, ldc, ext=None):
        """C = sum_i X_i W_i^T (+ the bf16 LoRA K-extension `ext`: the keywords emit._kext returns) as ONE MX-FP8 contraction over the
        concatenated K of `parts` = [(X_i [M, K_i] bf16, row stride, K_i, W_i^T as [N, >= K_i] bf16)]: the operands are quantised
        side by side into one byte buffer / one tile-major scale array (K_i % 128 == 0: MX blocks and scale tiles never straddle a
        seam), the weights once (cached on the model).  Used for dX contractions that sum several frozen linears ("mxfp8-fb")."""
        Kt = sum(K for _, _, K, _ in parts)
        cache = self.plan.model._wq_cache
        key = ("cat", N) + tuple((Wt.data_ptr(), K) for _, _, K, Wt in parts)
        if key not in cache:
            cache[key] = ops.quant_mxfp8(torch.cat([Wt[:N, :K] for _, _, K, Wt in parts], dim=1).contiguous())
        wq, ws = cache[key]
        xq, xs = self._slot(("cat", M, Kt), M, Kt)
        col = 0
        for X, ldx, K, _ in parts:
            assert K % 128 == 0
            qa = L.QuantArgs()
            qa.X, qa.ldx, qa.M, qa.K = _ptr(X), ldx, M, K
            qa.Q, qa.ldq, qa.S, qa.lds = xq.data_ptr() + col, Kt, xs.data_ptr() + (col // 128) * M * 4, 0
            qa.rows_per_batch, qa.x_batch_rows, qa.x_row_off = M, 0, 0
            prog.keep.append(qa)
            prog.c(lib.qfx_quant_mxfp8, C.byref(qa))
            col += K
        g = _gargs(A1=xq, lda1=Kt, B1=wq, K1=Kt, M=M, N=N, C_=C_, ldc=ldc, **(ext or {})).args
        f = L.GemmFp8Args()
        C.memmove(C.byref(f.g), C.byref(g), C.sizeof(L.GemmArgs))
        f.sa, f.ldsa, f.sb, f.ldsb = _ptr(xs), 0, _ptr(ws), 0
        prog.keep.append((f, wq, ws))
        prog.c(lib.qfx_gemm_mxfp8, C.byref(f))
