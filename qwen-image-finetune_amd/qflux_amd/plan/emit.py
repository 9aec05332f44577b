"""Argument-struct builders (pure functions of their arguments), the batching flushes and the attention-backward emitter: what needs
no plan state."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch

from .. import _lib as L
from .. import ops
from .prog import _ptr

lib = L.lib

# One GEMM problem: the argument struct, the python-side identities of its operands (A1, lda1, a_map, rows_per_batch, B1: the
# low-precision trunk re-targets them) and, where the consumer of its output is a GEMM too, nxt = (output tensor, row stride,
# bf16 copy still needed) for the quantising epilogue of the MX-FP8 trunk.
_GemmOp = namedtuple("_GemmOp", "args src nxt")


def _gargs(*, A1, lda1, B1, K1, M, N, C_, ldc, ldb1=None, bias=None, A2=None, lda2=0, B2=None, ldb2=0, K2=0,
           epi=L.EPI_NONE, C2=None, ldc2=0, aux=None, ldaux=0, gate=None, gate_bs=0, rpb=None, a_map=(0, 0), c_map=(0, 0),
           seg2_plain=0, aux_unmapped=0, row_mask=None, nxt=None):
    g = L.GemmArgs()
    g.A1, g.B1, g.lda1, g.ldb1, g.K1 = _ptr(A1), _ptr(B1), lda1, (K1 if ldb1 is None else ldb1), K1
    if K2:
        g.A2, g.B2, g.lda2, g.ldb2, g.K2 = _ptr(A2), _ptr(B2), lda2, ldb2, K2
    g.M, g.N = M, N
    g.bias = _ptr(bias)
    g.C, g.ldc = _ptr(C_), ldc
    g.C2, g.ldc2 = _ptr(C2), ldc2
    g.aux, g.ldaux = _ptr(aux), ldaux
    g.gate, g.gate_bstride = _ptr(gate), gate_bs
    g.rows_per_batch = M if rpb is None else rpb
    g.a_batch_rows, g.a_row_off = a_map
    g.c_batch_rows, g.c_row_off = c_map
    g.epi = epi
    g.seg2_plain = seg2_plain
    g.aux_unmapped = aux_unmapped
    g.row_mask = _ptr(row_mask)
    return _GemmOp(g, (A1, lda1, a_map, g.rows_per_batch, B1), nxt)


def _kext(ext, ld, W, K2):
    """Keywords of a GEMM's second K segment: `ext` (row stride ld) against W over K2 columns -- an adapter's K-extension."""
    return dict(A2=ext, lda2=ld, B2=W, ldb2=W.stride(0), K2=K2)


def emit_attn_backward(p, a, A, mode):
    """Emit the attention backward of one block into launch program `p`: the two-pass pair qfx_attn_bwd_dq + qfx_attn_bwd_dkv, or the
    one-pass qfx_attn_bwd_fused (csrc/qfx_attn_bwd1.hip) with its workspace kept once per plan in the arena `A`.  mode (the plan's
    QFX_ATTN_BWD lever) = 2pass | 1pass | auto; auto (default) = whichever measured faster for the shape: the two-pass pair
    everywhere as of round 6 (profiles/r06_attn_onepass.json: the ordered fp32 dQ accumulation across key blocks costs what the
    saved recompute returns)."""
    if mode == "1pass":
        if "dq_ws" not in A:
            A["dq_ws"] = ops.attn_bwd_fused_workspace(a)
        ws = A["dq_ws"]
        if ws is not None:
            a.dq_acc, a.dq_turn = ws[0].data_ptr(), ws[1].data_ptr()
            p.c(lib.qfx_attn_bwd_fused, C.byref(a))
            return "1pass"
    p.c(lib.qfx_attn_bwd_dq, C.byref(a))
    p.c(lib.qfx_attn_bwd_dkv, C.byref(a))
    return "2pass"


def _emit_or_defer(prog, a, fn, defer):
    """One launch for the problem `a`, or -- defer: a list -- the problem joins a batched launch its caller flushes."""
    if defer is not None:
        defer.append(a)
        return
    prog.keep.append(a)
    prog.c(fn, C.byref(a))


def _down_args(*, X, ldx, M, K, W_hi, W_lo, ldw, R, ext=None, ld_ext=0, Ut=None, group_R=None,
               group_stride=0, rpb=None, x_map=(0, 0), xq=None):
    a = L.LoraDownArgs()
    if xq is not None:      # (bytes, scales, row stride, scale rows, first 32-column block): X's MX-FP8 image rides along
        a.xq, a.xs, a.ldxq, a.xs_rows, a.xq_kb0 = xq
    a.X, a.ldx, a.M, a.K = _ptr(X), ldx, M, K
    a.W_hi, a.W_lo, a.ldw, a.R = _ptr(W_hi), _ptr(W_lo), ldw, R
    a.ext, a.ld_ext = _ptr(ext), ld_ext
    if Ut is not None:
        a.Ut_hi, a.Ut_lo, a.ld_ut = _ptr(Ut[0]), _ptr(Ut[1]), Ut[0].stride(0)
    a.group_R = R if group_R is None else group_R
    a.group_stride = group_stride
    a.rows_per_batch = M if rpb is None else rpb
    a.x_batch_rows, a.x_row_off = x_map
    return a


def _grad_args(prog, det, *, Vt, R, r_valid, X, ldx, M, K, G, g_sr, g_sc, group_R=None, rpb=None, x_map=(0, 0), out_scale=1.0):
    a = L.LoraGradArgs()
    Gs = G if isinstance(G, (tuple, list)) else (G,)
    a.Vt_hi, a.Vt_lo, a.ldvt, a.R, a.r_valid = _ptr(Vt[0]), _ptr(Vt[1]), Vt[0].stride(0), R, r_valid
    a.group_R = R // len(Gs) if group_R is None else group_R
    a.X, a.ldx, a.M, a.K = _ptr(X), ldx, M, K
    a.G = _ptr(Gs[0])
    a.G1 = _ptr(Gs[1]) if len(Gs) > 1 else None
    a.G2 = _ptr(Gs[2]) if len(Gs) > 2 else None
    a.g_sr, a.g_sc = g_sr, g_sc
    a.rows_per_batch = M if rpb is None else rpb
    a.x_batch_rows, a.x_row_off = x_map
    a.out_scale = out_scale
    # ABI 7: chunk partials through a scratch of the problem's own, added up in chunk order by the last block to arrive -- the flat
    # LoRA gradient is bit-reproducible (det off, QFX_GRAD_DET=0: the fp32 atomics of rounds 1-5).  One scratch per problem of the plan:
    # launches on the main and the side stream may overlap, 288 GB make sharing pointless (~10 MB per block).
    if det:
        nfl = int(lib.qfx_lora_grad_ws_floats(M, K, R))
        ws = torch.empty(max(nfl, 4), dtype=torch.float32, device=X.device)
        cnt = torch.zeros((K + 127) // 128, dtype=torch.int32, device=X.device)
        a.ws, a.ws_count, a.ws_floats = _ptr(ws), _ptr(cnt), ws.numel()
        prog.keep.append((ws, cnt))
    return a


def _mod_grad_args(D, *, dy, x, rows, rpb, dshift, dscale, out_bs, dgate=None, dxo=None, y=None, row_mask=None, ld=None):
    a = L.ModGradArgs()
    ld = D if ld is None else ld
    a.dy, a.ld_dy, a.x, a.ld_x = _ptr(dy), ld, _ptr(x), ld
    a.dxo, a.ld_dxo, a.y, a.ld_y = _ptr(dxo), ld, _ptr(y), ld
    a.dshift, a.dscale, a.dgate, a.out_bstride = _ptr(dshift), _ptr(dscale), _ptr(dgate), out_bs
    a.row_mask, a.rows, a.D, a.rows_per_batch, a.eps = _ptr(row_mask), rows, D, rpb, 1e-6
    return a


def _ln_fwd_args(x, shift, scale, mod_bs, y, rows, D, rpb, eps):
    a = L.LnFwdArgs()
    a.x, a.shift, a.scale, a.mod_bstride, a.y = _ptr(x), _ptr(shift), _ptr(scale), mod_bs, _ptr(y)
    a.rows, a.D, a.rows_per_batch, a.eps = rows, D, rpb, eps
    return a


def _ln_bwd_args(dy, x, scale, mod_bs, dres, gate, gate_bs, dx, dyg, rows, D, rpb, eps, row_mask):
    a = L.LnBwdArgs()
    a.dy, a.x, a.scale, a.mod_bstride = _ptr(dy), _ptr(x), _ptr(scale), mod_bs
    a.dres, a.gate, a.gate_bstride, a.dx, a.dyg = _ptr(dres), _ptr(gate), gate_bs, _ptr(dx), _ptr(dyg)
    a.row_mask, a.rows, a.D, a.rows_per_batch, a.eps = _ptr(row_mask), rows, D, rpb, eps
    return a


def _head_reduce_args(part, H, R, M, rpb, x_batch_rows, off, ext, Ut, group_R, group_stride):
    r = L.LoraHeadReduceArgs()
    r.part, r.part_hstride, r.ld_part, r.H = _ptr(part), part.shape[1] * part.shape[2], part.shape[2], H
    r.M, r.R = M, R
    r.ext, r.ld_ext = _ptr(ext), ext.stride(0)
    r.Ut_hi, r.Ut_lo, r.ld_ut = _ptr(Ut[0]), _ptr(Ut[1]), Ut[0].stride(0)
    r.group_R, r.group_stride = group_R, group_stride
    r.rows_per_batch, r.x_batch_rows, r.x_row_off = rpb, x_batch_rows, off
    return r


def _flush_head_reduce(prog, pending):
    if pending:
        arr = (L.LoraHeadReduceArgs * len(pending))(*pending)
        prog.keep.append(arr)
        prog.c(lib.qfx_lora_head_reduce, arr, len(pending))
        pending.clear()


def _flush_ln(prog, pending, struct, fn):
    """One launch for the LayerNorm problems of both streams (ragged row counts go last: only the last problem of a batch
    may have rows % 4 != 0)."""
    pend = sorted(pending, key=lambda a: (a.rows % 4 != 0))
    while pend:
        chunk = []
        while pend and len(chunk) < L.MAX_LN_BATCH:
            chunk.append(pend.pop(0))
            if chunk[-1].rows % 4:
                break
        arr = (struct * len(chunk))(*chunk)
        prog.keep.append(arr)
        prog.c(fn, arr, len(chunk))
    pending.clear()


def _flush_batch(prog, pending, struct, fn, side=False):
    """Emit deferred skinny-kernel problems as batched launches: same R per launch, at most QFX_MAX_BATCH each."""
    by_r = {}
    for a in pending:
        by_r.setdefault(a.R, []).append(a)
    for lst in by_r.values():
        for i in range(0, len(lst), L.MAX_BATCH):
            chunk = lst[i:i + L.MAX_BATCH]
            arr = (struct * len(chunk))(*chunk)
            prog.keep.append(arr)
            (prog.c_side if side else prog.c)(fn, arr, len(chunk))
    pending.clear()


def _flush_dropout(prog, pending, state):
    """Emit the collected dropout problems (ops.lora_dropout_args, one per rank-r producer call) as batched qfx_lora_dropout_apply
    launches over the device state `state`: directly behind the producers' own flush and before the first launch that reads their
    buffers (the K-extension GEMMs, the weight-gradient problems)."""
    for i in range(0, len(pending), L.MAX_BATCH):
        chunk = pending[i:i + L.MAX_BATCH]
        arr = (L.LoraDropoutArgs * len(chunk))(*chunk)
        prog.keep.append(arr)
        prog.c(lib.qfx_lora_dropout_apply, arr, len(chunk), _ptr(state.words))
    pending.clear()


def _flush_mod_grad(prog, pending):
    for i in range(0, len(pending), L.MAX_LN_BATCH):
        chunk = pending[i:i + L.MAX_LN_BATCH]
        arr = (L.ModGradArgs * len(chunk))(*chunk)
        prog.keep.append(arr)
        prog.c(lib.qfx_mod_grad_batch, arr, len(chunk))
    pending.clear()
