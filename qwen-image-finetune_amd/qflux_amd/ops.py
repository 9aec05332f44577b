"""Tensor-level wrappers over the C ABI (one Python function per entry point of include/qfx.h).
These are what the per-kernel parity tests call; the model builds cached argument structs instead
(plan/qwen.py, plan/flux.py) so that a training step is a flat list of C calls."""
from __future__ import annotations

import collections
import ctypes as C
import math

import torch

from . import _lib as L

lib = L.lib
BF = torch.bfloat16


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _bf(t, name):
    assert t.dtype == BF and t.is_cuda, f"{name}: bf16 CUDA tensor required"
    return t


def gemm(a1, b1, *, bias=None, a2=None, b2=None, out=None, epi=L.EPI_NONE, out2=None, aux=None, gate=None,
         rows_per_batch=None, a_map=(0, 0), c_map=(0, 0), M=None, c_rows=None, row_mask=None):
    """C = a1 @ b1.T (+ a2 @ b2.T) + bias -> epilogue.  a1 [*,K1] (row stride = a1.stride(0)), b1 [N,K1]."""
    _bf(a1, "a1"); _bf(b1, "b1")
    M = a1.shape[0] if M is None else M
    N, K1 = b1.shape
    if out is None:
        out = torch.empty(M if c_rows is None else c_rows, N, dtype=BF, device=a1.device)
    g = L.GemmArgs()
    g.A1, g.B1, g.lda1, g.ldb1, g.K1 = _p(a1), _p(b1), a1.stride(0), b1.stride(0), K1
    if a2 is not None:
        g.A2, g.B2, g.lda2, g.ldb2, g.K2 = _p(a2), _p(b2), a2.stride(0), b2.stride(0), b2.shape[1]
    g.M, g.N = M, N
    g.bias = _p(bias)
    g.C, g.ldc = _p(out), out.stride(0)
    if out2 is not None:
        g.C2, g.ldc2 = _p(out2), out2.stride(0)
    if aux is not None:
        g.aux, g.ldaux = _p(aux), aux.stride(0)
    if gate is not None:
        g.gate, g.gate_bstride = _p(gate), gate.stride(0)
    g.rows_per_batch = M if rows_per_batch is None else rows_per_batch
    g.a_batch_rows, g.a_row_off = a_map
    g.c_batch_rows, g.c_row_off = c_map
    g.epi = epi
    g.row_mask = _p(row_mask)
    L.check(lib.qfx_gemm_bf16(C.byref(g), stream_ptr()), "qfx_gemm_bf16")
    return out


def gemm_grouped(arg_list):
    """arg_list: list of (a1, b1, out, kwargs) -> one grouped launch (kwargs as for gemm's struct fields)."""
    gs = []
    for (a1, b1, out, kw) in arg_list:
        g = L.GemmArgs()
        g.A1, g.B1, g.lda1, g.ldb1, g.K1 = _p(a1), _p(b1), a1.stride(0), b1.stride(0), b1.shape[1]
        g.M, g.N = kw.get("M", a1.shape[0]), b1.shape[0]
        g.bias = _p(kw.get("bias"))
        g.C, g.ldc = _p(out), out.stride(0)
        g.rows_per_batch = g.M
        g.epi = kw.get("epi", L.EPI_NONE)
        gs.append(g)
    arr = (L.GemmArgs * len(gs))(*gs)
    L.check(lib.qfx_gemm_grouped(arr, len(gs), stream_ptr()), "qfx_gemm_grouped")


def lora_down(x, w_hi, w_lo, *, U=None, ext=None, Ut=None, group_R=None, group_stride=0, M=None, rows_per_batch=None, x_map=(0, 0)):
    """Ut = (Ut_hi, Ut_lo) bf16 [R, ld] zero-initialised transposed split outputs (optional)."""
    a = L.LoraDownArgs()
    M = x.shape[0] if M is None else M
    R, K = w_hi.shape
    a.X, a.ldx, a.M, a.K = _p(x), x.stride(0), M, K
    a.W_hi, a.W_lo, a.ldw, a.R = _p(w_hi), _p(w_lo), w_hi.stride(0), R
    if U is not None:
        a.U, a.ldu = _p(U), U.stride(0)
    if ext is not None:
        a.ext, a.ld_ext = _p(ext), ext.stride(0)
    if Ut is not None:
        a.Ut_hi, a.Ut_lo, a.ld_ut = _p(Ut[0]), _p(Ut[1]), Ut[0].stride(0)
    a.group_R = R if group_R is None else group_R
    a.group_stride = group_stride
    a.rows_per_batch = M if rows_per_batch is None else rows_per_batch
    a.x_batch_rows, a.x_row_off = x_map
    L.check(lib.qfx_lora_down(C.byref(a), stream_ptr()), "qfx_lora_down")


def lora_grad(Vt, X, G, g_sr, g_sc, *, M, r_valid=None, group_R=None, K=None, rows_per_batch=None, x_map=(0, 0), out_scale=1.0, deterministic=True):
    """Vt = (Vt_hi, Vt_lo) bf16 [R, ld>=roundup(M,32)] ; G a tensor or a tuple of up to 3 tensors (fused targets)."""
    a = L.LoraGradArgs()
    Gs = G if isinstance(G, (tuple, list)) else (G,)
    R = Vt[0].shape[0]
    a.Vt_hi, a.Vt_lo, a.ldvt, a.R = _p(Vt[0]), _p(Vt[1]), Vt[0].stride(0), R
    a.group_R = R // len(Gs) if group_R is None else group_R
    a.r_valid = a.group_R if r_valid is None else r_valid
    a.X, a.ldx, a.M, a.K = _p(X), X.stride(0), M, (X.shape[1] if K is None else K)
    a.G = _p(Gs[0]); a.G1 = _p(Gs[1]) if len(Gs) > 1 else None; a.G2 = _p(Gs[2]) if len(Gs) > 2 else None
    a.g_sr, a.g_sc = g_sr, g_sc
    a.rows_per_batch = M if rows_per_batch is None else rows_per_batch
    a.x_batch_rows, a.x_row_off = x_map
    a.out_scale = out_scale
    if deterministic:      # ABI 7: chunk partials through scratch, summed in chunk order (False: the fp32 atomics of rounds 1-5)
        ws = torch.empty(max(int(lib.qfx_lora_grad_ws_floats(a.M, a.K, a.R)), 4), dtype=torch.float32, device=X.device)
        cnt = torch.zeros((a.K + 127) // 128, dtype=torch.int32, device=X.device)
        a.ws, a.ws_count, a.ws_floats = _p(ws), _p(cnt), ws.numel()
    L.check(lib.qfx_lora_grad(C.byref(a), stream_ptr()), "qfx_lora_grad")
    if deterministic:
        assert int(cnt.abs().max()) == 0      # (synchronises: this helper is for tests)


def pack_descs_tensor(descs, device):
    """list[LoraPackArgs] -> uint8 device tensor holding the C array."""
    arr = (L.LoraPackArgs * len(descs))(*descs)
    raw = bytes(arr)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)


def lora_pack(desc_tensor, n, max_dim):
    L.check(lib.qfx_lora_pack(desc_tensor.data_ptr(), n, max_dim, stream_ptr()), "qfx_lora_pack")


def ln_modulate_fwd(x, shift, scale, rows_per_batch, eps=1e-6, out=None):
    rows, D = x.shape
    out = torch.empty_like(x) if out is None else out
    assert shift.stride(0) == scale.stride(0)
    L.check(lib.qfx_ln_modulate_fwd(_p(x), _p(shift), _p(scale), shift.stride(0), _p(out), rows, D, rows_per_batch, eps,
                                    stream_ptr()), "qfx_ln_modulate_fwd")
    return out


def ln_modulate_bwd(dy, x, scale, rows_per_batch, dres=None, gate=None, eps=1e-6, want_dyg=False, row_mask=None):
    rows, D = x.shape
    dx = torch.empty_like(x)
    dyg = torch.empty_like(x) if want_dyg else None
    L.check(lib.qfx_ln_modulate_bwd(_p(dy), _p(x), _p(scale), scale.stride(0), _p(dres), _p(gate),
                                    gate.stride(0) if gate is not None else 0, _p(dx), _p(dyg), rows, D, rows_per_batch, eps,
                                    _p(row_mask), stream_ptr()), "qfx_ln_modulate_bwd")
    return dx, dyg


def gate_mul(dx, gate, rows_per_batch):
    rows, D = dx.shape
    out = torch.empty_like(dx)
    L.check(lib.qfx_gate_mul(_p(dx), _p(gate), gate.stride(0), _p(out), rows, D, rows_per_batch, stream_ptr()), "qfx_gate_mul")
    return out


def rmsnorm_fwd(x, w, eps=1e-6):
    rows, D = x.shape
    out = torch.empty_like(x)
    L.check(lib.qfx_rmsnorm_fwd(_p(x), _p(w), _p(out), rows, D, eps, stream_ptr()), "qfx_rmsnorm_fwd")
    return out


def ptr_table(tensors, device):
    return torch.tensor([t.data_ptr() if t is not None else 0 for t in tensors], dtype=torch.int64, device=device)


def mod_gemv(temb, weights, biases, apply_silu=True):
    B, K = temb.shape
    N = weights[0].shape[0]
    wt = ptr_table(weights, temb.device)
    bt = ptr_table(biases, temb.device) if biases is not None else None
    out = torch.empty(len(weights), B, N, dtype=BF, device=temb.device)
    L.check(lib.qfx_mod_gemv(_p(temb), B, K, _p(wt), _p(bt), len(weights), N, int(apply_silu), _p(out), stream_ptr()), "qfx_mod_gemv")
    return out


def mod_gemv_tables(temb, wt, bt, nmat, N, apply_silu=True):
    """qfx_mod_gemv with prepared device pointer tables (wt / bt: int64 tensors of nmat device pointers)."""
    B, K = temb.shape
    out = torch.empty(nmat, B, N, dtype=BF, device=temb.device)
    L.check(lib.qfx_mod_gemv(_p(temb), B, K, _p(wt), _p(bt), nmat, N, int(apply_silu), _p(out), stream_ptr()), "qfx_mod_gemv")
    return out


def mod_gemv_unless(temb, weights, biases, out, skip, apply_silu=True):
    """qfx_mod_gemv into `out` [nmat, B, N] unless the device int32 cell `skip` (None: no guard) holds a non-zero value."""
    B, K = temb.shape
    N = weights[0].shape[0]
    wt = ptr_table(weights, temb.device)
    bt = ptr_table(biases, temb.device) if biases is not None else None
    L.check(lib.qfx_mod_gemv_unless(_p(temb), B, K, _p(wt), _p(bt), len(weights), N, int(apply_silu), _p(out), _p(skip), stream_ptr()),
            "qfx_mod_gemv_unless")
    return out


def mod_table_fetch(t, keys, tbl_mods, tbl_out, mods, mod_out, hit):
    """Serve mods [nmat, B, N] / mod_out [B, N_out] from the table rows (tbl_mods [n, nmat, N], tbl_out [n, N_out]) of the fp32
    timesteps t [B] when every one of them is in keys [n]; the device int32 cell `hit` tells which way it went."""
    n, nmat, N = tbl_mods.shape
    L.check(lib.qfx_mod_table_fetch(_p(t), t.shape[0], _p(keys), n, _p(tbl_mods), tbl_mods.stride(0), nmat, N, _p(tbl_out),
                                    tbl_out.stride(0), tbl_out.shape[1], _p(mods), _p(mod_out), _p(hit), stream_ptr()),
            "qfx_mod_table_fetch")
    return hit


def mod_gemv_t(dy, weights=None, out=None, table=None):
    """out[b, k] += sum_mat dy[mat, b, :] @ W_mat  (fp32 [B, K]); dy bf16 [nmat, B, N] contiguous; weights: list of [N, K] bf16
    tensors, or table = (prepared device pointer table, K)."""
    nmat, B, N = dy.shape
    if table is None:
        K = weights[0].shape[1]
        wt = ptr_table(weights, dy.device)
    else:
        wt, K = table
    out = torch.zeros(B, K, dtype=torch.float32, device=dy.device) if out is None else out
    L.check(lib.qfx_mod_gemv_t(_p(dy), B, N, K, _p(wt), nmat, _p(out), stream_ptr()), "qfx_mod_gemv_t")
    return out


def timestep_embed(t, dim=256, scale=1000.0, pre_scale=1.0):
    out = torch.empty(t.shape[0], dim, dtype=BF, device=t.device)
    L.check(lib.qfx_timestep_embed(_p(t.float().contiguous()), t.shape[0], dim, scale, pre_scale, _p(out), stream_ptr()),
            "qfx_timestep_embed")
    return out


def add3(a, b, c=None):
    out = torch.empty_like(a)
    L.check(lib.qfx_add3_bf16(_p(a), _p(b), _p(c), _p(out), a.numel(), stream_ptr()), "qfx_add3_bf16")
    return out


def qk_norm_rope(qkv, saved, rope, wq_txt, wk_txt, wq_img, wk_img, B, S, T, H, dh, eps=1e-6, backward=False, flags=0, rope_bstride=0):
    fn = lib.qfx_qk_norm_rope_bwd if backward else lib.qfx_qk_norm_rope_fwd
    L.check(fn(_p(qkv), _p(saved), _p(rope), _p(wq_txt), _p(wk_txt), _p(wq_img), _p(wk_img), B, S, T, H, dh, eps, flags, rope_bstride, stream_ptr()),
            "qfx_qk_norm_rope")


def transpose_heads(x, ld, B, S, S_pad, H, dh, out=None):
    """x: pointer-carrying tensor whose element 0 is [b=0,s=0,h=0,d=0]; row stride ld."""
    out = torch.empty(B, H, dh, S_pad, dtype=BF, device=x.device) if out is None else out
    L.check(lib.qfx_transpose_heads(_p(x), ld, _p(out), B, S, S_pad, H, dh, stream_ptr()), "qfx_transpose_heads")
    return out


def attn_args(B, S, S_pad, H, dh, scale, **kw):
    a = L.AttnArgs()
    a.B, a.S, a.S_pad, a.H, a.dh, a.scale = B, S, S_pad, H, dh, scale
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return a


def attn_call(name, a):
    L.check(getattr(lib, name)(C.byref(a), stream_ptr()), name)


def attn_tune(spec: str):
    """Kernel-selection policy of the attention entry points (qfx_attn_tune): "fwd64=0|1|1p|auto,dq64=0|1|auto,fwd_waves=0|4|8"."""
    L.check(lib.qfx_attn_tune(spec.encode() if spec else None), "qfx_attn_tune")


def attn_bwd_fused_workspace(a, device=None):
    """Allocates (once per shape, by the caller) the workspace of qfx_attn_bwd_fused for the shape in `a` and points a.dq_acc / a.dq_turn
    at it.  Returns (acc fp32 tensor, turn int32 tensor) -- keep them alive -- or None where the one-pass backward does not exist."""
    nb_acc, nb_turn = C.c_int64(0), C.c_int64(0)
    rc = lib.qfx_attn_bwd_fused_workspace(C.byref(a), C.byref(nb_acc), C.byref(nb_turn))
    if rc != 0 or nb_acc.value == 0:
        return None
    device = device or torch.device("cuda", torch.cuda.current_device())
    acc = torch.empty(nb_acc.value // 4, dtype=torch.float32, device=device)
    turn = torch.zeros(nb_turn.value // 4, dtype=torch.int32, device=device)      # zero before the first launch; launches leave it zero
    a.dq_acc, a.dq_turn = acc.data_ptr(), turn.data_ptr()
    return acc, turn


def mse_loss_fwd_bwd(pred, target, S_t, gscale=1.0, want_grad=True):
    B, S_all, Cc = pred.shape
    loss = torch.zeros((), dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    L.check(lib.qfx_mse_loss_fwd_bwd(_p(pred), _p(target), _p(loss), _p(dpred), B, S_all, S_t, Cc, gscale, stream_ptr()),
            "qfx_mse_loss_fwd_bwd")
    return loss, dpred


def mse_token_weighted_fwd_bwd(pred, target, token_w, S_t, inv_denom, gscale=1.0, want_grad=True):
    B, S_all, Cc = pred.shape
    loss = torch.zeros((), dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    L.check(lib.qfx_mse_token_weighted_fwd_bwd(_p(pred), _p(target), _p(token_w), _p(loss), _p(dpred), B, S_all, S_t, Cc, inv_denom,
                                               gscale, stream_ptr()), "qfx_mse_token_weighted_fwd_bwd")
    return loss, dpred


LOSS_KINDS = {"l2": L.LOSS_L2, "huber": L.LOSS_HUBER, "smooth_l1": L.LOSS_SMOOTH_L1}


def criterion_workspace(B, S_t, C_, device):
    """The workspace of criterion_fwd_bwd for this shape (fp64 partial sums; not zeroed: every launch writes all it reads)."""
    return torch.empty(lib.qfx_criterion_workspace_bytes(B, S_t, C_) // 8, dtype=torch.float64, device=device)


def criterion_fwd_bwd(pred, target, S_t, *, sample_w=None, token_w=None, huber_c=None, kind="l2", inv_denom=None, gscale=1.0,
                      want_grad=True, workspace=None):
    """The general criterion (qfx_criterion_fwd_bwd, see qfx.h): loss = mean_b sample_w[b] * loss_per_sample[b] over the first S_t
    rows of pred, token-weighted with token_w [B,S_t], rho = d^2 ("l2") or kohya's "huber" / "smooth_l1" with the per-sample
    threshold huber_c [B] (> 0 and finite: the caller's to check on the host).  inv_denom: 1/(B S_t) when None.  Returns
    (loss, loss_per_sample [B], dpred or None); nothing is accumulated, nothing needs zeroing, no host sync."""
    B, S_all, Cc = pred.shape
    if kind not in LOSS_KINDS:
        raise ValueError(f"criterion_fwd_bwd: kind is one of {sorted(LOSS_KINDS)}, not {kind!r}")
    if kind != "l2" and huber_c is None:
        raise ValueError(f"criterion_fwd_bwd: kind {kind!r} needs huber_c")
    dev = pred.device
    _bf(pred, "pred"); _bf(target, "target")
    assert pred.is_contiguous() and target.is_contiguous() and tuple(target.shape) == (B, S_t, Cc), "criterion_fwd_bwd: pred [B,S_all,C], target [B,S_t,C], contiguous"
    for name, t, n in (("sample_w", sample_w, B), ("token_w", token_w, B * S_t), ("huber_c", huber_c, B)):
        assert t is None or (t.dtype == torch.float32 and t.device == dev and t.is_contiguous() and t.numel() == n), \
            f"criterion_fwd_bwd: {name} is a contiguous float32 tensor of {n} elements on {dev}"
    ws = criterion_workspace(B, S_t, Cc, dev) if workspace is None else workspace
    assert ws.device == dev and ws.is_contiguous(), "criterion_fwd_bwd: workspace on the device of pred"
    loss = torch.empty((), dtype=torch.float32, device=dev)
    lps = torch.empty(B, dtype=torch.float32, device=dev)
    dpred = torch.empty_like(pred) if want_grad else None
    a = L.CriterionArgs()
    a.pred, a.target, a.sample_w, a.token_w, a.huber_c = _p(pred), _p(target), _p(sample_w), _p(token_w), _p(huber_c)
    a.loss, a.loss_per_sample, a.dpred, a.workspace, a.workspace_bytes = _p(loss), _p(lps), _p(dpred), _p(ws), ws.numel() * ws.element_size()
    a.B, a.S_all, a.S_t, a.C, a.kind = B, S_all, S_t, Cc, LOSS_KINDS[kind]
    a.inv_denom, a.gscale = (1.0 / (B * S_t) if inv_denom is None else inv_denom), gscale
    L.check(lib.qfx_criterion_fwd_bwd(C.byref(a), stream_ptr()), "qfx_criterion_fwd_bwd")
    return loss, lps, dpred


def flowmatch_prepare(x0, noise, ctrl, sigma, mode=0):
    B, S_t, Cc = x0.shape
    S_c = ctrl.shape[1] if ctrl is not None else 0
    packed = torch.empty(B, S_t + S_c, Cc, dtype=BF, device=x0.device)
    target = torch.empty(x0.shape, dtype=BF, device=x0.device)   # x0 may hold fp16 bits (mode 1); outputs are always bf16
    L.check(lib.qfx_flowmatch_prepare(_p(x0), _p(noise), _p(ctrl), _p(sigma), _p(packed), _p(target), B, S_t, S_c, Cc, mode, stream_ptr()),
            "qfx_flowmatch_prepare")
    return packed, target


def sumsq(g, out):
    L.check(lib.qfx_sumsq(_p(g), g.numel(), _p(out), stream_ptr()), "qfx_sumsq")


def sumsq_det(g, out, partials):
    """Deterministic sum of squares (fixed reduction order): out[0] is overwritten; partials = fp32 workspace."""
    L.check(lib.qfx_sumsq_det(_p(g), g.numel(), _p(out), _p(partials), partials.numel(), stream_ptr()), "qfx_sumsq_det")


_side_streams = {}


def side_stream(device):
    """Process-wide side stream of `device` at the lowest priority, as a torch stream object."""
    key = torch.device(device).index or 0
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(device=torch.device("cuda", key), priority=1)
    return _side_streams[key]


def prodigy_init_state(state, d0=1e-6):
    """state: fp64[PRODIGY_STATE] device tensor (d, d_max, d_numerator, d_denom, d_hat, k, scratch...)."""
    L.check(lib.qfx_prodigy_init_state(_p(state), float(d0), stream_ptr()), "qfx_prodigy_init_state")


def prodigy_step(p, g, exp_avg, exp_avg_sq, s, p0, state, lr=1.0, betas=(0.9, 0.999), beta3=None, eps=1e-8, weight_decay=0.0,
                 decouple=True, use_bias_correction=False, safeguard_warmup=False, d0=1e-6, d_coef=1.0, growth_rate=float("inf"),
                 gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
    a = L.ProdigyArgs(_p(p), _p(g), _p(exp_avg), _p(exp_avg_sq), _p(s), _p(p0), p.numel(), _p(state), lr, betas[0], betas[1],
                      0.0 if beta3 is None else beta3, eps, weight_decay, d0, d_coef, growth_rate, int(use_bias_correction),
                      int(safeguard_warmup), int(decouple), _p(gnorm_sq), max_norm, grad_scale)
    L.check(lib.qfx_prodigy_step(a, stream_ptr()), "qfx_prodigy_step")


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, wd, step, gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    L.check(lib.qfx_adamw_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, wd, bc1, bc2, _p(gnorm_sq), max_norm,
                               grad_scale, stream_ptr()), "qfx_adamw_step")


def sgd_step(p, g, buf, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, first=False, gnorm_sq=None, max_norm=0.0,
             grad_scale=1.0):
    """One torch.optim.SGD step over the flat buffers p / g (qfx.h); buf: the momentum buffer, None iff momentum == 0; first: buf is
    created by this step (buf = the decayed gradient, no dampening)."""
    L.check(lib.qfx_sgd_step(_p(p), _p(g), _p(buf), p.numel(), lr, momentum, dampening, weight_decay, int(bool(nesterov)),
                             int(bool(first)), _p(gnorm_sq), max_norm, grad_scale, stream_ptr()), "qfx_sgd_step")


class Adam8bitLayout:
    """Block table of one flat-buffer layout for qfx_adam8bit_step, built once per layout.  `tensors[i]` = (off, numel, eight_bit,
    first absmax index, number of absmax blocks, first element in the fp32 moment buffers) of entry i."""

    def __init__(self, table, tensors, blocksize, min_8bit_size, n_absmax, n_fp32, extent):
        self.table, self.tensors, self.blocksize, self.min_8bit_size = table, tensors, blocksize, min_8bit_size
        self.n_blocks = table.numel() // C.sizeof(L.Adam8bitBlock)
        self.n_absmax, self.n_fp32, self.extent = n_absmax, n_fp32, extent


def adam8bit_block_table(entries, blocksize=256, min_8bit_size=4096, device=None):
    """entries: (offset, numel) of every tensor in the flat buffers (offsets multiples of 4).  A tensor with numel >= min_8bit_size is
    cut into ceil(numel / blocksize) 8-bit blocks (the last one short) with an absmax slot each, in entry order; a smaller one keeps
    fp32 moments, packed at 64-element-aligned offsets of m32 / v32 and walked in blocksize chunks."""
    if blocksize not in (256, 2048):
        raise ValueError(f"adam8bit blocksize must be 256 or 2048, not {blocksize}")
    rows, tensors, n_abs, n_fp32, extent = [], [], 0, 0, 0
    for off, k in entries:
        off, k = int(off), int(k)
        if off % 4 or k <= 0:
            raise ValueError(f"adam8bit block table: offset {off} / numel {k}")
        nb = (k + blocksize - 1) // blocksize
        if k >= min_8bit_size:
            tensors.append((off, k, True, n_abs, nb, -1))
            rows += [(off + j * blocksize, n_abs + j, min(blocksize, k - j * blocksize), L.ADAM8BIT_BLOCKWISE) for j in range(nb)]
            n_abs += nb
        else:
            tensors.append((off, k, False, -1, 0, n_fp32))
            rows += [(off + j * blocksize, n_fp32 + j * blocksize, min(blocksize, k - j * blocksize), L.ADAM8BIT_FP32) for j in range(nb)]
            n_fp32 += (k + 63) // 64 * 64
        extent = max(extent, off + k)
    if not rows:
        raise ValueError("adam8bit block table: no tensors")
    arr = (L.Adam8bitBlock * len(rows))(*[L.Adam8bitBlock(*r) for r in rows])
    table = torch.frombuffer(bytearray(arr), dtype=torch.uint8)
    if device is not None:
        table = table.to(device)
    return Adam8bitLayout(table, tensors, blocksize, min_8bit_size, n_abs, n_fp32, extent)


def _check_tensors(what, p, specs):
    """specs: (name, tensor, dtype, need[, word]) -- every tensor contiguous, of that dtype, on p's device, with at least `need`
    elements; word: how the message names the dtype (the flat fp32 steps have always said "float32")."""
    for name, t, dt, need, *word in specs:
        if t.dtype != dt or not t.is_cuda or not t.is_contiguous() or t.numel() < need or t.device != p.device:
            raise ValueError(f"{what}: {name} must be a contiguous {word[0] if word else dt} tensor on {p.device} with >= {need} elements")


def adam8bit_step(p, g, q1, q2, absmax1, absmax2, m32, v32, layout, qmap1, qmap2, lr, betas, eps, weight_decay, step, gnorm_sq=None,
                  max_norm=0.0, grad_scale=1.0):
    """One blockwise 8-bit Adam step (bitsandbytes' Adam8bit / AdamW8bit state layout) over the flat buffers p / g; see qfx.h.
    q1 / q2: uint8 codes indexed like p; absmax1 / absmax2: fp32[>= layout.n_absmax]; m32 / v32: fp32[>= layout.n_fp32] (one element
    when unused); qmap1 / qmap2: fp32[256] ascending."""
    f32, u8 = torch.float32, torch.uint8
    _check_tensors("adam8bit_step", p, (("p", p, f32, layout.extent), ("g", g, f32, layout.extent), ("q1", q1, u8, layout.extent),
                                        ("q2", q2, u8, layout.extent), ("absmax1", absmax1, f32, max(1, layout.n_absmax)),
                                        ("absmax2", absmax2, f32, max(1, layout.n_absmax)), ("m32", m32, f32, max(1, layout.n_fp32)),
                                        ("v32", v32, f32, max(1, layout.n_fp32)), ("qmap1", qmap1, f32, 256), ("qmap2", qmap2, f32, 256)))
    if layout.table.device != p.device:
        raise ValueError("adam8bit_step: the block table lives on another device")
    a = L.Adam8bitArgs(_p(p), _p(g), _p(q1), _p(q2), _p(absmax1), _p(absmax2), _p(m32), _p(v32), _p(layout.table), layout.n_blocks,
                       layout.blocksize, _p(qmap1), _p(qmap2), lr, betas[0], betas[1], eps, weight_decay, int(step), _p(gnorm_sq),
                       max_norm, grad_scale)
    L.check(lib.qfx_adam8bit_step(a, stream_ptr()), "qfx_adam8bit_step")


def lion_step(p, g, m, lr, beta1, beta2, weight_decay=0.0, gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
    """One Lion step (lion_pytorch.Lion / bitsandbytes.optim.Lion) over the flat fp32 buffers p / g with the one moment m; see qfx.h."""
    _check_tensors("lion_step", p, [(n, t, torch.float32, p.numel(), "float32") for n, t in (("p", p),) + (("g", g), ("m", m))])
    L.check(lib.qfx_lion_step(_p(p), _p(g), _p(m), p.numel(), lr, beta1, beta2, weight_decay, _p(gnorm_sq), max_norm, grad_scale,
                              stream_ptr()), "qfx_lion_step")


def lion8bit_step(p, g, q1, absmax1, m32, layout, qmap1, lr, betas, weight_decay=0.0, gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
    """One blockwise 8-bit Lion step (bitsandbytes' Lion8bit state layout) over the flat buffers p / g; see qfx.h.  layout: an
    adam8bit_block_table; q1: uint8 codes indexed like p; absmax1: fp32[>= layout.n_absmax]; m32: fp32[>= layout.n_fp32] (one element
    when unused); qmap1: fp32[256] ascending."""
    f32, u8 = torch.float32, torch.uint8
    _check_tensors("lion8bit_step", p, (("p", p, f32, layout.extent), ("g", g, f32, layout.extent), ("q1", q1, u8, layout.extent),
                                        ("absmax1", absmax1, f32, max(1, layout.n_absmax)), ("m32", m32, f32, max(1, layout.n_fp32)),
                                        ("qmap1", qmap1, f32, 256)))
    if layout.table.device != p.device:
        raise ValueError("lion8bit_step: the block table lives on another device")
    a = L.Lion8bitArgs(_p(p), _p(g), _p(q1), _p(absmax1), _p(m32), _p(layout.table), layout.n_blocks, layout.blocksize, _p(qmap1),
                       lr, betas[0], betas[1], weight_decay, _p(gnorm_sq), max_norm, grad_scale)
    L.check(lib.qfx_lion8bit_step(a, stream_ptr()), "qfx_lion8bit_step")


# ---- parameter groups (qfx.h): the one-byte maps from the flat layout to a group, and the grouped step launches
MAX_PARAM_GROUPS = L.MAX_PARAM_GROUPS


def grouped_sweep_elems(blocksize=0):
    """Elements one grid sweep of a grouped launcher covers (0: the fp32 kernels; 256 / 2048: the blockwise kernels)."""
    return int(lib.qfx_grouped_sweep_elems(int(blocksize)))


def _check_assign(what, n_entries, assign, n_groups):
    if not 1 <= n_groups <= MAX_PARAM_GROUPS:
        raise ValueError(f"{what}: {n_groups} parameter groups, 1 to {MAX_PARAM_GROUPS} are supported")
    if len(assign) != n_entries:
        raise ValueError(f"{what}: {len(assign)} group indices for {n_entries} tensors")
    for i, gi in enumerate(assign):
        if int(gi) != gi or not 0 <= gi < n_groups:
            raise ValueError(f"{what}: tensor {i} is assigned to group {gi}, outside 0..{n_groups - 1}")


def tile_group_map(entries, assign, n_groups, numel=None, device=None):
    """uint8[ceil(numel / 64)]: the group of every 64-element tile of the flat buffers.  entries: (offset, numel) of every tensor, in
    ascending order, every offset a multiple of 64 (LoraStore's layout: a tile never holds two tensors); assign[i]: the group of
    tensor i.  The padding behind a tensor (the tail of its last tile, and any whole tile up to the next tensor) carries the tensor's
    group.  Range-checked here, on the host, before the upload: the kernels cannot."""
    _check_assign("tile_group_map", len(entries), assign, n_groups)
    extent = max((int(off) + int(k) for off, k in entries), default=0)
    numel = extent if numel is None else int(numel)
    if not entries or numel < extent:
        raise ValueError(f"tile_group_map: {len(entries)} tensors up to element {extent} in a buffer of {numel}")
    tiles = torch.empty((numel + 63) // 64, dtype=torch.uint8)
    last = 0
    for i, ((off, k), gi) in enumerate(zip(entries, assign)):
        off, k = int(off), int(k)
        if off % 64 or k <= 0 or off < last:
            raise ValueError(f"tile_group_map: tensor {i} at offset {off} with {k} elements (offsets are ascending multiples of 64)")
        nxt = int(entries[i + 1][0]) // 64 if i + 1 < len(entries) else tiles.numel()
        tiles[off // 64 if i else 0:nxt] = int(gi)
        last = off + k
    return tiles if device is None else tiles.to(device)


def block_group_map(layout, assign, n_groups, device=None):
    """uint8[layout.n_blocks]: the group of every entry of an adam8bit_block_table (its rows are per tensor, in entry order: an entry
    never spans two tensors, so never two groups).  Range-checked on the host before the upload."""
    _check_assign("block_group_map", len(layout.tensors), assign, n_groups)
    rows = []
    for (off, k, *_), gi in zip(layout.tensors, assign):
        rows += [int(gi)] * ((k + layout.blocksize - 1) // layout.blocksize)
    if len(rows) != layout.n_blocks:
        raise ValueError(f"block_group_map: {len(rows)} rows for a table of {layout.n_blocks}")
    t = torch.tensor(rows, dtype=torch.uint8)
    return t if device is None else t.to(device)


def _group_rows(what, ctype, rows, tmap, need, p):
    if not 1 <= len(rows) <= MAX_PARAM_GROUPS:
        raise ValueError(f"{what}: {len(rows)} parameter groups, 1 to {MAX_PARAM_GROUPS} are supported")
    _check_tensors(what, p, (("the group map", tmap, torch.uint8, need),))
    return (ctype * len(rows))(*[ctype(*r) for r in rows])


def adamw_step_grouped(p, g, m, v, tile_group, groups, step, gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
    """adamw_step with per-group hyperparameters: groups = [(lr, beta1, beta2, eps, weight_decay)], tile_group from tile_group_map."""
    rows = _group_rows("adamw_step_grouped", L.AdamwGroup, [(lr, b1, b2, eps, wd, 1.0 - b1 ** step, 1.0 - b2 ** step)
                                                            for lr, b1, b2, eps, wd in groups], tile_group, (p.numel() + 63) // 64, p)
    _check_tensors("adamw_step_grouped", p, [(n, t, torch.float32, p.numel(), "float32") for n, t in (("p", p), ("g", g), ("m", m), ("v", v))])
    L.check(lib.qfx_adamw_step_grouped(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(tile_group), rows, len(groups), _p(gnorm_sq), max_norm,
                                       grad_scale, stream_ptr()), "qfx_adamw_step_grouped")


def sgd_step_grouped(p, g, buf, tile_group, groups, first=False, gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
    """sgd_step with per-group hyperparameters: groups = [(lr, momentum, dampening, weight_decay, nesterov)]; buf: None iff every
    group's momentum is 0."""
    rows = _group_rows("sgd_step_grouped", L.SgdGroup, [(lr, mom, damp, wd, int(bool(nes))) for lr, mom, damp, wd, nes in groups],
                       tile_group, (p.numel() + 63) // 64, p)
    _check_tensors("sgd_step_grouped", p, [(n, t, torch.float32, p.numel(), "float32") for n, t in (("p", p), ("g", g)) + ((("buf", buf),) if buf is not None else ())])
    L.check(lib.qfx_sgd_step_grouped(_p(p), _p(g), _p(buf), p.numel(), _p(tile_group), rows, len(groups), int(bool(first)), _p(gnorm_sq),
                                     max_norm, grad_scale, stream_ptr()), "qfx_sgd_step_grouped")


def lion_step_grouped(p, g, m, tile_group, groups, gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
    """lion_step with per-group hyperparameters: groups = [(lr, beta1, beta2, weight_decay)]."""
    rows = _group_rows("lion_step_grouped", L.LionGroup, groups, tile_group, (p.numel() + 63) // 64, p)
    _check_tensors("lion_step_grouped", p, [(n, t, torch.float32, p.numel(), "float32") for n, t in (("p", p), ("g", g), ("m", m))])
    L.check(lib.qfx_lion_step_grouped(_p(p), _p(g), _p(m), p.numel(), _p(tile_group), rows, len(groups), _p(gnorm_sq), max_norm,
                                      grad_scale, stream_ptr()), "qfx_lion_step_grouped")


def adam8bit_step_grouped(p, g, q1, q2, absmax1, absmax2, m32, v32, layout, qmap1, qmap2, block_group, groups, step, gnorm_sq=None,
                          max_norm=0.0, grad_scale=1.0):
    """adam8bit_step with per-group hyperparameters: groups = [(lr, beta1, beta2, eps, weight_decay)], block_group from block_group_map."""
    f32, u8 = torch.float32, torch.uint8
    rows = _group_rows("adam8bit_step_grouped", L.Adam8bitGroup, groups, block_group, layout.n_blocks, p)
    _check_tensors("adam8bit_step_grouped", p, (("p", p, f32, layout.extent), ("g", g, f32, layout.extent), ("q1", q1, u8, layout.extent),
                                                ("q2", q2, u8, layout.extent), ("absmax1", absmax1, f32, max(1, layout.n_absmax)),
                                                ("absmax2", absmax2, f32, max(1, layout.n_absmax)), ("m32", m32, f32, max(1, layout.n_fp32)),
                                                ("v32", v32, f32, max(1, layout.n_fp32)), ("qmap1", qmap1, f32, 256), ("qmap2", qmap2, f32, 256)))
    if layout.table.device != p.device:
        raise ValueError("adam8bit_step_grouped: the block table lives on another device")
    a = L.Adam8bitArgs(_p(p), _p(g), _p(q1), _p(q2), _p(absmax1), _p(absmax2), _p(m32), _p(v32), _p(layout.table), layout.n_blocks,
                       layout.blocksize, _p(qmap1), _p(qmap2), 0.0, 0.0, 0.0, 0.0, 0.0, int(step), _p(gnorm_sq), max_norm, grad_scale)
    L.check(lib.qfx_adam8bit_step_grouped(a, _p(block_group), rows, len(groups), stream_ptr()), "qfx_adam8bit_step_grouped")


def lion8bit_step_grouped(p, g, q1, absmax1, m32, layout, qmap1, block_group, groups, gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
    """lion8bit_step with per-group hyperparameters: groups = [(lr, beta1, beta2, weight_decay)]."""
    f32, u8 = torch.float32, torch.uint8
    rows = _group_rows("lion8bit_step_grouped", L.LionGroup, groups, block_group, layout.n_blocks, p)
    _check_tensors("lion8bit_step_grouped", p, (("p", p, f32, layout.extent), ("g", g, f32, layout.extent), ("q1", q1, u8, layout.extent),
                                                ("absmax1", absmax1, f32, max(1, layout.n_absmax)), ("m32", m32, f32, max(1, layout.n_fp32)),
                                                ("qmap1", qmap1, f32, 256)))
    if layout.table.device != p.device:
        raise ValueError("lion8bit_step_grouped: the block table lives on another device")
    a = L.Lion8bitArgs(_p(p), _p(g), _p(q1), _p(absmax1), _p(m32), _p(layout.table), layout.n_blocks, layout.blocksize, _p(qmap1),
                       0.0, 0.0, 0.0, 0.0, _p(gnorm_sq), max_norm, grad_scale)
    L.check(lib.qfx_lion8bit_step_grouped(a, _p(block_group), rows, len(groups), stream_ptr()), "qfx_lion8bit_step_grouped")


# ---- torch.optim.RAdam / NAdam / Adamax (qfx.h: qfx_adamx_step).  The per-step scalars torch forms as Python floats, formed here as
# torch forms them (the same double expressions, statement for statement) and rounded to the row's floats
ADAMX_VARIANTS = {"radam": L.ADAMX_RADAM, "nadam": L.ADAMX_NADAM, "adamax": L.ADAMX_ADAMAX}


def adamx_check(lr, betas, eps, weight_decay, momentum_decay=0.0):
    """The constructor checks torch.optim.RAdam / NAdam / Adamax share, with their messages."""
    if not 0.0 <= lr:
        raise ValueError(f"Invalid learning rate: {lr}")
    if not 0.0 <= eps:
        raise ValueError(f"Invalid epsilon value: {eps}")
    if len(betas) != 2:
        raise ValueError(f"betas is a pair (beta1, beta2), not {betas!r}")
    for i in (0, 1):
        if not 0.0 <= betas[i] < 1.0:
            raise ValueError(f"Invalid beta parameter at index {i}: {betas[i]}")
    if not 0.0 <= weight_decay:
        raise ValueError(f"Invalid weight_decay value: {weight_decay}")
    if not 0.0 <= momentum_decay:
        raise ValueError(f"Invalid momentum_decay value: {momentum_decay}")


def radam_scalars(step, beta1, beta2):
    """_single_tensor_radam's Python floats at step `step` (from 1): (bias_correction1, bias_correction2 ** 0.5, rho_t > 5, the
    rectification factor or 0.0 where it does not apply)."""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    rho_inf = 2 / (1 - beta2) - 1
    rho_t = rho_inf - 2 * step * (beta2 ** step) / bias_correction2
    if not rho_t > 5.0:
        return bias_correction1, bias_correction2 ** 0.5, False, 0.0
    rect = ((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)) ** 0.5
    return bias_correction1, bias_correction2 ** 0.5, True, rect


def nadam_mu(step, beta1, momentum_decay):
    """(mu_t, mu_{t+1}) of _single_tensor_nadam."""
    mu = beta1 * (1.0 - 0.5 * (0.96 ** (step * momentum_decay)))
    mu_next = beta1 * (1.0 - 0.5 * (0.96 ** ((step + 1) * momentum_decay)))
    return mu, mu_next


def nadam_scalars(step, lr, beta1, beta2, momentum_decay, mu_product):
    """_single_tensor_nadam's Python floats at step `step`: mu_product, torch's 0-dim fp32 CPU tensor (the product through step - 1),
    is advanced IN PLACE as torch advances it (`mu_product *= mu`: one fp32 rounding per step, no device involved); returns
    (bias_correction2, the value= of the gradient's addcdiv_, the value= of exp_avg's)."""
    bias_correction2 = 1 - beta2 ** step
    mu, mu_next = nadam_mu(step, beta1, momentum_decay)
    mu_product *= mu
    mp = mu_product.item()
    mu_product_next = mp * mu_next
    return bias_correction2, -lr * (1.0 - mu) / (1.0 - mp), (-lr * mu_next) / (1.0 - mu_product_next)


def adamx_rows(variant, groups, step, mu_products=None):
    """The rows of qfx_adamx_step: groups = [dict(lr, betas, eps, weight_decay[, decoupled_weight_decay][, momentum_decay])] -> a list
    of field tuples in AdamxGroup's order.  "nadam": mu_products = one 0-dim fp32 CPU tensor per group, advanced in place."""
    rows = []
    for k, r in enumerate(groups):
        lr, (beta1, beta2), eps, wd = float(r["lr"]), r["betas"], r["eps"], r["weight_decay"]
        decoupled = bool(r.get("decoupled_weight_decay", False)) and variant != "adamax"
        bc1 = bc2 = sq2 = rect = c_grad = c_avg = neg_clr = 0.0
        rectified = False
        if variant == "radam":
            bc1, sq2, rectified, rect = radam_scalars(step, beta1, beta2)
        elif variant == "nadam":
            bc2, c_grad, c_avg = nadam_scalars(step, lr, beta1, beta2, r.get("momentum_decay", 4e-3), mu_products[k])
        else:
            neg_clr = -(lr / (1 - beta1 ** step))
        rows.append((lr, beta1, beta2, eps, wd, 1 - beta1, 1 - beta2, 1 - lr * wd, bc1, bc2, sq2, rect, c_grad, c_avg, neg_clr,
                     int(decoupled), int(rectified), 0))
    return rows


def adamx_step(variant, p, g, exp_avg, state2, groups, step, tile_group=None, mu_products=None, gnorm_sq=None, max_norm=0.0,
               grad_scale=1.0):
    """One torch.optim.RAdam / NAdam / Adamax step (variant "radam" | "nadam" | "adamax") over the flat fp32 buffers p / g with
    exp_avg and state2 (exp_avg_sq, Adamax: exp_inf); see qfx.h.  groups: one dict per parameter group (adamx_rows); tile_group from
    tile_group_map, None with one group; step: the count this step brings the state to (from 1)."""
    if variant not in ADAMX_VARIANTS:
        raise ValueError(f"adamx_step: unknown variant {variant!r}")
    what = f"adamx_step({variant})"
    if not 1 <= len(groups) <= MAX_PARAM_GROUPS:
        raise ValueError(f"{what}: {len(groups)} parameter groups, 1 to {MAX_PARAM_GROUPS} are supported")
    if tile_group is None and len(groups) != 1:
        raise ValueError(f"{what}: {len(groups)} parameter groups need a group map")
    for r in groups:
        adamx_check(r["lr"], r["betas"], r["eps"], r["weight_decay"], r.get("momentum_decay", 0.0))
    _check_tensors(what, p, [(n, t, torch.float32, p.numel(), "float32") for n, t in (("p", p), ("g", g), ("exp_avg", exp_avg),
                                                                                       ("state2", state2))])
    if tile_group is not None:
        _check_tensors(what, p, (("the group map", tile_group, torch.uint8, (p.numel() + 63) // 64),))
    rows = adamx_rows(variant, groups, step, mu_products)
    arr = (L.AdamxGroup * len(rows))(*[L.AdamxGroup(*r) for r in rows])
    a = L.AdamxArgs(_p(p), _p(g), _p(exp_avg), _p(state2), p.numel(), ADAMX_VARIANTS[variant], len(rows), arr, _p(tile_group),
                    _p(gnorm_sq), max_norm, grad_scale)
    L.check(lib.qfx_adamx_step(a, stream_ptr()), "qfx_adamx_step")


# ---- AdEMAMix (qfx.h: qfx_ademamix_step / qfx_ademamix8bit_step).  The listing in include/qfx.h is the specification; the two
# schedules and every other per-step scalar are formed here in double, per group and per step, and rounded to the row's floats
def ademamix_check(lr, betas, eps, weight_decay, alpha=5.0, t_alpha=None, t_beta3=None):
    """The constructor checks of the AdEMAMix classes: lr, eps, weight_decay and alpha >= 0, three betas each in [0, 1), t_alpha /
    t_beta3 None or > 0.  The beta3 schedule interpolates ln(beta): with t_beta3, beta1 and beta3 must be > 0."""
    if not 0.0 <= lr:
        raise ValueError(f"Invalid learning rate: {lr}")
    if not 0.0 <= eps:
        raise ValueError(f"Invalid epsilon value: {eps}")
    if not isinstance(betas, (tuple, list)) or len(betas) != 3:
        raise ValueError(f"AdEMAMix's betas is a triple (beta1, beta2, beta3), not {betas!r}")
    for i in (0, 1, 2):
        if not 0.0 <= betas[i] < 1.0:
            raise ValueError(f"Invalid beta parameter at index {i}: {betas[i]}")
    if not 0.0 <= weight_decay:
        raise ValueError(f"Invalid weight_decay value: {weight_decay}")
    if not 0.0 <= alpha:
        raise ValueError(f"Invalid alpha value: {alpha}")
    for n, t in (("t_alpha", t_alpha), ("t_beta3", t_beta3)):
        if t is not None and not t > 0:
            raise ValueError(f"Invalid {n} value: {t} (None or > 0)")
    if t_beta3 is not None and not (betas[0] > 0.0 and betas[2] > 0.0):
        raise ValueError(f"the beta3 schedule (t_beta3={t_beta3}) interpolates ln(beta): beta1 and beta3 must be > 0, not {betas!r}")


def ademamix_alpha(step, alpha, t_alpha=None):
    """alpha_t at step `step` (from 1): the linear warm-up of the slow average's weight, alpha from t_alpha on."""
    return alpha if t_alpha is None else min(step * alpha / t_alpha, alpha)


def ademamix_beta3(step, beta1, beta3, t_beta3=None):
    """beta3_t at step `step` (from 1): the slow average's rate, warmed up from beta1 so that its half-life grows linearly."""
    if t_beta3 is None:
        return beta3
    s = step / t_beta3
    ln1, ln3 = math.log(beta1), math.log(beta3)
    return min(math.exp(ln1 * ln3 / ((1 - s) * ln3 + s * ln1)), beta3)


def ademamix_rows(groups, step):
    """The rows of the AdEMAMix entries: groups = [dict(lr, betas (the triple), eps, weight_decay[, alpha][, t_alpha][, t_beta3])] -> a
    list of field tuples in AdemamixGroup's order, every scalar formed in double."""
    rows = []
    for r in groups:
        lr, (beta1, beta2, beta3), eps, wd = float(r["lr"]), r["betas"], r["eps"], r["weight_decay"]
        b3t = ademamix_beta3(step, beta1, beta3, r.get("t_beta3"))
        rows.append((lr, beta1, beta2, eps, wd, 1 - beta1, 1 - beta2, b3t, 1 - b3t, ademamix_alpha(step, r.get("alpha", 5.0), r.get("t_alpha")),
                     1 - beta1 ** step, math.sqrt(1 - beta2 ** step), 1 - lr * wd))
    return rows


def _ademamix_groups(what, groups, need_map):
    if not 1 <= len(groups) <= MAX_PARAM_GROUPS:
        raise ValueError(f"{what}: {len(groups)} parameter groups, 1 to {MAX_PARAM_GROUPS} are supported")
    if need_map and len(groups) != 1:
        raise ValueError(f"{what}: {len(groups)} parameter groups need a group map")
    for r in groups:
        ademamix_check(r["lr"], r["betas"], r["eps"], r["weight_decay"], r.get("alpha", 5.0), r.get("t_alpha"), r.get("t_beta3"))


def ademamix_step(p, g, m1, m2, nu, groups, step, tile_group=None, gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
    """One AdEMAMix step over the flat fp32 buffers p / g with the fast average m1, the slow average m2 and the second moment nu; see
    qfx.h.  groups: one dict per parameter group (ademamix_rows); tile_group from tile_group_map, None with one group; step: the count
    this step brings the state to (from 1) -- both schedules and the bias corrections depend on it."""
    what = "ademamix_step"
    _ademamix_groups(what, groups, tile_group is None)
    _check_tensors(what, p, [(n, t, torch.float32, p.numel(), "float32") for n, t in (("p", p), ("g", g), ("m1", m1), ("m2", m2), ("nu", nu))])
    if tile_group is not None:
        _check_tensors(what, p, (("the group map", tile_group, torch.uint8, (p.numel() + 63) // 64),))
    rows = ademamix_rows(groups, step)
    arr = (L.AdemamixGroup * len(rows))(*[L.AdemamixGroup(*r) for r in rows])
    a = L.AdemamixArgs(_p(p), _p(g), _p(m1), _p(m2), _p(nu), p.numel(), len(rows), 0, arr, _p(tile_group), _p(gnorm_sq), max_norm,
                       grad_scale)
    L.check(lib.qfx_ademamix_step(a, stream_ptr()), "qfx_ademamix_step")


def ademamix8bit_step(p, g, q1, q2, absmax1, absmax2, m32, v32, layout, qmap1, qmap2, groups, step, block_group=None, gnorm_sq=None,
                      max_norm=0.0, grad_scale=1.0):
    """One blockwise 8-bit AdEMAMix step (bitsandbytes' AdEMAMix8bit state layout) over the flat buffers p / g; see qfx.h.  layout: an
    adam8bit_block_table.  state1 holds both averages: q1 uint8[2, plane >= layout.extent] (plane 0 = m1, plane 1 = m2, each indexed
    like p), absmax1 fp32[2, >= layout.n_absmax], m32 fp32[2, >= layout.n_fp32]; q2 / absmax2 / v32 hold nu as adam8bit_step's do;
    the planes of q1 and m32 are multiples of 4 long.  groups / step as ademamix_step's; block_group (block_group_map) selects the
    grouped entry and may be None with one group."""
    what = "ademamix8bit_step"
    f32, u8 = torch.float32, torch.uint8
    _ademamix_groups(what, groups, block_group is None)
    for n, t, need in (("q1", q1, layout.extent), ("absmax1", absmax1, max(1, layout.n_absmax)), ("m32", m32, max(1, layout.n_fp32))):
        if t.dim() != 2 or t.shape[0] != 2 or t.shape[1] < need or (n != "absmax1" and t.shape[1] % 4):
            raise ValueError(f"{what}: {n} must be shaped [2, plane] with plane >= {need}" + ("" if n == "absmax1" else " and a multiple of 4") +
                             f", not {tuple(t.shape)}")
    _check_tensors(what, p, (("p", p, f32, layout.extent), ("g", g, f32, layout.extent), ("q1", q1, u8, 2 * layout.extent),
                             ("q2", q2, u8, layout.extent), ("absmax1", absmax1, f32, 2 * max(1, layout.n_absmax)),
                             ("absmax2", absmax2, f32, max(1, layout.n_absmax)), ("m32", m32, f32, 2 * max(1, layout.n_fp32)),
                             ("v32", v32, f32, max(1, layout.n_fp32)), ("qmap1", qmap1, f32, 256), ("qmap2", qmap2, f32, 256)))
    if layout.table.device != p.device:
        raise ValueError(f"{what}: the block table lives on another device")
    rows = ademamix_rows(groups, step)
    a = L.Ademamix8bitArgs(_p(p), _p(g), _p(q1), _p(q2), _p(absmax1), _p(absmax2), _p(m32), _p(v32), q1.shape[1], absmax1.shape[1],
                           m32.shape[1], _p(layout.table), layout.n_blocks, layout.blocksize, _p(qmap1), _p(qmap2),
                           L.AdemamixGroup(*rows[0]), _p(gnorm_sq), max_norm, grad_scale)
    if block_group is None:
        return L.check(lib.qfx_ademamix8bit_step(a, stream_ptr()), "qfx_ademamix8bit_step")
    _check_tensors(what, p, (("the group map", block_group, torch.uint8, layout.n_blocks),))
    arr = (L.AdemamixGroup * len(rows))(*[L.AdemamixGroup(*r) for r in rows])
    L.check(lib.qfx_ademamix8bit_step_grouped(a, _p(block_group), arr, len(rows), stream_ptr()), "qfx_ademamix8bit_step_grouped")


def sfadamw_schedule(k, lr, beta2, warmup_steps, r, weight_lr_power, lr_max, weight_sum):
    """The group scalars of Schedule-Free AdamW's step k (counted from 0), in Python doubles as schedulefree.AdamWScheduleFree forms
    them: (lr_t, bias_corr2, ckp1, lr_max, weight_sum) with the two running values updated."""
    sched = (k + 1) / warmup_steps if k < warmup_steps else 1.0
    bc2 = 1 - beta2 ** (k + 1)
    lr_t = lr * sched
    lr_max = max(lr_t, lr_max)
    weight = ((k + 1) ** r) * (lr_max ** weight_lr_power)
    weight_sum = weight_sum + weight
    ckp1 = weight / weight_sum if weight_sum != 0 else 0.0
    return lr_t, bc2, ckp1, lr_max, weight_sum


def sfadamw_step(p, g, z, v, lr_t, beta1, beta2, eps, weight_decay, bias_corr2, ckp1, first=False, gnorm_sq=None, max_norm=0.0,
                 grad_scale=1.0):
    """One Schedule-Free AdamW step (schedulefree.AdamWScheduleFree) over the flat fp32 buffers: p holds y, z the base sequence, v
    exp_avg_sq; lr_t, bias_corr2 and ckp1 from sfadamw_schedule; first: z = y and v = 0 are taken, not read; see qfx.h."""
    _check_tensors("sfadamw_step", p, [(n, t, torch.float32, p.numel(), "float32") for n, t in (("p", p),) + (("g", g), ("z", z), ("v", v))])
    L.check(lib.qfx_sfadamw_step(_p(p), _p(g), _p(z), _p(v), p.numel(), lr_t, beta1, beta2, eps, weight_decay, bias_corr2, ckp1,
                                 int(bool(first)), _p(gnorm_sq), max_norm, grad_scale, stream_ptr()), "qfx_sfadamw_step")


def sf_swap(p, z, beta1, to_eval):
    """Schedule-free mode swap in place: y -> x = lerp(y, z, 1 - 1 / beta1) (to_eval) or x -> y = lerp(x, z, 1 - beta1); see qfx.h."""
    if not 0.0 < beta1 < 1.0:
        raise ValueError(f"sf_swap: beta1 must lie in (0, 1) for the train / eval swap, not {beta1!r}")
    _check_tensors("sf_swap", p, [(n, t, torch.float32, p.numel(), "float32") for n, t in (("p", p),) + (("z", z),)])
    L.check(lib.qfx_sf_swap(_p(p), _p(z), p.numel(), 1.0 - 1.0 / beta1 if to_eval else 1.0 - beta1, stream_ptr()), "qfx_sf_swap")


EMA_MAX_SHADOWS = L.EMA_MAX_SHADOWS


def ema_update(p, shadows, one_minus_decays):
    """One EMA step of up to EMA_MAX_SHADOWS shadow buffers towards p in ONE launch: s_k -= float32(omd_k) * (s_k - p), the three
    roundings of diffusers' EMAModel.step; p is read once and not written.  See qfx.h."""
    if not 1 <= len(shadows) <= EMA_MAX_SHADOWS or len(one_minus_decays) != len(shadows):
        raise ValueError(f"ema_update: 1..{EMA_MAX_SHADOWS} shadows and one rate for each, not {len(shadows)} and {len(one_minus_decays)}")
    _check_tensors("ema_update", p, [("p", p, torch.float32, p.numel(), "float32")] +
                   [(f"shadow {k}", s, torch.float32, p.numel(), "float32") for k, s in enumerate(shadows)])
    a = L.EmaArgs()
    for k, (s, omd) in enumerate(zip(shadows, one_minus_decays)):
        a.shadow[k], a.one_minus_decay[k] = _p(s), omd
    a.n_shadows = len(shadows)
    L.check(lib.qfx_ema_update(_p(p), p.numel(), C.byref(a), stream_ptr()), "qfx_ema_update")


def ema_swap(p, s):
    """Exchange the contents of the flat fp32 buffers p and s bit for bit, in ONE launch; see qfx.h."""
    _check_tensors("ema_swap", p, [(n, t, torch.float32, p.numel(), "float32") for n, t in (("p", p), ("s", s))])
    L.check(lib.qfx_ema_swap(_p(p), _p(s), p.numel(), stream_ptr()), "qfx_ema_swap")


MAXNORM_MAX_RANK = 128


class PairLayout:
    """Descriptor table of one flat-buffer layout for a per-pair kernel, built once per layout (and, for scaled AdamW, grouping).
    `pairs[i]` = (off_a, off_b, r, in_features, out_features, ...) of adapter pair i, the rest of the row as its table builder
    documents it; extent: elements the flat buffers need; host: the ctypes array the device table was made from."""

    def __init__(self, table, pairs, extent, host=None):
        self.table, self.pairs, self.extent, self.host = table, pairs, extent, host
        self.n_pairs = len(pairs)


MaxnormLayout = ScaledAdamwLayout = LoraSvdLayout = PairLayout


def _table_tensor(arr, device):
    """The bytes of a ctypes array as a uint8 tensor, on `device` if one is given."""
    t = torch.frombuffer(bytearray(arr), dtype=torch.uint8)
    return t if device is None else t.to(device)


# What differs between the descriptor tables: the name in qfx_<what>_check_table and in the messages, the ctypes row, the rank cap,
# what the check may have refused, and the wording of a rank above the cap and of an empty table.
_TableSpec = collections.namedtuple("_TableSpec", "what ctype cap refused over none",
                                    defaults=("pair {i} has rank {r}: ranks above {cap} are not implemented", "pairs"))
_BuiltTable = collections.namedtuple("_BuiltTable", "table rows extent host")


def _pair_table(spec, rows, device, n_elems):
    """The common part of the descriptor-table builders.  rows: an iterable of (row, ctypes fields) with row = (off_a, off_b, rank,
    in_features, out_features, ...) already coerced.  A rank above spec.cap is a NotImplementedError; an empty table and a table
    that qfx_<what>_check_table refuses against n_elems (default: the extent of the rows themselves) are ValueErrors."""
    kept, structs, extent = [], [], 0
    for i, (row, fields) in enumerate(rows):
        if row[2] > spec.cap:
            raise NotImplementedError(f"{spec.what} table: " + spec.over.format(i=i, r=row[2], cap=spec.cap))
        kept.append(row)
        structs.append(spec.ctype(*fields))
        extent = max(extent, row[0] + row[2] * row[3], row[1] + row[4] * row[2])
    if not kept:
        raise ValueError(f"{spec.what} table: no {spec.none}")
    arr = (spec.ctype * len(kept))(*structs)
    if getattr(lib, f"qfx_{spec.what}_check_table")(arr, len(kept), extent if n_elems is None else int(n_elems)) != 0:
        raise ValueError(f"{spec.what} table: refused by qfx_{spec.what}_check_table ({spec.refused})")
    return _BuiltTable(_table_tensor(arr, device), kept, extent, arr)


def _pair_layout(spec, rows, device, n_elems):
    b = _pair_table(spec, rows, device, n_elems)
    return PairLayout(table=b.table, pairs=b.rows, extent=b.extent, host=b.host)


_MAXNORM_TABLE = _TableSpec("maxnorm", L.MaxnormPair, MAXNORM_MAX_RANK, refused="a dimension, an offset, an overlap or a scale")


def maxnorm_table(pairs, device=None, n_elems=None):
    """pairs: (off_a, off_b, r, in_features, out_features, scale) of every adapter pair in the flat buffer -- A [r, in] at off_a,
    B [out, r] at off_b, scale = lora_alpha / r.  Checked by qfx_maxnorm_check_table against n_elems (default: the extent of the
    pairs themselves) before it goes to the device."""
    def rows():
        for off_a, off_b, r, nin, nout, scale in pairs:
            row = (int(off_a), int(off_b), int(r), int(nin), int(nout), float(scale))
            yield row, row
    return _pair_layout(_MAXNORM_TABLE, rows(), device, n_elems)


def maxnorm_apply(pflat, table, max_norm, norms, ratios, summary):
    """kohya's apply_max_norm_regularization over the flat fp32 buffer in ONE launch (plus the one-block summary): every pair of
    `table` (a maxnorm_table) whose ||scale B A||_F exceeds max_norm is scaled onto it in place; norms / ratios [n_pairs] and
    summary [4] = (keys_scaled, mean norm, max norm, 0) are written on the device, nothing synchronises.  See qfx.h."""
    max_norm = float(max_norm)
    if not max_norm > 0:
        raise ValueError(f"maxnorm_apply: max_norm must be positive (inf allowed), not {max_norm}")
    for name, t, n in (("pflat", pflat, table.extent), ("norms", norms, table.n_pairs), ("ratios", ratios, table.n_pairs),
                       ("summary", summary, 4)):
        if t is None or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() < n or t.device != pflat.device:
            raise ValueError(f"maxnorm_apply: {name} must be a contiguous float32 tensor on {pflat.device} with >= {n} elements")
    if table.table.device != pflat.device:
        raise ValueError("maxnorm_apply: the descriptor table lives on another device")
    a = L.MaxnormArgs(_p(pflat), _p(table.table), table.n_pairs, max_norm, _p(norms), _p(ratios), _p(summary))
    L.check(lib.qfx_maxnorm_apply(a, stream_ptr()), "qfx_maxnorm_apply")


LORA_SVD_MAX_RANK = 64
LORA_SVD_RANK_TOL = 1e-6
LORA_SVD_MAX_SWEEPS = 30
LORA_SVD_WS_DOUBLES = 2 * 64 * 64          # per pair: T_B and T_A, [64][64] fp64 each


_LORA_SVD_TABLE = _TableSpec("lora_svd", L.LoraSvdPair, LORA_SVD_MAX_RANK, refused="a dimension, an offset or an overlap")


def lora_svd_table(pairs, device=None, n_elems=None):
    """pairs: (off_a, off_b, r, in_features, out_features) of every adapter pair in the flat buffer -- A [r, in] at off_a,
    B [out, r] at off_b.  Checked by qfx_lora_svd_check_table against n_elems (default: the extent of the pairs themselves)
    before it goes to the device."""
    def rows():
        for off_a, off_b, r, nin, nout in pairs:
            row = (int(off_a), int(off_b), int(r), int(nin), int(nout))
            yield row, row + (0,)
    return _pair_layout(_LORA_SVD_TABLE, rows(), device, n_elems)


def _svd_buf(what, name, t, dtype, n, dev):
    if t is None or t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or t.numel() < n or t.device != dev:
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} tensor on {dev} with >= {n} elements")


def lora_spectrum(pflat, table, sv, info, skipped, ws=None, rank_tol=LORA_SVD_RANK_TOL, max_sweeps=LORA_SVD_MAX_SWEEPS):
    """The singular values of B A of every pair of `table` (a lora_svd_table) in ONE launch: sv [n_pairs, ld_sv >= 64] fp64,
    info [n_pairs, 4] int32 (numeric rank, sweeps of the two solves, converged), skipped [1] int32, and with ws
    [n_pairs * LORA_SVD_WS_DOUBLES] fp64 the transforms T_B / T_A that lora_project reads.  Nothing synchronises.  See qfx.h."""
    rank_tol, max_sweeps = float(rank_tol), int(max_sweeps)
    if not 0.0 < rank_tol < 1.0:
        raise ValueError(f"lora_spectrum: rank_tol must lie in (0, 1), not {rank_tol}")
    if not 1 <= max_sweeps <= 64:
        raise ValueError(f"lora_spectrum: max_sweeps must lie in 1..64, not {max_sweeps}")
    dev, n = pflat.device, table.n_pairs
    if sv is None or sv.dim() != 2 or sv.shape[0] < n or sv.shape[1] < 64:
        raise ValueError(f"lora_spectrum: sv must be [>= {n}, >= 64]")
    _svd_buf("lora_spectrum", "pflat", pflat, torch.float32, table.extent, dev)
    _svd_buf("lora_spectrum", "sv", sv, torch.float64, n * 64, dev)
    _svd_buf("lora_spectrum", "info", info, torch.int32, 4 * n, dev)
    _svd_buf("lora_spectrum", "skipped", skipped, torch.int32, 1, dev)
    if ws is not None:
        _svd_buf("lora_spectrum", "ws", ws, torch.float64, n * LORA_SVD_WS_DOUBLES, dev)
    if table.table.device != dev:
        raise ValueError("lora_spectrum: the descriptor table lives on another device")
    a = L.LoraSpectrumArgs(_p(pflat), _p(table.table), n, max_sweeps, rank_tol, _p(sv), sv.shape[1], _p(info),
                           _p(ws) if ws is not None else None, _p(skipped))
    L.check(lib.qfx_lora_spectrum(a, stream_ptr()), "qfx_lora_spectrum")


def lora_project_table(table, dst, device=None, n_elems=None):
    """dst: (dst_off_a, dst_off_b, k, r_dst) per pair of `table` (a lora_svd_table).  Checked by qfx_lora_project_check_table
    against n_elems, the extent of the destination buffer (default: the extent of the rows themselves).  -> (device table, extent)"""
    if len(dst) != table.n_pairs:
        raise ValueError(f"lora_project table: {len(dst)} destinations for {table.n_pairs} pairs")
    rows, extent = [], 0
    for (off_a, off_b, k, r_dst), (_, _, _, nin, nout) in zip(dst, table.pairs):
        row = (int(off_a), int(off_b), int(k), int(r_dst))
        rows.append(row)
        extent = max(extent, row[0] + row[3] * nin, row[1] + nout * row[3])
    arr = (L.LoraSvdDst * len(rows))(*[L.LoraSvdDst(*r) for r in rows])
    if lib.qfx_lora_project_check_table(table.host, arr, len(rows), extent if n_elems is None else int(n_elems)) != 0:
        raise ValueError("lora_project table: refused by qfx_lora_project_check_table (k, r_dst, an offset or an overlap)")
    return _table_tensor(arr, device), extent


def lora_project(pflat, qflat, table, dst_table, ws):
    """B' = fp32(B T_B[:, :k]), A' = fp32(T_A[:k] A) of every pair into another flat buffer, in ONE launch; dst_table from
    lora_project_table, ws what lora_spectrum wrote.  See qfx.h."""
    dev, n = pflat.device, table.n_pairs
    dst, extent = dst_table
    _svd_buf("lora_project", "pflat", pflat, torch.float32, table.extent, dev)
    _svd_buf("lora_project", "qflat", qflat, torch.float32, extent, dev)
    _svd_buf("lora_project", "ws", ws, torch.float64, n * LORA_SVD_WS_DOUBLES, dev)
    if qflat.data_ptr() == pflat.data_ptr():
        raise ValueError("lora_project: the destination must be another buffer")
    if table.table.device != dev or dst.device != dev:
        raise ValueError("lora_project: a descriptor table lives on another device")
    a = L.LoraProjectArgs(_p(pflat), _p(qflat), _p(table.table), _p(dst), n, 0, _p(ws))
    L.check(lib.qfx_lora_project(a, stream_ptr()), "qfx_lora_project")


LOWRANK_MAX_K = 64
LOWRANK_MAX_POWER_ITERS = 4
LOWRANK_ORTH_TOL = 1e-12
_LOWRANK_DTYPES = {torch.bfloat16: 0, torch.float32: 1}


class LowrankLayout:
    """Descriptor table of qfx_lowrank_sketch, built once per set of matrices.  rows[i] = (off_a, off_b, k, in_features,
    out_features): the same rows are a lora_svd_table of the output buffer with r = k.  extent: elements the output needs;
    host: the ctypes array (read again at every launch); ws_bytes: the workspace; keep: the tensors the table points at."""

    def __init__(self, table, rows, extent, host, ws_bytes, keep):
        self.table, self.rows, self.extent, self.host, self.ws_bytes, self.keep = table, rows, extent, host, ws_bytes, keep
        self.n_mats = len(rows)


_LOWRANK_TABLE = _TableSpec("lowrank", L.LowrankMat, LOWRANK_MAX_K, refused="a dimension, a leading dimension, an offset or an overlap",
                            over="matrix {i} asks for k = {r}: sketches wider than {cap} are not implemented", none="matrices")


def lowrank_table(mats, device=None, n_elems=None):
    """mats: (W1, W0 or None, k, off_a, off_b[, index]) per matrix -- W1 / W0 2-D device tensors [out, in] with unit column stride,
    both bfloat16 or both float32; Q [out, k] goes to off_b and C [k, in] to off_a of the flat output buffer; index (default: the
    position in the list) keys the test matrix.  Checked by qfx_lowrank_check_table against n_elems (default: the extent of the
    rows themselves) before it goes to the device."""
    keep = []

    def described():
        for i, mat in enumerate(mats):
            W1, W0, k, off_a, off_b = mat[:5]
            index = int(mat[5]) if len(mat) > 5 else i
            if W1 is None or W1.dim() != 2 or W1.dtype not in _LOWRANK_DTYPES or W1.stride(1) != 1:
                raise ValueError(f"lowrank table: matrix {i}: W1 must be a 2-D bfloat16 or float32 tensor with unit column stride")
            if W0 is not None and (W0.shape != W1.shape or W0.dtype != W1.dtype or W0.stride(1) != 1 or W0.device != W1.device):
                raise ValueError(f"lowrank table: matrix {i}: W0 must match W1 in shape, dtype and device")
            nout, nin = W1.shape
            row = (int(off_a), int(off_b), int(k), int(nin), int(nout))
            keep.append((W1, W0))
            yield row, (_p(W1), _p(W0) if W0 is not None else None, W1.stride(0) if nout > 1 else max(W1.stride(0), nin),
                        (W0.stride(0) if nout > 1 else max(W0.stride(0), nin)) if W0 is not None else 0,
                        row[0], row[1], row[2], row[3], row[4], _LOWRANK_DTYPES[W1.dtype], index)
    b = _pair_table(_LOWRANK_TABLE, described(), device, n_elems)
    return LowrankLayout(b.table, b.rows, b.extent, b.host, int(lib.qfx_lowrank_sketch_workspace(b.host, len(b.rows))), keep)


def lowrank_sketch(table, pflat, normsq, info, skipped, ws, power_iters=2, seed=0, orth_tol=LOWRANK_ORTH_TOL,
                   max_sweeps=LORA_SVD_MAX_SWEEPS):
    """D = W1 - W0 ~ Q C of every matrix of `table` (a lowrank_table) by a randomized range finder with `power_iters` power
    iterations: Q [out, k] and C [k, in] into pflat at the table's offsets, normsq [n] fp64 = ||D||_F^2, info [n, 2] int32 (columns
    kept, converged), skipped [1] int32; ws: uint8, >= table.ws_bytes.  A fixed sequence of launches, nothing synchronises.  See qfx.h."""
    power_iters, max_sweeps, orth_tol, seed = int(power_iters), int(max_sweeps), float(orth_tol), int(seed)
    if not 0 <= power_iters <= LOWRANK_MAX_POWER_ITERS:
        raise ValueError(f"lowrank_sketch: power_iters must lie in 0..{LOWRANK_MAX_POWER_ITERS}, not {power_iters}")
    if not 0.0 <= orth_tol < 1.0:
        raise ValueError(f"lowrank_sketch: orth_tol must lie in [0, 1), not {orth_tol}")
    if not 1 <= max_sweeps <= 64:
        raise ValueError(f"lowrank_sketch: max_sweeps must lie in 1..64, not {max_sweeps}")
    dev, n = pflat.device, table.n_mats
    _svd_buf("lowrank_sketch", "pflat", pflat, torch.float32, table.extent, dev)
    _svd_buf("lowrank_sketch", "normsq", normsq, torch.float64, n, dev)
    _svd_buf("lowrank_sketch", "info", info, torch.int32, 2 * n, dev)
    _svd_buf("lowrank_sketch", "skipped", skipped, torch.int32, 1, dev)
    _svd_buf("lowrank_sketch", "ws", ws, torch.uint8, table.ws_bytes, dev)
    if table.table.device != dev or any(w1.device != dev for w1, _ in table.keep):
        raise ValueError("lowrank_sketch: the descriptor table or a matrix lives on another device")
    a = L.LowrankArgs(_p(table.table), C.cast(table.host, C.c_void_p), n, power_iters, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF,
                      orth_tol, max_sweeps, 0, _p(pflat), pflat.numel(), _p(normsq), _p(info), _p(skipped), _p(ws), ws.numel())
    L.check(lib.qfx_lowrank_sketch(a, stream_ptr()), "qfx_lowrank_sketch")


LORA_FOLD_MAX_RANK = 64


class LoraFoldLayout:
    """Descriptor table of qfx_lora_fold, built once per set of matrices.  rows[i] = (off_a, off_b, r, in_features, out_features,
    c); extent: elements the flat buffer of A / B needs; host: the ctypes array (read again at every launch); tile_start: the
    device words the launch writes; keep: the tensors the table points at."""

    def __init__(self, table, rows, extent, host, tile_start, keep):
        self.table, self.rows, self.extent, self.host, self.tile_start, self.keep = table, rows, extent, host, tile_start, keep
        self.n_mats = len(rows)


_LORA_FOLD_TABLE = _TableSpec("lora_fold", L.LoraFoldMat, LORA_FOLD_MAX_RANK,
                              refused="a dimension, a leading dimension, an offset, or two matrices that overlap",
                              over="matrix {i} has rank {r}: ranks above {cap} are not implemented", none="matrices")


def lora_fold_table(mats, device=None, n_elems=None):
    """mats: (W, off_a, off_b, r, c) per matrix -- W a 2-D device tensor [out, in] with unit column stride, bfloat16 or float32,
    folded in place; A [r, in] at off_a and B [out, r] at off_b of the flat fp32 buffer; c the coefficient of B A.  Checked by
    qfx_lora_fold_check_table against n_elems (default: the extent of the rows themselves) before it goes to the device."""
    keep = []

    def described():
        for i, (W, off_a, off_b, r, c) in enumerate(mats):
            if W is None or W.dim() != 2 or W.dtype not in _LOWRANK_DTYPES or W.stride(1) != 1:
                raise ValueError(f"lora_fold table: matrix {i}: W must be a 2-D bfloat16 or float32 tensor with unit column stride")
            nout, nin = W.shape
            row = (int(off_a), int(off_b), int(r), int(nin), int(nout), float(c))
            keep.append(W)
            yield row, (_p(W), W.stride(0) if nout > 1 else max(W.stride(0), nin), row[0], row[1], row[2], row[3], row[4],
                        _LOWRANK_DTYPES[W.dtype], row[5])
    b = _pair_table(_LORA_FOLD_TABLE, described(), device, n_elems)
    tile_start = torch.zeros(len(b.rows) + 1, dtype=torch.int64, device=device)
    return LoraFoldLayout(b.table, b.rows, b.extent, b.host, tile_start, keep)


def lora_fold(table, pflat):
    """W <- W + c B A for every matrix of `table` (a lora_fold_table), in place, with A and B read from pflat: fp64 dots in
    index order, one rounding to fp32 and for a bfloat16 W one more to bfloat16 -- the same bits at any address and in any table
    order.  One launch over (64 x 64 tile, matrix) behind a one-workgroup prefix launch; nothing synchronises.  See qfx.h."""
    dev = pflat.device
    _svd_buf("lora_fold", "pflat", pflat, torch.float32, table.extent, dev)
    if table.table.device != dev or table.tile_start.device != dev or any(w.device != dev for w in table.keep):
        raise ValueError("lora_fold: the descriptor table or a matrix lives on another device")
    a = L.LoraFoldArgs(_p(table.table), C.cast(table.host, C.c_void_p), table.n_mats, 0, _p(pflat), pflat.numel(), _p(table.tile_start))
    L.check(lib.qfx_lora_fold(a, stream_ptr()), "qfx_lora_fold")


SCALED_ADAMW_MAX_RANK = 64


_SCALED_ADAMW_TABLE = _TableSpec("scaled_adamw", L.ScaledAdamwPair, SCALED_ADAMW_MAX_RANK,
                                 refused="a dimension, an offset, an overlap, an lr ratio or a weight decay")


def scaled_adamw_table(pairs, device=None, n_elems=None):
    """pairs: (off_a, off_b, r, in_features, out_features, lr_ratio_a, lr_ratio_b, wd_a, wd_b) of every adapter pair in the flat
    buffers -- A [r, in] at off_a, B [out, r] at off_b, the tensors' learning rates over the step's lr and their weight decays.
    Checked by qfx_scaled_adamw_check_table against n_elems (default: the extent of the pairs themselves) before it goes to the
    device."""
    def rows():
        for off_a, off_b, r, nin, nout, ra, rb, wa, wb in pairs:
            row = (int(off_a), int(off_b), int(r), int(nin), int(nout), float(ra), float(rb), float(wa), float(wb))
            yield row, row + (0,)
    return _pair_layout(_SCALED_ADAMW_TABLE, rows(), device, n_elems)


def scaled_adamw_check(lr, betas, eps, reg=1e-6, precondition=True):
    """The constructor checks of the scaled AdamW family (torch.optim.AdamW's, with its messages, and reg > 0)."""
    if not 0.0 <= lr:
        raise ValueError(f"Invalid learning rate: {lr}")
    if not 0.0 <= eps:
        raise ValueError(f"Invalid epsilon value: {eps}")
    if len(betas) != 2:
        raise ValueError(f"scaled_adamw: betas is a pair, not {betas!r}")
    for i, b in enumerate(betas):
        if not 0.0 <= b < 1.0:
            raise ValueError(f"Invalid beta parameter at index {i}: {b}")
    if isinstance(reg, bool) or not isinstance(reg, (int, float)) or not (reg > 0 and math.isfinite(reg)):
        raise ValueError(f"scaled_adamw: reg must be a finite float > 0, not {reg!r}")
    if not isinstance(precondition, bool):
        raise ValueError(f"scaled_adamw: precondition must be a bool, not {precondition!r}")


def scaled_adamw_step(p, g, m, v, layout, skipped, lr, beta1, beta2, eps, step, reg=1e-6, precondition=True, gnorm_sq=None, max_norm=0.0,
                      grad_scale=1.0):
    """One Riemannian-preconditioned AdamW step (qfx.h: qfx_scaled_adamw_step, whose listing is the specification) over the flat
    fp32 buffers p / g with the moments m / v, one launch for every pair of `layout` (a scaled_adamw_table: the per-tensor lr
    ratios and weight decays are part of it).  skipped: int32 device tensor of one element, zeroed and written by the launch -- the
    number of pairs left untouched (a non-finite gradient, a failed factorisation).  Nothing synchronises."""
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        if t is None or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() < layout.extent or t.device != p.device:
            raise ValueError(f"scaled_adamw_step: {name} must be a contiguous float32 tensor on {p.device} with >= {layout.extent} elements")
    if skipped is None or skipped.dtype != torch.int32 or skipped.numel() < 1 or skipped.device != p.device:
        raise ValueError(f"scaled_adamw_step: skipped must be an int32 tensor on {p.device}")
    if layout.table.device != p.device:
        raise ValueError("scaled_adamw_step: the descriptor table lives on another device")
    scaled_adamw_check(lr, (beta1, beta2), eps, reg, bool(precondition))
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    a = L.ScaledAdamwArgs(_p(p), _p(g), _p(m), _p(v), _p(layout.table), layout.n_pairs, int(bool(precondition)), lr, beta1, beta2, eps,
                          reg, bc1, bc2, _p(gnorm_sq), max_norm, grad_scale, _p(skipped))
    L.check(lib.qfx_scaled_adamw_step(a, stream_ptr()), "qfx_scaled_adamw_step")


STATS_ROW_FIELDS = tuple(n for n, _ in L.StatsRow._fields_)
STATS_ROW_DTYPE = [(n, "<i4" if t is C.c_int32 else "<f4") for n, t in L.StatsRow._fields_]      # numpy view of the 32-byte rows


class StatsLayout:
    """Descriptor table of one flat-buffer layout for qfx_adapter_stats, built once per layout.  `entries[i]` = (off, numel) of
    table entry i, names[i] its name, kinds[i] "A" / "B" (lora_A / lora_B) or None; extent: elements p / g / prev need."""

    def __init__(self, table, entries, names, kinds, extent):
        self.table, self.entries, self.names, self.kinds, self.extent = table, entries, names, kinds, extent
        self.n_entries = len(entries)


def stats_table_entries(entries, device=None, names=None, kinds=None):
    """entries: (off, numel) of every tensor in the flat buffers, in any order.  An entry with numel <= 0 or a negative offset is
    kept (the kernel skips it and reports a row of zeros); it does not count towards the extent."""
    rows = [(int(off), int(k)) for off, k in entries]
    if not rows:
        raise ValueError("stats table: no tensors")
    for i, (off, k) in enumerate(rows):
        if k >= 1 << 31 or k < -(1 << 31):
            raise ValueError(f"stats table: entry {i} has {k} elements (an entry holds fewer than 2^31)")
    extent = max([off + k for off, k in rows if k > 0 and off >= 0], default=0)
    arr = (L.StatsEntry * len(rows))(*[L.StatsEntry(off, k, 0) for off, k in rows])
    table = torch.frombuffer(bytearray(arr), dtype=torch.uint8)
    if device is not None:
        table = table.to(device)
    names = [f"entry{i}" for i in range(len(rows))] if names is None else list(names)
    kinds = [None] * len(rows) if kinds is None else list(kinds)
    if len(names) != len(rows) or len(kinds) != len(rows):
        raise ValueError("stats table: one name and one kind per entry")
    return StatsLayout(table, rows, names, kinds, extent)


def stats_table(store, device=None):
    """The descriptor table of a LoraStore: one entry per adapter tensor of store.params(), in that order, at the offset and with
    the element count the store packed it with (the padding up to the next multiple of 64 belongs to no entry).  A tensor is named
    by the key save_lora_weights writes it under (the diffusers style: `transformer.<module>.lora.down.weight` / `.lora.up.weight`
    for the attention projections, `.lora_A.weight` / `.lora_B.weight` elsewhere); the tensor of an adapter that is not the
    module's active one -- save_lora_weights leaves it out -- keeps its parameter name."""
    from .lora_io import _DIFFUSERS_RENAMED
    from .modules import QfxLoraLinear
    if store.pflat is None:
        raise ValueError("stats table: the model has no adapters")
    where = {id(p): (off, k) for _, p, off, k in store.entries}
    keys = {}
    for name, m in store.model.named_modules():
        if isinstance(m, QfxLoraLinear):
            down, up = ("lora.down", "lora.up") if name.endswith(_DIFFUSERS_RENAMED) else ("lora_A", "lora_B")
            keys[id(m.A)] = f"transformer.{name}.{down}.weight"
            keys[id(m.B)] = f"transformer.{name}.{up}.weight"
    entries, names, kinds = [], [], []
    for n, p in store.params():
        if id(p) not in where:
            raise ValueError(f"stats table: adapter parameter {n!r} is not in the flat LoRA store")
        entries.append(where[id(p)])
        names.append(keys.get(id(p), n))
        kinds.append("A" if ".lora_A." in n else "B" if ".lora_B." in n else None)
    return stats_table_entries(entries, device=store.pflat.device if device is None else device, names=names, kinds=kinds)


def adapter_stats(p, g, prev, table, out, phase, gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
    """One launch of qfx_adapter_stats on the current stream (qfx.h).  phase 0, before the optimizer's launch: the squared norm,
    the largest magnitude and the non-finite count of the clipped gradient of every tensor of `table` (a stats_table) into the rows
    of `out` (uint8 [n_entries * 32]), and prev = p over the tensors.  phase 1, behind it: the squared weight norm, its non-finite
    count and the squared norm of p - prev.  g may be None in phase 1.  Nothing synchronises."""
    if phase not in (0, 1):
        raise ValueError(f"adapter_stats: phase is 0 or 1, not {phase!r}")
    need = [("p", p), ("prev", prev)] + ([("g", g)] if phase == 0 or g is not None else [])
    for name, t in need:
        if t is None or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() < table.extent or t.device != p.device:
            raise ValueError(f"adapter_stats: {name} must be a contiguous float32 tensor on {p.device} with >= {table.extent} elements")
    if out is None or out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < 32 * table.n_entries or out.device != p.device:
        raise ValueError(f"adapter_stats: out must be a contiguous uint8 tensor on {p.device} with >= {32 * table.n_entries} bytes")
    if table.table.device != p.device:
        raise ValueError("adapter_stats: the descriptor table lives on another device")
    if gnorm_sq is not None and (gnorm_sq.dtype != torch.float32 or gnorm_sq.device != p.device):
        raise ValueError(f"adapter_stats: gnorm_sq must be a float32 tensor on {p.device}")
    L.check(lib.qfx_adapter_stats(_p(p), _p(g), _p(prev), _p(table.table), table.n_entries, _p(out), phase, _p(gnorm_sq),
                                  float(max_norm), float(grad_scale), stream_ptr()), "qfx_adapter_stats")


def stats_rows(out, n_entries):
    """The rows of an `out` buffer as a numpy structured array (fields: STATS_ROW_FIELDS): the ONE device-to-host copy."""
    import numpy as np
    return np.frombuffer(out[:32 * n_entries].cpu().numpy().tobytes(), dtype=np.dtype(STATS_ROW_DTYPE))


LORA_DROPOUT_WORDS = 8      # seed_lo, seed_hi, step, active, thr_elem, thr_rank, scale (fp32 bits), sample0 (include/qfx.h)


def lora_dropout_threshold(p, what="dropout probability"):
    """floor(p * 2^32) for 0 <= p < 1: a 32-bit draw is kept iff it is >= the threshold."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{what} must satisfy 0 <= p < 1, not {p}")
    return int(math.floor(p * 4294967296.0))


def lora_dropout_state_words(seed=0, step=0, active=1, network_dropout=0.0, rank_dropout=0.0, sample0=0):
    """The 8 state words of qfx_lora_dropout_* as a list of Python ints (host side; see include/qfx.h)."""
    import struct
    te = lora_dropout_threshold(network_dropout, "network_dropout")
    tr = lora_dropout_threshold(rank_dropout, "rank_dropout")
    scale = 1.0 / ((1.0 - float(network_dropout)) * (1.0 - float(rank_dropout)))      # in double, rounded once to fp32
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"dropout seed must fit 64 bits, not {seed}")
    return [seed & 0xFFFFFFFF, seed >> 32, int(step) & 0xFFFFFFFF, int(bool(active)), te, tr,
            struct.unpack("<I", struct.pack("<f", scale))[0], int(sample0) & 0xFFFFFFFF]


def lora_dropout_args(*, Ut, M, R, rows_per_batch, sites, ext=None, ld_ext=0, group_R=None, group_stride=0):
    """One problem of qfx_lora_dropout_apply: the outputs of one rank-r producer call.  Ut = (hi, lo) tensors [R, >= M] (or a
    (hi pointer, lo pointer, row stride) triple), ext a tensor (row stride ld_ext, default its own) or a pointer, or None; sites: one
    32-bit key per group of group_R columns (up to 3)."""
    a = L.LoraDropoutArgs()
    if isinstance(ext, torch.Tensor):
        ld_ext = ld_ext or ext.stride(0)
        ext = ext.data_ptr()
    a.ext, a.ld_ext = ext, ld_ext
    if len(Ut) == 3:
        a.Ut_hi, a.Ut_lo, a.ld_ut = Ut
    else:
        a.Ut_hi, a.Ut_lo, a.ld_ut = Ut[0].data_ptr(), Ut[1].data_ptr(), Ut[0].stride(0)
    a.M, a.R, a.group_R, a.group_stride, a.rows_per_batch = M, R, (R if group_R is None else group_R), group_stride, rows_per_batch
    sites = list(sites)
    if not 1 <= len(sites) <= 3:
        raise ValueError("lora_dropout_args: one to three site keys")
    for i, s in enumerate(sites):
        a.site[i] = int(s) & 0xFFFFFFFF
    return a


def lora_dropout_apply(problems, state):
    """problems (lora_dropout_args, up to QFX_MAX_BATCH per launch) are multiplied in place by the factors that `state` (int32 [8]
    on the device) yields; nothing happens on the device while state.active == 0 or both probabilities are 0."""
    if state.dtype != torch.int32 or state.numel() < LORA_DROPOUT_WORDS or not state.is_contiguous():
        raise ValueError("lora_dropout_apply: state must be a contiguous int32 tensor of 8 words")
    problems = list(problems)
    for i in range(0, len(problems), L.MAX_BATCH):
        chunk = problems[i:i + L.MAX_BATCH]
        arr = (L.LoraDropoutArgs * len(chunk))(*chunk)
        L.check(lib.qfx_lora_dropout_apply(arr, len(chunk), _p(state), stream_ptr()), "qfx_lora_dropout_apply")


def lora_dropout_advance(state):
    """state.step += 1 on the device when state.active != 0 (what a forward program does first)."""
    L.check(lib.qfx_lora_dropout_advance(_p(state), stream_ptr()), "qfx_lora_dropout_advance")


def lora_dropout_factors_host(words, site, b, t, r):
    """The factors f[0..r) of token t of local sample b of adapter `site` under the 8 host words `words`: a float32 tensor [r],
    computed on the host by the inline function the kernel calls (no GPU)."""
    st = (C.c_uint32 * LORA_DROPOUT_WORDS)(*[int(w) & 0xFFFFFFFF for w in words])
    out = (C.c_float * int(r))() if r > 0 else (C.c_float * 1)()
    L.check(lib.qfx_lora_dropout_factors_host(st, int(site) & 0xFFFFFFFF, int(b), int(t), int(r), out), "qfx_lora_dropout_factors_host")
    return torch.tensor(list(out), dtype=torch.float32)


MUON_ADJUST_LR = (None, "original", "match_rms_adamw")
MUON_MAX_SHORT_SIDE = 96


class MuonLayout:
    """Descriptor table of one flat-buffer layout for qfx_muon_step, built once per layout.  `tensors[i]` = (off, rows, cols, lr
    ratio) of matrix i; extent: elements p / g / buf need; ws_bytes: what the bf16 workspace needs (0 when every X fits LDS)."""

    def __init__(self, table, tensors, extent, ws_bytes, adjust_lr_fn):
        self.table, self.tensors, self.extent, self.ws_bytes, self.adjust_lr_fn = table, tensors, extent, ws_bytes, adjust_lr_fn
        self.n_tensors = len(tensors)


def muon_lr_ratio(adjust_lr_fn, rows, cols):
    """torch.optim._muon._adjust_lr's factor on the learning rate of a [rows, cols] matrix."""
    if adjust_lr_fn not in MUON_ADJUST_LR:
        raise ValueError(f"Adjust learning rate function {adjust_lr_fn} is not supported")
    if adjust_lr_fn == "match_rms_adamw":
        return 0.2 * math.sqrt(max(rows, cols))
    return math.sqrt(max(1, rows / cols))


def muon_table(entries, adjust_lr_fn=None, device=None):
    """entries: (offset, shape) of every matrix in the flat buffers.  Muon is defined on 2-D parameters only (torch's refusal), and the
    kernel keeps the Gram matrix of the short side on chip: min(rows, cols) <= 96, which every adapter matrix satisfies."""
    rows_, tensors, extent = [], [], 0
    for i, (off, shape) in enumerate(entries):
        off, shape = int(off), tuple(int(d) for d in shape)
        if len(shape) != 2:
            raise ValueError(f"Muon only supports 2D parameters whereas we found a parameter with size: {shape}")
        r, c = shape
        if off < 0 or r <= 0 or c <= 0 or r * c > 1 << 30:
            raise ValueError(f"muon table: entry {i}: offset {off} / shape {shape}")
        if min(r, c) > MUON_MAX_SHORT_SIDE:
            raise ValueError(f"muon table: entry {i} has shape {shape}: the short side of a matrix is at most {MUON_MAX_SHORT_SIDE} "
                             "(an adapter's rank); larger Gram matrices are not implemented")
        ratio = muon_lr_ratio(adjust_lr_fn, r, c)
        tensors.append((off, r, c, ratio))
        rows_.append((off, r, c, ratio, 0))
        extent = max(extent, off + r * c)
    if not rows_:
        raise ValueError("muon table: no tensors")
    arr = (L.MuonTensor * len(rows_))(*[L.MuonTensor(*r) for r in rows_])
    ws_bytes = int(lib.qfx_muon_ws_bytes(arr, len(rows_)))
    if ws_bytes < 0:
        raise ValueError("muon table: refused by qfx_muon_ws_bytes")
    table = torch.frombuffer(bytearray(arr), dtype=torch.uint8)
    if device is not None:
        table = table.to(device)
    return MuonLayout(table, tensors, extent, ws_bytes, adjust_lr_fn)


def muon_step(p, g, buf, ws, layout, lr, weight_decay=0.1, momentum=0.95, nesterov=True, ns_coefficients=(3.4445, -4.7750, 2.0315),
              eps=1e-7, ns_steps=5, gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
    """One Muon step (torch.optim.Muon) over the flat fp32 buffers p / g with the momentum buffer buf; see qfx.h.  layout: a
    muon_table (the adjust_lr_fn is part of it); ws: bf16 (or int16) workspace of >= layout.ws_bytes bytes, None when that is 0."""
    for name, t in (("p", p), ("g", g), ("buf", buf)):
        if t is None or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() < layout.extent or t.device != p.device:
            raise ValueError(f"muon_step: {name} must be a contiguous float32 tensor on {p.device} with >= {layout.extent} elements")
    if layout.table.device != p.device:
        raise ValueError("muon_step: the descriptor table lives on another device")
    have = 0
    if ws is not None:
        if ws.element_size() != 2 or not ws.is_cuda or not ws.is_contiguous() or ws.device != p.device:
            raise ValueError(f"muon_step: ws must be a contiguous 2-byte tensor on {p.device}")
        have = ws.numel() * 2
    if have < layout.ws_bytes:
        raise ValueError(f"muon_step: the workspace holds {have} bytes, the layout needs {layout.ws_bytes}")
    if len(ns_coefficients) != 3:
        raise ValueError("Coefficients must be a tuple of exactly 3 values")
    ca, cb, cc = (float(x) for x in ns_coefficients)
    a = L.MuonArgs(_p(p), _p(g), _p(buf), _p(ws), have, _p(layout.table), layout.n_tensors, int(bool(nesterov)), int(ns_steps),
                   float(lr), float(weight_decay), float(momentum), 1.0 - float(momentum), ca, cb, cc, float(eps),
                   _p(gnorm_sq), max_norm, grad_scale)
    L.check(lib.qfx_muon_step(a, stream_ptr()), "qfx_muon_step")


class AdafactorLayout:
    """Descriptor table of one flat-buffer layout for qfx_adafactor_step, built once per layout.  `tensors[i]` = (off, rows, cols,
    factored, first element in row, in col, in v) of entry i (-1 where the entry has none); n_row / n_col / n_v: elements the row /
    col / v buffers need; extent: elements p / g / m need."""

    def __init__(self, table, tensors, n_row, n_col, n_v, extent):
        self.table, self.tensors, self.n_row, self.n_col, self.n_v, self.extent = table, tensors, n_row, n_col, n_v, extent
        self.n_tensors = len(tensors)


def adafactor_table(entries, device=None):
    """entries: (offset, shape) of every tensor in the flat buffers.  A 2-D tensor is factored (rows + cols statistics, packed in
    entry order), a 0-/1-D one keeps an elementwise second moment in v; exp_avg is indexed like the parameters."""
    rows_, tensors, n_row, n_col, n_v, extent = [], [], 0, 0, 0, 0
    for i, (off, shape) in enumerate(entries):
        off, shape = int(off), tuple(int(d) for d in shape)
        if len(shape) > 2:
            raise ValueError(f"adafactor table: entry {i} has {len(shape)} dimensions (adapter matrices are 2-D; more is not implemented)")
        numel = 1
        for d in shape:
            numel *= d
        if off < 0 or numel <= 0 or numel > 1 << 30:
            raise ValueError(f"adafactor table: entry {i}: offset {off} / shape {shape}")
        if len(shape) == 2:
            tensors.append((off, shape[0], shape[1], True, n_row, n_col, -1))
            rows_.append((off, n_row, n_col, 0, off, shape[0], shape[1], i, 1))
            n_row, n_col = n_row + shape[0], n_col + shape[1]
        else:
            tensors.append((off, 1, numel, False, -1, -1, n_v))
            rows_.append((off, 0, 0, n_v, off, 1, numel, i, 0))
            n_v += numel
        extent = max(extent, off + numel)
    if not rows_:
        raise ValueError("adafactor table: no tensors")
    arr = (L.AdafactorTensor * len(rows_))(*[L.AdafactorTensor(*r) for r in rows_])
    table = torch.frombuffer(bytearray(arr), dtype=torch.uint8)
    if device is not None:
        table = table.to(device)
    return AdafactorLayout(table, tensors, n_row, n_col, n_v, extent)


def adafactor_scalars(step, lr=None, decay_rate=-0.8, relative_step=True, warmup_init=False):
    """(lr or the relative step, beta2_t, 1 - beta2_t) of 1-based step `step`, formed in double (what the launch rounds to fp32)."""
    if relative_step:
        lr = min(1e-6 * step if warmup_init else 1e-2, 1.0 / math.sqrt(step))
    beta2t = 1.0 - math.pow(step, decay_rate)
    return float(lr), beta2t, 1.0 - beta2t


def adafactor_step(p, g, row, col, v, m, rms, layout, step, lr=None, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None,
                   weight_decay=0.0, scale_parameter=True, relative_step=True, warmup_init=False, gnorm_sq=None, max_norm=0.0,
                   grad_scale=1.0):
    """One Adafactor step (transformers.optimization.Adafactor) over the flat buffers p / g; see qfx.h.  row / col / v: fp32 with >=
    layout.n_row / n_col / n_v elements (one when unused); m: fp32 like p, None iff beta1 is None; rms: fp32[layout.n_tensors];
    step: 1-based count t.  lr: the external learning rate, None with relative_step."""
    if relative_step and lr is not None:
        raise ValueError("Cannot combine manual `lr` and `relative_step=True` options")
    if warmup_init and not relative_step:
        raise ValueError("`warmup_init=True` requires `relative_step=True`")
    if lr is None and not relative_step:
        raise ValueError("adafactor_step: relative_step=False needs a learning rate")
    if int(step) < 1:
        raise ValueError(f"adafactor_step: step {step} (counted from 1)")
    f32 = torch.float32
    for name, t, need in (("p", p, layout.extent), ("g", g, layout.extent), ("row", row, max(1, layout.n_row)),
                          ("col", col, max(1, layout.n_col)), ("v", v, max(1, layout.n_v)), ("rms", rms, layout.n_tensors)) + \
            ((("m", m, layout.extent),) if beta1 is not None else ()):
        if t is None or t.dtype != f32 or not t.is_cuda or not t.is_contiguous() or t.numel() < need or t.device != p.device:
            raise ValueError(f"adafactor_step: {name} must be a contiguous float32 tensor on {p.device} with >= {need} elements")
    if layout.table.device != p.device:
        raise ValueError("adafactor_step: the descriptor table lives on another device")
    lr_t, beta2t, omb2 = adafactor_scalars(int(step), lr, decay_rate, relative_step, warmup_init)
    b1 = 0.0 if beta1 is None else float(beta1)
    a = L.AdafactorArgs(_p(p), _p(g), _p(row), _p(col), _p(v), _p(m) if beta1 is not None else None, _p(rms), _p(layout.table),
                        layout.n_tensors, int(bool(scale_parameter)), int(beta1 is not None), lr_t, beta2t, omb2, float(eps[0]),
                        float(eps[1]), float(clip_threshold), b1, 1.0 - b1, float(weight_decay), _p(gnorm_sq), max_norm, grad_scale)
    L.check(lib.qfx_adafactor_step(a, stream_ptr()), "qfx_adafactor_step")


class CameLayout:
    """Descriptor table of one flat-buffer layout for qfx_came_step, built once per layout.  `tensors[i]` = (off, rows, cols,
    factored, first element in row / rrow, in col / rcol, in v) of entry i (-1 where the entry has none); n_row / n_col / n_v:
    elements the row and rrow / col and rcol / v buffers need; extent: elements p / g / m need."""

    def __init__(self, table, tensors, n_row, n_col, n_v, extent):
        self.table, self.tensors, self.n_row, self.n_col, self.n_v, self.extent = table, tensors, n_row, n_col, n_v, extent
        self.n_tensors = len(tensors)


def came_table(entries, device=None):
    """entries: (offset, shape) of every tensor in the flat buffers.  A 2-D tensor is factored (rows + cols statistics of the squared
    gradient and of the instability, packed in entry order), a 1-D one keeps an elementwise second moment in v; more dimensions are
    refused.  exp_avg is indexed like the parameters.  The bounds are adafactor_table's."""
    rows_, tensors, n_row, n_col, n_v, extent = [], [], 0, 0, 0, 0
    for i, (off, shape) in enumerate(entries):
        off, shape = int(off), tuple(int(d) for d in shape)
        if len(shape) not in (1, 2):
            raise ValueError(f"came table: entry {i} has {len(shape)} dimensions (adapter matrices are 2-D; only 1-D and 2-D are implemented)")
        numel = 1
        for d in shape:
            numel *= d
        if off < 0 or numel <= 0 or numel > 1 << 30:
            raise ValueError(f"came table: entry {i}: offset {off} / shape {shape}")
        if len(shape) == 2:
            tensors.append((off, shape[0], shape[1], True, n_row, n_col, -1))
            rows_.append((off, n_row, n_col, n_row, n_col, 0, shape[0], shape[1], i, 1))
            n_row, n_col = n_row + shape[0], n_col + shape[1]
        else:
            tensors.append((off, 1, numel, False, -1, -1, n_v))
            rows_.append((off, 0, 0, 0, 0, n_v, 1, numel, i, 0))
            n_v += numel
        extent = max(extent, off + numel)
    if not rows_:
        raise ValueError("came table: no tensors")
    arr = (L.CameTensor * len(rows_))(*[L.CameTensor(*r) for r in rows_])
    table = torch.frombuffer(bytearray(arr), dtype=torch.uint8)
    if device is not None:
        table = table.to(device)
    return CameLayout(table, tensors, n_row, n_col, n_v, extent)


def came_check(lr, betas, eps, clip_threshold, weight_decay=0.0):
    """What a CAME launch needs of its scalars: a betas triple and an eps pair, every beta in [0, 1] (came_pytorch.CAME's constructor
    check), a learning rate >= 0 (the package asks > 0 of its constructor; a schedule may pass through 0)."""
    if not isinstance(betas, (tuple, list)) or len(betas) != 3:
        raise ValueError(f"CAME's betas is a triple (beta1, beta2, beta3), not {betas!r}")
    if not isinstance(eps, (tuple, list)) or len(eps) != 2:
        raise ValueError(f"CAME's eps is a pair (eps1, eps2), not {eps!r}")
    if lr is None or not float(lr) >= 0.0:
        raise ValueError(f"CAME needs a learning rate >= 0, not {lr!r}")
    if not all(0.0 <= float(b) <= 1.0 for b in betas):
        raise ValueError(f"Invalid betas value: {tuple(betas)} (each in [0, 1])")
    if not float(clip_threshold) > 0 or float(eps[0]) < 0 or float(eps[1]) < 0 or float(weight_decay) < 0:
        raise ValueError(f"CAME: clip_threshold must be positive, eps and weight_decay non-negative ({clip_threshold}, {eps}, {weight_decay})")


def came_step(p, g, row, col, rrow, rcol, v, m, rms, layout, lr, betas=(0.9, 0.999, 0.9999), eps=(1e-30, 1e-16), clip_threshold=1.0,
              weight_decay=0.0, gnorm_sq=None, max_norm=0.0, grad_scale=1.0):
    """One CAME step (came_pytorch.CAME) over the flat buffers p / g; see qfx.h.  row, rrow / col, rcol / v: fp32 with >= layout.n_row
    / n_col / n_v elements (one when unused); m: fp32 like p; rms: fp32[layout.n_tensors]."""
    came_check(lr, betas, eps, clip_threshold, weight_decay)
    f32 = torch.float32
    for name, t, need in (("p", p, layout.extent), ("g", g, layout.extent), ("m", m, layout.extent), ("row", row, max(1, layout.n_row)),
                          ("col", col, max(1, layout.n_col)), ("rrow", rrow, max(1, layout.n_row)), ("rcol", rcol, max(1, layout.n_col)),
                          ("v", v, max(1, layout.n_v)), ("rms", rms, layout.n_tensors)):
        if t is None or t.dtype != f32 or not t.is_cuda or not t.is_contiguous() or t.numel() < need or t.device != p.device:
            raise ValueError(f"came_step: {name} must be a contiguous float32 tensor on {p.device} with >= {need} elements")
    if layout.table.device != p.device:
        raise ValueError("came_step: the descriptor table lives on another device")
    b1, b2, b3 = (float(b) for b in betas)
    a = L.CameArgs(_p(p), _p(g), _p(row), _p(col), _p(rrow), _p(rcol), _p(v), _p(m), _p(rms), _p(layout.table), layout.n_tensors,
                   float(lr), b1, 1.0 - b1, b2, 1.0 - b2, b3, 1.0 - b3, float(eps[0]), float(eps[1]), float(clip_threshold),
                   float(weight_decay), _p(gnorm_sq), max_norm, grad_scale)
    L.check(lib.qfx_came_step(a, stream_ptr()), "qfx_came_step")


# ---------------------------------------------------------------------------------------------- MX-FP8 (low-precision trunk)
def quant_mxfp8(x, M=None, rows_per_batch=None, x_map=(0, 0), out=None):
    """x [*, K] bf16 (row stride x.stride(0)) -> (q uint8 [M, K], s uint8 [K/128, M, 4] tile-major scales) in the OCP MX-FP8
    format (qfx.h)."""
    _bf(x, "x")
    M = x.shape[0] if M is None else M
    K = x.shape[1]
    q, s = out if out is not None else (torch.empty(M, K, dtype=torch.uint8, device=x.device),
                                        torch.empty(K // 128, M, 4, dtype=torch.uint8, device=x.device))
    a = L.QuantArgs()
    a.X, a.ldx, a.M, a.K = _p(x), x.stride(0), M, K
    a.Q, a.ldq, a.S, a.lds = _p(q), q.stride(0), _p(s), 0
    a.rows_per_batch = M if rows_per_batch is None else rows_per_batch
    a.x_batch_rows, a.x_row_off = x_map
    L.check(lib.qfx_quant_mxfp8(C.byref(a), stream_ptr()), "qfx_quant_mxfp8")
    return q, s


def mxfp8_scales_rowmajor(s):
    """tile-major scale bytes [K/128, M, 4] -> [M, K/32]."""
    return s.permute(1, 0, 2).reshape(s.shape[1], -1)


def mxfp8_dequant(q, s):
    """Host/torch view of an MX-FP8 operand as fp32 (test helper; not on the product path)."""
    v = q.view(torch.float8_e4m3fn).float().view(q.shape[0], -1, 32)
    sc = torch.pow(2.0, mxfp8_scales_rowmajor(s).float() - 127.0).unsqueeze(-1)
    return (v * sc).view(q.shape[0], -1)


def gemm_mxfp8(aq, asc, bq, bsc, *, bias=None, a2=None, b2=None, out=None, epi=L.EPI_NONE, out2=None, aux=None, gate=None,
               rows_per_batch=None, c_map=(0, 0), c_rows=None, row_mask=None):
    """C = dequant(aq, asc) @ dequant(bq, bsc).T (+ a2 @ b2.T in bf16) + bias -> epilogue (same contract as ops.gemm)."""
    M, K1 = aq.shape
    N = bq.shape[0]
    if out is None:
        out = torch.empty(M if c_rows is None else c_rows, N, dtype=BF, device=aq.device)
    f = L.GemmFp8Args()
    g = f.g
    g.A1, g.B1, g.lda1, g.ldb1, g.K1 = _p(aq), _p(bq), aq.stride(0), bq.stride(0), K1
    if a2 is not None:
        g.A2, g.B2, g.lda2, g.ldb2, g.K2 = _p(a2), _p(b2), a2.stride(0), b2.stride(0), b2.shape[1]
    g.M, g.N = M, N
    g.bias = _p(bias)
    g.C, g.ldc = _p(out), out.stride(0)
    if out2 is not None:
        g.C2, g.ldc2 = _p(out2), out2.stride(0)
    if aux is not None:
        g.aux, g.ldaux = _p(aux), aux.stride(0)
    if gate is not None:
        g.gate, g.gate_bstride = _p(gate), gate.stride(0)
    g.rows_per_batch = M if rows_per_batch is None else rows_per_batch
    g.c_batch_rows, g.c_row_off = c_map
    g.epi = epi
    g.row_mask = _p(row_mask)
    f.sa, f.ldsa, f.sb, f.ldsb = _p(asc), 0, _p(bsc), 0
    L.check(lib.qfx_gemm_mxfp8(C.byref(f), stream_ptr()), "qfx_gemm_mxfp8")
    return out
