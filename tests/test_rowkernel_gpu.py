"""GPU parity tests of the row kernels (csrc/qfx_elem.hip) and of the conditioning-head kernels (csrc/qfx_cond.hip) at every
dispatch path, through the C ABI, against the fp64 restatements of tests/rowkernel_ref.py.

Acceptance.  exact_case data: the outputs rowkernel_ref.exact_outputs names must equal the fp64 value BIT FOR BIT.  Everything else:
the worst error in bf16 ulps of the reference's `scale` tensor must stay within rowkernel_ref.BARS, which are twice the reference's
own fp32 reordering noise (tests/test_rowkernel_ref_cpu.py), never what the kernels give.  Every output buffer has at least 3
extra rows and its columns padded to the next multiple of 512 plus 8, starts as a canary (bf16 0x7FC1, fp32 NaN; buffers the kernel
adds into: a finite fill where it adds, the canary elsewhere) and is compared WHOLE.  Worst errors: rowkernel_parity.json.

Which case family selects which instantiation or branch:
  ln_mod_fwd_kernel (one instantiation, MAXP = 8 passes, `col < D` guard in every pass)
      LN_FWD_CASES      D = 8 (one lane), 264 / 520 / 3080 (guard cuts inside pass 1 / 2 / 7), 512 / 1536 / 3072 / 3584 / 4096 (whole passes);
                        rows 1, 4, 5, 7 with rpb = 3 (samples change inside a block, idle waves); mod_bstride 0, D, 6 D
      LN_FWD_BATCHES    n = 2, 3, 4 (the pi walk of the batched entry), mixed D, ragged last problem; bit-identical to n = 1 launches
      refusals          n = 5, ragged non-last problem, D % 8, D > 4096, mod_bstride % 8
  ln_mod_bwd_kernel<6> D = 8, 520, 3072;  <8> D = 3080, 3584, 4096   (LN_BWD_CASES: dres / dyg present and NULL, gate_bstride 0 / 6 D,
                        row_mask rows at the first and last row of a block);  LN_BWD_BATCH 3072 + 3584: all in <8>, singles in <6> and <8>
  mod_grad_kernel<1> 512, <2> 520, <3> 1032, <4> 2048, <6> 2056 (5 -> 6) and 3072, <8> 3080 (7 -> 8) and 4096; NS = 2 (two-round LDS
                        combine) is <8>; rpb 1, 8, 9, 17 (one wave, one block, two blocks, three blocks per sample); B 1, 3; short last
                        sample; gate on / off; row_mask; ld_* > D, out_bstride 3 D + 8;  MG_BATCHES n = 4 / 2 with different B
  rmsnorm_fwd_kernel    D = 8, 520, 3584, 4096, rows 1, 5
  mod_gemv_kernel       GEMV_CASES: B 1, 3, 8; K 8 (one lane), 256, 520 (second trip of the k loop, partly), 4096; N 1, 15, 17, 130 (clamped
                        n = N - 1 row loads, idle waves), 16; nmat 1, 3; SiLU on / off; bias NULL; 64 KiB of LDS at B = 8, K = 4096;
                        qfx_mod_gemv_unless with *skip = 0 and 1; B = 8, K = 4104: QFX_EUNSUPPORTED
  mod_gemv_t_kernel<2,2> / <1,2> K 8, 520, 1024;  <2,4> / <1,4> K 1536, 2048;  <2,6> / <1,6> K 3072;  B 1 (<1,*>), 2 (<2,*>), 3 (both),
                        8 (four passes of the b0 loop); N 1, 3, 5 (clamped rows), 4, 130; K = 3080: QFX_EINVAL
  qk_norm_rope_kernel<64 | 128, fwd | bwd>   QK_CASES: rope_bstride = S dh and 0, flags & 1, T = 0 and T = S and between,
                        saved NULL, B S 2 H not a multiple of the items per block (the clamped tail items)
  transpose_heads_kernel S_pad one tile beyond S, ld_in > 3 H dh;   mse_kernel (C = 4; C = 8 at a 2-byte offset), mse_kernel8 (C = 8, 16),
                        dpred NULL, S_t < S_all;  mse_tw_kernel;  flowmatch_prepare mode 1 (S_c = 0 and > 0) and mode 0;  add3 with c NULL;
                        timestep_embed with pre_scale != 1
  cond_u / cond_add / cond_bwd_b / cond_bwd_a   COND_CASES: B 1, 3, 8; r 1, 16, 64; K 8, 300 (second block partly), 3072; N 1, 255, 256,
                        257 (one column into the second block), 1000; na 1, 3; SiLU on / off; ldy, ldg > N; dx NULL / present;
                        cast_bf16_kernel / silu_bwd_kernel: n just past 2048 * 256 / 1024 * 256 (the grid-stride second trip)"""
import ctypes as C
import functools

import pytest
import torch

import rowkernel_ref as R
from parity_util import _observe

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DEV = "cuda:0"
EINVAL, EUNSUPPORTED = -1, -2
_STATS = {}


def _L():
    from qflux_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def record_worst(key, case, err, tol):
    old = _STATS.get(key)
    if old is None or err >= old["ulps"]:
        _STATS[key] = dict(ulps=err, bar=tol, case=str(case))
        _observe(None, None, dump=("rowkernel_parity.json", _STATS))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(R.bits(a), R.bits(b))


def is_canary(t):
    return bool((R.bits(t.cpu()) == (R.CANARY_BF16 if t.dtype == BF else R.CANARY_F32)).all())


def padded(rows, D):
    """Elements of an output buffer for a [rows, D] result: 3 more rows, columns padded to the next multiple of 512 plus 8."""
    return (rows + 3) * (R.roundup(D, 512) + 8)


def dev(t, pad=4104):
    """A device copy of `t` with `pad` zero elements behind it (a kernel that lost a mask reads zeros, not another allocation)."""
    buf = torch.zeros(t.numel() + pad, dtype=t.dtype, device=DEV)
    buf[:t.numel()] = t.contiguous().flatten().to(DEV)
    return buf[:t.numel()].view(t.shape)


def ptr(t):
    return t.data_ptr() if t is not None else None


def ptr_array(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=DEV)


def out_bf16(rows, D):
    return R.canary_bf16(padded(rows, D), device=DEV)


def out_f32(rows, D, filled=0, fill=None):
    buf = R.canary_f32(padded(rows, D), device=DEV)
    if fill is not None:
        buf[:filled] = fill
    return buf


@functools.lru_cache(maxsize=4)
def _case(family, case, kind):
    """(inputs, fp64 reference) of one case: computed once, shared by the tests that need it, never modified."""
    _, _, _, make, ref = R.FAMILIES[family]
    inp = make(case, kind)
    return inp, ref(inp, case)


def check(family, key, got, ref, case, kind, add=0.0):
    """got: the problem's part of an output buffer (CPU, reference shape).  Bit-equal where the case is exact, else within BARS."""
    val, scale = ref
    val = val + add
    if add:            # the initial fill the kernel adds onto is on the element's path too
        scale = torch.clamp(scale, min=abs(add))
    assert got.shape == val.shape, (got.shape, val.shape)
    if key in R.exact_outputs(family, case, kind):
        assert same_bits(got, val.to(got.dtype)), f"{family}.{key} {kind} {case}: not bit-equal, max |d| = {(got.double() - val).abs().max().item()}"
        return
    name = f"{R.FAMILIES[family][0]}.{key}"
    e = R.err_ulps(got, val, scale)
    record_worst(name, (kind, case), e, R.BARS[name])
    assert e <= R.BARS[name], f"{name} {kind} {case}: {e:.3f} ulps of scale > {R.BARS[name]}"


def check_flat(family, key, buf, ref, case, kind, add=0.0):
    """A flat canaried buffer whose first elements are the (row-major) result: values and store bounds in one pass."""
    got = buf.cpu()
    n = ref[0].numel()
    assert is_canary(got[n:]), f"{family}.{key} {kind} {case}: written outside the result"
    check(family, key, got[:n].view(ref[0].shape), ref, case, kind, add)


def mod_ptr(mod_d, D, stride, which):
    """(pointer, mod_bstride, keep-alive) of modulation vector `which` of the device table [B, 6 D] for the three stride kinds."""
    if stride == "tight":
        t = mod_d[:, which * D:(which + 1) * D].contiguous()
        return t.data_ptr(), D, t
    return mod_d.data_ptr() + 2 * which * D, (0 if stride == "shared" else 6 * D), mod_d


# ================================================================================================ LayerNorm + modulate, forward
def ln_fwd_args(inp, case, y):
    D, rows, stride = case
    a = _L().LnFwdArgs()
    keep = [dev(inp["x"]), dev(inp["mod"])]
    sh, bs, k1 = mod_ptr(keep[1], D, stride, 0)
    sc, _, k2 = mod_ptr(keep[1], D, stride, 1)
    a.x, a.shift, a.scale, a.mod_bstride, a.y = keep[0].data_ptr(), sh, sc, bs, y.data_ptr()
    a.rows, a.D, a.rows_per_batch, a.eps = rows, D, R.RPB, R.EPS
    return a, keep + [k1, k2]


@pytest.mark.parametrize("case", R.LN_FWD_CASES, ids=str)
def test_ln_fwd_every_width_rows_and_stride(case):
    D, rows, stride = case
    inp, ref = _case("ln_fwd", case, "rand")
    y = out_bf16(rows, D)
    a, keep = ln_fwd_args(inp, case, y)
    rc = _L().lib.qfx_ln_modulate_fwd(a.x, a.shift, a.scale, a.mod_bstride, a.y, rows, D, R.RPB, R.EPS, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    check_flat("ln_fwd", "y", y, ref["y"], case, "rand")


@pytest.mark.parametrize("probs", R.LN_FWD_BATCHES, ids=lambda p: f"n{len(p)}")
def test_ln_fwd_batch_is_bit_identical_to_single_launches(probs):
    L = _L()
    cases = [(D, rows, "six") for D, rows in probs]
    ys_b = [out_bf16(rows, D) for D, rows in probs]
    ys_s = [out_bf16(rows, D) for D, rows in probs]
    built = [ln_fwd_args(_case("ln_fwd", c, "rand")[0], c, y) for c, y in zip(cases, ys_b)]
    arr = (L.LnFwdArgs * len(probs))(*[b[0] for b in built])
    assert L.lib.qfx_ln_modulate_fwd_batch(arr, len(probs), _stream()) == 0
    for c, y in zip(cases, ys_s):
        a, keep = ln_fwd_args(_case("ln_fwd", c, "rand")[0], c, y)
        assert L.lib.qfx_ln_modulate_fwd_batch(C.byref(a), 1, _stream()) == 0
        torch.cuda.synchronize()
    torch.cuda.synchronize()
    for c, yb, ys in zip(cases, ys_b, ys_s):
        assert same_bits(yb.cpu(), ys.cpu()), f"batch differs from the single launch at {c}"
        check_flat("ln_fwd", "y", yb, _case("ln_fwd", c, "rand")[1]["y"], c, "rand")


def test_ln_fwd_batch_refusals_leave_the_output_alone():
    L = _L()
    y = out_bf16(8, 4096)

    def prob(D, rows, bstride=None, alloc_D=None):
        inp = dict(x=torch.zeros(rows, alloc_D or D, dtype=BF), mod=torch.zeros(3, 6 * (alloc_D or D), dtype=BF))
        a, keep = ln_fwd_args(inp, (alloc_D or D, rows, "six"), y)
        a.D = D
        if bstride is not None:
            a.mod_bstride = bstride
        return a, keep
    good = prob(512, 4)
    lists = {"n = 5": [good[0]] * 5, "ragged non-last": [prob(512, 5)[0], good[0]], "D % 8": [prob(516, 4, alloc_D=520)[0]],
             "D > 4096": [prob(4104, 4, alloc_D=4096)[0]], "mod stride % 8": [prob(512, 4, bstride=6 * 512 + 4)[0]]}
    for what, lst in lists.items():
        arr = (L.LnFwdArgs * len(lst))(*lst)
        assert L.lib.qfx_ln_modulate_fwd_batch(arr, len(lst), _stream()) == EINVAL, what
    torch.cuda.synchronize()
    assert is_canary(y)


# ================================================================================================ LayerNorm + modulate, backward
def ln_bwd_args(inp, case, dx, dyg):
    D, rows, dres, want_dyg, gstride, masked = case
    a = _L().LnBwdArgs()
    keep = [dev(inp["dy"]), dev(inp["x"]), dev(inp["mod"]), dev(inp["dres"]), dev(inp["mask"])]
    a.dy, a.x = keep[0].data_ptr(), keep[1].data_ptr()
    a.scale, a.mod_bstride, _ = mod_ptr(keep[2], D, "six", 1)
    a.dres = keep[3].data_ptr() if dres else None
    a.dx = dx.data_ptr()
    if want_dyg:
        a.gate, a.gate_bstride, _ = mod_ptr(keep[2], D, gstride, 2)
        a.dyg = dyg.data_ptr()
    a.row_mask = keep[4].data_ptr() if masked else None
    a.rows, a.D, a.rows_per_batch, a.eps = rows, D, R.RPB, R.EPS
    return a, keep


def ln_bwd_verify(case, dx, dyg):
    D, rows, dres, want_dyg, gstride, masked = case
    inp, ref = _case("ln_bwd", case, "rand")
    check_flat("ln_bwd", "dx", dx, ref["dx"], case, "rand")
    outs = [dx]
    if want_dyg:
        check_flat("ln_bwd", "dyg", dyg, ref["dyg"], case, "rand")
        outs.append(dyg)
    else:
        assert is_canary(dyg)
    for r in masked:
        if r < rows:
            for o in outs:      # exact (positive) zeros, not merely small values
                assert not R.bits(o.cpu()[r * D:(r + 1) * D]).any(), f"masked row {r} of {case} is not all zero bits"


@pytest.mark.parametrize("case", R.LN_BWD_CASES, ids=str)
def test_ln_bwd_both_instantiations_and_options(case):
    D, rows = case[:2]
    dx, dyg = out_bf16(rows, D), out_bf16(rows, D)
    a, keep = ln_bwd_args(_case("ln_bwd", case, "rand")[0], case, dx, dyg)
    rc = _L().lib.qfx_ln_modulate_bwd(a.dy, a.x, a.scale, a.mod_bstride, a.dres, a.gate, a.gate_bstride, a.dx, a.dyg, rows, D, R.RPB, R.EPS,
                                      a.row_mask, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    ln_bwd_verify(case, dx, dyg)


def test_ln_bwd_batch_in_the_wide_kernel_matches_the_singles():
    L = _L()
    cases = [(D, rows, True, True, "six", (0, 3)) for D, rows in R.LN_BWD_BATCH]
    outs_b = [(out_bf16(r, D), out_bf16(r, D)) for D, r in R.LN_BWD_BATCH]
    outs_s = [(out_bf16(r, D), out_bf16(r, D)) for D, r in R.LN_BWD_BATCH]
    built = [ln_bwd_args(_case("ln_bwd", c, "rand")[0], c, *o) for c, o in zip(cases, outs_b)]
    arr = (L.LnBwdArgs * len(cases))(*[b[0] for b in built])
    assert L.lib.qfx_ln_modulate_bwd_batch(arr, len(cases), _stream()) == 0
    torch.cuda.synchronize()
    for c, o in zip(cases, outs_s):
        a, keep = ln_bwd_args(_case("ln_bwd", c, "rand")[0], c, *o)
        assert L.lib.qfx_ln_modulate_bwd_batch(C.byref(a), 1, _stream()) == 0
        torch.cuda.synchronize()
    for c, ob, os_ in zip(cases, outs_b, outs_s):
        assert same_bits(ob[0].cpu(), os_[0].cpu()) and same_bits(ob[1].cpu(), os_[1].cpu()), f"batch differs from the single launch at {c}"
        ln_bwd_verify(c, *ob)


# ================================================================================================ mod_grad
class ModGrad:
    def __init__(self, case, kind):
        D, rpb, B, short, gate, mask, wide = case
        assert rpb <= R.EXACT_MAX_ROWS
        self.case, self.kind, self.gate = case, kind, gate
        self.inp, self.ref = _case("mod_grad", case, kind)
        self.rows, self.ld = R.mg_rows(case), R.mg_lds(case)
        obs = self.ld[4]
        self.keep = {k: dev(self.inp[k]) for k in ("dy", "x", "dxo", "y", "mask")}
        self.outs = {}
        for k in ("dshift", "dscale", "dgate"):
            buf = R.canary_f32(padded(B, obs), device=DEV)
            buf[:B * obs].view(B, obs)[:, :D] = R.FILL[k]
            self.outs[k] = buf

    def args(self):
        D, rpb, B, short, gate, mask, wide = self.case
        a = _L().ModGradArgs()
        k = self.keep
        a.dy, a.ld_dy, a.x, a.ld_x = k["dy"].data_ptr(), self.ld[0], k["x"].data_ptr(), self.ld[1]
        if gate:
            a.dxo, a.ld_dxo, a.y, a.ld_y, a.dgate = k["dxo"].data_ptr(), self.ld[2], k["y"].data_ptr(), self.ld[3], self.outs["dgate"].data_ptr()
        a.dshift, a.dscale, a.out_bstride = self.outs["dshift"].data_ptr(), self.outs["dscale"].data_ptr(), self.ld[4]
        a.row_mask = k["mask"].data_ptr() if mask else None
        a.rows, a.D, a.rows_per_batch, a.eps = self.rows, D, rpb, R.EPS
        return a

    def result(self, k):
        """The [B, D] sums of output k after asserting that nothing else in its buffer changed."""
        D, B, obs = self.case[0], self.case[2], self.ld[4]
        got = self.outs[k].cpu()
        body = got[:B * obs].view(B, obs)
        assert is_canary(got[B * obs:]) and is_canary(body[:, D:]), f"mod_grad.{k} {self.kind} {self.case}: written outside [B, D]"
        return body[:, :D].contiguous()

    def verify(self):
        for k in ("dshift", "dscale") + (("dgate",) if self.gate else ()):
            check("mod_grad", k, self.result(k), self.ref[k], self.case, self.kind, add=R.FILL[k])
        if not self.gate:
            assert same_bits(self.result("dgate"), torch.full((self.case[2], self.case[0]), R.FILL["dgate"]))


@pytest.mark.parametrize("case", R.MG_CASES, ids=str)
def test_mod_grad_every_switch_arm(case):
    for kind in ("exact", "rand"):
        p = ModGrad(case, kind)
        assert _L().lib.qfx_mod_grad(C.byref(p.args()), _stream()) == 0
        torch.cuda.synchronize()
        p.verify()


@pytest.mark.parametrize("D,probs", R.MG_BATCHES, ids=str)
def test_mod_grad_batch_with_different_sample_counts(D, probs):
    L = _L()
    for kind in ("exact", "rand"):
        cases = [(D, rpb, B, False, True, False, False) for rpb, B in probs]
        batch, single = [ModGrad(c, kind) for c in cases], [ModGrad(c, kind) for c in cases]
        arr = (L.ModGradArgs * len(cases))(*[p.args() for p in batch])
        assert L.lib.qfx_mod_grad_batch(arr, len(cases), _stream()) == 0
        for p in single:
            assert L.lib.qfx_mod_grad(C.byref(p.args()), _stream()) == 0
        torch.cuda.synchronize()
        for pb, ps in zip(batch, single):
            pb.verify()
            for k in ("dshift", "dscale", "dgate"):
                b, s = pb.result(k).double(), ps.result(k).double()
                assert (b - s).abs().max() <= 1e-5 * s.abs().max(), (k, pb.case)


# ================================================================================================ RMSNorm
@pytest.mark.parametrize("case", R.RMS_CASES, ids=str)
def test_rmsnorm_widths_and_rows(case):
    D, rows = case
    inp, ref = _case("rmsnorm", case, "rand")
    x, w, y = dev(inp["x"]), dev(inp["w"]), out_bf16(rows, D)
    assert _L().lib.qfx_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), rows, D, R.EPS, _stream()) == 0
    torch.cuda.synchronize()
    check_flat("rmsnorm", "y", y, ref["y"], case, "rand")


# ================================================================================================ modulation GEMV
def gemv_launch(inp, case, out, skip=None, unless=False):
    B, K, N, nmat, apply_silu, bias = case
    keep = [dev(inp["temb"]), [dev(w) for w in inp["Ws"]], [dev(b) for b in inp["bias"]] if bias else None]
    Wp = ptr_array(keep[1])
    bp = ptr_array(keep[2]) if bias else None
    L = _L()
    if unless:
        rc = L.lib.qfx_mod_gemv_unless(keep[0].data_ptr(), B, K, Wp.data_ptr(), ptr(bp), nmat, N, int(apply_silu), out.data_ptr(), ptr(skip), _stream())
    else:
        rc = L.lib.qfx_mod_gemv(keep[0].data_ptr(), B, K, Wp.data_ptr(), ptr(bp), nmat, N, int(apply_silu), out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("case", R.GEMV_CASES, ids=str)
def test_mod_gemv_shapes_and_options(case):
    B, K, N, nmat, apply_silu, bias = case
    assert K <= R.EXACT_MAX_GEMV_K
    for kind in ("exact", "rand"):
        inp, ref = _case("mod_gemv", case, kind)
        out = out_bf16(nmat * B, N)
        assert gemv_launch(inp, case, out) == 0
        check_flat("mod_gemv", "out", out, ref["out"], case, kind)


def test_mod_gemv_unless_skips_or_is_the_same_kernel():
    case = R.GEMV_CASES[7]
    B, K, N, nmat = case[:4]
    inp, ref = _case("mod_gemv", case, "rand")
    plain, zero, one = out_bf16(nmat * B, N), out_bf16(nmat * B, N), out_bf16(nmat * B, N)
    flag = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    assert gemv_launch(inp, case, plain) == 0
    assert gemv_launch(inp, case, zero, skip=flag[0:], unless=True) == 0
    assert gemv_launch(inp, case, one, skip=flag[1:], unless=True) == 0
    assert gemv_launch(inp, case, zero.clone(), skip=None, unless=True) == 0
    assert same_bits(plain.cpu(), zero.cpu())
    check_flat("mod_gemv", "out", zero, ref["out"], case, "rand")
    assert is_canary(one), "*skip = 1 must write nothing"


def test_mod_gemv_lds_limit():
    case = (8, 4104, 4, 1, False, False)
    inp = R.gemv_make(case, "exact")
    out = out_bf16(8, 4)
    assert gemv_launch(inp, case, out) == EUNSUPPORTED
    assert gemv_launch(inp, case, out, unless=True) == EUNSUPPORTED
    assert is_canary(out)


# ================================================================================================ transposed modulation GEMV
@pytest.mark.parametrize("case", R.GEMVT_CASES, ids=str)
def test_mod_gemv_t_every_instantiation(case):
    B, K, N, nmat = case
    assert nmat * N <= R.EXACT_MAX_GEMV_T
    for kind in ("exact", "rand"):
        inp, ref = _case("mod_gemv_t", case, kind)
        dy, Ws = dev(inp["dy"]), [dev(w) for w in inp["Ws"]]
        Wp = ptr_array(Ws)
        out = out_f32(B, K, B * K, R.FILL["gemv_t"])
        assert _L().lib.qfx_mod_gemv_t(dy.data_ptr(), B, N, K, Wp.data_ptr(), nmat, out.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        check_flat("mod_gemv_t", "out", out, ref["out"], case, kind)


def test_mod_gemv_t_refuses_wide_k():
    case = (2, 3080, 4, 1)
    inp = R.gemvt_make(case, "exact")
    dy, Ws = dev(inp["dy"]), [dev(w) for w in inp["Ws"]]
    out = out_f32(2, 3080)
    assert _L().lib.qfx_mod_gemv_t(dy.data_ptr(), 2, 4, 3080, ptr_array(Ws).data_ptr(), 1, out.data_ptr(), _stream()) == EINVAL
    torch.cuda.synchronize()
    assert is_canary(out)


# ================================================================================================ QK RMSNorm + RoPE
def qk_buffers(t, tail):
    """A device buffer holding `t` followed by `tail` canary elements."""
    buf = R.canary_bf16(t.numel() + tail, device=DEV)
    buf[:t.numel()] = t.flatten().to(DEV)
    return buf


def qk_launch(fn, buf, saved, inp, case):
    dh, B, S, T, H, flags, per_sample, _ = case
    rope, ws = dev(inp["rope"]), [dev(w) for w in inp["ws"]]
    rc = fn(buf.data_ptr(), ptr(saved), rope.data_ptr(), *[w.data_ptr() for w in ws], B, S, T, H, dh, R.EPS, flags, S * dh if per_sample else 0, _stream())
    torch.cuda.synchronize()
    return rc


def qk_verify(family, buf, orig, ref, case):
    """q | k sections against the reference, the v section and everything behind the tensor bit-identical to before."""
    dh, B, S, T, H = case[:5]
    Dm = H * dh
    got = buf.cpu()
    n = orig.numel()
    assert is_canary(got[n:]), f"{family} {case}: written past the tensor"
    g = got[:n].view(B, S, 3 * Dm)
    assert same_bits(g[..., 2 * Dm:].contiguous(), orig[..., 2 * Dm:].contiguous()), f"{family} {case}: v section touched"
    check(family, "out", g[..., :2 * Dm].reshape(B, S, 2, H, dh), ref["out"], case, "rand")


@pytest.mark.parametrize("case", R.QK_CASES, ids=str)
def test_qk_norm_rope_fwd_and_bwd(case):
    dh, B, S, T, H, flags, per_sample, want_saved = case
    L = _L()
    Dm = H * dh
    assert (B * S * 2 * H) % (256 // (dh // 8)) != 0      # the last block ends in clamped, store-less items
    inp, ref = _case("qk_fwd", case, "rand")
    tail = 3 * 3 * Dm + 8
    buf = qk_buffers(inp["qkv"], tail)
    saved = R.canary_bf16(B * S * 2 * Dm + tail, device=DEV)
    assert qk_launch(L.lib.qfx_qk_norm_rope_fwd, buf, saved if want_saved else None, inp, case) == 0
    qk_verify("qk_fwd", buf, inp["qkv"], ref, case)
    if want_saved:
        want = torch.cat([inp["qkv"][..., :2 * Dm].reshape(-1), R.canary_bf16(tail)])
        assert same_bits(saved.cpu(), want), f"{case}: saved is not the pre-norm q | k (or written past its end)"
    else:
        assert is_canary(saved)
    if per_sample and B > 1:
        # what a kernel that ignored rope_bstride would write for sample 1 is far outside the bar: the case tells the two apart
        shared = R.qk_fwd(inp["qkv"][1:2], inp["rope"][0:1], inp["ws"], T, H, dh, flags)["out"][0]
        assert R.err_ulps(shared, ref["out"][0][1:2], ref["out"][1][1:2]) > 8 * R.BARS["qk_fwd.out"]
    refb = _case("qk_bwd", case, "rand")[1]
    dbuf = qk_buffers(inp["dqkv"], tail)
    pre = dev(inp["qkv"][..., :2 * Dm].contiguous())
    assert qk_launch(L.lib.qfx_qk_norm_rope_bwd, dbuf, pre, inp, case) == 0
    qk_verify("qk_bwd", dbuf, inp["dqkv"], refb, case)
    assert same_bits(pre.cpu(), inp["qkv"][..., :2 * Dm].contiguous())


# ================================================================================================ small kernels
def test_transpose_heads_pad_tile_and_wide_rows():
    B, S, S_pad, H, dh = 2, 70, 192, 1, 64       # S_pad: the tile after the one S ends in is all padding
    HD, ld = H * dh, 3 * H * dh + 8
    x = R.rand_case(11, x=(B, S, ld))["x"]
    xd = dev(x)
    out = R.canary_bf16(B * HD + 3, S_pad, device=DEV)
    assert _L().lib.qfx_transpose_heads(xd.data_ptr() + 2 * HD, ld, out.data_ptr(), B, S, S_pad, H, dh, _stream()) == 0
    torch.cuda.synchronize()
    assert same_bits(out.cpu(), R.transpose_heads_image(x[:, :, HD:], S, S_pad, HD))


def _mse_run(case, tw, dpred_on):
    B, S_all, S_t, Cc, off = case
    fam = "mse_tw" if tw else "mse"
    inp, ref = _case(fam, case, "rand")
    pred = dev(inp["pred"])
    tbuf = torch.zeros(inp["target"].numel() + 16, dtype=BF, device=DEV)
    tbuf[off:off + inp["target"].numel()] = inp["target"].flatten().to(DEV)
    loss = R.canary_f32(4, device=DEV)
    loss[0] = 0.0
    dpred = out_bf16(B * S_all, Cc)
    L = _L()
    if tw:
        twd = dev(inp["tw"])
        rc = L.lib.qfx_mse_token_weighted_fwd_bwd(pred.data_ptr(), tbuf.data_ptr() + 2 * off, twd.data_ptr(), loss.data_ptr(), ptr(dpred if dpred_on else None),
                                                  B, S_all, S_t, Cc, R.MSE_INV_DENOM, R.MSE_GSCALE, _stream())
    else:
        rc = L.lib.qfx_mse_loss_fwd_bwd(pred.data_ptr(), tbuf.data_ptr() + 2 * off, loss.data_ptr(), ptr(dpred if dpred_on else None), B, S_all, S_t, Cc,
                                        R.MSE_GSCALE, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    lc = loss.cpu()
    assert is_canary(lc[1:])
    check(fam, "loss", lc[0], ref["loss"], case, "rand")
    if dpred_on:
        check_flat(fam, "dpred", dpred, ref["dpred"], case, "rand")
        g = dpred.cpu()[:B * S_all * Cc].view(B, S_all, Cc)
        assert not R.bits(g[:, S_t:].contiguous()).any(), "rows beyond S_t must be exact zeros"
    else:
        assert is_canary(dpred)


@pytest.mark.parametrize("case", R.MSE_CASES, ids=str)
@pytest.mark.parametrize("dpred_on", [True, False])
def test_mse_scalar_and_wide_forms(case, dpred_on):
    _mse_run(case, False, dpred_on)


@pytest.mark.parametrize("case", R.MSE_CASES[:2], ids=str)
def test_mse_token_weighted(case):
    _mse_run(case, True, True)
    _mse_run(case, True, False)


@pytest.mark.parametrize("case", R.FM_CASES, ids=str)
def test_flowmatch_prepare_modes(case):
    B, S_t, S_c, Cc, mode = case
    for kind in ("exact", "rand"):
        inp, ref = _case("flowmatch", case, kind)
        x0 = dev(inp["x0"].view(torch.int16))
        noise, sigma = dev(inp["noise"]), dev(inp["sigma"])
        ctrl = dev(inp["ctrl"]) if S_c else None
        packed, target = out_bf16(B * (S_t + S_c), Cc), out_bf16(B * S_t, Cc)
        rc = _L().lib.qfx_flowmatch_prepare(x0.data_ptr(), noise.data_ptr(), ptr(ctrl), sigma.data_ptr(), packed.data_ptr(), target.data_ptr(),
                                            B, S_t, S_c, Cc, mode, _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        check_flat("flowmatch", "packed", packed, ref["packed"], case, kind)
        check_flat("flowmatch", "target", target, ref["target"], case, kind)


@pytest.mark.parametrize("with_c", [False, True])
def test_add3(with_c):
    n = 1024 * 256 + 77        # past one trip of the capped grid
    for kind in ("exact", "rand"):
        d = R.case_data(kind, 21, a=(n,), b=(n,), c=(n,))
        ref = R.add3(d["a"], d["b"], d["c"] if with_c else None)["out"][0].to(BF)
        a, b, c = dev(d["a"]), dev(d["b"]), dev(d["c"])
        out = R.canary_bf16(n + 520, device=DEV)
        assert _L().lib.qfx_add3_bf16(a.data_ptr(), b.data_ptr(), ptr(c if with_c else None), out.data_ptr(), n, _stream()) == 0
        torch.cuda.synchronize()
        assert same_bits(out.cpu(), R.flat_image(ref, n + 520)), kind


@pytest.mark.parametrize("case", R.TS_CASES, ids=str)
def test_timestep_embed(case):
    B, dim, scale, pre = case
    inp, ref = _case("timestep", case, "rand")
    t = dev(inp["t"])
    out = out_bf16(B, dim)
    assert _L().lib.qfx_timestep_embed(t.data_ptr(), B, dim, scale, pre, out.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    check_flat("timestep", "out", out, ref["out"], case, "rand")


# ================================================================================================ conditioning head
class Cond:
    def __init__(self, case, kind):
        B, r, K, N, na, apply_silu, wide, dx = case
        lim = R.EXACT_MAX_COND
        assert B <= lim["B"] and r <= lim["r"] and K <= lim["K"] and N <= lim["N"] and na <= lim["na"]
        self.case, self.kind = case, kind
        self.inp, self.ref = _case("cond_fwd", case, kind)
        inp = self.inp
        self.ldy, self.ldg = (N + 13, N + 5) if wide else (N, N)
        self.x = dev(inp["x"])
        self.A, self.Bm = [dev(inp["A"][i]) for i in range(na)], [dev(inp["Bm"][i]) for i in range(na)]
        self.s = dev(inp["s"])
        self.u = out_f32(na * B, r)
        self.y = [R.strided_image(inp["y0"][i], B + 3, self.ldy).to(DEV) for i in range(na)]
        self.g = [dev(R.strided_image(inp["g"][i], B, self.ldg, fill=0.0)) for i in range(na)]
        self.dA = [out_f32(r, K, r * K, R.FILL["dA"]) for _ in range(na)]
        self.dB = [out_f32(N, r, N * r, R.FILL["dB"]) for _ in range(na)]
        self.du = out_f32(na * B, r, na * B * r, R.FILL["du"])
        self.dx = out_f32(B, K, B * K, R.FILL["dx"])
        self.arrays = [ptr_array(v) for v in (self.A, self.Bm, self.y, self.g, self.dA, self.dB)]

    def args(self):
        B, r, K, N, na, apply_silu, wide, dx = self.case
        a = _L().CondLoraArgs()
        a.x, a.B, a.K, a.apply_silu, a.na, a.r, a.N = self.x.data_ptr(), B, K, int(apply_silu), na, r, N
        a.A, a.Bm, a.y, a.g, a.dA, a.dB = [t.data_ptr() for t in self.arrays]
        a.scale, a.u, a.ldy, a.ldg, a.du = self.s.data_ptr(), self.u.data_ptr(), self.ldy, self.ldg, self.du.data_ptr()
        a.dx = self.dx.data_ptr() if dx else None
        return a

    def verify_fwd(self):
        B, r, K, N, na = self.case[:5]
        check_flat("cond_fwd", "u", self.u, self.ref["u"], self.case, self.kind)
        for i in range(na):
            got = self.y[i].cpu()
            assert is_canary(got[B:]) and is_canary(got[:B, N:]), f"cond.y {self.case}: written outside [B, N]"
            check("cond_fwd", "y", got[:B, :N].contiguous(), (self.ref["y"][0][i], self.ref["y"][1][i]), self.case, self.kind)

    def verify_bwd(self, launches):
        """After `launches` backward launches from the initial fills (du refilled between them: the caller's scratch)."""
        B, r, K, N, na, apply_silu, wide, dx = self.case
        u = self.u.cpu()[:na * B * r].view(na, B, r)
        ref = R.cond_bwd_ref(self.inp, self.case, u=u)
        for k, bufs in (("dA", self.dA), ("dB", self.dB)):
            for i in range(na):
                val, sc = ref[k][0][i], ref[k][1][i]
                check_flat("cond_bwd", k, bufs[i], (R.FILL[k] + launches * (val - R.FILL[k]), sc), self.case, self.kind)
        check_flat("cond_bwd", "du", self.du, ref["du"], self.case, self.kind)
        if dx:
            check_flat("cond_bwd", "dx", self.dx, (R.FILL["dx"] + launches * (ref["dx"][0] - R.FILL["dx"]), ref["dx"][1]), self.case, self.kind)
        else:
            assert same_bits(self.dx.cpu(), R.flat_image(torch.full((B * K,), R.FILL["dx"]), self.dx.numel(), torch.float32))


@pytest.mark.parametrize("case", R.COND_CASES, ids=str)
def test_cond_lora_fwd_bwd_and_accumulation(case):
    L = _L()
    for kind in ("exact", "rand"):
        p = Cond(case, kind)
        a = p.args()
        assert L.lib.qfx_cond_lora_fwd(C.byref(a), _stream()) == 0
        torch.cuda.synchronize()
        p.verify_fwd()
        assert L.lib.qfx_cond_lora_bwd(C.byref(a), _stream()) == 0
        torch.cuda.synchronize()
        p.verify_bwd(1)
        p.du[:case[4] * case[0] * case[1]] = R.FILL["du"]
        assert L.lib.qfx_cond_lora_bwd(C.byref(a), _stream()) == 0
        torch.cuda.synchronize()
        p.verify_bwd(2)


def test_cond_lora_refusals():
    L = _L()
    p = Cond(R.COND_CASES[1], "exact")
    before = [t.clone() for t in p.y + p.dA + p.dB + [p.u, p.du, p.dx]]

    def changed(**kw):
        a = p.args()
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    for what, a in (("r = 65", changed(r=65)), ("B = 9", changed(B=9))):
        assert L.lib.qfx_cond_lora_fwd(C.byref(a), _stream()) == EINVAL, what
        assert L.lib.qfx_cond_lora_bwd(C.byref(a), _stream()) == EINVAL, what
    assert L.lib.qfx_cond_lora_fwd(C.byref(changed(y=None)), _stream()) == EINVAL
    assert L.lib.qfx_cond_lora_bwd(C.byref(changed(g=None)), _stream()) == EINVAL
    torch.cuda.synchronize()
    for t0, t1 in zip(before, p.y + p.dA + p.dB + [p.u, p.du, p.dx]):
        assert same_bits(t0.cpu(), t1.cpu())


@pytest.mark.parametrize("n", (1000, R.GRID_STRIDE_N[0]))
def test_cast_f32_bf16(n):
    g = torch.Generator().manual_seed(n)
    for src in (torch.randn(n, generator=g), R.ints(g, n, dtype=torch.float32) * 2.0 ** -4):
        out = R.canary_bf16(n + 520, device=DEV)
        assert _L().lib.qfx_cast_f32_bf16(dev(src).data_ptr(), out.data_ptr(), n, _stream()) == 0
        torch.cuda.synchronize()
        assert same_bits(out.cpu(), R.flat_image(src.to(BF), n + 520))


@pytest.mark.parametrize("n", R.SILU_BWD_N)
def test_silu_bwd(n):
    inp, ref = _case("silu_bwd", n, "rand")
    ds, x = dev(inp["ds"]), dev(inp["x"])
    out = R.canary_bf16(n + 520, device=DEV)
    assert _L().lib.qfx_silu_bwd(ds.data_ptr(), x.data_ptr(), out.data_ptr(), n, _stream()) == 0
    torch.cuda.synchronize()
    check_flat("silu_bwd", "dx", out, ref["dx"], n, "rand")
