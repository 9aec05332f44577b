"""CPU: tests/rowkernel_ref.py is right, and the bars of tests/test_rowkernel_gpu.py are honest.
  * every backward restatement with its rounding points switched off equals fp64 autograd of the plain formula to 1e-12;
  * the forward restatements agree with the modules of oracle/qwen_dit.py on bf16 inputs;
  * the exactness premise of exact_case holds at the stated maximum contraction lengths;
  * BARS: 2 x the reference's own fp32 reordering noise, measured here on the GPU tests' case lists, fits under every bar;
  * the case lists hold every shape value the dispatch paths of the kernels are selected by."""
import math

import pytest
import torch
import torch.nn.functional as F

import rowkernel_ref as R
from oracle import qwen_dit as O

BF, F64 = torch.bfloat16, torch.float64
TOL = 1e-12


def close(a, b):
    return (a.double() - b.double()).abs().max().item() <= TOL * max(1.0, b.double().abs().max().item())


def g64(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64) * scale


# ------------------------------------------------------------------------------------------------ backward restatements vs autograd
def test_ln_bwd_and_mod_grad_without_rounding_are_autograd():
    rows, D, rpb = 7, 24, 3
    B = 3
    x, dy, dres, dxo = g64(rows, D, seed=1), g64(rows, D, seed=2), g64(rows, D, seed=3), g64(rows, D, seed=4)
    shift, scale, gate = [g64(B, D, seed=5 + i).requires_grad_() for i in range(3)]
    xl = x.clone().requires_grad_()
    b = torch.arange(rows) // rpb
    ln = F.layer_norm(xl, (D,), eps=float(torch.tensor(R.EPS, dtype=torch.float32)))
    xm = ln * (1 + scale[b]) + shift[b]
    xm.backward(dy)
    got = R.ln_bwd(dy, x, scale.detach(), rpb, dres=dres, gate=gate.detach(), rnd=False)
    assert close(got["dx"][0], dres + xl.grad)
    assert close(got["dyg"][0], gate.detach()[b] * (dres + xl.grad))
    assert close(R.ln_bwd(dy, x, scale.detach(), rpb, rnd=False)["dx"][0], xl.grad)
    # d(gate) of xo = res + gate * y
    y = g64(rows, D, seed=9)
    (gate[b] * y).backward(dxo)
    mg = R.mod_grad(dy, x, rpb, dxo=dxo, y=y, rnd=False)
    assert close(mg["dshift"][0], shift.grad) and close(mg["dscale"][0], scale.grad) and close(mg["dgate"][0], gate.grad)
    # masked rows: no gradient flows through them
    mask = torch.tensor([1.0, 0, 1, 1, 0, 1, 1])
    mgm = R.mod_grad(dy, x, rpb, dxo=dxo, y=y, mask=mask, rnd=False)
    mg0 = R.mod_grad(dy * mask[:, None], x, rpb, dxo=dxo * mask[:, None], y=y, rnd=False)
    assert all(close(mgm[k][0], mg0[k][0]) for k in mg0)
    masked = R.ln_bwd(dy, x, scale.detach(), rpb, dres=dres, gate=gate.detach(), mask=mask, rnd=False)
    assert not masked["dx"][0][[1, 4]].any() and not masked["dyg"][0][[1, 4]].any() and close(masked["dx"][0][[0, 2, 3, 5, 6]], got["dx"][0][[0, 2, 3, 5, 6]])


@pytest.mark.parametrize("flags,T", [(0, 2), (1, 0), (0, 5)])
def test_qk_bwd_without_rounding_is_autograd(flags, T):
    B, S, H, dh = 2, 5, 3, 16
    x = g64(B, S, 3 * H * dh, seed=1)
    dy = g64(B, S, 3 * H * dh, seed=2)
    ang = g64(B, S, dh // 2, seed=3)
    rope = torch.stack([torch.cos(ang), torch.sin(ang)], -1)
    ws = [1 + 0.1 * g64(dh, seed=4 + i) for i in range(4)]
    xl = x.clone().requires_grad_()
    xv = xl[..., :2 * H * dh].reshape(B, S, 2, H, dh)
    eps = float(torch.tensor(R.EPS, dtype=torch.float32))
    t = xv * torch.rsqrt(xv.pow(2).mean(-1, keepdim=True) + eps) * R._qk_w(ws, S, T, F64)
    tc = torch.view_as_complex(t.reshape(B, S, 2, H, dh // 2, 2))
    out = torch.view_as_real(tc * torch.complex(rope[..., 0], rope[..., 1])[:, :, None, None]).flatten(-2)
    assert close(R.qk_fwd(x, rope, ws, T, H, dh, flags, rnd=False)["out"][0], out.detach())
    out.backward(dy[..., :2 * H * dh].reshape(B, S, 2, H, dh))
    got = R.qk_bwd(dy, x[..., :2 * H * dh], rope, ws, T, H, dh, flags, rnd=False)["out"][0]
    assert close(got, xl.grad[..., :2 * H * dh].reshape(B, S, 2, H, dh))
    assert not xl.grad[..., 2 * H * dh:].any()


def test_silu_bwd_and_criteria_without_rounding_are_autograd():
    x = g64(50, seed=1, scale=2.0).requires_grad_()
    ds = g64(50, seed=2)
    F.silu(x).backward(ds)
    assert close(R.silu_bwd(ds, x.detach(), rnd=False)["dx"][0], x.grad)
    B, S_all, S_t, Cc, gs = 2, 5, 3, 4, 0.75
    pred = g64(B, S_all, Cc, seed=3).requires_grad_()
    target, tw = g64(B, S_t, Cc, seed=4), g64(B, S_t, seed=5).abs()
    loss = ((pred[:, :S_t] - target) ** 2).mean()
    (loss * gs).backward()
    got = R.mse(pred.detach(), target, S_t, gs, rnd=False)
    assert close(got["loss"][0], loss.detach()) and close(got["dpred"][0], pred.grad)
    pred.grad = None
    inv_denom = 1.0 / 5.5
    loss = (tw * ((pred[:, :S_t] - target) ** 2).mean(-1)).sum() * inv_denom
    (loss * gs).backward()
    got = R.mse_tw(pred.detach(), target, tw, S_t, inv_denom, gs, rnd=False)
    assert abs(got["loss"][0].item() - loss.item()) <= 1e-7 * abs(loss.item())       # inv_denom, gscale enter as fp32 words
    assert (got["dpred"][0] - pred.grad).abs().max().item() <= 1e-7 * pred.grad.abs().max().item()
    got = R.mse_tw(pred.detach(), target, tw, S_t, 0.25, gs, rnd=False)               # fp32-exact constants: the formula itself to 1e-12
    assert close(got["dpred"][0], pred.grad * (0.25 / inv_denom))


@pytest.mark.parametrize("apply_silu", [False, True])
def test_cond_adapter_gradients_without_rounding_are_autograd(apply_silu):
    B, r, K, N, na = 3, 4, 10, 7, 2
    x = g64(B, K, seed=1)
    A, Bm = g64(na, r, K, seed=2).requires_grad_(), g64(na, N, r, seed=3).requires_grad_()
    s = torch.tensor([0.5, 2.0], dtype=F64)
    y0, g = g64(na, B, N, seed=4), g64(na, B, N, seed=5)
    ax = (F.silu(x) if apply_silu else x.clone()).requires_grad_()
    y = y0 + s[:, None, None] * torch.einsum("anj,abj->abn", Bm, torch.einsum("ajk,bk->abj", A, ax))
    fwd = R.cond_fwd(x, A.detach(), Bm.detach(), s, y0, apply_silu, rnd=False)
    assert close(fwd["y"][0], y.detach())
    y.backward(g)
    z = lambda *sh: torch.zeros(*sh, dtype=F64)      # noqa: E731
    got = R.cond_bwd(x, A.detach(), Bm.detach(), s, fwd["u"][0], g, apply_silu, z(na, r, K), z(na, N, r), z(na, B, r), z(B, K), rnd=False)
    assert close(got["dA"][0], A.grad) and close(got["dB"][0], Bm.grad) and close(got["dx"][0], ax.grad)
    # accumulation onto the initial values
    got1 = R.cond_bwd(x, A.detach(), Bm.detach(), s, fwd["u"][0], g, apply_silu, z(na, r, K) + 0.5, z(na, N, r) - 1.5, z(na, B, r), z(B, K) + 2.0, rnd=False)
    assert close(got1["dA"][0], A.grad + 0.5) and close(got1["dB"][0], Bm.grad - 1.5) and close(got1["dx"][0], ax.grad + 2.0)


# ------------------------------------------------------------------------------------------------ forward restatements vs the oracle
def test_forward_restatements_agree_with_the_oracle_modules():
    g = torch.Generator().manual_seed(5)
    rows, D = 6, 520
    x, w = R.randn_bf(g, rows, D), (1 + 0.1 * torch.randn(D, generator=g)).to(BF)
    # OracleRMSNorm with a bf16 weight rounds at the restatement's two points: the fp32 form of the restatement gives its bits
    norm = O.OracleRMSNorm(D, eps=R.EPS)
    norm.weight.data = w.clone()
    want = norm(x).detach()
    assert want.dtype == BF
    got32, got64 = R.rmsnorm(x, w, dt=torch.float32)["y"][0], R.rmsnorm(x, w)
    assert torch.equal(R.bits(got32.to(BF)), R.bits(want))
    assert R.err_ulps(want, *got64["y"]) <= R.BARS["rmsnorm.y"]
    # the AdaLN expression of OracleQwenBlock._modulate on bf16 tensors: bf16(LN), bf16(1 + scale), bf16(product), bf16(sum)
    B, S = 2, 3
    xs = R.randn_bf(g, B, S, D)
    mod = R.randn_bf(g, B, 3 * D, scale=0.5)
    ln = F.layer_norm(xs, (D,), eps=R.EPS)
    want, _ = O.OracleQwenBlock._modulate(ln, mod)
    shift, scale, _ = mod.chunk(3, dim=-1)
    got = R.ln_fwd(xs.reshape(B * S, D), shift, scale, S)
    assert R.err_ulps(want.reshape(B * S, D), *got["y"]) <= R.BARS["ln_fwd.y"]
    assert (R.bits(got["y"][0].to(BF)) == R.bits(want.reshape(B * S, D))).float().mean().item() > 0.999
    # QK norm + rope: OracleRMSNorm over dh, then apply_rope_complex (fp32 complex product, one rounding)
    H, dh, T = 3, 64, 1
    qkv = R.randn_bf(g, B, S, 3 * H * dh)
    ws = [(1 + 0.1 * torch.randn(dh, generator=g)).to(BF) for _ in range(4)]
    ang = torch.rand(S, dh // 2, generator=g) * 6.28
    rope = torch.stack([torch.cos(ang), torch.sin(ang)], -1)[None]
    freqs = torch.complex(rope[0, ..., 0], rope[0, ..., 1])
    qn = O.OracleRMSNorm(dh, eps=R.EPS)
    want = []
    for which in (0, 1):
        sec = qkv[..., which * H * dh:(which + 1) * H * dh].reshape(B, S, H, dh)
        parts = []
        for lo, hi, wsel in ((0, T, ws[which]), (T, S, ws[2 + which])):
            qn.weight.data = wsel.clone()
            parts.append(qn(sec[:, lo:hi]).detach())
        want.append(O.apply_rope_complex(torch.cat(parts, 1), freqs))
    want = torch.stack(want, 2)
    got32 = R.qk_fwd(qkv, rope, ws, T, H, dh, dt=torch.float32)["out"][0]
    got64 = R.qk_fwd(qkv, rope, ws, T, H, dh)["out"]
    assert (R.bits(got32.to(BF)) == R.bits(want)).float().mean().item() > 0.999
    assert R.err_ulps(want, *got64) <= R.BARS["qk_fwd.out"] + 1      # the oracle's complex product may contract to FMAs
    # timestep_sinusoid (fp32, cos first): the same table within one rounding of the bf16 output
    t = torch.tensor([0.25, 0.7109, 0.93]).to(BF).float()
    want = O.timestep_sinusoid(t, 256, 1000.0).to(BF)
    got = R.timestep_embed(t, 256, 1000.0, 1.0)["out"]
    assert R.err_ulps(want, *got) <= 1.0


# ------------------------------------------------------------------------------------------------ the exactness premise
def _three_orders_exact(terms):
    """fp32 sums of `terms` (last axis) forward, reversed and pairwise give the bits of the fp64 sum."""
    want = terms.double().sum(-1)
    f = torch.zeros(terms.shape[:-1])
    b = torch.zeros(terms.shape[:-1])
    for i in range(terms.shape[-1]):
        f = f + terms[..., i]
        b = b + terms[..., terms.shape[-1] - 1 - i]
    p = terms.clone()
    while p.shape[-1] > 1:
        if p.shape[-1] % 2:
            p = torch.cat([p, torch.zeros_like(p[..., :1])], -1)
        p = p[..., 0::2] + p[..., 1::2]
    return all(torch.equal(v.double(), want) for v in (f, b, p[..., 0]))


def test_exact_case_premise_at_the_maximum_lengths():
    g = torch.Generator().manual_seed(1)
    worst = {   # (largest |term|, granularity, terms, largest addend beside the sum): magnitude / granularity must fit 24 bits
        "mod_grad": (4 * 2.0 ** -4 * 4, 2.0 ** -4, R.EXACT_MAX_ROWS, 2.0),
        "mod_gemv": (4 * 2.0 ** -4 * 4, 2.0 ** -4, R.EXACT_MAX_GEMV_K, 2.0),
        "mod_gemv_t": (4.0, 2.0 ** -4, R.EXACT_MAX_GEMV_T, 2.0),
    }
    for name, (term, gran, n, add) in worst.items():
        assert (term * n + add) / gran < 2 ** 24, name
    c = R.EXACT_MAX_COND
    u = 4 * c["K"]                              # |u| <= sum_k |A| |x|
    ga = 2 * 1.0                                # |s g|
    du = ga * 2 * c["N"] + 0.25
    for name, mag in (("y", 2 * u * c["r"] + 2), ("dB", ga * u * c["B"] + 1.5), ("du", du), ("dA", du * 2 * c["B"] + 0.5),
                      ("dx", du * 2 * c["r"] * c["na"] + 2.0)):
        assert mag / 0.25 < 2 ** 24, name
    # and on data: the three longest contractions in three orders
    for n, sc in ((R.EXACT_MAX_GEMV_K, 2.0 ** -4), (R.EXACT_MAX_GEMV_T, 2.0 ** -4), (R.EXACT_MAX_COND["K"], 1.0)):
        a, b = R.ints(g, 16, n, dtype=torch.float32), R.ints(g, 16, n, scale=sc, dtype=torch.float32)
        assert _three_orders_exact(a * b), n
    case = (8, 64, 3072, 1000, 3, False, True, True)
    assert case in R.COND_CASES
    inp = R.cond_make(case, "exact")
    r64, r32 = R.cond_bwd_ref(inp, case), R.cond_bwd_ref(inp, case, torch.float32, True)
    f64, f32 = R.cond_fwd_ref(inp, case), R.cond_fwd_ref(inp, case, torch.float32, True)
    for k in ("dA", "dB", "du", "dx"):
        assert torch.equal(r32[k][0].double(), r64[k][0]), k
    assert torch.equal(f32["u"][0].double(), f64["u"][0]) and torch.equal(f32["y"][0].double(), f64["y"][0])


# ------------------------------------------------------------------------------------------------ where the tolerance comes from
def test_bars_are_twice_the_reference_noise():
    floors = R.measure_floors()
    assert set(floors) == set(R.BARS), set(floors) ^ set(R.BARS)
    for k, f in sorted(floors.items()):
        print(f"{k:20s} floor {f:.3g} ulps, bar {R.BARS[k]}")
        assert R.BARS[k] == int(R.BARS[k]) and R.BARS[k] >= 1
        assert 2 * f <= R.BARS[k], (k, f, R.BARS[k])
        assert R.BARS[k] == max(1, math.ceil(2 * f)), (k, f, "the bar is 2 x floor rounded up, no more")


def test_exact_outputs_are_exact_in_the_reference_too():
    """On exact_case data the fp32, reversed-order restatement gives the fp64 bits for every output the GPU tests hold to bit-equality."""
    for fam, (prefix, cases, kinds, make, ref) in R.FAMILIES.items():
        if "exact" not in kinds:
            continue
        for case in cases:
            names = R.exact_outputs(fam, case, "exact")
            if not names:
                continue
            inp = make(case, "exact")
            r64, r32 = ref(inp, case), ref(inp, case, torch.float32, True)
            for k in names:
                if k in r64:       # (d(gate) only where the case has a gate)
                    assert torch.equal(r32[k][0].double(), r64[k][0]), (fam, case, k)


# ------------------------------------------------------------------------------------------------ the case lists reach every path
def test_case_lists_hold_every_dispatch_value():
    def vals(cases, i):
        return {c[i] for c in cases}
    assert vals(R.LN_FWD_CASES, 0) == {8, 264, 512, 520, 1536, 3072, 3080, 3584, 4096} and vals(R.LN_FWD_CASES, 1) == {1, 4, 5, 7}
    assert vals(R.LN_FWD_CASES, 2) == {"shared", "tight", "six"} and [len(b) for b in R.LN_FWD_BATCHES] == [2, 3, 4]
    assert all(r % 4 == 0 for b in R.LN_FWD_BATCHES for _, r in b[:-1]) and all(b[-1][1] % 4 for b in R.LN_FWD_BATCHES)
    assert vals(R.LN_BWD_CASES, 0) == {8, 520, 3072, 3080, 3584, 4096}
    for D in R.LN_BWD_D:       # both instantiations see dres and dyg present and absent; both gate strides; masks
        mine = [c for c in R.LN_BWD_CASES if (c[0] <= 3072) == (D <= 3072)]
        assert {c[2] for c in mine} == {True, False} and {c[3] for c in mine} == {True, False} and {c[4] for c in mine if c[3]} == {"shared", "six"}
        assert any(0 in c[5] or 4 in c[5] for c in mine) and any(3 in c[5] for c in mine)
    assert vals(R.MG_CASES, 0) == {512, 520, 1032, 2048, 2056, 3072, 3080, 4096} and vals(R.MG_CASES, 1) == {1, 8, 9, 17} and vals(R.MG_CASES, 2) == {1, 3}
    assert {(c[0] + 511) // 512 for c in R.MG_CASES} == {1, 2, 3, 4, 5, 6, 7, 8}
    for i in (3, 4, 5, 6):
        assert vals(R.MG_CASES, i) == {True, False}
    assert any(c[3] and R.mg_rows(c) < c[1] * c[2] for c in R.MG_CASES)
    assert any(len({B for _, B in probs}) > 1 and len(probs) == 4 for _, probs in R.MG_BATCHES)
    assert set(R.RMS_CASES) >= {(8, 1), (520, 5), (3584, 1), (4096, 5)}
    assert vals(R.GEMV_CASES, 0) == {1, 3, 8} and vals(R.GEMV_CASES, 1) == {8, 256, 520, 4096} and vals(R.GEMV_CASES, 2) == {1, 15, 16, 17, 130}
    assert vals(R.GEMV_CASES, 3) == {1, 3} and vals(R.GEMV_CASES, 4) == {True, False} and vals(R.GEMV_CASES, 5) == {True, False}
    assert any(c[0] == 8 and c[1] == 4096 for c in R.GEMV_CASES)
    assert vals(R.GEMVT_CASES, 0) == {1, 2, 3, 8} and vals(R.GEMVT_CASES, 1) == {8, 520, 1024, 1536, 2048, 3072} and vals(R.GEMVT_CASES, 2) == {1, 3, 4, 5, 130}
    for np_ in (2, 4, 6):      # every <NB, NP> of the transposed GEMV: a pair pass and a single pass
        mine = [c for c in R.GEMVT_CASES if (2 if c[1] <= 1024 else 4 if c[1] <= 2048 else 6) == np_]
        assert any(c[0] >= 2 for c in mine) and any(c[0] % 2 for c in mine), np_
    assert any(c[0] == 8 for c in R.GEMVT_CASES)
    for dh in (64, 128):
        mine = [c for c in R.QK_CASES if c[0] == dh]
        assert any(c[6] and c[1] > 1 for c in mine) and any(c[5] & 1 for c in mine) and any(c[3] == 0 for c in mine) or dh == 128
        assert any(c[3] == c[2] for c in mine) and any(not c[7] for c in mine)
    assert any(c[0] == 128 and c[3] == 0 for c in R.QK_CASES) and any(c[0] == 128 and c[5] & 1 for c in R.QK_CASES)
    assert vals(R.COND_CASES, 0) == {1, 3, 8} and vals(R.COND_CASES, 1) == {1, 16, 64} and vals(R.COND_CASES, 2) == {8, 300, 3072}
    assert vals(R.COND_CASES, 3) == {1, 255, 256, 257, 1000} and vals(R.COND_CASES, 4) == {1, 3}
    for i in (5, 6, 7):
        assert vals(R.COND_CASES, i) == {True, False}
    assert R.GRID_STRIDE_N[0] > 2048 * 256 and R.GRID_STRIDE_N[1] > 1024 * 256
