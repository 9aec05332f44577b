"""CPU: tests/gemm_ref.py is right, and the bars of tests/test_gemm_gpu.py are honest.
  * with its rounding points off the restatement is torch's fp64 A @ B.T + bias; gelu_tanh / gelu_tanh' are F.gelu(approximate="tanh")
    and its fp64 autograd, to 1e-12;
  * quant_mxfp8_ref + dequantisation equals oracle.mxfp8.mx_qdq on random data and on the edge blocks; the scale bytes sit where
    include/qfx.h puts them;
  * the exactness premise of exact_case holds at EXACT_MAX_K (fp32 in three summation orders = fp64, bit for bit);
  * BARS: exactly 2 x the reference's own fp32 noise, measured here on the GPU tests' case lists, rounded up, at least one ulp;
  * the flush clause of gelu_sweep_case covers under 2 % of the table;
  * the case lists hold every shape value the dispatch paths are selected by."""
import math

import pytest
import torch
import torch.nn.functional as F

import gemm_ref as G
from oracle import mxfp8 as QX

BF, F64, F32 = torch.bfloat16, torch.float64, torch.float32
TOL = 1e-12


def close(a, b):
    return (a.double() - b.double()).abs().max().item() <= TOL * max(1.0, b.double().abs().max().item())


@pytest.mark.parametrize("seg2_plain", [False, True])
def test_without_rounding_the_restatement_is_a_plain_product(seg2_plain):
    case = G.Case(G.NONE, 37, 20, 64, 64, rpb=13, seg2_plain=seg2_plain)
    inp = G.make_inputs(case, "rand")
    want = inp["A1"].double() @ inp["B1"].double().t() + inp["A2"].double() @ inp["B2"].double().t() + inp["bias"].double()
    assert close(G.gemm_ref(inp, case, rnd=False)["C"][0], want)
    assert close(G.gemm_ref(inp, case, rnd=False, flip="perm")["C"][0], want)
    # epilogues on top of it
    y = want
    gel = G.gemm_ref(inp, G.replace(case, epi=G.GELU), rnd=False)
    assert close(gel["C"][0], y) and close(gel["C2"][0], F.gelu(y, approximate="tanh"))
    gr = G.gemm_ref(inp, G.replace(case, epi=G.GATE_RES, c2=True), rnd=False)
    b = torch.arange(37) // 13
    assert close(gr["C"][0], inp["aux"].double() + inp["gate"].double()[b] * y) and close(gr["C2"][0], y)
    h = inp["aux"].double().requires_grad_()
    F.gelu(h, approximate="tanh").sum().backward()
    assert close(G.gemm_ref(inp, G.replace(case, epi=G.DGELU), rnd=False)["C"][0], y * h.grad)
    # masked rows are zeros, the others untouched
    m = G.replace(case, mask=(0, 36))
    got = G.gemm_ref(G.make_inputs(m, "rand"), m, rnd=False)["C"][0]
    assert not got[[0, 36]].any() and close(got[1:36], want[1:36])


def test_gelu_forms():
    x = torch.linspace(-12, 12, 4001, dtype=F64).requires_grad_()
    y = F.gelu(x, approximate="tanh")
    y.sum().backward()
    assert close(G.gelu_tanh(x.detach()), y.detach()) and close(G.gelu_tanh_grad(x.detach()), x.grad)
    # the kernels' rewrite is the same function (fp32 arithmetic: 1e-6)
    x32 = x.detach().float()
    assert (G.gelu_kernel_form(x32).double() - y.detach()).abs().max() < 1e-6
    assert (G.gelu_grad_kernel_form(x32).double() - x.grad).abs().max() < 1e-5       # (the exponent's argument reaches 2^7: 2^-17 absolute)


def _edge_blocks():
    x = G.quant_input((4, 256, 0, 0))
    x[1, :32] = 300.0 * 2.0 ** 40
    x[2, 32:64] = -(2.0 ** -100)
    return x


def test_quant_mxfp8_ref_is_the_oracle_quantiser():
    for x in (G.quant_input((33, 384, 0, 0)), _edge_blocks(), (torch.randn(16, 128, generator=torch.Generator().manual_seed(1)) * 1e-3).to(BF)):
        byte, S, deq = G.quant_mxfp8_ref(x)
        assert torch.equal(deq, QX.mx_qdq(x).double())
        # the bytes are the e4m3fn encoding of the scaled elements, negative zeros included
        M, K = x.shape
        sc = S.view(K // 128, M, 4).permute(1, 0, 2).reshape(M, K // 32).double() - 127
        again = byte.view(torch.float8_e4m3fn).double().view(M, K // 32, 32) * torch.pow(2.0, sc)[..., None]
        assert torch.equal(again.view(M, K), deq) and torch.equal(torch.signbit(again.view(M, K)), torch.signbit(x.double()))
    x = _edge_blocks()
    byte, S, deq = G.quant_mxfp8_ref(x)
    r = 3
    assert S[(0 * 4 + 0) * 4 + 0] == 0 and not byte[0, :32].any()                               # all-zero block: scale byte 0
    assert byte[r, 40] == 0x7E and deq[r, 40] == 56.0                                           # 448 * 2^-3 -> the code of 448
    assert byte[0, 70] == 0xFE and deq[0, 70] == -1.75                                          # 496 saturates at 448 (RNE alone: 512)
    assert deq[r, 100] == 1.75 and byte[r, 100] == 0x7E and S[(0 * 4 + r) * 4 + 3] == 127 - 8   # a maximum just below 2: exponent of 1, 510 saturates
    assert S[(0 * 4 + 0) * 4 + 3] == 0 and byte[0, 100] == 0x80                                 # E8M0 minimum; -0 keeps its sign


def test_scale_bytes_are_tile_major():
    M, K = 5, 384
    x = torch.zeros(M, K, dtype=BF)
    for m in range(M):
        for kb in range(K // 32):
            x[m, kb * 32] = 2.0 ** (m + 4 * kb - 20)
    _, S, _ = G.quant_mxfp8_ref(x)
    for m in range(M):
        for kb in range(K // 32):
            assert S[((kb // 4) * M + m) * 4 + kb % 4] == (m + 4 * kb - 20) - 8 + 127
    img = G.scale_image(S, M, torch.tensor([1, 2, 3, 7, 8]), 10)
    assert img.view(3, 10, 4)[2, 7, 1] == S[(2 * M + 3) * 4 + 1] and img.view(3, 10, 4)[0, 0, 0] == G.CANARY_U8


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("epi,seg2_plain", [(G.NONE, False), (G.NONE, True), (G.GELU, False), (G.GATE_RES, False), (G.GATE_RES, True)])
def test_exact_case_premise_at_the_longest_contraction(epi, seg2_plain, fp8):
    """Worst-case magnitude x granularity fits fp32, and fp32 sums in three orders give the fp64 bits."""
    K2 = 128
    K1 = G.EXACT_MAX_K - K2
    assert (4 * K1 + 2 + K2 / 64) * 2 ** 8 < 2 ** 24
    case = G.Case(epi, 24, 32, K1, K2, rpb=12, c2=True, seg2_plain=seg2_plain, fp8=fp8)
    inp = G.make_inputs(case, "exact")
    if fp8:      # the MX image of exact_case data is the data
        x = G.make_inputs(G.replace(case, fp8=False), "exact")["A1"]
        assert torch.equal(G.quant_mxfp8_ref(x)[2], x.double())
    r64 = G.gemm_ref(inp, case)
    assert r64["C"][0].abs().max() > 8            # (not a trivial case)
    for flip in (False, True, "perm"):
        r32 = G.gemm_ref(inp, case, F32, flip, kernel_form=True)
        for k in r64:
            if G.key_of(case, k) in G.EXACT_OUTPUTS:
                assert torch.equal(r32[k][0].double(), r64[k][0]), (k, flip)
                assert torch.equal(r64[k][0], r64[k][0].to(BF).double())


def test_exact_case_data_make_the_mid_rounding_matter():
    """On exact_case data with K1 >= 192 the base sums pass 2^8: rounding them before the LoRA segment (the contract) and rounding once at
    the end (seg2_plain, or a kernel that lost its mid-rounding) give different bits on a good share of the elements."""
    for K1 in (192, 320):
        case = G.Case(G.NONE, 64, 64, K1, 64)
        inp = G.make_inputs(case, "exact")
        assert inp["A1"].abs().max() <= 2 and inp["B1"].abs().max() <= 2 and torch.equal(inp["A1"], inp["A1"].round())
        mid = G.gemm_ref(inp, case)["C"][0]
        once = G.gemm_ref(inp, G.replace(case, seg2_plain=True))["C"][0]
        assert (mid != once).double().mean().item() > 0.05, (K1, (mid != once).double().mean().item())


def test_bars_are_twice_the_reference_noise():
    floors = G.measure_floors()
    assert set(floors) == set(G.BARS), set(floors) ^ set(G.BARS)
    for k, f in sorted(floors.items()):
        print(f"{k:14s} floor {f:.3g} ulps, bar {G.BARS[k]}")
        assert G.BARS[k] == int(G.BARS[k]) and G.BARS[k] >= 1
        assert 2 * f <= G.BARS[k], (k, f, G.BARS[k])
        assert G.BARS[k] == max(1, math.ceil(2 * f)), (k, f, "the bar is 2 x floor rounded up, no more")


def test_sweep_table_and_flush_clause():
    tab = G.sweep_table()
    assert tab.numel() == 2 * (68 * 128 + 1) + 2 and tab.unique().numel() == tab.numel() - 1      # (+0 == -0 as values)
    a = tab.double().abs()
    assert a[2:].min() == 2.0 ** -64 and a.max() == 16.0
    for case in G.SWEEP_CASES:
        inp = G.make_inputs(case, "rand")
        ref = G.gemm_ref(inp, case)
        # h (GELU) / y (DGELU) come out of the contraction exactly
        want = inp["B1"].t() if case.epi == G.GELU else None
        if want is not None:
            assert torch.equal(G.bits(ref["C"][0].to(BF)), G.bits((want.double() + 0.0).to(BF)))      # (a sum never gives -0: h = -0 arrives as +0)
            assert set(G.bits(want).flatten().tolist()) == set(G.bits(tab).tolist())
        else:
            assert set(G.bits(inp["aux"]).flatten().tolist()) == set(G.bits(tab).tolist())
        k = "C2" if case.epi == G.GELU else "C"
        # (the clause is counted over the distinct table values, i.e. the first tab.numel() slots)
        fl = G.flushed(ref[k][0]).flatten()[:tab.numel()] & (inp["aux"].flatten()[:tab.numel()].double() != 0)
        assert fl.double().mean().item() < 0.02, fl.double().mean().item()


def test_case_lists_hold_every_dispatch_value():
    for e in G.EPIS:
        cs = G.SMALL_CASES[e]
        assert {c.M for c in cs} == set(G.SMALL_M) and {c.N for c in cs} == set(G.SMALL_N)
        assert {(c.M, c.N) for c in cs} >= {(m, n) for m in G.SMALL_M for n in G.SMALL_N}
        assert {(c.K1, c.K2) for c in cs} == {(a, b) for a in G.K1S for b in G.K2S}
        assert all(((c.M + 255) // 256) * ((c.N + 127) // 128) < 160 for c in cs)
        for geo, (bmt, tn) in G.GEOS.items():
            cs = G.PERSIST_CASES[(geo, e)]
            assert {c.M for c in cs} == set(G.persist_ms(bmt)) and {c.N for c in cs} == set(G.persist_ns(geo))
            assert {(c.K1, c.K2) for c in cs} == {(a, b) for a in G.K1S for b in G.K2S}
            assert tn != 256 or all(c.N % 256 == 0 for c in cs)
            assert all(c.N % 8 == 0 for c in cs)
        assert {(c.K1, c.K2) for c in G.FP8_PERSIST_CASES[e]} == {(a, b) for a in G.FP8_K1S for b in G.FP8_K2S}
        assert all(c.fp8 and not c.a_map for c in G.FP8_SMALL_CASES[e] + G.FP8_PERSIST_CASES[e])
        assert any(c.c_map for c in G.FP8_SMALL_CASES[e]) and any(c.c_map for c in G.FP8_PERSIST_CASES[e])
    every = [c for cs in G.ALL_FAMILIES.values() for c in cs]
    for flag in ("mask", "c_map", "a_map", "aux_unmapped", "seg2_plain", "c2", "gate_shared"):
        assert any(getattr(c, flag) for c in every) and any(not getattr(c, flag) for c in every), flag
    assert {c.pad for c in every} == {0, 8, 24} and any(c.B == 3 and c.epi == G.GATE_RES and not c.gate_shared for c in every)
    assert all(c.K1 + c.K2 <= G.EXACT_MAX_K for c in every)
    for geo, (bmt, tn) in G.GEOS.items():
        assert all(((c.M + bmt - 1) // bmt) * ((c.N + tn - 1) // tn) > 256 for c in G.MANY_TILE_CASES[geo])
    assert all(c.N % 256 for c in G.FALLBACK_CASES)
    assert sorted(len(p) for _, p in G.GROUPED_CASES) == [2, 2, 2, 3, 6, 6]
    assert all(len({c.epi for c in p}) == 1 for _, p in G.GROUPED_CASES)
    for geo, cs in G.LANDING_CASES.items():
        bmt, tn = G.GEOS[geo]
        assert all(c.epi == G.DGELU and ((c.M + bmt - 1) // bmt) * ((c.N + tn - 1) // tn) <= 3 for c in cs)
        assert {bool(c.mask) for c in cs} == {True, False} and {c.M % 16 == 0 for c in cs} == {True, False}
        assert {c.bias and (c.K2 == 0 or c.seg2_plain) for c in cs} == {True, False} and {c.aux_unmapped for c in cs} == {True, False}
        wrows = bmt // 2                   # rows per compute wave of both geometries (2 x 4 waves)
        assert {bool(c.c_map) and c.rpb < min(c.M, wrows) for c in cs} == {True, False}      # a sample boundary inside a wave's rows, or not
    assert all(c.N % 128 == 0 and c.epi != G.GATE_RES for c in G.FP8_QUANT_EPI_CASES) and {c.epi for c in G.FP8_QUANT_EPI_CASES} == {0, 1, 3}
