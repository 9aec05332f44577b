"""CPU: tests/attn_ref.py is right, and the bars of tests/test_attn_gpu.py are honest.
  * with its rounding points off the restatement is fp64 autograd of softmax(Q K^T scale + mask) V to 1e-12 on O, dQ, dK, dV -- every
    mask kind; the fused mode through an fp64 RMSNorm + RoPE, both norm_flags values, shared and per-sample RoPE tables;
  * BARS: exactly 2 x the reference's own fp32 noise (keys reversed / permuted, P and dS rounded at a shifted reference), measured here on
    the GPU tests' case lists, rounded up, at least one ulp;
  * select data give the exact outputs bit for bit under the fp32 restatement in every key order, and the 160-unit gap holds in fp64;
  * every spike case reaches the regimes it was built for, and every regime is reached at the tile widths and vote units of all three forward
    kernels -- the condition that keeps the GPU test from passing without touching the rescale path;
  * the case lists hold every value of the argument space the issue names."""
import math

import pytest
import torch

import attn_ref as A
import rowkernel_ref as RK

BF, F64, F32 = torch.bfloat16, torch.float64, torch.float32
TOL = 1e-12
# (key tile, rows per vote): attn_fwd_kernel votes per 32-query wave over 64-key tiles; the skewed 64-query kernel votes per 32-query
# block of its wave over 64-key tiles, its pipelined form per 32-query block over 32-key sub-tiles.  (64, 64) / (32, 64), a vote of the
# whole 64-query wave, are not what the kernels do and stay as further units the regimes must survive.
WIDTHS = ((64, 32), (32, 32), (64, 64), (32, 64))
DH128_ONLY = ((32, 32), (64, 64), (32, 64))      # the units of the 64-query kernels, which take dh = 128 only


def close(a, b):
    return (a.double() - b.double()).abs().max().item() <= TOL * max(1.0, b.double().abs().max().item())


def _autograd(inp, case, q, k):
    """fp64 autograd of the joint SDPA on q, k [B, S, H, dh] (leaves or functions of leaves): (O, dV) and the backward already run."""
    v = inp["v"].double().requires_grad_()
    s = (q.permute(0, 2, 1, 3) @ k.permute(0, 2, 3, 1)) * float(torch.tensor(case.scale, dtype=F32))
    if inp["mask"] is not None:
        s = s + inp["mask"].double()[:, None, None, :]
    o = (torch.softmax(s, -1) @ v.permute(0, 2, 1, 3)).permute(0, 2, 1, 3)
    o.backward(inp["dO"].double())
    return o.detach(), v.grad


@pytest.mark.parametrize("mask", A.MASKS)
def test_without_rounding_the_restatement_is_autograd(mask):
    case = A.Case(137, H=2, B=2, dh=64, mask=mask)
    inp = A.make_inputs(case)
    q, k = inp["q"].double().requires_grad_(), inp["k"].double().requires_grad_()
    o, dv = _autograd(inp, case, q, k)
    for flip in (False, "perm"):
        fwd = A.attn_fwd_ref(inp, case, rnd=False, flip=flip)
        bwd = A.attn_bwd_ref(inp, case, fwd["O"][0], fwd["lse2"][0], rnd=False, flip=flip)
        assert close(fwd["O"][0], o) and close(bwd["dQ"][0], q.grad) and close(bwd["dK"][0], k.grad) and close(bwd["dV"][0], dv)
        assert close(bwd["dsum"][0], (inp["dO"].double() * o).sum(-1).permute(0, 2, 1))
    # lse2 is the log2-domain logsumexp
    s2 = A.scores2(inp, case)
    assert close(fwd["lse2"][0], torch.logsumexp(s2 * math.log(2.0), -1) / math.log(2.0))


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("rope_b", [False, True])
def test_fused_mode_is_autograd_through_rmsnorm_and_rope(flags, rope_b):
    case = A.Case(70, H=2, B=2, dh=64, mask="finite", fused=True, flags=flags, rope_b=rope_b, T=32)
    inp = A.make_inputs(case)
    x = inp["saved"].double().requires_grad_()
    rot = RK.qk_fwd(x, inp["rope"], inp["ws"], case.T, case.H, case.dh, flags, A.NORM_EPS, rnd=False)["out"][0]      # [B, S, 2, H, dh]
    inp = dict(inp, q=rot[:, :, 0].detach(), k=rot[:, :, 1].detach())
    o, dv = _autograd(inp, case, rot[:, :, 0], rot[:, :, 1])
    fwd = A.attn_fwd_ref(inp, case, rnd=False)
    bwd = A.attn_bwd_ref(inp, case, fwd["O"][0], fwd["lse2"][0], rnd=False)
    g = A._qk_view(x.grad, case.H, case.dh)
    assert close(bwd["dQ"][0], g[:, :, 0]) and close(bwd["dK"][0], g[:, :, 1]) and close(bwd["dV"][0], dv)


def test_part_ref_is_a_per_head_projection_with_the_text_rows_on_their_own_weights():
    case = A.Case(40, H=3, B=2, dh=64, fused=True, T=16, R=16)
    inp = A.make_inputs(case)
    X = inp["v"]
    val, sc = A.part_ref(X, inp, case, 2)
    (ihi, ilo), (thi, tlo) = inp["W"][2]
    for h in range(3):
        cols = slice(h * 64, (h + 1) * 64)
        xh = X[:, :, h].double()
        wi, wt = (ihi.double() + ilo.double())[:, cols], (thi.double() + tlo.double())[:, cols]
        want = torch.cat([torch.cat([xh[b, :16] @ wt.t(), xh[b, 16:] @ wi.t()]) for b in range(2)])
        assert close(val[h], want)
    for flip in (False, True, "perm"):      # the fp32 evaluation is the same projection, within the bar its own noise sets
        assert A.err_ulps32(A.part_ref(X, inp, case, 2, F32, flip)[0], val, sc) <= A.BARS["part"], flip
    assert A.part_rows(A.replace(case, no_txt=True), 1).view(2, 40)[:, :16].sum() == 0 and A.part_rows(A.replace(case, no_img=True), 1).sum() == 32


def test_bars_are_twice_the_reference_noise():
    floors = A.measure_floors()
    assert set(floors) == set(A.BARS), set(floors) ^ set(A.BARS)
    for k, f in sorted(floors.items()):
        print(f"{k:10s} floor {f:.3g} ulps, bar {A.BARS[k]}")
    for k, f in sorted(floors.items()):
        assert A.BARS[k] == int(A.BARS[k]) and A.BARS[k] >= 1
        assert 2 * f <= A.BARS[k], (k, f, A.BARS[k])
        assert A.BARS[k] == max(1, math.ceil(2 * f)), (k, f, "the bar is 2 x floor rounded up, no more")


@pytest.mark.parametrize("idx", range(len(A.SELECT_CASES)))
def test_select_data_are_exact_in_every_key_order(idx):
    case = A.SELECT_CASES[idx]
    inp = A.make_inputs(case)
    # the gap, in fp64: the selected score exceeds every other by at least SELECT_GAP units
    s2 = A.scores2(inp, case)
    top = s2.gather(-1, inp["sel"][:, None, :, None].expand(case.B, case.H, case.S, 1))
    rest = s2.scatter(-1, inp["sel"][:, None, :, None].expand(case.B, case.H, case.S, 1), A.NEG_INF)
    assert (top.squeeze(-1) - rest.amax(-1) >= A.SELECT_GAP).all(), (top.squeeze(-1) - rest.amax(-1)).min().item()
    assert inp["mask"] is None or torch.isfinite(inp["mask"].gather(1, inp["sel"])).all()
    O, dV, dsum = A.select_expected(inp, case)
    fwd, bwd, O_in, lse_in = A.reference(inp, case)
    assert torch.equal(fwd["O"][0], O) and torch.equal(bwd["dV"][0], dV) and torch.equal(bwd["dsum"][0], dsum)
    assert torch.equal(O, O.to(BF).double()) and torch.equal(dV, dV.to(BF).double())
    for flip in (False, True, "perm"):
        f32 = A.attn_fwd_ref(inp, case, F32, flip)      # P rounded at the row maximum: a lazy reference cannot lag 160 units behind
        assert torch.equal(f32["O"][0].double(), O), flip
        b32 = A.attn_bwd_ref(inp, case, O_in, lse_in, F32, flip)
        assert torch.equal(b32["dV"][0].double(), dV) and torch.equal(b32["dsum"][0].double(), dsum), flip
        assert not b32["dQ"][0].any() and not b32["dK"][0].any(), flip
        if case.R:
            for slot in (0, 3):
                X = A.slot_x(slot, fwd, bwd)
                if slot in case.slots and (slot == 0 or case.fused):
                    assert torch.equal(A.part_ref(X, inp, case, slot, F32, flip)[0].double(), A.part_ref(X, inp, case, slot)[0]), (slot, flip)


def test_select_cases_select_late_keys_in_every_tile():
    """Every 64-key tile that holds an unmasked key holds a selected one, and a query of the first rows selects a key of a later tile."""
    for case in A.SELECT_CASES:
        inp = A.make_inputs(case)
        for b in range(case.B):
            live = torch.ones(case.S, dtype=torch.bool) if inp["mask"] is None else torch.isfinite(inp["mask"][b])
            assert {int(j) // 64 for j in inp["sel"][b]} == {int(j) // 64 for j in torch.nonzero(live).flatten()}, case
            assert not live[64:].any() or (inp["sel"][b][:64] >= 64).any(), case
    assert any(c.mask in ("head", "tile", "tail") for c in A.SELECT_CASES)


@pytest.mark.parametrize("idx", range(len(A.SPIKE_CASES)))
def test_spike_case_reaches_its_regimes(idx):
    case = A.SPIKE_CASES[idx]
    inp = A.make_inputs(case)
    for tile, wave in WIDTHS:
        got = A.regimes(inp, case, tile, wave)
        assert set(case.expect) <= got, (case, tile, wave, got)


def test_every_regime_is_reached_at_every_width_and_rand_data_reach_none():
    for tile, wave in WIDTHS:
        got = set()
        for case in A.SPIKE_CASES:
            if case.dh == 128 or (tile, wave) not in DH128_ONLY:
                got |= A.regimes(A.make_inputs(case), case, tile, wave)
        assert got == set(A.REGIMES), (tile, wave, set(A.REGIMES) - got)
    # the premise of the issue: on randn data the reference never moves after tile 0
    for case in A.RAND_CASES:
        if case.mask in ("none", "tail"):
            assert not A.regimes(A.make_inputs(case), case) & {"rescale", "staircase"}, case


def test_case_lists_hold_the_argument_space():
    for fam in (A.RAND_CASES, A.SELECT_CASES):
        assert {c.S for c in fam} == set(A.SHAPES) and {c.H for c in fam} == {1, 2, 3} and {c.B for c in fam} == {1, 2}
        assert {c.mask for c in fam} == set(A.MASKS) and {c.dh for c in fam} == {64, 128}
        fused = [c for c in fam if c.fused]
        assert {c.flags for c in fused} == {0, 1} and {c.rope_b for c in fused} == {False, True}
        assert {c.T for c in fused} >= {0, 16, 48} and any(c.T == c.S // 16 * 16 and c.T > 48 for c in fused)
        lora = [c for c in fam if c.R]
        assert {c.R for c in lora} == {16, 32} and any(c.c0 == 4 and c.ld_part == c.R + 4 for c in lora) and any(c.ld_part > c.R + c.c0 for c in lora)
        assert any(c.no_img and 0 < c.T < c.S for c in lora) and any(len(c.slots) < 4 for c in lora)
        # a missing text adapter is only seen where text rows exist: on the one-pass line, on a 64-query line, in plain forward mode
        assert all(0 < c.T < c.S for c in lora if c.no_txt)
        assert any(c.no_txt and c.fused and c.onepass() for c in lora) and any(c.no_txt and not c.fused and c.dh == 128 for c in lora)
        assert all(c.ld_part > c.R + c.c0 or c.c0 for c in lora) and all(c.ld_part >= c.R + 4 for c in lora)
        assert any(0 < c.T < c.S and c.fused for c in lora)                       # a 16-row fragment on either side of T
        assert {c.slice_ for c in fam} == {False, True} and {c.narrow for c in fam} == {False, True}
        for line_ok in (lambda c: c.dh == 128, lambda c: c.onepass(), lambda c: c.dh == 64):
            assert any(line_ok(c) and c.fused for c in fam) and any(line_ok(c) and not c.fused for c in fam)
    assert all(c.kind == "spike" and c.plant and c.expect for c in A.SPIKE_CASES)
    assert any(c.fused for c in A.SPIKE_CASES) and any(not c.fused for c in A.SPIKE_CASES) and any(c.onepass() for c in A.SPIKE_CASES)
    assert any(c.no_txt and c.fused and c.onepass() and 0 < c.T < c.S for c in A.SPIKE_CASES)
    assert all(c.S <= 577 and c.B * c.H <= 6 for fam in A.ALL_FAMILIES.values() for c in fam)
