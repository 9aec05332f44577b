"""CPU: tests/ln_down_ref.py is right, and the bars of tests/test_ln_down_gpu.py are honest.
  * BAR_Y is 2 x the fp32-reversed-order noise of rowkernel_ref.ln_fwd on this file's case list, BAR_U is 2 x the noise of the fp32
    restatement of the contraction plus what the bf16 hi / lo split cannot carry; the restatement itself passes with half the bar;
  * the exactness premise of the `exact` data: range arithmetic, three summation orders, and every case of the list;
  * ln_down with its roundings switched off is layer_norm * (1 + scale) + shift followed by an fp64 matmul; the images obey include/qfx.h;
  * the case list holds every value of every axis and runs every arm; gate_mul against a loop."""
import math

import torch
import torch.nn.functional as F

import ln_down_ref as LD
import rowkernel_ref as R
import skinny_ref as S

BF, F64, F32 = torch.bfloat16, torch.float64, torch.float32
_FLOORS = []


def floors():
    if not _FLOORS:
        _FLOORS.append(LD.measure_floors())
    return _FLOORS[0]


# ------------------------------------------------------------------------------------------------ where the tolerances come from
def test_y_bar_is_twice_the_reference_noise_on_this_case_list():
    (fy, where), _ = floors()
    print(f"ln_down.y floor {fy:.3g} ulps at {where}, bar {LD.BAR_Y}; rowkernel_ref's ln_fwd.y bar {R.BARS['ln_fwd.y']}")
    assert LD.BAR_Y == int(LD.BAR_Y) and LD.BAR_Y >= 1
    assert 2 * fy <= LD.BAR_Y and LD.BAR_Y == max(1, math.ceil(2 * fy)), (fy, "the bar is 2 x floor rounded up, no more")
    # the expectation was rowkernel_ref's ln_fwd.y bar of 2 (floor 1.00); this case list (modulation of scale 0.3, x of scale 2, rows up to
    # 33) holds a draw whose flipped bf16(LN) is stretched by t1 > 1 into two ulps, see the comment at ln_down_ref.BAR_Y
    assert R.BARS["ln_fwd.y"] == 2 and 1.5 < fy <= 2.0 and LD.BAR_Y == 4
    assert LD.FLOOR_DRAWS == R.FLOOR_DRAWS


def test_u_bar_is_twice_the_reference_noise_plus_the_split():
    _, (fu, where) = floors()
    print(f"ln_down.U floor {fu:.3g} of max |U| at {where}, U_FLOOR {LD.U_FLOOR}, bar {LD.BAR_U:.4g}")
    assert fu <= LD.U_FLOOR <= 2 * fu, (fu, "U_FLOOR is the measured floor, rounded up, no more")
    assert LD.BAR_U == 2 * LD.U_FLOOR + 2.0 ** -16
    # the restatement itself (fp32, reversed order, split into bf16 hi + lo) passes with half the bar: its fp32 error is at most the floor,
    # and hi + lo misses an fp32 u by at most 2^-17 |u| (lo = bf16 of a residue below 2^-8 |u|, rounded to 2^-9 of itself)
    worst = 0.0
    for case in LD.CASES:
        inp = LD.make(case, "rand")
        r64 = LD.case_ref(inp, case)
        hi, lo = S.split(LD.contract32(r64["y"][0].to(BF), inp["W_hi"], inp["W_lo"]))
        worst = max(worst, LD.rel_u(hi.double() + lo.double(), r64["U"]))
    print(f"hi + lo of the fp32 restatement: {worst:.4g} of max |U|")
    assert worst <= LD.BAR_U / 2
    assert worst > LD.U_FLOOR           # the split term is what the bar is made of: a bar of 2 x floor alone would refuse the restatement


# ------------------------------------------------------------------------------------------------ the exactness premise
def _sums_exact(y, hi, lo):
    """fp32 sums of the hi and lo products over k -- forward, reversed, and split over 8 waves as the kernel splits k (wave w takes the
    32-column k-steps w, w + 8, ...; the wave sums are added in wave order) -- all give the bits of the fp64 sum."""
    want = y.double() @ (hi.double() + lo.double()).t()
    assert torch.equal(want.float().double(), want)
    th, tl = y.float()[:, None, :] * hi.float()[None], y.float()[:, None, :] * lo.float()[None]        # [rows, R, K], exact products
    K = y.shape[1]

    def seq(order):
        acc = torch.zeros(y.shape[0], hi.shape[0])
        for k in order:
            acc = acc + th[..., k]
            acc = acc + tl[..., k]
        return acc
    fwd, rev = seq(range(K)), seq(range(K - 1, -1, -1))
    waves = torch.zeros(y.shape[0], hi.shape[0])
    for w in range(8):
        waves = waves + seq([ks * 32 + c for ks in range(w, K // 32, 8) for c in range(32)])
    return all(torch.equal(v.double(), want) for v in (fwd, rev, waves, LD.contract32(y, hi, lo)))


def test_exact_data_premise_holds_at_the_widest_row():
    D = LD.EXACT_MAX_D
    assert max(LD.ALL_D) == D and max(c.D for c in LD.CASES) == D
    assert max(D for Dp, _, _ in LD.TWO_PROBLEM_CASES for D in Dp) <= D and max(D for D, _ in LD.MX_CASES) <= D
    # worst-case magnitude x granularity: |y| < 128 in multiples of 2^-1, |W_hi| + |W_lo| <= 1 in multiples of 2^-4
    y_max = LD.EXACT_Y_MAX - LD.EXACT_Y_GRAN
    gran = LD.EXACT_Y_GRAN * LD.EXACT_W_GRAN
    assert D * y_max * LD.EXACT_W_MAX / gran < 2 ** 24
    # the shift range keeps y inside [64, 128) for any |p| <= EXACT_P_MAX (p itself rounds to a multiple of 2^-1 or is absorbed)
    assert 80 - LD.EXACT_P_MAX - 1 >= LD.EXACT_Y_MIN and 111 + LD.EXACT_P_MAX + 1 < LD.EXACT_Y_MAX
    # on data: the extreme row (every product at its largest magnitude, one sign) and random rows of the exact value ranges
    g = torch.Generator().manual_seed(3)
    y = (torch.randint(128, 256, (6, D), generator=g).float() * 0.5 * (torch.randint(0, 2, (6, D), generator=g).float() * 2 - 1)).to(BF)
    y[0] = y_max
    hi = (torch.randint(-14, 15, (16, D), generator=g).float() * LD.EXACT_W_GRAN).to(BF)
    lo = (torch.randint(-2, 3, (16, D), generator=g).float() * LD.EXACT_W_GRAN).to(BF)
    hi[0], lo[0] = 14 * LD.EXACT_W_GRAN, 2 * LD.EXACT_W_GRAN
    assert (y.float().abs() >= LD.EXACT_Y_MIN).all() and (y.float().abs() < LD.EXACT_Y_MAX).all()
    assert _sums_exact(y, hi, lo)
    assert (y[0].double() @ (hi[0].double() + lo[0].double())).item() == D * y_max


def test_exact_cases_keep_the_premise_and_the_restatement_is_exact_on_them():
    for case in LD.CASES + [LD.REPRO_CASE]:
        inp = LD.make(case, "exact")
        for t, unit, top in ((inp["W_hi"], LD.EXACT_W_GRAN, 14), (inp["W_lo"], LD.EXACT_W_GRAN, 2)):
            v = t.double() / unit
            assert (v == v.round()).all() and v.abs().max() <= top
        assert ((inp["W_hi"].double().abs() + inp["W_lo"].double().abs()) <= LD.EXACT_W_MAX).all()
        shift, scale = LD.mod_of(inp, case)
        assert (shift.double().abs() >= 80).all() and (shift.double().abs() <= 111).all() and (shift.double() == shift.double().round()).all()
        ref = LD.case_ref(inp, case)
        y, sc = ref["y"]
        # y - shift is p = bf16(LN * t1) up to the last rounding (half of 2^-1)
        b = torch.arange(case.rows) // LD.rpb_of(case) if shift.shape[0] > 1 else torch.zeros(case.rows, dtype=torch.int64)
        p = y - shift.double()[b]
        assert p.abs().max() <= LD.EXACT_P_MAX, (case, p.abs().max())
        assert (y.abs() >= LD.EXACT_Y_MIN).all() and (y.abs() < LD.EXACT_Y_MAX).all() and ((y / LD.EXACT_Y_GRAN) == (y / LD.EXACT_Y_GRAN).round()).all()
        r32 = LD.case_ref(inp, case, dt=F32, flip=True, y=y.to(BF))
        assert torch.equal(r32["U"].double(), ref["U"]), case


# ------------------------------------------------------------------------------------------------ the restatement
def test_ln_down_without_rounding_is_layer_norm_modulate_matmul():
    case = LD.Case(256, 32, 7, 3, "six", "tight", True, "ET")
    inp = LD.make(case, "rand")
    shift, scale = LD.mod_of(inp, case)
    got = LD.ln_down(inp["x"], shift, scale, 3, inp["W_hi"], inp["W_lo"], rnd=False)
    b = torch.arange(7) // 3
    eps = float(torch.tensor(LD.EPS, dtype=F32))
    want = F.layer_norm(inp["x"].double(), (256,), eps=eps) * (1 + scale.double()[b]) + shift.double()[b]
    assert (got["y"][0] - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    wu = want @ (inp["W_hi"].double() + inp["W_lo"].double()).t()
    assert (got["U"] - wu).abs().max().item() <= 1e-12 * wu.abs().max().item()
    # with the roundings: y is ln_fwd's, bit for bit, and a given y replaces it in the contraction
    r = LD.case_ref(inp, case)
    ry = R.ln_fwd(inp["x"], shift, scale, 3)["y"]
    assert torch.equal(r["y"][0], ry[0]) and torch.equal(r["y"][1], ry[1])
    assert torch.equal(r["U"], S.down_ref(ry[0].to(BF), inp["W_hi"], inp["W_lo"], torch.arange(7)))
    other = R.randn_bf(torch.Generator().manual_seed(1), 7, 256)
    assert torch.equal(LD.case_ref(inp, case, y=other)["U"], S.down_ref(other, inp["W_hi"], inp["W_lo"], torch.arange(7)))
    assert "U" not in LD.ln_down(inp["x"], shift, scale, 3)            # a plain problem: y alone


def test_images_obey_the_header_layout_for_groups_narrower_than_R():
    case = LD.Case(256, 48, 5, 3, "tight", "tight", True, "ET")
    gR, gs, ld_ext = LD.group_of(case)
    assert (gR, gs) == (16, 64) and ld_ext == 2 * 64 + 48 + 11
    inp = LD.make(case, "rand")
    r = LD.case_ref(inp, case, ld_ut=case.rows + 9)
    U32 = r["U"].float()
    hi, lo = S.split(U32)
    written = torch.zeros(case.rows, ld_ext, dtype=torch.bool)
    for m in range(case.rows):
        for j in range(case.R):
            c = (j // gR) * gs + j % gR                     # include/qfx.h: group j / group_R at group_stride, [hi | lo | hi] of group_R each
            assert S.bits(r["ext"])[m, c] == S.bits(hi)[m, j] == S.bits(r["ext"])[m, c + 2 * gR] and S.bits(r["ext"])[m, c + gR] == S.bits(lo)[m, j]
            assert S.bits(r["Ut_hi"])[j, m] == S.bits(hi)[m, j] and S.bits(r["Ut_lo"])[j, m] == S.bits(lo)[m, j]
            written[m, c] = written[m, c + gR] = written[m, c + 2 * gR] = True
    assert (S.bits(r["ext"])[~written] == S.CANARY_BF16).all() and written.sum() == 3 * case.rows * case.R
    assert (S.bits(r["Ut_hi"])[:, case.rows:] == S.CANARY_BF16).all() and (S.bits(r["Ut_lo"])[:, case.rows:] == S.CANARY_BF16).all()
    ch, cl, ch2 = LD.ext_columns(case.R, gR, gs)
    assert torch.equal(S.bits(r["ext"][:, ch]), S.bits(hi)) and torch.equal(S.bits(r["ext"][:, cl]), S.bits(lo)) and torch.equal(S.bits(r["ext"][:, ch2]), S.bits(hi))
    for Rr in LD.ALL_R:                                      # one group: [hi | lo | hi] of R columns
        ch, cl, ch2 = LD.ext_columns(Rr, Rr, 0)
        assert ch.tolist() == list(range(Rr)) and cl.tolist() == list(range(Rr, 2 * Rr)) and ch2.tolist() == list(range(2 * Rr, 3 * Rr))


def test_contract32_is_a_second_order_of_the_same_sum():
    case = LD.CASES[7]
    inp = LD.make(case, "rand")
    y = LD.case_ref(inp, case)["y"][0].to(BF)
    U64 = S.down_ref(y, inp["W_hi"], inp["W_lo"], torch.arange(case.rows))
    a, b = LD.contract32(y, inp["W_hi"], inp["W_lo"], flip=True), LD.contract32(y, inp["W_hi"], inp["W_lo"], flip=False)
    assert a.dtype == F32 and LD.rel_u(a, U64) < 1e-6 and LD.rel_u(b, U64) < 1e-6 and not torch.equal(a, b)


def test_gate_mul_restatement_matches_the_loop():
    g = torch.Generator().manual_seed(2)
    dx, gate = R.randn_bf(g, 5, 8), R.randn_bf(g, 3, 8)
    got = LD.gate_mul(dx, gate, 2)
    for m in range(5):
        for k in range(8):
            want = torch.tensor(float(dx[m, k]) * float(gate[m // 2, k])).to(BF)          # the fp32 product is exact: one rounding
            assert S.bits(got)[m, k] == S.bits(want)
    assert torch.equal(S.bits(LD.gate_mul(dx, gate[:1], 2)), S.bits((dx.float() * gate[:1].float()).to(BF)))


# ------------------------------------------------------------------------------------------------ the case lists reach every path
def test_case_list_holds_every_axis_value_and_every_arm():
    cs = LD.CASES
    assert 36 <= len(cs) <= 44 and len(set(cs)) == len(cs)
    for name, vals in (("D", LD.ALL_D), ("R", LD.ALL_R), ("rows", LD.ALL_ROWS), ("rpb", LD.ALL_RPB), ("stride", LD.ALL_STRIDES),
                       ("weights", LD.ALL_WEIGHTS), ("outs", LD.ALL_OUTS), ("grouped", (True, False))):
        assert {getattr(c, name) for c in cs} == set(vals), name
    assert LD.ALL_D == tuple(256 * k for k in range(1, 13)) and all(c.rows <= 49 and c.D <= 3072 for c in cs)
    run = set().union(*(LD.arms(c) for c in cs))
    assert run >= {"NF1", "NF2", "NF3", "frag", "rowmajor", "ldw_tight", "ldw_wide", "ring_partly_filled", "ring_full_no_refill", "ring_refilled",
                   "grouped", "one_group", "sample_changes_inside_a_block", "dead_lanes"} | {f"ksteps{k}" for k in range(1, 13)}
    # every instantiation meets every state of the weight ring, every weight layout, every output set, both group forms, every row tail
    for Rr in LD.ALL_R:
        mine = [c for c in cs if c.R == Rr]
        assert {a for c in mine for a in LD.arms(c) if a.startswith("ring_")} == {"ring_partly_filled", "ring_full_no_refill", "ring_refilled"}, Rr
        assert {c.weights for c in mine} == set(LD.ALL_WEIGHTS) and {c.outs for c in mine} == set(LD.ALL_OUTS) and {c.rows for c in mine} == set(LD.ALL_ROWS)
        assert {c.grouped for c in mine} == {True, False}
    assert {c.outs for c in cs if c.R == 32 and c.grouped} >= {"ET", "E"}           # group_R < R for R = 32, with ext written
    # both load arms at every number of k-steps; the refill guard changes arm inside the loop at 4 .. 11 k-steps
    assert {(c.weights == "frag", c.D // 256) for c in cs} == {(f, k) for f in (True, False) for k in range(1, 13)}
    # rows = 1 (fifteen dead lanes re-read row 0) with every NF; a sample boundary inside a block with every row count that has one
    assert {c.R for c in cs if c.rows == 1} == set(LD.ALL_R)
    assert {c.rows for c in cs if "sample_changes_inside_a_block" in LD.arms(c)} == {15, 16, 17, 33}
    assert {c.stride for c in cs if "sample_changes_inside_a_block" in LD.arms(c)} == set(LD.ALL_STRIDES)
    # the launches with two problems, the MX-FP8 image, gate_mul
    pairs = {tuple(a for _, a in pair) for _, _, pair in LD.TWO_PROBLEM_CASES}
    assert pairs == {(True, False), (False, True), (True, True)} and {Rr for _, Rr, _ in LD.TWO_PROBLEM_CASES} == {16, 48}
    assert any(pair[0][0] % 16 for _, _, pair in LD.TWO_PROBLEM_CASES)               # start[1] is no multiple of what a full first problem gives
    assert {D for D, _ in LD.MX_CASES} == {256, 1280, 3072} and {r for _, r in LD.MX_CASES} == {17, 33} and LD.MX_RPB == 3
    assert LD.REPRO_CASE[:3] == (3072, 48, 33)
    big = LD.GATE_CASES[-1]
    assert LD.GATE_GRID_ELEMS < big[0] * big[1] < LD.GATE_GRID_ELEMS + 256 * 8 * 16 and (big[0] * big[1]) % (256 * 8)
    assert set(LD.GATE_CASES[:3]) == {(1, 8, 1, "shared"), (7, 520, 3, "tight"), (5, 3072, 2, "six")}
