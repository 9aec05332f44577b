"""CPU restatement and case lists of the fused LayerNorm+modulate forward + rank-r down projection (ln_down_kernel<NF> of
csrc/qfx_skinny.hip, entered through qfx_ln_down_fwd) and of qfx_gate_mul: the yardstick of tests/test_ln_down_gpu.py.

Nothing here is a second statement of something the suite already has: y comes from rowkernel_ref.ln_fwd (its rounding points, `flip`
and `dt`), the fp64 contraction from skinny_ref.down_ref, the images from skinny_ref.ext_image / ut_image.  What this file adds:

  * ln_down(): y exactly as ln_fwd gives it; U64 = y (W_hi + W_lo)^T of a GIVEN bf16 y (the GPU tests pass the kernel's own y bits, so
    the LayerNorm half and the contraction half are judged apart); the three images the kernel writes from fp32(U).  The kernel has no
    fp32 U output: U is only observable as hi + lo.
  * contract32(): the same contraction in fp32 in a second order (reversed k, 64-term chains, explicit elementwise adds: the same bits on
    every machine) -- the reference's own noise, from which the bar of hi + lo is taken.
  * the case list: a latin-square walk over the axes the kernel's paths are selected by, with arms(case) naming which case runs which arm.

Two kinds of data.
  rand:  x Gaussian bf16 of scale 2, modulation of scale 0.3, W the bf16 split of a Gaussian fp32 matrix of scale 0.05.
  exact: shift = +-(80 + integer in [0, 31]) and scale clamped to [-1, 1], so p = bf16(LN(x) * bf16(1 + scale)) stays below 16 in
         magnitude (asserted on the data by tests/test_ln_down_ref_cpu.py) and every y = bf16(p + shift) lies in 64 <= |y| < 128, where
         bf16 is spaced 2^-1: y is a multiple of 2^-1 below 128 WHATEVER the fp32 noise of the row statistics does to p (the GPU test
         asserts this of the kernel's own y).  W_hi = integers in [-14, 14] times 2^-4, W_lo = integers in [-2, 2] times 2^-4: the products
         are multiples of 2^-5, and any partial sum of the hi and lo products of D <= 3072 columns is at most 3072 * 127.5 * 1 = 391680
         = 12.5 M granules < 2^24: every fp32 partial sum is exact in every order, the kernel must give the fp64 sum bit for bit.

Bars (tests/test_ln_down_ref_cpu.py derives and asserts them; none is taken from what the kernel gives):
  BAR_Y  bf16 ulps of ln_fwd's `scale`: 2 x the fp32-reversed-order floor of ln_fwd on THIS case list, rounded up, at least 1.  One flipped
         rounding of bf16(LN) is one ulp of LN, but t1 = bf16(1 + scale) > 1 stretches it before p is rounded again: the floor here is 2.
  BAR_U  |hi + lo - U64| / max |U64| on rand data: 2 x U_FLOOR + 2^-16.  U_FLOOR is contract32 against fp64 on this case list; 2^-16 is what
         the bf16 hi / lo split cannot carry (lo's rounding is at most 2^-9 of a value <= 2^-8 |U|, doubled)."""
from __future__ import annotations

import collections

import torch

import rowkernel_ref as R
import skinny_ref as S

BF, F64, F32 = torch.bfloat16, torch.float64, torch.float32
EPS = R.EPS

# floor 2.00 ulps, not the 1.00 that rowkernel_ref.BARS["ln_fwd.y"] = 2 rests on: draw 1 of the (D = 1024, rows = 17, shared) case holds a
# LN value within 4e-7 of a bf16 tie (1.39453136); the flipped bf16(LN) times t1 = 1.34 moves p by 1.34 ulps, which round to 2, and y with it
BAR_Y = 4
U_FLOOR = 3.1e-7                        # measured 3.03e-7 (D = 2560, rows = 33, R = 32)
BAR_U = 2 * U_FLOOR + 2.0 ** -16        # 1.588e-5
FLOOR_DRAWS = R.FLOOR_DRAWS

# exact data: the value ranges the premise is proven for
EXACT_Y_MIN, EXACT_Y_MAX, EXACT_Y_GRAN = 64.0, 128.0, 0.5
EXACT_P_MAX = 15.0                      # |p| <= 15 < 16 = 80 - 64 = 128 - 112: p + shift cannot leave [64, 128)
EXACT_W_GRAN, EXACT_W_MAX = 2.0 ** -4, 1.0
EXACT_MAX_D = 3072

# ---------------------------------------------------------------------------------------------- the case lists
Case = collections.namedtuple("Case", "D R rows rpb stride weights grouped outs")
ALL_D = tuple(range(256, 3073, 256))    # 1 .. 12 k-steps per wave
ALL_R = (16, 32, 48)                    # ln_down_kernel<1>, <2>, <3>
ALL_ROWS = (1, 15, 16, 17, 33)          # one lane live; a dead last lane; a full block; one row into a second block; into a third
ALL_RPB = (3, 16, "rows")               # samples change inside a block; per block; one sample
ALL_STRIDES = R.LN_STRIDES              # mod_bstride 0, D, 6 D
ALL_WEIGHTS = ("tight", "wide", "frag") # row-major ldw = D; row-major ldw = D + 8; the fragment image W_fr
ALL_OUTS = ("ET", "E", "T")             # ext + Ut, ext only, Ut only
GROUP_R, GROUP_STRIDE = 16, 64          # the grouped form: group_R = 16 < R, group_stride = 64


def _walk():
    out = []
    for i, D in enumerate(ALL_D):
        for j in range(3):
            out.append(Case(D, ALL_R[(i + j) % 3], ALL_ROWS[(2 * i + j) % 5], ALL_RPB[(i + 2 * j) % 3], ALL_STRIDES[(i // 3 + j) % 3],
                            ALL_WEIGHTS[(i + i // 3 + 2 * j) % 3], (i + i // 2 + j) % 2 == 1, ALL_OUTS[(i // 2 + j) % 3]))
    # what the walk leaves out: the grouped form with R = 32 under both output sets that hold ext, rows = 1 with a partly filled ring
    # and every NF, the widest rows with the fragment image
    out += [Case(512, 32, 1, 3, "six", "frag", True, "ET"), Case(256, 48, 1, "rows", "shared", "wide", True, "E"),
            Case(512, 16, 1, 16, "tight", "tight", False, "T"), Case(3072, 32, 33, 3, "six", "frag", True, "E")]
    return out


CASES = _walk()
KINDS = ("exact", "rand")

# (D, R, [(rows, adapted) of problem 0, of problem 1]): every order of adapted and plain problems, a first problem with rows % 16 != 0
TWO_PROBLEM_CASES = [(Dp, Rr, pair) for Rr, Dp in ((16, (1280, 512)), (48, (768, 3072)))
                     for pair in (((17, True), (5, False)), ((33, False), (16, True)), ((15, True), (49, True)))]
MX_CASES = [(D, rows) for D in (256, 1280, 3072) for rows in (17, 33)]       # the MX-FP8 image of y beside adapted rows
MX_RPB, MX_LDYQ_EXTRA, MX_YS_ROWS_EXTRA = 3, 16, 5
REPRO_CASE = Case(3072, 48, 33, 3, "six", "frag", True, "ET")
# (rows, D, rpb, gate stride kind): the last one is just past what the capped grid of 4096 blocks x 256 threads x 8 elements covers
GATE_CASES = [(1, 8, 1, "shared"), (7, 520, 3, "tight"), (5, 3072, 2, "six"), (2731, 3080, 1000, "tight")]
GATE_GRID_ELEMS = 4096 * 256 * 8


def rpb_of(case):
    return case.rows if case.rpb == "rows" else case.rpb


def group_of(case):
    """(group_R, group_stride, ld_ext): 11 spare columns behind the last group's [hi | lo | hi]."""
    gR, gs = (GROUP_R, GROUP_STRIDE) if case.grouped else (case.R, 0)
    return gR, gs, (case.R // gR - 1) * gs + 3 * gR + 11


def arms(case):
    """The arms of ln_down_kernel and of its host code that one n = 1 launch of `case` runs."""
    ks = case.D // 256                                       # k-steps of every wave
    a = {f"NF{case.R // 16}", f"ksteps{ks}", "frag" if case.weights == "frag" else "rowmajor", f"ldw_{case.weights}",
         "ring_partly_filled" if ks < 3 else "ring_full_no_refill" if ks == 3 else "ring_refilled",
         f"rows{case.rows}", f"stride_{case.stride}", f"outs_{case.outs}", "grouped" if case.grouped and case.R > GROUP_R else "one_group"}
    if rpb_of(case) < min(16, case.rows):
        a.add("sample_changes_inside_a_block")
    if case.rows % 16:
        a.add("dead_lanes")
    return a


# ---------------------------------------------------------------------------------------------- data
def make(case, kind, salt=0):
    """CPU inputs of one case (draw rowkernel_ref._DRAW): x [rows, D], mod [B, 6 D] (shift, scale, gate, ... sections), W_hi, W_lo [R, D].
    salt: other data for the same shape (the second problem of a launch)."""
    idx = CASES.index(case) if case in CASES else 900 + case.D // 256 + case.rows
    g = R._gen(77000 + 13 * idx + (0 if kind == "rand" else 5) + 1009 * salt)
    B = (case.rows + rpb_of(case) - 1) // rpb_of(case)
    D = case.D
    x = R.randn_bf(g, case.rows, D, scale=2.0)
    mod = R.randn_bf(g, B, 6 * D, scale=0.3)
    if kind == "exact":
        sign = torch.randint(0, 2, (B, D), generator=g).float() * 2 - 1
        mod[:, :D] = (sign * (80 + torch.randint(0, 32, (B, D), generator=g).float())).to(BF)
        mod[:, D:2 * D] = mod[:, D:2 * D].float().clamp(-1.0, 1.0).to(BF)
        hi = (torch.randint(-14, 15, (case.R, D), generator=g).float() * EXACT_W_GRAN).to(BF)
        lo = (torch.randint(-2, 3, (case.R, D), generator=g).float() * EXACT_W_GRAN).to(BF)
    else:
        hi, lo = S.split(torch.randn(case.R, D, generator=g) * 0.05)
    return dict(x=x, mod=mod, W_hi=hi, W_lo=lo)


def mod_of(inp, case):
    """(shift, scale) views [B or 1, D] of the case's stride kind."""
    return R.mod_views(inp["mod"], case.D, case.stride, 0)[0], R.mod_views(inp["mod"], case.D, case.stride, 1)[0]


# ---------------------------------------------------------------------------------------------- the restatement
def _chain(t):
    acc = t[..., 0].clone()
    for i in range(1, t.shape[-1]):
        acc = acc + t[..., i]
    return acc


def contract32(y, W_hi, W_lo, flip=True, chain=64):
    """fp32 U [rows, R]: the hi and the lo products (each exact in fp32: two bf16 factors) summed apart, as the kernel's two MFMAs per
    k-step take them, over the reversed k axis in chains of `chain` terms, the chain sums in a chain again; hi sum + lo sum."""
    yf = y.float()
    parts = []
    for W in (W_hi, W_lo):
        t = yf[:, None, :] * W.float()[None]
        if flip:
            t = t.flip(-1)
        parts.append(_chain(_chain(t.reshape(t.shape[0], t.shape[1], -1, chain))))
    return parts[0] + parts[1]


def ln_down(x, shift, scale, rpb, W_hi=None, W_lo=None, *, y=None, group_R=None, group_stride=0, ld_ext=None, ld_ut=None, eps=EPS,
            dt=F64, flip=False, rnd=True):
    """{"y": (value, scale)} exactly as rowkernel_ref.ln_fwd returns it, and for an adapted problem (W_hi given)
         "U":   y (W_hi + W_lo)^T of the GIVEN bf16 `y` (default: the restatement's own y), fp64 -- or fp32 by contract32 for dt = fp32;
         "ext", "Ut_hi", "Ut_lo":  the whole-buffer images of fp32(U) ([rows, ld_ext], [R, ld_ut]; canary where the kernel has no
                business writing), when ld_ext / ld_ut are given.
    rnd = False: the plain formula, U from the unrounded y."""
    out = R.ln_fwd(x, shift, scale, rpb, eps=eps, dt=dt, flip=flip, rnd=rnd)
    if W_hi is None:
        return out
    if y is None:
        y = out["y"][0].to(BF) if rnd else out["y"][0]
    rows = torch.arange(y.shape[0])
    if not rnd:
        U = y.double() @ (W_hi.double() + W_lo.double()).t()
    elif dt == F64:
        U = S.down_ref(y, W_hi, W_lo, rows)
    else:
        U = contract32(y, W_hi, W_lo, flip)
    out["U"] = U
    if rnd and ld_ext is not None:
        out["ext"] = S.ext_image(U.float(), W_hi.shape[0] if group_R is None else group_R, group_stride, ld_ext)
    if rnd and ld_ut is not None:
        out["Ut_hi"], out["Ut_lo"] = S.ut_image(U.float(), ld_ut)
    return out


def ext_columns(Rr, group_R, group_stride):
    """Columns of the first hi, the lo and the second hi copy of U column j in an ext row (include/qfx.h), to read an image back;
    tests/test_ln_down_ref_cpu.py holds it against skinny_ref.ext_image."""
    j = torch.arange(Rr)
    c = (j // group_R) * group_stride + j % group_R
    return c, c + group_R, c + 2 * group_R


def case_ref(inp, case, dt=F64, flip=False, y=None, ld_ut=None):
    shift, scale = mod_of(inp, case)
    gR, gs, ld_ext = group_of(case)
    return ln_down(inp["x"], shift, scale, rpb_of(case), inp["W_hi"], inp["W_lo"], y=y, group_R=gR, group_stride=gs, ld_ext=ld_ext,
                   ld_ut=ld_ut, dt=dt, flip=flip)


def rel_u(got, U64):
    return ((got.double() - U64).abs().max() / U64.abs().max()).item()


def measure_floors(draws=FLOOR_DRAWS):
    """(y floor in bf16 ulps of scale over both kinds and `draws` draws of every case, U floor relative to max |U64| over the rand cases
    of draw 0, the case of each): the fp32, reversed-order restatement against the fp64 one.  Nothing here runs the code under test."""
    fy, fu = (0.0, None), (0.0, None)
    try:
        for draw in range(draws):
            R._DRAW[0] = draw
            for case in CASES:
                for kind in KINDS:
                    inp = make(case, kind)
                    shift, scale = mod_of(inp, case)
                    r64 = R.ln_fwd(inp["x"], shift, scale, rpb_of(case))["y"]
                    r32 = R.ln_fwd(inp["x"], shift, scale, rpb_of(case), dt=F32, flip=True)["y"]
                    fy = max(fy, (R.err_ulps(r32[0], *r64), (kind, case, draw)), key=lambda t: t[0])
                    if kind == "rand" and draw == 0:
                        yb = r64[0].to(BF)
                        U64 = S.down_ref(yb, inp["W_hi"], inp["W_lo"], torch.arange(case.rows))
                        fu = max(fu, (rel_u(contract32(yb, inp["W_hi"], inp["W_lo"]), U64), case), key=lambda t: t[0])
    finally:
        R._DRAW[0] = 0
    return fy, fu


# ---------------------------------------------------------------------------------------------- gate_mul
def gate_mul(dx, gate, rpb):
    """bf16(dx * gate[row // rpb]): the product of two bf16 values is exact in fp32 (and in fp64), so one rounding and no tolerance."""
    b = torch.arange(dx.shape[0]) // rpb if gate.shape[0] > 1 else torch.zeros(dx.shape[0], dtype=torch.int64)
    return (dx.double() * gate.double()[b]).float().to(BF)
