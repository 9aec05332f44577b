"""CPU restatement (torch only) of the GEMM entry points of csrc/qfx_gemm.hip and csrc/qfx_gemm_fp8.hip as include/qfx.h states
them -- qfx_gemm_bf16, qfx_gemm_grouped, qfx_gemm_mxfp8, qfx_gemm_mxfp8_grouped, qfx_quant_mxfp8 -- the yardstick of
tests/test_gemm_gpu.py.  Rounding points (`q` = round to bf16, nearest even):

    acc = A1[row_a(m)] . B1^T
    K2 > 0 and not seg2_plain:   acc = q(acc + bias);  acc += A2 . B2^T              (the bias is consumed here)
    otherwise:                   acc += A2 . B2^T (K2 > 0);  acc += bias
    EPI_NONE      C = q(acc)
    EPI_GELU      C = h = q(acc),  C2 = q(gelu_tanh(h))
    EPI_GATE_RES  y = q(acc),  C = q(aux + q(gate[b] y)),  C2[m] = y if given (rows unmapped)
    EPI_DGELU     C = q(q(acc) gelu_tanh'(aux))
    row_mask[m] == 0: every output of row m is +0.

Row maps (remap_row, qfx_common.h): row(m) = m when batch_rows == 0, else (m / rpb) * batch_rows + off + m % rpb; a_* applies to A1
only (A2 rows are compact), c_* to C, to C2 of GELU, and to aux unless aux_unmapped.  gelu_tanh and its derivative are the true tanh
form in fp64; the kernels' published rewrite x / (1 + 2^(-2u log2 e)) is `kernel_form`, used by the fp32 floor measurement only.

gemm_ref returns per output (value, scale) over the COMPACT rows m: scale is the largest magnitude among the bf16-rounded
intermediates on the element's path and, as in rowkernel_ref.mod_gemv, the largest addend of its contractions (max_k |a b|, |bias|:
an fp32 sum that cancels is no more accurate than its terms); a flipped rounding of an intermediate moves the output by one bf16 ulp
of that intermediate, so errors are counted in bf16 ulps of scale (err_ulps).  `image` places a compact result into the WHOLE output
buffer -- row stride, row map, extra rows -- with the canary everywhere the kernel must not write.

Arguments of the restatement: dt (fp64 = the reference, fp32 = the same arithmetic in the kernels' precision), flip (False, True =
K axis reversed, "perm" = a fixed permutation of K), rnd (False: every rounding point off).  fp32 + flip against fp64 is the
reference's OWN noise; tests/test_gemm_ref_cpu.py measures it on the case lists below and holds BARS to 2 x that floor.

exact_case: A1, B1, bias hold integers in [-2, 2]; A2, B2, gate and the residual hold integers in [-2, 2] times 2^-4.  Magnitude
argument: a base partial sum is an integer of magnitude <= 4 K1 + 2; a LoRA term is a multiple of 2^-8 of magnitude <= 2^-6, so with
K1 + K2 <= EXACT_MAX_K = 4096 every partial sum (any order, either segment, with or without the mid-rounding) is a multiple of 2^-8
below 2^15: 23 bits, inside the 24-bit significand of fp32.  q of an exactly known value is the same in every implementation.
gate y: a 3-bit times an 8-bit significand, exact; aux + q(gate y): q(gate y) has 8 bits, aux is a multiple of 2^-4 below 2^-2, so
the sum spans at most 8 + 12 bits.  An fp32-accumulating kernel must therefore give C of NONE, C and C2 of GATE_RES and the
pre-activation C of GELU BIT FOR BIT in any K order on any tile geometry (EXACT_OUTPUTS).  The integers are powers of two or zero
times a sign, so an MX block of them is exactly representable in e4m3 under its power-of-two scale: the same holds for the MX-FP8
entries.  C2 of GELU and C of DGELU pass through exp2 / rcp and are held to their bars."""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import torch

from rowkernel_ref import BF, CANARY_BF16, bits, canary_bf16, err_ulps, q_bf16, ulp_bf16   # noqa: F401  (re-exported)
from skinny_ref import remap_rows

F64, F32 = torch.float64, torch.float32
NONE, GELU, GATE_RES, DGELU = 0, 1, 2, 3
EPI_NAME = {NONE: "none", GELU: "gelu", GATE_RES: "gate_res", DGELU: "dgelu"}
EXACT_MAX_K = 4096
EXACT_OUTPUTS = {"none.C", "gelu.C", "gate_res.C", "gate_res.C2"}
Y_OUTPUTS = ("none.C", "gelu.C", "gate_res.C2")      # all three are y = q(acc): one noise floor (measure_floors)
CANARY_U8 = 0xA5             # fill of the fp8 byte / scale byte buffers
FLUSH = 2.0 ** -100          # gelu_sweep_case: outputs below this magnitude only have to stay below it (hardware exp2 / rcp flush)
FLOOR_DRAWS = 4              # draws of every case in measure_floors
FLOOR_EXTRA_DRAWS = 8        # further draws of the cases of at most FLOOR_EXTRA_ELEMS output elements: a flip is a rare event per element,
FLOOR_EXTRA_ELEMS = 1 << 16  # and the small cases are where a draw costs least

# ---------------------------------------------------------------------------------------------- bars, in bf16 ulps of `scale`
# BARS[output] = 2 x the floor measured by tests/test_gemm_ref_cpu.py::test_bars_are_twice_the_reference_noise (the restatement in fp32,
# K reversed, gelu / gelu' in the kernels' published form, against fp64 with the tanh form; every case list below, FLOOR_DRAWS draws,
# FLOOR_EXTRA_DRAWS more of the small cases),
# rounded up to a whole ulp, at least one.  Never taken from what the kernels give.  The fp32 evaluation has an explicit summation order
# (_mm), so these floors are the same numbers on every host.
BARS = {
    "none.C": 3,          # floor 1.50  (y: a flipped mid-rounding, one ulp of the base output, that carries y across a binade: another half)
    "gelu.C": 3,          # floor 1.50  (y)
    "gelu.C2": 4,         # floor 2.00  (a flipped h under a gelu(h) just below a power of two)
    "gate_res.C": 4,      # floor 2.00  (a flipped y times a gate just below a power of two)
    "gate_res.C2": 3,     # floor 1.50  (y)
    "dgelu.C": 4,         # floor 2.00
}


# ---------------------------------------------------------------------------------------------- cases
@dataclass(frozen=True)
class Case:
    """One GEMM problem.  rpb = 0: one sample (rows_per_batch = M).  a_map / c_map: (text rows T) -> batch_rows = rpb + T, off = T.
    mask: compact rows whose row_mask is 0.  pad: elements every row stride exceeds its extent by (operands then start at column 8 of
    the wider buffer when pad >= 16: column slices); 0 = tight.  c2: GATE_RES writes C2.  gate_shared: gate_bstride = 0."""
    epi: int
    M: int
    N: int
    K1: int
    K2: int = 0
    bias: bool = True
    rpb: int = 0
    a_map: int = 0
    c_map: int = 0
    mask: tuple = ()
    aux_unmapped: bool = False
    seg2_plain: bool = False
    c2: bool = False
    gate_shared: bool = False
    pad: int = 8
    fp8: bool = False
    sweep: bool = False

    @property
    def rows_per_batch(self):
        return self.rpb or self.M

    @property
    def B(self):
        return (self.M + self.rows_per_batch - 1) // self.rows_per_batch

    def row_map(self, T):
        """(destination row of every compact row, rows of the joint buffer, batch_rows, off) for T text rows per sample (0: identity)."""
        if not T:
            return torch.arange(self.M), self.M, 0, 0
        br = self.rows_per_batch + T
        return remap_rows(self.M, self.rows_per_batch, br, T), self.B * br, br, T

    def outputs(self):
        return {NONE: ["C"], GELU: ["C", "C2"], GATE_RES: ["C", "C2"] if self.c2 else ["C"], DGELU: ["C"]}[self.epi]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed(case, draw):
    return (hash((case.epi, case.M, case.N, case.K1, case.K2, case.rpb, case.fp8)) & 0xFFFFFF) * 8 + draw


def _ints(g, shape, scale=1.0):
    return (torch.randint(-2, 3, shape, generator=g).float() * scale).to(BF)


def make_inputs(case, kind, draw=0):
    """Logical (tight, compact-row) bf16 operands of a case: A1 [M, K1], B1 [N, K1], A2 [M, K2], B2 [N, K2], bias [N], aux [M, N], gate
    [B, N], mask [M] fp32.  kind "rand": Gaussian data at the scales of tests/test_kernels_gpu.py; "exact": see the module docstring.
    fp8 cases add A1q / B1q (bytes), sa / sb (tile-major scale bytes) and replace A1 / B1 by the dequantised fp64 operands."""
    if case.sweep:
        return gelu_sweep_case(case)
    assert kind in ("rand", "exact")
    g = _gen(_seed(case, draw))
    M, N, K1, K2 = case.M, case.N, case.K1, case.K2
    if kind == "exact":
        assert K1 + K2 <= EXACT_MAX_K
        mk = lambda shape, sc, lo=False: _ints(g, shape, 2.0 ** -4 if lo else 1.0)          # noqa: E731  (sc: the Gaussian scale, unused here)
    else:
        mk = lambda shape, sc, lo=False: (torch.randn(*shape, generator=g) * sc).to(BF)    # noqa: E731
    inp = dict(A1=mk((M, K1), 1.0), B1=mk((N, K1), 0.05), A2=mk((M, K2), 0.1, True), B2=mk((N, K2), 0.1, True),
               bias=mk((N,), 1.0) if case.bias else None, aux=mk((M, N), 1.0, True),
               gate=mk((1 if case.gate_shared else case.B, N), 1.0, True))
    if kind == "exact":
        # B1 rows and every second A1 row carry ONE sign each: those base sums grow like 1.44 K1 instead of 2.4 sqrt(K1) and pass 2^8
        # from K1 = 192 on, where the bf16 mid-rounding (and the rounding of y) actually drops bits -- ties included; the other rows
        # keep independent signs.  Still integers in [-2, 2]: the magnitude argument of the module docstring is the worst case.
        sm = torch.where(torch.arange(M) % 2 == 0, torch.randint(0, 2, (M,), generator=g) * 2 - 1, torch.zeros(M, dtype=torch.int64)).float()[:, None]
        sn = (torch.randint(0, 2, (N,), generator=g) * 2 - 1).float()[:, None]
        a1 = inp["A1"].float()
        inp["A1"] = torch.where(sm != 0, a1.abs() * sm, a1).to(BF)
        inp["B1"] = (inp["B1"].float().abs() * sn).to(BF)
    mask = torch.ones(M)
    mask[[r for r in case.mask if r < M]] = 0
    inp["mask"] = mask if case.mask else None
    if case.fp8:
        for k in ("A1", "B1"):
            qb, sc, deq = quant_mxfp8_ref(inp[k])
            inp[k + "q"], inp["s" + k[0].lower()], inp[k] = qb, sc, deq
    return inp


# ---------------------------------------------------------------------------------------------- gelu
K0 = math.sqrt(2.0 / math.pi)
K1C = 0.044715


def _one_plus_tanh(u):
    """1 + tanh(u).  Below u = -8 the sum cancels (tanh = -1 + 2 e^2u, e^2u < 2^-23) and is formed as 2 e^2u / (1 + e^2u) instead: the
    same function at full relative accuracy, so that the far negative tail of gelu has a reference at all."""
    e = torch.exp(2.0 * u.clamp(max=0.0))
    return torch.where(u < -8.0, 2.0 * e / (1.0 + e), 1.0 + torch.tanh(u))


def gelu_tanh(x):
    return 0.5 * x * _one_plus_tanh(K0 * (x + K1C * x ** 3))


def gelu_tanh_grad(x):
    p = _one_plus_tanh(K0 * (x + K1C * x ** 3))            # 1 + t;  1 - t^2 = (1 + t) (2 - (1 + t))
    return 0.5 * p + 0.5 * x * p * (2.0 - p) * K0 * (1.0 + 3.0 * K1C * x * x)


def _kernel_sigmoid(x, x2):
    """s(2u) as csrc/qfx_common.h evaluates it (fp32): 1 / (1 + 2^t), t = x (x^2 c1 + c0) = -2u log2 e."""
    c0, c1 = torch.tensor(-2.3022082, dtype=F32), torch.tensor(-0.10294324, dtype=F32)
    return 1.0 / (1.0 + torch.exp2(x * (x2 * c1 + c0)))


def gelu_kernel_form(x):
    assert x.dtype == F32
    return x * _kernel_sigmoid(x, x * x)


def gelu_grad_kernel_form(x):
    assert x.dtype == F32
    x2 = x * x
    s = _kernel_sigmoid(x, x2)
    du2 = x2 * torch.tensor(0.21406445, dtype=F32) + torch.tensor(1.5957692, dtype=F32)
    return x * du2 * (s - s * s) + s


# ---------------------------------------------------------------------------------------------- the restatement
_PERM = {}


def _korder(K, flip):
    if flip is False:
        return None
    if flip is True:
        return torch.arange(K - 1, -1, -1)
    if K not in _PERM:
        _PERM[K] = torch.randperm(K, generator=_gen(K))
    return _PERM[K]


KSTEP = 32      # K elements per fp32 accumulation step of the noise model (one MFMA k-step)


def _mm(A, B, dt, flip):
    """A . B^T.  fp64: the host's matrix product (its own error, 2^-53 relative, never decides a bf16 rounding).  fp32: an EXPLICIT
    order, the same on every host -- the K axis in the order `flip` selects, cut into steps of KSTEP elements; each step's partial
    product is formed in fp64 and rounded to fp32 once, the steps are added one after the other in fp32 (elementwise IEEE additions).
    Nothing of it depends on how a BLAS blocks its sums, so the floors of measure_floors are the same numbers everywhere."""
    idx = _korder(A.shape[1], flip)
    if idx is not None:
        A, B = A[:, idx], B[:, idx]
    if dt == F64:
        return A.double() @ B.double().t()
    assert dt == F32
    M, K = A.shape
    acc = torch.zeros(M, B.shape[0], dtype=F32)
    if K == 0:
        return acc
    assert K % KSTEP == 0
    a = A.double().reshape(M, K // KSTEP, KSTEP).transpose(0, 1)                       # [steps, M, KSTEP]
    b = B.double().reshape(B.shape[0], K // KSTEP, KSTEP).permute(1, 2, 0)             # [steps, KSTEP, N]
    for part in torch.bmm(a, b).float():
        acc = acc + part
    return acc


def _max_term(A, B):
    """max_k |A[m, k] B[n, k]| as [M, N] fp64 (the largest addend of the contraction), in row chunks."""
    M, K = A.shape
    out = torch.zeros(M, B.shape[0], dtype=F64)
    if K == 0:
        return out
    a, b = A.float().abs(), B.float().abs()
    step = max(1, (1 << 22) // max(1, b.numel()))
    for m0 in range(0, M, step):
        out[m0:m0 + step] = (a[m0:m0 + step, None, :] * b[None]).amax(2).double()
    return out


def gemm_ref(inp, case, dt=F64, flip=False, rnd=True, kernel_form=False, with_y=False):
    """{"C": (value, scale), "C2": ...} over compact rows [M, N].  Scales are formed for dt = fp64 only (zeros otherwise).
    with_y: also "y", the rounded linear output q(acc) every epilogue starts from (C of NONE and GELU, C2 of GATE_RES)."""
    q = q_bf16 if rnd else (lambda t: t)
    M, N = case.M, case.N
    acc = _mm(inp["A1"], inp["B1"], dt, flip)
    bias = inp["bias"].to(dt)[None] if inp["bias"] is not None else None
    sc = torch.zeros(M, N, dtype=F64)
    if dt == F64:      # the addends of the fp32 sum are on the element's path too: a cancelling sum is no better than its largest term
        sc = torch.maximum(_max_term(inp["A1"], inp["B1"]), _max_term(inp["A2"], inp["B2"]))
        if bias is not None:
            sc = torch.maximum(sc, bias.abs().double().expand(M, N))
    if case.K2 > 0 and not case.seg2_plain:
        if bias is not None:
            acc = acc + bias
        acc = q(acc)
        sc = torch.maximum(sc, acc.abs().double())
        acc = acc + _mm(inp["A2"], inp["B2"], dt, flip)
    else:
        if case.K2 > 0:
            acc = acc + _mm(inp["A2"], inp["B2"], dt, flip)
        if bias is not None:
            acc = acc + bias
    y = q(acc)
    sc = torch.maximum(sc, y.abs().double())
    out = {"y": (y, sc)} if with_y else {}
    if case.epi == NONE:
        out["C"] = (y, sc)
    elif case.epi == GELU:
        g = q(gelu_kernel_form(y) if kernel_form else gelu_tanh(y))
        out["C"] = (y, sc)
        out["C2"] = (g, torch.maximum(sc, g.abs().double()))
    elif case.epi == GATE_RES:
        b = torch.zeros(M, dtype=torch.int64) if case.gate_shared else torch.arange(M) // case.rows_per_batch
        gt = inp["gate"].to(dt)[b]
        gy = q(gt * y)
        c = q(inp["aux"].to(dt) + gy)
        out["C"] = (c, torch.maximum(torch.maximum(gt.abs().double() * sc, gy.abs().double()), c.abs().double()))
        if case.c2:
            out["C2"] = (y, sc)
    else:
        h = inp["aux"].to(dt)
        c = q(y * (gelu_grad_kernel_form(h) if kernel_form else gelu_tanh_grad(h)))
        out["C"] = (c, torch.maximum(sc, c.abs().double()))
    if inp.get("mask") is not None:
        keep = (inp["mask"] != 0)[:, None]
        out = {k: (torch.where(keep, v, torch.zeros_like(v)), torch.where(keep, s, torch.zeros_like(s))) for k, (v, s) in out.items()}
    return out


def image(val, rows, buf_rows, ld, fill=CANARY_BF16):
    """The whole bf16 output buffer [buf_rows, ld]: val [M, N] at the rows `rows`, columns [0, N); `fill` everywhere else."""
    M, N = val.shape
    assert ld >= N and rows.numel() == M and (M == 0 or int(rows.max()) < buf_rows)
    img = torch.full((buf_rows, ld), fill, dtype=torch.int16).view(BF)
    img[rows, :N] = val.to(BF)
    return img


# ---------------------------------------------------------------------------------------------- MX-FP8
def _e4m3_rne(v):
    """fp64 values of magnitude <= 448 -> (e4m3fn bytes, the values they encode): round to nearest even on the e4m3 grid."""
    a = v.abs()
    _, ex = torch.frexp(a.clamp_min(2.0 ** -40))
    E = (ex - 1).clamp(min=-6)                         # binade; below 2^-6 the subnormal grid 2^-9
    quantum = torch.ldexp(torch.ones_like(a), E - 3)
    qa = torch.round(a / quantum) * quantum            # torch.round: half to even
    _, ex2 = torch.frexp(qa.clamp_min(2.0 ** -40))
    E2 = (ex2 - 1).clamp(min=-6)
    normal = qa >= 2.0 ** -6
    mant = torch.where(normal, qa / torch.ldexp(torch.ones_like(a), E2 - 3) - 8.0, qa * 2.0 ** 9).to(torch.int64)
    expf = torch.where(normal, E2 + 7, torch.zeros_like(E2)).to(torch.int64)
    byte = (torch.signbit(v).to(torch.int64) << 7) | (expf << 3) | mant
    return byte.to(torch.uint8), torch.where(torch.signbit(v), -qa, qa)


def quant_mxfp8_ref(x):
    """OCP MX-FP8 of x [M, K] (K % 128 == 0) along K as include/qfx.h states it: per 32 consecutive elements the shared exponent
    e = floor(log2 max|v|) - 8 (clamped at the E8M0 minimum -127, which is also what an all-zero block gets: scale byte 0), elements
    RNE(v / 2^e) on the e4m3fn grid after saturation at +-448, scale byte e + 127 at ((kb / 4) * M + m) * 4 + kb % 4.
    Returns (bytes [M, K] uint8, scale bytes [K / 128 * M * 4] uint8, dequantised fp64 [M, K])."""
    M, K = x.shape
    assert K % 128 == 0
    v = x.double().view(M, K // 32, 32)
    amax = v.abs().amax(-1)
    _, ex = torch.frexp(amax.clamp_min(2.0 ** -140))
    e = torch.where(amax > 0, ex - 1 - 8, torch.full_like(ex, -127)).clamp(min=-127)
    sc = torch.ldexp(torch.ones_like(amax), e)[..., None]
    byte, qv = _e4m3_rne((v / sc).clamp(-448.0, 448.0))
    m = torch.arange(M)[:, None]
    kb = torch.arange(K // 32)[None]
    S = torch.full((K // 128 * M * 4,), CANARY_U8, dtype=torch.uint8)
    S[(((kb // 4) * M + m) * 4 + kb % 4).flatten()] = (e + 127).to(torch.uint8).flatten()
    return byte.view(M, K), S, (qv * sc).view(M, K)


def scale_image(S, M, rows, buf_rows, fill=CANARY_U8):
    """Tile-major scale bytes of M compact rows re-homed to the rows `rows` of a [*, buf_rows, 4] array (the quantising epilogue)."""
    t = S.view(-1, M, 4)
    img = torch.full((t.shape[0], buf_rows, 4), fill, dtype=torch.uint8)
    img[:, rows] = t
    return img.flatten()


# ---------------------------------------------------------------------------------------------- gelu sweep
SWEEP_Y = (1.0, -1.0, 0.5, 1.5, -2.0, 0.75)


def sweep_table():
    """Every bf16 value with 2^-64 <= |h| <= 16, and +-0 (17412 values)."""
    lo, hi = (127 - 64) << 7, ((127 + 4) << 7) + 1
    pos = torch.arange(lo, hi, dtype=torch.int32)
    allb = torch.cat([torch.tensor([0, 0x8000], dtype=torch.int32), pos, pos | 0x8000])
    return allb.to(torch.int16).view(BF)


def gelu_sweep_case(case):
    """M = K1 = 128, N = 256, A1 = identity: C[m, n] = B1[n, m].  GELU: B1 holds the table (repeated to fill), so h takes every table
    value exactly.  DGELU: aux holds the table, B1 a handful of exact y values.
    What the sweep is NOT: scale is at least |h| (GELU) resp. |y| (DGELU), so where gelu(h) or gelu'(aux) is much smaller than its
    argument -- the negative tail, the zero of gelu' -- the output is judged in ulps of the INPUT magnitude, an absolute check.  A
    kernel that is wrong only there, by less than that, passes; FLUSH and the cancellation-free tail of _one_plus_tanh merely keep the
    reference itself meaningful.  The sweep catches a gelu / gelu' that is off by a bf16 ulp of h / y anywhere on the range."""
    assert case.sweep and case.M == case.K1 == 128 and case.N == 256 and case.K2 == 0 and not case.bias
    tab = sweep_table()
    full = tab.repeat(128 * 256 // tab.numel() + 1)[:128 * 256].view(128, 256)        # [m, n]
    ys = torch.tensor(SWEEP_Y).to(BF)[(torch.arange(128)[:, None] + torch.arange(256)[None]) % len(SWEEP_Y)]
    B1 = (full if case.epi == GELU else ys).t().contiguous()
    return dict(A1=torch.eye(128).to(BF), B1=B1, A2=torch.zeros(128, 0, dtype=BF), B2=torch.zeros(256, 0, dtype=BF), bias=None, aux=full,
                gate=torch.zeros(1, 256, dtype=BF), mask=None)


def flushed(ref_val):
    return ref_val.double().abs() < FLUSH


# ---------------------------------------------------------------------------------------------- case lists (CPU and GPU tests walk these)
SMALL_M = (1, 15, 16, 17, 127, 128, 129, 257)
SMALL_N = (4, 8, 60, 64, 124, 128, 132, 260)
K1S, K2S = (64, 128, 192, 320), (0, 64, 128)
GEOS = {"256x128": (256, 128), "256x256": (256, 256), "160x192": (160, 192)}
EPIS = (NONE, GELU, GATE_RES, DGELU)


def _variety(c, i):
    """Cycle the optional arms over a list of shapes: bias, row maps, masks, C2, gate stride, three samples, tight strides."""
    M = c.M
    kw = dict(bias=i % 5 != 0, c2=i % 2 == 0, gate_shared=i % 4 == 3, pad=(8, 24, 0, 8)[i % 4])
    if M >= 3 and i % 3 != 0:
        kw["rpb"] = (M + 2) // 3 if i % 3 == 1 else (M + 1) // 2
        kw["c_map"] = 5 if i % 2 else 0
        kw["a_map"] = 3 if i % 3 == 1 and not c.fp8 else 0
    if i % 7 == 3:
        kw["mask"] = (0, M // 2, M - 1)
    return replace(c, **kw)


def _grid(epi, Ms, Ns, k1s=K1S, k2s=K2S, **kw):
    out = []
    for i, M in enumerate(Ms):
        for j, N in enumerate(Ns):
            idx = i * len(Ns) + j
            out.append(_variety(Case(epi, M, N, k1s[(i + j) % len(k1s)], k2s[(i + 2 * j + epi) % len(k2s)], **kw), idx + epi))
    return out


def _kcross(epi, M, N, k1s=K1S, k2s=K2S, **kw):
    return [_variety(Case(epi, M, N, k1, k2, **kw), 1 + n) for n, (k1, k2) in enumerate((a, b) for a in k1s for b in k2s)]


SMALL_CASES = {e: _grid(e, SMALL_M, SMALL_N) + _kcross(e, 129, 132) for e in EPIS}


def persist_ms(bmt):
    return (1, 16, bmt - 1, bmt, bmt + 1, 2 * bmt + 17)


def persist_ns(geo):
    bmt, tn = GEOS[geo]
    return (256, 512) if tn == 256 else (8, tn - 8, tn, 2 * tn + 8)


PERSIST_CASES = {(geo, e): _grid(e, persist_ms(GEOS[geo][0]), persist_ns(geo)) + _kcross(e, GEOS[geo][0] + 1, persist_ns(geo)[-1])
                 for geo in GEOS for e in EPIS}
# more tiles than the 256 CUs: one tile row of 17 / 33 rows, 260 tile columns, thin K -- a block runs two tiles back to back and the
# loader waves cross the tile boundary with the ring full (K = 64: every K tile is a tile boundary; K = 192: exactly the 3-stage ring)
MANY_TILE_CASES = {geo: [Case(NONE, 17, 260 * GEOS[geo][1], 64, 0), Case(GATE_RES, 33, 260 * GEOS[geo][1], 192, 64, rpb=17, c_map=5, c2=True)]
                   for geo in GEOS}
# qfx_gemm_grouped(256x256) with an N that is no multiple of 256: the launcher must fall back to a narrow tile
FALLBACK_CASES = [Case(NONE, 257, 264, 128, 64), Case(GELU, 300, 136, 64, 0)]

# arms no other test reaches
ARM_CASES = [
    # aux_unmapped with a c_* map: both epilogues that read aux
    Case(DGELU, 129, 256, 128, 64, rpb=43, c_map=5, aux_unmapped=True),
    Case(GATE_RES, 129, 256, 128, 0, rpb=65, c_map=7, aux_unmapped=True, c2=True),
    Case(DGELU, 129, 136, 128, 0, rpb=65, c_map=7, aux_unmapped=False),
    # seg2_plain: no mid-rounding, bias at the end
    Case(NONE, 129, 256, 192, 128, seg2_plain=True),
    Case(GELU, 130, 136, 64, 64, seg2_plain=True, rpb=65, c_map=5),
    Case(GATE_RES, 257, 256, 128, 64, seg2_plain=True, c2=True),
    Case(DGELU, 17, 264, 320, 128, seg2_plain=True, bias=False),
    Case(DGELU, 300, 256, 64, 64, seg2_plain=True),
    # GATE_RES with C2 and a row mask: C2 rows +0, unmapped
    Case(GATE_RES, 130, 256, 128, 64, rpb=44, c_map=5, c2=True, mask=(0, 43, 44, 129)),
    # three samples, a_* and c_* maps together
    Case(GATE_RES, 129, 256, 128, 64, rpb=43, a_map=3, c_map=5, c2=True),
    Case(NONE, 258, 72, 64, 0, rpb=86, a_map=9, c_map=2, pad=24),
]

# the landing-buffer conditions (use_dma) of the 256x256 / 160x192 d(GELU) epilogue, both sides of each; <= 3 tiles
def landing_cases(geo):
    bmt, tn = GEOS[geo]
    on = Case(DGELU, 48, tn, 128, 64, bias=True)                        # every condition holds: aux rows by LDS-DMA
    lst = [on,
           replace(on, K2=0, bias=False),                               # no bias at all
           replace(on, mask=(3, 47)),                                   # a row mask
           replace(on, M=40),                                           # M % 16 != 0
           replace(on, M=bmt + 32),                                          # a second tile whose later passes lie past M (the early return)
           replace(on, K2=0),                                           # bias pending for the epilogue
           replace(on, seg2_plain=True),                                # ... through seg2_plain
           replace(on, rpb=24, c_map=5),                                # a wave's rows straddle a sample boundary
           replace(on, M=2 * bmt, rpb=bmt, c_map=5),                    # mapped, one sample per tile: still DMA, row_delta != 0
           replace(on, M=2 * bmt, rpb=bmt, c_map=5, aux_unmapped=True),  # ... with compact aux rows
           replace(on, rpb=24, c_map=5, aux_unmapped=True)]
    if tn != 256:
        lst.append(replace(on, N=tn + 8))                               # ragged column range of the second tile's first wave
        lst.append(replace(on, N=tn - 8))                               # ... and of the last wave of a single tile
    return lst


LANDING_CASES = {geo: landing_cases(geo) for geo in ("256x256", "160x192")}

# grouped launches: (geometry, problems); same epilogue per launch
GROUPED_CASES = [
    ("256x128", [Case(NONE, 300, 136, 128, 64), Case(NONE, 17, 264, 64, 0, bias=False)]),
    ("160x192", [Case(GELU, 161, 200, 192, 0), Case(GELU, 16, 8, 64, 128, bias=False), Case(GELU, 330, 192, 320, 64, rpb=165, c_map=5)]),
    ("256x256", [Case(GATE_RES, 257, 256, 128, 64, c2=True), Case(GATE_RES, 31, 512, 64, 0, bias=False, gate_shared=True)]),
    # n = 6 selects gm = 4: five M-tiles make the second supertile a short one
    ("256x128", [Case(DGELU, 1025 + 16 * i, 136, 64, 64 if i % 2 else 0, bias=i % 3 != 0) for i in range(6)]),
    ("160x192", [Case(NONE, 640 + i, 200, 128, 0 if i % 2 else 64, bias=i % 2 == 0) for i in range(6)]),
    # 200 + 100 tiles on 152 blocks: the boundary between the two problems falls inside a block's tile list
    ("256x128", [Case(NONE, 17, 200 * 128, 64, 0), Case(NONE, 33, 100 * 128, 128, 64, bias=False)]),
]

SWEEP_CASES = [Case(GELU, 128, 256, 128, bias=False, sweep=True), Case(DGELU, 128, 256, 128, bias=False, sweep=True)]

# MX-FP8
FP8_K1S, FP8_K2S = (128, 256, 384), (0, 64)
FP8_SMALL_CASES = {e: _grid(e, (1, 17, 129, 257), (4, 60, 132, 260), FP8_K1S, FP8_K2S, fp8=True) for e in EPIS}
FP8_PERSIST_CASES = {e: _grid(e, persist_ms(256), (8, 120, 128, 264), FP8_K1S, FP8_K2S, fp8=True) + _kcross(e, 257, 264, FP8_K1S, FP8_K2S, fp8=True)
                     for e in EPIS}
FP8_QUANT_EPI_CASES = [Case(NONE, 257, 128, 128, 64, fp8=True), Case(GELU, 300, 256, 256, 0, fp8=True, rpb=150, c_map=5),
                       Case(DGELU, 257, 128, 128, 0, fp8=True, rpb=129, c_map=5),
                       Case(NONE, 129, 256, 256, 0, fp8=True, mask=(0, 64, 128)), Case(GELU, 130, 128, 128, 64, fp8=True, mask=(0, 129)),
                       Case(DGELU, 129, 256, 384, 64, fp8=True, rpb=65, c_map=3, mask=(1, 128))]
FP8_GROUPED_CASES = [[Case(NONE, 257, 136, 128, 64, fp8=True), Case(NONE, 17, 264, 256, 0, fp8=True, bias=False),
                      Case(NONE, 300, 128, 384, 64, fp8=True, rpb=150, c_map=5)]]
# qfx_quant_mxfp8: (M, K, rpb, text rows of the X row map)
QUANT_CASES = [(1, 128, 0, 0), (17, 256, 0, 0), (130, 384, 65, 5), (64, 1024, 0, 0)]


def quant_input(case, draw=0):
    """bf16 X [M, K] with the edge blocks: all zero, one element at 448 * 2^e, a value RNE would carry past 448, a block maximum
    just below a power of two, the E8M0 minimum, negative zeros."""
    M, K, _, _ = case
    g = _gen(M * 131 + K + draw)
    x = (torch.randn(M, K, generator=g) * torch.exp(2.0 * torch.randn(M, 1, generator=g))).to(BF)
    r = M - 1
    x[0, :32] = 0
    x[r, 32:64] = 0.01
    x[r, 40] = 448.0 * 2.0 ** -3                    # 1.75 * 2^5: maps onto 448 exactly
    x[0, 64:96] = 1.0
    x[0, 70] = -1.9375                              # 1.9375 * 256 = 496: between 448 and the next grid point -> saturates
    x[r, 96:128] = 0.25
    x[r, 100] = 1.9921875                           # the largest bf16 below 2
    x[0, 96:128] = 2.0 ** -126                      # exponent clamps at the E8M0 minimum
    x[0, 100] = -0.0
    return x


ALL_FAMILIES = {
    "small": [c for e in EPIS for c in SMALL_CASES[e]],
    **{f"persist_{geo}": [c for e in EPIS for c in PERSIST_CASES[(geo, e)]] for geo in GEOS},
    "many_tiles": [c for geo in GEOS for c in MANY_TILE_CASES[geo]],
    "fallback": FALLBACK_CASES,
    "arms": ARM_CASES,
    "landing": [c for geo in LANDING_CASES for c in LANDING_CASES[geo]],
    "grouped": [c for _, probs in GROUPED_CASES for c in probs],
    "sweep": SWEEP_CASES,
    "fp8_small": [c for e in EPIS for c in FP8_SMALL_CASES[e]],
    "fp8_persist": [c for e in EPIS for c in FP8_PERSIST_CASES[e]],
    "fp8_quant_epi": FP8_QUANT_EPI_CASES,
    "fp8_grouped": [c for probs in FP8_GROUPED_CASES for c in probs],
}


def key_of(case, out):
    return f"{EPI_NAME[case.epi]}.{out}"


def measure_floors(families=None, draws=FLOOR_DRAWS, extra=FLOOR_EXTRA_DRAWS):
    """{BARS key: worst error of the fp32, K-reversed, kernel-form restatement against the fp64 tanh-form one, in bf16 ulps of scale}
    over every case list -- the reference's own noise; nothing here runs the code under test.  Draw 0 is the data of the GPU tests.
    The outputs in Y_OUTPUTS are one quantity, the rounded linear output y = q(acc) that EVERY case forms before its epilogue: their
    floor is measured once, on y of all cases, which is four times the sample any one of them has alone.
    Flushed elements of the sweep (|reference| < FLUSH) are outside the bar and outside the floor."""
    floors = {}
    seen = set()
    for fam, cases in ALL_FAMILIES.items():
        if families is not None and fam not in families:
            continue
        for case in cases:
            if case in seen:
                continue
            seen.add(case)
            n = draws + (extra if case.M * case.N <= FLOOR_EXTRA_ELEMS else 0)
            for draw in range(1 if case.sweep else n):
                inp = make_inputs(case, "rand", draw)
                r64, r32 = gemm_ref(inp, case, with_y=True), gemm_ref(inp, case, F32, True, kernel_form=True, with_y=True)
                for k, (v, sc) in r64.items():
                    got = r32[k][0]
                    if case.sweep:
                        live = ~flushed(v)
                        got, v, sc = got[live], v[live], sc[live]
                    key = "y" if k == "y" or key_of(case, k) in Y_OUTPUTS else key_of(case, k)
                    floors[key] = max(floors.get(key, 0.0), err_ulps(got, v, sc))
    y = floors.pop("y")
    floors.update({k: y for k in Y_OUTPUTS})
    return floors
