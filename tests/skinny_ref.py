"""CPU restatement (fp64 sums, torch only) of the rank-r LoRA kernels of csrc/qfx_skinny.hip, the yardstick of tests/test_skinny_gpu.py:
qfx_lora_down(_batch), qfx_lora_grad(_batch), qfx_lora_head_reduce and qfx_lora_pack as include/qfx.h states them.

  * row(m) of compact row m:  m when x_batch_rows == 0, else (m / rpb) * x_batch_rows + x_row_off + m % rpb      (remap_row, qfx_common.h);
  * down:   U[m, j] = sum_k X[row(m), k] (W_hi + W_lo)[j, k]                                                     fp32 in the kernel;
  * split:  hi = bf16(u) (round to nearest even), lo = bf16(u - hi), both from the fp32 u;
  * ext:    U column j goes to columns (j / group_R) * group_stride + j % group_R + {0, group_R, 2 group_R} as hi, lo, hi;
  * Ut:     Ut_hi[j, m] = hi(U[m, j]), Ut_lo[j, m] = lo(U[m, j]);
  * grad:   G_grp[jj, k] += out_scale * sum_m (Vt_hi + Vt_lo)[grp * group_R + jj, m] X[row(m), k]   for jj < r_valid;
  * pack:   A_hi / A_lo [Rp, K] = split(A) with rows r.. zero, Bt_hi / Bt_lo [Rp, N] = split(fp32(scale * B)^T) likewise,
            We [N, Kext] = [Bt_hi^T | Bt_hi^T | Bt_lo^T | 0], WeT [K, Kext] = [A_hi^T | A_hi^T | A_lo^T | 0].

The image builders return WHOLE output buffers: every element the kernel has no business writing holds `fill`, by default the canary
the GPU tests put there before the launch, so one bit comparison checks the values and the bounds of the stores at once.

Two data generators: rand_case (Gaussian bf16 data, as tests/test_kernels_gpu.py uses) and exact_case, whose values are small integers
(hi parts, X) and small integers times 2^-4 (lo parts): every product is a multiple of 2^-4 of magnitude <= 4, so every partial sum of up
to 2^15 of them, in any order, is a multiple of 2^-4 of magnitude <= 2^17 and fits the 24-bit significand of fp32 (21 bits) -- an fp32 kernel must
give the fp64 sum bit for bit whatever its summation order (tests/test_skinny_ref_cpu.py checks that claim at the largest sizes used)."""
from __future__ import annotations

import torch

BF = torch.bfloat16
CANARY_BF16 = 0x7FC1         # a bf16 NaN no conversion produces
CANARY_F32 = 0x7FC00000      # torch's fp32 NaN
# the longest contractions the GPU tests may run on exact_case data (down: over K, grad: over tokens, head_reduce: over heads);
# tests/test_skinny_ref_cpu.py proves the exactness claim at these lengths, tests/test_skinny_gpu.py asserts it stays within them
EXACT_MAX_K = 12288
EXACT_MAX_M = 2048


def canary_bf16(*shape, device="cpu"):
    return torch.full(shape, CANARY_BF16, dtype=torch.int16, device=device).view(BF)


def canary_f32(*shape, device="cpu"):
    return torch.full(shape, CANARY_F32, dtype=torch.int32, device=device).view(torch.float32)


def bits(t):
    """The bit pattern of a bf16 / fp32 tensor as an integer tensor (NaN canaries compare equal, -0 differs from +0)."""
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def split(u32):
    assert u32.dtype == torch.float32
    hi = u32.to(BF)
    lo = (u32 - hi.float()).to(BF)
    return hi, lo


def remap_rows(M, rpb, batch_rows, off):
    m = torch.arange(M, dtype=torch.int64)
    if batch_rows == 0:
        return m
    b = m // rpb
    return b * batch_rows + off + (m - b * rpb)


def down_ref(X, W_hi, W_lo, rows):
    """fp64 U [len(rows), R]; X may be wider than K = W_hi.shape[1] (a column slice of a wider buffer)."""
    K = W_hi.shape[1]
    return X[rows, :K].double() @ (W_hi.double() + W_lo.double()).t()


def ext_image(U32, group_R, group_stride, ld_ext, fill=CANARY_BF16):
    M, R = U32.shape
    assert R % group_R == 0 and ld_ext >= (R // group_R - 1) * group_stride + 3 * group_R
    hi, lo = split(U32)
    img = torch.full((M, ld_ext), fill, dtype=torch.int16).view(BF)
    j = torch.arange(R)
    col = (j // group_R) * group_stride + j % group_R
    img[:, col] = hi
    img[:, col + group_R] = lo
    img[:, col + 2 * group_R] = hi
    return img


def ut_image(U32, ld_ut, fill=CANARY_BF16):
    M, R = U32.shape
    assert ld_ut >= M
    hi, lo = split(U32)
    out = []
    for t in (hi, lo):
        img = torch.full((R, ld_ut), fill, dtype=torch.int16).view(BF)
        img[:, :M] = t.t()
        out.append(img)
    return out[0], out[1]


def grad_ref(Vt_hi, Vt_lo, X, rows, group_R, r_valid):
    """fp64 [r_valid, K] per group; Vt [R, >= M] (columns beyond M = len(rows) are ignored), X [*, K]."""
    M = rows.numel()
    R = Vt_hi.shape[0]
    assert R % group_R == 0 and r_valid <= group_R
    V = Vt_hi[:, :M].double() + Vt_lo[:, :M].double()
    full = V @ X[rows].double()
    return [full[g * group_R:g * group_R + r_valid] for g in range(R // group_R)]


def pack_ref(A, B, r, Rp, Kext, scale):
    """A fp32 [r, K], B fp32 [N, r] -> dict of the four images (A_hi, A_lo), (Bt_hi, Bt_lo), We, WeT (bf16, tight)."""
    K, N = A.shape[1], B.shape[0]
    assert A.shape[0] == r and B.shape[1] == r and r <= Rp and Rp % 16 == 0 and Kext >= 3 * Rp
    Ap = torch.zeros(Rp, K, dtype=torch.float32)
    Ap[:r] = A
    Bp = torch.zeros(Rp, N, dtype=torch.float32)
    Bp[:r] = (torch.tensor(scale, dtype=torch.float32) * B).t()
    A_hi, A_lo = split(Ap)
    Bt_hi, Bt_lo = split(Bp)
    zero = lambda n: torch.zeros(n, Kext - 3 * Rp, dtype=BF)   # noqa: E731
    We = torch.cat([Bt_hi.t(), Bt_hi.t(), Bt_lo.t(), zero(N)], dim=1).contiguous()
    WeT = torch.cat([A_hi.t(), A_hi.t(), A_lo.t(), zero(K)], dim=1).contiguous()
    return dict(A_hi=A_hi, A_lo=A_lo, Bt_hi=Bt_hi, Bt_lo=Bt_lo, We=We, WeT=WeT)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rand_case(seed, x_shape, w_shape, w_scale=0.1):
    """(X bf16 x_shape, hi, lo bf16 w_shape): Gaussian X, the bf16 split of a Gaussian fp32 matrix of scale w_scale."""
    g = _gen(seed)
    X = torch.randn(*x_shape, generator=g).to(BF)
    hi, lo = split(torch.randn(*w_shape, generator=g) * w_scale)
    return X, hi, lo


def exact_ints(g, shape, scale=1.0):
    return (torch.randint(-2, 3, shape, generator=g).float() * scale)


def exact_case(seed, x_shape, w_shape):
    """(X, hi, lo): integers in [-2, 2], integers in [-2, 2], integers in [-2, 2] times 2^-4 -- see the module docstring."""
    g = _gen(seed)
    X = exact_ints(g, x_shape).to(BF)
    hi = exact_ints(g, w_shape).to(BF)
    lo = exact_ints(g, w_shape, 2.0 ** -4).to(BF)
    return X, hi, lo
