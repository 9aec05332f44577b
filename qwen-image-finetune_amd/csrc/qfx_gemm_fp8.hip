// qfx_gemm_fp8.hip -- low-precision trunk: MX-FP8 (OCP e4m3 elements, E8M0 scale per 32 K-elements) base GEMM on the
// block-scaled MFMA of gfx950 (v_mfma_scale_f32_16x16x128_f8f6f4, twice the bf16 matrix rate) + the quantiser that produces
// its operands.  Same contract as qfx_gemm.hip (bias, bf16 mid-rounding, bf16 LoRA K-extension, epilogues): what holds the two
// to it is shared code.  This file has the quantiser kernel, the shell of the small kernel and the two single-problem entries:
//   gemm_fp8_kernel<EPI>      = gemm_tile_body<EPI, true> of qfx_gemm_tile.h, the 128x128 tile body of the bf16 gemm_kernel<EPI> with
//                               the scale loads and the scaled MFMA on the base K segment (a K tile of 128 fp8 bytes per row is the
//                               SAME LDS image as 64 bf16: staging, fragment reads, LoRA segment, mid-rounding, epilogue are one text);
//   quant_mxfp8_kernel        = amax over the 4 lanes of an MX block + mx_quant8 of qfx_common.h, as in every producer that quantises
//                               on the fly (row kernels, skinny kernels, the quantising epilogue of gemm256_kernel in qfx_gemm.hip);
//   qfx_gemm_mxfp8            = validate_fp8 of qfx_gemm_tile.h (the checks of qfx_gemm_mxfp8_grouped in qfx_gemm.hip, which runs the
//                               large problems on the persistent kernel), then the small kernel.
// Hardware K order of the scaled MFMA's operand (measured, tools/mx_probe): k = (byte/16)*64 + g*16 + byte%16, and the scale supplied
// by lane group g covers hardware k in [32g, 32g+32) = chunks {2g', 2g'+1} of the row with g' = g: i.e. exactly the MX block g of the K
// tile when lane group g holds chunks (g, g+4) ... see the MX-FP8 row of the kernel table in profiles/HISTORY.md section 3.
#include "qfx_gemm_tile.h"

namespace {

// ------------------------------------------------------------------------------------------------ quantiser
// 4 lanes per MX block (8 elements each), 16 blocks per wave-instruction; grid-stride over blocks.
__global__ __launch_bounds__(256) void quant_mxfp8_kernel(const qfx_quant_args a) {
  const int nbk = a.K / 32;
  const int64_t nblocks = (int64_t)a.M * nbk;
  const int sub = threadIdx.x & 3;
  for (int64_t blk = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 2; blk < nblocks; blk += ((int64_t)gridDim.x * 256) >> 2) {
    const int m = (int)(blk / nbk), kb = (int)(blk % nbk);
    const int64_t xr = remap_row(m, a.rows_per_batch, a.x_batch_rows, a.x_row_off);
    const u32x4 u = *(const u32x4*)(a.X + xr * a.ldx + kb * 32 + sub * 8);
    float v[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(u[i] << 16); v[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u); }
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[i]));
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    amax = fmaxf(amax, __shfl_xor(amax, 2));
    int eb;
    *(u32x2*)(a.Q + (int64_t)m * a.ldq + kb * 32 + sub * 8) = mx_quant8(v, amax, eb);
    if (sub == 0) a.S[((int64_t)(kb >> 2) * a.M + m) * 4 + (kb & 3)] = (uint8_t)eb;   // tile-major: [K/128][M][4]
  }
}

// ------------------------------------------------------------------------------------------------ GEMM
template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_fp8_kernel(const qfx_gemm_fp8_args q) {
  gemm_tile_body<EPI, true>(q.g, q.sa, q.sb);
}

}  // namespace

extern "C" int qfx_quant_mxfp8(const qfx_quant_args* a, void* stream) {
  if (!a || !a->X || !a->Q || !a->S) return QFX_EINVAL;
  if (a->M <= 0 || a->K <= 0 || (a->K % 128) || (a->ldx % 8) || (a->ldq % 16) || a->rows_per_batch <= 0) return QFX_EINVAL;
  const int64_t nblocks = (int64_t)a->M * (a->K / 32);
  int64_t grid = (nblocks * 4 + 255) / 256;
  if (grid > 16384) grid = 16384;
  hipLaunchKernelGGL(quant_mxfp8_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, *a);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_gemm_mxfp8(const qfx_gemm_fp8_args* a, void* stream) {
  if (!a) return QFX_EINVAL;
  qfx_gemm_args g;      // the problem in 2-byte units, checked; the small kernel takes *a (byte units)
  const int rc = validate_fp8(*a, g);
  if (rc) return rc;
  // large problems: warp-specialised persistent kernel (256x128 tiles); small ones keep the 128x128 kernel
  const int tiles256 = ((g.M + 255) / 256) * ((g.N + BN - 1) / BN);
  if (tiles256 >= 160 && !g.seg2_plain && ok256(&g)) return qfx_gemm_mxfp8_grouped(a, 1, stream);
  if (a->cq || a->cq_only) return QFX_EUNSUPPORTED;   // the quantising epilogue lives in the persistent kernel only
  const int tiles = ((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN);
  hipStream_t s = (hipStream_t)stream;
  switch (g.epi) {
    case QFX_EPI_NONE: hipLaunchKernelGGL(gemm_fp8_kernel<QFX_EPI_NONE>, dim3(tiles), dim3(256), 0, s, *a); break;
    case QFX_EPI_GELU: hipLaunchKernelGGL(gemm_fp8_kernel<QFX_EPI_GELU>, dim3(tiles), dim3(256), 0, s, *a); break;
    case QFX_EPI_GATE_RES: hipLaunchKernelGGL(gemm_fp8_kernel<QFX_EPI_GATE_RES>, dim3(tiles), dim3(256), 0, s, *a); break;
    default: hipLaunchKernelGGL(gemm_fp8_kernel<QFX_EPI_DGELU>, dim3(tiles), dim3(256), 0, s, *a); break;
  }
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
