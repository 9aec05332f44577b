// qfx_gemm_tile.h -- what the bf16 GEMM (qfx_gemm.hip) and the MX-FP8 GEMM (qfx_gemm_fp8.hip) share: the 128x128 small-tile body
// behind gemm_kernel<EPI> / gemm_fp8_kernel<EPI>, and the host-side argument checks of every GEMM entry.
//
// One K tile is 128 BYTES per row -- 64 bf16 or 128 fp8 -- so both element types have the same LDS image (lane-linear LDS-DMA with
// the bank swizzle chunk' = chunk ^ ((row>>1)&7) on the SOURCE address and again on the ds_read_b128), the same staging and the same
// fragment reads: lane (g = lane>>4, li = lane&15) reads the 16-byte chunks g and g+4 of row li -- two bf16 k-steps, or the two
// halves of ONE scaled-MFMA operand.  Operands are addressed in bytes in both instantiations.
#pragma once
#include "qfx_common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) int v8i32;   // operand of the scaled MFMA (32 fp8 bytes)
constexpr int BM = 128, BN = 128, BK = 64;  // BK: bf16 elements per K tile
constexpr int ROWB = BK * 2;                // bytes per tile row (64 bf16 or 128 fp8)
constexpr int TILE_BYTES = BM * ROWB;       // 16 KiB per operand tile

__device__ __forceinline__ void glds16(const void* g, char* lds) {
  __builtin_amdgcn_global_load_lds((const QFX_AS1 void*)g, (QFX_AS3 void*)lds, 16, 0, 0);
}

// Tile 128x128x(128 bytes), 256 threads = 4 waves (2x2), each wave 64x64 = 4x4 MFMA 16x16 fragments; double buffered, one barrier
// per K tile.  MFMA operands are swapped (D' = B A^T) so each lane ends up with 4 consecutive N for one M row: 8-byte bf16x4
// stores / bias / gate / residual accesses in the epilogue.
// FP8: A1 / B1 are e4m3 bytes (lda1 / ldb1 / K1 in bytes) with tile-major E8M0 scales sa / sb ([K1/128][rows][4]), contracted by
// v_mfma_scale_f32_16x16x128_f8f6f4; A rows are not remapped (the entry refuses a_batch_rows).  The LoRA segment is bf16 in both.
// `p` by VALUE on purpose: taken by reference, hipcc (ROCm 7.2) emits 100-450 more instructions per instantiation.
template <int EPI, bool FP8>
__device__ __forceinline__ void gemm_tile_body(const qfx_gemm_args p, const uint8_t* sa, const uint8_t* sb) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE_BYTES];  // [buf][A|B]
  constexpr int ESZ = FP8 ? 1 : 2;      // bytes per element of the base segment's operands

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 1, wc = w & 1;

  // ---- XCD-aware tile mapping (bijective for any grid size): each XCD walks a contiguous chunk of the tile list
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7, idx = bid >> 3;
  const int swz = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
  const int tiles_m = (p.M + BM - 1) / BM;
  const int m0 = (swz % tiles_m) * BM;
  const int n0 = (swz / tiles_m) * BN;

  // ---- staging addresses: wave w stages rows [w*32, w*32+32) of both tiles, 8 rows x 128 bytes per DMA instruction
  const int srow = lane >> 3, schunk = lane & 7;
  const char* pa[4];
  const char* pb[4];
  int64_t a_row[4], b_row[4];
  int scb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lr = w * 32 + i * 8 + srow;
    scb[i] = (schunk ^ ((lr >> 1) & 7)) * 16;  // source BYTE offset inside the 128-byte K tile row
    int gm = m0 + lr; gm = gm < p.M ? gm : p.M - 1;
    int gn = n0 + lr; gn = gn < p.N ? gn : p.N - 1;
    a_row[i] = gm; b_row[i] = gn;
    int64_t am = gm;
    if constexpr (!FP8) am = remap_row(gm, p.rows_per_batch, p.a_batch_rows, p.a_row_off);
    pa[i] = (const char*)p.A1 + am * p.lda1 * ESZ + scb[i];
    pb[i] = (const char*)p.B1 + (int64_t)gn * p.ldb1 * ESZ + scb[i];
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nt1 = p.K1 * ESZ / ROWB, nt2 = p.K2 / BK, nt = nt1 + nt2;
  const int g = lane >> 4, li = lane & 15;

  auto stage = [&](int t) {
    char* sA = smem + (t & 1) * 2 * TILE_BYTES;
    char* sB = sA + TILE_BYTES;
    const int koff = (t < nt1 ? t : t - nt1) * ROWB;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      glds16(pa[i] + koff, sA + (w * 32 + i * 8) * ROWB);
      glds16(pb[i] + koff, sB + (w * 32 + i * 8) * ROWB);
    }
  };
  // FP8: scales of this lane's fragment rows for K tile t: one dword (4 MX blocks) per row, byte g is this lane group's block
  [[maybe_unused]] const uint8_t* sap[4];
  [[maybe_unused]] const uint8_t* sbp[4];
  [[maybe_unused]] int64_t sa_tile = 0, sb_tile = 0;      // bytes between K tiles of the tile-major scale arrays
  [[maybe_unused]] uint32_t sca[4], scbv[4], scan[4], scbn[4];
  [[maybe_unused]] auto load_scales = [&](int t, uint32_t (&sa_)[4], uint32_t (&sb_)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { sa_[i] = *(const uint32_t*)(sap[i] + t * sa_tile); sb_[i] = *(const uint32_t*)(sbp[i] + t * sb_tile); }
  };
  if constexpr (FP8) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int gm = m0 + wr * 64 + i * 16 + li; gm = gm < p.M ? gm : p.M - 1;
      int gn = n0 + wc * 64 + i * 16 + li; gn = gn < p.N ? gn : p.N - 1;
      sap[i] = sa + (int64_t)gm * 4;
      sbp[i] = sb + (int64_t)gn * 4;
    }
    sa_tile = (int64_t)p.M * 4; sb_tile = (int64_t)p.N * 4;
  }

  stage(0);
  if constexpr (FP8) load_scales(0, sca, scbv);
  __syncthreads();

  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) {
      if (t + 1 == nt1) {  // switch to the bf16 LoRA K segment
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          pa[i] = (const char*)(p.A2 + a_row[i] * p.lda2) + scb[i];
          pb[i] = (const char*)(p.B2 + b_row[i] * p.ldb2) + scb[i];
        }
      }
      stage(t + 1);
      if constexpr (FP8) { if (t + 1 < nt1) load_scales(t + 1, scan, scbn); }
    }
    const char* sA = smem + (t & 1) * 2 * TILE_BYTES;
    const char* sB = sA + TILE_BYTES;
    auto rd = [&](const char* tile, int row, int kk) {
      return *(const bf16x8*)(tile + row * ROWB + (((kk * 4 + g) ^ ((row >> 1) & 7)) << 4));
    };
    auto bf16_ktile = [&]() {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        bf16x8 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = rd(sA, wr * 64 + i * 16 + li, kk);
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = rd(sB, wc * 64 + i * 16 + li, kk);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int ni = 0; ni < 4; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[ni], a[mi], acc[mi][ni], 0, 0, 0);
      }
    };
    if constexpr (FP8) {
      if (t < nt1) {
        v8i32 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bf16x8 a0 = rd(sA, wr * 64 + i * 16 + li, 0), a1 = rd(sA, wr * 64 + i * 16 + li, 1);
          const bf16x8 b0 = rd(sB, wc * 64 + i * 16 + li, 0), b1 = rd(sB, wc * 64 + i * 16 + li, 1);
          const u32x4 a0u = __builtin_bit_cast(u32x4, a0), a1u = __builtin_bit_cast(u32x4, a1);
          const u32x4 b0u = __builtin_bit_cast(u32x4, b0), b1u = __builtin_bit_cast(u32x4, b1);
#pragma unroll
          for (int j = 0; j < 4; ++j) { a[i][j] = (int)a0u[j]; a[i][4 + j] = (int)a1u[j]; b[i][j] = (int)b0u[j]; b[i][4 + j] = (int)b1u[j]; }
        }
        int sav[4], sbv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { sav[i] = (int)((sca[i] >> (8 * g)) & 0xffu); sbv[i] = (int)((scbv[i] >> (8 * g)) & 0xffu); }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int ni = 0; ni < 4; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(b[ni], a[mi], acc[mi][ni], 0, 0, 0, sbv[ni], 0, sav[mi]);
#pragma unroll
        for (int i = 0; i < 4; ++i) { sca[i] = scan[i]; scbv[i] = scbn[i]; }
      } else {
        bf16_ktile();
      }
    } else {
      bf16_ktile();
    }
    if (nt2 > 0 && !p.seg2_plain && t == nt1 - 1) {
      // base nn.Linear output is a bf16 tensor in the reference: round (acc + bias) before the LoRA add
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const int n = n0 + wc * 64 + ni * 16 + 4 * g;
        float bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (p.bias != nullptr && n + 3 < p.N) {
          const bf16x4 bb = *(const bf16x4*)(p.bias + n);
#pragma unroll
          for (int r = 0; r < 4; ++r) bv[r] = bf2f((bf16_t)bb[r]);
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[mi][ni][r] = rbf(acc[mi][ni][r] + bv[r]);
      }
    }
    __syncthreads();
  }

  // ---- epilogue: lane holds C[m = ..+li][n = ..+4g+r], r=0..3
  const bool bias_pending = (p.bias != nullptr) && (nt2 == 0 || p.seg2_plain);
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int m = m0 + wr * 64 + mi * 16 + li;
    if (m >= p.M) continue;
    const int bidx = m / p.rows_per_batch;
    const int64_t crow = remap_row(m, p.rows_per_batch, p.c_batch_rows, p.c_row_off);
    const bool keep = p.row_mask == nullptr || p.row_mask[m] != 0.f;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int n = n0 + wc * 64 + ni * 16 + 4 * g;
      if (n + 3 >= p.N) continue;
      if (!keep) {
        const bf16x4 z = {0, 0, 0, 0};
        *(bf16x4*)(p.C + crow * p.ldc + n) = z;
        if constexpr (EPI == QFX_EPI_GELU) *(bf16x4*)(p.C2 + crow * p.ldc2 + n) = z;
        if constexpr (EPI == QFX_EPI_GATE_RES) { if (p.C2) *(bf16x4*)(p.C2 + (int64_t)m * p.ldc2 + n) = z; }
        continue;
      }
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[mi][ni][r];
      if (bias_pending) {
        const bf16x4 bb = *(const bf16x4*)(p.bias + n);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += bf2f((bf16_t)bb[r]);
      }
      bf16x4 o;
      if constexpr (EPI == QFX_EPI_NONE) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (short)f2bf(v[r]);
        *(bf16x4*)(p.C + crow * p.ldc + n) = o;
      } else if constexpr (EPI == QFX_EPI_GELU) {
        bf16x4 o2;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bf16_t h = f2bf(v[r]);
          o[r] = (short)h;
          o2[r] = (short)f2bf(gelu_tanh_f(bf2f(h)));
        }
        *(bf16x4*)(p.C + crow * p.ldc + n) = o;
        *(bf16x4*)(p.C2 + crow * p.ldc2 + n) = o2;
      } else if constexpr (EPI == QFX_EPI_GATE_RES) {
        const bf16x4 gt = *(const bf16x4*)(p.gate + (int64_t)bidx * p.gate_bstride + n);
        const bf16x4 rs = *(const bf16x4*)(p.aux + (p.aux_unmapped ? (int64_t)m : crow) * p.ldaux + n);
        bf16x4 yo;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float y = rbf(v[r]);
          yo[r] = (short)f2bf(y);
          const float gy = rbf(bf2f((bf16_t)gt[r]) * y);
          o[r] = (short)f2bf(bf2f((bf16_t)rs[r]) + gy);
        }
        *(bf16x4*)(p.C + crow * p.ldc + n) = o;
        if (p.C2) *(bf16x4*)(p.C2 + (int64_t)m * p.ldc2 + n) = yo;   // pre-gate linear output (rows UNMAPPED), kept for d(gate)
      } else {  // QFX_EPI_DGELU
        const bf16x4 hx = *(const bf16x4*)(p.aux + (p.aux_unmapped ? (int64_t)m : crow) * p.ldaux + n);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float y = rbf(v[r]);
          o[r] = (short)f2bf(y * gelu_tanh_grad_f(bf2f((bf16_t)hx[r])));
        }
        *(bf16x4*)(p.C + crow * p.ldc + n) = o;
      }
    }
  }
}

// ---- host-side argument checks, shared by every GEMM entry ---------------------------------------------------------------
// 16-byte epilogue accesses of the persistent kernel (gemm256_kernel)
inline bool ok256(const qfx_gemm_args* a) {
  if ((a->N % 8) || (a->ldc % 8)) return false;
  if (a->epi == QFX_EPI_GELU && (a->ldc2 % 8)) return false;
  if (a->epi == QFX_EPI_GATE_RES && a->C2 && (a->ldc2 % 8)) return false;
  if ((a->epi == QFX_EPI_GATE_RES || a->epi == QFX_EPI_DGELU) && (a->ldaux % 8)) return false;
  if (a->epi == QFX_EPI_GATE_RES && (a->gate_bstride % 8)) return false;
  return true;
}

inline int validate(const qfx_gemm_args* a) {
  if (!a->A1 || !a->B1 || !a->C) return QFX_EINVAL;
  if (a->M <= 0 || a->N <= 0 || a->K1 <= 0 || (a->K1 % BK) != 0 || (a->K2 % BK) != 0 || a->K2 < 0) return QFX_EINVAL;
  if ((a->N % 4) != 0 || (a->lda1 % 8) || (a->ldb1 % 8) || (a->ldc % 4)) return QFX_EINVAL;
  if (a->K2 > 0 && (!a->A2 || !a->B2 || (a->lda2 % 8) || (a->ldb2 % 8))) return QFX_EINVAL;
  if (a->rows_per_batch <= 0) return QFX_EINVAL;
  if (a->epi == QFX_EPI_GELU && (!a->C2 || (a->ldc2 % 4))) return QFX_EINVAL;
  if (a->epi == QFX_EPI_GATE_RES && (!a->gate || !a->aux || (a->ldaux % 4))) return QFX_EINVAL;
  if (a->epi == QFX_EPI_DGELU && (!a->aux || (a->ldaux % 4))) return QFX_EINVAL;
  if (a->epi < 0 || a->epi > 3) return QFX_EUNSUPPORTED;
  return QFX_OK;
}

// An MX-FP8 problem as the checked bf16-shaped problem `g`: lda1 / ldb1 / K1 in 2-byte units (a 128-byte fp8 K tile is a 64-element
// bf16 K tile until it reaches the matrix pipe), so that validate() / ok256() and the persistent kernel's loaders apply as they are.
// Every QFX_EINVAL arm comes before validate()'s QFX_EUNSUPPORTED (epi out of range), in either entry.
inline int validate_fp8(const qfx_gemm_fp8_args& f, qfx_gemm_args& g) {
  g = f.g;
  if (!f.sa || !f.sb || (g.K1 % 128) || (g.lda1 % 16) || (g.ldb1 % 16) || g.a_batch_rows != 0) return QFX_EINVAL;
  g.lda1 /= 2; g.ldb1 /= 2; g.K1 /= 2;
  return validate(&g);
}

}  // namespace
