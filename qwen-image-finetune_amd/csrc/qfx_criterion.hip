// qfx_criterion.hip -- the general flow-matching criterion, see include/qfx.h: per-sample weights (diffusers'
// compute_loss_weighting_for_sd3), per-token weights (edit mask / attention mask), L2 or kohya's pseudo-Huber / smooth-L1 with a
// per-sample threshold, the loss of every sample beside the mean.  Two launches: criterion_kernel streams pred / target once, writes
// dpred and one fp64 partial sum per (sample, chunk of rows) into the caller's workspace; criterion_finish_kernel adds the partials
// in chunk order, then the samples in sample order.  No floating-point atomics: same inputs -> same bits.  The gradient's sequence
// of fp32 roundings is the specification (tests/criterion_ref.py restates it): the file is compiled without FMA contraction (the
// pragma below and -ffp-contract=off in the build), with the correctly rounded fp32 divide and square root hipcc emits by default.
#include "qfx_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CRIT_THREADS = 256;
constexpr int CRIT_CHUNK_ELEMS = 2048;      // one 16-byte access per lane and chunk at C % 8 == 0
constexpr int CRIT_MAX_BLOCKS = 256;        // one workgroup per CU; more (sample, chunk) items than that go by stride
constexpr int CRIT_FIN_TILE = 1024;         // partials the finishing block stages in LDS per round

// rows of one sample per chunk: ~CRIT_CHUNK_ELEMS elements, whole rows (a row's token weight is read by the chunk that owns it)
inline int crit_rows_per_chunk(int C) { return C >= CRIT_CHUNK_ELEMS ? 1 : CRIT_CHUNK_ELEMS / C; }
inline int64_t crit_chunks(int rows, int C) { const int rpc = crit_rows_per_chunk(C); return ((int64_t)rows + rpc - 1) / rpc; }

__device__ __forceinline__ void ld8f(const bf16_t* p, float (&v)[8]) {
  const u32x4 u = *(const u32x4*)p;
#pragma unroll
  for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(u[i] << 16); v[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u); }
}

// one element: rho (into the loss) and rho' (into the gradient) of d = pred - target; c = the sample's threshold, c2 = c * c
template <int KIND>
__device__ __forceinline__ void crit_elem(float d, float c, float c2, float& rho, float& drho) {
  if (KIND == QFX_LOSS_L2) {
    rho = d * d;
    drho = 2.0f * d;
  } else {
    const float dd = d * d;
    const float r = sqrtf(dd + c2);
    const float q = dd / (r + c);             // = r - c without the cancellation at |d| << c
    if (KIND == QFX_LOSS_HUBER) {
      const float c2x = 2.0f * c;
      rho = c2x * q;
      drho = (c2x * d) / r;
    } else {
      rho = 2.0f * q;
      drho = (2.0f * d) / r;
    }
  }
}

// the gradient's factors, left to right as qfx.h states them
__device__ __forceinline__ float crit_grad(float drho, float sw, float tw, float inv_c, float inv_denom, float gscale) {
  return drho * sw * tw * inv_c * inv_denom * gscale;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// item = (sample, chunk of rpc rows of S_all); the rows of a chunk are contiguous in pred, dpred and (below S_t) target.
// VEC: C % 8 == 0 and 16-byte aligned pred / target / dpred -> eight elements per lane and access; scalar otherwise.
template <bool VEC, int KIND>
__global__ __launch_bounds__(CRIT_THREADS) void criterion_kernel(const bf16_t* __restrict__ pred, const bf16_t* __restrict__ target,
                                                                 const float* __restrict__ sample_w, const float* __restrict__ token_w,
                                                                 const float* __restrict__ huber_c, bf16_t* __restrict__ dpred,
                                                                 double* __restrict__ partial, int B, int S_all, int S_t, int C, int rpc,
                                                                 int nchunk_all, int nchunk_t, float inv_c, float inv_denom, float gscale) {
  __shared__ double red[CRIT_THREADS / 64];
  const int64_t items = (int64_t)B * nchunk_all;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int b = (int)(item / nchunk_all), chunk = (int)(item - (int64_t)b * nchunk_all);
    const int r0 = chunk * rpc;
    const int rows = min(rpc, S_all - r0);
    const int n_e = rows * C;                                   // <= max(CRIT_CHUNK_ELEMS, C)
    const int64_t p_off = ((int64_t)b * S_all + r0) * C, t_off = ((int64_t)b * S_t + r0) * C;
    const float sw = sample_w ? sample_w[b] : 1.0f;
    const float c = KIND == QFX_LOSS_L2 ? 0.f : huber_c[b];
    const float c2 = c * c;
    double acc = 0.0;
    if (VEC) {
      for (int e = threadIdx.x * 8; e < n_e; e += CRIT_THREADS * 8) {
        const int row = r0 + e / C;
        float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (row < S_t) {
          const float tw = token_w ? token_w[(int64_t)b * S_t + row] : 1.0f;
          float pv[8], tv[8];
          ld8f(pred + p_off + e, pv);
          ld8f(target + t_off + e, tv);
          double s8 = 0.0;
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            float rho, drho;
            crit_elem<KIND>(pv[k] - tv[k], c, c2, rho, drho);
            s8 += (double)rho;
            g[k] = crit_grad(drho, sw, tw, inv_c, inv_denom, gscale);
          }
          acc += (double)tw * s8;
        }
        if (dpred) {
          u32x4 u;
#pragma unroll
          for (int i = 0; i < 4; ++i) u[i] = pack2bf(g[2 * i], g[2 * i + 1]);
          *(u32x4*)(dpred + p_off + e) = u;
        }
      }
    } else {
      for (int e = threadIdx.x; e < n_e; e += CRIT_THREADS) {
        const int row = r0 + e / C;
        float g = 0.f;
        if (row < S_t) {
          const float tw = token_w ? token_w[(int64_t)b * S_t + row] : 1.0f;
          float rho, drho;
          crit_elem<KIND>(bf2f(pred[p_off + e]) - bf2f(target[t_off + e]), c, c2, rho, drho);
          acc += (double)tw * (double)rho;
          g = crit_grad(drho, sw, tw, inv_c, inv_denom, gscale);
        }
        if (dpred) dpred[p_off + e] = f2bf(g);
      }
    }
    if (chunk < nchunk_t) {                                     // block-uniform: the chunks that hold rows below S_t
      acc = wave_sum_f64(acc);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
      __syncthreads();
      if (threadIdx.x == 0) partial[(int64_t)b * nchunk_t + chunk] = ((red[0] + red[1]) + red[2]) + red[3];
      __syncthreads();                                          // red is written again by the next item
    }
  }
}

// ONE block: per sample the partials in chunk order (staged through LDS, added by one lane), then the samples in sample order.
__global__ __launch_bounds__(CRIT_THREADS) void criterion_finish_kernel(const double* __restrict__ partial,
                                                                        const float* __restrict__ sample_w, float* __restrict__ loss,
                                                                        float* __restrict__ loss_per_sample, int B, int nchunk_t,
                                                                        double scale) {
  __shared__ double tile[CRIT_FIN_TILE];
  float total = 0.f;
  for (int b = 0; b < B; ++b) {
    double acc = 0.0;
    for (int base = 0; base < nchunk_t; base += CRIT_FIN_TILE) {
      const int n = min(CRIT_FIN_TILE, nchunk_t - base);
      for (int i = threadIdx.x; i < n; i += CRIT_THREADS) tile[i] = partial[(int64_t)b * nchunk_t + base + i];
      __syncthreads();
      if (threadIdx.x == 0)
        for (int i = 0; i < n; ++i) acc += tile[i];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const float lps = (float)(acc * scale);
      if (loss_per_sample) loss_per_sample[b] = lps;
      total += (sample_w ? sample_w[b] : 1.0f) * lps;
    }
  }
  if (threadIdx.x == 0) *loss = total / (float)B;
}

template <bool VEC>
void criterion_launch(int kind, int blocks, hipStream_t st, const qfx_criterion_args* a, int rpc, int nchunk_all, int nchunk_t,
                      float inv_c) {
#define QFX_CRIT(KIND_)                                                                                                              \
  hipLaunchKernelGGL((criterion_kernel<VEC, KIND_>), dim3(blocks), dim3(CRIT_THREADS), 0, st, a->pred, a->target, a->sample_w,       \
                     a->token_w, a->huber_c, a->dpred, (double*)a->workspace, a->B, a->S_all, a->S_t, a->C, rpc, nchunk_all, nchunk_t, \
                     inv_c, a->inv_denom, a->gscale)
  switch (kind) {
    case QFX_LOSS_L2: QFX_CRIT(QFX_LOSS_L2); break;
    case QFX_LOSS_HUBER: QFX_CRIT(QFX_LOSS_HUBER); break;
    default: QFX_CRIT(QFX_LOSS_SMOOTH_L1); break;
  }
#undef QFX_CRIT
}

}  // namespace

extern "C" int64_t qfx_criterion_workspace_bytes(int32_t B, int32_t S_t, int32_t C) {
  if (B <= 0 || S_t <= 0 || C <= 0) return 0;
  return (int64_t)B * crit_chunks(S_t, C) * (int64_t)sizeof(double);
}

extern "C" int qfx_criterion_fwd_bwd(const qfx_criterion_args* a, void* stream) {
  if (!a || !a->pred || !a->target || !a->loss || !a->workspace) return QFX_EINVAL;
  if (a->B <= 0 || a->S_all <= 0 || a->S_t <= 0 || a->S_t > a->S_all || a->C <= 0) return QFX_EINVAL;
  if (a->kind != QFX_LOSS_L2 && a->kind != QFX_LOSS_HUBER && a->kind != QFX_LOSS_SMOOTH_L1) return QFX_EINVAL;
  if (a->kind != QFX_LOSS_L2 && !a->huber_c) return QFX_EINVAL;
  if (a->workspace_bytes < qfx_criterion_workspace_bytes(a->B, a->S_t, a->C) || ((uintptr_t)a->workspace & 7)) return QFX_EINVAL;
  const int rpc = crit_rows_per_chunk(a->C);
  const int64_t nchunk_all = crit_chunks(a->S_all, a->C), nchunk_t = crit_chunks(a->S_t, a->C);
  const int64_t items = (int64_t)a->B * nchunk_all;
  const int blocks = (int)(items < CRIT_MAX_BLOCKS ? items : CRIT_MAX_BLOCKS);
  const float inv_c = 1.0f / (float)a->C;
  const bool vec = a->C % 8 == 0 && (((uintptr_t)a->pred | (uintptr_t)a->target | (uintptr_t)a->dpred) & 15) == 0;
  hipStream_t st = (hipStream_t)stream;
  if (vec) criterion_launch<true>(a->kind, blocks, st, a, rpc, (int)nchunk_all, (int)nchunk_t, inv_c);
  else     criterion_launch<false>(a->kind, blocks, st, a, rpc, (int)nchunk_all, (int)nchunk_t, inv_c);
  QFX_CHECK_LAUNCH();
  // loss_per_sample[b] = B * inv_denom * (1/C) * sum_s token_w * sum_c rho: the three factors meet in fp64, one rounding to fp32
  const double scale = (double)a->B * (double)a->inv_denom * (double)inv_c;
  hipLaunchKernelGGL(criterion_finish_kernel, dim3(1), dim3(CRIT_THREADS), 0, st, (const double*)a->workspace, a->sample_w, a->loss,
                     a->loss_per_sample, a->B, (int)nchunk_t, scale);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
