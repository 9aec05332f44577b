// qfx_adapter_stats.hip -- per-adapter training telemetry over the flat LoRA buffers (include/qfx.h): for every tensor of a device
// table the squared norms of its clipped gradient, of its weights and of the last optimizer update, the gradient's largest
// magnitude and the number of non-finite elements.  Two launches bracket the optimizer's: phase 0 reads g (and copies p to prev,
// in the same sweep), phase 1 reads p and prev.  One 256-lane workgroup per table entry, as qfx_adafactor.hip and qfx_maxnorm.hip
// walk their tables; nothing crosses a workgroup, no atomics: same inputs -> same bits.
//
// Order of every sum, the same on the 16-byte and on the scalar path: lane L owns the elements i = L (mod 256) of the tensor and
// adds their squares in index order (one fp32 multiply, one fp32 add: the file is built without FMA contraction); an xor-shuffle
// tree folds the 64 lanes of a wave; the four wave sums are folded through LDS as (w0 + w1) + (w2 + w3) (block_sum, qfx_optim.h).
// A 16-byte load hands a lane four CONSECUTIVE elements, which belong to four other lanes: the 16-byte path therefore stages each
// pass of 1024 elements through LDS (written as loaded, read back with stride 256), two tiles in turn so that one barrier per pass
// is enough.  What does not depend on an order -- the maximum, the counts, the snapshot copy -- is done on the values as loaded.
// An element that is not finite counts as 0 in the sums (adding +0 to a sum of squares changes no bit) and is skipped by the maximum.
#include "qfx_common.h"
#include "qfx_optim.h"      // opt_clip, block_sum, wave_max

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                 // four waves
constexpr int PASS = 4 * NT;            // elements of one 16-byte pass of the workgroup
constexpr int GRID_CAP = 4096;          // workgroups; more entries than this are walked by stride

__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__device__ __forceinline__ int block_count(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float finite_or_zero(float x) { return __builtin_isfinite(x) ? x : 0.f; }

// PHASE 0: sum of g'^2, max |g'|, the number of non-finite g' with g' = g * clip; prev = p.
// PHASE 1: sum of p^2, the number of non-finite p, sum of (p - prev)^2.
template <int PHASE>
__global__ __launch_bounds__(NT) void adapter_stats_kernel(const float* __restrict__ p, const float* __restrict__ g, float* prev,
                                                           const qfx_stats_entry* __restrict__ table, int n_entries,
                                                           qfx_stats_row* __restrict__ out, const float* __restrict__ gnorm_sq,
                                                           float max_norm, float grad_scale) {
  __shared__ __attribute__((aligned(16))) float tile[2][2][PASS];      // [turn][value][element of the pass]
  __shared__ float redf[4];
  __shared__ int redi[4];
  const int tid = threadIdx.x;
  const float clip = PHASE == 0 ? opt_clip(gnorm_sq, max_norm, grad_scale) : 1.0f;
  for (int ei = blockIdx.x; ei < n_entries; ei += gridDim.x) {
    const qfx_stats_entry t = table[ei];
    qfx_stats_row* row = out + ei;
    if (t.numel <= 0 || t.off < 0) {             // as the max-norm table: what a builder would refuse is never touched
      if (tid == 0) {
        if (PHASE == 0) {
          row->grad_sq = 0.f; row->grad_absmax = 0.f; row->grad_nonfinite = 0; row->r0 = 0.f; row->r1 = 0.f;
        }
        row->weight_sq = 0.f; row->update_sq = 0.f; row->weight_nonfinite = 0;
      }
      continue;
    }
    const int n = t.numel;
    const float* pe = p + t.off;
    const float* ge = PHASE == 0 ? g + t.off : nullptr;
    float* qe = prev + t.off;
    const bool vec = ((((uintptr_t)pe | (uintptr_t)qe) & 15) == 0) && (PHASE != 0 || ((uintptr_t)ge & 15) == 0);
    float s0 = 0.f, s1 = 0.f, amax = 0.f;
    int bad = 0;

    const int npass = vec ? n / PASS : 0;        // uniform over the workgroup: every lane reaches the barriers
    for (int c = 0; c < npass; ++c) {
      const int64_t base = (int64_t)c * PASS + 4 * tid;
      float* T0 = tile[c & 1][0];
      float* T1 = tile[c & 1][1];
      if (PHASE == 0) {
        const f32x4 gv = *reinterpret_cast<const f32x4*>(ge + base);
        *reinterpret_cast<f32x4*>(qe + base) = *reinterpret_cast<const f32x4*>(pe + base);
        f32x4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float gi = gv[j] * clip;
          const bool ok = __builtin_isfinite(gi);
          bad += !ok;
          if (ok) amax = fmaxf(amax, fabsf(gi));
          w[j] = ok ? gi : 0.f;
        }
        *reinterpret_cast<f32x4*>(T0 + 4 * tid) = w;
      } else {
        const f32x4 pv = *reinterpret_cast<const f32x4*>(pe + base);
        const f32x4 qv = *reinterpret_cast<const f32x4*>(qe + base);
        f32x4 w, d;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bad += !__builtin_isfinite(pv[j]);
          w[j] = finite_or_zero(pv[j]);
          d[j] = finite_or_zero(pv[j] - qv[j]);
        }
        *reinterpret_cast<f32x4*>(T0 + 4 * tid) = w;
        *reinterpret_cast<f32x4*>(T1 + 4 * tid) = d;
      }
      __syncthreads();                           // the tile of this turn is complete; the other turn's was read before this barrier
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float a = T0[s * NT + tid];
        s0 += a * a;
        if (PHASE == 1) {
          const float b = T1[s * NT + tid];
          s1 += b * b;
        }
      }
    }
    // the scalar path: the whole tensor without 16-byte alignment, else what is left behind the last whole pass
    for (int64_t i = (int64_t)npass * PASS + tid; i < n; i += NT) {
      if (PHASE == 0) {
        qe[i] = pe[i];
        const float gi = ge[i] * clip;
        const bool ok = __builtin_isfinite(gi);
        bad += !ok;
        if (ok) amax = fmaxf(amax, fabsf(gi));
        const float a = ok ? gi : 0.f;
        s0 += a * a;
      } else {
        const float pi = pe[i];
        bad += !__builtin_isfinite(pi);
        const float a = finite_or_zero(pi), b = finite_or_zero(pi - qe[i]);
        s0 += a * a;
        s1 += b * b;
      }
    }

    const float sum0 = block_sum(s0, redf);
    const int nbad = block_count(bad, redi);
    if (PHASE == 0) {
      const float mx = block_max(amax, redf);
      if (tid == 0) {                            // the whole row: the phase-1 fields and the reserved ones start from 0
        row->grad_sq = sum0; row->weight_sq = 0.f; row->update_sq = 0.f; row->grad_absmax = mx;
        row->grad_nonfinite = nbad; row->weight_nonfinite = 0; row->r0 = 0.f; row->r1 = 0.f;
      }
    } else {
      const float sum1 = block_sum(s1, redf);
      if (tid == 0) {
        row->weight_sq = sum0; row->update_sq = sum1; row->weight_nonfinite = nbad;
      }
    }
  }
}

}  // namespace

extern "C" int qfx_adapter_stats(const float* p, const float* g, float* prev, const qfx_stats_entry* table, int32_t n_entries,
                                 qfx_stats_row* out, int32_t phase, const float* gnorm_sq, float max_norm, float grad_scale,
                                 void* stream) {
  if (!p || !table || !out || !prev || n_entries <= 0) return QFX_EINVAL;
  if (phase != 0 && phase != 1) return QFX_EINVAL;
  if (phase == 0 && !g) return QFX_EINVAL;
  if (!(max_norm >= 0.f) || !__builtin_isfinite(grad_scale)) return QFX_EINVAL;      // a NaN max_norm fails
  const unsigned wgs = (unsigned)(n_entries < GRID_CAP ? n_entries : GRID_CAP);
  hipStream_t s = (hipStream_t)stream;
  if (phase == 0)
    hipLaunchKernelGGL(adapter_stats_kernel<0>, dim3(wgs), dim3(NT), 0, s, p, g, prev, table, n_entries, out, gnorm_sq, max_norm, grad_scale);
  else
    hipLaunchKernelGGL(adapter_stats_kernel<1>, dim3(wgs), dim3(NT), 0, s, p, g, prev, table, n_entries, out, gnorm_sq, max_norm, grad_scale);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
