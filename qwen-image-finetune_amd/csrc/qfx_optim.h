// What the fused optimizer kernels share: the gradient-clip prologue, the blockwise 8-bit tile helpers (bitsandbytes' state layout,
// include/qfx.h) and the grid policies.  Include after qfx_common.h.  Helpers only, and NO fp-contract pragma: contraction is
// lexical, so a helper rounds as the translation unit that includes it is built (-ffp-contract=off for qfx_adam8bit.hip,
// qfx_lion.hip, qfx_muon.hip and qfx_schedulefree.hip; the compiler's default for qfx_optim.hip and qfx_adafactor.hip), which is
// what each family's restatement under tests/ expects of it.
#pragma once
#include "qfx_common.h"

namespace {      // file-local in every translation unit: each unit's copy rounds as that unit is built

// clip = grad_scale * min(1, max_norm / (||g|| grad_scale + 1e-6)); grad_scale alone without a norm or with max_norm <= 0
__device__ __forceinline__ float opt_clip(const float* __restrict__ gnorm_sq, float max_norm, float grad_scale) {
  float clip = grad_scale;
  if (gnorm_sq != nullptr && max_norm > 0.f) {
    const float nrm = sqrtf(*gnorm_sq) * grad_scale;
    const float c = max_norm / (nrm + 1e-6f);
    clip *= c < 1.0f ? c : 1.0f;
  }
  return clip;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// sum over the 256 threads of a workgroup, the same bits on every thread (qfx_adafactor.hip, qfx_came.hip).  `red` (4 floats of
// LDS) may still be read by the previous call: barrier first.
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// number of midpoints below x (mid[255] = +inf): the nearest code, a tie (x == midpoint) going to the lower one
__device__ __forceinline__ int nearest_code(const float* mid, float x) {
  int c = 0;
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) c += (x > mid[c + s - 1]) ? s : 0;
  return c;
}

// E elements of one lane starting at element `base` of p / g / a moment / the codes, n of them valid (n may be < E or <= 0)
template <int E>
__device__ __forceinline__ void tile_load(const float* __restrict__ src, int64_t base, int n, float (&x)[E]) {
#pragma unroll
  for (int j = 0; j < E; j += 4) {
    if (n >= j + 4) {
      const f32x4 t = *(const f32x4*)(src + base + j);
      x[j] = t[0]; x[j + 1] = t[1]; x[j + 2] = t[2]; x[j + 3] = t[3];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) x[j + i] = (j + i < n) ? src[base + j + i] : 0.f;
    }
  }
}
template <int E>
__device__ __forceinline__ void tile_store(float* __restrict__ dst, int64_t base, int n, const float (&x)[E]) {
#pragma unroll
  for (int j = 0; j < E; j += 4) {
    if (n >= j + 4) {
      f32x4 t; t[0] = x[j]; t[1] = x[j + 1]; t[2] = x[j + 2]; t[3] = x[j + 3];
      *(f32x4*)(dst + base + j) = t;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) if (j + i < n) dst[base + j + i] = x[j + i];
    }
  }
}
template <int E>
__device__ __forceinline__ void tile_load_codes(const uint8_t* __restrict__ src, int64_t base, int n, int (&c)[E]) {
#pragma unroll
  for (int j = 0; j < E; j += 4) {
    if (n >= j + 4) {
      const uint32_t w = *(const uint32_t*)(src + base + j);
#pragma unroll
      for (int i = 0; i < 4; ++i) c[j + i] = (w >> (8 * i)) & 0xff;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) c[j + i] = (j + i < n) ? src[base + j + i] : 0;
    }
  }
}
template <int E>
__device__ __forceinline__ void tile_store_codes(uint8_t* __restrict__ dst, int64_t base, int n, const int (&c)[E]) {
#pragma unroll
  for (int j = 0; j < E; j += 4) {
    if (n >= j + 4) {     // packed 32-bit vector store
      *(uint32_t*)(dst + base + j) = (uint32_t)c[j] | ((uint32_t)c[j + 1] << 8) | ((uint32_t)c[j + 2] << 16) | ((uint32_t)c[j + 3] << 24);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) if (j + i < n) dst[base + j + i] = (uint8_t)c[j + i];
    }
  }
}

// grid of an elementwise kernel: one workgroup of 256 per 256 units of work, at most `cap`, the rest by stride
inline int flat_grid(int64_t work, int64_t cap) {
  const int64_t b = (work + 255) / 256;
  return (int)(b < cap ? b : cap);
}

// workgroup caps of the one-launch steps: the fp32 elementwise kernels (adamw_kernel's policy) and the blockwise 8-bit kernels
constexpr int64_t FLAT_STEP_CAP = 4096;
constexpr int64_t BLOCKWISE_CAP = 2048;

// grid of a blockwise 8-bit kernel over n_blocks table entries: a wave per entry (blocksize 256) or a workgroup per entry (2048)
inline unsigned blockwise_grid(int64_t n_blocks, int blocksize) {
  const int64_t wgs = blocksize == 256 ? (n_blocks + 3) / 4 : n_blocks;
  return (unsigned)(wgs < BLOCKWISE_CAP ? wgs : BLOCKWISE_CAP);
}

// ---- parameter groups (include/qfx.h): the grouped kernels take their hyperparameter rows by value in the argument block, the
// first n_groups lanes of every workgroup turn them into the family's per-group constants in LDS, and every 64-element tile (fp32
// kernels) or block-table entry (blockwise kernels) names its row with one byte.  An index the builder did not range-check is
// clamped to the rows the launch filled (an entry >= n_groups takes the last row, n_groups - 1), so that it can never read LDS
// outside the table or a row of it that nobody wrote.
template <typename Row>
struct GroupTable { Row g[QFX_MAX_PARAM_GROUPS]; };

template <typename Row>
inline GroupTable<Row> group_table(const Row* groups, int n_groups) {
  GroupTable<Row> t = {};
  for (int i = 0; i < n_groups; ++i) t.g[i] = groups[i];
  return t;
}

__device__ __forceinline__ int group_index(const uint8_t* __restrict__ map, int64_t i, int n_groups) {
  const int gi = map[i];
  return gi < n_groups ? gi : n_groups - 1;      // only rows 0 .. n_groups-1 of the LDS table are filled
}

inline bool groups_count_ok(const void* groups, int n_groups) { return groups != nullptr && n_groups >= 1 && n_groups <= QFX_MAX_PARAM_GROUPS; }
inline bool beta_ok(float b) { return b >= 0.f && b < 1.f; }      // a NaN fails

}  // namespace
