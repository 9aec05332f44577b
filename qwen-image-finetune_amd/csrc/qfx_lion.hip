// qfx_lion.hip -- Lion (Chen et al. 2023; lion_pytorch.Lion, bitsandbytes.optim.Lion / Lion8bit) over the flat LoRA buffers, see
// include/qfx.h.  Two entry points, ONE launch each: qfx_lion_step keeps the single moment in fp32 (20 B of traffic per element: p
// and m read and written, g read), qfx_lion8bit_step keeps it as blockwise 8-bit codes in bitsandbytes' layout and is driven by the
// block table of qfx_adam8bit_step.  Both are elementwise apart from the block maximum; no atomics, same inputs -> same bits.
// The update is the SIGN of c = m b1 + (1 - b1) g': the whole file is compiled without FMA contraction (the pragma below and
// -ffp-contract=off in the build), so every product and sum is rounded where tests/lion_ref.py rounds it and a near-cancelling c
// gets the restatement's sign.  Plain * and + only: the __fmul_rn / __fadd_rn wrappers are inlined from a header compiled WITH
// contraction and fuse again.
#include "qfx_common.h"
#include "qfx_optim.h"

#pragma clang fp contract(off)

namespace {

struct LionConst { float b1, b2, omb1, omb2, lr, decay, clip; int wd; };

__device__ __forceinline__ LionConst lion_const(float lr, float b1, float b2, float wd, float clip) {
  LionConst k;
  k.b1 = b1; k.b2 = b2; k.omb1 = 1.0f - b1; k.omb2 = 1.0f - b2;
  k.lr = lr; k.wd = wd > 0.f; k.decay = 1.0f - lr * wd; k.clip = clip;
  return k;
}

// one element: m in (fp32 or decoded), out updated; p decayed (decoupled, first) and moved by lr against the sign of c
__device__ __forceinline__ void lion_elem(float& p, float g, float& m, const LionConst& k) {
  const float gs = g * k.clip;
  if (!__builtin_isfinite(gs)) return;
  const float c = m * k.b1 + k.omb1 * gs;
  if (k.wd) p = p * k.decay;
  const float s = c > 0.f ? 1.0f : (c < 0.f ? -1.0f : 0.f);
  p = p - k.lr * s;
  m = m * k.b2 + k.omb2 * gs;
}

// VEC: p, g, m are 16-byte aligned -> one dwordx4 per buffer and lane; the n % 4 tail (and everything, without VEC) is scalar
template <bool VEC>
__global__ __launch_bounds__(256) void lion_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, int64_t n,
                                                   float lr, float b1, float b2, float wd, const float* __restrict__ gnorm_sq,
                                                   float max_norm, float grad_scale) {
  const LionConst k = lion_const(lr, b1, b2, wd, opt_clip(gnorm_sq, max_norm, grad_scale));
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int64_t nv = VEC ? n / 4 : 0;
  for (int64_t i = tid; i < nv; i += nt) {
    f32x4 pv = *(const f32x4*)(p + 4 * i);
    const f32x4 gv = *(const f32x4*)(g + 4 * i);
    f32x4 mv = *(const f32x4*)(m + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pj = pv[j], mj = mv[j];
      lion_elem(pj, gv[j], mj, k);
      pv[j] = pj; mv[j] = mj;
    }
    *(f32x4*)(p + 4 * i) = pv;
    *(f32x4*)(m + 4 * i) = mv;
  }
  for (int64_t i = 4 * nv + tid; i < n; i += nt) {
    float pi = p[i], mi = m[i];
    lion_elem(pi, g[i], mi, k);
    p[i] = pi; m[i] = mi;
  }
}

// parameter groups: lion_elem with the LionConst of the tile's group, formed by lion_const in LDS at workgroup start
template <bool VEC>
__global__ __launch_bounds__(256) void lion_grouped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           int64_t n, const uint8_t* __restrict__ tile_group,
                                                           const GroupTable<qfx_lion_group> tab, int n_groups,
                                                           const float* __restrict__ gnorm_sq, float max_norm, float grad_scale) {
  __shared__ LionConst ks[QFX_MAX_PARAM_GROUPS];
  if ((int)threadIdx.x < n_groups) {
    const qfx_lion_group q = tab.g[threadIdx.x];
    ks[threadIdx.x] = lion_const(q.lr, q.beta1, q.beta2, q.weight_decay, opt_clip(gnorm_sq, max_norm, grad_scale));
  }
  __syncthreads();
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int64_t nv = VEC ? n / 4 : 0;
  for (int64_t i = tid; i < nv; i += nt) {
    const LionConst k = ks[group_index(tile_group, i >> 4, n_groups)];
    f32x4 pv = *(const f32x4*)(p + 4 * i);
    const f32x4 gv = *(const f32x4*)(g + 4 * i);
    f32x4 mv = *(const f32x4*)(m + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pj = pv[j], mj = mv[j];
      lion_elem(pj, gv[j], mj, k);
      pv[j] = pj; mv[j] = mj;
    }
    *(f32x4*)(p + 4 * i) = pv;
    *(f32x4*)(m + 4 * i) = mv;
  }
  for (int64_t i = 4 * nv + tid; i < n; i += nt) {
    const LionConst k = ks[group_index(tile_group, i >> 6, n_groups)];
    float pi = p[i], mi = m[i];
    lion_elem(pi, g[i], mi, k);
    p[i] = pi; m[i] = mi;
  }
}

// ---- blockwise 8-bit state (the tile helpers of qfx_optim.h, shared with adam8bit_kernel).
// BS = 256: E = 4, a wave per entry (4 entries per workgroup and iteration), the block maximum a cross-lane reduction;
// BS = 2048: E = 8, the workgroup per entry, the maximum through LDS
// GROUPED: the LionConst of every table entry is the one of its group (block_group, one byte per entry; tab: the groups' rows)
template <int BS, bool GROUPED>
__device__ __forceinline__ void lion8bit_body(const qfx_lion8bit_args& a, const uint8_t* __restrict__ block_group,
                                              const GroupTable<qfx_lion_group>* tab, int n_groups) {
  constexpr bool WG = BS > 256;
  constexpr int E = WG ? 8 : 4;
  constexpr int LANES = WG ? 256 : 64;
  static_assert(E * LANES == BS, "tile");
  __shared__ float q1s[256], mid1[256];
  __shared__ float red[2][4];
  const int t = threadIdx.x;
  q1s[t] = a.qmap1[t];
  mid1[t] = t < 255 ? (a.qmap1[t] + a.qmap1[t + 1]) / 2.0f : INFINITY;
  __shared__ LionConst ks[GROUPED ? QFX_MAX_PARAM_GROUPS : 1];
  LionConst k;
  if (GROUPED) {
    if (t < n_groups) {
      const qfx_lion_group q = tab->g[t];
      ks[t] = lion_const(q.lr, q.beta1, q.beta2, q.weight_decay, opt_clip(a.gnorm_sq, a.max_norm, a.grad_scale));
    }
  } else {
    k = lion_const(a.lr, a.beta1, a.beta2, a.weight_decay, opt_clip(a.gnorm_sq, a.max_norm, a.grad_scale));
  }
  __syncthreads();
  const int lane = WG ? t : (t & 63);
  const int64_t first = WG ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + (t >> 6);
  const int64_t stride = WG ? (int64_t)gridDim.x : (int64_t)gridDim.x * 4;
  int parity = 0;
  for (int64_t bi = first; bi < a.n_blocks; bi += stride) {      // WG: bi is uniform over the workgroup, every thread reaches the barrier
    const qfx_adam8bit_block e = a.table[bi];
    if (GROUPED) k = ks[group_index(block_group, bi, n_groups)];
    const int64_t base = e.off + (int64_t)lane * E;
    const int n = e.len - lane * E;
    float p[E], g[E], m[E];
    tile_load<E>(a.p, base, n, p);
    tile_load<E>(a.g, base, n, g);
    if (e.mode == QFX_ADAM8BIT_FP32) {
      const int64_t sb = e.state + (int64_t)lane * E;
      tile_load<E>(a.m32, sb, n, m);
#pragma unroll
      for (int j = 0; j < E; ++j) lion_elem(p[j], g[j], m[j], k);
      tile_store<E>(a.p, base, n, p);
      tile_store<E>(a.m32, sb, n, m);
      continue;
    }
    int c1[E];
    tile_load_codes<E>(a.q1, base, n, c1);
    const float am1 = a.absmax1[e.state];
    float mx1 = 0.f;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      m[j] = q1s[c1[j]] * am1;
      if (j < n) {
        lion_elem(p[j], g[j], m[j], k);
        mx1 = fmaxf(mx1, fabsf(m[j]));
      }
    }
    mx1 = wave_max(mx1);
    if (WG) {
      if ((t & 63) == 0) red[parity][t >> 6] = mx1;
      __syncthreads();
      mx1 = fmaxf(fmaxf(red[parity][0], red[parity][1]), fmaxf(red[parity][2], red[parity][3]));
      parity ^= 1;
    }
    tile_store<E>(a.p, base, n, p);
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const float x1 = mx1 > 0.f ? m[j] / mx1 : 0.f;
      int c = nearest_code(mid1, x1);
      if (mx1 > 0.f && (__builtin_signbit(q1s[c]) != 0) != (__builtin_signbit(m[j]) != 0)) {      // state1 keeps its sign
        c += m[j] > 0.f ? 1 : -1;
        c = c < 0 ? 0 : (c > 255 ? 255 : c);
      }
      c1[j] = c;
    }
    tile_store_codes<E>(a.q1, base, n, c1);
    if (lane == 0) a.absmax1[e.state] = mx1;
  }
}

template <int BS>
__global__ __launch_bounds__(256) void lion8bit_kernel(const qfx_lion8bit_args a) {
  lion8bit_body<BS, false>(a, nullptr, nullptr, 0);
}
template <int BS>
__global__ __launch_bounds__(256) void lion8bit_grouped_kernel(const qfx_lion8bit_args a, const uint8_t* __restrict__ block_group,
                                                               const GroupTable<qfx_lion_group> tab, int n_groups) {
  lion8bit_body<BS, true>(a, block_group, &tab, n_groups);
}

bool lion_scalars_ok(float lr, float beta1, float beta2, float weight_decay) {
  return lr >= 0.f && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && weight_decay >= 0.f;      // a NaN fails each
}

}  // namespace

extern "C" int qfx_lion_step(float* p, const float* g, float* m, int64_t n, float lr, float beta1, float beta2, float weight_decay,
                             const float* gnorm_sq, float max_norm, float grad_scale, void* stream) {
  if (!p || !g || !m || n <= 0 || !lion_scalars_ok(lr, beta1, beta2, weight_decay)) return QFX_EINVAL;
  const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) == 0;
  const int blocks = flat_grid(vec ? (n + 3) / 4 : n, FLAT_STEP_CAP);      // adamw_kernel's grid policy
  if (vec)
    hipLaunchKernelGGL(lion_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, n, lr, beta1, beta2, weight_decay,
                       gnorm_sq, max_norm, grad_scale);
  else
    hipLaunchKernelGGL(lion_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, n, lr, beta1, beta2, weight_decay,
                       gnorm_sq, max_norm, grad_scale);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_lion8bit_step(const qfx_lion8bit_args* a, void* stream) {
  if (!a || !a->p || !a->g || !a->q1 || !a->absmax1 || !a->m32 || !a->table || !a->qmap1) return QFX_EINVAL;
  if ((a->blocksize != 256 && a->blocksize != 2048) || a->n_blocks <= 0) return QFX_EINVAL;
  if (!lion_scalars_ok(a->lr, a->beta1, a->beta2, a->weight_decay)) return QFX_EINVAL;
  const dim3 grid(blockwise_grid(a->n_blocks, a->blocksize));
  if (a->blocksize == 256)
    hipLaunchKernelGGL(lion8bit_kernel<256>, grid, dim3(256), 0, (hipStream_t)stream, *a);
  else
    hipLaunchKernelGGL(lion8bit_kernel<2048>, grid, dim3(256), 0, (hipStream_t)stream, *a);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

namespace {
bool lion_groups_ok(const qfx_lion_group* groups, int n_groups) {
  if (!groups_count_ok(groups, n_groups)) return false;
  for (int i = 0; i < n_groups; ++i)
    if (!lion_scalars_ok(groups[i].lr, groups[i].beta1, groups[i].beta2, groups[i].weight_decay)) return false;
  return true;
}
}  // namespace

extern "C" int qfx_lion_step_grouped(float* p, const float* g, float* m, int64_t n, const uint8_t* tile_group,
                                     const qfx_lion_group* groups, int32_t n_groups, const float* gnorm_sq, float max_norm,
                                     float grad_scale, void* stream) {
  if (!p || !g || !m || !tile_group || n <= 0 || !lion_groups_ok(groups, n_groups)) return QFX_EINVAL;
  const GroupTable<qfx_lion_group> tab = group_table(groups, n_groups);
  const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) == 0;
  const int blocks = flat_grid(vec ? (n + 3) / 4 : n, FLAT_STEP_CAP);
  if (vec)
    hipLaunchKernelGGL(lion_grouped_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, n, tile_group, tab, n_groups,
                       gnorm_sq, max_norm, grad_scale);
  else
    hipLaunchKernelGGL(lion_grouped_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, n, tile_group, tab, n_groups,
                       gnorm_sq, max_norm, grad_scale);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_lion8bit_step_grouped(const qfx_lion8bit_args* a, const uint8_t* block_group, const qfx_lion_group* groups,
                                         int32_t n_groups, void* stream) {
  if (!a || !a->p || !a->g || !a->q1 || !a->absmax1 || !a->m32 || !a->table || !a->qmap1 || !block_group) return QFX_EINVAL;
  if ((a->blocksize != 256 && a->blocksize != 2048) || a->n_blocks <= 0 || !lion_groups_ok(groups, n_groups)) return QFX_EINVAL;
  const GroupTable<qfx_lion_group> tab = group_table(groups, n_groups);
  const dim3 grid(blockwise_grid(a->n_blocks, a->blocksize));
  if (a->blocksize == 256)
    hipLaunchKernelGGL(lion8bit_grouped_kernel<256>, grid, dim3(256), 0, (hipStream_t)stream, *a, block_group, tab, n_groups);
  else
    hipLaunchKernelGGL(lion8bit_grouped_kernel<2048>, grid, dim3(256), 0, (hipStream_t)stream, *a, block_group, tab, n_groups);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
