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

struct LionConst { float b1, b2, omb1, omb2, lr, decay; int wd; };

__device__ __forceinline__ LionConst lion_const(const qfx_lion_group& q) {
  LionConst k;
  k.b1 = q.beta1; k.b2 = q.beta2; k.omb1 = 1.0f - q.beta1; k.omb2 = 1.0f - q.beta2;
  k.lr = q.lr; k.wd = q.weight_decay > 0.f; k.decay = 1.0f - q.lr * q.weight_decay;
  return k;
}

// one element: m in (fp32 or decoded), out updated; p decayed (decoupled, first) and moved by lr against the sign of c
__device__ __forceinline__ void lion_elem(float& p, float g, float& m, float clip, const LionConst& k) {
  const float gs = g * clip;
  if (!__builtin_isfinite(gs)) return;
  const float c = m * k.b1 + k.omb1 * gs;
  if (k.wd) p = p * k.decay;
  const float s = c > 0.f ? 1.0f : (c < 0.f ? -1.0f : 0.f);
  p = p - k.lr * s;
  m = m * k.b2 + k.omb2 * gs;
}

// one flat sweep (qfx_optim.h) for both fp32 entries.  GROUPED: lion_elem with the LionConst of the tile's group, formed by lion_const
// in LDS at workgroup start; else the one row `own`
template <bool VEC, bool GROUPED>
__device__ __forceinline__ void lion_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, int64_t n,
                                          const qfx_lion_group& own, const uint8_t* __restrict__ tile_group,
                                          const GroupTable<qfx_lion_group>* tab, int n_groups, float clip) {
  __shared__ LionConst ks[GROUPED ? QFX_MAX_PARAM_GROUPS : 1];
  LionConst k;
  if (GROUPED) {
    if ((int)threadIdx.x < n_groups) ks[threadIdx.x] = lion_const(tab->g[threadIdx.x]);
    __syncthreads();
  } else {
    k = lion_const(own);
  }
  flat_sweep<VEC>(n, [&](int64_t i, int64_t tile, auto w) {
    constexpr int W = decltype(w)::value;
    if (GROUPED) k = ks[group_index(tile_group, tile, n_groups)];
    float pv[W], gv[W], mv[W];
    flat_load(p + i, pv); flat_load(g + i, gv); flat_load(m + i, mv);
#pragma unroll
    for (int j = 0; j < W; ++j) lion_elem(pv[j], gv[j], mv[j], clip, k);
    flat_store(p + i, pv); flat_store(m + i, mv);
  });
}

template <bool VEC>
__global__ __launch_bounds__(256) void lion_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, int64_t n,
                                                   float lr, float b1, float b2, float wd, const float* __restrict__ gnorm_sq,
                                                   float max_norm, float grad_scale) {
  lion_body<VEC, false>(p, g, m, n, qfx_lion_group{lr, b1, b2, wd}, nullptr, nullptr, 0, opt_clip(gnorm_sq, max_norm, grad_scale));
}
template <bool VEC>
__global__ __launch_bounds__(256) void lion_grouped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           int64_t n, const uint8_t* __restrict__ tile_group,
                                                           const GroupTable<qfx_lion_group> tab, int n_groups,
                                                           const float* __restrict__ gnorm_sq, float max_norm, float grad_scale) {
  lion_body<VEC, true>(p, g, m, n, qfx_lion_group{}, tile_group, &tab, n_groups, opt_clip(gnorm_sq, max_norm, grad_scale));
}

// ---- blockwise 8-bit state: blockwise8_body (qfx_optim.h) with one signed plane and no unsigned one (no second code book in LDS)
struct Lion8 {
  static constexpr int NS = 1, NU = 0;
  typedef qfx_lion8bit_args Args;
  typedef qfx_lion_group Row;
  typedef LionConst Const;
  static __device__ __forceinline__ LionConst konst(const qfx_lion_group& q) { return lion_const(q); }
  static __device__ __forceinline__ uint8_t* codes(const Args& a, int) { return a.q1; }
  static __device__ __forceinline__ float* absmax(const Args& a, int) { return a.absmax1; }
  static __device__ __forceinline__ float* moment(const Args& a, int) { return a.m32; }
  template <bool FP32_ENTRY>
  static __device__ __forceinline__ void elem(float& p, float g, float (&s)[1], float clip, const LionConst& k) {
    lion_elem(p, g, s[0], clip, k);
  }
};

template <int BS>
__global__ __launch_bounds__(256) void lion8bit_kernel(const qfx_lion8bit_args a) {
  blockwise8_body<BS, false, Lion8>(a, qfx_lion_group{a.lr, a.beta1, a.beta2, a.weight_decay}, nullptr, nullptr, 0);
}
template <int BS>
__global__ __launch_bounds__(256) void lion8bit_grouped_kernel(const qfx_lion8bit_args a, const uint8_t* __restrict__ block_group,
                                                               const GroupTable<qfx_lion_group> tab, int n_groups) {
  blockwise8_body<BS, true, Lion8>(a, qfx_lion_group{}, block_group, &tab, n_groups);
}

bool lion_scalars_ok(float lr, float beta1, float beta2, float weight_decay) {
  return lr >= 0.f && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && weight_decay >= 0.f;      // a NaN fails each
}

bool lion_groups_ok(const qfx_lion_group* groups, int n_groups) {
  if (!groups_count_ok(groups, n_groups)) return false;
  for (int i = 0; i < n_groups; ++i)
    if (!lion_scalars_ok(groups[i].lr, groups[i].beta1, groups[i].beta2, groups[i].weight_decay)) return false;
  return true;
}

}  // namespace

extern "C" int qfx_lion_step(float* p, const float* g, float* m, int64_t n, float lr, float beta1, float beta2, float weight_decay,
                             const float* gnorm_sq, float max_norm, float grad_scale, void* stream) {
  if (!p || !g || !m || n <= 0 || !lion_scalars_ok(lr, beta1, beta2, weight_decay)) return QFX_EINVAL;
  const FlatShape s = flat_launch_shape(n, FLAT_STEP_CAP, p, g, m);      // adamw_kernel's grid policy
  launch_either<lion_kernel<true>, lion_kernel<false>>(s.vec, s.blocks, stream, p, g, m, n, lr, beta1, beta2, weight_decay, gnorm_sq,
                                                       max_norm, grad_scale);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_lion8bit_step(const qfx_lion8bit_args* a, void* stream) {
  if (!blockwise_args_ok<Lion8>(a) || !lion_scalars_ok(a->lr, a->beta1, a->beta2, a->weight_decay)) return QFX_EINVAL;
  return launch_blockwise<lion8bit_kernel<256>, lion8bit_kernel<2048>>(*a, stream);
}

extern "C" int qfx_lion_step_grouped(float* p, const float* g, float* m, int64_t n, const uint8_t* tile_group,
                                     const qfx_lion_group* groups, int32_t n_groups, const float* gnorm_sq, float max_norm,
                                     float grad_scale, void* stream) {
  if (!p || !g || !m || !tile_group || n <= 0 || !lion_groups_ok(groups, n_groups)) return QFX_EINVAL;
  const FlatShape s = flat_launch_shape(n, FLAT_STEP_CAP, p, g, m);
  launch_either<lion_grouped_kernel<true>, lion_grouped_kernel<false>>(s.vec, s.blocks, stream, p, g, m, n, tile_group,
                                                                       group_table(groups, n_groups), n_groups, gnorm_sq, max_norm,
                                                                       grad_scale);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_lion8bit_step_grouped(const qfx_lion8bit_args* a, const uint8_t* block_group, const qfx_lion_group* groups,
                                         int32_t n_groups, void* stream) {
  if (!blockwise_args_ok<Lion8>(a) || !block_group || !lion_groups_ok(groups, n_groups)) return QFX_EINVAL;
  return launch_blockwise<lion8bit_grouped_kernel<256>, lion8bit_grouped_kernel<2048>>(*a, stream, block_group,
                                                                                        group_table(groups, n_groups), n_groups);
}
