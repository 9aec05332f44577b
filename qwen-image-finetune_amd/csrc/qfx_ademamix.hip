// qfx_ademamix.hip -- AdEMAMix (Pagliardini et al. 2024; bitsandbytes.optim.AdEMAMix / AdEMAMix8bit) over the flat LoRA buffers, see
// include/qfx.h: Adam with a second, slow gradient average.  Three states -- the fast average m1, the slow average m2 and Adam's nu
// -- and two hyperparameters that move every step (alpha_t, beta3_t).  Three entry points, ONE launch each: qfx_ademamix_step keeps
// the states in fp32 (44 B of traffic per element: p, m1, m2 and nu read and written, g read) and is always grouped;
// qfx_ademamix8bit_step / _grouped keep them as blockwise 8-bit codes in bitsandbytes' layout (m1 and m2 as two planes of ONE
// signed-map state, nu on the unsigned map) and are driven by the block table of qfx_adam8bit_step.
// The specification is the listing in include/qfx.h, NOT the package: it restates what bitsandbytes' 32-bit AdEMAMix kernel is
// understood to compute and was written without a copy of bitsandbytes at hand.  Every per-step scalar (the two schedules, the bias
// corrections, the decay factor) arrives in the group's row, formed in double on the host; ONE element function (ademamix_elem)
// serves the fp32 kernel, the fp32 entries of the block table and the decoded 8-bit blocks, one rounding per operation.  The whole
// file is compiled without FMA contraction (the pragma below and -ffp-contract=off in the build), so tests/ademamix_ref.py can
// state every rounding.  Elementwise apart from the block maxima, no atomics: same inputs -> same bits, and a grouped step gives
// every tensor the bits a one-group step with its row gives it.
#include "qfx_common.h"
#include "qfx_optim.h"

#pragma clang fp contract(off)

namespace {

// one element: the three states in (fp32 or decoded), out updated; p moved, then decayed (decoupled, after the update)
__device__ __forceinline__ void ademamix_elem(float& p, float g, float& m1, float& m2, float& nu, float clip,
                                              const qfx_ademamix_group& k) {
  const float gs = g * clip;
  if (!__builtin_isfinite(gs)) return;
  m1 = m1 * k.beta1 + k.one_minus_beta1 * gs;
  m2 = m2 * k.beta3_t + k.one_minus_beta3_t * gs;
  nu = nu * k.beta2 + (k.one_minus_beta2 * gs) * gs;
  p = p - k.lr * ((m1 / k.bias_corr1 + k.alpha_t * m2) / (sqrtf(nu) / k.sqrt_bias_corr2 + k.eps));
  if (k.weight_decay > 0.f) p = p * k.decay;
}

// the flat sweep of qfx_optim.h over p, g, m1, m2, nu.  map == nullptr: one group, row 0.
template <bool VEC>
__global__ __launch_bounds__(256) void ademamix_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m1,
                                                       float* __restrict__ m2, float* __restrict__ nu, int64_t n,
                                                       const uint8_t* __restrict__ tile_group, const GroupTable<qfx_ademamix_group> tab,
                                                       int n_groups, const float* __restrict__ gnorm_sq, float max_norm,
                                                       float grad_scale) {
  __shared__ qfx_ademamix_group rows[QFX_MAX_PARAM_GROUPS];
  if ((int)threadIdx.x < n_groups) rows[threadIdx.x] = tab.g[threadIdx.x];
  const float clip = opt_clip(gnorm_sq, max_norm, grad_scale);
  __syncthreads();
  flat_sweep<VEC>(n, [&](int64_t i, int64_t tile, auto w) {
    constexpr int W = decltype(w)::value;
    const qfx_ademamix_group k = rows[tile_group ? group_index(tile_group, tile, n_groups) : 0];
    float pv[W], gv[W], av[W], bv[W], sv[W];
    flat_load(p + i, pv); flat_load(g + i, gv); flat_load(m1 + i, av); flat_load(m2 + i, bv); flat_load(nu + i, sv);
#pragma unroll
    for (int j = 0; j < W; ++j) ademamix_elem(pv[j], gv[j], av[j], bv[j], sv[j], clip, k);
    flat_store(p + i, pv); flat_store(m1 + i, av); flat_store(m2 + i, bv); flat_store(nu + i, sv);
  });
}

// ---- blockwise 8-bit state: blockwise8_body (qfx_optim.h).  m1 and m2 are the two planes of state1 -- ONE signed code book and ONE
// table of midpoints in LDS serve both, each plane has its own absmax -- and nu is the unsigned plane.  The row is the constant.
struct AdEMAMix8 {
  static constexpr int NS = 2, NU = 1;
  typedef qfx_ademamix8bit_args Args;
  typedef qfx_ademamix_group Row;
  typedef qfx_ademamix_group Const;
  static __device__ __forceinline__ const Row& konst(const Row& q) { return q; }
  static __device__ __forceinline__ uint8_t* codes(const Args& a, int i) { return i == 0 ? a.q1 : (i == 1 ? a.q1 + a.q1_plane : a.q2); }
  static __device__ __forceinline__ float* absmax(const Args& a, int i) {
    return i == 0 ? a.absmax1 : (i == 1 ? a.absmax1 + a.absmax1_plane : a.absmax2);
  }
  static __device__ __forceinline__ float* moment(const Args& a, int i) { return i == 0 ? a.m32 : (i == 1 ? a.m32 + a.m32_plane : a.v32); }
  template <bool FP32_ENTRY>
  static __device__ __forceinline__ void elem(float& p, float g, float (&s)[3], float clip, const Row& k) {
    ademamix_elem(p, g, s[0], s[1], s[2], clip, k);
  }
};

template <int BS>
__global__ __launch_bounds__(256) void ademamix8bit_kernel(const qfx_ademamix8bit_args a) {
  blockwise8_body<BS, false, AdEMAMix8>(a, a.hp, nullptr, nullptr, 0);
}
template <int BS>
__global__ __launch_bounds__(256) void ademamix8bit_grouped_kernel(const qfx_ademamix8bit_args a, const uint8_t* __restrict__ block_group,
                                                                   const GroupTable<qfx_ademamix_group> tab, int n_groups) {
  blockwise8_body<BS, true, AdEMAMix8>(a, a.hp, block_group, &tab, n_groups);
}

bool row_ok(const qfx_ademamix_group& q) {      // a NaN fails each
  return q.lr >= 0.f && q.eps >= 0.f && q.weight_decay >= 0.f && q.alpha_t >= 0.f && beta_ok(q.beta1) && beta_ok(q.beta2) &&
         beta_ok(q.beta3_t) && q.bias_corr1 > 0.f;
}
bool rows_ok(const qfx_ademamix_group* groups, int n_groups) {
  if (!groups_count_ok(groups, n_groups)) return false;
  for (int i = 0; i < n_groups; ++i)
    if (!row_ok(groups[i])) return false;
  return true;
}

bool args8_ok(const qfx_ademamix8bit_args* a) {
  return blockwise_args_ok<AdEMAMix8>(a) && a->q1_plane > 0 && a->q1_plane % 4 == 0 && a->m32_plane > 0 && a->m32_plane % 4 == 0 &&
         a->absmax1_plane > 0;
}

}  // namespace

extern "C" int qfx_ademamix_step(const qfx_ademamix_args* a, void* stream) {
  if (!a || !a->p || !a->g || !a->m1 || !a->m2 || !a->nu || a->n <= 0 || !rows_ok(a->groups, a->n_groups)) return QFX_EINVAL;
  if (!a->tile_group && a->n_groups != 1) return QFX_EINVAL;
  const FlatShape s = flat_launch_shape(a->n, FLAT_STEP_CAP, a->p, a->g, a->m1, a->m2, a->nu);      // adamw_kernel's grid policy
  launch_either<ademamix_kernel<true>, ademamix_kernel<false>>(s.vec, s.blocks, stream, a->p, a->g, a->m1, a->m2, a->nu, a->n, a->tile_group,
                                                               group_table(a->groups, a->n_groups), a->n_groups, a->gnorm_sq,
                                                               a->max_norm, a->grad_scale);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_ademamix8bit_step(const qfx_ademamix8bit_args* a, void* stream) {
  if (!args8_ok(a) || !row_ok(a->hp)) return QFX_EINVAL;
  return launch_blockwise<ademamix8bit_kernel<256>, ademamix8bit_kernel<2048>>(*a, stream);
}

extern "C" int qfx_ademamix8bit_step_grouped(const qfx_ademamix8bit_args* a, const uint8_t* block_group,
                                             const qfx_ademamix_group* groups, int32_t n_groups, void* stream) {
  if (!args8_ok(a) || !block_group || !rows_ok(groups, n_groups)) return QFX_EINVAL;
  return launch_blockwise<ademamix8bit_grouped_kernel<256>, ademamix8bit_grouped_kernel<2048>>(*a, stream, block_group,
                                                                                                group_table(groups, n_groups), n_groups);
}
