// qfx_adamx.hip -- torch.optim.RAdam, NAdam and Adamax over the flat LoRA buffers, see include/qfx.h: ONE entry (qfx_adamx_step),
// ONE launch, ONE element function (adamx_elem) whose variant is a template parameter chosen per launch.  The specification is
// torch's single-tensor implementation (_single_tensor_radam / _single_tensor_nadam / _single_tensor_adamax): every per-step scalar
// torch forms as a Python float arrives in the group's row, formed in double on the host; the element function applies torch's
// fp32 tensor operations in torch's order, one rounding per operation.  The whole file is compiled without FMA contraction (the
// pragma below and -ffp-contract=off in the build); the three fmaf are the fused multiply-adds torch's own CPU kernels issue
// (lerp_, add(alpha=) and addcmul_), so tests/adamx_ref.py can state every rounding.  Elementwise, no atomics: same inputs -> same
// bits, and a grouped step gives every tensor the bits a one-group step with its row gives it.
#include "qfx_common.h"
#include "qfx_optim.h"

#pragma clang fp contract(off)

namespace {

// exp_avg.lerp_(grad, w), torch's form: start + w (end - start) below |w| = 0.5, end - (end - start)(1 - w) from there on
__device__ __forceinline__ float lerp_torch(float start, float end, float w) {
  const float diff = end - start;
  return fabsf(w) < 0.5f ? fmaf(diff, w, start) : fmaf(diff, w - 1.0f, end);
}

// one element of variant V.  s: the second state -- exp_avg_sq (RAdam, NAdam) or exp_inf (Adamax)
template <int V>
__device__ __forceinline__ void adamx_elem(float& p, float g, float& m, float& s, float clip, const qfx_adamx_group& k) {
  float pi = p;
  float gi = g * clip;
  if (k.weight_decay != 0.f) {
    if (V != QFX_ADAMX_ADAMAX && k.decoupled) pi = pi * k.decay;      // param.mul_(1 - lr * weight_decay)
    else gi = fmaf(pi, k.weight_decay, gi);                           // grad.add(param, alpha=weight_decay)
  }
  const float mi = lerp_torch(m, gi, k.one_minus_beta1);
  if (V == QFX_ADAMX_ADAMAX) {
    const float a = s * k.beta2, b = fabsf(gi) + k.eps;
    const float u = (a >= b || a != a) ? a : b;                       // torch.maximum: a NaN propagates
    pi = pi + (k.neg_clr * mi) / u;                                   // addcdiv_(exp_avg, exp_inf, value=-clr)
    s = u;
  } else {
    const float vi = fmaf(k.one_minus_beta2 * gi, gi, s * k.beta2);   // mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    if (V == QFX_ADAMX_RADAM) {
      float upd = (mi / k.bias_corr1) * k.lr;
      if (k.rectified) upd = (upd * ((1.0f / (sqrtf(vi) + k.eps)) * k.sqrt_bias_corr2)) * k.rect;
      pi = pi - upd;
    } else {
      const float den = sqrtf(vi / k.bias_corr2) + k.eps;
      pi = pi + (k.c_grad * gi) / den;                                // addcdiv_(grad, denom, value=-lr (1 - mu) / (1 - mu_product))
      pi = pi + (k.c_avg * mi) / den;                                 // addcdiv_(exp_avg, denom, value=-lr mu_next / (1 - mu_product_next))
    }
    s = vi;
  }
  p = pi; m = mi;
}

// VEC: p, g, m, s are 16-byte aligned -> one dwordx4 per buffer and lane (a quad never leaves its tile: tiles start at multiples of
// 64); the n % 4 tail (and everything, without VEC) is scalar.  map == nullptr: one group, row 0.
template <int V, bool VEC>
__global__ __launch_bounds__(256) void adamx_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ s, int64_t n, const uint8_t* __restrict__ tile_group,
                                                    const GroupTable<qfx_adamx_group> tab, int n_groups,
                                                    const float* __restrict__ gnorm_sq, float max_norm, float grad_scale) {
  __shared__ qfx_adamx_group rows[QFX_MAX_PARAM_GROUPS];
  if ((int)threadIdx.x < n_groups) rows[threadIdx.x] = tab.g[threadIdx.x];
  const float clip = opt_clip(gnorm_sq, max_norm, grad_scale);
  __syncthreads();
  flat_sweep<VEC>(n, [&](int64_t i, int64_t tile, auto w) {
    constexpr int W = decltype(w)::value;
    const qfx_adamx_group k = rows[tile_group ? group_index(tile_group, tile, n_groups) : 0];
    float pv[W], gv[W], mv[W], sv[W];
    flat_load(p + i, pv); flat_load(g + i, gv); flat_load(m + i, mv); flat_load(s + i, sv);
#pragma unroll
    for (int j = 0; j < W; ++j) adamx_elem<V>(pv[j], gv[j], mv[j], sv[j], clip, k);
    flat_store(p + i, pv); flat_store(m + i, mv); flat_store(s + i, sv);
  });
}

template <int V>
void adamx_launch(const qfx_adamx_args& a, void* stream) {
  const FlatShape s = flat_launch_shape(a.n, FLAT_STEP_CAP, a.p, a.g, a.exp_avg, a.state2);      // adamw_kernel's grid policy
  launch_either<adamx_kernel<V, true>, adamx_kernel<V, false>>(s.vec, s.blocks, stream, a.p, a.g, a.exp_avg, a.state2, a.n, a.tile_group,
                                                               group_table(a.groups, a.n_groups), a.n_groups, a.gnorm_sq, a.max_norm,
                                                               a.grad_scale);
}

}  // namespace

extern "C" int qfx_adamx_step(const qfx_adamx_args* a, void* stream) {
  if (!a || !a->p || !a->g || !a->exp_avg || !a->state2 || a->n <= 0 || !groups_count_ok(a->groups, a->n_groups)) return QFX_EINVAL;
  if (a->variant != QFX_ADAMX_RADAM && a->variant != QFX_ADAMX_NADAM && a->variant != QFX_ADAMX_ADAMAX) return QFX_EINVAL;
  if (!a->tile_group && a->n_groups != 1) return QFX_EINVAL;
  for (int i = 0; i < a->n_groups; ++i) {
    const qfx_adamx_group& q = a->groups[i];
    if (!(q.lr >= 0.f) || !beta_ok(q.beta1) || !beta_ok(q.beta2) || !(q.eps >= 0.f) || !(q.weight_decay >= 0.f)) return QFX_EINVAL;
    if (a->variant == QFX_ADAMX_RADAM && !(q.bias_corr1 > 0.f)) return QFX_EINVAL;
    if (a->variant == QFX_ADAMX_NADAM && !(q.bias_corr2 > 0.f)) return QFX_EINVAL;
  }
  if (a->variant == QFX_ADAMX_RADAM) adamx_launch<QFX_ADAMX_RADAM>(*a, stream);
  else if (a->variant == QFX_ADAMX_NADAM) adamx_launch<QFX_ADAMX_NADAM>(*a, stream);
  else adamx_launch<QFX_ADAMX_ADAMAX>(*a, stream);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
