// qfx_schedulefree.hip -- Schedule-Free AdamW (Defazio et al., "The Road Less Scheduled", 2024; schedulefree.AdamWScheduleFree) over
// the flat LoRA buffers, see include/qfx.h.  Two entry points, ONE launch each: qfx_sfadamw_step updates y (the parameter buffer in
// train mode), z and exp_avg_sq in one pass (28 B of traffic per element: p, z and v read and written, g read -- the seven array
// passes of qfx_adamw_step), qfx_sf_swap moves the parameter buffer between y and the averaged point x (12 B per element).  Both
// are elementwise: no atomics, same inputs -> same bits.  The package's sequence of roundings is the specification: the whole file
// is compiled without FMA contraction (the pragma below and -ffp-contract=off in the build), so every product and sum is rounded
// where tests/schedulefree_ref.py rounds it.  Plain operators only, as in qfx_lion.hip.
#include "qfx_common.h"
#include "qfx_optim.h"

#pragma clang fp contract(off)

namespace {

// b2 .. eps as passed; ylr = lr_t (beta1 (1 - ckp1) - 1), formed in double on the host as the package forms it; w / omw: the lerp weight
// ckp1 and 1 - ckp1 in fp32
struct SfConst { float b2, omb2, bc2, eps, wd, w, omw, ylr, lr, clip; int wdon, first; };

// torch.lerp's formula, w uniform over the launch
__device__ __forceinline__ float sf_lerp(float a, float b, float w, float omw) {
  const float d = b - a;
  return fabsf(w) < 0.5f ? a + w * d : b - d * omw;
}

// one element: on the first step z = y and v = 0 are taken instead of read
__device__ __forceinline__ void sf_elem(float& y, float g, float& z, float& v, const SfConst& k) {
  const float gs = g * k.clip;
  if (k.first) { z = y; v = 0.f; }
  v = v * k.b2 + k.omb2 * gs * gs;
  float gn = gs / (sqrtf(v / k.bc2) + k.eps);
  if (k.wdon) gn = gn + k.wd * y;
  y = sf_lerp(y, z, k.w, k.omw);
  y = y + k.ylr * gn;
  z = z - k.lr * gn;
}

// VEC: p, g, z, v are 16-byte aligned -> one dwordx4 per buffer and lane; the n % 4 tail (and everything, without VEC) is scalar.
// FIRST: z and v are written only.
template <bool VEC, bool FIRST>
__global__ __launch_bounds__(256) void sfadamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ z,
                                                      float* __restrict__ v, int64_t n, SfConst k, const float* __restrict__ gnorm_sq,
                                                      float max_norm, float grad_scale) {
  k.clip = opt_clip(gnorm_sq, max_norm, grad_scale);
  k.first = FIRST;
  flat_sweep<VEC>(n, [&](int64_t i, int64_t, auto w) {
    constexpr int W = decltype(w)::value;
    float pv[W], gv[W], zv[W] = {}, vv[W] = {};
    flat_load(p + i, pv); flat_load(g + i, gv);
    if (!FIRST) { flat_load(z + i, zv); flat_load(v + i, vv); }
#pragma unroll
    for (int j = 0; j < W; ++j) sf_elem(pv[j], gv[j], zv[j], vv[j], k);
    flat_store(p + i, pv); flat_store(z + i, zv); flat_store(v + i, vv);
  });
}

template <bool VEC>
__global__ __launch_bounds__(256) void sf_swap_kernel(float* __restrict__ p, const float* __restrict__ z, int64_t n, float w, float omw) {
  flat_sweep<VEC>(n, [&](int64_t i, int64_t, auto wd) {
    constexpr int W = decltype(wd)::value;
    float pv[W], zv[W];
    flat_load(p + i, pv); flat_load(z + i, zv);
#pragma unroll
    for (int j = 0; j < W; ++j) pv[j] = sf_lerp(pv[j], zv[j], w, omw);
    flat_store(p + i, pv);
  });
}

}  // namespace

extern "C" int qfx_sfadamw_step(float* p, const float* g, float* z, float* v, int64_t n, float lr_t, float beta1, float beta2, float eps,
                                float weight_decay, float bias_corr2, float ckp1, int32_t first, const float* gnorm_sq, float max_norm,
                                float grad_scale, void* stream) {
  if (!p || !g || !z || !v || n <= 0) return QFX_EINVAL;
  if (!(lr_t >= 0.f) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f) || !(weight_decay >= 0.f) ||
      !(bias_corr2 > 0.f) || !(ckp1 >= 0.f && ckp1 <= 1.f))
    return QFX_EINVAL;      // a NaN fails each
  SfConst k;
  k.b2 = beta2; k.omb2 = 1.0f - beta2; k.bc2 = bias_corr2; k.eps = eps; k.wd = weight_decay; k.wdon = weight_decay != 0.f;
  k.w = ckp1; k.omw = 1.0f - ckp1; k.lr = lr_t; k.clip = 1.0f; k.first = 0;
  k.ylr = (float)((double)lr_t * ((double)beta1 * (1.0 - (double)ckp1) - 1.0));
  // one 16-byte (or one scalar) access per lane and pass, at most 256 CUs x 8 workgroups, the rest by stride
  const FlatShape s = flat_launch_shape(n, 2048, p, g, z, v);
  if (first)
    launch_either<sfadamw_kernel<true, true>, sfadamw_kernel<false, true>>(s.vec, s.blocks, stream, p, g, z, v, n, k, gnorm_sq, max_norm,
                                                                           grad_scale);
  else
    launch_either<sfadamw_kernel<true, false>, sfadamw_kernel<false, false>>(s.vec, s.blocks, stream, p, g, z, v, n, k, gnorm_sq, max_norm,
                                                                             grad_scale);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_sf_swap(float* p, const float* z, int64_t n, float weight, void* stream) {
  if (!p || !z || n <= 0 || !__builtin_isfinite(weight)) return QFX_EINVAL;
  const FlatShape s = flat_launch_shape(n, 2048, p, z);
  launch_either<sf_swap_kernel<true>, sf_swap_kernel<false>>(s.vec, s.blocks, stream, p, z, n, weight, 1.0f - weight);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
