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
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int64_t nv = VEC ? n / 4 : 0;
  for (int64_t i = tid; i < nv; i += nt) {
    f32x4 pv = *(const f32x4*)(p + 4 * i);
    const f32x4 gv = *(const f32x4*)(g + 4 * i);
    f32x4 zv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
    if (!FIRST) { zv = *(const f32x4*)(z + 4 * i); vv = *(const f32x4*)(v + 4 * i); }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pj = pv[j], zj = zv[j], vj = vv[j];
      sf_elem(pj, gv[j], zj, vj, k);
      pv[j] = pj; zv[j] = zj; vv[j] = vj;
    }
    *(f32x4*)(p + 4 * i) = pv;
    *(f32x4*)(z + 4 * i) = zv;
    *(f32x4*)(v + 4 * i) = vv;
  }
  for (int64_t i = 4 * nv + tid; i < n; i += nt) {
    float pi = p[i], zi = FIRST ? 0.f : z[i], vi = FIRST ? 0.f : v[i];
    sf_elem(pi, g[i], zi, vi, k);
    p[i] = pi; z[i] = zi; v[i] = vi;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void sf_swap_kernel(float* __restrict__ p, const float* __restrict__ z, int64_t n, float w, float omw) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int64_t nv = VEC ? n / 4 : 0;
  for (int64_t i = tid; i < nv; i += nt) {
    f32x4 pv = *(const f32x4*)(p + 4 * i);
    const f32x4 zv = *(const f32x4*)(z + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) pv[j] = sf_lerp(pv[j], zv[j], w, omw);
    *(f32x4*)(p + 4 * i) = pv;
  }
  for (int64_t i = 4 * nv + tid; i < n; i += nt) p[i] = sf_lerp(p[i], z[i], w, omw);
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
  const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)z | (uintptr_t)v) & 15) == 0;
  // one 16-byte (or one scalar) access per lane and pass, at most 256 CUs x 8 workgroups, the rest by stride
  const int blocks = flat_grid(vec ? (n + 3) / 4 : n, 2048);
  hipStream_t s = (hipStream_t)stream;
#define SF_LAUNCH(VEC, FIRST) \
  hipLaunchKernelGGL((sfadamw_kernel<VEC, FIRST>), dim3(blocks), dim3(256), 0, s, p, g, z, v, n, k, gnorm_sq, max_norm, grad_scale)
  if (vec) { if (first) SF_LAUNCH(true, true); else SF_LAUNCH(true, false); }
  else     { if (first) SF_LAUNCH(false, true); else SF_LAUNCH(false, false); }
#undef SF_LAUNCH
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_sf_swap(float* p, const float* z, int64_t n, float weight, void* stream) {
  if (!p || !z || n <= 0 || !__builtin_isfinite(weight)) return QFX_EINVAL;
  const bool vec = (((uintptr_t)p | (uintptr_t)z) & 15) == 0;
  const int blocks = flat_grid(vec ? (n + 3) / 4 : n, 2048);
  if (vec)
    hipLaunchKernelGGL(sf_swap_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, z, n, weight, 1.0f - weight);
  else
    hipLaunchKernelGGL(sf_swap_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, z, n, weight, 1.0f - weight);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
