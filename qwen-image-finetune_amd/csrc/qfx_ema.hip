// qfx_ema.hip -- exponential moving averages of the adapter weights (diffusers.training_utils.EMAModel) over the flat LoRA buffer,
// see include/qfx.h.  Two entry points, ONE launch each: qfx_ema_update moves up to QFX_EMA_MAX_SHADOWS shadow buffers towards the
// parameters, each at its own rate (p is read once for all of them: 4 + 8 n_shadows bytes of traffic per element), qfx_ema_swap
// exchanges the parameter buffer with one shadow bit for bit (16 B per element).  Both are elementwise: no atomics, same inputs ->
// same bits.  The package's sequence of roundings is the specification: the whole file is compiled without FMA contraction (the
// pragma below and -ffp-contract=off in the build), so the difference, the product and the second difference are each rounded
// where tests/ema_ref.py rounds them.  Plain operators only, as in qfx_schedulefree.hip.
#include "qfx_common.h"
#include "qfx_optim.h"

#pragma clang fp contract(off)

namespace {

// the shadow pointers and rates, by value in the kernel argument block
struct EmaConst { float* s[QFX_EMA_MAX_SHADOWS]; float omd[QFX_EMA_MAX_SHADOWS]; };

// EMAModel.step's s.sub_(one_minus_decay * (s - p))
__device__ __forceinline__ float ema_elem(float s, float p, float omd) {
  const float d = s - p;
  const float m = omd * d;
  return s - m;
}

// VEC: p and the NS shadows are 16-byte aligned -> one dwordx4 per buffer and lane; the n % 4 tail (and everything, without VEC) is
// scalar.  NS shadows are updated from the one p held in registers: all loads first, then the arithmetic, then the stores.
template <bool VEC, int NS>
__global__ __launch_bounds__(256) void ema_update_kernel(const float* __restrict__ p, int64_t n, EmaConst k) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int64_t nv = VEC ? n / 4 : 0;
  for (int64_t i = tid; i < nv; i += nt) {
    const f32x4 pv = *(const f32x4*)(p + 4 * i);
    f32x4 sv[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) sv[q] = *(const f32x4*)(k.s[q] + 4 * i);
#pragma unroll
    for (int q = 0; q < NS; ++q) {
#pragma unroll
      for (int j = 0; j < 4; ++j) sv[q][j] = ema_elem(sv[q][j], pv[j], k.omd[q]);
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) *(f32x4*)(k.s[q] + 4 * i) = sv[q];
  }
  for (int64_t i = 4 * nv + tid; i < n; i += nt) {
    const float pi = p[i];
    float si[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) si[q] = k.s[q][i];
#pragma unroll
    for (int q = 0; q < NS; ++q) k.s[q][i] = ema_elem(si[q], pi, k.omd[q]);
  }
}

// the words travel as integers: no float operation sees a NaN payload, a denormal or a signed zero
template <bool VEC>
__global__ __launch_bounds__(256) void ema_swap_kernel(uint32_t* __restrict__ p, uint32_t* __restrict__ s, int64_t n) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int64_t nv = VEC ? n / 4 : 0;
  for (int64_t i = tid; i < nv; i += nt) {
    const u32x4 pv = *(const u32x4*)(p + 4 * i);
    const u32x4 sv = *(const u32x4*)(s + 4 * i);
    *(u32x4*)(p + 4 * i) = sv;
    *(u32x4*)(s + 4 * i) = pv;
  }
  for (int64_t i = 4 * nv + tid; i < n; i += nt) {
    const uint32_t pi = p[i], si = s[i];
    p[i] = si;
    s[i] = pi;
  }
}

template <bool VEC>
void ema_update_launch(int blocks, hipStream_t st, const float* p, int64_t n, const EmaConst& k, int ns) {
  switch (ns) {
    case 1: hipLaunchKernelGGL((ema_update_kernel<VEC, 1>), dim3(blocks), dim3(256), 0, st, p, n, k); break;
    case 2: hipLaunchKernelGGL((ema_update_kernel<VEC, 2>), dim3(blocks), dim3(256), 0, st, p, n, k); break;
    case 3: hipLaunchKernelGGL((ema_update_kernel<VEC, 3>), dim3(blocks), dim3(256), 0, st, p, n, k); break;
    default: hipLaunchKernelGGL((ema_update_kernel<VEC, 4>), dim3(blocks), dim3(256), 0, st, p, n, k); break;
  }
}

}  // namespace

extern "C" int qfx_ema_update(const float* p, int64_t n, const qfx_ema_args* a, void* stream) {
  if (!p || !a || n < 0 || a->n_shadows < 1 || a->n_shadows > QFX_EMA_MAX_SHADOWS) return QFX_EINVAL;
  EmaConst k = {};
  uintptr_t bits = (uintptr_t)p;
  for (int q = 0; q < a->n_shadows; ++q) {
    if (!a->shadow[q] || a->shadow[q] == p) return QFX_EINVAL;
    if (!(a->one_minus_decay[q] >= 0.f && a->one_minus_decay[q] <= 1.f)) return QFX_EINVAL;      // a NaN fails
    for (int r = 0; r < q; ++r)
      if (a->shadow[r] == a->shadow[q]) return QFX_EINVAL;
    k.s[q] = a->shadow[q];
    k.omd[q] = a->one_minus_decay[q];
    bits |= (uintptr_t)a->shadow[q];
  }
  if (n == 0) return QFX_OK;
  const bool vec = (bits & 15) == 0;
  // one 16-byte (or one scalar) access per lane, buffer and pass, at most FLAT_STEP_CAP workgroups, the rest by stride
  const int blocks = flat_grid(vec ? (n + 3) / 4 : n, FLAT_STEP_CAP);
  if (vec) ema_update_launch<true>(blocks, (hipStream_t)stream, p, n, k, a->n_shadows);
  else     ema_update_launch<false>(blocks, (hipStream_t)stream, p, n, k, a->n_shadows);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_ema_swap(float* p, float* s, int64_t n, void* stream) {
  if (!p || !s || p == s || n < 0) return QFX_EINVAL;
  if (n == 0) return QFX_OK;
  const bool vec = (((uintptr_t)p | (uintptr_t)s) & 15) == 0;
  const int blocks = flat_grid(vec ? (n + 3) / 4 : n, FLAT_STEP_CAP);
  if (vec)
    hipLaunchKernelGGL(ema_swap_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (uint32_t*)p, (uint32_t*)s, n);
  else
    hipLaunchKernelGGL(ema_swap_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (uint32_t*)p, (uint32_t*)s, n);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
