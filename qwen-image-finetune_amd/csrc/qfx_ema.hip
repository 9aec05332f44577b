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
  flat_sweep<VEC>(n, [&](int64_t i, int64_t, auto w) {
    constexpr int W = decltype(w)::value;
    float pv[W], sv[NS][W];
    flat_load(p + i, pv);
#pragma unroll
    for (int q = 0; q < NS; ++q) flat_load(k.s[q] + i, sv[q]);
#pragma unroll
    for (int q = 0; q < NS; ++q) {
#pragma unroll
      for (int j = 0; j < W; ++j) sv[q][j] = ema_elem(sv[q][j], pv[j], k.omd[q]);
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) flat_store(k.s[q] + i, sv[q]);
  });
}

// the words travel as integers: no float operation sees a NaN payload, a denormal or a signed zero
template <bool VEC>
__global__ __launch_bounds__(256) void ema_swap_kernel(uint32_t* __restrict__ p, uint32_t* __restrict__ s, int64_t n) {
  flat_sweep<VEC>(n, [&](int64_t i, int64_t, auto w) {
    constexpr int W = decltype(w)::value;
    uint32_t pv[W], sv[W];
    flat_load(p + i, pv); flat_load(s + i, sv);
    flat_store(p + i, sv); flat_store(s + i, pv);
  });
}

template <int NS>
void ema_update_launch(const FlatShape& s, void* stream, const float* p, int64_t n, const EmaConst& k) {
  launch_either<ema_update_kernel<true, NS>, ema_update_kernel<false, NS>>(s.vec, s.blocks, stream, p, n, k);
}

}  // namespace

extern "C" int qfx_ema_update(const float* p, int64_t n, const qfx_ema_args* a, void* stream) {
  if (!p || !a || n < 0 || a->n_shadows < 1 || a->n_shadows > QFX_EMA_MAX_SHADOWS) return QFX_EINVAL;
  EmaConst k = {};
  for (int q = 0; q < a->n_shadows; ++q) {
    if (!a->shadow[q] || a->shadow[q] == p) return QFX_EINVAL;
    if (!(a->one_minus_decay[q] >= 0.f && a->one_minus_decay[q] <= 1.f)) return QFX_EINVAL;      // a NaN fails
    for (int r = 0; r < q; ++r)
      if (a->shadow[r] == a->shadow[q]) return QFX_EINVAL;
    k.s[q] = a->shadow[q];
    k.omd[q] = a->one_minus_decay[q];
  }
  if (n == 0) return QFX_OK;
  // one 16-byte (or one scalar) access per lane, buffer and pass, at most FLAT_STEP_CAP workgroups, the rest by stride; the slots
  // of k.s behind n_shadows are null
  static_assert(QFX_EMA_MAX_SHADOWS == 4, "the pointer list below");
  const FlatShape s = flat_launch_shape(n, FLAT_STEP_CAP, p, k.s[0], k.s[1], k.s[2], k.s[3]);
  switch (a->n_shadows) {
    case 1: ema_update_launch<1>(s, stream, p, n, k); break;
    case 2: ema_update_launch<2>(s, stream, p, n, k); break;
    case 3: ema_update_launch<3>(s, stream, p, n, k); break;
    default: ema_update_launch<4>(s, stream, p, n, k); break;
  }
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_ema_swap(float* p, float* s, int64_t n, void* stream) {
  if (!p || !s || p == s || n < 0) return QFX_EINVAL;
  if (n == 0) return QFX_OK;
  const FlatShape sh = flat_launch_shape(n, FLAT_STEP_CAP, p, s);
  launch_either<ema_swap_kernel<true>, ema_swap_kernel<false>>(sh.vec, sh.blocks, stream, (uint32_t*)p, (uint32_t*)s, n);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
