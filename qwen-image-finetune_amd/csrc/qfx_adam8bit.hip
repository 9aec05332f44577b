// qfx_adam8bit.hip -- blockwise 8-bit Adam / AdamW with bitsandbytes' state layout over the flat LoRA buffers, see include/qfx.h.
// ONE launch, driven by the block table: the tile walk is blockwise8_body (qfx_optim.h), this file states the family -- one signed
// and one unsigned state plane and the element function.  The moment / parameter arithmetic is written out operation by operation
// and the whole file is compiled without FMA contraction (the pragma below and -ffp-contract=off in the build), so every rounding
// point, the clip prologue's included, is the one of the restatement in tests/bnb8_ref.py.  Plain operators only, as in qfx_lion.hip.
#include "qfx_common.h"
#include "qfx_optim.h"

#pragma clang fp contract(off)

namespace {

// a group's row as the kernel takes it: the caller's scalars and the two values the host forms in double from them and the step
struct A8Row { float lr, beta1, beta2, weight_decay, step_size, eps_hat; };
struct A8Const { float b1, b2, omb1, omb2, step_size, eps_hat, decay; int wd; };

struct Adam8 {
  static constexpr int NS = 1, NU = 1;
  typedef qfx_adam8bit_args Args;
  typedef A8Row Row;
  typedef A8Const Const;
  // 1 - b1, 1 - b2 and decay = 1 - lr wd formed in fp32 here, step_size / eps_hat on the host
  static __device__ __forceinline__ A8Const konst(const A8Row& q) {
    A8Const k;
    k.b1 = q.beta1; k.b2 = q.beta2; k.omb1 = 1.0f - q.beta1; k.omb2 = 1.0f - q.beta2;
    k.step_size = q.step_size; k.eps_hat = q.eps_hat;
    k.wd = q.weight_decay > 0.f; k.decay = 1.0f - q.lr * q.weight_decay;
    return k;
  }
  static __device__ __forceinline__ uint8_t* codes(const Args& a, int i) { return i == 0 ? a.q1 : a.q2; }
  static __device__ __forceinline__ float* absmax(const Args& a, int i) { return i == 0 ? a.absmax1 : a.absmax2; }
  static __device__ __forceinline__ float* moment(const Args& a, int i) { return i == 0 ? a.m32 : a.v32; }
  // s[0] = m, s[1] = v.  bnb's two kernels associate the g'^2 term differently: FP32_ENTRY is its 32-bit kernel's form
  template <bool FP32_ENTRY>
  static __device__ __forceinline__ void elem(float& p, float g, float (&s)[2], float clip, const A8Const& k) {
    const float gs = g * clip;
    if (!__builtin_isfinite(gs)) return;
    float &m = s[0], &v = s[1];
    m = m * k.b1 + k.omb1 * gs;
    v = FP32_ENTRY ? v * k.b2 + k.omb2 * (gs * gs) : v * k.b2 + (k.omb2 * gs) * gs;
    p = p + k.step_size * (m / (sqrtf(v) + k.eps_hat));
    if (k.wd) p = p * k.decay;
  }
};

template <int BS>
__global__ __launch_bounds__(256) void adam8bit_kernel(const qfx_adam8bit_args a, float step_size, float eps_hat) {
  blockwise8_body<BS, false, Adam8>(a, A8Row{a.lr, a.beta1, a.beta2, a.weight_decay, step_size, eps_hat}, nullptr, nullptr, 0);
}
template <int BS>
__global__ __launch_bounds__(256) void adam8bit_grouped_kernel(const qfx_adam8bit_args a, const uint8_t* __restrict__ block_group,
                                                               const GroupTable<A8Row> tab, int n_groups) {
  blockwise8_body<BS, true, Adam8>(a, A8Row{}, block_group, &tab, n_groups);
}

// bnb's correction1 / correction2 / step_size, formed once in double on the host (the same value on every lane and every replica)
void a8_host_scalars(float lr, float beta1, float beta2, float eps, int step, float* step_size, float* eps_hat) {
  const double c1 = 1.0 - pow((double)beta1, (double)step);
  const double c2 = sqrt(1.0 - pow((double)beta2, (double)step));
  *step_size = (float)(-(double)lr * c2 / c1);
  *eps_hat = (float)((double)eps * c2);
}

}  // namespace

extern "C" int qfx_adam8bit_step(const qfx_adam8bit_args* a, void* stream) {
  if (!blockwise_args_ok<Adam8>(a) || a->step < 1 || !(a->lr >= 0.f) || !beta_ok(a->beta1) || !beta_ok(a->beta2)) return QFX_EINVAL;
  float step_size, eps_hat;
  a8_host_scalars(a->lr, a->beta1, a->beta2, a->eps, a->step, &step_size, &eps_hat);
  return launch_blockwise<adam8bit_kernel<256>, adam8bit_kernel<2048>>(*a, stream, step_size, eps_hat);
}

extern "C" int qfx_adam8bit_step_grouped(const qfx_adam8bit_args* a, const uint8_t* block_group, const qfx_adam8bit_group* groups,
                                         int32_t n_groups, void* stream) {
  if (!blockwise_args_ok<Adam8>(a) || !block_group || a->step < 1 || !groups_count_ok(groups, n_groups)) return QFX_EINVAL;
  GroupTable<A8Row> tab = {};
  for (int i = 0; i < n_groups; ++i) {
    const qfx_adam8bit_group& q = groups[i];
    if (!(q.lr >= 0.f) || !beta_ok(q.beta1) || !beta_ok(q.beta2) || !(q.eps >= 0.f) || !(q.weight_decay >= 0.f)) return QFX_EINVAL;
    A8Row& r = tab.g[i];
    r.lr = q.lr; r.beta1 = q.beta1; r.beta2 = q.beta2; r.weight_decay = q.weight_decay;
    a8_host_scalars(q.lr, q.beta1, q.beta2, q.eps, a->step, &r.step_size, &r.eps_hat);
  }
  return launch_blockwise<adam8bit_grouped_kernel<256>, adam8bit_grouped_kernel<2048>>(*a, stream, block_group, tab, n_groups);
}
