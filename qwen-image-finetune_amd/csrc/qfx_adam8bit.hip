// qfx_adam8bit.hip -- blockwise 8-bit Adam / AdamW with bitsandbytes' state layout over the flat LoRA buffers, see include/qfx.h.
// ONE launch, driven by the block table.  The moment / parameter arithmetic is written out operation by operation and the whole
// file is compiled without FMA contraction (the pragma below and -ffp-contract=off in the build), so every rounding point, the
// clip prologue's included, is the one of the restatement in tests/bnb8_ref.py.  Plain operators only, as in qfx_lion.hip.
// blocksize 256: one wave per table entry, 4 elements per lane (one dwordx4 of p and of g, one dword of four codes per moment), the
// block maximum a cross-lane reduction.  blocksize 2048: one 256-thread workgroup per entry, 8 elements per lane, maximum through LDS.
#include "qfx_common.h"
#include "qfx_optim.h"

#pragma clang fp contract(off)

namespace {

struct A8Const { float b1, b2, omb1, omb2, step_size, eps_hat, decay, clip; int wd; };

// one element: moments in (decoded or fp32), out updated; p updated.  bnb's two kernels associate the g'^2 term differently.
template <bool FP32_FORM>
__device__ __forceinline__ void a8_elem(float& p, float g, float& m, float& v, const A8Const& k) {
  const float gs = g * k.clip;
  if (!__builtin_isfinite(gs)) return;
  m = m * k.b1 + k.omb1 * gs;
  v = FP32_FORM ? v * k.b2 + k.omb2 * (gs * gs) : v * k.b2 + (k.omb2 * gs) * gs;
  p = p + k.step_size * (m / (sqrtf(v) + k.eps_hat));
  if (k.wd) p = p * k.decay;
}

// the per-launch (per-group) constants: 1 - b1, 1 - b2 and decay = 1 - lr wd formed in fp32 here, step_size / eps_hat on the host
__device__ __forceinline__ A8Const a8_const(float lr, float b1, float b2, float wd, float step_size, float eps_hat, float clip) {
  A8Const k;
  k.clip = clip;
  k.b1 = b1; k.b2 = b2; k.omb1 = 1.0f - b1; k.omb2 = 1.0f - b2;
  k.step_size = step_size; k.eps_hat = eps_hat;
  k.wd = wd > 0.f; k.decay = 1.0f - lr * wd;
  return k;
}

// a group's row as the kernel takes it: the caller's scalars and the two values the host forms in double from them and the step
struct A8Row { float lr, beta1, beta2, weight_decay, step_size, eps_hat; };

// BS = 256: E = 4, a wave per entry (4 entries per workgroup and iteration); BS = 2048: E = 8, the workgroup per entry.
// GROUPED: the A8Const of every table entry is the one of its group (block_group, one byte per entry; tab: the groups' rows)
template <int BS, bool GROUPED>
__device__ __forceinline__ void adam8bit_body(const qfx_adam8bit_args& a, float step_size, float eps_hat,
                                              const uint8_t* __restrict__ block_group, const GroupTable<A8Row>* tab, int n_groups) {
  constexpr bool WG = BS > 256;
  constexpr int E = WG ? 8 : 4;
  constexpr int LANES = WG ? 256 : 64;
  static_assert(E * LANES == BS, "tile");
  __shared__ float q1s[256], q2s[256], mid1[256], mid2[256];
  __shared__ float red[2][2][4];
  __shared__ A8Const ks[GROUPED ? QFX_MAX_PARAM_GROUPS : 1];
  const int t = threadIdx.x;
  q1s[t] = a.qmap1[t];
  q2s[t] = a.qmap2[t];
  mid1[t] = t < 255 ? (a.qmap1[t] + a.qmap1[t + 1]) / 2.0f : INFINITY;
  mid2[t] = t < 255 ? (a.qmap2[t] + a.qmap2[t + 1]) / 2.0f : INFINITY;
  float clip = a.grad_scale;
  if (a.gnorm_sq != nullptr && a.max_norm > 0.f) {      // = opt_clip (qfx_optim.h), written out: inlined, it compiles to other code here
    const float nrm = sqrtf(*a.gnorm_sq) * a.grad_scale;
    const float c = a.max_norm / (nrm + 1e-6f);
    clip *= c < 1.0f ? c : 1.0f;
  }
  A8Const k;
  if (GROUPED) {
    if (t < n_groups) {
      const A8Row q = tab->g[t];
      ks[t] = a8_const(q.lr, q.beta1, q.beta2, q.weight_decay, q.step_size, q.eps_hat, clip);
    }
  } else {
    k = a8_const(a.lr, a.beta1, a.beta2, a.weight_decay, step_size, eps_hat, clip);
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
    float p[E], g[E], m[E], v[E];
    tile_load<E>(a.p, base, n, p);
    tile_load<E>(a.g, base, n, g);
    if (e.mode == QFX_ADAM8BIT_FP32) {
      const int64_t sb = e.state + (int64_t)lane * E;
      tile_load<E>(a.m32, sb, n, m);
      tile_load<E>(a.v32, sb, n, v);
#pragma unroll
      for (int j = 0; j < E; ++j) a8_elem<true>(p[j], g[j], m[j], v[j], k);
      tile_store<E>(a.p, base, n, p);
      tile_store<E>(a.m32, sb, n, m);
      tile_store<E>(a.v32, sb, n, v);
      continue;
    }
    int c1[E], c2[E];
    tile_load_codes<E>(a.q1, base, n, c1);
    tile_load_codes<E>(a.q2, base, n, c2);
    const float am1 = a.absmax1[e.state], am2 = a.absmax2[e.state];
    float mx1 = 0.f, mx2 = 0.f;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      m[j] = q1s[c1[j]] * am1;
      v[j] = q2s[c2[j]] * am2;
      if (j < n) {
        a8_elem<false>(p[j], g[j], m[j], v[j], k);
        mx1 = fmaxf(mx1, fabsf(m[j]));
        mx2 = fmaxf(mx2, fabsf(v[j]));
      }
    }
    mx1 = wave_max(mx1);
    mx2 = wave_max(mx2);
    if (WG) {
      if ((t & 63) == 0) { red[parity][0][t >> 6] = mx1; red[parity][1][t >> 6] = mx2; }
      __syncthreads();
      mx1 = fmaxf(fmaxf(red[parity][0][0], red[parity][0][1]), fmaxf(red[parity][0][2], red[parity][0][3]));
      mx2 = fmaxf(fmaxf(red[parity][1][0], red[parity][1][1]), fmaxf(red[parity][1][2], red[parity][1][3]));
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
      c2[j] = nearest_code(mid2, mx2 > 0.f ? v[j] / mx2 : 0.f);
    }
    tile_store_codes<E>(a.q1, base, n, c1);
    tile_store_codes<E>(a.q2, base, n, c2);
    if (lane == 0) { a.absmax1[e.state] = mx1; a.absmax2[e.state] = mx2; }
  }
}

template <int BS>
__global__ __launch_bounds__(256) void adam8bit_kernel(const qfx_adam8bit_args a, float step_size, float eps_hat) {
  adam8bit_body<BS, false>(a, step_size, eps_hat, nullptr, nullptr, 0);
}
template <int BS>
__global__ __launch_bounds__(256) void adam8bit_grouped_kernel(const qfx_adam8bit_args a, const uint8_t* __restrict__ block_group,
                                                               const GroupTable<A8Row> tab, int n_groups) {
  adam8bit_body<BS, true>(a, 0.f, 0.f, block_group, &tab, n_groups);
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
  if (!a || !a->p || !a->g || !a->q1 || !a->q2 || !a->absmax1 || !a->absmax2 || !a->m32 || !a->v32 || !a->table || !a->qmap1 ||
      !a->qmap2)
    return QFX_EINVAL;
  if ((a->blocksize != 256 && a->blocksize != 2048) || a->n_blocks <= 0 || a->step < 1 || !(a->lr >= 0.f)) return QFX_EINVAL;
  if (!(a->beta1 >= 0.f && a->beta1 < 1.f) || !(a->beta2 >= 0.f && a->beta2 < 1.f)) return QFX_EINVAL;
  float step_size, eps_hat;
  a8_host_scalars(a->lr, a->beta1, a->beta2, a->eps, a->step, &step_size, &eps_hat);
  const dim3 grid(blockwise_grid(a->n_blocks, a->blocksize));
  if (a->blocksize == 256)
    hipLaunchKernelGGL(adam8bit_kernel<256>, grid, dim3(256), 0, (hipStream_t)stream, *a, step_size, eps_hat);
  else
    hipLaunchKernelGGL(adam8bit_kernel<2048>, grid, dim3(256), 0, (hipStream_t)stream, *a, step_size, eps_hat);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_adam8bit_step_grouped(const qfx_adam8bit_args* a, const uint8_t* block_group, const qfx_adam8bit_group* groups,
                                         int32_t n_groups, void* stream) {
  if (!a || !a->p || !a->g || !a->q1 || !a->q2 || !a->absmax1 || !a->absmax2 || !a->m32 || !a->v32 || !a->table || !a->qmap1 ||
      !a->qmap2 || !block_group)
    return QFX_EINVAL;
  if ((a->blocksize != 256 && a->blocksize != 2048) || a->n_blocks <= 0 || a->step < 1 || !groups_count_ok(groups, n_groups)) return QFX_EINVAL;
  GroupTable<A8Row> tab = {};
  for (int i = 0; i < n_groups; ++i) {
    const qfx_adam8bit_group& q = groups[i];
    if (!(q.lr >= 0.f) || !beta_ok(q.beta1) || !beta_ok(q.beta2) || !(q.eps >= 0.f) || !(q.weight_decay >= 0.f)) return QFX_EINVAL;
    A8Row& r = tab.g[i];
    r.lr = q.lr; r.beta1 = q.beta1; r.beta2 = q.beta2; r.weight_decay = q.weight_decay;
    a8_host_scalars(q.lr, q.beta1, q.beta2, q.eps, a->step, &r.step_size, &r.eps_hat);
  }
  const dim3 grid(blockwise_grid(a->n_blocks, a->blocksize));
  if (a->blocksize == 256)
    hipLaunchKernelGGL(adam8bit_grouped_kernel<256>, grid, dim3(256), 0, (hipStream_t)stream, *a, block_group, tab, n_groups);
  else
    hipLaunchKernelGGL(adam8bit_grouped_kernel<2048>, grid, dim3(256), 0, (hipStream_t)stream, *a, block_group, tab, n_groups);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
