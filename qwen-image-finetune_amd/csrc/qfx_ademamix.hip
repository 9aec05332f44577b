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

// VEC: p, g, m1, m2, nu are 16-byte aligned -> one dwordx4 per buffer and lane (a quad never leaves its tile: tiles start at
// multiples of 64); the n % 4 tail (and everything, without VEC) is scalar.  map == nullptr: one group, row 0.
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
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  const int64_t nv = VEC ? n / 4 : 0;
  for (int64_t i = tid; i < nv; i += nt) {
    const qfx_ademamix_group k = rows[tile_group ? group_index(tile_group, i >> 4, n_groups) : 0];
    f32x4 pv = *(const f32x4*)(p + 4 * i);
    const f32x4 gv = *(const f32x4*)(g + 4 * i);
    f32x4 av = *(const f32x4*)(m1 + 4 * i);
    f32x4 bv = *(const f32x4*)(m2 + 4 * i);
    f32x4 sv = *(const f32x4*)(nu + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pj = pv[j], aj = av[j], bj = bv[j], sj = sv[j];
      ademamix_elem(pj, gv[j], aj, bj, sj, clip, k);
      pv[j] = pj; av[j] = aj; bv[j] = bj; sv[j] = sj;
    }
    *(f32x4*)(p + 4 * i) = pv;
    *(f32x4*)(m1 + 4 * i) = av;
    *(f32x4*)(m2 + 4 * i) = bv;
    *(f32x4*)(nu + 4 * i) = sv;
  }
  for (int64_t i = 4 * nv + tid; i < n; i += nt) {
    const qfx_ademamix_group k = rows[tile_group ? group_index(tile_group, i >> 6, n_groups) : 0];
    float pi = p[i], ai = m1[i], bi = m2[i], si = nu[i];
    ademamix_elem(pi, g[i], ai, bi, si, clip, k);
    p[i] = pi; m1[i] = ai; m2[i] = bi; nu[i] = si;
  }
}

// keep-the-sign rule of a signed state (qfx_adam8bit_step's state1): the nearest code of x = m / mx, moved one index towards m when
// its value carries the other sign bit; mx == 0 stores the code of 0.0
__device__ __forceinline__ int signed_code(const float* q1s, const float* mid1, float m, float mx) {
  int c = nearest_code(mid1, mx > 0.f ? m / mx : 0.f);
  if (mx > 0.f && (__builtin_signbit(q1s[c]) != 0) != (__builtin_signbit(m) != 0)) {
    c += m > 0.f ? 1 : -1;
    c = c < 0 ? 0 : (c > 255 ? 255 : c);
  }
  return c;
}

// ---- blockwise 8-bit state (the tile helpers of qfx_optim.h, shared with adam8bit_kernel and lion8bit_kernel).
// BS = 256: E = 4, a wave per entry (4 entries per workgroup and iteration), the three block maxima cross-lane reductions;
// BS = 2048: E = 8, the workgroup per entry, the maxima through LDS.  m1 and m2 are the two planes of state1: ONE signed code book
// and ONE table of midpoints in LDS serve both, each plane has its own absmax.
// GROUPED: the row of every table entry is the one of its group (block_group, one byte per entry); else a.hp
template <int BS, bool GROUPED>
__device__ __forceinline__ void ademamix8bit_body(const qfx_ademamix8bit_args& a, const uint8_t* __restrict__ block_group,
                                                  const GroupTable<qfx_ademamix_group>* tab, int n_groups) {
  constexpr bool WG = BS > 256;
  constexpr int E = WG ? 8 : 4;
  constexpr int LANES = WG ? 256 : 64;
  static_assert(E * LANES == BS, "tile");
  __shared__ float q1s[256], q2s[256], mid1[256], mid2[256];
  __shared__ float red[2][3][4];
  __shared__ qfx_ademamix_group ks[GROUPED ? QFX_MAX_PARAM_GROUPS : 1];
  const int t = threadIdx.x;
  q1s[t] = a.qmap1[t];
  q2s[t] = a.qmap2[t];
  mid1[t] = t < 255 ? (a.qmap1[t] + a.qmap1[t + 1]) / 2.0f : INFINITY;
  mid2[t] = t < 255 ? (a.qmap2[t] + a.qmap2[t + 1]) / 2.0f : INFINITY;
  const float clip = opt_clip(a.gnorm_sq, a.max_norm, a.grad_scale);
  if (GROUPED) {
    if (t < n_groups) ks[t] = tab->g[t];
  } else if (t == 0) {
    ks[0] = a.hp;
  }
  __syncthreads();
  uint8_t* const q1b = a.q1 + a.q1_plane;            // plane 1: the slow average
  float* const absmax1b = a.absmax1 + a.absmax1_plane;
  float* const m32b = a.m32 + a.m32_plane;
  const int lane = WG ? t : (t & 63);
  const int64_t first = WG ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + (t >> 6);
  const int64_t stride = WG ? (int64_t)gridDim.x : (int64_t)gridDim.x * 4;
  int parity = 0;
  for (int64_t bi = first; bi < a.n_blocks; bi += stride) {      // WG: bi is uniform over the workgroup, every thread reaches the barrier
    const qfx_adam8bit_block e = a.table[bi];
    const qfx_ademamix_group k = ks[GROUPED ? group_index(block_group, bi, n_groups) : 0];
    const int64_t base = e.off + (int64_t)lane * E;
    const int n = e.len - lane * E;
    float p[E], g[E], m1[E], m2[E], nu[E];
    tile_load<E>(a.p, base, n, p);
    tile_load<E>(a.g, base, n, g);
    if (e.mode == QFX_ADAM8BIT_FP32) {
      const int64_t sb = e.state + (int64_t)lane * E;
      tile_load<E>(a.m32, sb, n, m1);
      tile_load<E>(m32b, sb, n, m2);
      tile_load<E>(a.v32, sb, n, nu);
#pragma unroll
      for (int j = 0; j < E; ++j) ademamix_elem(p[j], g[j], m1[j], m2[j], nu[j], clip, k);
      tile_store<E>(a.p, base, n, p);
      tile_store<E>(a.m32, sb, n, m1);
      tile_store<E>(m32b, sb, n, m2);
      tile_store<E>(a.v32, sb, n, nu);
      continue;
    }
    int c[E];
    const float am1 = a.absmax1[e.state], am1b = absmax1b[e.state], am2 = a.absmax2[e.state];
    tile_load_codes<E>(a.q1, base, n, c);
#pragma unroll
    for (int j = 0; j < E; ++j) m1[j] = q1s[c[j]] * am1;
    tile_load_codes<E>(q1b, base, n, c);
#pragma unroll
    for (int j = 0; j < E; ++j) m2[j] = q1s[c[j]] * am1b;
    tile_load_codes<E>(a.q2, base, n, c);
    float mx1 = 0.f, mx1b = 0.f, mx2 = 0.f;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      nu[j] = q2s[c[j]] * am2;
      if (j < n) {
        ademamix_elem(p[j], g[j], m1[j], m2[j], nu[j], clip, k);
        mx1 = fmaxf(mx1, fabsf(m1[j]));
        mx1b = fmaxf(mx1b, fabsf(m2[j]));
        mx2 = fmaxf(mx2, fabsf(nu[j]));
      }
    }
    mx1 = wave_max(mx1);
    mx1b = wave_max(mx1b);
    mx2 = wave_max(mx2);
    if (WG) {
      if ((t & 63) == 0) { red[parity][0][t >> 6] = mx1; red[parity][1][t >> 6] = mx1b; red[parity][2][t >> 6] = mx2; }
      __syncthreads();
      mx1 = fmaxf(fmaxf(red[parity][0][0], red[parity][0][1]), fmaxf(red[parity][0][2], red[parity][0][3]));
      mx1b = fmaxf(fmaxf(red[parity][1][0], red[parity][1][1]), fmaxf(red[parity][1][2], red[parity][1][3]));
      mx2 = fmaxf(fmaxf(red[parity][2][0], red[parity][2][1]), fmaxf(red[parity][2][2], red[parity][2][3]));
      parity ^= 1;
    }
    tile_store<E>(a.p, base, n, p);
#pragma unroll
    for (int j = 0; j < E; ++j) c[j] = signed_code(q1s, mid1, m1[j], mx1);
    tile_store_codes<E>(a.q1, base, n, c);
#pragma unroll
    for (int j = 0; j < E; ++j) c[j] = signed_code(q1s, mid1, m2[j], mx1b);
    tile_store_codes<E>(q1b, base, n, c);
#pragma unroll
    for (int j = 0; j < E; ++j) c[j] = nearest_code(mid2, mx2 > 0.f ? nu[j] / mx2 : 0.f);
    tile_store_codes<E>(a.q2, base, n, c);
    if (lane == 0) { a.absmax1[e.state] = mx1; absmax1b[e.state] = mx1b; a.absmax2[e.state] = mx2; }
  }
}

template <int BS>
__global__ __launch_bounds__(256) void ademamix8bit_kernel(const qfx_ademamix8bit_args a) {
  ademamix8bit_body<BS, false>(a, nullptr, nullptr, 0);
}
template <int BS>
__global__ __launch_bounds__(256) void ademamix8bit_grouped_kernel(const qfx_ademamix8bit_args a, const uint8_t* __restrict__ block_group,
                                                                   const GroupTable<qfx_ademamix_group> tab, int n_groups) {
  ademamix8bit_body<BS, true>(a, block_group, &tab, n_groups);
}

bool row_ok(const qfx_ademamix_group& q) {      // a NaN fails each
  return q.lr >= 0.f && q.eps >= 0.f && q.weight_decay >= 0.f && q.alpha_t >= 0.f && beta_ok(q.beta1) && beta_ok(q.beta2) &&
         beta_ok(q.beta3_t) && q.bias_corr1 > 0.f;
}

bool args8_ok(const qfx_ademamix8bit_args* a) {
  if (!a || !a->p || !a->g || !a->q1 || !a->q2 || !a->absmax1 || !a->absmax2 || !a->m32 || !a->v32 || !a->table || !a->qmap1 ||
      !a->qmap2)
    return false;
  if ((a->blocksize != 256 && a->blocksize != 2048) || a->n_blocks <= 0) return false;
  return a->q1_plane > 0 && a->q1_plane % 4 == 0 && a->m32_plane > 0 && a->m32_plane % 4 == 0 && a->absmax1_plane > 0;
}

}  // namespace

extern "C" int qfx_ademamix_step(const qfx_ademamix_args* a, void* stream) {
  if (!a || !a->p || !a->g || !a->m1 || !a->m2 || !a->nu || a->n <= 0 || !groups_count_ok(a->groups, a->n_groups)) return QFX_EINVAL;
  if (!a->tile_group && a->n_groups != 1) return QFX_EINVAL;
  for (int i = 0; i < a->n_groups; ++i)
    if (!row_ok(a->groups[i])) return QFX_EINVAL;
  const GroupTable<qfx_ademamix_group> tab = group_table(a->groups, a->n_groups);
  const bool vec = (((uintptr_t)a->p | (uintptr_t)a->g | (uintptr_t)a->m1 | (uintptr_t)a->m2 | (uintptr_t)a->nu) & 15) == 0;
  const int blocks = flat_grid(vec ? (a->n + 3) / 4 : a->n, FLAT_STEP_CAP);      // adamw_kernel's grid policy
  if (vec)
    hipLaunchKernelGGL(ademamix_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a->p, a->g, a->m1, a->m2, a->nu, a->n,
                       a->tile_group, tab, a->n_groups, a->gnorm_sq, a->max_norm, a->grad_scale);
  else
    hipLaunchKernelGGL(ademamix_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a->p, a->g, a->m1, a->m2, a->nu, a->n,
                       a->tile_group, tab, a->n_groups, a->gnorm_sq, a->max_norm, a->grad_scale);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_ademamix8bit_step(const qfx_ademamix8bit_args* a, void* stream) {
  if (!args8_ok(a) || !row_ok(a->hp)) return QFX_EINVAL;
  const dim3 grid(blockwise_grid(a->n_blocks, a->blocksize));
  if (a->blocksize == 256)
    hipLaunchKernelGGL(ademamix8bit_kernel<256>, grid, dim3(256), 0, (hipStream_t)stream, *a);
  else
    hipLaunchKernelGGL(ademamix8bit_kernel<2048>, grid, dim3(256), 0, (hipStream_t)stream, *a);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_ademamix8bit_step_grouped(const qfx_ademamix8bit_args* a, const uint8_t* block_group,
                                             const qfx_ademamix_group* groups, int32_t n_groups, void* stream) {
  if (!args8_ok(a) || !block_group || !groups_count_ok(groups, n_groups)) return QFX_EINVAL;
  for (int i = 0; i < n_groups; ++i)
    if (!row_ok(groups[i])) return QFX_EINVAL;
  const GroupTable<qfx_ademamix_group> tab = group_table(groups, n_groups);
  const dim3 grid(blockwise_grid(a->n_blocks, a->blocksize));
  if (a->blocksize == 256)
    hipLaunchKernelGGL(ademamix8bit_grouped_kernel<256>, grid, dim3(256), 0, (hipStream_t)stream, *a, block_group, tab, n_groups);
  else
    hipLaunchKernelGGL(ademamix8bit_grouped_kernel<2048>, grid, dim3(256), 0, (hipStream_t)stream, *a, block_group, tab, n_groups);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
