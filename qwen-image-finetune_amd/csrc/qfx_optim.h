// What the fused optimizer kernels share: the gradient-clip prologue, the flat sweep of the fp32 elementwise kernels, the blockwise
// 8-bit tile walk (bitsandbytes' state layout, include/qfx.h), the grid policies and the parameter-group table.  Include after
// qfx_common.h.  Helpers only, and NO fp-contract pragma: contraction is lexical, so a helper rounds as the translation unit that
// includes it is built, which is what each family's restatement under tests/ expects of it:
//   the compiler's default contraction: qfx_optim.hip, qfx_adafactor.hip, qfx_elem.hip, qfx_scaled_adamw.hip (which switches it
//     off itself below its clip prologue)
//   -ffp-contract=off: qfx_adam8bit.hip, qfx_lion.hip, qfx_ademamix.hip, qfx_adamx.hip, qfx_schedulefree.hip, qfx_ema.hip,
//     qfx_came.hip, qfx_muon.hip, qfx_adapter_stats.hip
// flat_sweep and blockwise8_body hold index arithmetic, loads and stores only; every floating-point operation of a step is in the
// element function its family passes in.
#pragma once
#include <type_traits>
#include "qfx_common.h"

namespace {      // file-local in every translation unit: each unit's copy rounds as that unit is built

// clip = grad_scale * min(1, max_norm / (||g|| grad_scale + 1e-6)); grad_scale alone without a norm or with max_norm <= 0
__device__ __forceinline__ float opt_clip(const float* __restrict__ gnorm_sq, float max_norm, float grad_scale) {
  float clip = grad_scale;
  if (gnorm_sq != nullptr && max_norm > 0.f) {
    const float nrm = sqrtf(*gnorm_sq) * grad_scale;
    const float c = max_norm / (nrm + 1e-6f);
    clip *= c < 1.0f ? c : 1.0f;
  }
  return clip;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// sum over the 256 threads of a workgroup, the same bits on every thread (qfx_adafactor.hip, qfx_came.hip).  `red` (4 floats of
// LDS) may still be read by the previous call: barrier first.
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// number of midpoints below x (mid[255] = +inf): the nearest code, a tie (x == midpoint) going to the lower one
__device__ __forceinline__ int nearest_code(const float* mid, float x) {
  int c = 0;
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) c += (x > mid[c + s - 1]) ? s : 0;
  return c;
}

// E elements of one lane starting at element `base` of p / g / a moment / the codes, n of them valid (n may be < E or <= 0)
template <int E>
__device__ __forceinline__ void tile_load(const float* __restrict__ src, int64_t base, int n, float (&x)[E]) {
#pragma unroll
  for (int j = 0; j < E; j += 4) {
    if (n >= j + 4) {
      const f32x4 t = *(const f32x4*)(src + base + j);
      x[j] = t[0]; x[j + 1] = t[1]; x[j + 2] = t[2]; x[j + 3] = t[3];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) x[j + i] = (j + i < n) ? src[base + j + i] : 0.f;
    }
  }
}
template <int E>
__device__ __forceinline__ void tile_store(float* __restrict__ dst, int64_t base, int n, const float (&x)[E]) {
#pragma unroll
  for (int j = 0; j < E; j += 4) {
    if (n >= j + 4) {
      f32x4 t; t[0] = x[j]; t[1] = x[j + 1]; t[2] = x[j + 2]; t[3] = x[j + 3];
      *(f32x4*)(dst + base + j) = t;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) if (j + i < n) dst[base + j + i] = x[j + i];
    }
  }
}
template <int E>
__device__ __forceinline__ void tile_load_codes(const uint8_t* __restrict__ src, int64_t base, int n, int (&c)[E]) {
#pragma unroll
  for (int j = 0; j < E; j += 4) {
    if (n >= j + 4) {
      const uint32_t w = *(const uint32_t*)(src + base + j);
#pragma unroll
      for (int i = 0; i < 4; ++i) c[j + i] = (w >> (8 * i)) & 0xff;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) c[j + i] = (j + i < n) ? src[base + j + i] : 0;
    }
  }
}
template <int E>
__device__ __forceinline__ void tile_store_codes(uint8_t* __restrict__ dst, int64_t base, int n, const int (&c)[E]) {
#pragma unroll
  for (int j = 0; j < E; j += 4) {
    if (n >= j + 4) {     // packed 32-bit vector store
      *(uint32_t*)(dst + base + j) = (uint32_t)c[j] | ((uint32_t)c[j + 1] << 8) | ((uint32_t)c[j + 2] << 16) | ((uint32_t)c[j + 3] << 24);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) if (j + i < n) dst[base + j + i] = (uint8_t)c[j + i];
    }
  }
}

// grid of an elementwise kernel: one workgroup of 256 per 256 units of work, at most `cap`, the rest by stride
inline int flat_grid(int64_t work, int64_t cap) {
  const int64_t b = (work + 255) / 256;
  return (int)(b < cap ? b : cap);
}

// workgroup caps of the one-launch steps: the fp32 elementwise kernels (adamw_kernel's policy) and the blockwise 8-bit kernels
constexpr int64_t FLAT_STEP_CAP = 4096;
constexpr int64_t BLOCKWISE_CAP = 2048;

// ---- the flat sweep of the fp32 elementwise kernels: f(i, tile, FlatWidth<W>) steps the W elements from i, all of 64-element tile
// `tile`.  VEC (every buffer 16-byte aligned): a quad per lane (W = 4; a quad never leaves its tile, tiles start at multiples of
// 64), then the n % 4 tail one element per lane (W = 1); without VEC every element takes the W = 1 form.  The rest by stride.
// Workgroups of 256, as flat_grid counts them and launch_either starts them.
template <int W> struct FlatWidth { static constexpr int value = W; };

template <bool VEC, typename F>
__device__ __forceinline__ void flat_sweep(int64_t n, F f) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nt = (int64_t)gridDim.x * 256;
  const int64_t nv = VEC ? n / 4 : 0;
  for (int64_t i = tid; i < nv; i += nt) f(4 * i, i >> 4, FlatWidth<4>());
  for (int64_t i = 4 * nv + tid; i < n; i += nt) f(i, i >> 6, FlatWidth<1>());
}
// W = 4: one dwordx4; W = 1: one dword.  T: float, or uint32_t where the words must not meet a float operation
template <int W, typename T>
__device__ __forceinline__ void flat_load(const T* __restrict__ src, T (&x)[W]) {
  static_assert(W == 1 || W == 4, "width");
  typedef __attribute__((ext_vector_type(4))) T V4;
  if constexpr (W == 4) {
    const V4 t = *(const V4*)src;
    x[0] = t[0]; x[1] = t[1]; x[2] = t[2]; x[3] = t[3];
  } else {
    x[0] = src[0];
  }
}
template <int W, typename T>
__device__ __forceinline__ void flat_store(T* __restrict__ dst, const T (&x)[W]) {
  typedef __attribute__((ext_vector_type(4))) T V4;
  if constexpr (W == 4) {
    V4 t; t[0] = x[0]; t[1] = x[1]; t[2] = x[2]; t[3] = x[3];
    *(V4*)dst = t;
  } else {
    dst[0] = x[0];
  }
}

// launch shape of a flat sweep: the 16-byte form when every buffer is 16-byte aligned (a null pointer does not count), and its grid
struct FlatShape { bool vec; int blocks; };
template <typename... P>
inline FlatShape flat_launch_shape(int64_t n, int64_t cap, const P*... ptr) {
  const bool vec = ((... | (uintptr_t)ptr) & 15) == 0;
  return {vec, flat_grid(vec ? (n + 3) / 4 : n, cap)};
}

// one launch of 256-thread workgroups: kernel KT when `which`, else KF (the two instantiations of one kernel template)
template <auto KT, auto KF, typename... X>
inline void launch_either(bool which, unsigned blocks, void* stream, X... args) {
  if (which) hipLaunchKernelGGL(KT, dim3(blocks), dim3(256), 0, (hipStream_t)stream, args...);
  else hipLaunchKernelGGL(KF, dim3(blocks), dim3(256), 0, (hipStream_t)stream, args...);
}

// grid of a blockwise 8-bit kernel over n_blocks table entries: a wave per entry (blocksize 256) or a workgroup per entry (2048)
inline unsigned blockwise_grid(int64_t n_blocks, int blocksize) {
  const int64_t wgs = blocksize == 256 ? (n_blocks + 3) / 4 : n_blocks;
  return (unsigned)(wgs < BLOCKWISE_CAP ? wgs : BLOCKWISE_CAP);
}

// ---- parameter groups (include/qfx.h): the grouped kernels take their hyperparameter rows by value in the argument block, the
// first n_groups lanes of every workgroup turn them into the family's per-group constants in LDS, and every 64-element tile (fp32
// kernels) or block-table entry (blockwise kernels) names its row with one byte.  An index the builder did not range-check is
// clamped to the rows the launch filled (an entry >= n_groups takes the last row, n_groups - 1), so that it can never read LDS
// outside the table or a row of it that nobody wrote.
template <typename Row>
struct GroupTable { Row g[QFX_MAX_PARAM_GROUPS]; };

template <typename Row>
inline GroupTable<Row> group_table(const Row* groups, int n_groups) {
  GroupTable<Row> t = {};
  for (int i = 0; i < n_groups; ++i) t.g[i] = groups[i];
  return t;
}

__device__ __forceinline__ int group_index(const uint8_t* __restrict__ map, int64_t i, int n_groups) {
  const int gi = map[i];
  return gi < n_groups ? gi : n_groups - 1;      // only rows 0 .. n_groups-1 of the LDS table are filled
}

inline bool groups_count_ok(const void* groups, int n_groups) { return groups != nullptr && n_groups >= 1 && n_groups <= QFX_MAX_PARAM_GROUPS; }
inline bool beta_ok(float b) { return b >= 0.f && b < 1.f; }      // a NaN fails

// ---- the blockwise 8-bit tile walk (qfx_adam8bit.hip, qfx_lion.hip, qfx_ademamix.hip), driven by the block table of include/qfx.h.
// A code book in LDS: the 256 values and the 255 midpoints between neighbours (mid[255] = +inf)
struct CodeBook {
  float q[256], mid[256];
  __device__ __forceinline__ void fill(const float* __restrict__ qmap, int t) {
    q[t] = qmap[t];
    mid[t] = t < 255 ? (qmap[t] + qmap[t + 1]) / 2.0f : INFINITY;
  }
};

// keep-the-sign rule of a signed state (bitsandbytes' state1): the nearest code of x = m / mx, moved one index towards m when its
// value carries the other sign bit; mx == 0 stores the code of 0.0
__device__ __forceinline__ int signed_code(const CodeBook& b, float m, float mx) {
  int c = nearest_code(b.mid, mx > 0.f ? m / mx : 0.f);
  if (mx > 0.f && (__builtin_signbit(b.q[c]) != 0) != (__builtin_signbit(m) != 0)) {
    c += m > 0.f ? 1 : -1;
    c = c < 0 ? 0 : (c > 255 ? 255 : c);
  }
  return c;
}

// One walk for every family.  BS = 256: E = 4, a wave per table entry (4 entries per workgroup and iteration), the block maxima
// cross-lane reductions; BS = 2048: E = 8, the workgroup per entry, the maxima through LDS.  A family F states
//   NS, NU           its state planes: NS >= 1 on the signed code book (they share ONE book), then NU on the unsigned one (NU == 0:
//                    no second book in LDS)
//   Args, Row, Const its argument struct, the hyperparameter row of a group (GroupTable<Row>) and the constants an element takes
//   konst(row)       Row -> Const; `own` is the row of the ungrouped entry, GROUPED takes the row of every entry's group from tab
//   codes / absmax / moment(a, i)   plane i's code bytes (indexed like p), block maxima and fp32 state (the table's fp32 entries)
//   elem<FP32_ENTRY>(p, g, s, clip, k)   one element: s[NS + NU] in (fp32 or decoded), out updated; p updated
template <int BS, bool GROUPED, typename F>
__device__ __forceinline__ void blockwise8_body(const typename F::Args& a, const typename F::Row& own,
                                                const uint8_t* __restrict__ block_group, const GroupTable<typename F::Row>* tab,
                                                int n_groups) {
  constexpr bool WG = BS > 256;
  constexpr int E = WG ? 8 : 4, LANES = WG ? 256 : 64, NS = F::NS, NP = F::NS + F::NU;
  static_assert(E * LANES == BS && NS >= 1, "tile");
  __shared__ CodeBook book[F::NU > 0 ? 2 : 1];
  __shared__ float red[2][NP][4];
  __shared__ typename F::Const ks[GROUPED ? QFX_MAX_PARAM_GROUPS : 1];
  const CodeBook& sbook = book[0];
  const CodeBook& ubook = book[F::NU > 0 ? 1 : 0];
  const int t = threadIdx.x;
  book[0].fill(a.qmap1, t);
  if constexpr (F::NU > 0) book[1].fill(a.qmap2, t);
  const float clip = opt_clip(a.gnorm_sq, a.max_norm, a.grad_scale);
  typename F::Const k;
  if (GROUPED) {
    if (t < n_groups) ks[t] = F::konst(tab->g[t]);
  } else {
    k = F::konst(own);
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
    float p[E], g[E], s[NP][E];
    const auto step = [&](auto fp32_entry, int j) {
      float x[NP];
#pragma unroll
      for (int i = 0; i < NP; ++i) x[i] = s[i][j];
      F::template elem<decltype(fp32_entry)::value>(p[j], g[j], x, clip, k);
#pragma unroll
      for (int i = 0; i < NP; ++i) s[i][j] = x[i];
    };
    tile_load<E>(a.p, base, n, p);
    tile_load<E>(a.g, base, n, g);
    if (e.mode == QFX_ADAM8BIT_FP32) {
      const int64_t sb = e.state + (int64_t)lane * E;
#pragma unroll
      for (int i = 0; i < NP; ++i) tile_load<E>(F::moment(a, i), sb, n, s[i]);
#pragma unroll
      for (int j = 0; j < E; ++j) step(std::true_type(), j);
      tile_store<E>(a.p, base, n, p);
#pragma unroll
      for (int i = 0; i < NP; ++i) tile_store<E>(F::moment(a, i), sb, n, s[i]);
      continue;
    }
    int c[E];
    float am[NP], mx[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) am[i] = F::absmax(a, i)[e.state];      // all block maxima first: the loads the decode waits for longest
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      tile_load_codes<E>(F::codes(a, i), base, n, c);
#pragma unroll
      for (int j = 0; j < E; ++j) s[i][j] = (i < NS ? sbook : ubook).q[c[j]] * am[i];
      mx[i] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < E; ++j) {
      if (j < n) {
        step(std::false_type(), j);
#pragma unroll
        for (int i = 0; i < NP; ++i) mx[i] = fmaxf(mx[i], fabsf(s[i][j]));
      }
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) mx[i] = wave_max(mx[i]);
    if (WG) {
#pragma unroll
      for (int i = 0; i < NP; ++i)
        if ((t & 63) == 0) red[parity][i][t >> 6] = mx[i];
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NP; ++i) mx[i] = fmaxf(fmaxf(red[parity][i][0], red[parity][i][1]), fmaxf(red[parity][i][2], red[parity][i][3]));
      parity ^= 1;
    }
    tile_store<E>(a.p, base, n, p);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
#pragma unroll
      for (int j = 0; j < E; ++j)
        c[j] = i < NS ? signed_code(sbook, s[i][j], mx[i]) : nearest_code(ubook.mid, mx[i] > 0.f ? s[i][j] / mx[i] : 0.f);
      tile_store_codes<E>(F::codes(a, i), base, n, c);
      if (lane == 0) F::absmax(a, i)[e.state] = mx[i];
    }
  }
}

// what every blockwise entry refuses: a null pointer (gnorm_sq may be null), a blocksize outside {256, 2048}, an empty table
template <typename F>
inline bool blockwise_args_ok(const typename F::Args* a) {
  if (!a || !a->p || !a->g || !a->q1 || !a->absmax1 || !a->m32 || !a->table || !a->qmap1) return false;
  if constexpr (F::NU > 0)
    if (!a->q2 || !a->absmax2 || !a->v32 || !a->qmap2) return false;
  return (a->blocksize == 256 || a->blocksize == 2048) && a->n_blocks > 0;
}

// one launch of a family's kernel at the table's block size; `rest`: what the kernel takes behind the argument struct
template <auto K256, auto K2048, typename A, typename... X>
inline int launch_blockwise(const A& a, void* stream, X... rest) {
  launch_either<K256, K2048>(a.blocksize == 256, blockwise_grid(a.n_blocks, a.blocksize), stream, a, rest...);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

}  // namespace
