// qfx_maxnorm.hip -- max-norm regularisation of the adapters (kohya's --scale_weight_norms, LoRANetwork.apply_max_norm_regularization)
// over the flat LoRA buffer, see include/qfx.h.  ONE launch of one 256-lane workgroup per adapter pair, driven by a device table, and
// a second one-block launch for the three summary numbers.  Per pair the product B A is never formed:
//   ||B A||_F^2 = sum_ij (A A^T)_ij (B^T B)_ij
// Both r x r Gram matrices are accumulated in fp64 from the fp32 weights (a product of two widened fp32 values is exact in fp64, so
// an fma and a separately rounded multiply-add give the same bits).  The upper triangle is cut into T x T blocks (T = 4 up to r = 64,
// 8 above); a lane owns ONE block and one residue class of the summed index (`ksplit` classes, as many as 256 lanes allow), its
// T x T partial sums stay in fp64 registers.  A and B stream through one LDS tile, stored k-major with an odd row stride: the lanes
// of a wave that share a block read consecutive k conflict-free, the lanes that share a k read one short row.  A's partial sums are
// folded over the residue classes through LDS in class order into the full Gram matrix (LDS, fp64); B's partial sums are contracted
// with it where they are (the contraction is linear in them) and the 256 lane sums are folded by a fixed tree.  One lane forms
// norm_raw, ratio and q; then the whole workgroup scales the pair.  No atomics, nothing crosses a workgroup, every sum runs in an
// order fixed by the shape: same inputs -> same bits.
// Compiled without FMA contraction (the pragma below and -ffp-contract=off in the build): ratio, q, the scaled norm and the scaled
// weights are one fp32 operation each, where tests/maxnorm_ref.py rounds them.
#include "qfx_common.h"

#include <cmath>

#pragma clang fp contract(off)

#include "qfx_pair_linalg.h"                // fill_a, fill_b, gram_tile and the table check

namespace {

constexpr int RMAX = 128;                   // largest rank
constexpr int TILE_F = 16384;               // 64 KB: the A / B tile; then the staging area of the fold (16 x 256 fp64 = 32 KB)
constexpr int NBLK_MAX = 136;               // 16 * 17 / 2 blocks of the upper triangle: r = 64 at T = 4, r = 128 at T = 8
constexpr int G_ELEMS = NBLK_MAX * 64;      // the full Gram matrix of A, block by block (68 KB of fp64 at T = 8)
constexpr int SUM_TILE = 1024;

// x[0..n) *= q, one fp32 multiply per element: scalar accesses up to the first 16-byte boundary and behind the last whole quad
__device__ __forceinline__ void scale_range(float* x, int64_t n, float q, int tid) {
  int64_t head = (4 - (int64_t)(((uintptr_t)x >> 2) & 3)) & 3;
  head = head < n ? head : n;
  if (tid < head) x[tid] = x[tid] * q;
  const int64_t nv = (n - head) >> 2;
  float* body = x + head;
  for (int64_t i = tid; i < nv; i += NT) {
    f32x4 v = *reinterpret_cast<f32x4*>(body + 4 * i);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = v[j] * q;
    *reinterpret_cast<f32x4*>(body + 4 * i) = v;
  }
  for (int64_t i = head + 4 * nv + tid; i < n; i += NT) x[i] = x[i] * q;
}

template <int T>
__device__ __forceinline__ void pair_body(const qfx_maxnorm_args& a, const qfx_maxnorm_pair& t, int pi, float* tile, double* G,
                                          double* red, float* bcast) {
  constexpr int TT = T * T;
  const int tid = threadIdx.x;
  const int r = t.r, nin = t.in_features, nout = t.out_features;
  const int nb = (r + T - 1) / T, nblk = nb * (nb + 1) / 2, ksplit = NT / nblk;
  const int rp = nb * T, S = rp + 1, KT = (TILE_F / S) & ~3;          // S odd; KT >= 124 rows of the tile, a multiple of 4
  const int blk = tid / ksplit, ks = tid - blk * ksplit;
  const bool active = blk < nblk;
  int bi = 0, bj = 0;                                                  // block (bi, bj), bi <= bj, row-major over the upper triangle
  if (active) {
    int rem = blk;
    while (rem >= nb - bi) { rem -= nb - bi; ++bi; }
    bj = bi + rem;
  }
  const int i0 = bi * T, j0 = bj * T;
  float* A = a.p + t.off_a;
  float* B = a.p + t.off_b;
  const bool vec_a = (((uintptr_t)A & 15) == 0) && (nin & 3) == 0;
  const bool vec_b = (((uintptr_t)B & 15) == 0) && (r & 3) == 0;

  double acc[TT];
#pragma unroll
  for (int u = 0; u < TT; ++u) acc[u] = 0.0;
  for (int64_t k0 = 0; k0 < nin; k0 += KT) {
    const int kt = (int)(nin - k0 < KT ? nin - k0 : KT);
    __syncthreads();                       // the previous tile has been read
    fill_a(tile, A, r, rp, S, nin, k0, kt, vec_a, tid);
    __syncthreads();
    if (active) gram_tile<T>(tile, S, kt, i0, j0, ks, ksplit, acc);
  }

  // G = A A^T: per block and element the partial sums of the residue classes in class order, 16 elements of the block at a time
  double* stage = reinterpret_cast<double*>(tile);
#pragma unroll
  for (int sl = 0; sl < TT / 16; ++sl) {
    __syncthreads();                       // the tile (or the previous slice) has been read
#pragma unroll
    for (int u = 0; u < 16; ++u) stage[u * NT + tid] = acc[sl * 16 + u];
    __syncthreads();
    for (int e = tid; e < nblk * 16; e += NT) {
      const int b = e >> 4, u = e & 15;
      const double* s = stage + u * NT + b * ksplit;
      double v = s[0];
      for (int x = 1; x < ksplit; ++x) v += s[x];
      G[b * TT + sl * 16 + u] = v;
    }
  }

#pragma unroll
  for (int u = 0; u < TT; ++u) acc[u] = 0.0;
  for (int64_t k0 = 0; k0 < nout; k0 += KT) {
    const int kt = (int)(nout - k0 < KT ? nout - k0 : KT);
    __syncthreads();                       // the stage / the previous tile has been read; G is complete
    fill_b(tile, B, r, rp, S, k0, kt, vec_b, tid);
    __syncthreads();
    if (active) gram_tile<T>(tile, S, kt, i0, j0, ks, ksplit, acc);
  }

  // sum_ij G_ij (B^T B)_ij: a diagonal block holds both triangles, every other block stands for its mirror image too
  double loc = 0.0;
  if (active) {
#pragma unroll
    for (int u = 0; u < TT; ++u) loc += G[blk * TT + u] * acc[u];
    if (bi != bj) loc *= 2.0;
  }
  red[tid] = loc;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    double sum = red[0];
    if (sum < 0.0) sum = 0.0;              // rounding of a cancelling sum; a NaN stays
    const float norm_raw = (float)(fabs((double)t.scale) * sqrt(sum));
    float ratio = 1.0f, q = 1.0f;
    if (__builtin_isfinite(norm_raw) && norm_raw > a.max_norm) {
      ratio = a.max_norm / norm_raw;
      q = sqrtf(ratio);
    }
    a.norms[pi] = norm_raw * ratio;
    a.ratios[pi] = ratio;
    bcast[0] = q;
    bcast[1] = ratio != 1.0f ? 1.0f : 0.0f;
  }
  __syncthreads();
  if (bcast[1] != 0.0f) {
    const float q = bcast[0];
    scale_range(A, (int64_t)r * nin, q, tid);
    scale_range(B, (int64_t)nout * r, q, tid);
  }
}

__global__ __launch_bounds__(NT) void maxnorm_kernel(const qfx_maxnorm_args a) {
  __shared__ __attribute__((aligned(16))) float tile[TILE_F];
  __shared__ double G[G_ELEMS];
  __shared__ double red[NT];
  __shared__ float bcast[2];
  const int pi = blockIdx.x;
  const qfx_maxnorm_pair t = a.table[pi];
  if (QFX_PAIR_REFUSED(t, RMAX)) {         // what qfx_maxnorm_check_table refuses is never touched
    if (threadIdx.x == 0) {
      a.norms[pi] = 0.f;
      a.ratios[pi] = 1.f;
    }
    return;
  }
  if (t.r <= 64) pair_body<4>(a, t, pi, tile, G, red, bcast);
  else           pair_body<8>(a, t, pi, tile, G, red, bcast);
}

// ONE block: the per-pair values staged through LDS and read by one lane in pair order
__global__ __launch_bounds__(NT) void maxnorm_summary_kernel(const float* __restrict__ norms, const float* __restrict__ ratios, int n,
                                                             float* __restrict__ summary) {
  __shared__ float tn[SUM_TILE];
  __shared__ float tr[SUM_TILE];
  double sum = 0.0;
  float mx = -INFINITY;
  int cnt = 0;
  for (int base = 0; base < n; base += SUM_TILE) {
    const int m = min(SUM_TILE, n - base);
    for (int i = threadIdx.x; i < m; i += NT) {
      tn[i] = norms[base + i];
      tr[i] = ratios[base + i];
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < m; ++i) {
        const float v = tn[i];
        sum += (double)v;
        if (v > mx || v != v) mx = v;      // a NaN norm is reported: it stays once taken
        cnt += tr[i] != 1.0f;
      }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    summary[0] = (float)cnt;
    summary[1] = (float)(sum / (double)n);
    summary[2] = mx;
    summary[3] = 0.f;
  }
}

}  // namespace

extern "C" int qfx_maxnorm_check_table(const qfx_maxnorm_pair* host_table, int32_t n_pairs, int64_t n_elems) {
  return check_pair_table(n_pairs, n_elems, host_table != nullptr, RMAX, [&](int32_t i, PairDims& d) {
    d = pair_dims(host_table[i]);
    return std::isfinite(host_table[i].scale);
  });
}

extern "C" int qfx_maxnorm_apply(const qfx_maxnorm_args* a, void* stream) {
  if (!a || a->n_pairs < 0) return QFX_EINVAL;
  if (!(a->max_norm > 0.f)) return QFX_EINVAL;                        // a NaN fails
  if (a->n_pairs == 0) return QFX_OK;
  if (!a->p || !a->table || !a->norms || !a->ratios || !a->summary) return QFX_EINVAL;
  hipLaunchKernelGGL(maxnorm_kernel, dim3((unsigned)a->n_pairs), dim3(NT), 0, (hipStream_t)stream, *a);
  QFX_CHECK_LAUNCH();
  hipLaunchKernelGGL(maxnorm_summary_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (const float*)a->norms, (const float*)a->ratios,
                     a->n_pairs, a->summary);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
