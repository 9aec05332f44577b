// qfx_scaled_adamw.hip -- Riemannian-preconditioned ("scaled") AdamW for LoRA pairs (Zhang & Pilanci, "Riemannian Preconditioned
// LoRA", ICML 2024) over the flat LoRA buffers; the listing in include/qfx.h is the specification.  ONE launch of one 256-lane
// workgroup per adapter pair, driven by a device table, laid out like qfx_maxnorm.hip:
//   0. every g of the pair is read once: a non-finite one and the pair is left (nothing has been written yet)
//   1. G_A = A A^T and G_B = B^T B in fp64 from the fp32 weights (every product exact): the upper triangle in 4 x 4 blocks, a lane
//      owns one block and one residue class of the summed index, A / B stream through one LDS tile stored k-major with an odd row
//      stride; the classes are folded through LDS in class order into the two full matrices (LDS, fp64), reg is added to the diagonals
//   2. both matrices are factorised in place (Cholesky, right-looking, lanes 0-127 on G_A and 128-255 on G_B); a pivot that is not
//      positive and finite and the pair is left.  Wave 0 / wave 1 then solve L Y = I and L^T X = Y, a lane per column of the
//      identity: P_A = G_A^-1, P_B = G_B^-1, copied over the factors
//   3. a second sweep streams g' = g * clip through the LDS tile, forms g^ = fp32(P_B g'_A) resp. fp32(g'_B P_A) -- an fp64 dot over
//      the r terms in index order -- and applies AdamW to the element it belongs to
// One fp64 rounding per fp64 operation (no FMA contraction; the Gram products are exact either way).  Nothing crosses a workgroup
// but the integer skip counter (an integer atomic add: its value does not depend on the order), every sum runs in an order fixed
// by the shape: same inputs -> same bits.  16-byte accesses for a tensor whose four addresses (p, g, exp_avg, exp_avg_sq at its
// offset) are 16-byte aligned and whose row length (in_features for A, r for B) is a multiple of 4, scalar ones otherwise.
// Built with the compiler's default contraction like qfx_optim.hip, so that opt_clip (qfx_optim.h, included above the pragma) forms
// the clip factor as adamw_kernel's does; everything below the pragma rounds every operation, and adamw_apply pins adamw_elem's
// fusions (qfx_optim.hip) with explicit fmaf calls: precondition = 0 gives qfx_adamw_step's bits.
#include "qfx_common.h"
#include "qfx_optim.h"

#include <cmath>

#pragma clang fp contract(off)

#include "qfx_pair_linalg.h"                // the Gram sweep and the table check

namespace {

constexpr int RMAX = MAT_N;                 // largest rank
constexpr int TILE_F = 16384;               // 64 KB: the A / B tile of the Gram sweeps; the staging area of the fold (16 x 256 fp64);
                                            // the two [64][64] fp64 right-hand sides of the solves; the g tile of the second sweep

struct Hyper { float lr, b1, b2, eps, wd, step, rs2; };

// adamw_elem of qfx_optim.hip behind its g * clip: the same operations with the same fusions, on the gradient the caller formed
__device__ __forceinline__ void adamw_apply(float& p, float gi, float& m, float& v, const Hyper& h) {
  const float pi = p * fmaf(-h.lr, h.wd, 1.0f);
  const float mi = fmaf(1.0f - h.b1, gi, h.b1 * m);
  const float vi = h.b2 * v + ((1.0f - h.b2) * gi) * gi;
  p = pi - (h.step * mi) / fmaf(h.rs2, sqrtf(vi), h.eps);
  m = mi; v = vi;
}

// In-place Cholesky factor (lower triangle and diagonal of M) by `nth` lanes, lane lt of them; every lane of the workgroup takes
// every barrier.  Returns 1 when a pivot was not positive and finite (the factor is then garbage and is not used).
__device__ __forceinline__ int cholesky(double* M, int r, int lt, int nth) {
  int bad = 0;
  for (int k = 0; k < r; ++k) {
    __syncthreads();                       // the trailing update of column k - 1 is complete
    const double piv = M[k * LDM + k];
    const bool ok = piv > 0.0 && __builtin_isfinite(piv);
    bad |= !ok;
    const double d = ok ? sqrt(piv) : 1.0;
    __syncthreads();                       // every lane has read the pivot
    for (int i = k + lt; i < r; i += nth) M[i * LDM + k] = i == k ? d : M[i * LDM + k] / d;
    __syncthreads();
    const int m = r - k - 1;
    for (int e = lt; e < m * m; e += nth) {
      const int i = k + 1 + e / m, j = k + 1 + e % m;
      if (j <= i) M[i * LDM + j] = M[i * LDM + j] - M[i * LDM + k] * M[j * LDM + k];
    }
  }
  return bad;
}

// Column c of (L L^T)^-1 into W[.][c] (W [r][RMAX]): L Y = e_c forward, L^T X = Y backward, in place.  One lane per column.
__device__ __forceinline__ void solve_column(const double* L, double* W, int r, int c) {
  for (int i = 0; i < r; ++i) {
    double s = i == c ? 1.0 : 0.0;
    for (int j = 0; j < i; ++j) s = s - L[i * LDM + j] * W[j * RMAX + c];
    W[i * RMAX + c] = s / L[i * LDM + i];
  }
  for (int i = r - 1; i >= 0; --i) {
    double s = W[i * RMAX + c];
    for (int j = i + 1; j < r; ++j) s = s - L[j * LDM + i] * W[j * RMAX + c];
    W[i * RMAX + c] = s / L[i * LDM + i];
  }
}

// Second sweep over one tensor of n_rows rows of `len` elements at `off`: g' = g * clip through the LDS tile in slices of whole
// rows (is_a = false: B, a slice is one contiguous run) or of columns (is_a = true: A), then per element
//   A: g^[i][k] = fp32(sum_j P[i][j] g'[j][k])      B: g^[o][i] = fp32(sum_j g'[o][j] P[j][i])      (pre; else g^ = g')
// and AdamW.  E = 4: 16-byte accesses (the four addresses 16-byte aligned, the row length a multiple of 4), E = 1: scalar ones.
template <int E, bool IS_A>
__device__ __forceinline__ void sweep(const qfx_scaled_adamw_args& a, int64_t off, int r, int n, float clip, const double* P, bool pre,
                                      float* tile, const Hyper& h, int tid) {
  const float* __restrict__ g = a.g + off;
  float* p = a.p + off;
  float* m = a.exp_avg + off;
  float* v = a.exp_avg_sq + off;
  // A [r, n]: KT columns of all r rows, tile[j * KT + k].  B [n, r]: KT whole rows, tile[o * r + j].
  const int KT = IS_A ? (TILE_F / r) & ~3 : TILE_F / r;
  for (int64_t k0 = 0; k0 < n; k0 += KT) {
    const int kt = (int)(n - k0 < KT ? n - k0 : KT);
    const int items = IS_A ? r * (kt / E) : (kt * r) / E;      // E = 4: kt resp. r is a multiple of 4
    const int ktq = kt / E;
    __syncthreads();                       // the previous slice has been read; P is complete
    for (int e = tid; e < items; e += NT) {
      int at_t;                            // first element of the item in the tile
      int64_t at_g;                        // ... and in the tensor
      if (IS_A) {
        const int j = e / ktq, kq = e - j * ktq;
        at_t = j * KT + E * kq;
        at_g = (int64_t)j * n + k0 + E * kq;
      } else {
        at_t = E * e;
        at_g = k0 * r + E * e;
      }
      if (E == 4) {
        f32x4 x = *reinterpret_cast<const f32x4*>(g + at_g);
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = x[c] * clip;
        *reinterpret_cast<f32x4*>(tile + at_t) = x;
      } else {
        tile[at_t] = g[at_g] * clip;
      }
    }
    __syncthreads();
    for (int e = tid; e < items; e += NT) {
      int at_t, row, col;                  // A: (row i, first column) of the item; B: (row o, first rank index i)
      int64_t at_g;
      if (IS_A) {
        row = e / ktq;
        col = E * (e - row * ktq);
        at_t = row * KT + col;
        at_g = (int64_t)row * n + k0 + col;
      } else {
        row = (E * e) / r;
        col = E * e - row * r;
        at_t = E * e;
        at_g = k0 * r + E * e;
      }
      float gh[E];
      if (pre) {
        double acc[E];
#pragma unroll
        for (int c = 0; c < E; ++c) acc[c] = 0.0;
        for (int j = 0; j < r; ++j) {
          if (IS_A) {
            const double pij = P[row * LDM + j];
#pragma unroll
            for (int c = 0; c < E; ++c) acc[c] = acc[c] + pij * (double)tile[j * KT + col + c];
          } else {
            const double gj = (double)tile[row * r + j];
#pragma unroll
            for (int c = 0; c < E; ++c) acc[c] = acc[c] + gj * P[j * LDM + col + c];
          }
        }
#pragma unroll
        for (int c = 0; c < E; ++c) gh[c] = (float)acc[c];
      } else {
#pragma unroll
        for (int c = 0; c < E; ++c) gh[c] = tile[at_t + c];
      }
      if (E == 4) {
        f32x4 pv = *reinterpret_cast<const f32x4*>(p + at_g);
        f32x4 mv = *reinterpret_cast<const f32x4*>(m + at_g);
        f32x4 vv = *reinterpret_cast<const f32x4*>(v + at_g);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float pj = pv[c], mj = mv[c], vj = vv[c];
          adamw_apply(pj, gh[c], mj, vj, h);
          pv[c] = pj; mv[c] = mj; vv[c] = vj;
        }
        *reinterpret_cast<f32x4*>(p + at_g) = pv;
        *reinterpret_cast<f32x4*>(m + at_g) = mv;
        *reinterpret_cast<f32x4*>(v + at_g) = vv;
      } else {
        float pj = p[at_g], mj = m[at_g], vj = v[at_g];
        adamw_apply(pj, gh[0], mj, vj, h);
        p[at_g] = pj; m[at_g] = mj; v[at_g] = vj;
      }
    }
  }
}

__device__ __forceinline__ bool aligned16(const qfx_scaled_adamw_args& a, int64_t off) {
  return ((((uintptr_t)(a.p + off)) | ((uintptr_t)(a.g + off)) | ((uintptr_t)(a.exp_avg + off)) | ((uintptr_t)(a.exp_avg_sq + off))) & 15) == 0;
}

__device__ __forceinline__ Hyper hyper_of(const qfx_scaled_adamw_args& a, float lr_ratio, float wd) {
  Hyper h;
  h.lr = a.lr * lr_ratio;
  h.b1 = a.beta1; h.b2 = a.beta2; h.eps = a.eps; h.wd = wd;
  h.step = h.lr / a.bias_corr1;            // as adamw_kernel forms them, once per tensor
  h.rs2 = 1.0f / sqrtf(a.bias_corr2);
  return h;
}

__global__ __launch_bounds__(NT) void scaled_adamw_kernel(const qfx_scaled_adamw_args a) {
  __shared__ __attribute__((aligned(16))) float tile[TILE_F];
  __shared__ double MA[RMAX * LDM];        // G_A, its factor, then P_A
  __shared__ double MB[RMAX * LDM];        // G_B, its factor, then P_B
  const int tid = threadIdx.x;
  const qfx_scaled_adamw_pair t = a.table[blockIdx.x];
  if (QFX_PAIR_REFUSED(t, RMAX)) return;   // what qfx_scaled_adamw_check_table refuses is never touched
  const int r = t.r, nin = t.in_features, nout = t.out_features;
  const int64_t na = (int64_t)r * nin, nb = (int64_t)nout * r;
  const float clip = opt_clip(a.gnorm_sq, a.max_norm, a.grad_scale);
  const bool pre = a.precondition != 0;

  int bad = 0;
  for (int64_t i = tid; i < na; i += NT) bad |= !__builtin_isfinite(a.g[t.off_a + i]);
  for (int64_t i = tid; i < nb; i += NT) bad |= !__builtin_isfinite(a.g[t.off_b + i]);
  if (pre) {
    const double reg = (double)a.reg;
    gram<TILE_F, true>(a.p + t.off_a, true, r, nin, tile, MA, tid, reg);
    gram<TILE_F, true>(a.p + t.off_b, false, r, nout, tile, MB, tid, reg);
    bad |= cholesky(tid < NT / 2 ? MA : MB, r, tid & (NT / 2 - 1), NT / 2);
  }
  if (__syncthreads_or(bad)) {             // the same verdict on every lane; nothing of the pair has been written
    if (tid == 0) atomicAdd(a.skipped, 1);
    return;
  }
  if (pre) {
    double* W = reinterpret_cast<double*>(tile);
    if (tid < 2 * 64) {
      const int c = tid & 63;
      if (c < r) solve_column(tid < 64 ? MA : MB, W + (tid < 64 ? 0 : RMAX * RMAX), r, c);
    }
    __syncthreads();
    for (int e = tid; e < 2 * r * r; e += NT) {
      const int which = e >= r * r, f = e - which * r * r, i = f / r, j = f - i * r;
      (which ? MB : MA)[i * LDM + j] = W[which * RMAX * RMAX + i * RMAX + j];
    }
  }
  const Hyper ha = hyper_of(a, t.lr_ratio_a, t.wd_a), hb = hyper_of(a, t.lr_ratio_b, t.wd_b);
  if (aligned16(a, t.off_a) && (nin & 3) == 0) sweep<4, true>(a, t.off_a, r, nin, clip, MB, pre, tile, ha, tid);
  else                                         sweep<1, true>(a, t.off_a, r, nin, clip, MB, pre, tile, ha, tid);
  if (aligned16(a, t.off_b) && (r & 3) == 0)   sweep<4, false>(a, t.off_b, r, nout, clip, MA, pre, tile, hb, tid);
  else                                         sweep<1, false>(a, t.off_b, r, nout, clip, MA, pre, tile, hb, tid);
}

inline bool ratio_ok(float x) { return std::isfinite(x) && x >= 0.f; }

}  // namespace

extern "C" int qfx_scaled_adamw_check_table(const qfx_scaled_adamw_pair* host_table, int32_t n_pairs, int64_t n_elems) {
  return check_pair_table(n_pairs, n_elems, host_table != nullptr, RMAX, [&](int32_t i, PairDims& d) {
    const qfx_scaled_adamw_pair& t = host_table[i];
    d = pair_dims(t);
    return ratio_ok(t.lr_ratio_a) && ratio_ok(t.lr_ratio_b) && ratio_ok(t.wd_a) && ratio_ok(t.wd_b);
  });
}

extern "C" int qfx_scaled_adamw_step(const qfx_scaled_adamw_args* a, void* stream) {
  if (!a || a->n_pairs < 0) return QFX_EINVAL;
  if (!(a->lr >= 0.f) || !beta_ok(a->beta1) || !beta_ok(a->beta2) || !(a->eps >= 0.f)) return QFX_EINVAL;
  if (!(a->bias_corr1 > 0.f) || !(a->bias_corr2 > 0.f)) return QFX_EINVAL;
  if (a->precondition != 0 && a->precondition != 1) return QFX_EINVAL;
  if (a->precondition && (!(a->reg > 0.f) || !std::isfinite(a->reg))) return QFX_EINVAL;
  if (!(a->max_norm == a->max_norm) || !std::isfinite(a->grad_scale)) return QFX_EINVAL;
  if (a->n_pairs == 0) return QFX_OK;
  if (!a->p || !a->g || !a->exp_avg || !a->exp_avg_sq || !a->table || !a->skipped) return QFX_EINVAL;
  if (hipMemsetAsync(a->skipped, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return QFX_EINVAL;
  hipLaunchKernelGGL(scaled_adamw_kernel, dim3((unsigned)a->n_pairs), dim3(NT), 0, (hipStream_t)stream, *a);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
