// What the one-workgroup-per-LoRA-pair kernels share (qfx_maxnorm.hip, qfx_scaled_adamw.hip, qfx_lora_svd.hip and
// qfx_lora_extract.hip): the descriptor check of a pair table, the streamed fp64 Gram sweep of A [r, in] / B [out, r] and the
// cyclic Jacobi eigensolver of a small symmetric matrix in LDS.  Helpers only, and NO fp-contract pragma: contraction is lexical,
// so include this BELOW the unit's `#pragma clang fp contract(off)` -- every fp64 operation here rounds once, which is what the
// restatements under tests/ (maxnorm_ref.py, scaled_adamw_ref.py, lora_svd_ref.py, lora_extract_ref.py) expect of it.
// The bodies keep the shape in which the kernels were written, so that the instruction streams of the four files did not move.
#pragma once
#include "qfx_common.h"

#include <algorithm>
#include <utility>
#include <vector>

namespace {      // file-local in every translation unit

constexpr int NT = 256;                     // four waves: the workgroup of every kernel here
constexpr int DIM_MAX = 1 << 24;            // largest in_features / out_features
constexpr int MAT_N = 64;                   // largest order of an fp64 matrix in LDS
constexpr int LDM = MAT_N + 1;              // its row stride

// ---- the descriptor of a pair, as every table states it -------------------------------------------------------------------------

struct PairDims { int64_t off_a, off_b; int32_t r, in_features, out_features; };

template <class P>
__host__ __device__ inline PairDims pair_dims(const P& t) { return {t.off_a, t.off_b, t.r, t.in_features, t.out_features}; }

// The dimensions and offsets a kernel will not touch: the host check refuses a table with such a row, and a kernel leaves the row
// alone.  t: a table row or a PairDims.  A macro, not a function: as an inlined callee the same expression compiles to another
// prologue in every kernel.
#define QFX_PAIR_REFUSED(t, rmax)                                                                                  \
  ((t).r < 1 || (t).r > (rmax) || (t).in_features < 1 || (t).in_features > DIM_MAX || (t).out_features < 1 || \
   (t).out_features > DIM_MAX || (t).off_a < 0 || (t).off_b < 0)

// The common part of every *_check_table: the guards, then per row row(i, d) -- false refuses the row for a reason of that table's
// own (a scale, an lr ratio, k / r_dst, a leading dimension), otherwise d is the row's A [r, in] at off_a and B [out, r] at off_b
// -- QFX_PAIR_REFUSED, both matrices inside [0, n_elems), and no two matrices of the table overlapping (of one pair or of two).
template <class Row>
inline int check_pair_table(int32_t n_pairs, int64_t n_elems, bool have_table, int rmax, Row row) {
  if (n_pairs < 0 || n_elems < 0 || (n_pairs > 0 && !have_table)) return QFX_EINVAL;
  std::vector<std::pair<int64_t, int64_t>> spans;
  spans.reserve(2 * (size_t)n_pairs);
  for (int32_t i = 0; i < n_pairs; ++i) {
    PairDims d;
    if (!row(i, d) || QFX_PAIR_REFUSED(d, rmax)) return QFX_EINVAL;
    const int64_t na = (int64_t)d.r * d.in_features, nb = (int64_t)d.out_features * d.r;
    if (na > n_elems || nb > n_elems || d.off_a > n_elems - na || d.off_b > n_elems - nb) return QFX_EINVAL;
    spans.emplace_back(d.off_a, d.off_a + na);
    spans.emplace_back(d.off_b, d.off_b + nb);
  }
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i)
    if (spans[i].first < spans[i - 1].second) return QFX_EINVAL;
  return QFX_OK;
}

// ---- the Gram sweep --------------------------------------------------------------------------------------------------------------

// A tile: element (i, k) of the r x kt slice that starts at column k0 of A [r, ld] -> tile[k * S + i]; rows r..rp-1 are zeros.
// vec: A and ld are multiples of 16 bytes / 4 elements (k0 and kt then are, too).
__device__ __forceinline__ void fill_a(float* tile, const float* __restrict__ g, int r, int rp, int S, int64_t ld, int64_t k0, int kt,
                                       bool vec, int tid) {
  if (vec) {
    const unsigned nq = (unsigned)kt >> 2;
#pragma unroll 4
    for (unsigned e = tid; e < (unsigned)r * nq; e += NT) {
      const unsigned i = e / nq, kq = e - i * nq;
      const f32x4 v = *reinterpret_cast<const f32x4*>(g + (int64_t)i * ld + k0 + 4 * kq);
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[(4 * kq + j) * S + i] = v[j];
    }
    const unsigned np = (unsigned)(rp - r);
    for (unsigned e = tid; e < (unsigned)kt * np; e += NT) {
      const unsigned k = e / np;
      tile[k * S + r + (e - k * np)] = 0.f;
    }
  } else {
#pragma unroll 4
    for (unsigned e = tid; e < (unsigned)rp * (unsigned)kt; e += NT) {
      const unsigned i = e / (unsigned)kt, k = e - i * (unsigned)kt;
      tile[k * S + i] = i < (unsigned)r ? g[(int64_t)i * ld + k0 + k] : 0.f;
    }
  }
}

// B tile: element (i, k) of the kt rows that start at row k0 of B [out, r] -> tile[k * S + i] (the summed index is B's row index:
// the slice is one contiguous run of kt * r floats).  vec: B is 16-byte aligned and r % 4 == 0 (a quad then lies in one row).
__device__ __forceinline__ void fill_b(float* tile, const float* __restrict__ g, int r, int rp, int S, int64_t k0, int kt, bool vec,
                                       int tid) {
  const float* src = g + k0 * r;
  if (vec) {
    const unsigned nq = ((unsigned)kt * (unsigned)r) >> 2;
#pragma unroll 4
    for (unsigned q = tid; q < nq; q += NT) {
      const unsigned k = (4 * q) / (unsigned)r, i = 4 * q - k * (unsigned)r;
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[k * S + i + j] = v[j];
    }
    const unsigned np = (unsigned)(rp - r);
    for (unsigned e = tid; e < (unsigned)kt * np; e += NT) {
      const unsigned k = e / np;
      tile[k * S + r + (e - k * np)] = 0.f;
    }
  } else {
#pragma unroll 4
    for (unsigned e = tid; e < (unsigned)kt * (unsigned)rp; e += NT) {
      const unsigned k = e / (unsigned)rp, i = e - k * (unsigned)rp;
      tile[k * S + i] = i < (unsigned)r ? src[(int64_t)k * r + i] : 0.f;
    }
  }
}

// acc[u][v] += sum over this lane's k of tile[k][i0 + u] * tile[k][j0 + v]: both factors are widened fp32, the product is exact
template <int T>
__device__ __forceinline__ void gram_tile(const float* tile, int S, int kt, int i0, int j0, int ks, int ksplit, double (&acc)[T * T]) {
  for (int k = ks; k < kt; k += ksplit) {
    const float* row = tile + k * S;
    double a[T], c[T];
#pragma unroll
    for (int u = 0; u < T; ++u) {
      a[u] = (double)row[i0 + u];
      c[u] = (double)row[j0 + u];
    }
#pragma unroll
    for (int u = 0; u < T; ++u) {
#pragma unroll
      for (int v = 0; v < T; ++v) acc[u * T + v] = __builtin_fma(a[u], c[v], acc[u * T + v]);
    }
  }
}

// The Gram matrix of one tensor into M [r][LDM] (both triangles).  is_a: X = A [r, n], summed over its columns; else X = B [n, r],
// summed over its rows.  The upper triangle in 4 x 4 blocks: a lane owns ONE block (bi, bj) and one residue class ks of the summed
// index (`ksplit` classes, as many as 256 lanes allow); X streams through a tile of TILE_F floats, stored k-major with the odd row
// stride S, KT rows (a multiple of 4) at a time; then the partial sums of the classes are folded through the tile (16 x 256 fp64)
// in class order.  REG: reg is added to the diagonal.  Opens with a barrier (whatever the caller kept in the tile has been read);
// M is complete at the caller's next barrier.
template <int TILE_F, bool REG = false>
__device__ __forceinline__ void gram(const float* __restrict__ X, bool is_a, int r, int n, float* tile, double* M, int tid,
                                     double reg = 0.0) {
  constexpr int T = 4, TT = T * T;
  const int nb = (r + T - 1) / T, nblk = nb * (nb + 1) / 2, ksplit = NT / nblk;
  const int rp = nb * T, S = rp + 1, KT = (TILE_F / S) & ~3;
  const int blk = tid / ksplit, ks = tid - blk * ksplit;
  const bool active = blk < nblk;
  int bi = 0, bj = 0;                                                  // block (bi, bj), bi <= bj, row-major over the upper triangle
  if (active) {
    int rem = blk;
    while (rem >= nb - bi) { rem -= nb - bi; ++bi; }
    bj = bi + rem;
  }
  const bool vec = (((uintptr_t)X & 15) == 0) && ((is_a ? n : r) & 3) == 0;
  double acc[TT];
#pragma unroll
  for (int u = 0; u < TT; ++u) acc[u] = 0.0;
  for (int64_t k0 = 0; k0 < n; k0 += KT) {
    const int kt = (int)(n - k0 < KT ? n - k0 : KT);
    __syncthreads();                       // the previous tile has been read
    if (is_a) fill_a(tile, X, r, rp, S, n, k0, kt, vec, tid);
    else      fill_b(tile, X, r, rp, S, k0, kt, vec, tid);
    __syncthreads();
    if (active) gram_tile<T>(tile, S, kt, bi * T, bj * T, ks, ksplit, acc);
  }
  double* stage = reinterpret_cast<double*>(tile);
  __syncthreads();                         // the tile has been read
#pragma unroll
  for (int u = 0; u < TT; ++u) stage[u * NT + tid] = acc[u];
  __syncthreads();
  for (int e = tid; e < nblk * TT; e += NT) {
    const int b = e >> 4, u = e & 15;
    const double* s = stage + u * NT + b * ksplit;
    double v = s[0];
    for (int x = 1; x < ksplit; ++x) v += s[x];
    int ei = 0, rem = b;
    while (rem >= nb - ei) { rem -= nb - ei; ++ei; }
    const int i = ei * T + (u >> 2), j = (ei + rem) * T + (u & 3);
    if (i < r && j < r) {
      if (REG && i == j) v += reg;
      M[i * LDM + j] = v;
      if (rem != 0) M[j * LDM + i] = v;    // a diagonal block holds both triangles itself (the same products in the same order)
    }
  }
}

// ---- reductions over the workgroup and the Jacobi solve -------------------------------------------------------------------------

// the sum of the 256 lane values by a fixed tree; every lane gets it
__device__ __forceinline__ double block_sum(double loc, double* red, int tid) {
  red[tid] = loc;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  const double v = red[0];
  __syncthreads();
  return v;
}

// max |M_ij| over i < j; a NaN stays once taken
__device__ __forceinline__ double block_offmax(const double* M, int n, double* red, int tid) {
  double loc = 0.0;
  for (int e = tid; e < n * n; e += NT) {
    const int i = e / n, j = e - i * n;
    if (i < j) {
      const double x = fabs(M[i * LDM + j]);
      if (x > loc || x != x) loc = x;
    }
  }
  red[tid] = loc;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const double x = red[tid + s], y = red[tid];
      red[tid] = (x > y || x != x) ? x : y;
    }
    __syncthreads();
  }
  const double v = red[0];
  __syncthreads();
  return v;
}

struct JacobiRot {                          // the rotations of a round: cosine, sine and the index pair (p < 0: nothing to rotate)
  double rc[MAT_N / 2], rs[MAT_N / 2];
  int rp[MAT_N / 2], rq[MAT_N / 2];
};

// M [n][LDM] symmetric -> diagonal (in place), V = the rotations' product (M0 = V diag V^T), by cyclic Jacobi: the round-robin
// ordering (n - 1 | 1 rounds of disjoint index pairs per sweep), the rotations of a round formed from one state of the matrix,
// applied to the columns of M and V, then to the rows of M.  Returns the sweeps used; conv = 1 when
// max_{i<j} |M_ij| <= 2^-52 ||M0||_F / n was met within `cap` sweeps.  At most cap * (n - 1 | 1) rounds: the kernel cannot spin.
// rot and red (256 doubles) are LDS scratch.
__device__ __forceinline__ int jacobi(double* M, double* V, int n, int cap, JacobiRot& rot, double* red, int& conv, int tid) {
  const int m = (n + 1) & ~1, half = m >> 1, mod = m - 1;
  double loc = 0.0;
  for (int e = tid; e < n * n; e += NT) {
    const int i = e / n, j = e - i * n;
    const double x = M[i * LDM + j];
    loc = loc + x * x;
    V[i * LDM + j] = i == j ? 1.0 : 0.0;
  }
  const double thr = 0x1p-52 * sqrt(block_sum(loc, red, tid)) / (double)n;
  int sweeps = 0;
  conv = 0;
  for (int s = 0; s <= cap; ++s) {
    const double off = block_offmax(M, n, red, tid);
    if (off <= thr) { conv = 1; break; }   // a NaN is never <=
    if (s == cap) break;
    for (int rd = 0; rd < mod; ++rd) {
      if (tid < half) {
        const int a = tid == 0 ? mod : (rd + tid) % mod, b = tid == 0 ? rd : (rd - tid + mod) % mod;
        int p = a < b ? a : b;
        const int q = a < b ? b : a;
        double c = 1.0, sn = 0.0;
        if (q < n) {
          const double apq = M[p * LDM + q];
          if (fabs(apq) > 0.0) {           // false for a NaN
            const double tau = (M[q * LDM + q] - M[p * LDM + p]) / (2.0 * apq);
            const double t = copysign(1.0, tau) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + t * t);
            sn = t * c;
          }
        } else {
          p = -1;                          // the padding index of an odd n: nothing to rotate
        }
        rot.rp[tid] = p; rot.rq[tid] = q; rot.rc[tid] = c; rot.rs[tid] = sn;
      }
      __syncthreads();
      for (int e = tid; e < half * n; e += NT) {          // M <- M J, V <- V J
        const int k = e / n, i = e - k * n, p = rot.rp[k], q = rot.rq[k];
        if (p < 0) continue;
        const double c = rot.rc[k], sn = rot.rs[k];
        const double x = M[i * LDM + p], y = M[i * LDM + q];
        M[i * LDM + p] = c * x - sn * y;
        M[i * LDM + q] = sn * x + c * y;
        const double vx = V[i * LDM + p], vy = V[i * LDM + q];
        V[i * LDM + p] = c * vx - sn * vy;
        V[i * LDM + q] = sn * vx + c * vy;
      }
      __syncthreads();
      for (int e = tid; e < half * n; e += NT) {          // M <- J^T M; the rotated element itself is set to 0
        const int k = e / n, j = e - k * n, p = rot.rp[k], q = rot.rq[k];
        if (p < 0) continue;
        const double c = rot.rc[k], sn = rot.rs[k];
        const double x = M[p * LDM + j], y = M[q * LDM + j];
        M[p * LDM + j] = j == q ? 0.0 : c * x - sn * y;
        M[q * LDM + j] = j == p ? 0.0 : sn * x + c * y;
      }
      __syncthreads();
    }
    ++sweeps;
  }
  return sweeps;
}

}  // namespace
