// qfx_lora_svd.hip -- the singular value decomposition of every adapter pair dW = B A over the flat LoRA buffer, without ever forming
// the [out, in] product: the spectrum (qfx_lora_spectrum) and the re-expression of a pair at a lower rank (qfx_lora_project, kohya's
// resize_lora.py).  The listing in include/qfx.h is the specification.  ONE launch of one 256-lane workgroup per pair, driven by a
// device table, laid out like qfx_scaled_adamw.hip:
//   1. G_A = A A^T and G_B = B^T B in fp64 from the fp32 weights (every product exact): the upper triangle in 4 x 4 blocks, a lane
//      owns one block and one residue class of the summed index, A / B stream through one LDS tile stored k-major with an odd row
//      stride; the classes are folded through LDS in class order into the two full matrices (the Gram sweep of qfx_maxnorm.hip /
//      qfx_scaled_adamw.hip, restated here: those files keep their own copy so that what they compile to does not move)
//   2. G_A = V L V^T by cyclic Jacobi in LDS: the round-robin ordering (r - 1 rounds of r / 2 disjoint index pairs per sweep), the
//      rotations of a round formed from one state of the matrix, applied to the columns of M and V, then to the rows of M
//   3. K = L^1/2 V^T G_B, H = K V L^1/2 symmetrised, H = W Th W^T by the same solve, Th sorted
//   4. sv, the numeric rank, and (with a workspace) T_B = V L^1/2 W and T_A = Th^-1 W^T K
// LDS: the 65 KB tile doubles as two [64][65] fp64 matrices once the Gram sweeps are over (V and K), G_A / G_B are overwritten by
// their diagonalised forms, H and W: 130 KB + 4 KB of small arrays, one workgroup per CU.
// Every loop has a trip count fixed by r and the sweep cap; a solve leaves early only when its off-diagonal criterion is met, a
// NaN never meets it and runs to the cap.  One fp64 rounding per operation (no FMA contraction).  Nothing crosses a workgroup but
// the integer skip counter: same inputs -> same bits at any address.
#include "qfx_common.h"

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                     // four waves
constexpr int RMAX = 64;                    // largest rank
constexpr int DIM_MAX = 1 << 24;            // largest in_features / out_features
constexpr int LDM = RMAX + 1;               // row stride of the fp64 matrices in LDS
constexpr int MSZ = RMAX * LDM;             // one such matrix
constexpr int TILE_F = 4 * MSZ;             // 65 KB of floats: the A / B tile of the Gram sweeps, the staging area of the fold
                                            // (16 x 256 fp64), then two fp64 matrices
constexpr int T = 4, TT = T * T;            // block of the Gram matrices' upper triangle a lane owns
constexpr int WS_LD = 64;                   // row stride of T_B / T_A in the workspace
constexpr int WS_PAIR = 2 * 64 * 64;        // doubles per pair

struct Small {                              // the small LDS arrays of a workgroup
  double red[NT];
  double lamh[RMAX];                        // L^1/2
  double theta[RMAX];                       // Th, unsorted
  double ths[RMAX];                         // Th, sorted descending
  double rc[RMAX / 2], rs[RMAX / 2];        // the rotations of a round
  int rp[RMAX / 2], rq[RMAX / 2];
  int perm[RMAX];                           // perm[rank] = index into theta
  int rho;
};

// (qfx_maxnorm.hip's fill_a) element (i, k) of the r x kt slice that starts at column k0 of A [r, ld] -> tile[k * S + i]
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

// (qfx_maxnorm.hip's fill_b) element (i, k) of the kt rows that start at row k0 of B [out, r] -> tile[k * S + i]
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
__device__ __forceinline__ void gram_tile(const float* tile, int S, int kt, int i0, int j0, int ks, int ksplit, double (&acc)[TT]) {
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
// summed over its rows.  (qfx_scaled_adamw.hip's gram without its reg.)
__device__ __forceinline__ void gram(const float* __restrict__ X, bool is_a, int r, int n, float* tile, double* M, int tid) {
  const int nb = (r + T - 1) / T, nblk = nb * (nb + 1) / 2, ksplit = NT / nblk;
  const int rp = nb * T, S = rp + 1, KT = (TILE_F / S) & ~3;          // S odd; KT >= 256 rows of the tile, a multiple of 4
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
    if (active) gram_tile(tile, S, kt, bi * T, bj * T, ks, ksplit, acc);
  }
  // per block and element the partial sums of the residue classes in class order
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
      M[i * LDM + j] = v;
      if (rem != 0) M[j * LDM + i] = v;    // a diagonal block holds both triangles itself (the same products in the same order)
    }
  }
  __syncthreads();                         // M is complete, the stage has been read
}

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

// M [n][LDM] symmetric -> diagonal (in place), V = the rotations' product (M0 = V diag V^T).  Returns the sweeps used; conv = 1 when
// max_{i<j} |M_ij| <= 2^-52 ||M0||_F / n was met within `cap` sweeps.  At most cap * (n - 1 | 1) rounds: the kernel cannot spin.
__device__ __forceinline__ int jacobi(double* M, double* V, int n, int cap, Small& sm, int& conv, int tid) {
  const int m = (n + 1) & ~1, half = m >> 1, mod = m - 1;
  double loc = 0.0;
  for (int e = tid; e < n * n; e += NT) {
    const int i = e / n, j = e - i * n;
    const double x = M[i * LDM + j];
    loc = loc + x * x;
    V[i * LDM + j] = i == j ? 1.0 : 0.0;
  }
  const double thr = 0x1p-52 * sqrt(block_sum(loc, sm.red, tid)) / (double)n;
  int sweeps = 0;
  conv = 0;
  for (int s = 0; s <= cap; ++s) {
    const double off = block_offmax(M, n, sm.red, tid);
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
        sm.rp[tid] = p; sm.rq[tid] = q; sm.rc[tid] = c; sm.rs[tid] = sn;
      }
      __syncthreads();
      for (int e = tid; e < half * n; e += NT) {          // M <- M J, V <- V J
        const int k = e / n, i = e - k * n, p = sm.rp[k], q = sm.rq[k];
        if (p < 0) continue;
        const double c = sm.rc[k], sn = sm.rs[k];
        const double x = M[i * LDM + p], y = M[i * LDM + q];
        M[i * LDM + p] = c * x - sn * y;
        M[i * LDM + q] = sn * x + c * y;
        const double vx = V[i * LDM + p], vy = V[i * LDM + q];
        V[i * LDM + p] = c * vx - sn * vy;
        V[i * LDM + q] = sn * vx + c * vy;
      }
      __syncthreads();
      for (int e = tid; e < half * n; e += NT) {          // M <- J^T M; the rotated element itself is set to 0
        const int k = e / n, j = e - k * n, p = sm.rp[k], q = sm.rq[k];
        if (p < 0) continue;
        const double c = sm.rc[k], sn = sm.rs[k];
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

__device__ __forceinline__ void write_empty(const qfx_lora_spectrum_args& a, int pi, int tid) {
  for (int64_t i = tid; i < a.ld_sv; i += NT) a.sv[(int64_t)pi * a.ld_sv + i] = 0.0;
  if (tid < 4) a.info[4 * pi + tid] = 0;
  if (a.ws)
    for (int e = tid; e < WS_PAIR; e += NT) a.ws[(int64_t)pi * WS_PAIR + e] = 0.0;
}

__global__ __launch_bounds__(NT) void lora_spectrum_kernel(const qfx_lora_spectrum_args a) {
  __shared__ __attribute__((aligned(16))) float tile[TILE_F];
  __shared__ double MA[MSZ];               // G_A, its diagonal form, then H and its diagonal form
  __shared__ double MB[MSZ];               // G_B, then W
  __shared__ Small sm;
  const int tid = threadIdx.x, pi = blockIdx.x;
  const qfx_lora_svd_pair t = a.table[pi];
  // what qfx_lora_svd_check_table refuses is never touched
  if (t.r < 1 || t.r > RMAX || t.in_features < 1 || t.in_features > DIM_MAX || t.out_features < 1 || t.out_features > DIM_MAX ||
      t.off_a < 0 || t.off_b < 0) {
    write_empty(a, pi, tid);
    return;
  }
  const int r = t.r;
  gram(a.p + t.off_a, true, r, t.in_features, tile, MA, tid);
  gram(a.p + t.off_b, false, r, t.out_features, tile, MB, tid);
  int bad = 0;
  for (int e = tid; e < r * r; e += NT) {
    const int i = e / r, j = e - i * r;
    bad |= !__builtin_isfinite(MA[i * LDM + j]) || !__builtin_isfinite(MB[i * LDM + j]);
  }
  if (__syncthreads_or(bad)) {             // the same verdict on every lane
    write_empty(a, pi, tid);
    if (tid == 0) atomicAdd(a.skipped, 1);
    return;
  }
  double* V = reinterpret_cast<double*>(tile);
  double* K = V + MSZ;
  double* W = MB;
  int conv_a = 0, conv_h = 0;
  const int sweeps_a = jacobi(MA, V, r, a.max_sweeps, sm, conv_a, tid);
  if (tid < r) {
    const double d = MA[tid * LDM + tid];
    sm.lamh[tid] = d > 0.0 ? sqrt(d) : 0.0;
  }
  __syncthreads();
  for (int e = tid; e < r * r; e += NT) {                 // K = L^1/2 V^T G_B
    const int i = e / r, j = e - i * r;
    double acc = 0.0;
    for (int k = 0; k < r; ++k) acc = acc + V[k * LDM + i] * MB[k * LDM + j];
    K[i * LDM + j] = sm.lamh[i] * acc;
  }
  __syncthreads();
  for (int e = tid; e < r * r; e += NT) {                 // H = K V L^1/2
    const int i = e / r, j = e - i * r;
    double acc = 0.0;
    for (int k = 0; k < r; ++k) acc = acc + K[i * LDM + k] * V[k * LDM + j];
    MA[i * LDM + j] = acc * sm.lamh[j];
  }
  __syncthreads();
  for (int e = tid; e < r * r; e += NT) {
    const int i = e / r, j = e - i * r;
    if (i < j) {
      const double h = 0.5 * (MA[i * LDM + j] + MA[j * LDM + i]);
      MA[i * LDM + j] = h;
      MA[j * LDM + i] = h;
    }
  }
  __syncthreads();
  const int sweeps_h = jacobi(MA, W, r, a.max_sweeps, sm, conv_h, tid);
  if (tid < r) {
    const double d = MA[tid * LDM + tid];
    sm.theta[tid] = d > 0.0 ? d : 0.0;
  }
  __syncthreads();
  if (tid < r) {                                          // descending, ties by index
    const double me = sm.theta[tid];
    int rank = 0;
    for (int j = 0; j < r; ++j) {
      const double o = sm.theta[j];
      rank += (o > me) || (o == me && j < tid);
    }
    sm.perm[rank] = tid;
    sm.ths[rank] = me;
  }
  __syncthreads();
  if (tid == 0) {
    const double s0 = sqrt(sm.ths[0]);
    int rho = 0;
    if (s0 > 0.0)
      for (int i = 0; i < r; ++i) rho += sqrt(sm.ths[i]) > a.rank_tol * s0;
    sm.rho = rho;
    a.info[4 * pi + 0] = rho;
    a.info[4 * pi + 1] = sweeps_a;
    a.info[4 * pi + 2] = sweeps_h;
    a.info[4 * pi + 3] = conv_a & conv_h;
  }
  for (int64_t i = tid; i < a.ld_sv; i += NT) a.sv[(int64_t)pi * a.ld_sv + i] = i < r ? sqrt(sm.ths[i]) : 0.0;
  if (!a.ws) return;
  __syncthreads();
  const int rho = sm.rho;
  double* TB = a.ws + (int64_t)pi * WS_PAIR;
  double* TA = TB + 64 * 64;
  for (int e = tid; e < 64 * 64; e += NT) {
    const int i = e >> 6, j = e & 63;
    double tb = 0.0, ta = 0.0;
    if (i < r && j < rho) {                               // T_B = V L^1/2 W, its columns in the sorted order
      const int pj = sm.perm[j];
      for (int k = 0; k < r; ++k) tb = tb + (V[i * LDM + k] * sm.lamh[k]) * W[k * LDM + pj];
    }
    if (i < rho && j < r) {                               // T_A = Th^-1 W^T K
      const int pi_ = sm.perm[i];
      for (int k = 0; k < r; ++k) ta = ta + W[k * LDM + pi_] * K[k * LDM + j];
      ta = ta / sm.ths[i];
    }
    TB[i * WS_LD + j] = tb;
    TA[i * WS_LD + j] = ta;
  }
}

__global__ __launch_bounds__(NT) void lora_project_kernel(const qfx_lora_project_args a) {
  __shared__ double TB[64 * 64];
  __shared__ double TA[64 * 64];
  const int tid = threadIdx.x, pi = blockIdx.x;
  const qfx_lora_svd_pair t = a.table[pi];
  const qfx_lora_svd_dst d = a.dst[pi];
  // what the two check functions refuse is never touched
  if (t.r < 1 || t.r > RMAX || t.in_features < 1 || t.in_features > DIM_MAX || t.out_features < 1 || t.out_features > DIM_MAX ||
      t.off_a < 0 || t.off_b < 0 || d.k < 1 || d.k > t.r || d.r_dst < d.k || d.r_dst > RMAX || d.dst_off_a < 0 || d.dst_off_b < 0)
    return;
  const int r = t.r, nin = t.in_features, nout = t.out_features, k = d.k, rd = d.r_dst;
  const double* ws = a.ws + (int64_t)pi * WS_PAIR;
  for (int e = tid; e < 64 * 64; e += NT) {
    TB[e] = ws[e];
    TA[e] = ws[64 * 64 + e];
  }
  __syncthreads();
  const float* __restrict__ A = a.p + t.off_a;
  const float* __restrict__ B = a.p + t.off_b;
  float* A2 = a.q + d.dst_off_a;
  float* B2 = a.q + d.dst_off_b;

  // B'[o][j] = fp32(sum_i B[o][i] T_B[i][j]), j < k; +0.0 for k <= j < r_dst
  if ((((uintptr_t)B2 & 15) == 0) && (rd & 3) == 0) {
    const int jq_n = rd >> 2;
    for (int64_t e = tid; e < (int64_t)nout * jq_n; e += NT) {
      const int64_t o = e / jq_n;
      const int j0 = 4 * (int)(e - o * jq_n);
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      if (j0 < k)
        for (int i = 0; i < r; ++i) {
          const double b = (double)B[o * r + i];
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[c] = acc[c] + b * TB[i * 64 + j0 + c];
        }
      f32x4 v;
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = j0 + c < k ? (float)acc[c] : 0.f;
      *reinterpret_cast<f32x4*>(B2 + o * rd + j0) = v;
    }
  } else {
    for (int64_t e = tid; e < (int64_t)nout * rd; e += NT) {
      const int64_t o = e / rd;
      const int j = (int)(e - o * rd);
      double acc = 0.0;
      if (j < k)
        for (int i = 0; i < r; ++i) acc = acc + (double)B[o * r + i] * TB[i * 64 + j];
      B2[e] = j < k ? (float)acc : 0.f;
    }
  }

  // A'[j][c] = fp32(sum_i T_A[j][i] A[i][c]), j < k; +0.0 for k <= j < r_dst
  if ((((uintptr_t)A & 15) == 0) && (((uintptr_t)A2 & 15) == 0) && (nin & 3) == 0) {
    const int cq_n = nin >> 2;
    for (int64_t e = tid; e < (int64_t)rd * cq_n; e += NT) {
      const int j = (int)(e / cq_n);
      const int64_t c0 = 4 * (e - (int64_t)j * cq_n);
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      if (j < k)
        for (int i = 0; i < r; ++i) {
          const double tji = TA[j * 64 + i];
          const f32x4 x = *reinterpret_cast<const f32x4*>(A + (int64_t)i * nin + c0);
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[c] = acc[c] + tji * (double)x[c];
        }
      f32x4 v;
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = j < k ? (float)acc[c] : 0.f;
      *reinterpret_cast<f32x4*>(A2 + (int64_t)j * nin + c0) = v;
    }
  } else {
    for (int64_t e = tid; e < (int64_t)rd * nin; e += NT) {
      const int j = (int)(e / nin);
      const int64_t c = e - (int64_t)j * nin;
      double acc = 0.0;
      if (j < k)
        for (int i = 0; i < r; ++i) acc = acc + TA[j * 64 + i] * (double)A[(int64_t)i * nin + c];
      A2[e] = j < k ? (float)acc : 0.f;
    }
  }
}

inline bool dims_ok(const qfx_lora_svd_pair& t) {
  return t.r >= 1 && t.r <= RMAX && t.in_features >= 1 && t.in_features <= DIM_MAX && t.out_features >= 1 && t.out_features <= DIM_MAX;
}

// the half-open spans inside [0, n_elems) and disjoint
inline int spans_ok(std::vector<std::pair<int64_t, int64_t>>& spans) {
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i)
    if (spans[i].first < spans[i - 1].second) return 0;   // two matrices overlap (of one pair or of two)
  return 1;
}

inline bool span_in(int64_t off, int64_t n, int64_t n_elems) { return off >= 0 && n <= n_elems && off <= n_elems - n; }

}  // namespace

extern "C" int qfx_lora_svd_check_table(const qfx_lora_svd_pair* host_table, int32_t n_pairs, int64_t n_elems) {
  if (n_pairs < 0 || n_elems < 0 || (n_pairs > 0 && !host_table)) return QFX_EINVAL;
  std::vector<std::pair<int64_t, int64_t>> spans;
  spans.reserve(2 * (size_t)n_pairs);
  for (int32_t i = 0; i < n_pairs; ++i) {
    const qfx_lora_svd_pair& t = host_table[i];
    if (!dims_ok(t)) return QFX_EINVAL;
    const int64_t na = (int64_t)t.r * t.in_features, nb = (int64_t)t.out_features * t.r;
    if (!span_in(t.off_a, na, n_elems) || !span_in(t.off_b, nb, n_elems)) return QFX_EINVAL;
    spans.emplace_back(t.off_a, t.off_a + na);
    spans.emplace_back(t.off_b, t.off_b + nb);
  }
  return spans_ok(spans) ? QFX_OK : QFX_EINVAL;
}

extern "C" int qfx_lora_project_check_table(const qfx_lora_svd_pair* host_table, const qfx_lora_svd_dst* host_dst, int32_t n_pairs,
                                            int64_t n_elems_dst) {
  if (n_pairs < 0 || n_elems_dst < 0 || (n_pairs > 0 && (!host_table || !host_dst))) return QFX_EINVAL;
  std::vector<std::pair<int64_t, int64_t>> spans;
  spans.reserve(2 * (size_t)n_pairs);
  for (int32_t i = 0; i < n_pairs; ++i) {
    const qfx_lora_svd_pair& t = host_table[i];
    const qfx_lora_svd_dst& d = host_dst[i];
    if (!dims_ok(t)) return QFX_EINVAL;
    if (d.k < 1 || d.k > t.r || d.r_dst < d.k || d.r_dst > RMAX) return QFX_EINVAL;
    const int64_t na = (int64_t)d.r_dst * t.in_features, nb = (int64_t)t.out_features * d.r_dst;
    if (!span_in(d.dst_off_a, na, n_elems_dst) || !span_in(d.dst_off_b, nb, n_elems_dst)) return QFX_EINVAL;
    spans.emplace_back(d.dst_off_a, d.dst_off_a + na);
    spans.emplace_back(d.dst_off_b, d.dst_off_b + nb);
  }
  return spans_ok(spans) ? QFX_OK : QFX_EINVAL;
}

extern "C" int qfx_lora_spectrum(const qfx_lora_spectrum_args* a, void* stream) {
  if (!a || a->n_pairs < 0) return QFX_EINVAL;
  if (!(a->rank_tol > 0.0 && a->rank_tol < 1.0)) return QFX_EINVAL;                  // a NaN fails
  if (a->max_sweeps < 1 || a->max_sweeps > 64 || a->ld_sv < 64) return QFX_EINVAL;
  if (a->n_pairs == 0) return QFX_OK;
  if (!a->p || !a->table || !a->sv || !a->info || !a->skipped) return QFX_EINVAL;    // ws may be NULL: the spectrum only
  if (hipMemsetAsync(a->skipped, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return QFX_EINVAL;
  hipLaunchKernelGGL(lora_spectrum_kernel, dim3((unsigned)a->n_pairs), dim3(NT), 0, (hipStream_t)stream, *a);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_lora_project(const qfx_lora_project_args* a, void* stream) {
  if (!a || a->n_pairs < 0) return QFX_EINVAL;
  if (a->q && (const float*)a->q == a->p) return QFX_EINVAL;                         // never in place: B' and A' are read from B and A
  if (a->n_pairs == 0) return QFX_OK;
  if (!a->p || !a->q || !a->table || !a->dst || !a->ws) return QFX_EINVAL;
  hipLaunchKernelGGL(lora_project_kernel, dim3((unsigned)a->n_pairs), dim3(NT), 0, (hipStream_t)stream, *a);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
