// qfx_lora_svd.hip -- the singular value decomposition of every adapter pair dW = B A over the flat LoRA buffer, without ever forming
// the [out, in] product: the spectrum (qfx_lora_spectrum) and the re-expression of a pair at a lower rank (qfx_lora_project, kohya's
// resize_lora.py).  The listing in include/qfx.h is the specification.  ONE launch of one 256-lane workgroup per pair, driven by a
// device table, laid out like qfx_scaled_adamw.hip:
//   1. G_A = A A^T and G_B = B^T B in fp64 from the fp32 weights (every product exact): the upper triangle in 4 x 4 blocks, a lane
//      owns one block and one residue class of the summed index, A / B stream through one LDS tile stored k-major with an odd row
//      stride; the classes are folded through LDS in class order into the two full matrices (gram of qfx_pair_linalg.h, as in
//      qfx_scaled_adamw.hip)
//   2. G_A = V L V^T by cyclic Jacobi in LDS (jacobi of qfx_pair_linalg.h): the round-robin ordering (r - 1 rounds of r / 2
//      disjoint index pairs per sweep), the rotations of a round formed from one state of the matrix, applied to the columns of
//      M and V, then to the rows of M
//   3. K = L^1/2 V^T G_B, H = K V L^1/2 symmetrised, H = W Th W^T by the same solve, Th sorted
//   4. sv, the numeric rank, and (with a workspace) T_B = V L^1/2 W and T_A = Th^-1 W^T K
// LDS: the 65 KB tile doubles as two [64][65] fp64 matrices once the Gram sweeps are over (V and K), G_A / G_B are overwritten by
// their diagonalised forms, H and W: 130 KB + 4 KB of small arrays, one workgroup per CU.
// Every loop has a trip count fixed by r and the sweep cap; a solve leaves early only when its off-diagonal criterion is met, a
// NaN never meets it and runs to the cap.  One fp64 rounding per operation (no FMA contraction).  Nothing crosses a workgroup but
// the integer skip counter: same inputs -> same bits at any address.
#include "qfx_common.h"

#include <cmath>

#pragma clang fp contract(off)

#include "qfx_pair_linalg.h"                // the Gram sweep, the Jacobi solve and the table check

namespace {

constexpr int RMAX = MAT_N;                 // largest rank
constexpr int MSZ = RMAX * LDM;             // one fp64 matrix in LDS
constexpr int TILE_F = 4 * MSZ;             // 65 KB of floats: the A / B tile of the Gram sweeps, the staging area of the fold
                                            // (16 x 256 fp64), then two fp64 matrices
constexpr int WS_LD = 64;                   // row stride of T_B / T_A in the workspace
constexpr int WS_PAIR = 2 * 64 * 64;        // doubles per pair

struct Small {                              // the small LDS arrays of a workgroup
  double red[NT];
  double lamh[RMAX];                        // L^1/2
  double theta[RMAX];                       // Th, unsorted
  double ths[RMAX];                         // Th, sorted descending
  JacobiRot rot;
  int perm[RMAX];                           // perm[rank] = index into theta
  int rho;
};

// the ranks of a destination row that qfx_lora_project_check_table refuses: not 1 <= k <= r, k <= r_dst <= RMAX (a macro for
// the reason QFX_PAIR_REFUSED is one)
#define QFX_DST_REFUSED(d, r) ((d).k < 1 || (d).k > (r) || (d).r_dst < (d).k || (d).r_dst > RMAX)

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
  if (QFX_PAIR_REFUSED(t, RMAX)) {         // what qfx_lora_svd_check_table refuses is never touched
    write_empty(a, pi, tid);
    return;
  }
  const int r = t.r;
  gram<TILE_F>(a.p + t.off_a, true, r, t.in_features, tile, MA, tid);
  __syncthreads();                         // MA is complete, the stage has been read
  gram<TILE_F>(a.p + t.off_b, false, r, t.out_features, tile, MB, tid);
  __syncthreads();
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
  const int sweeps_a = jacobi(MA, V, r, a.max_sweeps, sm.rot, sm.red, conv_a, tid);
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
  const int sweeps_h = jacobi(MA, W, r, a.max_sweeps, sm.rot, sm.red, conv_h, tid);
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
  if (QFX_PAIR_REFUSED(t, RMAX) || QFX_DST_REFUSED(d, t.r) || d.dst_off_a < 0 || d.dst_off_b < 0) return;
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

}  // namespace

extern "C" int qfx_lora_svd_check_table(const qfx_lora_svd_pair* host_table, int32_t n_pairs, int64_t n_elems) {
  return check_pair_table(n_pairs, n_elems, host_table != nullptr, RMAX, [&](int32_t i, PairDims& d) {
    d = pair_dims(host_table[i]);
    return true;
  });
}

// the spans are those of A' [r_dst, in] and B' [out, r_dst] in the destination buffer
extern "C" int qfx_lora_project_check_table(const qfx_lora_svd_pair* host_table, const qfx_lora_svd_dst* host_dst, int32_t n_pairs,
                                            int64_t n_elems_dst) {
  return check_pair_table(n_pairs, n_elems_dst, host_table && host_dst, RMAX, [&](int32_t i, PairDims& d) {
    const qfx_lora_svd_pair& t = host_table[i];
    const qfx_lora_svd_dst& dst = host_dst[i];
    d = {dst.dst_off_a, dst.dst_off_b, dst.r_dst, t.in_features, t.out_features};
    // of the source row only its rank is left to test here (its in / out features are d's); its offsets are not this check's
    return !(t.r < 1 || t.r > RMAX || QFX_DST_REFUSED(dst, t.r));
  });
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
