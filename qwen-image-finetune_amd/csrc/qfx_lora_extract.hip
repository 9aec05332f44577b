// qfx_lora_extract.hip -- a rank-k factorisation D ~ Q C of every dense difference D = W1 - W0 of a device table by a randomized
// range finder with power iterations (kohya's extract_lora_from_models.py without its full SVD).  The listing in include/qfx.h
// is the specification.  A fixed sequence of launches over (matrix, chunk of 64 rows or columns), all on one stream:
//   init      the per-matrix workspace offsets (a prefix sum over the table) and the per-matrix state words
//   omega     the +-1 test matrix from Philox4x32-10 into Z [in, k]
//   product   Y = D X (a block owns 64 rows of D) or Z = D^T X (a block owns 64 columns): 64 x 64 tiles of D, formed as
//             fp32(W1) - fp32(W0) on the way into LDS, times a 64 x k tile of X, fp32 FMA in ascending order of the summed index,
//             a 4 x 4 register block per lane; the epilogue writes the chunk and its k x k fp64 Gram partial
//   solve     one workgroup per matrix: the partials folded in chunk order, the cyclic Jacobi solve that qfx_lora_svd.hip uses
//             (jacobi of qfx_pair_linalg.h), T = V L^-1/2 with the kept columns first
//   apply     Y <- fp32(Y T), fp64 sums in index order, in place (the last one writes Q to its place in the flat buffer)
// Nothing crosses a workgroup but through the ordered partials and the integer skip counter: same inputs -> same bits.
#include "qfx_common.h"

#pragma clang fp contract(off)

#include "qfx_pair_linalg.h"                // the Jacobi solve, block_sum and the table check

namespace {

constexpr int KMAX = MAT_N;                 // widest sketch
constexpr int TS = 64;                      // rows of a row chunk = columns of a column chunk = the tile edge
constexpr int LDD = TS + 4;                 // row stride of the fp32 tiles in LDS (16-byte rows)
constexpr int MSZ = KMAX * LDM;             // one fp64 matrix of the solve
constexpr int MAX_MATS = 65535;             // grid.y
constexpr uint32_t OMEGA_TAG = 0x4C524B58u; // counter word 2 of the test matrix ("LRKX")

// Philox4x32-10 (Salmon et al., Random123), as qfx_lora_dropout.hip states it
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__host__ __device__ inline int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }
__host__ __device__ inline int chunks_of(int n) { return (n + TS - 1) / TS; }

// the workspace: [offset of each matrix: int64 x n][state of each matrix: int32 x 4 x n] then, per matrix, 256-byte aligned:
//   T [64][64] fp64 | Gram partials [max chunks][k * k] fp64 | normsq partials [row chunks] fp64 | flags [row chunks] int32 |
//   Y [out, k] fp32 | Z [in, k] fp32
__host__ __device__ inline int64_t header_bytes(int n) { return round_up((int64_t)n * 24, 256); }
__host__ __device__ inline int64_t mat_bytes(int k, int nin, int nout) {
  const int64_t cm = chunks_of(nin) > chunks_of(nout) ? chunks_of(nin) : chunks_of(nout);
  return round_up(64 * 64 * 8 + cm * k * k * 8 + (int64_t)chunks_of(nout) * 8 + round_up((int64_t)chunks_of(nout) * 4, 8) +
                  round_up((int64_t)nout * k * 4, 16) + round_up((int64_t)nin * k * 4, 16), 256);
}

struct MatWs { double* T; double* part; double* nsq; int* flag; float* Y; float* Z; };

__device__ __forceinline__ MatWs mat_ws(const qfx_lowrank_args& a, int m, const qfx_lowrank_mat& t) {
  char* b = reinterpret_cast<char*>(a.ws) + reinterpret_cast<const int64_t*>(a.ws)[m];
  const int64_t cm = chunks_of(t.in_features) > chunks_of(t.out_features) ? chunks_of(t.in_features) : chunks_of(t.out_features);
  const int64_t co = chunks_of(t.out_features);
  MatWs w;
  w.T = reinterpret_cast<double*>(b);                 b += 64 * 64 * 8;
  w.part = reinterpret_cast<double*>(b);              b += cm * t.k * t.k * 8;
  w.nsq = reinterpret_cast<double*>(b);               b += co * 8;
  w.flag = reinterpret_cast<int*>(b);                 b += round_up(co * 4, 8);
  w.Y = reinterpret_cast<float*>(b);                  b += round_up((int64_t)t.out_features * t.k * 4, 16);
  w.Z = reinterpret_cast<float*>(b);
  return w;
}

// state words of matrix m: { bad, kept, converged, - }
__device__ __forceinline__ int* mat_state(const qfx_lowrank_args& a, int m) {
  return reinterpret_cast<int*>(reinterpret_cast<char*>(a.ws) + (int64_t)a.n_mats * 8) + 4 * m;
}

__host__ __device__ inline bool dims_ok(const qfx_lowrank_mat& t) {
  return t.k >= 1 && t.k <= KMAX && t.in_features >= 1 && t.in_features <= DIM_MAX && t.out_features >= 1 && t.out_features <= DIM_MAX &&
         (t.dtype == 0 || t.dtype == 1) && t.w1 != nullptr && t.ld1 >= t.in_features && (t.w0 == nullptr || t.ld0 >= t.in_features) &&
         t.off_a >= 0 && t.off_b >= 0;
}

// 16-byte loads of W1 / W0: both 16-byte aligned, the leading dimensions whole 16-byte groups
__device__ __forceinline__ bool d_vec(const qfx_lowrank_mat& t) {
  const int64_t g = t.dtype == 0 ? 8 : 4;
  return (((uintptr_t)t.w1 & 15) == 0) && (t.ld1 % g) == 0 && (t.w0 == nullptr || ((((uintptr_t)t.w0 & 15) == 0) && (t.ld0 % g) == 0));
}

__global__ void lowrank_init_kernel(const qfx_lowrank_args a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t* off = reinterpret_cast<int64_t*>(a.ws);
  int64_t at = header_bytes(a.n_mats);
  for (int m = 0; m < a.n_mats; ++m) {
    const qfx_lowrank_mat t = a.table[m];
    off[m] = at;
    if (dims_ok(t)) at += mat_bytes(t.k, t.in_features, t.out_features);
    int* st = mat_state(a, m);
    st[0] = 0; st[1] = 0; st[2] = 0; st[3] = 0;
  }
}

// Omega [in, k] into Z: +1 where bit j & 31 of word j >> 5 of Philox(key = seed, counter = (i, index, tag, 0)) is clear
__global__ __launch_bounds__(NT) void lowrank_omega_kernel(const qfx_lowrank_args a) {
  const int m = blockIdx.y, tid = threadIdx.x;
  const qfx_lowrank_mat t = a.table[m];
  if (!dims_ok(t)) return;
  const int64_t i = (int64_t)blockIdx.x * TS + (tid >> 2);
  if (i >= t.in_features) return;
  const MatWs w = mat_ws(a, m, t);
  uint32_t o[4];
  philox4x32_10((uint32_t)i, (uint32_t)t.index, OMEGA_TAG, 0u, a.seed_lo, a.seed_hi, o);
  const int j0 = (tid & 3) * 16;
#pragma unroll
  for (int jj = 0; jj < 16; ++jj) {
    const int j = j0 + jj;
    if (j < t.k) w.Z[i * t.k + j] = ((o[j >> 5] >> (j & 31)) & 1u) ? -1.f : 1.f;
  }
}

// Dl[r][c] = D[row0 + r][col0 + c] for r, c < 64, +0 outside the matrix.  STATS: the lane's sum of squares and finiteness.
template <bool STATS>
__device__ __forceinline__ void load_d(const qfx_lowrank_mat& t, bool vec, int64_t row0, int64_t col0, float* Dl, int tid, double& nsq, int& bad) {
  const int nr = (int)(t.out_features - row0 < TS ? t.out_features - row0 : TS);
  const int nc = (int)(t.in_features - col0 < TS ? t.in_features - col0 : TS);
  if (t.dtype == 0) {
    const bf16_t* __restrict__ w1 = reinterpret_cast<const bf16_t*>(t.w1);
    const bf16_t* __restrict__ w0 = reinterpret_cast<const bf16_t*>(t.w0);
#pragma unroll
    for (int g = tid; g < TS * 8; g += NT) {
      const int r = g >> 3, c = (g & 7) * 8;
      float v[8];
      if (r < nr && vec && c + 8 <= nc) {
        const u32x4 x = *reinterpret_cast<const u32x4*>(w1 + (row0 + r) * t.ld1 + col0 + c);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[2 * i] = __uint_as_float(x[i] << 16);
          v[2 * i + 1] = __uint_as_float(x[i] & 0xFFFF0000u);
        }
        if (w0) {
          const u32x4 y = *reinterpret_cast<const u32x4*>(w0 + (row0 + r) * t.ld0 + col0 + c);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            v[2 * i] = v[2 * i] - __uint_as_float(y[i] << 16);
            v[2 * i + 1] = v[2 * i + 1] - __uint_as_float(y[i] & 0xFFFF0000u);
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float d = 0.f;
          if (r < nr && c + j < nc) {
            d = bf2f(w1[(row0 + r) * t.ld1 + col0 + c + j]);
            if (w0) d = d - bf2f(w0[(row0 + r) * t.ld0 + col0 + c + j]);
          }
          v[j] = d;
        }
      }
      *reinterpret_cast<f32x4*>(Dl + r * LDD + c) = (f32x4){v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(Dl + r * LDD + c + 4) = (f32x4){v[4], v[5], v[6], v[7]};
      if (STATS) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          bad |= !__builtin_isfinite(v[j]);
          nsq = __builtin_fma((double)v[j], (double)v[j], nsq);
        }
      }
    }
  } else {
    const float* __restrict__ w1 = reinterpret_cast<const float*>(t.w1);
    const float* __restrict__ w0 = reinterpret_cast<const float*>(t.w0);
#pragma unroll
    for (int g = tid; g < TS * 16; g += NT) {
      const int r = g >> 4, c = (g & 15) * 4;
      f32x4 v;
      if (r < nr && vec && c + 4 <= nc) {
        v = *reinterpret_cast<const f32x4*>(w1 + (row0 + r) * t.ld1 + col0 + c);
        if (w0) {
          const f32x4 y = *reinterpret_cast<const f32x4*>(w0 + (row0 + r) * t.ld0 + col0 + c);
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = v[j] - y[j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float d = 0.f;
          if (r < nr && c + j < nc) {
            d = w1[(row0 + r) * t.ld1 + col0 + c + j];
            if (w0) d = d - w0[(row0 + r) * t.ld0 + col0 + c + j];
          }
          v[j] = d;
        }
      }
      *reinterpret_cast<f32x4*>(Dl + r * LDD + c) = v;
      if (STATS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bad |= !__builtin_isfinite(v[j]);
          nsq = __builtin_fma((double)v[j], (double)v[j], nsq);
        }
      }
    }
  }
}

// Xl[r][c] = X[row0 + r][c] for r < 64, c < 64 (X [n, k], contiguous rows), +0 for r >= nr or c >= k
__device__ __forceinline__ void load_x(const float* __restrict__ X, int k, int64_t row0, int nr, bool vec, float* Xl, int tid) {
#pragma unroll
  for (int g = tid; g < TS * 16; g += NT) {
    const int r = g >> 4, c = (g & 15) * 4;
    f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (r < nr && c < k) {
      const float* src = X + (row0 + r) * k + c;
      if (vec) {
        v = *reinterpret_cast<const f32x4*>(src);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (c + j < k) v[j] = src[j];
      }
    }
    *reinterpret_cast<f32x4*>(Xl + r * LDD + c) = v;
  }
}

// the k x k Gram partial of the nm rows of Yl, fp64, rows in index order
__device__ __forceinline__ void gram_partial(const float* Yl, int k, int nm, double* part, int tid) {
  for (int e = tid; e < k * k; e += NT) {
    const int i = e / k, j = e - i * k;
    double g = 0.0;
    for (int mm = 0; mm < nm; ++mm) g = __builtin_fma((double)Yl[mm * LDD + i], (double)Yl[mm * LDD + j], g);
    part[e] = g;
  }
}

// TRANS = false: Y [out, k] = D X with X = Z [in, k]; a block owns rows chunk * 64 ...
// TRANS = true:  Z [in, k] = D^T X with X = Y [out, k] (fin: X = Q in the flat buffer, the result goes to A [k, in] transposed)
template <bool TRANS>
__global__ __launch_bounds__(NT) void lowrank_product_kernel(const qfx_lowrank_args a, int first, int fin) {
  __shared__ __attribute__((aligned(16))) float Dl[TS * LDD];
  __shared__ __attribute__((aligned(16))) float Xl[TS * LDD];
  __shared__ double red[NT];
  const int m = blockIdx.y, tid = threadIdx.x;
  const qfx_lowrank_mat t = a.table[m];
  if (!dims_ok(t)) return;
  const int k = t.k;
  const int64_t nM = TRANS ? t.in_features : t.out_features, nK = TRANS ? t.out_features : t.in_features;
  const int64_t m0 = (int64_t)blockIdx.x * TS;
  if (m0 >= nM) return;
  const int nm = (int)(nM - m0 < TS ? nM - m0 : TS);
  const MatWs w = mat_ws(a, m, t);
  const float* __restrict__ X = TRANS ? (fin ? a.p + t.off_b : w.Y) : w.Z;
  float* O = TRANS ? w.Z : w.Y;
  float* A = a.p + t.off_a;
  double* part = w.part + (int64_t)blockIdx.x * k * k;
  if (!first && mat_state(a, m)[0]) {            // a skipped matrix: zeros
    if (fin) {
      for (int e = tid; e < k * TS; e += NT)
        if ((e & 63) < nm) A[(int64_t)(e >> 6) * t.in_features + m0 + (e & 63)] = 0.f;
    } else {
      for (int e = tid; e < nm * k; e += NT) O[m0 * k + e] = 0.f;
      for (int e = tid; e < k * k; e += NT) part[e] = 0.0;
    }
    return;
  }
  const bool dvec = d_vec(t), xvec = (k & 3) == 0 && (((uintptr_t)X & 15) == 0);
  const int rg = tid >> 4, cg = tid & 15;
  float acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0.f;
  double nsq = 0.0;
  int bad = 0;
  for (int64_t k0 = 0; k0 < nK; k0 += TS) {
    const int nk = (int)(nK - k0 < TS ? nK - k0 : TS);
    __syncthreads();                             // the previous tiles have been read
    if (TRANS) {
      load_d<false>(t, dvec, k0, m0, Dl, tid, nsq, bad);
    } else if (first) {
      load_d<true>(t, dvec, m0, k0, Dl, tid, nsq, bad);
    } else {
      load_d<false>(t, dvec, m0, k0, Dl, tid, nsq, bad);
    }
    load_x(X, k, k0, nk, xvec, Xl, tid);
    __syncthreads();
    if (4 * cg < k) {                            // the summed index ascends: one fp32 FMA per term
      if (TRANS) {
#pragma unroll 8
        for (int kk = 0; kk < TS; ++kk) {
          const f32x4 d = *reinterpret_cast<const f32x4*>(Dl + kk * LDD + 4 * rg);
          const f32x4 x = *reinterpret_cast<const f32x4*>(Xl + kk * LDD + 4 * cg);
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[u][v] = __builtin_fmaf(d[u], x[v], acc[u][v]);
        }
      } else {
#pragma unroll 2
        for (int kq = 0; kq < TS / 4; ++kq) {
          f32x4 d[4], x[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) d[u] = *reinterpret_cast<const f32x4*>(Dl + (4 * rg + u) * LDD + 4 * kq);
#pragma unroll
          for (int j = 0; j < 4; ++j) x[j] = *reinterpret_cast<const f32x4*>(Xl + (4 * kq + j) * LDD + 4 * cg);
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
              for (int v = 0; v < 4; ++v) acc[u][v] = __builtin_fmaf(d[u][j], x[j][v], acc[u][v]);
        }
      }
    }
  }
  __syncthreads();
  float* Yl = Xl;
#pragma unroll
  for (int u = 0; u < 4; ++u) *reinterpret_cast<f32x4*>(Yl + (4 * rg + u) * LDD + 4 * cg) = (f32x4){acc[u][0], acc[u][1], acc[u][2], acc[u][3]};
  __syncthreads();
  if (fin) {
    for (int e = tid; e < k * TS; e += NT) {
      const int c = e >> 6, mm = e & 63;
      if (mm < nm) A[(int64_t)c * t.in_features + m0 + mm] = Yl[mm * LDD + c];
    }
    return;
  }
  for (int e = tid; e < nm * k; e += NT) {
    const int mm = e / k, c = e - mm * k;
    O[m0 * k + e] = Yl[mm * LDD + c];
  }
  gram_partial(Yl, k, nm, part, tid);
  if (!TRANS && first) {
    const double s = block_sum(nsq, red, tid);
    const int b = __syncthreads_or(bad);
    if (tid == 0) {
      w.nsq[blockIdx.x] = s;
      w.flag[blockIdx.x] = b;
    }
  }
}

struct Small {
  double red[NT];
  double ls[KMAX];                          // the eigenvalues, sorted descending
  JacobiRot rot;
  int perm[KMAX];
  int keep;
};

// side 0: the Gram partials of Y (row chunks of D), side 1: of Z (column chunks).  first: also the skip verdict and normsq.
__global__ __launch_bounds__(NT) void lowrank_solve_kernel(const qfx_lowrank_args a, int side, int first, int last) {
  __shared__ double M[MSZ];
  __shared__ double V[MSZ];
  __shared__ Small sm;
  const int m = blockIdx.x, tid = threadIdx.x;
  const qfx_lowrank_mat t = a.table[m];
  if (!dims_ok(t)) {
    if (last && tid == 0) { a.info[2 * m] = 0; a.info[2 * m + 1] = 0; a.normsq[m] = 0.0; }
    return;
  }
  const int k = t.k;
  const MatWs w = mat_ws(a, m, t);
  int* st = mat_state(a, m);
  int bad;
  if (first) {
    const int co = chunks_of(t.out_features);
    int loc = 0;
    double s = 0.0;
    for (int c = tid; c < co; c += NT) {
      loc |= w.flag[c];
      s = s + w.nsq[c];
    }
    bad = __syncthreads_or(loc);
    s = block_sum(s, sm.red, tid);
    if (tid == 0) {
      st[0] = bad;
      a.normsq[m] = bad ? 0.0 : s;
    }
  } else {
    bad = st[0];
  }
  if (bad) {                                 // uniform over the block
    for (int e = tid; e < 64 * 64; e += NT) w.T[e] = 0.0;
    if (tid == 0) {
      st[1] = 0; st[2] = 0;
      if (last) {
        a.info[2 * m] = 0; a.info[2 * m + 1] = 0;
        atomicAdd(a.skipped, 1);
      }
    }
    return;
  }
  const int nch = chunks_of(side ? t.in_features : t.out_features);
  for (int e = tid; e < k * k; e += NT) {
    double g = 0.0;
    for (int c = 0; c < nch; ++c) g = g + w.part[(int64_t)c * k * k + e];
    const int i = e / k, j = e - i * k;
    M[i * LDM + j] = g;
  }
  __syncthreads();
  int conv = 0;
  jacobi(M, V, k, a.max_sweeps, sm.rot, sm.red, conv, tid);
  if (tid < k) {                             // descending, ties by index
    const double me = M[tid * LDM + tid];
    int rank = 0;
    for (int j = 0; j < k; ++j) {
      const double o = M[j * LDM + j];
      rank += (o > me) || (o == me && j < tid);
    }
    sm.perm[rank] = tid;
    sm.ls[rank] = me;
  }
  __syncthreads();
  if (tid == 0) {
    const double lmax = sm.ls[0];
    int keep = 0;
    if (lmax > 0.0)
      for (int i = 0; i < k; ++i) keep += sm.ls[i] > a.orth_tol * lmax;
    sm.keep = keep;
    const int cv = first ? conv : (st[2] & conv);
    st[1] = keep;
    st[2] = cv;
    if (last) { a.info[2 * m] = keep; a.info[2 * m + 1] = cv; }
  }
  __syncthreads();
  const int keep = sm.keep;
  for (int e = tid; e < 64 * 64; e += NT) {
    const int i = e >> 6, j = e & 63;
    w.T[e] = (i < k && j < keep) ? V[i * LDM + sm.perm[j]] / sqrt(sm.ls[j]) : 0.0;
  }
}

// Y <- fp32(Y T) over the chunk's rows, in place (to_b: into B of the flat buffer); gram: the partial of the result
__global__ __launch_bounds__(NT) void lowrank_apply_kernel(const qfx_lowrank_args a, int side, int gram, int to_b) {
  __shared__ double Tl[64 * 64];
  __shared__ __attribute__((aligned(16))) float Yl[TS * LDD];
  __shared__ __attribute__((aligned(16))) float Y2[TS * LDD];
  const int m = blockIdx.y, tid = threadIdx.x;
  const qfx_lowrank_mat t = a.table[m];
  if (!dims_ok(t)) return;
  const int k = t.k;
  const int64_t n = side ? t.in_features : t.out_features;
  const int64_t m0 = (int64_t)blockIdx.x * TS;
  if (m0 >= n) return;
  const int nm = (int)(n - m0 < TS ? n - m0 : TS);
  const MatWs w = mat_ws(a, m, t);
  const float* src = (side ? w.Z : w.Y) + m0 * k;
  float* dst = (to_b ? a.p + t.off_b : (side ? w.Z : w.Y)) + m0 * k;
  double* part = w.part + (int64_t)blockIdx.x * k * k;
  if (mat_state(a, m)[0]) {
    for (int e = tid; e < nm * k; e += NT) dst[e] = 0.f;
    if (gram)
      for (int e = tid; e < k * k; e += NT) part[e] = 0.0;
    return;
  }
  for (int e = tid; e < 64 * 64; e += NT) Tl[e] = w.T[e];
  for (int e = tid; e < nm * k; e += NT) {
    const int mm = e / k;
    Yl[mm * LDD + (e - mm * k)] = src[e];
  }
  __syncthreads();
  for (int e = tid; e < nm * k; e += NT) {
    const int mm = e / k, c = e - mm * k;
    double acc = 0.0;
    for (int i = 0; i < k; ++i) acc = acc + (double)Yl[mm * LDD + i] * Tl[i * 64 + c];
    const float v = (float)acc;
    dst[e] = v;
    Y2[mm * LDD + c] = v;
  }
  if (!gram) return;
  __syncthreads();
  gram_partial(Y2, k, nm, part, tid);
}

inline int check_host(const qfx_lowrank_mat* tab, int32_t n_mats, int64_t n_elems) {
  return check_pair_table(n_mats, n_elems, tab != nullptr, KMAX, [&](int32_t i, PairDims& d) {
    const qfx_lowrank_mat& t = tab[i];
    d = {t.off_a, t.off_b, t.k, t.in_features, t.out_features};
    return dims_ok(t);                       // also the dtype, the pointers and the leading dimensions
  });
}

}  // namespace

extern "C" int qfx_lowrank_check_table(const qfx_lowrank_mat* host_table, int32_t n_mats, int64_t n_elems) {
  return check_host(host_table, n_mats, n_elems);
}

extern "C" int64_t qfx_lowrank_sketch_workspace(const qfx_lowrank_mat* host_table, int32_t n_mats) {
  if (n_mats < 0 || (n_mats > 0 && !host_table)) return QFX_EINVAL;
  int64_t at = header_bytes(n_mats);
  for (int32_t i = 0; i < n_mats; ++i) {
    if (!dims_ok(host_table[i])) return QFX_EINVAL;
    at += mat_bytes(host_table[i].k, host_table[i].in_features, host_table[i].out_features);
  }
  return at;
}

extern "C" int qfx_lowrank_sketch(const qfx_lowrank_args* a, void* stream) {
  if (!a || a->n_mats < 0 || a->n_mats > MAX_MATS) return QFX_EINVAL;
  if (a->q < 0 || a->q > 4 || a->max_sweeps < 1 || a->max_sweeps > 64) return QFX_EINVAL;
  if (!(a->orth_tol >= 0.0 && a->orth_tol < 1.0)) return QFX_EINVAL;                 // a NaN fails
  if (a->n_mats == 0) return QFX_OK;
  if (!a->table || !a->host_table || !a->p || !a->normsq || !a->info || !a->skipped || !a->ws) return QFX_EINVAL;
  if (((uintptr_t)a->ws & 15) != 0) return QFX_EINVAL;
  if (check_host(a->host_table, a->n_mats, a->n_elems) != QFX_OK) return QFX_EINVAL;
  if (a->ws_bytes < qfx_lowrank_sketch_workspace(a->host_table, a->n_mats)) return QFX_EINVAL;
  int co = 1, ci = 1;
  for (int32_t i = 0; i < a->n_mats; ++i) {
    co = std::max(co, chunks_of(a->host_table[i].out_features));
    ci = std::max(ci, chunks_of(a->host_table[i].in_features));
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 go((unsigned)co, (unsigned)a->n_mats), gi((unsigned)ci, (unsigned)a->n_mats), gm((unsigned)a->n_mats), nt(NT);
  if (hipMemsetAsync(a->skipped, 0, sizeof(int32_t), s) != hipSuccess) return QFX_EINVAL;
  hipLaunchKernelGGL(lowrank_init_kernel, dim3(1), dim3(64), 0, s, *a);
  hipLaunchKernelGGL(lowrank_omega_kernel, gi, nt, 0, s, *a);
  // orth twice over Y (side 0) or Z (side 1); the last apply of the sequence writes Q into the flat buffer
  auto orth = [&](int side, int first, int last) {
    const dim3& g = side ? gi : go;
    hipLaunchKernelGGL(lowrank_solve_kernel, gm, nt, 0, s, *a, side, first, 0);
    hipLaunchKernelGGL(lowrank_apply_kernel, g, nt, 0, s, *a, side, 1, 0);
    hipLaunchKernelGGL(lowrank_solve_kernel, gm, nt, 0, s, *a, side, 0, last);
    hipLaunchKernelGGL(lowrank_apply_kernel, g, nt, 0, s, *a, side, 0, last);
  };
  hipLaunchKernelGGL(lowrank_product_kernel<false>, go, nt, 0, s, *a, 1, 0);
  orth(0, 1, a->q == 0);
  for (int it = 0; it < a->q; ++it) {
    hipLaunchKernelGGL(lowrank_product_kernel<true>, gi, nt, 0, s, *a, 0, 0);
    orth(1, 0, 0);
    hipLaunchKernelGGL(lowrank_product_kernel<false>, go, nt, 0, s, *a, 0, 0);
    orth(0, 0, it == a->q - 1);
  }
  hipLaunchKernelGGL(lowrank_product_kernel<true>, gi, nt, 0, s, *a, 0, 1);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
