// qfx_lora_fold.hip -- W <- W + c B A over every dense matrix of a device table, in place: the residual trunk of a PiSSA
// initialisation (c = -scaling) in one pass, bit-reproducible.  The listing in include/qfx.h is the specification
// (tests/pissa_ref.py restates it).  Two launches on one stream:
//   prefix    one workgroup: tile_start[m] = the number of 64 x 64 tiles of the matrices before m (the host sizes the grid from
//             its copy of the table by the same count)
//   fold      a flat grid over (tile, matrix): the block's first wave finds its matrix in tile_start (a 64-ary search of the
//             sorted table), the block stages the tile's B [64, r] and A [r, 64] in LDS as fp32, and every lane folds its own elements: an fp64 dot over j in ascending order, the multiply by c,
//             the addition to the widened W, the rounding to fp32 and, for a bf16 W, to bf16.  A lane reads and writes the same
//             elements (two runs of 8 bf16 or four runs of 4 fp32, in rows 32 resp. 16 apart: the widened A values are shared)
// No atomics, nothing crosses a workgroup: same inputs -> same bits at any address and in any table order.
#include "qfx_common.h"

#pragma clang fp contract(off)

#include <algorithm>
#include <utility>
#include <vector>

namespace {

constexpr int NT = 256;                     // four waves
constexpr int TS = 64;                      // the tile edge
constexpr int RMAX = 64;                    // largest rank
constexpr int DIM_MAX = 1 << 24;            // largest in_features / out_features
constexpr int MAX_MATS = 65535;
constexpr int64_t MAX_TILES = (1 << 24) - 1;   // the flat grid: blocks x 256 lanes stay below 2^32
constexpr int LDA = TS + 4;                 // row stride of the A tile in LDS (16-byte rows)
constexpr int LDB = RMAX + 1;               // row stride of the B tile (odd: the rows of a wave fall on different banks)

__host__ __device__ inline bool dims_ok(const qfx_lora_fold_mat& t) {
  return t.r >= 1 && t.r <= RMAX && t.in_features >= 1 && t.in_features <= DIM_MAX && t.out_features >= 1 && t.out_features <= DIM_MAX &&
         (t.dtype == 0 || t.dtype == 1) && t.w != nullptr && t.ld >= t.in_features && t.off_a >= 0 && t.off_b >= 0;
}

__host__ __device__ inline int64_t tiles_of(const qfx_lora_fold_mat& t) {
  return (int64_t)((t.out_features + TS - 1) / TS) * ((t.in_features + TS - 1) / TS);
}

// tile_start [n_mats + 1]: a row the fold would not touch counts no tiles
__global__ __launch_bounds__(NT) void lora_fold_prefix_kernel(const qfx_lora_fold_args a) {
  __shared__ int64_t part[NT];
  const int tid = threadIdx.x, n = a.n_mats;
  const int per = (n + NT - 1) / NT, lo = tid * per, hi = lo + per < n ? lo + per : n;
  int64_t s = 0;
  for (int m = lo; m < hi; ++m) {
    const qfx_lora_fold_mat t = a.table[m];
    s += dims_ok(t) ? tiles_of(t) : 0;
  }
  part[tid] = s;
  __syncthreads();
  int64_t at = 0;
  for (int i = 0; i < tid; ++i) at += part[i];
  for (int m = lo; m < hi; ++m) {
    const qfx_lora_fold_mat t = a.table[m];
    a.tile_start[m] = at;
    at += dims_ok(t) ? tiles_of(t) : 0;
  }
  if (tid == NT - 1) a.tile_start[n] = at;  // (the last lane's range ends the table, or is empty behind it)
}

// BF: W is bf16, a lane owns 2 runs of 8 elements; else fp32, 4 runs of 4
template <bool BF>
__device__ __forceinline__ void fold_tile(const qfx_lora_fold_mat& t, int64_t row0, int64_t col0, const float* Al, const float* Bl, int tid) {
  constexpr int E = BF ? 8 : 4, NR = BF ? 2 : 4, RSTEP = TS / NR, GPR = TS / E;      // run length, runs per lane, rows between them
  const int nr = (int)(t.out_features - row0 < TS ? t.out_features - row0 : TS);
  const int nc = (int)(t.in_features - col0 < TS ? t.in_features - col0 : TS);
  const int r0 = tid / GPR, c = (tid % GPR) * E;
  const bool vec = (((uintptr_t)t.w & 15) == 0) && (t.ld % E) == 0;
  const bool whole = c + E <= nc;
  bf16_t* wb = reinterpret_cast<bf16_t*>(t.w);
  float* wf = reinterpret_cast<float*>(t.w);
  float w[NR][E];
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    const int r = r0 + u * RSTEP;
    const int64_t at = (row0 + r) * t.ld + col0 + c;
#pragma unroll
    for (int e = 0; e < E; ++e) w[u][e] = 0.f;
    if (r >= nr) continue;
    if (vec && whole) {
      if (BF) {
        const u32x4 x = *reinterpret_cast<const u32x4*>(wb + at);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          w[u][2 * i] = __uint_as_float(x[i] << 16);
          w[u][2 * i + 1] = __uint_as_float(x[i] & 0xFFFF0000u);
        }
      } else {
        const f32x4 x = *reinterpret_cast<const f32x4*>(wf + at);
#pragma unroll
        for (int e = 0; e < 4; ++e) w[u][e] = x[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (c + e < nc) w[u][e] = BF ? bf2f(wb[at + e]) : wf[at + e];
    }
  }
  double acc[NR][E];
#pragma unroll
  for (int u = 0; u < NR; ++u)
#pragma unroll
    for (int e = 0; e < E; ++e) acc[u][e] = 0.0;
  for (int j = 0; j < t.r; ++j) {                // ascending j from +0; the product of two widened fp32 values is exact
    double av[E], bv[NR];
#pragma unroll
    for (int q = 0; q < E / 4; ++q) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(Al + j * LDA + c + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) av[4 * q + e] = (double)x[e];
    }
#pragma unroll
    for (int u = 0; u < NR; ++u) bv[u] = (double)Bl[(r0 + u * RSTEP) * LDB + j];
#pragma unroll
    for (int u = 0; u < NR; ++u)
#pragma unroll
      for (int e = 0; e < E; ++e) acc[u][e] = __builtin_fma(bv[u], av[e], acc[u][e]);
  }
  const double cd = (double)t.c;
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    const int r = r0 + u * RSTEP;
    if (r >= nr) continue;
    const int64_t at = (row0 + r) * t.ld + col0 + c;
    float o[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const double tt = cd * acc[u][e];
      const double wn = (double)w[u][e] + tt;
      o[e] = (float)wn;
    }
    if (vec && whole) {
      if (BF) {
        u32x4 x;
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = (uint32_t)f2bf(o[2 * i]) | ((uint32_t)f2bf(o[2 * i + 1]) << 16);
        *reinterpret_cast<u32x4*>(wb + at) = x;
      } else {
        *reinterpret_cast<f32x4*>(wf + at) = (f32x4){o[0], o[1], o[2], o[3]};
      }
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (c + e < nc) {
          if (BF) wb[at + e] = f2bf(o[e]);
          else    wf[at + e] = o[e];
        }
      }
    }
  }
}

__global__ __launch_bounds__(NT) void lora_fold_kernel(const qfx_lora_fold_args a) {
  __shared__ __attribute__((aligned(16))) float Al[RMAX * LDA];
  __shared__ float Bl[TS * LDB];
  __shared__ int which;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (tid < 64) {                                  // wave 0: a 64-ary search of the sorted prefix table, one load per lane and round
    int lo = 0, len = a.n_mats;                    // b lies in a matrix of [lo, lo + len): tile_start[lo] <= b throughout
    while (len > 1) {
      const int step = (len + 63) >> 6, idx = lo + tid * step;
      const bool below = idx < lo + len && a.tile_start[idx] <= b;      // true for the sub-ranges up to the one that holds b
      const int j = __popcll(__ballot(below)) - 1;
      const int end = lo + len;
      lo = lo + (j < 0 ? 0 : j) * step;
      len = end - lo < step ? end - lo : step;
    }
    if (tid == 0) which = (a.tile_start[lo] <= b && b < a.tile_start[lo + 1]) ? lo : -1;
  }
  __syncthreads();
  if (which < 0) return;                           // (a device table that is not the host table's copy: nothing is touched)
  const qfx_lora_fold_mat t = a.table[which];
  const int64_t local = b - a.tile_start[which];
  const int64_t tcols = (t.in_features + TS - 1) / TS;
  const int64_t row0 = (local / tcols) * TS, col0 = (local % tcols) * TS;
  const int nr = (int)(t.out_features - row0 < TS ? t.out_features - row0 : TS);
  const int nc = (int)(t.in_features - col0 < TS ? t.in_features - col0 : TS);
  const float* __restrict__ A = a.p + t.off_a;
  const float* __restrict__ B = a.p + t.off_b;
  for (int e = tid; e < t.r * TS; e += NT) {       // A [r, 64 columns of the tile], +0 past the matrix
    const int j = e >> 6, cc = e & 63;
    Al[j * LDA + cc] = cc < nc ? A[(int64_t)j * t.in_features + col0 + cc] : 0.f;
  }
  for (int e = tid; e < TS * t.r; e += NT) {       // B [64 rows of the tile, r]: one contiguous run of nr * r floats
    const int rr = e / t.r, j = e - rr * t.r;
    Bl[rr * LDB + j] = rr < nr ? B[row0 * t.r + e] : 0.f;
  }
  __syncthreads();
  if (t.dtype == 0) fold_tile<true>(t, row0, col0, Al, Bl, tid);
  else              fold_tile<false>(t, row0, col0, Al, Bl, tid);
}

inline int check_host(const qfx_lora_fold_mat* tab, int32_t n_mats, int64_t n_elems) {
  if (n_mats < 0 || n_mats > MAX_MATS || n_elems < 0 || (n_mats > 0 && !tab)) return QFX_EINVAL;
  std::vector<std::pair<uintptr_t, uintptr_t>> spans;
  spans.reserve((size_t)n_mats);
  int64_t tiles = 0;
  for (int32_t i = 0; i < n_mats; ++i) {
    const qfx_lora_fold_mat& t = tab[i];
    if (!dims_ok(t)) return QFX_EINVAL;
    const int64_t na = (int64_t)t.r * t.in_features, nb = (int64_t)t.out_features * t.r;
    if (na > n_elems || nb > n_elems || t.off_a > n_elems - na || t.off_b > n_elems - nb) return QFX_EINVAL;
    const uintptr_t lo = (uintptr_t)t.w;
    const uint64_t bytes = ((uint64_t)(t.out_features - 1) * (uint64_t)t.ld + (uint64_t)t.in_features) * (t.dtype == 0 ? 2u : 4u);
    if (bytes > UINTPTR_MAX - lo) return QFX_EINVAL;
    spans.emplace_back(lo, lo + bytes);
    tiles += tiles_of(t);
    if (tiles > MAX_TILES) return QFX_EINVAL;
  }
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i)
    if (spans[i].first < spans[i - 1].second) return QFX_EINVAL;
  return QFX_OK;
}

}  // namespace

extern "C" int qfx_lora_fold_check_table(const qfx_lora_fold_mat* host_table, int32_t n_mats, int64_t n_elems) {
  return check_host(host_table, n_mats, n_elems);
}

extern "C" int qfx_lora_fold(const qfx_lora_fold_args* a, void* stream) {
  if (!a || a->n_mats < 0 || a->n_mats > MAX_MATS) return QFX_EINVAL;
  if (a->n_mats == 0) return QFX_OK;
  if (!a->table || !a->host_table || !a->p || !a->tile_start) return QFX_EINVAL;
  if (check_host(a->host_table, a->n_mats, a->n_elems) != QFX_OK) return QFX_EINVAL;
  int64_t tiles = 0;
  for (int32_t i = 0; i < a->n_mats; ++i) tiles += tiles_of(a->host_table[i]);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lora_fold_prefix_kernel, dim3(1), dim3(NT), 0, s, *a);
  hipLaunchKernelGGL(lora_fold_kernel, dim3((unsigned)tiles), dim3(NT), 0, s, *a);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
