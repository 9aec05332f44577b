// qfx_came.hip -- CAME (came_pytorch.CAME) over the flat LoRA buffers: ONE launch, one workgroup per tensor, driven by a device table
// of per-tensor descriptors (include/qfx.h).  Adafactor's factored second moment, a full first moment m, and a second factored pair
// over the instability (upd - m)^2 that rescales m.  Per tensor: is every g' finite, |p|^2 (sweep 1); row and column means of
// g'^2 + eps1 (2a, 2b); |upd|^2 (3); m and the row means of the instability (4a), its column means (4b); the parameters (5).  Every
// sum is formed inside the tensor's own workgroup in an order that depends only on the tensor's shape: a lane owns groups of four
// consecutive columns (one 16-byte access where the tensor's alignment allows, four 4-byte ones otherwise -- the same order of
// additions either way), xor-shuffle trees fold the lanes of a row, fixed folds through LDS fold the rows of a column.  No atomics,
// same inputs -> same bits.  A tensor is 0.2 - 3 MB of fp32; after the first sweep it is read from L2.  Built without FMA
// contraction: the update is formed twice (4a, 4b) and must round the same way both times, and tests/came_ref.py states every
// rounding point.
#include "qfx_common.h"
#include "qfx_optim.h"

namespace {

constexpr int NT = 256;

// four consecutive elements at s, nv of them valid (the rest read as 0); vec: s is 16-byte aligned and nv == 4
__device__ __forceinline__ void ld4(const float* __restrict__ s, int nv, bool vec, float (&x)[4]) {
  if (vec) {
    const f32x4 t = *(const f32x4*)s;
    x[0] = t[0]; x[1] = t[1]; x[2] = t[2]; x[3] = t[3];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = j < nv ? s[j] : 0.f;
  }
}
__device__ __forceinline__ void st4(float* __restrict__ d, int nv, bool vec, const float (&x)[4]) {
  if (vec) {
    f32x4 t; t[0] = x[0]; t[1] = x[1]; t[2] = x[2]; t[3] = x[3];
    *(f32x4*)d = t;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) if (j < nv) d[j] = x[j];
  }
}

__device__ __forceinline__ float rsq(float x) { return 1.0f / sqrtf(x); }

// column sums of one statistic, part 2: fold the CY partial sums of every column of the trip q0 in the order of cy and blend them
// into `stat`.  part[j * NT + cy * TXc + cx] holds the partial sum of column 4 (q0 + cx) + j.
__device__ __forceinline__ void fold_columns(const float* part, float* __restrict__ stat, int q0, int TXc, int CY, int C, int R, float b,
                                             float omb) {
  for (int w = threadIdx.x; w < 4 * TXc; w += NT) {
    const int j = w / TXc, x = w - j * TXc;
    const int c = (q0 + x) * 4 + j;
    if (c < C) {
      float tot = part[j * NT + x];
      for (int y = 1; y < CY; ++y) tot += part[j * NT + y * TXc + x];
      stat[c] = b * stat[c] + omb * (tot / (float)R);
    }
  }
}

__global__ __launch_bounds__(256) void came_kernel(const qfx_came_args a) {
  __shared__ float red[4];
  __shared__ float part[4 * NT];
  const int tid = threadIdx.x;
  const float clip = opt_clip(a.gnorm_sq, a.max_norm, a.grad_scale);
  const float b1 = a.beta1, omb1 = a.one_minus_beta1, b2 = a.beta2, omb2 = a.one_minus_beta2, b3 = a.beta3, omb3 = a.one_minus_beta3;
  const float eps1 = a.eps1, eps2 = a.eps2, lr = a.lr;
  const float decay = -(a.weight_decay * lr);
  for (int ti = blockIdx.x; ti < a.n_tensors; ti += gridDim.x) {
    const qfx_came_tensor t = a.table[ti];
    const int R = t.rows, C = t.cols, n = R * C;
    float* p = a.p + t.off;
    const float* g = a.g + t.off;
    float* m = a.m + t.off;
    const bool alf = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m)) & 15) == 0;      // the tensor starts on 16 bytes everywhere
    const bool alr = alf && (C & 3) == 0;                                                 // and so does every row

    // sweep 1: is every clipped gradient finite?  |p|^2.  Nothing has been written yet: a tensor with a non-finite gradient is left.
    float pp = 0.f;
    int bad = 0;
    for (int i = tid * 4; i < n; i += NT * 4) {
      const int nv = n - i < 4 ? n - i : 4;
      float gx[4], px[4];
      ld4(g + i, nv, alf && nv == 4, gx);
      ld4(p + i, nv, alf && nv == 4, px);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nv) {
          bad |= !__builtin_isfinite(gx[j] * clip);
          pp += px[j] * px[j];
        }
    }
    if (__syncthreads_or(bad)) continue;       // the same verdict on every thread
    const float prms = sqrtf(block_sum(pp, red)) / sqrtf((float)n);
    if (tid == 0) a.rms[t.rms] = prms;

    float ss = 0.f;      // |upd|^2
    if (t.factored) {
      float* row = a.row + t.row;
      float* col = a.col + t.col;
      float* rrow = a.rrow + t.rrow;
      float* rcol = a.rcol + t.rcol;
      const int CG = (C + 3) >> 2;             // groups of four columns
      // the row walk: TX lanes of one wave (a power of two, 1 .. 64) own a row and stride over its column groups, GY rows at a time
      int TX = 1;
      while (TX < CG && TX < 64) TX <<= 1;
      const int tx = tid & (TX - 1), gy = tid / TX, GY = NT / TX;
      // the column walk: TXc threads side by side on the column groups, CY = 256 / TXc of them down the rows
      int TXc = 1;
      while (TXc < CG && TXc < NT) TXc <<= 1;
      const int cx = tid & (TXc - 1), cy = tid / TXc, CY = NT / TXc;

      // sweep 2a: row means of g'^2 + eps1 -> row, and the mean of row
      float racc = 0.f;
      for (int r0 = 0; r0 < R; r0 += GY) {           // uniform trip count: every lane reaches the shuffles
        const int r = r0 + gy;
        float s = 0.f;
        if (r < R) {
          const float* gr = g + (int64_t)r * C;
          for (int q = tx; q < CG; q += TX) {
            const int c0 = q * 4, nv = C - c0 < 4 ? C - c0 : 4;
            float gx[4];
            ld4(gr + c0, nv, alr, gx);
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (j < nv) {
                const float gi = gx[j] * clip;
                s += gi * gi + eps1;
              }
          }
        }
        for (int o = TX >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (r < R && tx == 0) {
          const float nr = b2 * row[r] + omb2 * (s / (float)C);
          row[r] = nr;
          racc += nr;
        }
      }
      const float rmean = block_sum(racc, red) / (float)R;
      // sweep 2b: column means of g'^2 + eps1 -> col
      for (int q0 = 0; q0 < CG; q0 += TXc) {
        const int q = q0 + cx;
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        if (q < CG) {
          const int c0 = q * 4, nv = C - c0 < 4 ? C - c0 : 4;
          for (int r = cy; r < R; r += CY) {
            float gx[4];
            ld4(g + (int64_t)r * C + c0, nv, alr, gx);
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (j < nv) {
                const float gi = gx[j] * clip;
                s[j] += gi * gi + eps1;
              }
          }
        }
        __syncthreads();                             // part: the previous trip's fold has read it
#pragma unroll
        for (int j = 0; j < 4; ++j) part[j * NT + tid] = s[j];      // tid == cy * TXc + cx
        __syncthreads();
        fold_columns(part, col, q0, TXc, CY, C, R, b2, omb2);
      }
      __syncthreads();                               // row / col as written above are what the sweeps below read
      // sweep 3: |upd|^2 with upd = (rsqrt(row / mean(row)) * rsqrt(col)) * g'
      for (int r0 = 0; r0 < R; r0 += GY) {
        const int r = r0 + gy;
        if (r < R) {
          const float rf = rsq(row[r] / rmean);
          const float* gr = g + (int64_t)r * C;
          for (int q = tx; q < CG; q += TX) {
            const int c0 = q * 4, nv = C - c0 < 4 ? C - c0 : 4;
            float gx[4];
            ld4(gr + c0, nv, alr, gx);
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (j < nv) {
                const float u = (rf * rsq(col[c0 + j])) * (gx[j] * clip);
                ss += u * u;
              }
          }
        }
      }
      const float urms = sqrtf(block_sum(ss, red)) / sqrtf((float)n);
      const float den = fmaxf(1.0f, urms / a.clip_threshold);
      // sweep 4a: the clipped update, m, row means of the instability (upd - m)^2 + eps2 -> rrow, and the mean of rrow
      float rracc = 0.f;
      for (int r0 = 0; r0 < R; r0 += GY) {
        const int r = r0 + gy;
        float s = 0.f;
        if (r < R) {
          const float rf = rsq(row[r] / rmean);
          const int64_t base = (int64_t)r * C;
          for (int q = tx; q < CG; q += TX) {
            const int c0 = q * 4, nv = C - c0 < 4 ? C - c0 : 4;
            float gx[4], mx[4];
            ld4(g + base + c0, nv, alr, gx);
            ld4(m + base + c0, nv, alr, mx);
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (j < nv) {
                const float u = ((rf * rsq(col[c0 + j])) * (gx[j] * clip)) / den;
                const float mn = b1 * mx[j] + omb1 * u;
                const float d = u - mn;
                mx[j] = mn;
                s += d * d + eps2;
              }
            st4(m + base + c0, nv, alr, mx);
          }
        }
        for (int o = TX >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (r < R && tx == 0) {
          const float nr = b3 * rrow[r] + omb3 * (s / (float)C);
          rrow[r] = nr;
          rracc += nr;
        }
      }
      const float rrmean = block_sum(rracc, red) / (float)R;      // its barriers: m and rrow as written above are visible below
      // sweep 4b: column means of the instability -> rcol; the update is formed again, with the roundings of 4a
      for (int q0 = 0; q0 < CG; q0 += TXc) {
        const int q = q0 + cx;
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        if (q < CG) {
          const int c0 = q * 4, nv = C - c0 < 4 ? C - c0 : 4;
          float cf[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) cf[j] = j < nv ? rsq(col[c0 + j]) : 0.f;
          for (int r = cy; r < R; r += CY) {
            const float rf = rsq(row[r] / rmean);
            float gx[4], mx[4];
            ld4(g + (int64_t)r * C + c0, nv, alr, gx);
            ld4(m + (int64_t)r * C + c0, nv, alr, mx);
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (j < nv) {
                const float u = ((rf * cf[j]) * (gx[j] * clip)) / den;
                const float d = u - mx[j];
                s[j] += d * d + eps2;
              }
          }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) part[j * NT + tid] = s[j];
        __syncthreads();
        fold_columns(part, rcol, q0, TXc, CY, C, R, b3, omb3);
      }
      __syncthreads();                               // rcol
      // sweep 5: out = (rsqrt(rrow / mean(rrow)) * rsqrt(rcol)) * m; decay; parameters
      for (int r0 = 0; r0 < R; r0 += GY) {
        const int r = r0 + gy;
        if (r < R) {
          const float rf = rsq(rrow[r] / rrmean);
          const int64_t base = (int64_t)r * C;
          for (int q = tx; q < CG; q += TX) {
            const int c0 = q * 4, nv = C - c0 < 4 ? C - c0 : 4;
            float mx[4], px[4];
            ld4(m + base + c0, nv, alr, mx);
            ld4(p + base + c0, nv, alr, px);
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (j < nv) {
                const float out = (rf * rsq(rcol[c0 + j])) * mx[j];
                float pi = px[j];
                if (a.weight_decay != 0.f) pi += pi * decay;
                px[j] = pi - lr * out;
              }
            st4(p + base + c0, nv, alr, px);
          }
        }
      }
    } else {
      // unfactored: v is elementwise, out = m; every element is read and written by the thread that owns it
      float* v = a.v + t.v;
      for (int i = tid; i < n; i += NT) {
        const float gi = g[i] * clip;
        const float vi = b2 * v[i] + omb2 * (gi * gi + eps1);
        v[i] = vi;
        const float u = rsq(vi) * gi;
        ss += u * u;
      }
      const float urms = sqrtf(block_sum(ss, red)) / sqrtf((float)n);
      const float den = fmaxf(1.0f, urms / a.clip_threshold);
      for (int i = tid; i < n; i += NT) {
        const float u = (rsq(v[i]) * (g[i] * clip)) / den;
        const float mn = b1 * m[i] + omb1 * u;
        m[i] = mn;
        float pi = p[i];
        if (a.weight_decay != 0.f) pi += pi * decay;
        p[i] = pi - lr * mn;
      }
    }
  }
}

inline bool unit(float b) { return b >= 0.f && b <= 1.f; }      // a NaN fails

}  // namespace

extern "C" int qfx_came_step(const qfx_came_args* a, void* stream) {
  if (!a || a->n_tensors < 0) return QFX_EINVAL;
  if (a->n_tensors == 0) return QFX_OK;
  if (!a->table || !a->p || !a->g || !a->row || !a->col || !a->rrow || !a->rcol || !a->v || !a->m || !a->rms) return QFX_EINVAL;
  if (!(a->lr >= 0.f) || !unit(a->beta1) || !unit(a->beta2) || !unit(a->beta3) || !unit(a->one_minus_beta1) ||
      !unit(a->one_minus_beta2) || !unit(a->one_minus_beta3))
    return QFX_EINVAL;
  if (!(a->eps1 >= 0.f) || !(a->eps2 >= 0.f) || !(a->clip_threshold > 0.f) || !(a->weight_decay >= 0.f)) return QFX_EINVAL;
  const int wgs = a->n_tensors < 2048 ? a->n_tensors : 2048;
  hipLaunchKernelGGL(came_kernel, dim3((unsigned)wgs), dim3(NT), 0, (hipStream_t)stream, *a);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
