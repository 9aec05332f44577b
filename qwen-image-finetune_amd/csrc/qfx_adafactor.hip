// qfx_adafactor.hip -- Adafactor (transformers.optimization.Adafactor) over the flat LoRA buffers: ONE launch, one workgroup per
// tensor, driven by a device table of per-tensor descriptors (include/qfx.h).  The step is not elementwise: every tensor needs its
// row / column means of g^2, |p|^2 and |update|^2 before its parameters move.  All of them are formed inside the tensor's own
// workgroup in an order that depends only on the tensor's shape (per-lane strided sums, xor-shuffle trees, fixed folds through LDS):
// no atomics, same inputs -> same bits.  A tensor is 0.2 - 3 MB of fp32 and is swept several times; after the first sweep it is
// read from L2.
#include "qfx_common.h"
#include "qfx_optim.h"      // block_sum

namespace {

constexpr int NT = 256;

__global__ __launch_bounds__(256) void adafactor_kernel(const qfx_adafactor_args a) {
  __shared__ float red[4];
  __shared__ float part[NT];
  const int tid = threadIdx.x;
  float clip = a.grad_scale;
  if (a.gnorm_sq != nullptr && a.max_norm > 0.f) {      // = opt_clip (qfx_optim.h), written out: inlined, it compiles to other code here
    const float nrm = sqrtf(*a.gnorm_sq) * a.grad_scale;
    const float c = a.max_norm / (nrm + 1e-6f);
    clip *= c < 1.0f ? c : 1.0f;
  }
  const float b2 = a.beta2t, omb2 = a.one_minus_beta2t, eps1 = a.eps1;
  for (int ti = blockIdx.x; ti < a.n_tensors; ti += gridDim.x) {
    const qfx_adafactor_tensor t = a.table[ti];
    const int R = t.rows, C = t.cols, n = R * C;
    float* p = a.p + t.off;
    const float* g = a.g + t.off;

    // sweep 0: is every clipped gradient finite?  |p|^2.  Nothing has been written yet: a tensor with a non-finite gradient is left.
    float pp = 0.f;
    int bad = 0;
    for (int i = tid; i < n; i += NT) {
      const float gi = g[i] * clip;
      bad |= !__builtin_isfinite(gi);
      const float pi = p[i];
      pp += pi * pi;
    }
    if (__syncthreads_or(bad)) continue;       // the same verdict on every thread
    const float rms = sqrtf(block_sum(pp, red)) / sqrtf((float)n);
    if (tid == 0) a.rms[t.rms] = rms;
    float lr = a.lr;
    if (a.scale_parameter) lr *= fmaxf(a.eps2, rms);

    // rows are walked by groups of TX lanes of one wave (TX = 1 .. 64, a power of two): a group owns a row, its lanes stride over
    // the columns, an xor tree folds them.  [r, in] gives 4 rows per wave pass, [out, r] with r = 16 gives 16.
    int TX = 1;
    while (TX < C && TX < 64) TX <<= 1;
    const int tx = tid & (TX - 1), gy = tid / TX, GY = NT / TX;
    float ss = 0.f;      // |update|^2
    float rmean = 1.f;

    if (t.factored) {
      float* row = a.row + t.row;
      float* col = a.col + t.col;
      // sweep 1a: row means of g'^2 + eps1 -> row statistics, and their mean
      float racc = 0.f;
      for (int r0 = 0; r0 < R; r0 += GY) {           // uniform trip count: every lane reaches the shuffles
        const int r = r0 + gy;
        float s = 0.f;
        if (r < R) {
          const float* gr = g + (int64_t)r * C;
          for (int c = tx; c < C; c += TX) {
            const float gi = gr[c] * clip;
            s += gi * gi + eps1;
          }
        }
        for (int o = TX >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (r < R && tx == 0) {
          const float nr = b2 * row[r] + omb2 * (s / (float)C);
          row[r] = nr;
          racc += nr;
        }
      }
      rmean = block_sum(racc, red) / (float)R;
      // sweep 1b: column means.  TXc threads side by side on the columns (coalesced), CY = 256 / TXc of them down the rows, folded
      // through LDS in the order of cy.
      int TXc = 1;
      while (TXc < C && TXc < NT) TXc <<= 1;
      const int cx = tid & (TXc - 1), cy = tid / TXc, CY = NT / TXc;
      for (int c0 = 0; c0 < C; c0 += TXc) {
        const int c = c0 + cx;
        float s = 0.f;
        if (c < C)
          for (int r = cy; r < R; r += CY) {
            const float gi = g[(int64_t)r * C + c] * clip;
            s += gi * gi + eps1;
          }
        __syncthreads();                             // part: the previous trip's fold has read it
        part[tid] = s;                               // tid == cy * TXc + cx
        __syncthreads();
        if (cy == 0 && c < C) {
          float tot = part[cx];
          for (int y = 1; y < CY; ++y) tot += part[y * TXc + cx];
          col[c] = b2 * col[c] + omb2 * (tot / (float)R);
        }
      }
      __syncthreads();                               // row / col as written above are what the sweeps below read
      // sweep 2: |update|^2 with update = (rsqrt(row / mean(row)) * rsqrt(col)) * g'
      for (int r0 = 0; r0 < R; r0 += GY) {
        const int r = r0 + gy;
        if (r < R) {
          const float rf = 1.0f / sqrtf(row[r] / rmean);
          const float* gr = g + (int64_t)r * C;
          for (int c = tx; c < C; c += TX) {
            const float u = (rf * (1.0f / sqrtf(col[c]))) * (gr[c] * clip);
            ss += u * u;
          }
        }
      }
    } else {
      // unfactored: v is elementwise; sweep 1 and 2 are one
      float* v = a.v + t.v;
      for (int i = tid; i < n; i += NT) {
        const float gi = g[i] * clip;
        const float vi = b2 * v[i] + omb2 * (gi * gi + eps1);
        v[i] = vi;
        const float u = (1.0f / sqrtf(vi)) * gi;
        ss += u * u;
      }
    }

    const float urms = sqrtf(block_sum(ss, red)) / sqrtf((float)n);
    const float den = fmaxf(1.0f, urms / a.clip_threshold);
    const float decay = -(a.weight_decay * lr);
    float* m = a.use_beta1 ? a.m + t.m : nullptr;

    // sweep 3: the update again, clipped by its RMS, times lr; first moment; decay; parameters.  Every element is read and written
    // by the thread that owned it in sweep 2.
    if (t.factored) {
      const float* row = a.row + t.row;
      const float* col = a.col + t.col;
      for (int r0 = 0; r0 < R; r0 += GY) {
        const int r = r0 + gy;
        if (r < R) {
          const float rf = 1.0f / sqrtf(row[r] / rmean);
          const int64_t base = (int64_t)r * C;
          for (int c = tx; c < C; c += TX) {
            float u = (rf * (1.0f / sqrtf(col[c]))) * (g[base + c] * clip);
            u = (u / den) * lr;
            if (m != nullptr) {
              u = a.beta1 * m[base + c] + a.one_minus_beta1 * u;
              m[base + c] = u;
            }
            float pi = p[base + c];
            if (a.weight_decay != 0.f) pi += pi * decay;
            p[base + c] = pi - u;
          }
        }
      }
    } else {
      const float* v = a.v + t.v;
      for (int i = tid; i < n; i += NT) {
        float u = (1.0f / sqrtf(v[i])) * (g[i] * clip);
        u = (u / den) * lr;
        if (m != nullptr) {
          u = a.beta1 * m[i] + a.one_minus_beta1 * u;
          m[i] = u;
        }
        float pi = p[i];
        if (a.weight_decay != 0.f) pi += pi * decay;
        p[i] = pi - u;
      }
    }
  }
}

}  // namespace

extern "C" int qfx_adafactor_step(const qfx_adafactor_args* a, void* stream) {
  if (!a || a->n_tensors < 0) return QFX_EINVAL;
  if (a->n_tensors == 0) return QFX_OK;
  if (!a->table || !a->p || !a->g || !a->row || !a->col || !a->v || !a->rms) return QFX_EINVAL;
  if (a->use_beta1 && (!a->m || !(a->beta1 >= 0.f && a->beta1 < 1.f))) return QFX_EINVAL;
  if (!(a->lr >= 0.f) || !(a->beta2t >= 0.f && a->beta2t < 1.f) || !(a->one_minus_beta2t > 0.f && a->one_minus_beta2t <= 1.f))
    return QFX_EINVAL;
  if (!(a->eps1 >= 0.f) || !(a->eps2 >= 0.f) || !(a->clip_threshold > 0.f) || !(a->weight_decay >= 0.f)) return QFX_EINVAL;
  const int wgs = a->n_tensors < 2048 ? a->n_tensors : 2048;
  hipLaunchKernelGGL(adafactor_kernel, dim3((unsigned)wgs), dim3(NT), 0, (hipStream_t)stream, *a);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
