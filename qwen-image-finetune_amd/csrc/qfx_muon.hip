// qfx_muon.hip -- Muon (torch.optim.Muon) over the flat LoRA buffers: ONE launch, one workgroup per adapter matrix, driven by a device
// table of per-matrix descriptors (include/qfx.h).  The step is per matrix: momentum, then ns_steps Newton-Schulz iterations on the
// bf16 image X [s, n] of the update (s = the short side, at most 96 for an adapter), then the parameters.  Every product of the
// iteration has bf16 operands and an fp32 accumulator (v_mfma_f32_16x16x32_bf16) and is rounded to bf16 once, where torch rounds:
//   G = X X^T   [s, s]   K = n: split over the four waves in 32-column chunks, the four partial tiles folded through LDS in wave order
//   H = b G + c G G      both in LDS, one wave per output tile
//   X = a X + H X        one wave per 16-column strip of X, in place (a strip depends on no other strip)
// X lives in LDS when its padded image (s up to a multiple of 16, n up to a multiple of 32, zero filled) takes at most 96 KB -- the
// headline [16, 3072] exactly -- and in the caller's workspace slot of this workgroup otherwise (L2-resident between the sweeps).
// No atomics, nothing crosses a workgroup, every sum runs in an order fixed by the shape: same inputs -> same bits.
// Built with -ffp-contract=off: g' = g * clip, the products of H and the a X term are rounded where they are written; the fused
// operations torch has (lerp, the parameter update) are explicit fmaf calls.
#include "qfx_common.h"

namespace {

constexpr int NT = 256;                    // four waves
constexpr int NW = NT / 64;
constexpr int SMAX = 96;                   // largest short side
constexpr int TMAX = SMAX / 16;            // 16-row tiles of G / H
constexpr int LDG = SMAX + 8;              // row stride of G / H in LDS: 208 B, a multiple of 16 B, off the 256-B bank period
constexpr int X_LDS_ELEMS = 16 * 3072;     // 96 KB of bf16
constexpr int MAX_WGS = 256;               // one per CU: a workgroup holds 137 KB of LDS, so no two share a CU anyway

__host__ __device__ inline int pad_to(int v, int m) { return (v + m - 1) / m * m; }

// sum over the 256 threads, the same bits on every thread.  `red` may still be read by the previous call: barrier first.
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// torch.lerp as ATen's vectorised CPU kernel evaluates it: one FMA on the nearer end.
__device__ __forceinline__ float lerp_f(float start, float end, float w) {
  const float diff = end - start;
  return w < 0.5f ? __builtin_fmaf(w, diff, start) : __builtin_fmaf(w - 1.0f, diff, end);
}

__device__ __forceinline__ bf16x8 zero8() { return (bf16x8){0, 0, 0, 0, 0, 0, 0, 0}; }

// eight bf16 down a column: element j = base[j * stride] (the B operand when the summed index is the row index of the source)
__device__ __forceinline__ bf16x8 load_col8(const bf16_t* base, int stride) {
  bf16x8 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (short)base[(int64_t)j * stride];
  return f;
}

__global__ __launch_bounds__(256) void muon_kernel(const qfx_muon_args a, const int64_t ws_slot) {
  __shared__ __attribute__((aligned(16))) bf16_t Xs[X_LDS_ELEMS];
  __shared__ __attribute__((aligned(16))) bf16_t Gs[SMAX * LDG];
  __shared__ __attribute__((aligned(16))) float Us[NW * TMAX * 256];    // the Gram partials of one tile row; then H
  __shared__ float red[4];
  bf16_t* Hs = reinterpret_cast<bf16_t*>(Us);                           // SMAX * LDG * 2 B = 19968 <= 24576
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lhi = lane >> 4;
  float clip = a.grad_scale;
  if (a.gnorm_sq != nullptr && a.max_norm > 0.f) {      // = opt_clip (qfx_optim.h), written out: inlined, it compiles to other code here
    const float nrm = sqrtf(*a.gnorm_sq) * a.grad_scale;
    const float c = a.max_norm / (nrm + 1e-6f);
    clip *= c < 1.0f ? c : 1.0f;
  }
  const float mu = a.momentum, omm = a.one_minus_momentum;
  const float decay = 1.0f - a.lr * a.weight_decay;
  const float eps_b = rbf(a.eps);

  for (int ti = blockIdx.x; ti < a.n_tensors; ti += gridDim.x) {
    const qfx_muon_tensor t = a.table[ti];
    const int R = t.rows, C = t.cols;
    if (R <= 0 || C <= 0) continue;
    const bool tr = R > C;                    // X = u^T: the short side indexes the rows of X
    const int s = tr ? C : R, n = tr ? R : C;
    const int sp = pad_to(s, 16), np = pad_to(n, 32), T = sp >> 4;
    const int64_t xe = (int64_t)sp * np;
    if (s > SMAX || (int64_t)R * C > (1 << 30)) continue;
    const bool in_lds = xe <= X_LDS_ELEMS;
    if (!in_lds && xe > ws_slot) continue;    // never past the slot (the builders size it: qfx_muon_ws_bytes)
    bf16_t* X = in_lds ? Xs : a.ws + (int64_t)blockIdx.x * ws_slot;
    const int nel = R * C;
    float* p = a.p + t.off;
    const float* g = a.g + t.off;
    float* buf = a.buf + t.off;

    // sweep 0: is every clipped gradient finite?  Nothing has been written yet: a matrix with a non-finite gradient is left.  X's
    // image is zeroed on the way (the pad rows and columns must be zeros).
    int bad = 0;
    for (int i = tid; i < nel; i += NT) bad |= !__builtin_isfinite(g[i] * clip);
    __syncthreads();                           // the previous matrix's last sweep has read X
    for (int64_t i = (int64_t)tid * 8; i < xe; i += NT * 8) *reinterpret_cast<u32x4*>(X + i) = (u32x4){0u, 0u, 0u, 0u};
    if (__syncthreads_or(bad)) continue;       // the same verdict on every thread

    // sweep 1: momentum, the update u, X = bf16(u), the sum of X^2
    float ss = 0.f;
    for (int i = tid; i < nel; i += NT) {
      const float gi = g[i] * clip;
      const float b = lerp_f(buf[i], gi, omm);
      buf[i] = b;
      const float u = a.nesterov ? lerp_f(gi, b, mu) : b;
      const bf16_t xb = f2bf(u);
      const float xf = bf2f(xb);
      ss += xf * xf;
      const int r = (int)((unsigned)i / (unsigned)C), c = i - r * C;
      X[tr ? (int64_t)c * np + r : (int64_t)r * np + c] = xb;
    }
    const float nrm = rbf(sqrtf(block_sum(ss, red)));        // block_sum's barriers also publish X
    const float den = fmaxf(nrm, eps_b);
    for (int64_t i = tid; i < xe; i += NT) X[i] = f2bf(bf2f(X[i]) / den);
    __syncthreads();

    for (int it = 0; it < a.ns_steps; ++it) {
      // G = bf16(X X^T), one 16-row strip of tiles at a time
      for (int gi = 0; gi < T; ++gi) {
        f32x4 acc[TMAX];
#pragma unroll
        for (int gj = 0; gj < TMAX; ++gj) acc[gj] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int k0 = wave * 32; k0 < np; k0 += NW * 32) {
          const int64_t ko = k0 + 8 * lhi;
          const bf16x8 fa = *reinterpret_cast<const bf16x8*>(X + (int64_t)(gi * 16 + l15) * np + ko);
#pragma unroll
          for (int gj = 0; gj < TMAX; ++gj)
            if (gj < T) {
              const bf16x8 fb = *reinterpret_cast<const bf16x8*>(X + (int64_t)(gj * 16 + l15) * np + ko);
              acc[gj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc[gj], 0, 0, 0);
            }
        }
        __syncthreads();                         // Us: the previous strip's fold (or the previous iteration's H) has been read
#pragma unroll
        for (int gj = 0; gj < TMAX; ++gj)
          if (gj < T) {
#pragma unroll
            for (int r = 0; r < 4; ++r) Us[((wave * TMAX + gj) * 4 + r) * 64 + lane] = acc[gj][r];
          }
        __syncthreads();
        {
          const int r = tid >> 6;                // thread tid folds element (r, lane) of every tile: the address it had as a writer
          for (int gj = 0; gj < T; ++gj) {
            const float* q = Us + gj * 256 + tid;
            const float v = (q[0] + q[TMAX * 256]) + (q[2 * TMAX * 256] + q[3 * TMAX * 256]);
            Gs[(gi * 16 + lhi * 4 + r) * LDG + gj * 16 + l15] = f2bf(v);
          }
        }
      }
      __syncthreads();                           // G complete; Us free

      // H = bf16(b G + c G G), tile (hi, hj) on wave (hi T + hj) % 4
      for (int tt = wave; tt < T * T; tt += NW) {
        const int hi = tt / T, hj = tt - hi * T;
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < sp; k0 += 32) {
          const int k = k0 + 8 * lhi;            // a fragment lies wholly inside or wholly outside the sp rows (sp % 16 == 0)
          bf16x8 fa = zero8(), fb = zero8();
          if (k < sp) {
            fa = *reinterpret_cast<const bf16x8*>(Gs + (hi * 16 + l15) * LDG + k);
            fb = load_col8(Gs + k * LDG + hj * 16 + l15, LDG);
          }
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = (hi * 16 + lhi * 4 + r) * LDG + hj * 16 + l15;
          Hs[o] = f2bf(a.b * bf2f(Gs[o]) + a.c * acc[r]);
        }
      }
      __syncthreads();

      // X = bf16(a X + H X), 16 columns per wave pass.  Every element of the strip is read (as the B operand, all rows) before the
      // MFMAs whose results are stored, and the a X term is read by the lane that stores it.
      for (int c0 = wave * 16; c0 < np; c0 += NW * 16) {
        bf16x8 fb[SMAX / 32];
#pragma unroll
        for (int ks = 0; ks < SMAX / 32; ++ks) {
          const int k = ks * 32 + 8 * lhi;
          fb[ks] = k < sp ? load_col8(X + (int64_t)k * np + c0 + l15, np) : zero8();
        }
        for (int xi = 0; xi < T; ++xi) {
          f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < SMAX / 32; ++ks) {
            const int k = ks * 32 + 8 * lhi;
            if (ks * 32 < sp) {
              const bf16x8 fa = k < sp ? *reinterpret_cast<const bf16x8*>(Hs + (xi * 16 + l15) * LDG + k) : zero8();
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb[ks], acc, 0, 0, 0);
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            bf16_t* x = X + (int64_t)(xi * 16 + lhi * 4 + r) * np + c0 + l15;
            *x = f2bf(a.a * bf2f(*x) + acc[r]);
          }
        }
      }
      __syncthreads();
    }

    // the parameters: decoupled decay, then minus the adjusted learning rate times O = X (transposed back)
    const float alr = a.lr * t.lr_ratio;
    for (int i = tid; i < nel; i += NT) {
      const int r = (int)((unsigned)i / (unsigned)C), c = i - r * C;
      const float o = bf2f(X[tr ? (int64_t)c * np + r : (int64_t)r * np + c]);
      p[i] = __builtin_fmaf(-alr, o, p[i] * decay);
    }
  }
}

int64_t slot_elems(const qfx_muon_tensor* t, int32_t n) {
  int64_t slot = 0;
  for (int32_t i = 0; i < n; ++i) {
    const int R = t[i].rows, C = t[i].cols;
    if (R <= 0 || C <= 0 || t[i].off < 0 || (R < C ? R : C) > SMAX || (int64_t)R * C > (1 << 30)) return -1;
    const int64_t xe = (int64_t)pad_to(R < C ? R : C, 16) * pad_to(R < C ? C : R, 32);
    if (xe > X_LDS_ELEMS && xe > slot) slot = xe;
  }
  return slot;
}

}  // namespace

extern "C" int64_t qfx_muon_ws_bytes(const qfx_muon_tensor* host_table, int32_t n_tensors) {
  if (n_tensors < 0 || (n_tensors > 0 && !host_table)) return QFX_EINVAL;
  const int64_t slot = slot_elems(host_table, n_tensors);
  if (slot < 0) return QFX_EINVAL;
  return slot * 2 * (n_tensors < MAX_WGS ? n_tensors : MAX_WGS);
}

extern "C" int qfx_muon_step(const qfx_muon_args* a, void* stream) {
  if (!a || a->n_tensors < 0) return QFX_EINVAL;
  if (a->n_tensors == 0) return QFX_OK;
  if (!a->table || !a->p || !a->g || !a->buf || a->ws_bytes < 0 || (a->ws_bytes > 0 && !a->ws)) return QFX_EINVAL;
  if (((uintptr_t)a->ws & 15) != 0) return QFX_EINVAL;
  if (!(a->lr >= 0.f) || !(a->weight_decay >= 0.f) || !(a->momentum >= 0.f) || !(a->eps > 0.f)) return QFX_EINVAL;
  if (!(a->one_minus_momentum == a->one_minus_momentum)) return QFX_EINVAL;
  if (a->ns_steps < 0 || a->ns_steps >= 100) return QFX_EINVAL;
  const int wgs = a->n_tensors < MAX_WGS ? a->n_tensors : MAX_WGS;
  const int64_t ws_slot = (a->ws_bytes / 2 / wgs) & ~(int64_t)7;     // slots stay 16-byte aligned
  hipLaunchKernelGGL(muon_kernel, dim3((unsigned)wgs), dim3(NT), 0, (hipStream_t)stream, *a, ws_slot);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
