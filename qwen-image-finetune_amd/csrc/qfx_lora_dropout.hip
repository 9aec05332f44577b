// qfx_lora_dropout.hip -- kohya's network_dropout / rank_dropout on the rank-r activation of the adapters (include/qfx.h): the
// outputs of a rank-r producer (the transposed hi / lo split Ut[R][M] and the K-extension image ext[M][...]) are multiplied in
// place by the factor f[token, rank] that a counter-based generator yields, the same in the forward and the backward pass.
// Bandwidth-trivial (M x R x 10 bytes); what matters is that both sides stay coalesced: m is the fast index of Ut, j of ext.  A
// block owns 64 rows: lane = row for the Ut side (128-byte runs per wave and rank), the re-split values cross through LDS, and the
// ext side writes 8-byte pieces with consecutive lanes on consecutive pieces of a row.
#include "qfx_common.h"

namespace {

// Philox4x32-10 (Salmon et al., Random123): 10 rounds, the key bumped by the Weyl constants between rounds.
__host__ __device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
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

struct DropState { uint32_t seed_lo, seed_hi, step, active, thr_elem, thr_rank, scale_bits, sample0; };

__host__ __device__ inline float bits_float(uint32_t u) {
  union { uint32_t u; float f; } v;
  v.u = u;
  return v.f;
}

// The factors of ranks 4q .. 4q+3 of adapter `site` for token t of global sample `sample`: THE definition of the mask (qfx.h),
// called by the kernel and by qfx_lora_dropout_factors_host.
__host__ __device__ inline void dropout_quad(const DropState& s, uint32_t site, uint32_t sample, uint32_t t, uint32_t q, float f[4]) {
  const float scale = bits_float(s.scale_bits);
  bool keep[4] = {true, true, true, true};
  uint32_t w[4];
  if (s.thr_elem) {
    philox4x32_10(t * 32u + q, sample, s.step, site, s.seed_lo, s.seed_hi, w);
#pragma unroll
    for (int i = 0; i < 4; ++i) keep[i] = w[i] >= s.thr_elem;
  }
  if (s.thr_rank) {
    philox4x32_10(0xFFFFFFE0u + q, sample, s.step, site, s.seed_lo, s.seed_hi, w);
#pragma unroll
    for (int i = 0; i < 4; ++i) keep[i] = keep[i] && w[i] >= s.thr_rank;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) f[i] = keep[i] ? scale : 0.f;
}

#define QFX_AS4 __attribute__((address_space(4)))
constexpr int TM = 64;        // rows per block
constexpr int MAX_R = 96;     // what qfx_lora_down produces
struct DropBatch { qfx_lora_dropout_args a[QFX_MAX_BATCH]; int start[QFX_MAX_BATCH + 1]; int n; const uint32_t* state; };

__global__ __launch_bounds__(256) void lora_dropout_kernel(const DropBatch batch_by_value) {
  // (the argument block is read from the kernarg segment, as in qfx_skinny.hip: indexing the by-value copy would go through scratch)
  const QFX_AS4 DropBatch& kb = *(const QFX_AS4 DropBatch*)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t* sp = kb.state;
  DropState s;
  s.seed_lo = sp[0]; s.seed_hi = sp[1]; s.step = sp[2]; s.active = sp[3];
  s.thr_elem = sp[4]; s.thr_rank = sp[5]; s.scale_bits = sp[6]; s.sample0 = sp[7];
  if (s.active == 0 || (s.thr_elem == 0 && s.thr_rank == 0)) return;      // uniform over the grid
  __shared__ uint32_t tile[TM][MAX_R + 1];      // hi | lo << 16 of the re-split u'; odd row stride: lane = row writes without conflicts
  int pi = 0;
#pragma unroll
  for (int i = 1; i < QFX_MAX_BATCH; ++i)
    if (i < kb.n && (int)blockIdx.x >= kb.start[i]) pi = i;
  const QFX_AS4 qfx_lora_dropout_args& p = kb.a[pi];
  const int tid = threadIdx.x, ml = tid & 63, wv = tid >> 6;
  const int M = p.M, R = p.R, gR = p.group_R;
  const int m0 = ((int)blockIdx.x - kb.start[pi]) * TM;
  const int m = m0 + ml;
  if (m < M) {
    const uint32_t b = (uint32_t)(m / p.rows_per_batch), t = (uint32_t)(m % p.rows_per_batch);
    for (int q = wv; q < R / 4; q += 4) {      // quads of ranks: group_R % 4 == 0, a quad lies within one adapter
      const int j0 = 4 * q, g = j0 / gR;
      float f[4];
      dropout_quad(s, p.site[g], s.sample0 + b, t, (uint32_t)((j0 - g * gR) >> 2), f);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t at = (int64_t)(j0 + i) * p.ld_ut + m;
        const float u = bf2f(p.Ut_hi[at]) + bf2f(p.Ut_lo[at]);
        const float v = f[i] == 0.f ? 0.f : u * f[i];      // a dropped element is +0 whatever the sign of u
        const bf16_t hi = f2bf(v);
        const bf16_t lo = f2bf(v - bf2f(hi));
        p.Ut_hi[at] = hi;
        p.Ut_lo[at] = lo;
        tile[ml][j0 + i] = (uint32_t)hi | ((uint32_t)lo << 16);
      }
    }
  }
  if (p.ext == nullptr) return;      // block-uniform
  __syncthreads();
  // ext row m, per group g: [hi (gR) | lo (gR) | hi (gR)] at column g * group_stride; 8-byte pieces of 4 ranks
  const int cpg = 3 * gR / 4, cpr = (R / gR) * cpg;      // pieces per group / per row
  const int rows = M - m0 < TM ? M - m0 : TM;
  for (int e = tid; e < rows * cpr; e += 256) {
    const int row = e / cpr, c = e - row * cpr;
    const int g = c / cpg, cc = (c - g * cpg) * 4;
    const int seg = cc / gR, jl = cc - seg * gR;
    const uint32_t* src = &tile[row][g * gR + jl];
    const int sh = seg == 1 ? 16 : 0;
    u32x2 o;
    o.x = ((src[0] >> sh) & 0xFFFFu) | (((src[1] >> sh) & 0xFFFFu) << 16);
    o.y = ((src[2] >> sh) & 0xFFFFu) | (((src[3] >> sh) & 0xFFFFu) << 16);
    *(u32x2*)(p.ext + (int64_t)(m0 + row) * p.ld_ext + (int64_t)g * p.group_stride + seg * gR + jl) = o;
  }
}

__global__ void lora_dropout_advance_kernel(uint32_t* state) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && state[3] != 0) state[2] += 1u;
}

int check_problem(const qfx_lora_dropout_args& a) {
  if (a.M <= 0 || a.R <= 0 || (a.R % 16) || a.R > MAX_R) return QFX_EINVAL;
  if (a.group_R <= 0 || (a.group_R % 16) || (a.R % a.group_R) || a.group_R > 128 || a.R / a.group_R > 3) return QFX_EINVAL;
  if (a.rows_per_batch <= 0 || a.rows_per_batch >= (1 << 27) - 1) return QFX_EINVAL;
  if (!a.Ut_hi || !a.Ut_lo || a.ld_ut < a.M) return QFX_EINVAL;
  if (a.ext) {
    if (((uintptr_t)a.ext % 8) || (a.ld_ext % 4) || (a.group_stride % 4) || a.group_stride < 0) return QFX_EINVAL;
    if (a.ld_ext < (int64_t)(a.R / a.group_R - 1) * a.group_stride + 3 * a.group_R) return QFX_EINVAL;
  }
  return QFX_OK;
}

}  // namespace

extern "C" int qfx_lora_dropout_apply(const qfx_lora_dropout_args* list, int32_t n, const uint32_t* state, void* stream) {
  if (!list || !state || n <= 0 || n > QFX_MAX_BATCH) return QFX_EINVAL;
  DropBatch b;
  int blocks = 0;
  for (int i = 0; i < n; ++i) {
    const int rc = check_problem(list[i]);
    if (rc) return rc;
    b.a[i] = list[i];
    b.start[i] = blocks;
    blocks += (list[i].M + TM - 1) / TM;
  }
  for (int i = n; i <= QFX_MAX_BATCH; ++i) b.start[i] = blocks;
  for (int i = n; i < QFX_MAX_BATCH; ++i) b.a[i] = list[0];
  b.n = n;
  b.state = state;
  hipLaunchKernelGGL(lora_dropout_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, b);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_lora_dropout_advance(uint32_t* state, void* stream) {
  if (!state) return QFX_EINVAL;
  hipLaunchKernelGGL(lora_dropout_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_lora_dropout_factors_host(const uint32_t* state, uint32_t site, int32_t b, int32_t t, int32_t r, float* out) {
  if (!state || !out || b < 0 || t < 0 || t >= (1 << 27) - 1 || r <= 0 || r > 128) return QFX_EINVAL;
  DropState s;
  s.seed_lo = state[0]; s.seed_hi = state[1]; s.step = state[2]; s.active = state[3];
  s.thr_elem = state[4]; s.thr_rank = state[5]; s.scale_bits = state[6]; s.sample0 = state[7];
  for (int q = 0; 4 * q < r; ++q) {
    float f[4];
    dropout_quad(s, site, s.sample0 + (uint32_t)b, (uint32_t)t, (uint32_t)q, f);
    for (int i = 0; i < 4 && 4 * q + i < r; ++i) out[4 * q + i] = f[i];
  }
  return QFX_OK;
}
