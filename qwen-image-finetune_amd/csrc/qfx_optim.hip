// qfx_optim.hip -- the fp32-state optimizers over the flat LoRA buffers and the gradient norm that feeds their clip, see
// include/qfx.h: the squared-sum kernels (atomic and deterministic form), AdamW and SGD (each with its parameter-group form) and
// Prodigy.  Built with the compiler's default contraction: the products and sums of these kernels fuse where the compiler chooses,
// the clip prologue's included -- except in adamw_elem / sgd_elem, which two kernels each must round alike and which pin them.
#include "qfx_common.h"
#include "qfx_optim.h"
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

namespace {

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ out) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) acc += g[i] * g[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) unsafeAtomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

// Deterministic form: per-block partial sums in a fixed slot each, folded by ONE block in a fixed order.  Data-parallel replicas
// hold bit-identical gradients after the all-reduce; with the atomic form above the clip coefficient differed in its last bits
// from rank to rank (fp32 atomics commute only approximately) and the replicas drifted apart by ~1e-10 per step.
__global__ __launch_bounds__(256) void sumsq_part_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) acc += g[i] * g[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void sumsq_fold_kernel(const float* __restrict__ part, int nb, float* __restrict__ out) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) acc += part[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one AdamW element (torch.optim.AdamW): the ONE statement of the arithmetic, called by adamw_kernel and adamw_grouped_kernel.
// step = lr / bias_corr1 and rs2 = 1 / sqrt(bias_corr2) are formed once per launch (per group); 1 - b1, 1 - b2 and 1 - lr wd here.
// Which products fuse with their sums is written out (contraction off inside, explicit fmaf): these are the fusions the default
// contraction chose for adamw_kernel when it held this arithmetic inline, and left to the compiler they moved with the code
// around them (the operand order of the first moment's FMA changed when the loads were reordered) -- pinned, the ungrouped step
// keeps its bits and the grouped step rounds like it.
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float clip, float lr, float b1, float b2, float eps,
                                           float wd, float step, float rs2) {
#pragma clang fp contract(off)
  const float gi = g * clip;
  const float pi = p * fmaf(-lr, wd, 1.0f);
  const float mi = fmaf(1.0f - b1, gi, b1 * m);
  const float vi = b2 * v + ((1.0f - b2) * gi) * gi;
  p = pi - (step * mi) / fmaf(rs2, sqrtf(vi), eps);
  m = mi; v = vi;
}

__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps,
                                                    float wd, float bc1, float bc2, const float* __restrict__ gnorm_sq,
                                                    float max_norm, float grad_scale) {
  const float clip = opt_clip(gnorm_sq, max_norm, grad_scale);
  const float step = lr / bc1;
  const float rs2 = 1.0f / sqrtf(bc2);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float pi = p[i], mi = m[i], vi = v[i];
    adamw_elem(pi, g[i], mi, vi, clip, lr, b1, b2, eps, wd, step, rs2);
    p[i] = pi; m[i] = mi; v[i] = vi;
  }
}

// ---- parameter groups: the same element function, its scalars read per 64-element tile from the group's row in LDS.
// VEC: p, g, m, v are 16-byte aligned -> one dwordx4 per buffer and lane (a quad never leaves its tile: tiles start at multiples
// of 64); the n % 4 tail (and everything, without VEC) is scalar.
struct AdamWRow { float lr, b1, b2, eps, wd, step, rs2, pad; };

template <bool VEC>
__global__ __launch_bounds__(256) void adamw_grouped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, int64_t n, const uint8_t* __restrict__ tile_group,
                                                            const GroupTable<qfx_adamw_group> tab, int n_groups,
                                                            const float* __restrict__ gnorm_sq, float max_norm, float grad_scale) {
  __shared__ AdamWRow rows[QFX_MAX_PARAM_GROUPS];
  if ((int)threadIdx.x < n_groups) {
    const qfx_adamw_group q = tab.g[threadIdx.x];
    AdamWRow r;
    r.lr = q.lr; r.b1 = q.beta1; r.b2 = q.beta2; r.eps = q.eps; r.wd = q.weight_decay;
    r.step = q.lr / q.bias_corr1;
    r.rs2 = 1.0f / sqrtf(q.bias_corr2);
    r.pad = 0.f;
    rows[threadIdx.x] = r;
  }
  const float clip = opt_clip(gnorm_sq, max_norm, grad_scale);
  __syncthreads();
  flat_sweep<VEC>(n, [&](int64_t i, int64_t tile, auto w) {
    constexpr int W = decltype(w)::value;
    const AdamWRow r = rows[group_index(tile_group, tile, n_groups)];
    float pv[W], gv[W], mv[W], vv[W];
    flat_load(p + i, pv); flat_load(g + i, gv); flat_load(m + i, mv); flat_load(v + i, vv);
#pragma unroll
    for (int j = 0; j < W; ++j) adamw_elem(pv[j], gv[j], mv[j], vv[j], clip, r.lr, r.b1, r.b2, r.eps, r.wd, r.step, r.rs2);
    flat_store(p + i, pv); flat_store(m + i, mv); flat_store(v + i, vv);
  });
}

// torch.optim.SGD over the flat LoRA buffers after the clip prologue (include/qfx.h).  buf is never touched when mom == 0.
// one SGD element, called by sgd_kernel and sgd_grouped_kernel.  b: the element's momentum buffer value (read by the caller only
// when it exists and is not created by this step; written back by the caller when mom != 0); keep = 1 - dampening.  The fusions
// are pinned as in adamw_elem: the decayed gradient and the buffer update round every product, the Nesterov sum and the
// parameter update are one FMA each.
__device__ __forceinline__ void sgd_elem(float& p, float g, float& b, float clip, float lr, float mom, float keep, float wd, int nesterov,
                                         int first) {
#pragma clang fp contract(off)
  const float pi = p;
  float gi = g * clip;
  if (wd != 0.f) gi = wd * pi + gi;
  if (mom != 0.f) {
    const float bi = first ? gi : keep * gi + mom * b;
    b = bi;
    gi = nesterov ? fmaf(mom, bi, gi) : bi;
  }
  p = fmaf(-lr, gi, pi);
}

__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                  int64_t n, float lr, float mom, float damp, float wd, int nesterov, int first,
                                                  const float* __restrict__ gnorm_sq, float max_norm, float grad_scale) {
  const float clip = opt_clip(gnorm_sq, max_norm, grad_scale);
  const float keep = 1.0f - damp;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float pi = p[i], bi = 0.f;
    if (mom != 0.f && !first) bi = buf[i];
    sgd_elem(pi, g[i], bi, clip, lr, mom, keep, wd, nesterov, first);
    if (mom != 0.f) buf[i] = bi;
    p[i] = pi;
  }
}

// parameter groups: a group with momentum == 0 neither reads nor writes its part of buf
struct SgdRow { float lr, mom, keep, wd; int nesterov, pad0, pad1, pad2; };

template <bool VEC>
__global__ __launch_bounds__(256) void sgd_grouped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                          int64_t n, const uint8_t* __restrict__ tile_group,
                                                          const GroupTable<qfx_sgd_group> tab, int n_groups, int first,
                                                          const float* __restrict__ gnorm_sq, float max_norm, float grad_scale) {
  __shared__ SgdRow rows[QFX_MAX_PARAM_GROUPS];
  if ((int)threadIdx.x < n_groups) {
    const qfx_sgd_group q = tab.g[threadIdx.x];
    SgdRow r;
    r.lr = q.lr; r.mom = q.momentum; r.keep = 1.0f - q.dampening; r.wd = q.weight_decay; r.nesterov = q.nesterov;
    r.pad0 = r.pad1 = r.pad2 = 0;
    rows[threadIdx.x] = r;
  }
  const float clip = opt_clip(gnorm_sq, max_norm, grad_scale);
  __syncthreads();
  flat_sweep<VEC>(n, [&](int64_t i, int64_t tile, auto w) {
    constexpr int W = decltype(w)::value;
    const SgdRow r = rows[group_index(tile_group, tile, n_groups)];
    float pv[W], gv[W], bv[W] = {};
    flat_load(p + i, pv); flat_load(g + i, gv);
    if (r.mom != 0.f && !first) flat_load(buf + i, bv);
#pragma unroll
    for (int j = 0; j < W; ++j) sgd_elem(pv[j], gv[j], bv[j], clip, r.lr, r.mom, r.keep, r.wd, r.nesterov, first);
    if (r.mom != 0.f) flat_store(buf + i, bv);
    flat_store(p + i, pv);
  });
}

// ---- Prodigy (prodigyopt 1.x, Adam variant) over the flat LoRA buffers: see include/qfx.h.  Host scalars of the package (Python
// float64: d, d_max, d_numerator, d_denom, k) live in a device double[QFX_PRODIGY_STATE] so the step never synchronises.
enum { PS_D = 0, PS_DMAX, PS_NUM, PS_DEN, PS_DHAT, PS_K, PS_ACC_NUM, PS_ACC_DEN, PS_DLR, PS_SKIP };

__global__ void prodigy_begin_kernel(double* __restrict__ st, double lr, double b1, double b2, int use_bc) {
  const double k = st[PS_K];
  const double bc = use_bc ? sqrt(1.0 - pow(b2, k + 1.0)) / (1.0 - pow(b1, k + 1.0)) : 1.0;
  st[PS_DLR] = st[PS_D] * lr * bc;
  st[PS_ACC_NUM] = 0.0;
  st[PS_ACC_DEN] = 0.0;
  st[PS_SKIP] = 0.0;
}

__global__ __launch_bounds__(256) void prodigy_ema_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, float* __restrict__ sv, const float* __restrict__ p0,
                                                          int64_t n, double* __restrict__ st, float b1, float b2, float b3, double d0,
                                                          int safeguard, const float* __restrict__ gnorm_sq, float max_norm,
                                                          float grad_scale) {
  __shared__ float red[8];
  const float clip = opt_clip(gnorm_sq, max_norm, grad_scale);
  const double d = st[PS_D], dlr = st[PS_DLR];
  const float am = (float)(d * (1.0 - (double)b1)), av = (float)(d * d * (1.0 - (double)b2));
  const float as = (float)(safeguard ? (d / d0) * d : (d / d0) * dlr);
  float num = 0.f, den = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float gi = g[i] * clip;
    num += gi * (p0[i] - p[i]);
    m[i] = m[i] * b1 + gi * am;
    v[i] = v[i] * b2 + (av * gi) * gi;
    const float si = sv[i] * b3 + gi * as;
    sv[i] = si;
    den += fabsf(si);
  }
  num = wave_sum(num); den = wave_sum(den);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = num; red[4 + (threadIdx.x >> 6)] = den; }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(&st[PS_ACC_NUM], (double)red[0] + (double)red[1] + (double)red[2] + (double)red[3]);
    atomicAdd(&st[PS_ACC_DEN], (double)red[4] + (double)red[5] + (double)red[6] + (double)red[7]);
  }
}

__global__ void prodigy_d_kernel(double* __restrict__ st, double b3, double d0, double d_coef, double growth) {
  const double den = st[PS_ACC_DEN];
  if (den == 0.0) { st[PS_SKIP] = 1.0; return; }   // no progress: the package returns before storing anything
  double d = st[PS_D];
  const double num = st[PS_NUM] * b3 + (d / d0) * st[PS_DLR] * st[PS_ACC_NUM];
  const double d_hat = d_coef * num / den;
  // the package's `d == d0` (first jump not capped by growth): d0 reaches the step as the struct's float and the state as the double
  // qfx_prodigy_init_state was given, so 1e-6 and (float)1e-6 must compare equal -- in float, where both are one number
  if ((float)d == (float)d0) d = d > d_hat ? d : d_hat;
  double d_max = st[PS_DMAX];
  d_max = d_max > d_hat ? d_max : d_hat;
  const double dg = d * growth;
  d = d_max < dg ? d_max : dg;
  st[PS_NUM] = num; st[PS_DEN] = den; st[PS_D] = d; st[PS_DMAX] = d_max; st[PS_DHAT] = d_hat;
  st[PS_K] += 1.0;
}

__global__ __launch_bounds__(256) void prodigy_apply_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                            int64_t n, const double* __restrict__ st, float eps, float wd) {
  if (st[PS_SKIP] != 0.0) return;
  const double dlr = st[PS_DLR];
  const float deps = (float)(st[PS_D] * (double)eps);
  const float adec = (float)(-(double)wd * dlr), astep = (float)(-dlr);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float pi = p[i];
    if (wd != 0.f) pi = pi + pi * adec;
    p[i] = pi + astep * (m[i] / (sqrtf(v[i]) + deps));
  }
}
}  // namespace

extern "C" int qfx_sumsq(const float* g, int64_t n, float* out, void* stream) {
  if (!g || !out || n <= 0) return QFX_EINVAL;
  const int blocks = flat_grid(n, 2048);
  hipLaunchKernelGGL(sumsq_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, n, out);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_sumsq_det(const float* g, int64_t n, float* out, float* partials, int32_t nslots, void* stream) {
  if (!g || !out || !partials || n <= 0 || nslots <= 0) return QFX_EINVAL;
  const int blocks = flat_grid(n, nslots);
  hipLaunchKernelGGL(sumsq_part_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, n, partials);
  hipLaunchKernelGGL(sumsq_fold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, blocks, out);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                              float eps, float weight_decay, float bias_corr1, float bias_corr2, const float* gnorm_sq,
                              float max_norm, float grad_scale, void* stream) {
  if (!p || !g || !m || !v || n <= 0) return QFX_EINVAL;
  const int blocks = flat_grid(n, FLAT_STEP_CAP);
  hipLaunchKernelGGL(adamw_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1, beta2, eps,
                     weight_decay, bias_corr1, bias_corr2, gnorm_sq, max_norm, grad_scale);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_sgd_step(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float dampening,
                            float weight_decay, int32_t nesterov, int32_t first, const float* gnorm_sq, float max_norm,
                            float grad_scale, void* stream) {
  if (!p || !g || n <= 0) return QFX_EINVAL;
  if (!buf && momentum != 0.f) return QFX_EINVAL;
  if (nesterov && (!(momentum > 0.f) || dampening != 0.f)) return QFX_EINVAL;
  const int blocks = flat_grid(n, FLAT_STEP_CAP);
  hipLaunchKernelGGL(sgd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, g, buf, n, lr, momentum, dampening,
                     weight_decay, nesterov, first, gnorm_sq, max_norm, grad_scale);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int64_t qfx_grouped_sweep_elems(int32_t blocksize) {
  if (blocksize == 0) return FLAT_STEP_CAP * 256 * 4;      // the 16-byte form of the fp32 kernels: a quad per lane
  if (blocksize == 256) return BLOCKWISE_CAP * 4 * 256;    // a wave per table entry, four entries per workgroup
  if (blocksize == 2048) return BLOCKWISE_CAP * 2048;      // a workgroup per table entry
  return QFX_EINVAL;
}

extern "C" int qfx_adamw_step_grouped(float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* tile_group,
                                      const qfx_adamw_group* groups, int32_t n_groups, const float* gnorm_sq, float max_norm,
                                      float grad_scale, void* stream) {
  if (!p || !g || !m || !v || !tile_group || n <= 0 || !groups_count_ok(groups, n_groups)) return QFX_EINVAL;
  for (int i = 0; i < n_groups; ++i) {
    const qfx_adamw_group& q = groups[i];
    if (!(q.lr >= 0.f) || !beta_ok(q.beta1) || !beta_ok(q.beta2) || !(q.eps >= 0.f) || !(q.weight_decay >= 0.f)) return QFX_EINVAL;
    if (!(q.bias_corr1 > 0.f) || !(q.bias_corr2 > 0.f)) return QFX_EINVAL;
  }
  const FlatShape s = flat_launch_shape(n, FLAT_STEP_CAP, p, g, m, v);
  launch_either<adamw_grouped_kernel<true>, adamw_grouped_kernel<false>>(s.vec, s.blocks, stream, p, g, m, v, n, tile_group,
                                                                         group_table(groups, n_groups), n_groups, gnorm_sq, max_norm,
                                                                         grad_scale);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_sgd_step_grouped(float* p, const float* g, float* buf, int64_t n, const uint8_t* tile_group,
                                    const qfx_sgd_group* groups, int32_t n_groups, int32_t first, const float* gnorm_sq,
                                    float max_norm, float grad_scale, void* stream) {
  if (!p || !g || !tile_group || n <= 0 || !groups_count_ok(groups, n_groups)) return QFX_EINVAL;
  for (int i = 0; i < n_groups; ++i) {
    const qfx_sgd_group& q = groups[i];
    if (!(q.lr >= 0.f) || !(q.momentum >= 0.f) || !(q.weight_decay >= 0.f)) return QFX_EINVAL;
    if (!buf && q.momentum != 0.f) return QFX_EINVAL;
    if (q.nesterov && (!(q.momentum > 0.f) || q.dampening != 0.f)) return QFX_EINVAL;
  }
  const FlatShape s = flat_launch_shape(n, FLAT_STEP_CAP, p, g, buf);
  launch_either<sgd_grouped_kernel<true>, sgd_grouped_kernel<false>>(s.vec, s.blocks, stream, p, g, buf, n, tile_group,
                                                                     group_table(groups, n_groups), n_groups, first, gnorm_sq, max_norm,
                                                                     grad_scale);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}

extern "C" int qfx_prodigy_init_state(double* state, double d0, void* stream) {
  if (!state || !(d0 > 0.0)) return QFX_EINVAL;
  double h[QFX_PRODIGY_STATE] = {0};
  h[PS_D] = d0; h[PS_DMAX] = d0; h[PS_DHAT] = d0;
  if (hipMemcpyAsync(state, h, sizeof(h), hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) return QFX_EINVAL;
  return hipStreamSynchronize((hipStream_t)stream) == hipSuccess ? QFX_OK : QFX_EINVAL;   // h is a stack buffer
}

extern "C" int qfx_prodigy_step(const qfx_prodigy_args* a, void* stream) {
  if (!a || !a->p || !a->g || !a->exp_avg || !a->exp_avg_sq || !a->s || !a->p0 || !a->state || a->n <= 0) return QFX_EINVAL;
  if (!(a->beta1 > 0.f) || !(a->d0 > 0.f) || a->lr < 0.f) return QFX_EINVAL;
  if (a->weight_decay != 0.f && !a->decouple) return QFX_EUNSUPPORTED;   // coupled decay: not used by any reference config
  if (a->lr == 0.f) return QFX_OK;   // warm-up step 0: the package creates its state and returns; k does not advance
  hipStream_t s = (hipStream_t)stream;
  const double b3 = a->beta3 > 0.f ? (double)a->beta3 : sqrt((double)a->beta2);
  const int blocks = flat_grid(a->n, 2048);
  hipLaunchKernelGGL(prodigy_begin_kernel, dim3(1), dim3(1), 0, s, a->state, (double)a->lr, (double)a->beta1, (double)a->beta2,
                     a->use_bias_correction);
  hipLaunchKernelGGL(prodigy_ema_kernel, dim3(blocks), dim3(256), 0, s, a->p, a->g, a->exp_avg, a->exp_avg_sq, a->s, a->p0, a->n,
                     a->state, a->beta1, a->beta2, (float)b3, (double)a->d0, a->safeguard_warmup, a->gnorm_sq, a->max_norm,
                     a->grad_scale);
  hipLaunchKernelGGL(prodigy_d_kernel, dim3(1), dim3(1), 0, s, a->state, b3, (double)a->d0, (double)a->d_coef,
                     (double)a->growth_rate);
  hipLaunchKernelGGL(prodigy_apply_kernel, dim3(blocks), dim3(256), 0, s, a->p, a->exp_avg, a->exp_avg_sq, a->n, a->state, a->eps,
                     a->weight_decay);
  QFX_CHECK_LAUNCH();
  return QFX_OK;
}
