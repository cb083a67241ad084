// LAMB over the optimizer's flat slabs (C ABI: include/mmt_layer.h, mmt_lamb_step; DESIGN.md section 4, "LAMB"): AdamW's
// moments, then a trust ratio ||w|| / ||u|| per PARAMETER -- a segment of whole 1024-element chunks of the slab -- in
// front of the update.  lamb.h has the per-element update, the shape of every sum and the clamping of the segment
// table, which the kernels and mmt_lamb_step_host share.
//
//   launches of mmt_lamb_step, 256 threads, 16-byte accesses
//   1. moments  a workgroup per chunk (grid-stride beyond the grid): reads g m v w and wd[chunk], writes m v, writes the
//               update direction u OVER g (the gradient is dead from here on and is cleared at the end anyway), and
//               stores {sum w^2, sum u^2} of the chunk as one float2: wave fold, then the four wave sums through LDS
//   2. ratios   a workgroup per segment (grid-stride): adds the segment's chunk partials in the fixed order of lamb.h, in
//               double, and writes r = ||w|| / ||u|| (or 1) for every chunk of the segment
//   3. apply    a workgroup per chunk: w -= lr r u, the bf16 shadow, and the gradient slab cleared when zero_grad
//
// No atomics: the same inputs give the same bits on every run, and a parameter's ratio does not depend on what shares
// the slab with it.  Workspace (caller's): float2 partial[n / 1024], then float ratio[n / 1024].
//
// Bounds: lamb_segment_range() clamps every chunk index read from the device-resident segment table into
// [0, n / 1024]; chunk indices of launches 1 and 3 come from the grid-stride loops alone.  A wrong table gives wrong
// ratios, never a stray access.
#include "../../include/mmt_attn.h"
#include "../../include/mmt_layer.h"

#include <cstdint>

#include "lamb.h"
#include "mmt_err.h"

namespace mmt {
namespace {

struct LambParams {
  float* prm;
  float* grd;
  float* m1;
  float* m2;
  uint16_t* shadow;                    // bf16 bits, may be NULL
  const float* chunk_wd;
  const int32_t* segment_start;        // [n_segments + 1]
  const int32_t* segment_adapt;        // [n_segments]
  const float* grad_scale;             // may be NULL
  const float* hyper;                  // may be NULL
  float* partial;                      // [2 * n_chunks] in the workspace
  float* ratio;                        // [n_chunks] in the workspace
  long n_chunks, n_segments;
  LambHyper h;
  int zero_grad;
};

size_t lamb_workspace_bytes(int64_t n) { return (((size_t)(n >> kLambChunkLog) * 12) + 15) & ~(size_t)15; }

int check_lamb(const char* who, const mmt_lamb_desc* d, float* param, float* grad, float* exp_avg, float* exp_avg_sq, void* param_bf16,
               const float* chunk_wd, const int32_t* segment_start, const int32_t* segment_adapt, const float* grad_scale,
               void* workspace, size_t workspace_bytes, LambParams& p) {
  if (!d || !param || !grad || !exp_avg || !exp_avg_sq || !chunk_wd || !segment_start || !segment_adapt)
    return fail(MMT_E_INVALID, "%s: NULL argument (only param_bf16, grad_scale and the stream may be NULL)", who);
  if (d->n <= 0 || (d->n & (kLambChunk - 1))) return fail(MMT_E_INVALID, "%s: n must be a positive multiple of 1024", who);
  if (!(d->bias_correction1 > 0.f) || !(d->bias_correction2 > 0.f)) return fail(MMT_E_INVALID, "%s: bias corrections must be positive", who);
  if (d->n_segments < 1) return fail(MMT_E_INVALID, "%s: n_segments %d, at least one parameter segment is needed", who, d->n_segments);
  if ((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)workspace) & 15) != 0 || ((uintptr_t)param_bf16 & 7) != 0)
    return fail(MMT_E_INVALID, "%s: the fp32 slabs and the workspace must be 16-byte, the bf16 shadow 8-byte aligned", who);
  const size_t need = lamb_workspace_bytes(d->n);
  if (!workspace || workspace_bytes < need) return fail(MMT_E_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", who, need, workspace ? workspace_bytes : (size_t)0);
  p.prm = param; p.grd = grad; p.m1 = exp_avg; p.m2 = exp_avg_sq; p.shadow = (uint16_t*)param_bf16;
  p.chunk_wd = chunk_wd; p.segment_start = segment_start; p.segment_adapt = segment_adapt;
  p.grad_scale = grad_scale; p.hyper = d->hyper;
  p.n_chunks = (long)(d->n >> kLambChunkLog); p.n_segments = d->n_segments;
  p.partial = (float*)workspace; p.ratio = p.partial + 2 * p.n_chunks;
  p.h.beta1 = d->beta1; p.h.beta2 = d->beta2; p.h.eps = d->eps;
  lamb_step_scalars(p.h, d->lr, d->bias_correction1, d->bias_correction2);
  p.zero_grad = d->zero_grad;
  return MMT_OK;
}

#ifndef MMT_LAMB_HOST_ONLY
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

__device__ inline LambHyper lamb_hyper_dev(const LambParams& p) {
  LambHyper h = p.h;
  if (p.hyper) lamb_step_scalars(h, p.hyper[0], p.hyper[1], p.hyper[2]);     // device-resident {lr, bias corrections}
  return h;
}

__global__ __launch_bounds__(256) void lamb_moments_kernel(const LambParams p) {
  __shared__ float red[2][kLambThreads / 64];
  const int t = threadIdx.x;
  const LambHyper h = lamb_hyper_dev(p);
  const float gs = p.grad_scale ? *p.grad_scale : 1.f;
  for (long c = blockIdx.x; c < p.n_chunks; c += gridDim.x) {
    const long i = c * kLambChunk + t * 4;
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(p.prm + i), g4 = *reinterpret_cast<const f32x4*>(p.grd + i);
    f32x4 a4 = *reinterpret_cast<const f32x4*>(p.m1 + i), b4 = *reinterpret_cast<const f32x4*>(p.m2 + i);
    const float wd = p.chunk_wd[c];
    f32x4 u4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float mm = a4[j], vv = b4[j];
      u4[j] = lamb_direction(h, g4[j], gs, w4[j], wd, mm, vv);
      a4[j] = mm; b4[j] = vv;
    }
    *reinterpret_cast<f32x4*>(p.m1 + i) = a4;
    *reinterpret_cast<f32x4*>(p.m2 + i) = b4;
    *reinterpret_cast<f32x4*>(p.grd + i) = u4;
    float w2 = lamb_lane_sumsq(w4[0], w4[1], w4[2], w4[3]), u2 = lamb_lane_sumsq(u4[0], u4[1], u4[2], u4[3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      w2 += __shfl_xor(w2, o, 64);
      u2 += __shfl_xor(u2, o, 64);
    }
    if ((t & 63) == 0) { red[0][t >> 6] = w2; red[1][t >> 6] = u2; }
    __syncthreads();
    if (t == 0) {
      f32x2 s;
      s[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
      s[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
      *reinterpret_cast<f32x2*>(p.partial + 2 * c) = s;
    }
    __syncthreads();                                             // red is written again in the next round
  }
}

__global__ __launch_bounds__(256) void lamb_ratio_kernel(const LambParams p) {
  __shared__ double red[2][kLambThreads / 64];
  __shared__ float r_all;
  const int t = threadIdx.x;
  for (long s = blockIdx.x; s < p.n_segments; s += gridDim.x) {
    long c0, c1;
    lamb_segment_range(p.segment_start, s, p.n_chunks, c0, c1);
    double w2, u2;
    lamb_segment_lane_sum(p.partial, c0, c1, t, w2, u2);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      w2 += __shfl_xor(w2, o, 64);
      u2 += __shfl_xor(u2, o, 64);
    }
    if ((t & 63) == 0) { red[0][t >> 6] = w2; red[1][t >> 6] = u2; }
    __syncthreads();
    if (t == 0)
      r_all = lamb_ratio((red[0][0] + red[0][1]) + (red[0][2] + red[0][3]), (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]),
                         p.segment_adapt[s]);
    __syncthreads();
    const float r = r_all;
    for (long c = c0 + t; c < c1; c += kLambThreads) p.ratio[c] = r;
    __syncthreads();                                             // red and r_all are written again in the next round
  }
}

__global__ __launch_bounds__(256) void lamb_apply_kernel(const LambParams p) {
  const int t = threadIdx.x;
  const LambHyper h = lamb_hyper_dev(p);
  for (long c = blockIdx.x; c < p.n_chunks; c += gridDim.x) {
    const long i = c * kLambChunk + t * 4;
    const float r = p.ratio[c];
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(p.prm + i), u4 = *reinterpret_cast<const f32x4*>(p.grd + i);
    f32x4 o4;
    u16x4 s4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o4[j] = lamb_apply(w4[j], h.lr, r, u4[j]);
      s4[j] = lamb_bf16_bits(o4[j]);
    }
    *reinterpret_cast<f32x4*>(p.prm + i) = o4;
    if (p.shadow) *reinterpret_cast<u16x4*>(p.shadow + i) = s4;
    if (p.zero_grad) *reinterpret_cast<f32x4*>(p.grd + i) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

hipError_t launch_lamb(const LambParams& p, hipStream_t st) {
  const unsigned chunk_blocks = (unsigned)(p.n_chunks < 2048 ? p.n_chunks : 2048);
  const unsigned seg_blocks = (unsigned)(p.n_segments < 1024 ? p.n_segments : 1024);
  hipLaunchKernelGGL(lamb_moments_kernel, dim3(chunk_blocks), dim3(kLambThreads), 0, st, p);
  hipLaunchKernelGGL(lamb_ratio_kernel, dim3(seg_blocks), dim3(kLambThreads), 0, st, p);
  hipLaunchKernelGGL(lamb_apply_kernel, dim3(chunk_blocks), dim3(kLambThreads), 0, st, p);
  return hipGetLastError();
}
#endif  // MMT_LAMB_HOST_ONLY

}  // namespace
}  // namespace mmt

extern "C" {

size_t mmt_lamb_workspace_bytes(int64_t n) {
  if (n <= 0 || (n & (mmt::kLambChunk - 1))) return 0;
  return mmt::lamb_workspace_bytes(n);
}

int mmt_lamb_step_host(const mmt_lamb_desc* d, float* param, float* grad, float* exp_avg, float* exp_avg_sq, void* param_bf16,
                       const float* chunk_wd, const int32_t* segment_start, const int32_t* segment_adapt, const float* grad_scale,
                       void* workspace, size_t workspace_bytes) {
  using namespace mmt;
  LambParams p;
  const int rc = check_lamb("mmt_lamb_step_host", d, param, grad, exp_avg, exp_avg_sq, param_bf16, chunk_wd, segment_start, segment_adapt,
                            grad_scale, workspace, workspace_bytes, p);
  if (rc) return rc;
  LambHyper h = p.h;
  if (p.hyper) lamb_step_scalars(h, p.hyper[0], p.hyper[1], p.hyper[2]);
  const float gs = grad_scale ? *grad_scale : 1.f;
  float lane_w[kLambThreads], lane_u[kLambThreads];
  for (long c = 0; c < p.n_chunks; ++c) {                        // 1. moments
    const float wd = chunk_wd[c];
    for (int t = 0; t < kLambThreads; ++t) {
      const long i = c * kLambChunk + t * 4;
      float u[4];
      for (int j = 0; j < 4; ++j) {
        u[j] = lamb_direction(h, grad[i + j], gs, param[i + j], wd, exp_avg[i + j], exp_avg_sq[i + j]);
        grad[i + j] = u[j];
      }
      lane_w[t] = lamb_lane_sumsq(param[i], param[i + 1], param[i + 2], param[i + 3]);
      lane_u[t] = lamb_lane_sumsq(u[0], u[1], u[2], u[3]);
    }
    p.partial[2 * c] = lamb_fold_host(lane_w);
    p.partial[2 * c + 1] = lamb_fold_host(lane_u);
  }
  double seg_w[kLambThreads], seg_u[kLambThreads];
  for (long s = 0; s < p.n_segments; ++s) {                      // 2. ratios
    long c0, c1;
    lamb_segment_range(segment_start, s, p.n_chunks, c0, c1);
    for (int t = 0; t < kLambThreads; ++t) lamb_segment_lane_sum(p.partial, c0, c1, t, seg_w[t], seg_u[t]);
    const double w2 = lamb_fold_host(seg_w), u2 = lamb_fold_host(seg_u);
    const float r = lamb_ratio(w2, u2, segment_adapt[s]);
    for (long c = c0; c < c1; ++c) p.ratio[c] = r;
  }
  for (long c = 0; c < p.n_chunks; ++c) {                        // 3. apply
    const float r = p.ratio[c];
    for (long i = c * kLambChunk; i < (c + 1) * kLambChunk; ++i) {
      param[i] = lamb_apply(param[i], h.lr, r, grad[i]);
      if (p.shadow) p.shadow[i] = lamb_bf16_bits(param[i]);
      if (p.zero_grad) grad[i] = 0.f;
    }
  }
  return MMT_OK;
}

#ifndef MMT_LAMB_HOST_ONLY
int mmt_lamb_step(const mmt_lamb_desc* d, float* param, float* grad, float* exp_avg, float* exp_avg_sq, void* param_bf16,
                  const float* chunk_wd, const int32_t* segment_start, const int32_t* segment_adapt, const float* grad_scale,
                  void* workspace, size_t workspace_bytes, void* stream) {
  mmt::LambParams p;
  const int rc = mmt::check_lamb("mmt_lamb_step", d, param, grad, exp_avg, exp_avg_sq, param_bf16, chunk_wd, segment_start, segment_adapt,
                                 grad_scale, workspace, workspace_bytes, p);
  if (rc) return rc;
  const hipError_t e = mmt::launch_lamb(p, (hipStream_t)stream);
  return e == hipSuccess ? MMT_OK : mmt::fail(MMT_E_LAUNCH, "mmt_lamb_step: %s", hipGetErrorString(e));
}
#endif

}  // extern "C"
