// Exponential moving average of the weights over the optimizer's flat slabs (C ABI: include/mmt_layer.h, mmt_ema_step and
// mmt_ema_swap; DESIGN.md section 4, "EMA of the weights").  ema.h has the per-element update, which the kernels and the
// host mirrors share.
//
//   mmt_ema_step  one launch per slab: reads param and avg, writes avg.  12 bytes per element.
//   mmt_ema_swap  one launch per slab: exchanges param and avg in place and writes the bf16 shadow of the new param.
//
// Both are memory-bound streaming passes of the adamw_kernel family (fused_layer.hip): 256 threads, a workgroup takes
// whole 1024-element chunks (one 16-byte access per lane and array), two chunks per iteration -- four 16-byte loads in
// flight per thread before the first store -- and a grid of at most kEmaMaxBlocks workgroups strides over the chunks.
// Padding elements are zero in param and avg and stay zero: 0 + omd (0 - 0) = 0.
//
// Bounds: every index comes from the chunk loop, c < n / 1024; nothing is read from device memory but the slabs and the
// one-float decay word.
#include "../../include/mmt_attn.h"
#include "../../include/mmt_layer.h"

#include <cstdint>

#include "ema.h"
#include "mmt_err.h"

namespace mmt {
namespace {

int check_ema_slab(const char* who, int64_t n, const void* param, const void* avg, const void* param_bf16) {
  if (!param || !avg) return fail(MMT_E_INVALID, "%s: NULL argument (only param_bf16, the device decay word and the stream may be NULL)", who);
  if (n <= 0 || (n & (kEmaChunk - 1))) return fail(MMT_E_INVALID, "%s: n must be a positive multiple of 1024", who);
  if (param == avg) return fail(MMT_E_INVALID, "%s: avg and param are the same slab", who);
  if ((((uintptr_t)param | (uintptr_t)avg) & 15) != 0 || ((uintptr_t)param_bf16 & 7) != 0)
    return fail(MMT_E_INVALID, "%s: the fp32 slabs must be 16-byte, the bf16 shadow 8-byte aligned", who);
  return MMT_OK;
}

int check_ema_step(const char* who, const mmt_ema_desc* d, const float* param, const float* avg) {
  if (!d) return fail(MMT_E_INVALID, "%s: NULL descriptor", who);
  if (const int rc = check_ema_slab(who, d->n, param, avg, nullptr)) return rc;
  if (!d->one_minus_decay_dev && !(d->one_minus_decay >= 0.f && d->one_minus_decay <= 1.f))
    return fail(MMT_E_INVALID, "%s: one_minus_decay %g is not in [0, 1]", who, (double)d->one_minus_decay);
  return MMT_OK;
}

#ifndef MMT_EMA_HOST_ONLY
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void ema_step_kernel(const float* __restrict__ prm, float* __restrict__ avg, long n_chunks,
                                                       float omd, const float* __restrict__ omd_dev) {
  if (omd_dev) omd = *omd_dev;          // device-resident 1 - decay of a replayed step (mmt_ema_desc.one_minus_decay_dev)
  for (long c0 = blockIdx.x; c0 < n_chunks; c0 += 2L * gridDim.x) {
    const long c1 = c0 + gridDim.x;
    const bool two = c1 < n_chunks;
    const long i0 = c0 * kEmaChunk + threadIdx.x * 4, i1 = (two ? c1 : c0) * kEmaChunk + threadIdx.x * 4;
    const f32x4 p0 = *reinterpret_cast<const f32x4*>(prm + i0), a0 = *reinterpret_cast<const f32x4*>(avg + i0);
    const f32x4 p1 = *reinterpret_cast<const f32x4*>(prm + i1), a1 = *reinterpret_cast<const f32x4*>(avg + i1);
    f32x4 o0, o1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o0[j] = ema_update(omd, p0[j], a0[j]);
      o1[j] = ema_update(omd, p1[j], a1[j]);
    }
    *reinterpret_cast<f32x4*>(avg + i0) = o0;
    if (two) *reinterpret_cast<f32x4*>(avg + i1) = o1;
  }
}

__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ prm, float* __restrict__ avg,
                                                       uint16_t* __restrict__ shadow, long n_chunks) {
  for (long c0 = blockIdx.x; c0 < n_chunks; c0 += 2L * gridDim.x) {
    const long c1 = c0 + gridDim.x;
    const bool two = c1 < n_chunks;
    const long i0 = c0 * kEmaChunk + threadIdx.x * 4, i1 = (two ? c1 : c0) * kEmaChunk + threadIdx.x * 4;
    const f32x4 p0 = *reinterpret_cast<const f32x4*>(prm + i0), a0 = *reinterpret_cast<const f32x4*>(avg + i0);
    const f32x4 p1 = *reinterpret_cast<const f32x4*>(prm + i1), a1 = *reinterpret_cast<const f32x4*>(avg + i1);
    u16x4 s0, s1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s0[j] = lamb_bf16_bits(a0[j]);
      s1[j] = lamb_bf16_bits(a1[j]);
    }
    *reinterpret_cast<f32x4*>(prm + i0) = a0;
    *reinterpret_cast<f32x4*>(avg + i0) = p0;
    if (shadow) *reinterpret_cast<u16x4*>(shadow + i0) = s0;
    if (two) {
      *reinterpret_cast<f32x4*>(prm + i1) = a1;
      *reinterpret_cast<f32x4*>(avg + i1) = p1;
      if (shadow) *reinterpret_cast<u16x4*>(shadow + i1) = s1;
    }
  }
}
#endif  // MMT_EMA_HOST_ONLY

}  // namespace
}  // namespace mmt

extern "C" {

int mmt_ema_step_host(const mmt_ema_desc* d, const float* param, float* avg) {
  if (const int rc = mmt::check_ema_step("mmt_ema_step_host", d, param, avg)) return rc;
  const float omd = d->one_minus_decay_dev ? *d->one_minus_decay_dev : d->one_minus_decay;
  for (int64_t i = 0; i < d->n; ++i) avg[i] = mmt::ema_update(omd, param[i], avg[i]);
  return MMT_OK;
}

int mmt_ema_swap_host(int64_t n, float* param, float* avg, void* param_bf16) {
  if (const int rc = mmt::check_ema_slab("mmt_ema_swap_host", n, param, avg, param_bf16)) return rc;
  uint16_t* shadow = (uint16_t*)param_bf16;
  for (int64_t i = 0; i < n; ++i) {
    const float p = param[i];
    param[i] = avg[i];
    avg[i] = p;
    if (shadow) shadow[i] = mmt::lamb_bf16_bits(param[i]);
  }
  return MMT_OK;
}

#ifndef MMT_EMA_HOST_ONLY
int mmt_ema_step(const mmt_ema_desc* d, const float* param, float* avg, void* stream) {
  if (const int rc = mmt::check_ema_step("mmt_ema_step", d, param, avg)) return rc;
  const long n_chunks = (long)(d->n >> mmt::kEmaChunkLog);
  hipLaunchKernelGGL(mmt::ema_step_kernel, dim3((unsigned)mmt::ema_grid(n_chunks)), dim3(mmt::kEmaThreads), 0, (hipStream_t)stream,
                     param, avg, n_chunks, d->one_minus_decay, d->one_minus_decay_dev);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MMT_OK : mmt::fail(MMT_E_LAUNCH, "mmt_ema_step: %s", hipGetErrorString(e));
}

int mmt_ema_swap(int64_t n, float* param, float* avg, void* param_bf16, void* stream) {
  if (const int rc = mmt::check_ema_slab("mmt_ema_swap", n, param, avg, param_bf16)) return rc;
  const long n_chunks = (long)(n >> mmt::kEmaChunkLog);
  hipLaunchKernelGGL(mmt::ema_swap_kernel, dim3((unsigned)mmt::ema_grid(n_chunks)), dim3(mmt::kEmaThreads), 0, (hipStream_t)stream,
                     param, avg, (uint16_t*)param_bf16, n_chunks);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MMT_OK : mmt::fail(MMT_E_LAUNCH, "mmt_ema_swap: %s", hipGetErrorString(e));
}
#endif

}  // extern "C"
