// Exponential moving average of the weights over a flat parameter slab (ema.hip; C ABI: include/mmt_layer.h,
// mmt_ema_step / mmt_ema_swap; DESIGN.md section 4, "EMA of the weights"): the per-element update and the exchange,
// shared by the kernels and the host mirrors through __host__ __device__ functions.
//
// The fused multiply-add is spelt __builtin_fmaf on both sides, so the kernel and the host loop give the same bits
// whatever the contraction flags of either compile are.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lamb.h"                                      // the chunk geometry and lamb_bf16_bits, torch's fp32 -> bf16 rounding

namespace mmt {

constexpr int kEmaThreads = kLambThreads;              // lanes of a workgroup
constexpr int kEmaChunk = kLambChunk;                  // elements of a chunk: one float4 per lane
constexpr int kEmaChunkLog = kLambChunkLog;
constexpr int kEmaMaxBlocks = 2048;                    // 256 CUs x 8 workgroups; the chunk-strided loop takes the rest

// Workgroups of a launch over n_chunks chunks.  Every workgroup takes chunks b, b + G, b + 2G, ... two at a time.
__host__ __device__ inline long ema_grid(long n_chunks) { return n_chunks < kEmaMaxBlocks ? n_chunks : kEmaMaxBlocks; }

// avg <- avg + omd (param - avg), omd = 1 - decay: the subtraction rounded to fp32, then ONE fused multiply-add.  The two
// ends are exact by a select: fl(fl(p - a) + a) is not p when |a| is far above |p|, and 0 * inf is not 0, but decay 0
// means "the parameter itself" and decay 1 "no change".
__host__ __device__ inline float ema_update(float omd, float param, float avg) {
  if (omd == 1.f) return param;
  if (omd == 0.f) return avg;
  const float d = param - avg;
  return __builtin_fmaf(omd, d, avg);
}

}  // namespace mmt
