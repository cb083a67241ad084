// LAMB over a flat parameter slab (lamb.hip; C ABI: include/mmt_layer.h, mmt_lamb_step; DESIGN.md section 4, "LAMB"):
// the per-element update, the sums of one 1024-element chunk and of one parameter segment, the trust ratio and the
// clamped place of a segment in the slab, shared by the kernels and mmt_lamb_step_host through __host__ __device__
// functions.
//
// Every sum has one fixed shape.  A chunk is 256 lanes of four elements: a lane adds its four, (x0 + x1) + (x2 + x3),
// the 64 lanes of a wave fold by halves (distance 32, 16, .., 1), and the four wave sums add as (s0 + s1) + (s2 + s3).
// A segment's chunk partials are dealt to 256 lanes by their index INSIDE the segment (partial j goes to lane j mod 256,
// each lane adds its own in rising order, in double), and the lanes fold the same way.  Nothing depends on the grid, on
// where the segment lies in the slab or on what shares the slab with it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

namespace mmt {

constexpr int kLambThreads = 256;                      // lanes of a workgroup
constexpr int kLambChunk = 1024;                       // elements of a chunk: one float4 per lane
constexpr int kLambChunkLog = 10;
static_assert(kLambChunk == 4 * kLambThreads && (1 << kLambChunkLog) == kLambChunk, "a chunk is one float4 per lane");

struct LambHyper {
  float lr, beta1, beta2, eps, inv_bc1, inv_bc2;
};

// {lr, 1 - beta1^t, 1 - beta2^t}: mmt_lamb_desc.hyper when it is given, else the descriptor's own fields
__host__ __device__ inline void lamb_step_scalars(LambHyper& a, float lr, float bc1, float bc2) {
  a.lr = lr;
  a.inv_bc1 = 1.f / bc1;
  a.inv_bc2 = 1.f / bc2;
}

// One element: the moments in place, the update direction u returned.  wd is the element's chunk's decay rate.
__host__ __device__ inline float lamb_direction(const LambHyper& a, float grad, float scale, float w, float wd, float& m, float& v) {
  const float g = grad * scale;
  m = a.beta1 * m + (1.f - a.beta1) * g;
  v = a.beta2 * v + (1.f - a.beta2) * g * g;
  const float mh = m * a.inv_bc1, vh = v * a.inv_bc2;
  return mh / (sqrtf(vh) + a.eps) + wd * w;
}

__host__ __device__ inline float lamb_lane_sumsq(float x0, float x1, float x2, float x3) {
  return (x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3);
}

// r of a segment from its two sums of squares
__host__ __device__ inline float lamb_ratio(double w2, double u2, int adapt) {
  return (adapt != 0 && w2 > 0.0 && u2 > 0.0) ? (float)(sqrt(w2) / sqrt(u2)) : 1.f;
}

__host__ __device__ inline float lamb_apply(float w, float lr, float r, float u) { return w - lr * r * u; }

// float -> bfloat16 bits, round to nearest even, NaN to the quiet NaN torch writes
__host__ __device__ inline uint16_t lamb_bf16_bits(float x) {
  uint32_t u;
  __builtin_memcpy(&u, &x, 4);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0u;
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// Chunks [c0, c1) of segment s, whatever the table says: both ends clamped into [0, n_chunks], an end before its start
// gives an empty range.  segment_start has n_segments + 1 entries.
__host__ __device__ inline void lamb_segment_range(const int32_t* segment_start, long s, long n_chunks, long& c0, long& c1) {
  const long a = segment_start[s], b = segment_start[s + 1];
  c0 = a < 0 ? 0 : (a > n_chunks ? n_chunks : a);
  c1 = b < 0 ? 0 : (b > n_chunks ? n_chunks : b);
  if (c1 < c0) c1 = c0;
}

// What lane `lane` of the workgroup adds of a segment's partials (float2 {sum w^2, sum u^2} per chunk)
__host__ __device__ inline void lamb_segment_lane_sum(const float* partial, long c0, long c1, int lane, double& w2, double& u2) {
  w2 = 0.0; u2 = 0.0;
  for (long c = c0 + lane; c < c1; c += kLambThreads) {
    w2 += (double)partial[2 * c];
    u2 += (double)partial[2 * c + 1];
  }
}

// The fold of 256 lane values as the kernels do it, on an array (host side): within each wave by halves, then the four
// wave sums.  x is overwritten.
template <typename T>
inline T lamb_fold_host(T* x) {
  for (int wave = 0; wave < kLambThreads / 64; ++wave)
    for (int o = 32; o > 0; o >>= 1)
      for (int i = 0; i < o; ++i) x[64 * wave + i] += x[64 * wave + i + o];
  return (x[0] + x[64]) + (x[128] + x[192]);
}

}  // namespace mmt
