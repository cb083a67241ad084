// Random item masking in one launch (item_masking.hip; C ABI: include/mmt_layer.h, mmt_item_masking; DESIGN.md section 4,
// "Masking in one launch"): what one token and one item of a row decide, shared by the kernel and mmt_item_masking_host
// through __host__ __device__ functions.  The definition is feature_pipeline.random_item_masking, its torch ops.
//
// A row in three int32 arrays of T words (the kernel keeps them in LDS, the host variant in thread-local memory):
//   item[t]   item index of token t: (word starts among the valid tokens [0, t]) - 1, at least 0
//   image[i]  order-preserving uint32 image of item i's shuffle key; +inf for an index that is no selectable item
//   flag[i]   bit 0: a valid token of item i is unselectable; bit 1: item i is chosen
// The rank of item i in torch's stable ascending sort of the T keys is (images below image[i]) + (equal images at a lower
// index); an item is chosen when it is selectable and that rank is below n_sel.  The n_sel-th smallest image comes from
// four 8-bit histogram passes, the count among its equals from a prefix sum.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

namespace mmt {

constexpr int kMaskThreads = 1024;                     // lanes of a workgroup: one workgroup per row
constexpr int kMaskMaxTokens = 8192;                   // MMT_MASK_MAX_TOKENS: three int32 words a token in LDS
constexpr int kMaskMaxUnselectable = 8;                // MMT_MASK_MAX_UNSELECTABLE
constexpr int kMaskPerLane = kMaskMaxTokens / kMaskThreads;
constexpr uint32_t kMaskImageInf = 0xFF800000u;        // mask_image(+inf)

struct MaskParams {
  const int32_t* token_ids;            // [B, T]
  const void* n_tokens;                // [B], int64 or int32
  const uint8_t* word_start;           // [B, T] or NULL (every token is an item)
  const float* item_keys;              // [B, T]
  const float* value_u;                // [B, T]
  const int32_t* random_ids;           // [B, T]
  int32_t* masked;                     // [B, T]
  int32_t* positions;                  // [B, T]
  int64_t* n_masked;                   // [B]
  int32_t* labels;                     // [B, T]
  int B, T, max_selections, mask_token_id, n_unselectable, n_tokens_i64;
  int32_t unselectable[kMaskMaxUnselectable];
  float selection_rate, mask_threshold, random_threshold;
};

__host__ __device__ inline int mask_clamp(long x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : (int)x); }

// `n_tokens` is data: whatever it holds, a row has between 0 and T valid tokens (torch's `pos < n_tokens`)
__host__ __device__ inline int mask_row_tokens(const MaskParams& p, int b) {
  const long n = p.n_tokens_i64 ? (long)((const int64_t*)p.n_tokens)[b] : (long)((const int32_t*)p.n_tokens)[b];
  return mask_clamp(n, 0, p.T);
}

__host__ __device__ inline bool mask_unselectable(const MaskParams& p, int32_t token) {
  bool hit = false;
  for (int k = 0; k < kMaskMaxUnselectable; ++k) hit |= k < p.n_unselectable && token == p.unselectable[k];
  return hit;
}

// torch's float order as unsigned order: NaN (any) above everything, -0 == +0
__host__ __device__ inline uint32_t mask_image(float key) {
  if (key != key) return 0xFFFFFFFFu;
  if (key == 0.f) return 0x80000000u;
  uint32_t u;
  memcpy(&u, &key, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// min(ceil(float32(n_selectable) * float32(selection_rate)), float32(max_selections)) as an integer in [0, T]: one
// product, rounded once
__host__ __device__ inline int mask_selections(const MaskParams& p, int n_selectable) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float c = ceilf(__fmul_rn((float)n_selectable, p.selection_rate));
#else
  volatile float prod = (float)n_selectable * p.selection_rate;
  const float c = ceilf(prod);
#endif
  const float m = (float)p.max_selections;
  if (c != c) return 0;                                // (torch's cast of NaN is the most negative integer: nothing is chosen)
  const float r = c < m ? c : m;
  return r >= (float)p.T ? p.T : (r >= 1.f ? (int)r : 0);
}

// The value a chosen token takes: its item's value_u decides
__host__ __device__ inline int32_t mask_new_token(const MaskParams& p, float u, int32_t token, int32_t random_id) {
  if (u < p.mask_threshold) return p.mask_token_id;
  if (u < p.random_threshold) return random_id;
  return token;
}

}  // namespace mmt
