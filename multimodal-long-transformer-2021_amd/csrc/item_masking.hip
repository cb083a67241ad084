// Random item masking in one launch (C ABI: include/mmt_layer.h, mmt_item_masking; DESIGN.md section 4, "Masking in one
// launch"): feature_pipeline.random_item_masking -- tf_text.mask_language_model with the random draws as inputs -- for a
// padded [B, T] batch.  item_masking.h has what one token and one item decide, which the kernel and
// mmt_item_masking_host share.
//
//   ONE launch, one workgroup of 1024 threads per row, the row's three int32 arrays in LDS; a lane owns ceil(T / 1024)
//   consecutive positions
//   1. items     prefix sum of the word starts among the valid tokens -> item[t]
//   2. flags     a valid unselectable token marks its item (plain LDS stores of one value)
//   3. images    selectable items counted, n_sel from the one fp32 product, image[i] of every index
//   4. select    four 8-bit histogram passes (LDS atomics) for the n_sel-th smallest image, then a prefix sum among its
//                equals -> the chosen items
//   5. tokens    the new value of every token, a prefix sum of the chosen tokens -> positions and labels, compacted
//
// No atomics on global memory, no workspace, no floating-point sum, nothing outlives the launch: the same inputs give
// the same bits.
//
// Bounds: n_tokens is clamped into [0, T] where it is read; an item index is a count of word starts, so it is below T, and
// it is clamped again where it becomes an address; a compacted position is a count of chosen tokens, below T.  random_ids
// and token_ids are values only.  Wrong inputs give wrong rows, never a stray access.
#include "../../include/mmt_attn.h"
#include "../../include/mmt_layer.h"

#include <cstdint>

#include "item_masking.h"
#include "mmt_err.h"

static_assert(MMT_MASK_MAX_TOKENS == mmt::kMaskMaxTokens, "the header states the row limit");
static_assert(MMT_MASK_MAX_UNSELECTABLE == mmt::kMaskMaxUnselectable, "the header states the id limit");

namespace mmt {
namespace {

int check_mask(const char* who, const mmt_item_masking_desc* d, const int32_t* token_ids, const void* n_tokens, const uint8_t* word_start,
               const float* item_keys, const float* value_u, const int32_t* random_ids, int32_t* masked, int32_t* positions,
               int64_t* n_masked, int32_t* labels, MaskParams& p) {
  if (!d || !token_ids || !n_tokens || !item_keys || !value_u || !random_ids || !masked || !positions || !n_masked || !labels)
    return fail(MMT_E_INVALID, "%s: NULL argument (only word_start and the stream may be NULL)", who);
  if (d->B < 1 || d->T < 1) return fail(MMT_E_INVALID, "%s: B %d and T %d must be at least 1", who, d->B, d->T);
  if (d->n_unselectable < 0) return fail(MMT_E_INVALID, "%s: n_unselectable %d must not be negative", who, d->n_unselectable);
  if ((long)d->B * d->T > 0x7FFFFFFFL) return fail(MMT_E_INVALID, "%s: B * T must stay below 2^31", who);
  if (d->T > kMaskMaxTokens)
    return fail(MMT_E_UNSUPPORTED, "%s: T %d is above %d (MMT_MASK_MAX_TOKENS: a row lives in LDS)", who, d->T, kMaskMaxTokens);
  if (d->n_unselectable > kMaskMaxUnselectable)
    return fail(MMT_E_UNSUPPORTED, "%s: %d unselectable ids, at most %d (MMT_MASK_MAX_UNSELECTABLE)", who, d->n_unselectable,
                kMaskMaxUnselectable);
  p.token_ids = token_ids; p.n_tokens = n_tokens; p.word_start = word_start; p.item_keys = item_keys; p.value_u = value_u;
  p.random_ids = random_ids; p.masked = masked; p.positions = positions; p.n_masked = n_masked; p.labels = labels;
  p.B = d->B; p.T = d->T; p.max_selections = d->max_selections; p.mask_token_id = d->mask_token_id;
  p.n_unselectable = d->n_unselectable; p.n_tokens_i64 = d->n_tokens_i64 != 0;
  for (int k = 0; k < kMaskMaxUnselectable; ++k) p.unselectable[k] = d->unselectable[k];
  p.selection_rate = d->selection_rate; p.mask_threshold = d->mask_threshold; p.random_threshold = d->random_threshold;
  return MMT_OK;
}

#ifndef MMT_MASK_HOST_ONLY
constexpr int kMaskWaves = kMaskThreads / 64;

// Inclusive prefix sum of one value per lane over the workgroup, and the sum of all; wave_tot is kMaskWaves LDS words.
__device__ inline int mask_block_scan(int v, int32_t* wave_tot, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  if (lane == 63) wave_tot[w] = v;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int j = 0; j < kMaskWaves; ++j) {
    const int s = wave_tot[j];
    all += s;
    if (j < w) before += s;
  }
  __syncthreads();                                     // wave_tot is free again
  total = all;
  return v + before;
}

__global__ __launch_bounds__(kMaskThreads) void item_masking_kernel(const MaskParams p, const int chunk, const int t_words) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int32_t* item = (int32_t*)smem;                      // [t_words] each
  uint32_t* image = (uint32_t*)(item + t_words);
  int32_t* flag = (int32_t*)(image + t_words);
  int32_t* hist = flag + t_words;                      // [256]
  int32_t* wave_tot = hist + 256;                      // [kMaskWaves]
  int32_t* pick = wave_tot + kMaskWaves;               // [2]
  const int tid = threadIdx.x, T = p.T;
  const long row = (long)blockIdx.x * T;
  const int n = mask_row_tokens(p, (int)blockIdx.x);
  const int t0 = tid * chunk < T ? tid * chunk : T;    // chunk <= kMaskPerLane
  const int len = T - t0 < chunk ? T - t0 : chunk;

  // 1. items
  unsigned start_bits = 0;
  int mine = 0, total = 0;
#pragma unroll
  for (int j = 0; j < kMaskPerLane; ++j) {
    const int t = t0 + j;
    if (j < len && t < n && (!p.word_start || p.word_start[row + t] != 0)) { start_bits |= 1u << j; ++mine; }
  }
  int run = mask_block_scan(mine, wave_tot, total) - mine;
  const int n_items = n > 0 ? (total > 1 ? total : 1) : 0;
#pragma unroll
  for (int j = 0; j < kMaskPerLane; ++j) {
    if (j >= len) continue;
    run += (start_bits >> j) & 1u;
    item[t0 + j] = run > 0 ? run - 1 : 0;
    flag[t0 + j] = 0;
  }
  __syncthreads();

  // 2. flags
  int32_t tok[kMaskPerLane];
#pragma unroll
  for (int j = 0; j < kMaskPerLane; ++j) {
    const int t = t0 + j;
    tok[j] = j < len ? p.token_ids[row + t] : 0;
    if (j < len && t < n && mask_unselectable(p, tok[j])) flag[mask_clamp(item[t], 0, T - 1)] = 1;
  }
  __syncthreads();

  // 3. images
  mine = 0;
#pragma unroll
  for (int j = 0; j < kMaskPerLane; ++j) {
    const int i = t0 + j;
    if (j >= len) continue;
    const bool selectable = i < n_items && !(flag[i] & 1);
    mine += selectable;
    image[i] = selectable ? mask_image(p.item_keys[row + i]) : kMaskImageInf;
  }
  int n_selectable = 0;
  (void)mask_block_scan(mine, wave_tot, n_selectable);
  const int n_sel = mask_selections(p, n_selectable);  // the same in every lane

  // 4. select
  if (n_sel >= 1) {
    uint32_t prefix = 0, known = 0;
    int k = n_sel;                                     // the k-th smallest (from 1) among the images that match the prefix
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();                                 // (also: every image of step 3 is written)
#pragma unroll
      for (int j = 0; j < kMaskPerLane; ++j) {
        if (j >= len) continue;
        const uint32_t im = image[t0 + j];
        if ((im & known) == prefix) atomicAdd(&hist[(im >> shift) & 255u], 1);
      }
      __syncthreads();
      const int h = tid < 256 ? hist[tid] : 0;
      int all = 0;
      const int incl = mask_block_scan(h, wave_tot, all);
      if (tid < 256 && incl - h < k && k <= incl) { pick[0] = tid; pick[1] = incl - h; }     // one lane: all >= k
      __syncthreads();
      const int digit = pick[0] & 255, below = pick[1];
      prefix |= (uint32_t)digit << shift;
      known |= 255u << shift;
      k -= below;
    }
    mine = 0;
#pragma unroll
    for (int j = 0; j < kMaskPerLane; ++j) mine += j < len && image[t0 + j] == prefix;
    int equals = 0;
    run = mask_block_scan(mine, wave_tot, equals) - mine;
#pragma unroll
    for (int j = 0; j < kMaskPerLane; ++j) {
      const int i = t0 + j;
      if (j >= len) continue;
      const uint32_t im = image[i];
      const bool selectable = i < n_items && !(flag[i] & 1);
      if (selectable && (im < prefix || (im == prefix && run < k))) flag[i] |= 2;
      run += im == prefix;
    }
  }
  __syncthreads();

  // 5. tokens
  unsigned chosen_bits = 0;
  mine = 0;
#pragma unroll
  for (int j = 0; j < kMaskPerLane; ++j) {
    const int t = t0 + j;
    if (j >= len) continue;
    const int it = mask_clamp(item[t], 0, T - 1);
    const bool chosen = t < n && (flag[it] & 2);
    int32_t out = tok[j];
    if (chosen) {
      out = mask_new_token(p, p.value_u[row + it], tok[j], p.random_ids[row + t]);
      chosen_bits |= 1u << j;
      ++mine;
    }
    p.masked[row + t] = out;
  }
  int n_masked = 0;
  run = mask_block_scan(mine, wave_tot, n_masked) - mine;
#pragma unroll
  for (int j = 0; j < kMaskPerLane; ++j) {
    if (j >= len || !((chosen_bits >> j) & 1u)) continue;
    const int o = run < T - 1 ? run : T - 1;
    p.positions[row + o] = t0 + j;
    p.labels[row + o] = tok[j];
    ++run;
  }
  for (int o = n_masked + tid; o < T; o += kMaskThreads) { p.positions[row + o] = 0; p.labels[row + o] = 0; }
  if (tid == 0) p.n_masked[blockIdx.x] = n_masked;
}

hipError_t launch_mask(const MaskParams& p, hipStream_t st) {
  const int chunk = (p.T + kMaskThreads - 1) / kMaskThreads;
  const int t_words = (p.T + 3) & ~3;
  const size_t lds = ((size_t)3 * t_words + 256 + kMaskWaves + 4) * 4;
  if (lds > 64 * 1024) {                               // (no stream operation: legal while the stream is being captured)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(item_masking_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(item_masking_kernel, dim3((unsigned)p.B), dim3(kMaskThreads), lds, st, p, chunk, t_words);
  return hipGetLastError();
}
#endif  // MMT_MASK_HOST_ONLY

// One row as plain loops over the functions of item_masking.h
void mask_row_host(const MaskParams& p, int b, int32_t* item, uint32_t* image, int32_t* flag) {
  const int T = p.T;
  const long row = (long)b * T;
  const int n = mask_row_tokens(p, b);
  int run = 0;
  for (int t = 0; t < T; ++t) {                                  // 1. items
    run += t < n && (!p.word_start || p.word_start[row + t] != 0);
    item[t] = run > 0 ? run - 1 : 0;
    flag[t] = 0;
  }
  const int n_items = n > 0 ? (run > 1 ? run : 1) : 0;
  for (int t = 0; t < n; ++t)                                    // 2. flags
    if (mask_unselectable(p, p.token_ids[row + t])) flag[mask_clamp(item[t], 0, T - 1)] = 1;
  int n_selectable = 0;
  for (int i = 0; i < T; ++i) {                                  // 3. images
    const bool selectable = i < n_items && !(flag[i] & 1);
    n_selectable += selectable;
    image[i] = selectable ? mask_image(p.item_keys[row + i]) : kMaskImageInf;
  }
  const int n_sel = mask_selections(p, n_selectable);
  if (n_sel >= 1) {                                              // 4. select
    uint32_t prefix = 0, known = 0;
    int k = n_sel;
    for (int shift = 24; shift >= 0; shift -= 8) {
      int hist[256] = {0};
      for (int i = 0; i < T; ++i)
        if ((image[i] & known) == prefix) ++hist[(image[i] >> shift) & 255u];
      int digit = 0, below = 0;
      while (digit < 255 && below + hist[digit] < k) below += hist[digit++];
      prefix |= (uint32_t)digit << shift;
      known |= 255u << shift;
      k -= below;
    }
    run = 0;
    for (int i = 0; i < T; ++i) {
      const bool selectable = i < n_items && !(flag[i] & 1);
      if (selectable && (image[i] < prefix || (image[i] == prefix && run < k))) flag[i] |= 2;
      run += image[i] == prefix;
    }
  }
  run = 0;
  for (int t = 0; t < T; ++t) {                                  // 5. tokens
    const int it = mask_clamp(item[t], 0, T - 1);
    const int32_t token = p.token_ids[row + t];
    int32_t out = token;
    if (t < n && (flag[it] & 2)) {
      out = mask_new_token(p, p.value_u[row + it], token, p.random_ids[row + t]);
      p.positions[row + run] = t;
      p.labels[row + run] = token;
      ++run;
    }
    p.masked[row + t] = out;
  }
  p.n_masked[b] = run;
  for (int o = run; o < T; ++o) { p.positions[row + o] = 0; p.labels[row + o] = 0; }
}

}  // namespace
}  // namespace mmt

extern "C" {

int mmt_item_masking_host(const mmt_item_masking_desc* d, const int32_t* token_ids, const void* n_tokens, const uint8_t* word_start,
                          const float* item_keys, const float* value_u, const int32_t* random_ids, int32_t* masked,
                          int32_t* positions, int64_t* n_masked, int32_t* labels) {
  using namespace mmt;
  MaskParams p;
  const int rc = check_mask("mmt_item_masking_host", d, token_ids, n_tokens, word_start, item_keys, value_u, random_ids, masked,
                            positions, n_masked, labels, p);
  if (rc) return rc;
  static thread_local int32_t item[kMaskMaxTokens], flag[kMaskMaxTokens];
  static thread_local uint32_t image[kMaskMaxTokens];
  for (int b = 0; b < p.B; ++b) mask_row_host(p, b, item, image, flag);
  return MMT_OK;
}

#ifndef MMT_MASK_HOST_ONLY
int mmt_item_masking(const mmt_item_masking_desc* d, const int32_t* token_ids, const void* n_tokens, const uint8_t* word_start,
                     const float* item_keys, const float* value_u, const int32_t* random_ids, int32_t* masked, int32_t* positions,
                     int64_t* n_masked, int32_t* labels, void* stream) {
  mmt::MaskParams p;
  const int rc = mmt::check_mask("mmt_item_masking", d, token_ids, n_tokens, word_start, item_keys, value_u, random_ids, masked,
                                 positions, n_masked, labels, p);
  if (rc) return rc;
  const hipError_t e = mmt::launch_mask(p, (hipStream_t)stream);
  return e == hipSuccess ? MMT_OK : mmt::fail(MMT_E_LAUNCH, "mmt_item_masking: %s", hipGetErrorString(e));
}
#endif

}  // extern "C"
