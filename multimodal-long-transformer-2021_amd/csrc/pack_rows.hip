// Packing short examples into long rows (C ABI: include/mmt_layer.h, mmt_pack_rows; DESIGN.md section 4, "Packed
// batches"): E unpacked examples [E, S] with their lengths go into R rows of S_row positions by the next-fit rule in
// arrival order, with the layout tensors the packed kernels read.  pack_rows.h has the rule, the searches and what one
// output position and one example slot receive, which the kernels and mmt_pack_rows_host share.
//
//   launches of mmt_pack_rows, 256 threads
//   1. plan  ONE workgroup, the lengths in LDS: a lane clamps and adds its 16 consecutive lengths, the 256 lane sums
//            are offset in rising order, every lane finds the row end for each of its possible row beginnings (a binary
//            search over the prefix sums), lane 0 follows those ends from example 0 through at most R rows, and all lanes
//            write the plan to the workspace, the per-example outputs and `consumed`
//   2. fill  a thread per output position: the row's examples from the plan, its own example by a binary search over
//            their first positions, then the five [R, S_row] outputs
//
// Two launches whatever the data holds; no atomics, no floating-point sum: the same inputs give the same bits.
// Workspace (caller's, no initialisation): int32 row_begin[R + 1], first[E], clen[E].
//
// Bounds: lengths are clamped into [1, S] where they are read; the fill clamps every plan word it reads into its array
// again, a position-table entry is clamped into [0, S) and the flat index into [0, R * S_row).  Wrong lengths give wrong
// rows, never a stray access.
#include "../../include/mmt_attn.h"
#include "../../include/mmt_layer.h"

#include <cstdint>

#include "mmt_err.h"
#include "pack_rows.h"

static_assert(MMT_PACK_MAX_EXAMPLES == mmt::kPackMaxExamples, "the header states the plan's limit");

namespace mmt {
namespace {

size_t pack_workspace_bytes(long E, long R) { return (((size_t)(R + 1 + 2 * E) * 4) + 15) & ~(size_t)15; }

int check_pack(const char* who, const mmt_pack_desc* d, const int32_t* word_ids, const int32_t* segment_ids, const int32_t* lengths,
               const int32_t* mlm_positions, const int32_t* mpp_positions, int32_t* out_word_ids, int32_t* out_segment_ids,
               int32_t* example_ids, int32_t* example_starts, int32_t* patch_slots, int64_t* first_positions, float* example_weight,
               int32_t* out_mlm_positions, int32_t* out_mpp_positions, int32_t* consumed, void* workspace, size_t workspace_bytes,
               PackParams& p) {
  if (!d || !word_ids || !segment_ids || !lengths || !out_word_ids || !out_segment_ids || !example_ids || !example_starts ||
      !patch_slots || !first_positions || !example_weight || !consumed)
    return fail(MMT_E_INVALID, "%s: NULL argument (only the position tables and the stream may be NULL)", who);
  if (d->E < 1 || d->R < 1 || d->E_max < 1) return fail(MMT_E_INVALID, "%s: E %d, R %d and E_max %d must be at least 1", who, d->E, d->R, d->E_max);
  if (d->S < 1 || d->S_row < d->S) return fail(MMT_E_INVALID, "%s: S %d must be at least 1 and S_row %d at least S", who, d->S, d->S_row);
  if (d->E > kPackMaxExamples || d->E_max > kPackMaxExamples)
    return fail(MMT_E_INVALID, "%s: E %d and E_max %d must be at most %d (MMT_PACK_MAX_EXAMPLES)", who, d->E, d->E_max, kPackMaxExamples);
  if ((long)d->E * d->S > 0x7FFFFFFFL || (long)d->R * d->S_row > 0x7FFFFFFFL)
    return fail(MMT_E_INVALID, "%s: E * S and R * S_row must stay below 2^31 (flat positions are int32)", who);
  if ((mlm_positions && (d->n_mlm < 1 || !out_mlm_positions)) || (mpp_positions && (d->n_mpp < 1 || !out_mpp_positions)))
    return fail(MMT_E_INVALID, "%s: a position table needs its column count (at least 1) and its output", who);
  const size_t need = pack_workspace_bytes(d->E, d->R);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 3) != 0)
    return fail(MMT_E_WORKSPACE, "%s: 4-byte aligned workspace of %zu bytes needed, %zu given", who, need, workspace ? workspace_bytes : (size_t)0);
  p.in_word = word_ids; p.in_seg = segment_ids; p.lengths = lengths;
  p.in_pos[0] = mlm_positions; p.in_pos[1] = mpp_positions;
  p.out_word = out_word_ids; p.out_seg = out_segment_ids; p.example_ids = example_ids; p.example_starts = example_starts;
  p.patch_slots = patch_slots; p.first_positions = first_positions; p.example_weight = example_weight;
  p.out_pos[0] = out_mlm_positions; p.out_pos[1] = out_mpp_positions; p.consumed = consumed;
  p.row_begin = (int32_t*)workspace; p.first = p.row_begin + (d->R + 1); p.clen = p.first + d->E;
  p.E = d->E; p.S = d->S; p.R = d->R; p.S_row = d->S_row; p.E_max = d->E_max;
  p.n_pos[0] = mlm_positions ? d->n_mlm : 0; p.n_pos[1] = mpp_positions ? d->n_mpp : 0;
  return MMT_OK;
}

#ifndef MMT_PACK_HOST_ONLY
__global__ __launch_bounds__(256) void pack_plan_kernel(const PackParams p) {
  __shared__ int32_t prefix[kPackMaxExamples + 1];
  __shared__ int32_t row_end[kPackMaxExamples];        // row_end[b]: where the row that begins at b ends
  __shared__ int32_t rowb[kPackMaxExamples + 1];
  __shared__ int32_t lane_sum[kPackThreads];
  __shared__ int32_t plan[2];                          // rows formed, examples consumed
  const int t = threadIdx.x;
  const int limit = p.E < p.E_max ? p.E : p.E_max;
  // prefix sums: a lane's own 16, then the lanes before it
  int32_t mine[kPackPerLane];
  int32_t sum = 0;
#pragma unroll
  for (int j = 0; j < kPackPerLane; ++j) {
    const int e = t * kPackPerLane + j;
    mine[j] = e < limit ? pack_length(p.lengths, e, p.S) : 0;
    sum += mine[j];
  }
  lane_sum[t] = sum;
  __syncthreads();
  int32_t at = 0;
  for (int j = 0; j < t; ++j) at += lane_sum[j];
#pragma unroll
  for (int j = 0; j < kPackPerLane; ++j) {
    const int e = t * kPackPerLane + j;
    if (e <= limit) prefix[e] = at;
    at += mine[j];
  }
  if (t == kPackThreads - 1 && limit == kPackMaxExamples) prefix[limit] = at;      // the one entry no lane's 16 reach
  __syncthreads();
  for (int b = t; b < limit; b += kPackThreads) row_end[b] = pack_row_end(prefix, b, limit, p.S_row);
  __syncthreads();
  if (t == 0) {
    int r = 0, b = 0;
    while (r < p.R && b < limit) {                     // at most `limit` rounds: every row takes an example
      rowb[r++] = b;
      b = row_end[b];
    }
    rowb[r] = b;
    plan[0] = r; plan[1] = b;
    p.consumed[0] = b;
  }
  __syncthreads();
  const int rows = plan[0], consumed = plan[1];
  for (int r = t; r <= p.R; r += kPackThreads) p.row_begin[r] = r <= rows ? rowb[r] : consumed;
  const int slots = p.E > p.E_max ? p.E : p.E_max;
  for (int e = t; e < slots; e += kPackThreads) {
    int row = 0, first = 0;
    if (e < consumed) {
      row = pack_last_at_most(rowb, 0, rows, e);
      first = prefix[e] - prefix[rowb[row]];
    }
    if (e < p.E) { p.first[e] = first; p.clen[e] = pack_length(p.lengths, e, p.S); }
    if (e < p.E_max) pack_example(p, e, consumed, row, first);
  }
}

__global__ __launch_bounds__(256) void pack_fill_kernel(const PackParams p) {
  const unsigned i = blockIdx.x * (unsigned)kPackThreads + threadIdx.x;       // R * S_row < 2^31 (check_pack)
  if (i >= (unsigned)p.R * (unsigned)p.S_row) return;
  const unsigned r = i / (unsigned)p.S_row;
  pack_position(p, (int)r, (int)(i - r * (unsigned)p.S_row));
}

hipError_t launch_pack(const PackParams& p, hipStream_t st) {
  const long total = (long)p.R * p.S_row;
  hipLaunchKernelGGL(pack_plan_kernel, dim3(1), dim3(kPackThreads), 0, st, p);
  hipLaunchKernelGGL(pack_fill_kernel, dim3((unsigned)((total + kPackThreads - 1) / kPackThreads)), dim3(kPackThreads), 0, st, p);
  return hipGetLastError();
}
#endif  // MMT_PACK_HOST_ONLY

}  // namespace
}  // namespace mmt

extern "C" {

size_t mmt_pack_rows_workspace_bytes(const mmt_pack_desc* d) {
  if (!d || d->E < 1 || d->R < 1 || d->E > mmt::kPackMaxExamples) return 0;
  return mmt::pack_workspace_bytes(d->E, d->R);
}

int mmt_pack_rows_host(const mmt_pack_desc* d, const int32_t* word_ids, const int32_t* segment_ids, const int32_t* lengths,
                       const int32_t* mlm_positions, const int32_t* mpp_positions, int32_t* out_word_ids, int32_t* out_segment_ids,
                       int32_t* example_ids, int32_t* example_starts, int32_t* patch_slots, int64_t* first_positions,
                       float* example_weight, int32_t* out_mlm_positions, int32_t* out_mpp_positions, int32_t* consumed,
                       void* workspace, size_t workspace_bytes) {
  using namespace mmt;
  PackParams p;
  const int rc = check_pack("mmt_pack_rows_host", d, word_ids, segment_ids, lengths, mlm_positions, mpp_positions, out_word_ids,
                            out_segment_ids, example_ids, example_starts, patch_slots, first_positions, example_weight,
                            out_mlm_positions, out_mpp_positions, consumed, workspace, workspace_bytes, p);
  if (rc) return rc;
  static thread_local int32_t prefix[kPackMaxExamples + 1], rowb[kPackMaxExamples + 1];
  const int limit = p.E < p.E_max ? p.E : p.E_max;
  prefix[0] = 0;                                                 // 1. plan
  for (int e = 0; e < limit; ++e) prefix[e + 1] = prefix[e] + pack_length(p.lengths, e, p.S);
  int rows = 0, b = 0;
  while (rows < p.R && b < limit) {
    rowb[rows++] = b;
    b = pack_row_end(prefix, b, limit, p.S_row);
  }
  rowb[rows] = b;
  const int taken = b;
  p.consumed[0] = taken;
  for (int r = 0; r <= p.R; ++r) p.row_begin[r] = r <= rows ? rowb[r] : taken;
  const int slots = p.E > p.E_max ? p.E : p.E_max;
  for (int e = 0; e < slots; ++e) {
    int row = 0, first = 0;
    if (e < taken) {
      row = pack_last_at_most(rowb, 0, rows, e);
      first = prefix[e] - prefix[rowb[row]];
    }
    if (e < p.E) { p.first[e] = first; p.clen[e] = pack_length(p.lengths, e, p.S); }
    if (e < p.E_max) pack_example(p, e, taken, row, first);
  }
  for (int r = 0; r < p.R; ++r)                                  // 2. fill
    for (int s = 0; s < p.S_row; ++s) pack_position(p, r, s);
  return MMT_OK;
}

#ifndef MMT_PACK_HOST_ONLY
int mmt_pack_rows(const mmt_pack_desc* d, const int32_t* word_ids, const int32_t* segment_ids, const int32_t* lengths,
                  const int32_t* mlm_positions, const int32_t* mpp_positions, int32_t* out_word_ids, int32_t* out_segment_ids,
                  int32_t* example_ids, int32_t* example_starts, int32_t* patch_slots, int64_t* first_positions,
                  float* example_weight, int32_t* out_mlm_positions, int32_t* out_mpp_positions, int32_t* consumed,
                  void* workspace, size_t workspace_bytes, void* stream) {
  mmt::PackParams p;
  const int rc = mmt::check_pack("mmt_pack_rows", d, word_ids, segment_ids, lengths, mlm_positions, mpp_positions, out_word_ids,
                                 out_segment_ids, example_ids, example_starts, patch_slots, first_positions, example_weight,
                                 out_mlm_positions, out_mpp_positions, consumed, workspace, workspace_bytes, p);
  if (rc) return rc;
  const hipError_t e = mmt::launch_pack(p, (hipStream_t)stream);
  return e == hipSuccess ? MMT_OK : mmt::fail(MMT_E_LAUNCH, "mmt_pack_rows: %s", hipGetErrorString(e));
}
#endif

}  // extern "C"
