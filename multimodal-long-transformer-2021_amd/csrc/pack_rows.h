// Packing short examples into long rows (pack_rows.hip; C ABI: include/mmt_layer.h, mmt_pack_rows; DESIGN.md section 4,
// "Packed batches"): the clamping of the lengths, the end of a row under the next-fit rule, the searches of the fill, and
// what one output position and one example slot receive -- shared by the kernels and mmt_pack_rows_host through
// __host__ __device__ functions.
//
// The plan in three arrays, all of example indices or row positions:
//   prefix[i]     sum of the clamped lengths of examples [0, i), i in [0, limit], limit = min(E, E_max)
//   row_begin[r]  first example of row r, r in [0, R]; rows the rule does not reach begin (and end) at `consumed`
//   first[e]      position of example e in its row (0 for an example that is not consumed)
// A row that begins at b ends before the first j with prefix[j + 1] - prefix[b] > S_row.  Every clamped length is in
// [1, S] and S <= S_row, so a row that begins below the limit takes at least one example.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mmt {

constexpr int kPackThreads = 256;                      // lanes of a workgroup
constexpr int kPackMaxExamples = 4096;                 // MMT_PACK_MAX_EXAMPLES: the plan keeps E int32 words three times in LDS
constexpr int kPackPerLane = kPackMaxExamples / kPackThreads;

struct PackParams {
  const int32_t* in_word;              // [E, S]
  const int32_t* in_seg;               // [E, S]
  const int32_t* lengths;              // [E]
  const int32_t* in_pos[2];            // [E, n_pos[k]] or NULL
  int32_t* out_word;                   // [R, S_row]
  int32_t* out_seg;
  int32_t* example_ids;
  int32_t* example_starts;
  int32_t* patch_slots;
  int64_t* first_positions;            // [E_max, 2]
  float* example_weight;               // [E_max]
  int32_t* out_pos[2];                 // [E_max, n_pos[k]]
  int32_t* consumed;                   // [1]
  int32_t* row_begin;                  // workspace [R + 1]
  int32_t* first;                      // workspace [E]
  int32_t* clen;                       // workspace [E]
  int E, S, R, S_row, E_max, n_pos[2];
};

__host__ __device__ inline int pack_clamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// `lengths` is data: whatever it holds, an example takes between 1 and S positions
__host__ __device__ inline int pack_length(const int32_t* lengths, int e, int S) { return pack_clamp(lengths[e], 1, S); }

// Exclusive end of the row that begins at example b < limit: the largest j in (b, limit] with prefix[j] - prefix[b] <= S_row.
__host__ __device__ inline int pack_row_end(const int32_t* prefix, int b, int limit, int S_row) {
  int lo = b + 1, hi = limit;                          // the answer is in [lo, hi]; lo always fits (one example fits a row)
  const int base = prefix[b];
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] - base <= S_row) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The largest i in [lo, hi) with a[i] <= x, for a rising a[lo..hi) with a[lo] <= x: the row of an example among the row
// beginnings, and the example of a position among the first positions of its row.
__host__ __device__ inline int pack_last_at_most(const int32_t* a, int lo, int hi, int x) {
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// Output position s of row r.  Examples [lo, hi) make the row: ids fall from hi - lo to 1, the tail behind the last
// example is a run of its own with id 0 and slot -1.  Everything read from the workspace is clamped again: the plan of a
// call is this call's own, but nothing here trusts it with an address.
__host__ __device__ inline void pack_position(const PackParams& p, int r, int s) {
  const long o = (long)r * p.S_row + s;
  const int lo = pack_clamp(p.row_begin[r], 0, p.E), hi = pack_clamp(p.row_begin[r + 1], lo, p.E);
  int word = 0, seg = 0, id = 0, start = 0, slot = -1;
  if (hi > lo) {
    const int e = pack_last_at_most(p.first, lo, hi, s);
    const int f = pack_clamp(p.first[e], 0, p.S_row - 1), n = pack_clamp(p.clen[e], 1, p.S);
    if (s >= f && s < f + n) {
      const long i = (long)e * p.S + (s - f);
      word = p.in_word[i]; seg = p.in_seg[i];
      id = hi - e; start = f; slot = e;
    } else {
      start = pack_clamp(f + n, 0, p.S_row);           // the tail: only behind the row's last example, where e == hi - 1
    }
  }
  p.out_word[o] = word; p.out_seg[o] = seg;
  p.example_ids[o] = id; p.example_starts[o] = start; p.patch_slots[o] = slot;
}

// Example slot e of [0, E_max): (row, first position), weight, and the position tables as flat indices into [R * S_row].
// A slot at or behind `consumed` is absent: zeros.
__host__ __device__ inline void pack_example(const PackParams& p, int e, int consumed, int row, int first) {
  const bool here = e < consumed;
  p.first_positions[2 * (long)e] = here ? row : 0;
  p.first_positions[2 * (long)e + 1] = here ? first : 0;
  p.example_weight[e] = here ? 1.f : 0.f;
  const long last = (long)p.R * p.S_row - 1;
  for (int k = 0; k < 2; ++k) {
    if (!p.in_pos[k]) continue;
    const int n = p.n_pos[k];
    for (int j = 0; j < n; ++j) {
      long flat = 0;
      if (here) {
        flat = (long)row * p.S_row + first + pack_clamp(p.in_pos[k][(long)e * n + j], 0, p.S - 1);
        if (flat > last) flat = last;
      }
      p.out_pos[k][(long)e * n + j] = (int32_t)flat;
    }
  }
}

}  // namespace mmt
