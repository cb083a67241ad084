// JPEG entropy decode on the device (C ABI: include/mmt_layer.h, mmt_jpeg_entropy*): the Huffman decode of a batch of
// baseline scans as kernels, into the coefficient layout that stage 2 (jpeg_decode.hip) reads.  DESIGN.md section 4,
// "JPEG entropy decode on the device", has the algorithm and the bounds argument; jpeg_entropy.h has the decode of
// one subsequence, which the kernels and mmt_jpeg_entropy_host share.
//
//   launches, grid (groups, B) unless stated, 256 threads; a group is the K subsequences one workgroup owns
//   1. clear       (parts, B): zeroes the planes, the status word and the changed words
//   2. round r     x max_rounds: a group whose entry state did not change leaves at once; the others stage their bytes
//                  and the image's tables into LDS and decode until no state inside the group changes (at most K + 1
//                  passes between __syncthreads).  A group reads its left neighbour's exit of round r - 1 and writes its
//                  own of round r into the other half of `edge`: no workgroup reads what another writes in that launch.
//   3. sums        per group: slots from its last segment start to its end, and whether it holds a segment start
//   4. carries     (B): the running sum over the groups of an image, reset at segment starts
//   5. write       checks the chain of states (not converged otherwise), decodes from the stored entry state and
//                  stores the coefficients at the slots the prefix sums give; ranges of different lanes are disjoint
//   6. DC          (3, B): segmented prefix sum of the DC differences per component, in scan order
//
// Bounds: ent_image() and ent_sub() clamp every offset, count and index of the plan; the bit reader stops at the staged
// window and at the segment's end; a coefficient is stored only inside its component's block grid and inside coef.
#include "../../include/mmt_attn.h"
#include "../../include/mmt_layer.h"

#include <cstdint>
#include <cstring>

#include "jpeg_entropy.h"
#include "mmt_err.h"

namespace mmt {
namespace {

const unsigned char kZigzagHost[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct EntLayout {                      // of the workspace, in bytes from its start
  size_t changed, entry, exit_, slots, edge, tail, has_start, carry, total;
};

EntLayout ent_layout(int B, long n_subseq, int groups, int max_rounds) {
  EntLayout l;
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  size_t at = 0;
  l.changed = at; at = up(at + (size_t)max_rounds * B * 4);
  l.entry = at; at = up(at + (size_t)n_subseq * 8);
  l.exit_ = at; at = up(at + (size_t)n_subseq * 8);
  l.slots = at; at = up(at + (size_t)n_subseq * 4);
  l.edge = at; at = up(at + (size_t)2 * B * groups * 8);
  l.tail = at; at = up(at + (size_t)B * groups * 4);
  l.has_start = at; at = up(at + (size_t)B * groups * 4);
  l.carry = at; at = up(at + (size_t)B * groups * 4);
  l.total = at;
  return l;
}

int ent_groups(int max_subseq, int subseq_bytes) {
  const int K = jpeg_entropy_group(subseq_bytes);
  return (max_subseq + K - 1) / K;
}

int check_entropy(const char* who, int32_t B, const uint8_t* bytes, int64_t bytes_len, const mmt_jpeg_image* images,
                  const mmt_jpeg_scan* scans, const uint32_t* huff, const int32_t* segments, int64_t n_segments, const int32_t* subseqs,
                  int64_t n_subseq, int32_t max_subseq, int32_t subseq_bytes, int32_t max_rounds, int16_t* coef, int64_t coef_elems,
                  int32_t* status, void* workspace, size_t workspace_bytes, EntParams& p) {
  if (B < 1 || B > 65535) return fail(B < 1 ? MMT_E_INVALID : MMT_E_UNSUPPORTED, "%s: B (%d) outside [1, 65535]", who, B);
  if (!bytes || !images || !scans || !huff || !segments || !subseqs || !coef || !status)
    return fail(MMT_E_INVALID, "%s: NULL argument (only the stream may be NULL)", who);
  if (subseq_bytes < 8 || subseq_bytes > 1024 || (subseq_bytes & (subseq_bytes - 1)))
    return fail(MMT_E_INVALID, "%s: subseq_bytes (%d) must be a power of two in [8, 1024]", who, subseq_bytes);
  if (max_rounds < 1 || max_rounds > 65536) return fail(MMT_E_INVALID, "%s: max_rounds (%d) outside [1, 65536]", who, max_rounds);
  if (bytes_len < 1 || bytes_len >= ((int64_t)1 << 40)) return fail(MMT_E_INVALID, "%s: bytes_len %lld outside [1, 2^40)", who, (long long)bytes_len);
  if (n_segments < 1 || n_segments >= ((int64_t)1 << 30) || n_subseq < 1 || n_subseq >= ((int64_t)1 << 30) || max_subseq < 1 || max_subseq > n_subseq)
    return fail(MMT_E_INVALID, "%s: n_segments %lld, n_subseq %lld in [1, 2^30) and max_subseq %d in [1, n_subseq] are required", who,
                (long long)n_segments, (long long)n_subseq, max_subseq);
  if (coef_elems < 64 || coef_elems >= ((int64_t)1 << 60)) return fail(MMT_E_INVALID, "%s: coef_elems %lld outside [64, 2^60)", who, (long long)coef_elems);
  if ((((uintptr_t)bytes | (uintptr_t)huff | (uintptr_t)coef | (uintptr_t)segments) & 15) != 0)
    return fail(MMT_E_INVALID, "%s: bytes, huff, segments and coef must be 16-byte aligned", who);
  if ((((uintptr_t)images | (uintptr_t)scans) & 7) != 0 || (((uintptr_t)subseqs | (uintptr_t)status) & 3) != 0)
    return fail(MMT_E_INVALID, "%s: images and scans must be 8-byte, subseqs and status 4-byte aligned", who);
  const int groups = ent_groups(max_subseq, subseq_bytes);
  if (groups > 65535 * 16) return fail(MMT_E_UNSUPPORTED, "%s: %d groups per image are too many", who, groups);
  const EntLayout l = ent_layout(B, n_subseq, groups, max_rounds);
  if (!workspace || workspace_bytes < l.total)
    return fail(MMT_E_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", who, l.total, workspace ? workspace_bytes : (size_t)0);
  if (((uintptr_t)workspace & 15) != 0) return fail(MMT_E_INVALID, "%s: workspace must be 16-byte aligned", who);
  char* w = (char*)workspace;
  p.B = B; p.groups = groups; p.K = jpeg_entropy_group(subseq_bytes); p.subseq_bytes = subseq_bytes; p.max_subseq = max_subseq;
  p.max_rounds = max_rounds; p.round = 0;
  p.bytes = bytes; p.bytes_len = bytes_len; p.images = images; p.scans = scans; p.huff = huff; p.segments = segments;
  p.n_segments = n_segments; p.subseqs = subseqs; p.n_subseq = n_subseq; p.coef = coef; p.coef_elems = coef_elems; p.status = status;
  p.changed = (int*)(w + l.changed); p.entry = (EntState*)(w + l.entry); p.exit_ = (EntState*)(w + l.exit_);
  p.slots = (unsigned*)(w + l.slots); p.edge = (EntState*)(w + l.edge); p.tail = (unsigned*)(w + l.tail);
  p.has_start = (int*)(w + l.has_start); p.carry = (unsigned*)(w + l.carry);
  return MMT_OK;
}

// What the clear pass gives the status word: a plan without segments or subsequences, or with more than the call takes.
__host__ __device__ inline int ent_plan_status(const EntImage& im) {
  return im.nseg < 1 || im.nsub < 1 || im.cut ? MMT_JPEG_ST_BLOCKS : MMT_JPEG_ST_OK;
}

// What the end of a segment and of the scan must look like, for the lane that owns the segment's last subsequence.
__host__ __device__ inline int ent_end_status(const EntImage& im, const EntSub& sub, int i, unsigned slot_end, unsigned slots_max) {
  int err = 0;
  if (slot_end != slots_max) err = (slot_end & 63u) ? MMT_JPEG_ST_OVERRUN : MMT_JPEG_ST_BLOCKS;
  if (i == im.nsub - 1 && sub.first_mcu + sub.n_mcu != im.mcus && err < MMT_JPEG_ST_BLOCKS) err = MMT_JPEG_ST_BLOCKS;
  return err;
}

// Block (bx, by) of scan-order element e of component c; false when it lies outside the grid.  Also whether the DC
// prediction starts anew there.
__host__ __device__ inline bool ent_dc_place(const EntImage& im, const JpegGeom& g, int c, int e, long& addr, bool& reset) {
  const int per = c == 0 ? im.hv : 1;
  const int m = e / per, j = e - m * per;
  reset = j == 0 && (im.ri > 0 ? m % im.ri == 0 : m == 0);
  const int my = m / im.mcus_x, mx = m - my * im.mcus_x;
  const int bx = c == 0 && g.nc == 3 ? mx * g.hs + j % g.hs : mx;
  const int by = c == 0 && g.nc == 3 ? my * g.vs + j / g.hs : my;
  const int bw = ent_pick3(g.bw, c), bh = ent_pick3(g.bh, c);
  addr = ent_pick3(g.off, c) + ((long)by * bw + bx) * 64;
  return bx < bw && by < bh;
}

}  // namespace

#ifndef MMT_JPEG_HOST_ONLY
namespace {

__device__ const unsigned char kZigzagDevice[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Inclusive segmented sum over the workgroup: v[t] becomes the sum from the last flagged lane at or before t (or lane
// 0), f[t] whether there is one.
__device__ inline void ent_scan(unsigned* v, int* f, int t) {
  for (int off = 1; off < kEntThreads; off <<= 1) {
    unsigned a = v[t];
    int h = f[t];
    if (t >= off && !h) { a += v[t - off]; h = f[t - off]; }
    __syncthreads();
    v[t] = a; f[t] = h;
    __syncthreads();
  }
}

// The bytes of a group's subsequences (scan bytes [first_begin - 1, last_end + kEntSlack), cut to the scan and to the
// window) with 16-byte loads where the buffer allows; returns the scan position of win[0] and the staged end.
__device__ inline void ent_stage(const EntParams& p, const EntImage& im, int first_begin, int last_end, unsigned char* win, int win_bytes,
                                 int pad_shift, int t, int& org, int& lim) {
  const long a0 = (im.base + (first_begin > 0 ? first_begin - 1 : 0)) & ~15L;
  long a1 = im.base + last_end + kEntSlack;
  if (a1 > im.base + im.count) a1 = im.base + im.count;
  const int len = (int)jclampl(a1 - a0, 0, win_bytes);
  for (int i = t * 16; i < len; i += kEntThreads * 16) {
    const long a = a0 + i;
    unsigned* dst = reinterpret_cast<unsigned*>(win + ent_padded(i, pad_shift));      // 16 bytes never straddle a padding word
    if (a + 16 <= p.bytes_len) {
      const uint4 v = *reinterpret_cast<const uint4*>(p.bytes + a);
      dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    } else {
      for (int j = 0; j < 16; ++j) reinterpret_cast<unsigned char*>(dst)[j] = a + j < p.bytes_len ? p.bytes[a + j] : (unsigned char)0;
    }
  }
  org = (int)(a0 - im.base);
  lim = org + len;
}

__device__ inline void ent_stage_tables(const EntParams& p, int b, unsigned* tabs, unsigned char* zz, int t) {
  const uint4* src = reinterpret_cast<const uint4*>(p.huff + (size_t)b * 6 * kHuffWords);
  for (int i = t; i < 6 * kHuffWords / 4; i += kEntThreads) reinterpret_cast<uint4*>(tabs)[i] = src[i];
  if (t < 64) zz[t] = kZigzagDevice[t];
}

// A stored state as one 8-byte load into two registers.
__device__ inline EntState ent_get(const EntState* a) {
  const int2 v = *reinterpret_cast<const int2*>(a);
  EntState s;
  s.p = v.x; s.bz = v.y;
  return s;
}

__global__ __launch_bounds__(256) void ent_clear_kernel(const EntParams p) {
  const int b = blockIdx.y, t = threadIdx.x;
  const JpegGeom g = jpeg_geom(p.images[b], p.coef_elems, 3);
  for (int c = 0; c < g.nc; ++c) {
    const long n = (long)ent_pick3(g.nblk, c) * 64, off = ent_pick3(g.off, c);
    for (long i = ((long)blockIdx.x * kEntThreads + t) * 8; i < n; i += (long)gridDim.x * kEntThreads * 8)
      if (off + i + 8 <= p.coef_elems) *reinterpret_cast<uint4*>(p.coef + off + i) = make_uint4(0, 0, 0, 0);
  }
  if (blockIdx.x == 0) {
    if (t == 0) p.status[b] = ent_plan_status(ent_image(p.scans[b], g, p));
    for (int r = t; r < p.max_rounds; r += kEntThreads) p.changed[(size_t)r * p.B + b] = 0;
  }
}

__global__ __launch_bounds__(256) void ent_round_kernel(const EntParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char win[];
  __shared__ __attribute__((aligned(16))) unsigned tabs[6 * kHuffWords];
  __shared__ unsigned char zz[64];
  __shared__ EntState xs[kEntThreads];
  __shared__ int sh[4];
  const int b = blockIdx.y, grp = blockIdx.x, t = threadIdx.x, r = p.round;
  const JpegGeom g = jpeg_geom(p.images[b], p.coef_elems, 3);
  const EntImage im = ent_image(p.scans[b], g, p);
  const int s0 = grp * p.K;
  if (s0 >= im.nsub) return;
  const int nl = im.nsub - s0 < p.K ? im.nsub - s0 : p.K;
  const bool live = t < nl;
  const int i = live ? s0 + t : s0;
  const EntSub sub = ent_sub(im, p, i);
  const size_t w = (size_t)b * p.groups + grp, half = (size_t)p.B * p.groups;
  const bool known = sub.first || (t == 0 && grp == 0);          // the entry state is no neighbour's
  EntState outer = ent_start(sub);                              // lane 0: what the group to the left reached last round
  if (r > 0 && grp > 0) outer = ent_get(p.edge + (size_t)((r - 1) & 1) * half + w - 1);
  if (r > 0) {
    if (t == 0) {
      const EntState ne = known ? ent_start(sub) : outer;
      const bool same = !(ne != ent_get(p.entry + im.sub0 + s0));
      sh[0] = same;
      if (same) p.edge[(size_t)(r & 1) * half + w] = ent_get(p.exit_ + im.sub0 + s0 + nl - 1);
    }
    __syncthreads();
    if (sh[0]) return;                                          // nothing inside the group can change
  }
  if (t == 0) sh[1] = sub.begin;
  if (t == nl - 1) sh[2] = sub.end;
  __syncthreads();
  int org, lim;
  const int pad_shift = jpeg_entropy_pad_shift(p.subseq_bytes);
  ent_stage(p, im, sh[1], sh[2], win, jpeg_entropy_window(p.subseq_bytes) & ~15, pad_shift, t, org, lim);
  ent_stage_tables(p, b, tabs, zz, t);
  EntState e = ent_start(sub), x = e;
  unsigned n = 0;
  if (r > 0 && live) { e = ent_get(p.entry + im.sub0 + i); x = ent_get(p.exit_ + im.sub0 + i); n = p.slots[im.sub0 + i]; }
  xs[t] = x;
  __syncthreads();
  const EntSink none = {nullptr, 0, 0u, 0u, 0};
  bool dirty = false;
  for (int it = 0; it <= p.K; ++it) {
    bool ch = false;
    if (live) {
      const bool fresh = r == 0 && it == 0;
      const EntState ne = known || fresh ? ent_start(sub) : (t == 0 ? outer : ent_get(xs + t - 1));
      if (fresh || ne != e) {
        e = ne; x = e; n = 0;
        int err = 0;
        if (sub.live) n = ent_decode<false>(win, org, pad_shift, lim, sub, e, tabs, zz, im, g, none, x, err);
        ch = true;
      }
    }
    __syncthreads();                                            // every lane has read its neighbour
    if (ch) { xs[t] = x; dirty = true; }
    if (!__syncthreads_or(ch)) break;
  }
  if (dirty) { p.entry[im.sub0 + i] = e; p.exit_[im.sub0 + i] = x; p.slots[im.sub0 + i] = n; }
  if (t == nl - 1) p.edge[(size_t)(r & 1) * half + w] = x;
  if (t == 0) p.changed[(size_t)r * p.B + b] = 1;               // round 0 decodes everything; later a group gets here by a change
}

__global__ __launch_bounds__(256) void ent_sums_kernel(const EntParams p) {
  __shared__ unsigned sv[kEntThreads];
  __shared__ int sf[kEntThreads];
  const int b = blockIdx.y, grp = blockIdx.x, t = threadIdx.x;
  const JpegGeom g = jpeg_geom(p.images[b], p.coef_elems, 3);
  const EntImage im = ent_image(p.scans[b], g, p);
  const int s0 = grp * p.K;
  if (s0 >= im.nsub) return;
  const int nl = im.nsub - s0 < p.K ? im.nsub - s0 : p.K;
  const bool live = t < nl;
  const EntSub sub = ent_sub(im, p, live ? s0 + t : s0);
  sv[t] = live ? p.slots[im.sub0 + s0 + t] : 0u;
  sf[t] = live && sub.first;
  __syncthreads();
  ent_scan(sv, sf, t);
  if (t == 0) {
    p.tail[(size_t)b * p.groups + grp] = sv[nl - 1];
    p.has_start[(size_t)b * p.groups + grp] = sf[nl - 1];
  }
}

__global__ __launch_bounds__(256) void ent_carry_kernel(const EntParams p) {
  __shared__ unsigned sv[kEntThreads];
  __shared__ int sf[kEntThreads];
  const int b = blockIdx.x, t = threadIdx.x;
  const JpegGeom g = jpeg_geom(p.images[b], p.coef_elems, 3);
  const EntImage im = ent_image(p.scans[b], g, p);
  const int ng = (im.nsub + p.K - 1) / p.K;                     // <= groups
  unsigned c = 0;                                               // lane 0 carries it
  for (int g0 = 0; g0 < ng; g0 += kEntThreads) {
    if (g0 + t < ng) { sv[t] = p.tail[(size_t)b * p.groups + g0 + t]; sf[t] = p.has_start[(size_t)b * p.groups + g0 + t]; }
    __syncthreads();
    if (t == 0)
      for (int k = 0; k < kEntThreads && g0 + k < ng; ++k) {
        p.carry[(size_t)b * p.groups + g0 + k] = c;
        c = sf[k] ? sv[k] : c + sv[k];
      }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void ent_write_kernel(const EntParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char win[];
  __shared__ __attribute__((aligned(16))) unsigned tabs[6 * kHuffWords];
  __shared__ unsigned char zz[64];
  __shared__ unsigned sv[kEntThreads];
  __shared__ int sf[kEntThreads];
  __shared__ int sh[4];
  const int b = blockIdx.y, grp = blockIdx.x, t = threadIdx.x;
  const JpegGeom g = jpeg_geom(p.images[b], p.coef_elems, 3);
  const EntImage im = ent_image(p.scans[b], g, p);
  const int s0 = grp * p.K;
  if (s0 >= im.nsub) return;
  const int nl = im.nsub - s0 < p.K ? im.nsub - s0 : p.K;
  const bool live = t < nl;
  const int i = live ? s0 + t : s0;
  const EntSub sub = ent_sub(im, p, i);
  if (t == 0) sh[1] = sub.begin;
  if (t == nl - 1) sh[2] = sub.end;
  const unsigned n = live ? p.slots[im.sub0 + i] : 0u;
  sv[t] = n;
  sf[t] = live && sub.first;
  __syncthreads();
  int org, lim;
  const int pad_shift = jpeg_entropy_pad_shift(p.subseq_bytes);
  ent_stage(p, im, sh[1], sh[2], win, jpeg_entropy_window(p.subseq_bytes) & ~15, pad_shift, t, org, lim);
  ent_stage_tables(p, b, tabs, zz, t);
  ent_scan(sv, sf, t);                                          // ends with a barrier: the window and the tables are staged too
  if (!live) return;
  int err = 0;
  const EntState e = ent_get(p.entry + im.sub0 + i);
  const bool known = sub.first || i == 0;
  if (!known && ent_get(p.exit_ + im.sub0 + i - 1) != e) err = MMT_JPEG_ST_NOT_CONVERGED;
  const unsigned slot0 = sv[t] - n + (sf[t] ? 0u : p.carry[(size_t)b * p.groups + grp]);
  const unsigned slots_max = (unsigned)sub.n_mcu * (unsigned)im.bpm * 64u;
  const EntSink sink = {p.coef, p.coef_elems, slot0, slots_max, sub.first_mcu};
  EntState x = e;
  unsigned got = 0;
  if (sub.live) got = ent_decode<true>(win, org, pad_shift, lim, sub, e, tabs, zz, im, g, sink, x, err);
  if (sub.last) {
    const int end = ent_end_status(im, sub, i, slot0 + got, slots_max);
    if (end > err) err = end;
  }
  if (err) atomicMax(p.status + b, err);
}

constexpr int kDcPerLane = 8;

__global__ __launch_bounds__(256) void ent_dc_kernel(const EntParams p) {
  __shared__ unsigned sv[kEntThreads];
  __shared__ int sf[kEntThreads];
  __shared__ unsigned carry_sh;
  const int b = blockIdx.y, c = blockIdx.x, t = threadIdx.x;
  const JpegGeom g = jpeg_geom(p.images[b], p.coef_elems, 3);
  if (c >= g.nc) return;
  const EntImage im = ent_image(p.scans[b], g, p);
  const int total = im.mcus * (c == 0 ? im.hv : 1);             // <= 2^28
  if (t == 0) carry_sh = 0;
  __syncthreads();
  for (int c0 = 0; c0 < total; c0 += kEntThreads * kDcPerLane) {
    const int e0 = c0 + t * kDcPerLane;
    unsigned sum = 0;
    int flag = 0;
    unsigned v[kDcPerLane];
#pragma unroll
    for (int k = 0; k < kDcPerLane; ++k) {
      long addr = 0;
      bool reset = false;
      int d = 0;
      if (e0 + k < total) {
        const bool inside = ent_dc_place(im, g, c, e0 + k, addr, reset);
        if (inside && addr < p.coef_elems) d = p.coef[addr];
      }
      if (reset) { sum = 0; flag = 1; }
      sum += (unsigned)d;
      v[k] = sum;
    }
    const unsigned carry = carry_sh;
    sv[t] = sum; sf[t] = flag;
    __syncthreads();
    ent_scan(sv, sf, t);
    unsigned add = t > 0 ? (sf[t - 1] ? sv[t - 1] : sv[t - 1] + carry) : carry;
    const unsigned next = sf[kEntThreads - 1] ? sv[kEntThreads - 1] : sv[kEntThreads - 1] + carry;
#pragma unroll
    for (int k = 0; k < kDcPerLane; ++k) {
      if (e0 + k < total) {
        long addr = 0;
        bool reset = false;
        const bool inside = ent_dc_place(im, g, c, e0 + k, addr, reset);
        if (reset) add = 0;
        if (inside && addr < p.coef_elems) p.coef[addr] = (short)(v[k] + add);
      }
    }
    __syncthreads();
    if (t == 0) carry_sh = next;
    __syncthreads();
  }
}

}  // namespace

hipError_t launch_jpeg_entropy(EntParams p, hipStream_t st) {
  const dim3 grid((unsigned)p.groups, (unsigned)p.B), block(kEntThreads);
  const size_t lds = (size_t)jpeg_entropy_lds_bytes(p.subseq_bytes);
  // about one workgroup per 16 Ki coefficients of an image of average size, between 8 and 256 per image
  const long per_image = p.coef_elems / p.B / (kEntThreads * 8 * 8);
  const int parts = per_image < 8 ? 8 : (per_image > 256 ? 256 : (int)per_image);
  hipLaunchKernelGGL(ent_clear_kernel, dim3((unsigned)parts, (unsigned)p.B), block, 0, st, p);
  for (int r = 0; r < p.max_rounds; ++r) {
    p.round = r;
    hipLaunchKernelGGL(ent_round_kernel, grid, block, lds, st, p);
  }
  hipLaunchKernelGGL(ent_sums_kernel, grid, block, 0, st, p);
  hipLaunchKernelGGL(ent_carry_kernel, dim3((unsigned)p.B), block, 0, st, p);
  hipLaunchKernelGGL(ent_write_kernel, grid, block, lds, st, p);
  hipLaunchKernelGGL(ent_dc_kernel, dim3(3, (unsigned)p.B), block, 0, st, p);
  return hipGetLastError();
}
#endif  // MMT_JPEG_HOST_ONLY

}  // namespace mmt

extern "C" {

size_t mmt_jpeg_entropy_workspace_bytes(int32_t B, int64_t n_subseq, int32_t max_subseq, int32_t subseq_bytes, int32_t max_rounds) {
  if (B < 1 || B > 65535 || n_subseq < 1 || n_subseq >= ((int64_t)1 << 30) || max_subseq < 1 || max_subseq > n_subseq || subseq_bytes < 8 ||
      subseq_bytes > 1024 || (subseq_bytes & (subseq_bytes - 1)) || max_rounds < 1 || max_rounds > 65536)
    return 0;
  return mmt::ent_layout(B, n_subseq, mmt::ent_groups(max_subseq, subseq_bytes), max_rounds).total;
}

int mmt_jpeg_entropy_host(int32_t B, const uint8_t* bytes, int64_t bytes_len, const mmt_jpeg_image* images, const mmt_jpeg_scan* scans,
                          const uint32_t* huff, const int32_t* segments, int64_t n_segments, const int32_t* subseqs, int64_t n_subseq,
                          int32_t max_subseq, int32_t subseq_bytes, int32_t max_rounds, int16_t* coef, int64_t coef_elems, int32_t* status,
                          void* workspace, size_t workspace_bytes) {
  using namespace mmt;
  EntParams p;
  const int rc = check_entropy("mmt_jpeg_entropy_host", B, bytes, bytes_len, images, scans, huff, segments, n_segments, subseqs, n_subseq,
                               max_subseq, subseq_bytes, max_rounds, coef, coef_elems, status, workspace, workspace_bytes, p);
  if (rc) return rc;
  const size_t half = (size_t)B * p.groups;
  const EntSink none = {nullptr, 0, 0u, 0u, 0};
  for (int b = 0; b < B; ++b) {
    const JpegGeom g = jpeg_geom(images[b], coef_elems, 3);
    const EntImage im = ent_image(scans[b], g, p);
    const unsigned char* d = bytes + im.base;
    const unsigned* tabs = huff + (size_t)b * 6 * kHuffWords;
    const int ng = (im.nsub + p.K - 1) / p.K;
    // 1. clear
    for (int c = 0; c < g.nc; ++c)
      for (long i = 0; i < (long)g.nblk[c] * 64; i += 8)
        if (g.off[c] + i + 8 <= coef_elems) std::memset(coef + g.off[c] + i, 0, 16);
    status[b] = ent_plan_status(im);
    for (int r = 0; r < max_rounds; ++r) p.changed[(size_t)r * B + b] = 0;
    // 2. rounds: a group's lanes one after the other reach the state the workgroup's passes end in
    for (int r = 0; r < max_rounds; ++r)
      for (int grp = 0; grp < ng; ++grp) {
        const int s0 = grp * p.K, nl = im.nsub - s0 < p.K ? im.nsub - s0 : p.K;
        const size_t w = (size_t)b * p.groups + grp;
        const EntSub head = ent_sub(im, p, s0);
        EntState outer = ent_start(head);
        if (r > 0 && grp > 0) outer = p.edge[(size_t)((r - 1) & 1) * half + w - 1];
        if (r > 0) {
          const EntState ne = head.first || grp == 0 ? ent_start(head) : outer;
          if (!(ne != p.entry[im.sub0 + s0])) { p.edge[(size_t)(r & 1) * half + w] = p.exit_[im.sub0 + s0 + nl - 1]; continue; }
        }
        for (int t = 0; t < nl; ++t) {
          const int i = s0 + t;
          const EntSub sub = ent_sub(im, p, i);
          const bool known = sub.first || (t == 0 && grp == 0);
          const EntState ne = known ? ent_start(sub) : (t == 0 ? outer : p.exit_[im.sub0 + i - 1]);
          if (r == 0 || ne != p.entry[im.sub0 + i]) {
            EntState x = ne;
            unsigned n = 0;
            int err = 0;
            if (sub.live) n = ent_decode<false>(d, 0, 31, im.count, sub, ne, tabs, kZigzagHost, im, g, none, x, err);
            p.entry[im.sub0 + i] = ne; p.exit_[im.sub0 + i] = x; p.slots[im.sub0 + i] = n;
          }
        }
        p.edge[(size_t)(r & 1) * half + w] = p.exit_[im.sub0 + s0 + nl - 1];
        p.changed[(size_t)r * B + b] = 1;
      }
    // 3. - 5. offsets and the write pass
    unsigned run = 0;
    int worst = 0;
    for (int i = 0; i < im.nsub; ++i) {
      const EntSub sub = ent_sub(im, p, i);
      if (sub.first) run = 0;
      int err = 0;
      const EntState e = p.entry[im.sub0 + i];
      if (!(sub.first || i == 0) && p.exit_[im.sub0 + i - 1] != e) err = MMT_JPEG_ST_NOT_CONVERGED;
      const unsigned slots_max = (unsigned)sub.n_mcu * (unsigned)im.bpm * 64u;
      const EntSink sink = {coef, coef_elems, run, slots_max, sub.first_mcu};
      EntState x = e;
      unsigned got = 0;
      if (sub.live) got = ent_decode<true>(d, 0, 31, im.count, sub, e, tabs, kZigzagHost, im, g, sink, x, err);
      if (sub.last) {
        const int end = ent_end_status(im, sub, i, run + got, slots_max);
        if (end > err) err = end;
      }
      run += p.slots[im.sub0 + i];
      if (err > worst) worst = err;
    }
    if (worst > status[b]) status[b] = worst;
    // 6. DC prediction
    for (int c = 0; c < g.nc; ++c) {
      const int total = im.mcus * (c == 0 ? im.hv : 1);
      unsigned sum = 0;
      for (int e = 0; e < total; ++e) {
        long addr = 0;
        bool reset = false;
        const bool inside = ent_dc_place(im, g, c, e, addr, reset);
        if (reset) sum = 0;
        if (inside && addr < coef_elems) {
          sum += (unsigned)(int)coef[addr];
          coef[addr] = (short)sum;
        }
      }
    }
  }
  return MMT_OK;
}

#ifndef MMT_JPEG_HOST_ONLY
int mmt_jpeg_entropy(int32_t B, const uint8_t* bytes, int64_t bytes_len, const mmt_jpeg_image* images, const mmt_jpeg_scan* scans,
                     const uint32_t* huff, const int32_t* segments, int64_t n_segments, const int32_t* subseqs, int64_t n_subseq,
                     int32_t max_subseq, int32_t subseq_bytes, int32_t max_rounds, int16_t* coef, int64_t coef_elems, int32_t* status,
                     void* workspace, size_t workspace_bytes, void* stream) {
  mmt::EntParams p;
  const int rc = mmt::check_entropy("mmt_jpeg_entropy", B, bytes, bytes_len, images, scans, huff, segments, n_segments, subseqs, n_subseq,
                                    max_subseq, subseq_bytes, max_rounds, coef, coef_elems, status, workspace, workspace_bytes, p);
  if (rc) return rc;
  const hipError_t e = mmt::launch_jpeg_entropy(p, (hipStream_t)stream);
  return e == hipSuccess ? MMT_OK : mmt::fail(MMT_E_LAUNCH, "mmt_jpeg_entropy: %s", hipGetErrorString(e));
}
#endif

}  // extern "C"
