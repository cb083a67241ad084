// Inflate of a PNG's zlib stream by a group of 256 lanes (png_inflate.hip; DESIGN.md section 4 "PNG inflate on the
// device"): the functions the kernel and the host loop both run -- the bit reader over a staged window of compressed
// bytes, the Huffman table build (zlib's rules), the token decode, one lane's speculative walk, the rule that decides
// when an LZ77 copy may be made (a mark per lane), the Adler-32 combine -- and inf_image(), the rounds of one image written once over
// MMT_INF_LANES: on the device the body runs for the calling thread and ends in __syncthreads(); on the host it is a loop
// over the 256 lanes.  A value that lanes exchange lives in InfGroup (LDS on the device) and is written in one section
// and read after it; a field that uniform code reads behind a section is never written in the section that follows.
// Everything is integer.  No access leaves [comp, comp + comp_n) or [out, out + cap); every loop is bounded by those
// sizes or by a constant (the bounds are stated where the loops are).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mmt_layer.h"
#include "png_decode.h"

namespace mmt {

constexpr int kInfLanes = 256;
constexpr int kInfFast = 10;                                    // bits of the lookup in front of the canonical walk
constexpr int kInfMinSubseq = 8, kInfMaxSubseq = 128;           // bytes a lane owns in a round
constexpr int kInfStageWords = kInfLanes * kInfMaxSubseq / 4 + 4;
constexpr int kInfHeaderWords = 256;                            // a block header is at most 3 + 14 + 57 + 316 * 14 = 4498 bits
constexpr uint32_t kAdlerMod = 65521u;

enum { kTokLiteral = 0, kTokMatch = 1, kTokEnd = 2, kTokBad = 3 };
enum { kExitCont = 0, kExitEnd = 1, kExitBad = 2 };

#if defined(__HIP_DEVICE_COMPILE__)
#define MMT_INF_LANES(lane) for (int lane = (int)threadIdx.x, once_ = 1; once_; once_ = 0, __syncthreads())
#else
#define MMT_INF_LANES(lane) for (int lane = 0; lane < kInfLanes; ++lane)
#endif

struct InfHuff {
  uint16_t fast[1 << kInfFast];         // symbol | length << 9 for codes of at most kInfFast bits, 0 otherwise
  uint16_t count[16];
  uint16_t offs[16];                    // scratch of the build
  uint16_t symbol[288];                 // the symbols sorted by code length, then by value
  int total;                            // symbols with a code
};

struct InfBlock {                       // what lane 0 reads from a block header
  int status, last, type;
  int after;                            // first bit behind the header, from the staged window's first byte
  long stored_from, stored_n;           // a stored block's bytes: [stored_from, stored_from + stored_n) of the stream
  int nlen, ndist;
  uint8_t cl[19];
  uint8_t lens[288 + 32];
};

struct InfTok { int kind, bits, value, dist, err; };            // value: the literal, or the length of a match
struct InfExit { int exit, kind, err, ntok, nout; };

struct InfGroup {
  uint32_t stage[kInfStageWords];       // the compressed bytes of a round, little endian, zero behind the stream
  InfHuff lit, dist;
  InfBlock blk;
  int entry[kInfLanes], has[kInfLanes];                         // a lane's first bit, and whether it is on the chain
  int exit[kInfLanes], kind[kInfLanes], err[kInfLanes], ntok[kInfLanes], nout[kInfLanes];
  int want_entry[kInfLanes], flag[kInfLanes];
  int scan[2][kInfLanes];
  int own[kInfLanes];                                           // first output byte of the lane, from the round's first
  int cur_p[kInfLanes], cur_left[kInfLanes], cur_dst[kInfLanes];// the lane's next unresolved match: bit, tokens left, dst
  int fin[kInfLanes];                                           // cur_dst as the last barrier left it
  int red[4];
  int end_exit, end_kind, end_err;
  int build_status;
  uint32_t adler;
};

// ---------------------------------------------------------------------------------------------------------------------
// Reader.  The staged window holds the stream from byte `base` on; a bit position is relative to that byte.
// ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t inf_stage_word(const uint8_t* comp, long comp_n, long byte) {
  uint32_t w = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long at = byte + k;
    if (at >= 0 && at < comp_n) w |= (uint32_t)comp[at] << (8 * k);
  }
  return w;
}

// 64 bits from bit p on.  Reads words p / 32 .. p / 32 + 2.
__host__ __device__ inline uint64_t inf_window(const uint32_t* stage, int p) {
  const int q = p >> 5, s = p & 31;
  const uint64_t lo = (uint64_t)stage[q] | (uint64_t)stage[q + 1] << 32;
  return s ? (lo >> s) | ((uint64_t)stage[q + 2] << (64 - s)) : lo;
}

// ---------------------------------------------------------------------------------------------------------------------
// Tables: zlib's rule -- an over-subscribed set is invalid; an incomplete one too, unless it is a single code of one bit
// (or no code at all).  inf_build_counts is serial; inf_fill_fast takes one sorted symbol, so lanes share the fill.
// ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int inf_build_counts(InfHuff& h, const uint8_t* lengths, int n) {
  for (int l = 0; l < 16; ++l) h.count[l] = 0;
  for (int i = 0; i < n; ++i) h.count[lengths[i] & 15]++;
  h.count[0] = 0;
  int left = 1, longest = 0, total = 0;
  for (int l = 1; l <= 15; ++l) {
    left = (left << 1) - h.count[l];
    if (left < 0) return MMT_PNG_ST_CODE_LENGTHS;
    if (h.count[l]) longest = l;
    total += h.count[l];
  }
  if (left > 0 && longest > 1) return MMT_PNG_ST_CODE_LENGTHS;
  h.offs[0] = 0; h.offs[1] = 0;
  for (int l = 1; l < 15; ++l) h.offs[l + 1] = (uint16_t)(h.offs[l] + h.count[l]);
  for (int i = 0; i < n; ++i) {
    const int l = lengths[i] & 15;
    if (l) h.symbol[h.offs[l]++] = (uint16_t)i;
  }
  h.total = total;
  return 0;
}

__host__ __device__ inline void inf_fill_fast(InfHuff& h, int j) {                // j < h.total
  int l = 1, first = 0;
  unsigned code = 0;
  for (; l < 15; ++l) {                                                           // the length of sorted symbol j, its first code
    code = (code + (l > 1 ? h.count[l - 1] : 0u)) << 1;
    if (j < first + h.count[l]) break;
    first += h.count[l];
  }
  if (l == 15) code = (code + h.count[14]) << 1;
  if (l > kInfFast) return;
  const unsigned cd = code + (unsigned)(j - first);
  unsigned rev = 0;
  for (int k = 0; k < l; ++k) rev |= ((cd >> k) & 1u) << (l - 1 - k);
  const uint16_t e = (uint16_t)(h.symbol[j] | (l << 9));
  for (unsigned at = rev & ((1u << kInfFast) - 1u); at < (1u << kInfFast); at += 1u << l) h.fast[at] = e;
}

__host__ __device__ inline int inf_symbol_slow(const InfHuff& h, uint64_t& w, int& used) {
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= 15; ++l) {
    code |= (int)((w >> (l - 1)) & 1u);
    const int cnt = h.count[l];
    if (code - cnt < first) { w >>= l; used += l; return h.symbol[index + (code - first)]; }
    index += cnt; first += cnt; first <<= 1; code <<= 1;
  }
  used += 15;
  return -1;
}

__host__ __device__ inline int inf_symbol(const InfHuff& h, uint64_t& w, int& used) {
  const unsigned e = h.fast[w & ((1u << kInfFast) - 1u)];
  if (e) { w >>= e >> 9; used += (int)(e >> 9); return (int)(e & 511u); }
  return inf_symbol_slow(h, w, used);
}

// Length symbol s - 257 in 0..28 and distance symbol 0..29: base and extra bits, RFC 1951 section 3.2.5 as arithmetic.
__host__ __device__ inline int inf_len_extra(int s) { return s < 8 || s == 28 ? 0 : (s - 4) >> 2; }
__host__ __device__ inline int inf_len_base(int s) { return s < 8 ? 3 + s : (s == 28 ? 258 : 3 + ((4 + (s & 3)) << ((s - 4) >> 2))); }
__host__ __device__ inline int inf_dist_extra(int s) { return s < 4 ? 0 : (s - 2) >> 1; }
__host__ __device__ inline int inf_dist_base(int s) { return s < 4 ? 1 + s : 1 + ((2 + (s & 1)) << ((s - 2) >> 1)); }

// One token from the 64 bits w: at most 15 + 5 + 15 + 13 = 48 of them.
__host__ __device__ inline InfTok inf_token(const InfHuff& lit, const InfHuff& dist, uint64_t w) {
  InfTok t;
  t.bits = 0; t.dist = 0; t.err = 0; t.value = 0;
  int sym = inf_symbol(lit, w, t.bits);
  if (sym < 0) { t.kind = kTokBad; t.err = MMT_PNG_ST_BAD_CODE; return t; }
  if (sym < 256) { t.kind = kTokLiteral; t.value = sym; return t; }
  if (sym == 256) { t.kind = kTokEnd; return t; }
  sym -= 257;
  if (sym >= 29) { t.kind = kTokBad; t.err = MMT_PNG_ST_BAD_CODE; return t; }
  const int le = inf_len_extra(sym);
  t.value = inf_len_base(sym) + (int)(w & ((1u << le) - 1u));
  w >>= le; t.bits += le;
  const int ds = inf_symbol(dist, w, t.bits);
  if (ds < 0 || ds >= 30) { t.kind = kTokBad; t.err = MMT_PNG_ST_BAD_CODE; return t; }
  const int de = inf_dist_extra(ds);
  t.dist = inf_dist_base(ds) + (int)(w & ((1u << de) - 1u));
  t.bits += de;
  t.kind = kTokMatch;
  return t;
}

// One lane's walk: tokens from bit `entry` until one starts at or behind `end`, an end-of-block code, or a token that
// is invalid or used bits behind `avail` (padding).  At most end - entry tokens: a token has at least one bit.
__host__ __device__ inline InfExit inf_walk(const InfHuff& lit, const InfHuff& dist, const uint32_t* stage, int entry, int end, int avail) {
  InfExit x;
  x.kind = kExitCont; x.err = 0; x.ntok = 0; x.nout = 0;
  int p = entry;
  while (p < end) {
    const InfTok t = inf_token(lit, dist, inf_window(stage, p));
    if (p + t.bits > avail) { x.kind = kExitBad; x.err = MMT_PNG_ST_TRUNCATED; break; }
    if (t.kind == kTokBad) { x.kind = kExitBad; x.err = t.err; break; }
    p += t.bits;
    if (t.kind == kTokEnd) { x.kind = kExitEnd; break; }
    ++x.ntok;
    x.nout += t.kind == kTokLiteral ? 1 : t.value;
  }
  x.exit = p;
  return x;
}

// The resolution rule.  Positions count from the round's first output byte.  A match (dst, n, d) may be copied once every
// byte of [dst - d, dst - d + min(n, d)) is final.  Final are: everything in front of the round; [own, dst) of the lane
// itself (its literals are written and it copies its matches in order); and of any other lane k the bytes below fin[k],
// the dst of its first unresolved match as the last barrier left it (the end of the round's output once it has none) --
// the mark, kept per lane.  The smallest fin is the mark of the whole group: the lane that holds it finds every lane
// below it finished, so its matches always resolve.  own[] is ascending, own[k + 1] ends lane k.
__host__ __device__ inline bool inf_ready(const int* own, const int* fin, int lane, int dst, int n, int d) {
  long s0 = (long)dst - d, s1 = s0 + (n < d ? n : d);
  if (s0 < 0) s0 = 0;
  if (s1 > own[lane]) s1 = own[lane];                           // behind it: the lane's own bytes
  if (s0 >= s1) return true;
  int lo = 0, hi = lane;                                        // the lane that holds s0: the last with own[k] <= s0
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (own[mid] <= s0) lo = mid; else hi = mid;
  }
  for (int k = lo; k < lane; ++k) {                             // at most 256 lanes
    const long end = own[k + 1] < s1 ? own[k + 1] : s1;         // what the range needs of lane k
    if (fin[k] < end) return false;
    if (own[k + 1] >= s1) break;
  }
  return true;
}

// Adler-32 of a piece (at most 5552 bytes keep b inside 32 bits), and of two pieces that follow each other.
__host__ __device__ inline void inf_adler_piece(const uint8_t* p, int n, uint32_t& a, uint32_t& b) {
  for (int i = 0; i < n; ++i) { a += p[i]; b += a; }
  a %= kAdlerMod; b %= kAdlerMod;
}
__host__ __device__ inline void inf_adler_combine(uint32_t& a1, uint32_t& b1, uint32_t a2, uint32_t b2, long len2) {
  const uint64_t rem = (uint64_t)(len2 % (long)kAdlerMod);
  const uint64_t b = (uint64_t)b1 + b2 + rem * ((uint64_t)a1 + kAdlerMod - 1u);
  a1 = (uint32_t)(((uint64_t)a1 + a2 + kAdlerMod - 1u) % kAdlerMod);
  b1 = (uint32_t)(b % kAdlerMod);
}

// ---------------------------------------------------------------------------------------------------------------------
// Block header, by one lane.  cl is a table the group does not need yet (the code-length code lives in it).
// ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline unsigned inf_take(const uint32_t* stage, int& p, int k) {
  const unsigned v = (unsigned)(inf_window(stage, p) & ((1ull << k) - 1ull));
  p += k;
  return v;
}

__host__ __device__ inline void inf_header(const uint32_t* stage, int rel, int avail, long base, long comp_n, InfHuff& cl, InfBlock& b) {
  int p = rel;
  b.status = 0; b.stored_from = 0; b.stored_n = 0; b.nlen = 0; b.ndist = 0;
  b.last = (int)inf_take(stage, p, 1);
  b.type = (int)inf_take(stage, p, 2);
  b.after = p;
  if (p > avail) { b.status = MMT_PNG_ST_TRUNCATED; return; }
  if (b.type == 3) { b.status = MMT_PNG_ST_BLOCK_TYPE; return; }
  if (b.type == 0) {
    p = (p + 7) & ~7;
    if (p + 32 > avail) { b.status = MMT_PNG_ST_TRUNCATED; return; }
    const unsigned n = inf_take(stage, p, 16), inv = inf_take(stage, p, 16);
    if ((n ^ inv) != 0xffffu) { b.status = MMT_PNG_ST_STORED_LEN; return; }
    b.stored_from = base + (p >> 3);
    b.stored_n = n;
    if (b.stored_from + b.stored_n > comp_n) b.status = MMT_PNG_ST_TRUNCATED;
    return;
  }
  if (b.type == 1) {
    b.nlen = 288; b.ndist = 32;                                 // symbols 286, 287 and distances 30, 31 are refused by inf_token
    for (int i = 0; i < 288; ++i) b.lens[i] = (uint8_t)(i < 144 ? 8 : (i < 256 ? 9 : (i < 280 ? 7 : 8)));
    for (int i = 0; i < 32; ++i) b.lens[288 + i] = 5;
    return;
  }
  const int nlen = (int)inf_take(stage, p, 5) + 257, ndist = (int)inf_take(stage, p, 5) + 1, ncode = (int)inf_take(stage, p, 4) + 4;
  if (p > avail) { b.status = MMT_PNG_ST_TRUNCATED; return; }
  if (nlen > 286 || ndist > 30) { b.status = MMT_PNG_ST_CODE_LENGTHS; return; }
  for (int i = 0; i < 19; ++i) b.cl[i] = 0;
  for (int i = 0; i < ncode; ++i) b.cl[(unsigned char)"\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f"[i]] = (uint8_t)inf_take(stage, p, 3);
  if (p > avail) { b.status = MMT_PNG_ST_TRUNCATED; return; }
  int complete = 0;
  for (int i = 0; i < 19; ++i) if (b.cl[i]) complete += 1 << (7 - b.cl[i]);
  if (complete != 128 || inf_build_counts(cl, b.cl, 19)) { b.status = MMT_PNG_ST_CODE_LENGTHS; return; }
  int i = 0;
  while (i < nlen + ndist) {                                    // at most 316 symbols
    uint64_t w = inf_window(stage, p);
    int used = 0;
    const int sym = inf_symbol_slow(cl, w, used);
    if (sym < 0) { b.status = p + used > avail ? MMT_PNG_ST_TRUNCATED : MMT_PNG_ST_CODE_LENGTHS; return; }
    if (sym < 16) { b.lens[i++] = (uint8_t)sym; p += used; continue; }
    int rep, val = 0;
    if (sym == 16) {
      if (i == 0) { b.status = MMT_PNG_ST_CODE_LENGTHS; return; }
      val = b.lens[i - 1]; rep = 3 + (int)(w & 3u); used += 2;
    } else if (sym == 17) {
      rep = 3 + (int)(w & 7u); used += 3;
    } else {
      rep = 11 + (int)(w & 127u); used += 7;
    }
    p += used;
    if (p > avail) { b.status = MMT_PNG_ST_TRUNCATED; return; }
    if (i + rep > nlen + ndist) { b.status = MMT_PNG_ST_CODE_LENGTHS; return; }
    while (rep--) b.lens[i++] = (uint8_t)val;
  }
  if (p > avail) { b.status = MMT_PNG_ST_TRUNCATED; return; }
  if (b.lens[256] == 0) { b.status = MMT_PNG_ST_CODE_LENGTHS; return; }
  b.nlen = nlen; b.ndist = ndist;
  b.after = p;
}

// ---------------------------------------------------------------------------------------------------------------------
// Group operations: behind each, every lane holds the same result.
// ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int inf_any(InfGroup& g) {           // of g.flag[]
#if defined(__HIP_DEVICE_COMPILE__)
  return __syncthreads_or(g.flag[threadIdx.x]);
#else
  int any = 0;
  for (int i = 0; i < kInfLanes; ++i) any |= g.flag[i];
  return any;
#endif
}

__host__ __device__ inline int inf_min_dst(InfGroup& g) {       // of g.cur_dst[]
#if defined(__HIP_DEVICE_COMPILE__)
  int v = g.cur_dst[threadIdx.x];
  for (int o = 32; o; o >>= 1) { const int u = __shfl_xor(v, o); v = u < v ? u : v; }
  if ((threadIdx.x & 63) == 0) g.red[threadIdx.x >> 6] = v;
  __syncthreads();
  int m = g.red[0];
  for (int i = 1; i < 4; ++i) m = g.red[i] < m ? g.red[i] : m;
  __syncthreads();
  return m;
#else
  int m = g.cur_dst[0];
  for (int i = 1; i < kInfLanes; ++i) m = g.cur_dst[i] < m ? g.cur_dst[i] : m;
  return m;
#endif
}

__host__ __device__ inline void inf_scan(InfGroup& g) {         // g.scan[0][]: inclusive prefix sum in place
#if defined(__HIP_DEVICE_COMPILE__)
  const int t = threadIdx.x;
  int src = 0;
  for (int o = 1; o < kInfLanes; o <<= 1) {                     // 8 steps: the result is back in scan[0]
    g.scan[src ^ 1][t] = g.scan[src][t] + (t >= o ? g.scan[src][t - o] : 0);
    __syncthreads();
    src ^= 1;
  }
#else
  for (int i = 1; i < kInfLanes; ++i) g.scan[0][i] += g.scan[0][i - 1];
#endif
}

// The lane's cursor moves over literals (they are written) to its next match, or to the end of its tokens.
__host__ __device__ inline void inf_seek(InfGroup& g, int lane, int total) {
  int p = g.cur_p[lane], left = g.cur_left[lane], dst = g.cur_dst[lane];
  while (left > 0) {
    const InfTok t = inf_token(g.lit, g.dist, inf_window(g.stage, p));
    if (t.kind == kTokMatch) break;
    p += t.bits; ++dst; --left;
  }
  g.cur_p[lane] = p; g.cur_left[lane] = left; g.cur_dst[lane] = left > 0 ? dst : total;
}

// ---------------------------------------------------------------------------------------------------------------------
// One image: the zlib stream comp[0, comp_n) (header included) into out[0, cap); `want` is the exact length.  Returns the
// status, the same value on every lane.  S: bytes a lane owns in a round.
// ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int inf_image(InfGroup& g, const uint8_t* comp, long comp_n, uint8_t* out, long cap, long want, int S) {
  long lim = want < cap ? want : cap;
  if (lim < 0) lim = 0;
  long pos = 16, out_at = 0;                                    // bits of the stream taken, bytes written
  int in_block = 0, last = 0, done = 0;
  int status = comp_n < 6 ? MMT_PNG_ST_TRUNCATED : 0;           // the header, and the check value at the least
  // every round advances pos, and a round at or behind the stream's end fails: at most 8 * comp_n + 1 rounds
  while (!status && !done) {
    const long base = pos >> 3;
    const int rel = (int)(pos & 7);
    const int words = in_block ? 64 * S + 3 : kInfHeaderWords;
    MMT_INF_LANES(lane) {
      for (int j = lane; j < words; j += kInfLanes) g.stage[j] = inf_stage_word(comp, comp_n, base + 4 * (long)j);
    }
    const long left_bits = (comp_n - base) * 8;
    const int avail = left_bits < 0 ? 0 : (left_bits > (1 << 30) ? (1 << 30) : (int)left_bits);

    if (!in_block) {                                            // step 2: the block header
      MMT_INF_LANES(lane) {
        if (lane == 0) inf_header(g.stage, rel, avail, base, comp_n, g.lit, g.blk);
      }
      status = g.blk.status;
      if (status) break;
      last = g.blk.last;
      if (g.blk.type == 0) {
        const long from = g.blk.stored_from, n = g.blk.stored_n;
        if (n > lim - out_at) { status = MMT_PNG_ST_TOO_LONG; break; }
        MMT_INF_LANES(lane) {
          for (long k = lane; k < n; k += kInfLanes)
            if (from + k < comp_n && out_at + k < cap) out[out_at + k] = comp[from + k];
        }
        out_at += n;
        pos = (from + n) * 8;
        done = last;
        continue;
      }
      MMT_INF_LANES(lane) {
        if (lane == 0) {
          int st = inf_build_counts(g.lit, g.blk.lens, g.blk.nlen);
          if (!st) st = inf_build_counts(g.dist, g.blk.lens + g.blk.nlen, g.blk.ndist);
          g.build_status = st;
        }
        for (int j = lane; j < (1 << kInfFast); j += kInfLanes) { g.lit.fast[j] = 0; g.dist.fast[j] = 0; }
      }
      status = g.build_status;
      if (status) break;
      MMT_INF_LANES(lane) {
        for (int j = lane; j < g.lit.total; j += kInfLanes) inf_fill_fast(g.lit, j);
        for (int j = lane; j < g.dist.total; j += kInfLanes) inf_fill_fast(g.dist, j);
      }
      pos = base * 8 + g.blk.after;
      in_block = 1;
      continue;
    }

    // step 3: the speculative walk.  Lane 0 enters at pos, the others at their own first bit; then a lane whose left
    // neighbour's exit differs from its entry walks again from there.  Lane i is exact after pass i: 257 passes at most.
    // A lane behind an end-of-block or invalid exit gets no new entry: it keeps what it has and is dropped in step 4.
    MMT_INF_LANES(lane) {
      const int e = rel + 8 * lane * S;
      const InfExit x = inf_walk(g.lit, g.dist, g.stage, e, e + 8 * S, avail);
      g.entry[lane] = e;
      g.exit[lane] = x.exit; g.kind[lane] = x.kind; g.err[lane] = x.err; g.ntok[lane] = x.ntok; g.nout[lane] = x.nout;
    }
    for (int pass = 0; pass <= kInfLanes; ++pass) {
      MMT_INF_LANES(lane) {
        int changed = 0;
        if (lane > 0 && g.kind[lane - 1] == kExitCont) {
          g.want_entry[lane] = g.exit[lane - 1];
          changed = g.want_entry[lane] != g.entry[lane];
        }
        g.flag[lane] = changed;
      }
      if (!inf_any(g)) break;
      MMT_INF_LANES(lane) {
        if (g.flag[lane]) {
          const int e = g.want_entry[lane];
          const InfExit x = inf_walk(g.lit, g.dist, g.stage, e, rel + 8 * (lane + 1) * S, avail);
          g.entry[lane] = e;
          g.exit[lane] = x.exit; g.kind[lane] = x.kind; g.err[lane] = x.err; g.ntok[lane] = x.ntok; g.nout[lane] = x.nout;
        }
      }
    }

    // step 4: offsets.  The chain from lane 0 is exact; its first end-of-block or invalid exit ends the round's tokens.
    MMT_INF_LANES(lane) { g.cur_dst[lane] = g.kind[lane] != kExitCont ? lane : kInfLanes - 1; }
    const int stop = inf_min_dst(g);
    MMT_INF_LANES(lane) {
      const int live = lane <= stop;
      g.has[lane] = live;
      g.scan[0][lane] = live ? g.nout[lane] : 0;
      g.flag[lane] = 0;
      if (lane == stop) { g.end_exit = g.exit[lane]; g.end_kind = g.kind[lane]; g.end_err = g.err[lane]; }
    }
    inf_scan(g);
    const int total = g.scan[0][kInfLanes - 1];                 // <= 256 * 1024 * 258
    if (total > lim - out_at) { status = MMT_PNG_ST_TOO_LONG; break; }
    uint8_t* o = out + out_at;                                  // [o, o + total) lies inside out

    // step 5: literals, then the matches in rounds
    MMT_INF_LANES(lane) {
      if (g.has[lane]) {
        const int off = g.scan[0][lane] - g.nout[lane];
        int p = g.entry[lane], dst = off;
        for (int k = 0; k < g.ntok[lane]; ++k) {
          const InfTok t = inf_token(g.lit, g.dist, inf_window(g.stage, p));
          if (t.kind == kTokLiteral) { if (dst < total) o[dst] = (uint8_t)t.value; ++dst; }
          else dst += t.value;
          p += t.bits;
        }
        g.own[lane] = off; g.cur_p[lane] = g.entry[lane]; g.cur_left[lane] = g.ntok[lane]; g.cur_dst[lane] = off;
      } else {
        g.own[lane] = total; g.cur_p[lane] = 0; g.cur_left[lane] = 0; g.cur_dst[lane] = total;
      }
    }
    // the lane that holds the smallest mark finishes all its matches in a round: 256 rounds at most, and one to see the end
    for (int it = 0; it <= kInfLanes; ++it) {
      MMT_INF_LANES(lane) { inf_seek(g, lane, total); g.fin[lane] = g.cur_dst[lane]; }
      const int mark = inf_min_dst(g);
      if (mark >= total) break;
      MMT_INF_LANES(lane) {
        while (g.cur_left[lane] > 0) {
          const InfTok t = inf_token(g.lit, g.dist, inf_window(g.stage, g.cur_p[lane]));      // a match: inf_seek stopped here
          const int dst = g.cur_dst[lane], n = t.value, d = t.dist;
          if ((long)d > out_at + dst) {
            g.flag[lane] = 1;                                   // a distance before the start: nothing is copied
          } else {
            if (!inf_ready(g.own, g.fin, lane, dst, n, d)) break;
            // d < n overlaps itself: the d bytes in front, repeated.  They are final, so no load waits for a store of
            // this copy; 16 bytes are loaded before they are stored, which keeps the loads in flight together.
            const uint8_t* src = o + dst - d;
            for (int k = 0, j = 0; k < n; k += 16) {
              uint8_t t[16];
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                if (k + i < n) { t[i] = src[j]; if (++j == d) j = 0; }
              }
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                if (k + i < n && dst + k + i < total) o[dst + k + i] = t[i];
              }
            }
          }
          g.cur_p[lane] += t.bits; g.cur_left[lane] -= 1; g.cur_dst[lane] = dst + n;
          inf_seek(g, lane, total);
        }
      }
    }
    if (inf_any(g)) { status = MMT_PNG_ST_DISTANCE; break; }

    // step 6: advance
    out_at += total;
    const long npos = base * 8 + g.end_exit;
    if (g.end_kind == kExitBad) { status = g.end_err; break; }
    if (g.end_kind == kExitEnd) { in_block = 0; done = last; }
    if (npos <= pos) { status = MMT_PNG_ST_NO_PROGRESS; break; }
    pos = npos;
  }
  if (status) return status;

  // the end of the stream: the check value behind the byte boundary, the exact length, the Adler-32 of the output
  const long at = (pos + 7) >> 3;
  if (at + 4 > comp_n) return MMT_PNG_ST_TRUNCATED;
  if (out_at != want) return MMT_PNG_ST_TOO_SHORT;
  const uint32_t stored = (uint32_t)comp[at] << 24 | (uint32_t)comp[at + 1] << 16 | (uint32_t)comp[at + 2] << 8 | (uint32_t)comp[at + 3];
  const long chunk = (want + kInfLanes - 1) / kInfLanes;
  uint32_t* pa = (uint32_t*)g.entry;
  uint32_t* pb = (uint32_t*)g.exit;
  MMT_INF_LANES(lane) {
    long s = lane * chunk, e = s + chunk;
    if (e > want) e = want;
    uint32_t a = 1, b = 0;
    while (s < e) {                                             // pieces of a lane's slice, combined as they come
      const int m = e - s < 5552 ? (int)(e - s) : 5552;
      uint32_t a2 = 1, b2 = 0;
      inf_adler_piece(out + s, m, a2, b2);
      inf_adler_combine(a, b, a2, b2, m);
      s += m;
    }
    pa[lane] = a; pb[lane] = b;
  }
  MMT_INF_LANES(lane) {
    if (lane == 0) {
      uint32_t a = 1, b = 0;
      for (int i = 0; i < kInfLanes; ++i) {
        long n = want - i * chunk;
        n = n < 0 ? 0 : (n > chunk ? chunk : n);
        inf_adler_combine(a, b, pa[i], pb[i], n);
      }
      g.adler = (b << 16) | a;
    }
  }
  return g.adler == stored ? 0 : MMT_PNG_ST_ADLER;
}

// The filter-type byte of every scanline, by the pass geometry of png_decode.h (clamped into [g.raw, g.raw_end) of raw).
__host__ __device__ inline int inf_filter_bytes(InfGroup& g, const uint8_t* raw, const PngGeom& geom) {
  MMT_INF_LANES(lane) {
    int bad = 0;
    for (int p = 0; p < geom.passes; ++p) {
      const PngPass s = png_pass(geom, p);
      for (long r = lane; r < s.rows; r += kInfLanes) bad |= raw[s.off + r * (1 + s.rowbytes)] > 4;
    }
    g.flag[lane] = bad;
  }
  return inf_any(g) ? MMT_PNG_ST_FILTER : 0;
}

}  // namespace mmt
