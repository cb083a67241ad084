// Entropy decode of a JPEG scan by subsequences (jpeg_entropy.hip; DESIGN.md section 4, "JPEG entropy decode on the
// device"): the plan of one image with every offset and count clamped into the caller's buffers, the bit reader on
// the raw (byte-stuffed) bytes, and the decode of one subsequence, shared by the kernels and the host loops through
// __host__ __device__ functions.  Nothing here indexes a local array with a runtime value, so the state of a lane stays
// in registers.
#pragma once
#include "jpeg_decode.h"

namespace mmt {

constexpr int kEntThreads = 256;        // threads of every entropy workgroup
constexpr int kEntWindow = 32768;       // raw bytes the subsequences of one workgroup cover at the most
constexpr int kEntSlack = 32;           // bytes staged behind the last subsequence: the reader holds at most 4 data bytes (8
                                        // raw ones) and a symbol takes at most 4 more (8 raw), so 16 beyond the end at the most
constexpr int kHuffWords = MMT_JPEG_HUFF_WORDS;

// Subsequences one workgroup owns: 256 up to subseq_bytes = 128, then what fits the window.
__host__ __device__ inline int jpeg_entropy_group(int subseq_bytes) {
  const int k = kEntWindow / subseq_bytes;
  return k > kEntThreads ? kEntThreads : k;
}
// Bytes of the staged window: each subsequence may be followed by a 2-byte restart marker; 16 in front for alignment.
__host__ __device__ inline int jpeg_entropy_window(int subseq_bytes) {
  return jpeg_entropy_group(subseq_bytes) * (subseq_bytes + 2) + kEntSlack + 32;
}
// The window in LDS is padded by one 4-byte word per 2^pad_shift bytes (a subsequence, at least 64 bytes): lanes that
// walk subsequences of 64 bytes and more would otherwise start a power-of-two number of banks apart and read the same
// bank.  Byte i of the window lives at ent_padded(i, pad_shift); host memory passes 31 (no padding).
__host__ __device__ inline int jpeg_entropy_pad_shift(int subseq_bytes) {
  int lg = 6;
  while ((1 << lg) < subseq_bytes) ++lg;
  return lg;
}
__host__ __device__ inline int ent_padded(int i, int pad_shift) { return i + ((i >> pad_shift) << 2); }
__host__ __device__ inline int jpeg_entropy_lds_bytes(int subseq_bytes) {
  const int w = jpeg_entropy_window(subseq_bytes) & ~15;
  return (ent_padded(w, jpeg_entropy_pad_shift(subseq_bytes)) + 15) & ~15;
}

struct EntState {                       // a decoder between two symbols
  int p;                                // bit position from the scan's first byte, on the raw bytes
  int bz;                               // (block inside the MCU << 8) | zigzag index; z = 0: a DC code comes next.  The block
                                        // stays 0 where all components share their tables: it decides nothing there, and a
                                        // state that carried it could never synchronise (the bits do not tell it)
};
__host__ __device__ inline bool operator!=(const EntState& a, const EntState& b) { return a.p != b.p || a.bz != b.bz; }

struct EntParams {
  int B, groups, K, subseq_bytes, max_subseq, max_rounds, round;
  const unsigned char* bytes;
  long bytes_len;
  const mmt_jpeg_image* images;
  const mmt_jpeg_scan* scans;
  const unsigned* huff;
  const int* segments;
  long n_segments;
  const int* subseqs;
  long n_subseq;
  short* coef;
  long coef_elems;
  int* status;
  // workspace
  int* changed;                         // [max_rounds][B]
  EntState* entry;                      // [n_subseq] the state a subsequence was last decoded from
  EntState* exit_;                      // [n_subseq] and the state it reached
  unsigned* slots;                      // [n_subseq] coefficient slots it advanced
  EntState* edge;                       // [2][B * groups] exit of a group's last subsequence, by round parity
  unsigned* tail;                       // [B * groups] slots from the group's last segment start (or its start) to its end
  int* has_start;                       // [B * groups] the group holds a segment start
  unsigned* carry;                      // [B * groups] slots of the open segment in front of the group
};

// One image's plan, clamped: no field lets an index leave bytes, segments or subseqs.
struct EntImage {
  long base;                            // first byte of the scan in bytes, in [0, bytes_len]
  int count;                            // bytes of the scan, base + count <= bytes_len, < 2^28
  long seg0, sub0;                      // first entries in segments and subseqs
  int nseg, nsub;                       // seg0 + nseg <= n_segments, sub0 + nsub <= n_subseq, nsub <= max_subseq
  int hv, bpm;                          // luma blocks and all blocks of an MCU (1 for a grey image)
  int ri, mcus_x, mcus;                 // restart interval (0: none), MCUs per row and in all
  bool cut;                             // the plan names more subsequences than max_subseq or the table hold
  bool uniform;                         // one table pair for all blocks: the block inside the MCU stays 0 in every state
};

__host__ __device__ inline EntImage ent_image(const mmt_jpeg_scan& sc, const JpegGeom& g, const EntParams& p) {
  EntImage im;
  im.base = jclampl(sc.byte_offset, 0, p.bytes_len);
  const long room = p.bytes_len - im.base;
  im.count = (int)jclampl(sc.byte_count, 0, room < (1L << 28) - 1 ? room : (1L << 28) - 1);
  im.seg0 = jclampl(sc.segment_offset, 0, p.n_segments);
  im.nseg = (int)jclampl(sc.n_segments, 0, jclampl(p.n_segments - im.seg0, 0, 1L << 30));
  im.sub0 = jclampl(sc.subseq_offset, 0, p.n_subseq);
  const long sub_room = jclampl(p.n_subseq - im.sub0, 0, p.max_subseq);
  im.nsub = (int)jclampl(sc.n_subseq, 0, sub_room);
  im.cut = sc.n_subseq > sub_room;
  im.hv = g.nc == 3 ? g.hs * g.vs : 1;
  im.bpm = g.nc == 3 ? im.hv + 2 : 1;
  im.mcus_x = g.bw[0] / (g.nc == 3 ? g.hs : 1);
  if (im.mcus_x < 1) im.mcus_x = 1;
  int mcus_y = g.bh[0] / (g.nc == 3 ? g.vs : 1);
  if (mcus_y < 1) mcus_y = 1;
  im.mcus = im.mcus_x * mcus_y;                                 // <= 2^26
  im.ri = jclampi(sc.restart_interval, 0, 65535);
  im.uniform = sc.uniform_tables != 0 || im.bpm == 1;
  return im;
}

// One subsequence of an image (i < nsub), clamped: 0 <= seg_begin <= begin <= end <= seg_end <= count.
struct EntSub {
  int seg_begin, seg_end;               // its restart segment, in bytes from the scan's first byte
  int begin, end;                       // its own bytes
  int first_mcu, n_mcu;                 // the segment's MCUs
  bool first, last;                     // of its segment
  bool live;                            // false: the plan gives it no bytes
};

__host__ __device__ inline EntSub ent_sub(const EntImage& im, const EntParams& p, int i) {
  EntSub s;
  s.live = im.nseg > 0;
  const int k = s.live ? jclampi(p.subseqs[im.sub0 + i], 0, im.nseg - 1) : 0;
  const int* g = p.segments + (s.live ? (im.seg0 + k) * 4 : 0);
  const int g0 = s.live ? g[0] : 0, g1 = s.live ? g[1] : 0, g2 = s.live ? g[2] : 0, g3 = s.live ? g[3] : 0;
  s.seg_begin = jclampi(g0, 0, im.count);
  s.seg_end = jclampi(g1, s.seg_begin, im.count);
  s.first_mcu = jclampi(g2, 0, im.mcus);
  s.n_mcu = im.mcus - s.first_mcu;
  if (im.ri > 0 && s.n_mcu > im.ri) s.n_mcu = im.ri;
  const int j = i - jclampi(g3, 0, im.nsub);                    // position inside the segment
  const long at = (long)s.seg_begin + (long)(j < 0 ? 0 : j) * p.subseq_bytes;
  s.first = j == 0;
  if (j < 0 || (at >= s.seg_end && j > 0)) s.live = false;
  s.begin = (int)(at < s.seg_end ? at : s.seg_end);
  s.end = s.seg_end - s.begin > p.subseq_bytes ? s.begin + p.subseq_bytes : s.seg_end;
  s.last = s.end == s.seg_end;
  return s;
}

template <class T>
__host__ __device__ inline T ent_pick3(const T (&a)[3], int c) { return c == 0 ? a[0] : (c == 1 ? a[1] : a[2]); }

// Bits of one restart segment.  at(i) is byte i of the scan (d holds them from byte org on, padded as ent_padded says); bytes at and beyond lim read as zero bits, which are
// counted.  0xff 0x00 is one 0xff byte.  The raw position of the next unread bit follows from the position behind the
// last byte taken, the unread bits and the stuffed zeros among the unread bytes (one flag per byte taken, the newest
// lowest).
struct EntBits {
  const unsigned char* d;
  int org, pos, lim, pad;
  unsigned acc, stuffed;
  int n, fake;                          // unread bits (the lowest n of acc); how many zero bits were made up

  __host__ __device__ unsigned at(int i) const { return d[ent_padded(i - org, pad)]; }
  __host__ __device__ void open(const unsigned char* data, int origin, int pad_shift, int seg_begin, int limit, int p) {
    d = data; org = origin; pad = pad_shift; lim = limit; acc = 0; stuffed = 0; n = 0; fake = 0;
    pos = p >> 3;
    if (pos < seg_begin) pos = seg_begin;                       // a state from garbage stays inside the staged bytes
    if (pos > lim) pos = lim;
    const int bit = p & 7;
    // a subsequence that begins on the 0x00 of a stuffed pair skips it
    if (bit == 0 && pos > seg_begin && pos < lim && at(pos - 1) == 0xff && at(pos) == 0x00) ++pos;
    fill();
    n -= bit;
  }
  __host__ __device__ void fill() {
    while (n <= 24) {
      unsigned b = 0, st = 0;
      if (pos < lim) {
        b = at(pos);
        ++pos;
        if (b == 0xff && pos < lim && at(pos) == 0x00) { ++pos; st = 1; }
      } else {
        fake += 8;
      }
      acc = (acc << 8) | b;
      stuffed = (stuffed << 1) | st;
      n += 8;
    }
  }
  __host__ __device__ unsigned peek(int k) const { return (acc >> (n - k)) & ((1u << k) - 1u); }   // 1 <= k <= 16 <= n
  __host__ __device__ void skip(int k) { n -= k; }
  __host__ __device__ int real() const { return n - fake; }
  __host__ __device__ int tell() const {
    if (n <= 0) return pos * 8 - n + fake;
    const unsigned among = stuffed & ((2u << ((n - 1) >> 3)) - 1u);       // the bytes from the one that holds the next bit on
    return pos * 8 - n + fake - 8 * __builtin_popcount(among);
  }
};

__host__ __device__ inline unsigned huff_look(const unsigned* t, unsigned i) { return (t[i >> 1] >> ((i & 1) * 16)) & 0xffffu; }
__host__ __device__ inline int huff_maxcode(const unsigned* t, int len) { return (int)t[256 + len - 10]; }
__host__ __device__ inline int huff_valoff(const unsigned* t, int len) { return (int)t[264 + len - 10]; }
__host__ __device__ inline int huff_val(const unsigned* t, unsigned i) { return (int)((t[272 + (i >> 2)] >> ((i & 3) * 8)) & 0xffu); }

// Where the write pass puts the coefficients of one subsequence.
struct EntSink {
  short* coef;
  long coef_elems;
  unsigned slot0;                       // the subsequence's first slot in its segment: 64 * block + zigzag index
  unsigned slots_max;                   // slots of the segment: what lies beyond is not written
  int first_mcu;
};

// Decodes the symbols that begin inside [in.p, 8 * sub.end) from state `in`; returns the slots advanced (a DC code 1, an
// AC code its run + 1, ZRL 16, EOB up to 64, all capped at the block's end) and the state behind the last symbol.
// Speculation meets garbage: a code that is not in the table counts as one bit and the symbol 0, a run past 63 ends
// the block.  With WRITE the same walk stores every non-zero coefficient, de-zigzagged, the DC as its difference, and
// reports these two cases in err.  A symbol that needs bits beyond the segment ends the walk and is not counted.
template <bool WRITE>
__host__ __device__ __forceinline__ unsigned ent_decode(const unsigned char* d, int org, int pad_shift, int lim, const EntSub& sub, EntState in,
                                               const unsigned* tables, const unsigned char* zigzag, const EntImage& im,
                                               const JpegGeom& g, const EntSink& sink, EntState& out, int& err) {
  EntBits r;
  r.open(d, org, pad_shift, sub.seg_begin > org ? sub.seg_begin : org, lim < sub.seg_end ? lim : sub.seg_end, in.p);
  int bim = im.uniform ? 0 : jclampi(in.bz >> 8, 0, im.bpm - 1), z = jclampi(in.bz & 255, 0, 63);
  unsigned L = 0;
  const int bound = sub.end * 8;
  long base = 0;                                                // of the block being written
  unsigned cur = ~0u;
  bool writable = false;
  for (int it = 0; it < (sub.end - sub.begin) * 8 + 8; ++it) {
    if (r.tell() >= bound) break;
    const int c = bim < im.hv ? 0 : (bim - im.hv + 1 > 2 ? 2 : bim - im.hv + 1);
    const unsigned* t = tables + (2 * c + (z ? 1 : 0)) * kHuffWords;
    if (r.n < 16) r.fill();
    const unsigned e = huff_look(t, r.peek(9));
    int len, sym;
    bool bad = false;
    if (e) {
      len = (int)(e >> 8); sym = (int)(e & 255u);
    } else {
      const int bits16 = (int)r.peek(16);
      len = 10;
      while (len <= 16 && (bits16 >> (16 - len)) > huff_maxcode(t, len)) ++len;
      if (len > 16) { bad = true; len = 1; sym = 0; }
      else sym = huff_val(t, (unsigned)((bits16 >> (16 - len)) + huff_valoff(t, len)) & 255u);
    }
    if (bad && r.real() < 16) break;                            // the padding at the end of the segment
    r.skip(len);
    if (z == 0 && sym > 15) { bad = true; sym &= 15; }          // a DC symbol is a size
    const int s = sym & 15, run = sym >> 4;
    int v = 0;
    if (s) {
      if (r.n < 16) r.fill();
      v = (int)r.peek(s);
      r.skip(s);
      if (v < (1 << (s - 1))) v = v - (1 << s) + 1;
    }
    if (r.n < r.fake) break;                                    // made-up bits were consumed: the symbol is not whole
    int adv, at = -1;                                           // at: zigzag offset of the coefficient from z, -1: none
    if (z == 0) { adv = 1; at = 0; }
    else if (s) {
      if (z + run > 63) { adv = 64 - z; if (WRITE && err < MMT_JPEG_ST_RUN) err = MMT_JPEG_ST_RUN; }
      else { adv = run + 1; at = run; }
    }
    else if (run == 15) adv = 64 - z < 16 ? 64 - z : 16;
    else adv = 64 - z;
    if (WRITE) {
      if (bad && err < MMT_JPEG_ST_BAD_CODE) err = MMT_JPEG_ST_BAD_CODE;
      if (at >= 0 && v != 0) {
        const unsigned slot = sink.slot0 + L + (unsigned)at;
        const unsigned blk = slot >> 6;
        if (blk != cur) {                                       // the block's first coefficient, from its place in the segment
          cur = blk;
          writable = slot < sink.slots_max;
          const unsigned m = (unsigned)sink.first_mcu + blk / (unsigned)im.bpm, j = blk % (unsigned)im.bpm;
          const int my = (int)(m / (unsigned)im.mcus_x), mx = (int)(m % (unsigned)im.mcus_x);
          const int cc = (int)j < im.hv ? 0 : ((int)j - im.hv + 1 > 2 ? 2 : (int)j - im.hv + 1);
          const int bx = cc == 0 && g.nc == 3 ? mx * g.hs + (int)j % g.hs : mx;
          const int by = cc == 0 && g.nc == 3 ? my * g.vs + (int)j / g.hs : my;
          const int bw = ent_pick3(g.bw, cc), bh = ent_pick3(g.bh, cc);
          writable = writable && bx < bw && by < bh;
          base = ent_pick3(g.off, cc) + ((long)by * bw + bx) * 64;
        }
        const long a = base + zigzag[slot & 63u];
        if (writable && a < sink.coef_elems) sink.coef[a] = (short)v;
      }
    }
    L += (unsigned)adv;
    z += adv;
    if (z >= 64) { z = 0; bim = im.uniform || bim + 1 == im.bpm ? 0 : bim + 1; }
  }
  out.p = r.tell();
  out.bz = (bim << 8) | z;
  return L;
}

// The state a subsequence is decoded from when its left neighbour has none to give: the known state at the start of a
// segment, the assumed one (a block of the MCU's first component begins) elsewhere.
__host__ __device__ inline EntState ent_start(const EntSub& s) {
  EntState e;
  e.p = s.begin * 8; e.bz = 0;
  return e;
}

hipError_t launch_jpeg_entropy(EntParams p, hipStream_t st);

}  // namespace mmt
