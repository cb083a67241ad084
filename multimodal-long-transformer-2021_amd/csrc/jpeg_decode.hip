// JPEG decode in front of the image front end (C ABI: include/mmt_layer.h, mmt_jpeg_*): `tf.io.decode_image` of
// `decode_fn` (src/data/data_utils.py:195) for JPEG bytes, as libjpeg decodes by default (JDCT_ISLOW, fancy
// upsampling).  DESIGN.md section 4 "JPEG decode" states the rules and the accepted files.
//
//   host    mmt_jpeg_info, mmt_jpeg_coefficients: markers and Huffman decoding -- serial by nature, plain C++ that a
//           sanitizer checks; a corrupt file can do no harm there.  Output: quantised coefficients in natural order,
//           [component][block_y][block_x][64], and one quantisation table per component.
//           mmt_jpeg_scan_plan: the same header parser in front of the device entropy decode (jpeg_entropy.hip), which
//           writes those coefficients from the uploaded bytes: tables in the kernels' form, restart segments,
//           subsequences.
//   device  two kernels, grid (images, parts), whatever B is:
//           1. dequantise + 8x8 inverse DCT into uint8 component planes in the workspace.  8 threads per block, 32
//              blocks per workgroup step: thread t loads row t (one 16-byte load), dequantises into LDS, runs column t,
//              then row t, and stores its 8 samples with one 8-byte store.  The transposition between the passes goes
//              through LDS, 72 ints per block so that the column reads of a 32-lane group cover the 32 banks.
//           2. chroma upsampling + YCbCr -> RGB + range limit: one thread per 4 output pixels of a row, three 4-byte
//              stores where the address allows, bytes otherwise.
//           The planes are written by one launch and read by the next (a chroma tap needs samples of neighbouring
//           blocks, so fusing would recompute or synchronise across workgroups; DESIGN.md has the reasoning).
//   mmt_jpeg_pixels_host is the same two steps as loops over host memory, through the functions of jpeg_decode.h.
//
// Bounds (the front end's rule): jpeg_geom() clamps sizes, grids and offsets into the buffers; on top of it every
// coefficient, plane and pixel address is capped and no byte is written at or beyond the end of a buffer.
#include "../../include/mmt_attn.h"
#include "../../include/mmt_layer.h"

#include <cstdint>
#include <cstring>

#include "jpeg_decode.h"
#include "mmt_err.h"

namespace mmt {
namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Host stage: markers and Huffman decoding.
// ---------------------------------------------------------------------------------------------------------------------
const unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kLook = 9;                // bits of the one-step Huffman lookup

struct Huff {
  bool defined;
  unsigned char vals[256];
  unsigned short look[1 << kLook];      // (length << 8) | symbol for codes of at most kLook bits, 0 otherwise
  int maxcode[17];                      // largest code of each length, -1 where there is none
  int valoff[17];                       // index into vals of the first code of each length, minus that code
};

struct Frame {
  int width, height, nc;
  int id[3], h[3], v[3], tq[3];
  int hmax, vmax, mcus_x, mcus_y;
};

struct Stream {
  const unsigned char* p;
  const unsigned char* end;
  Frame f;
  bool have_frame, jfif, adobe;
  int adobe_transform;
  int restart;                          // MCUs per restart interval, 0: none
  bool qdef[4];
  unsigned short q[4][64];              // natural order
  Huff dc[4], ac[4];
};

// Markers that fill no segment.
bool bare_marker(int m) { return m == 0x01 || (m >= 0xd0 && m <= 0xd9); }

// Moves to the next marker and returns it, -1 at the end of the data.
int next_marker(Stream& s) {
  while (s.p < s.end) {
    if (*s.p++ != 0xff) continue;
    while (s.p < s.end && *s.p == 0xff) ++s.p;
    if (s.p >= s.end) return -1;
    const int m = *s.p++;
    if (m != 0) return m;
  }
  return -1;
}

int build_huff(Huff& h, const unsigned char* bits /* [16] */, const unsigned char* vals, int n) {
  std::memset(h.look, 0, sizeof(h.look));
  std::memcpy(h.vals, vals, (size_t)n);
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    const int cnt = bits[len - 1];
    h.valoff[len] = k - code;
    if (cnt) {
      if (code + cnt > (1 << len)) return fail(MMT_E_INVALID, "jpeg: a DHT segment defines more codes of %d bits than there are", len);
      if (len <= kLook)
        for (int i = 0; i < cnt; ++i)
          for (int pad = 0; pad < (1 << (kLook - len)); ++pad)
            h.look[((code + i) << (kLook - len)) | pad] = (unsigned short)((len << 8) | vals[k + i]);
      code += cnt; k += cnt;
      h.maxcode[len] = code - 1;
    } else {
      h.maxcode[len] = -1;
    }
    code <<= 1;
  }
  h.defined = true;
  return MMT_OK;
}

// One marker segment in front of the scans (the length is checked here).  Returns MMT_OK or a refusal.
int read_segment(Stream& s, int m) {
  if (s.end - s.p < 2) return fail(MMT_E_INVALID, "jpeg: truncated in the header of segment 0x%02x", m);
  const int len = (s.p[0] << 8) | s.p[1];
  if (len < 2 || len > s.end - s.p) return fail(MMT_E_INVALID, "jpeg: segment 0x%02x of %d bytes leaves the data", m, len);
  const unsigned char* d = s.p + 2;
  const unsigned char* e = s.p + len;
  s.p = e;
  if (m == 0xdb) {                                              // DQT
    while (d < e) {
      const int pq = d[0] >> 4, tq = d[0] & 15;
      if (pq == 1) return fail(MMT_E_UNSUPPORTED, "jpeg: 16-bit quantisation tables are not supported");
      if (pq != 0 || tq > 3 || e - d < 65) return fail(MMT_E_INVALID, "jpeg: malformed DQT segment");
      for (int i = 0; i < 64; ++i) s.q[tq][kZigzag[i]] = d[1 + i];
      s.qdef[tq] = true;
      d += 65;
    }
  } else if (m == 0xc4) {                                       // DHT
    while (d < e) {
      if (e - d < 17) return fail(MMT_E_INVALID, "jpeg: malformed DHT segment");
      const int tc = d[0] >> 4, th = d[0] & 15;
      int n = 0;
      for (int i = 0; i < 16; ++i) n += d[1 + i];
      if (tc > 1 || th > 3 || n > 256 || e - d < 17 + n) return fail(MMT_E_INVALID, "jpeg: malformed DHT segment");
      const int rc = build_huff(tc ? s.ac[th] : s.dc[th], d + 1, d + 17, n);
      if (rc) return rc;
      d += 17 + n;
    }
  } else if (m == 0xdd) {                                       // DRI
    if (e - d != 2) return fail(MMT_E_INVALID, "jpeg: malformed DRI segment");
    s.restart = (d[0] << 8) | d[1];
  } else if (m == 0xe0) {
    if (e - d >= 5 && std::memcmp(d, "JFIF", 5) == 0) s.jfif = true;
  } else if (m == 0xee) {
    if (e - d >= 12 && std::memcmp(d, "Adobe", 5) == 0) { s.adobe = true; s.adobe_transform = d[11]; }
  }
  return MMT_OK;                                                // APPn, COM and everything else: skipped
}

int read_frame(Stream& s, int m) {
  if (m == 0xc2) return fail(MMT_E_UNSUPPORTED, "jpeg: progressive files (SOF2) are not supported; decode it on the host");
  if (m == 0xc3 || m == 0xcb) return fail(MMT_E_UNSUPPORTED, "jpeg: lossless files (SOF%d) are not supported", m - 0xc0);
  if (m == 0xc9 || m == 0xca) return fail(MMT_E_UNSUPPORTED, "jpeg: arithmetic coding (SOF%d) is not supported", m - 0xc0);
  if (m != 0xc0 && m != 0xc1) return fail(MMT_E_UNSUPPORTED, "jpeg: hierarchical files (SOF%d) are not supported", m - 0xc0);
  if (s.have_frame) return fail(MMT_E_INVALID, "jpeg: a second frame header");
  if (s.end - s.p < 2) return fail(MMT_E_INVALID, "jpeg: truncated in the frame header");
  const int len = (s.p[0] << 8) | s.p[1];
  if (len < 8 || len > s.end - s.p) return fail(MMT_E_INVALID, "jpeg: frame header of %d bytes leaves the data", len);
  const unsigned char* d = s.p + 2;
  s.p += len;
  Frame& f = s.f;
  const int precision = d[0];
  f.height = (d[1] << 8) | d[2];
  f.width = (d[3] << 8) | d[4];
  f.nc = d[5];
  if (precision != 8) return fail(MMT_E_UNSUPPORTED, "jpeg: %d-bit samples are not supported (8 only)", precision);
  if (f.nc == 4) return fail(MMT_E_UNSUPPORTED, "jpeg: 4 components (CMYK, YCCK) are not supported");
  if (f.nc != 1 && f.nc != 3) return fail(MMT_E_UNSUPPORTED, "jpeg: %d components are not supported (1 or 3)", f.nc);
  if (len != 8 + 3 * f.nc) return fail(MMT_E_INVALID, "jpeg: malformed frame header");
  if (f.width < 1 || f.height < 1) return fail(MMT_E_INVALID, "jpeg: dimensions of zero (%d x %d)", f.width, f.height);
  for (int c = 0; c < f.nc; ++c) {
    f.id[c] = d[6 + 3 * c];
    f.h[c] = d[7 + 3 * c] >> 4;
    f.v[c] = d[7 + 3 * c] & 15;
    f.tq[c] = d[8 + 3 * c];
    if (f.h[c] < 1 || f.h[c] > 4 || f.v[c] < 1 || f.v[c] > 4 || f.tq[c] > 3) return fail(MMT_E_INVALID, "jpeg: malformed frame header");
    for (int o = 0; o < c; ++o)
      if (f.id[o] == f.id[c]) return fail(MMT_E_INVALID, "jpeg: two components share id %d", f.id[c]);
  }
  if (f.nc == 1) {
    f.h[0] = f.v[0] = 1;                                        // a lone component is never interleaved: its factors mean nothing
  } else {
    const bool luma_ok = (f.h[0] == 1 && f.v[0] == 1) || (f.h[0] == 2 && f.v[0] == 1) || (f.h[0] == 2 && f.v[0] == 2);
    if (!luma_ok || f.h[1] != 1 || f.v[1] != 1 || f.h[2] != 1 || f.v[2] != 1)
      return fail(MMT_E_UNSUPPORTED, "jpeg: sampling %dx%d,%dx%d,%dx%d is not supported (4:4:4, 4:2:2 and 4:2:0 only)", f.h[0], f.v[0],
                  f.h[1], f.v[1], f.h[2], f.v[2]);
  }
  f.hmax = f.h[0]; f.vmax = f.v[0];
  f.mcus_x = (f.width + 8 * f.hmax - 1) / (8 * f.hmax);
  f.mcus_y = (f.height + 8 * f.vmax - 1) / (8 * f.vmax);
  s.have_frame = true;
  return MMT_OK;
}

// From the start of the data to just behind the first SOS marker (its segment unread).  Tables met on the way are kept.
int read_headers(Stream& s) {
  if (s.end - s.p < 2 || s.p[0] != 0xff || s.p[1] != 0xd8)
    return fail(MMT_E_UNSUPPORTED, "jpeg: the data does not start with a JPEG SOI marker (PNG, GIF, BMP, ...?): decode it on the host");
  s.p += 2;
  for (;;) {
    const int m = next_marker(s);
    if (m < 0) return fail(MMT_E_INVALID, "jpeg: truncated before the first scan");
    if (m == 0xda) break;
    if (m == 0xd9) return fail(MMT_E_INVALID, "jpeg: no scan before the end of the image");
    if (m == 0xcc) return fail(MMT_E_UNSUPPORTED, "jpeg: arithmetic coding (DAC) is not supported");
    if (m == 0xde) return fail(MMT_E_UNSUPPORTED, "jpeg: hierarchical files (DHP) are not supported");
    if (bare_marker(m)) continue;
    const int rc = m >= 0xc0 && m <= 0xcf && m != 0xc4 && m != 0xc8 ? read_frame(s, m) : read_segment(s, m);
    if (rc) return rc;
  }
  if (!s.have_frame) return fail(MMT_E_INVALID, "jpeg: a scan without a frame header");
  if (s.f.nc == 3) {                                            // libjpeg's rule for the colour space of 3 components
    const bool rgb_ids = s.f.id[0] == 'R' && s.f.id[1] == 'G' && s.f.id[2] == 'B';
    if (!s.jfif && ((s.adobe && s.adobe_transform == 0) || (!s.adobe && rgb_ids)))
      return fail(MMT_E_UNSUPPORTED, "jpeg: RGB stored directly (Adobe transform 0) is not supported");
  }
  return MMT_OK;
}

void fill_image(const Frame& f, mmt_jpeg_image* out) {
  std::memset(out, 0, sizeof(*out));
  out->width = f.width; out->height = f.height; out->components = f.nc;
  int64_t at = 0;
  for (int c = 0; c < f.nc; ++c) {
    out->h_samp[c] = f.h[c]; out->v_samp[c] = f.v[c];
    out->blocks_w[c] = f.mcus_x * f.h[c]; out->blocks_h[c] = f.mcus_y * f.v[c];
    out->coef_offset[c] = at;
    at += (int64_t)out->blocks_w[c] * out->blocks_h[c] * 64;
  }
  out->coef_elems = at;
}

// Entropy-coded bits.  A stuffed 0xff00 is one 0xff byte; at a marker or at the end of the data zero bits are supplied
// and counted, and whoever consumed one of them has read past the scan (checked per MCU).
struct Bits {
  const unsigned char* p;
  const unsigned char* end;
  uint64_t acc;
  int n, fake;                          // bits in acc (the newest lowest); how many of them, at the bottom, are made up
  void fill() {
    while (n <= 56) {
      unsigned b = 0;
      if (p < end && *p != 0xff) {
        b = *p++;
      } else if (p + 1 < end && p[1] == 0x00) {
        b = 0xff; p += 2;
      } else {
        fake += 8;
      }
      acc = (acc << 8) | b;
      n += 8;
    }
  }
  unsigned peek(int k) const { return (unsigned)(acc >> (n - k)) & ((1u << k) - 1u); }       // 1 <= k <= 16 <= n
  void skip(int k) { n -= k; }
  bool overrun() const { return n < fake; }
  void reset() { acc = 0; n = 0; fake = 0; }
};

// The next symbol, -1 when the bits are no code of the table.
inline int decode_symbol(Bits& b, const Huff& h) {
  if (b.n < 16) b.fill();
  const unsigned e = h.look[b.peek(kLook)];
  if (e) { b.skip(e >> 8); return e & 255; }
  int len = kLook + 1;
  const int bits16 = (int)b.peek(16);
  while (len <= 16 && (bits16 >> (16 - len)) > h.maxcode[len]) ++len;
  if (len > 16) return -1;
  b.skip(len);
  return h.vals[((bits16 >> (16 - len)) + h.valoff[len]) & 255];
}

inline int receive_extend(Bits& b, int nbits) {                 // 1 <= nbits <= 15
  if (b.n < 16) b.fill();
  const int v = (int)b.peek(nbits);
  b.skip(nbits);
  return v < (1 << (nbits - 1)) ? v - (1 << nbits) + 1 : v;
}

int decode_block(Bits& b, const Huff& dc, const Huff& ac, int& pred, short* out /* 64, zeroed */) {
  int s = decode_symbol(b, dc);
  if (s < 0 || s > 15) return fail(MMT_E_INVALID, "jpeg: corrupt scan: a Huffman code that is not in the DC table");
  if (s) pred = (int)((unsigned)pred + (unsigned)receive_extend(b, s));
  out[0] = (short)pred;
  for (int k = 1; k < 64;) {
    const int rs = decode_symbol(b, ac);
    if (rs < 0) return fail(MMT_E_INVALID, "jpeg: corrupt scan: a Huffman code that is not in the AC table");
    const int r = rs >> 4;
    s = rs & 15;
    if (s) {
      k += r;
      if (k > 63) return fail(MMT_E_INVALID, "jpeg: corrupt scan: a zero run past coefficient 63");
      out[kZigzag[k++]] = (short)receive_extend(b, s);
    } else if (r == 15) {
      k += 16;
    } else {
      break;
    }
  }
  return MMT_OK;
}

struct ScanComp { int c, td, ta; };

// The header of a scan: p stands behind the SOS marker and moves to the first entropy-coded byte.  Fills the scan's
// components and, per component met for the first time, its quantisation table.
int read_scan_header(Stream& s, ScanComp* sc, int& ns, unsigned short* qout, bool* seen) {
  const Frame& f = s.f;
  if (s.end - s.p < 2) return fail(MMT_E_INVALID, "jpeg: truncated in the scan header");
  const int len = (s.p[0] << 8) | s.p[1];
  if (len < 6 || len > s.end - s.p) return fail(MMT_E_INVALID, "jpeg: scan header of %d bytes leaves the data", len);
  const unsigned char* d = s.p + 2;
  s.p += len;
  ns = d[0];
  if (ns < 1 || ns > f.nc || len != 6 + 2 * ns) return fail(MMT_E_INVALID, "jpeg: malformed scan header");
  for (int i = 0; i < ns; ++i) {
    int c = 0;
    while (c < f.nc && f.id[c] != d[1 + 2 * i]) ++c;
    if (c == f.nc) return fail(MMT_E_INVALID, "jpeg: a scan names component id %d, which the frame does not have", d[1 + 2 * i]);
    for (int o = 0; o < i; ++o)
      if (sc[o].c == c) return fail(MMT_E_INVALID, "jpeg: a scan names component id %d twice", d[1 + 2 * i]);
    sc[i].c = c; sc[i].td = d[2 + 2 * i] >> 4; sc[i].ta = d[2 + 2 * i] & 15;
    if (sc[i].td > 3 || sc[i].ta > 3 || !s.dc[sc[i].td].defined || !s.ac[sc[i].ta].defined)
      return fail(MMT_E_INVALID, "jpeg: a scan uses a Huffman table that was not defined");
    if (!s.qdef[f.tq[c]]) return fail(MMT_E_INVALID, "jpeg: a scan uses a quantisation table that was not defined");
    if (!seen[c]) std::memcpy(qout + c * 64, s.q[f.tq[c]], 64 * sizeof(unsigned short));
    seen[c] = true;
  }
  const unsigned char* t = d + 1 + 2 * ns;
  if (t[0] != 0 || t[1] != 63 || t[2] != 0) return fail(MMT_E_INVALID, "jpeg: spectral selection or successive approximation in a sequential scan");
  return MMT_OK;
}

// One scan: p stands behind the SOS marker.  Planes are given per component (NULL: the caller has refused already).
int read_scan(Stream& s, const mmt_jpeg_image& im, short* coef, unsigned short* qout, bool* seen) {
  const Frame& f = s.f;
  ScanComp sc[3];
  int ns = 0;
  const int hrc = read_scan_header(s, sc, ns, qout, seen);
  if (hrc) return hrc;

  // a scan of one component walks that component's own blocks; an interleaved one walks MCUs of h x v blocks each
  int mx = f.mcus_x, my = f.mcus_y;
  if (ns == 1) {
    const int c = sc[0].c;
    mx = ((f.width * f.h[c] + f.hmax - 1) / f.hmax + 7) / 8;
    my = ((f.height * f.v[c] + f.vmax - 1) / f.vmax + 7) / 8;
  }
  Bits b = {s.p, s.end, 0, 0, 0};
  int pred[3] = {0, 0, 0};
  int left = s.restart, rst = 0;
  for (int y = 0; y < my; ++y) {
    for (int x = 0; x < mx; ++x) {
      if (s.restart && left == 0) {
        b.reset();
        if (b.end - b.p < 2 || b.p[0] != 0xff || b.p[1] != 0xd0 + rst)
          return fail(MMT_E_INVALID, "jpeg: corrupt scan: restart marker %d is missing", rst);
        b.p += 2;
        rst = (rst + 1) & 7;
        left = s.restart;
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int i = 0; i < ns; ++i) {
        const int c = sc[i].c;
        const int nh = ns == 1 ? 1 : f.h[c], nv = ns == 1 ? 1 : f.v[c];
        for (int v = 0; v < nv; ++v)
          for (int h = 0; h < nh; ++h) {
            const int64_t blk = (int64_t)(y * nv + v) * im.blocks_w[c] + (x * nh + h);
            short* out = coef + im.coef_offset[c] + blk * 64;
            std::memset(out, 0, 64 * sizeof(short));
            const int rc = decode_block(b, s.dc[sc[i].td], s.ac[sc[i].ta], pred[i], out);
            if (rc) return rc;
          }
      }
      if (b.overrun()) return fail(MMT_E_INVALID, "jpeg: corrupt or truncated scan: a marker or the end of the data where coded data should be");
      --left;
    }
  }
  s.p = b.p;
  return MMT_OK;
}

// A table in the form the entropy kernels read (include/mmt_layer.h, MMT_JPEG_HUFF_WORDS words).
void device_huff(const Huff& h, uint32_t* w) {
  std::memset(w, 0, MMT_JPEG_HUFF_WORDS * sizeof(uint32_t));
  std::memcpy(w, h.look, sizeof(h.look));
  for (int len = 10; len <= 16; ++len) {
    w[256 + len - 10] = (uint32_t)h.maxcode[len];
    w[264 + len - 10] = (uint32_t)h.valoff[len];
  }
  std::memcpy(w + 272, h.vals, 256);
}

// The entropy-coded bytes from `at` on, cut at RSTn markers: calls seg(begin, end) per restart segment, at most
// `expected` of them, and returns the end of the scan (the first marker that is no expected RSTn, or the end of the
// data).  A 0xff followed by 0x00 is data; any other 0xff ends the segment, as it does for read_scan's bit reader.
template <class F>
const unsigned char* walk_segments(const unsigned char* at, const unsigned char* end, int64_t expected, F seg) {
  const unsigned char* begin = at;
  int64_t k = 0;
  for (;;) {
    const unsigned char* ff = at < end ? (const unsigned char*)std::memchr(at, 0xff, (size_t)(end - at)) : nullptr;
    if (!ff) { seg(begin, end); return end; }
    if (ff + 1 < end && ff[1] == 0x00) { at = ff + 2; continue; }
    const unsigned char* m = ff + 1;                            // the marker's code: read_scan takes no fill bytes either
    seg(begin, ff);
    if (m < end && *m == 0xd0 + (k & 7) && k + 1 < expected) {
      ++k;
      begin = at = m + 1;
      continue;
    }
    return ff;
  }
}

int check_bytes(const char* who, const uint8_t* bytes, int64_t len) {
  if (!bytes) return fail(MMT_E_INVALID, "%s: bytes is NULL", who);
  if (len < 0) return fail(MMT_E_INVALID, "%s: len (%lld) is negative", who, (long long)len);
  return MMT_OK;
}

int check_stage2(const char* who, int32_t B, const mmt_jpeg_image* images, const int16_t* coef, int64_t coef_elems,
                 const uint16_t* qtables, uint8_t* pixels_out, int64_t pixels_bytes, void* workspace, size_t workspace_bytes) {
  if (B < 1) return fail(MMT_E_INVALID, "%s: B (%d) must be positive", who, B);
  if (!images || !coef || !qtables || !pixels_out)
    return fail(MMT_E_INVALID, "%s: NULL argument (images, coef, qtables and pixels_out are required)", who);
  if (coef_elems < 64 || coef_elems >= ((int64_t)1 << 60))
    return fail(MMT_E_INVALID, "%s: coef_elems %lld outside [64, 2^60)", who, (long long)coef_elems);
  if (pixels_bytes < 1 || pixels_bytes >= ((int64_t)1 << 60))
    return fail(MMT_E_INVALID, "%s: pixels_bytes %lld outside [1, 2^60)", who, (long long)pixels_bytes);
  if ((((uintptr_t)coef | (uintptr_t)qtables) & 15) != 0) return fail(MMT_E_INVALID, "%s: coef and qtables must be 16-byte aligned", who);
  const size_t need = mmt_jpeg_workspace_bytes(coef_elems);
  if (!workspace || workspace_bytes < need)
    return fail(MMT_E_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", who, need, workspace ? workspace_bytes : (size_t)0);
  if (((uintptr_t)workspace & 7) != 0) return fail(MMT_E_INVALID, "%s: workspace must be 8-byte aligned", who);
  return MMT_OK;
}

// The component and the block inside it of block j of an image (j < nblk[0] + nblk[1] + nblk[2]).
__host__ __device__ inline int jpeg_component_of(const JpegGeom& g, int& j) {
  if (j < g.nblk[0]) return 0;
  j -= g.nblk[0];
  if (j < g.nblk[1]) return 1;
  j -= g.nblk[1];
  return 2;
}

// a[c] by selection: a register-resident struct stays in registers on the device
template <class T>
__host__ __device__ inline T pick3(const T (&a)[3], int c) { return c == 0 ? a[0] : (c == 1 ? a[1] : a[2]); }

}  // namespace

#ifndef MMT_JPEG_HOST_ONLY
namespace {

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegParams p) {
  const int b = blockIdx.x, tid = threadIdx.x, t = tid & 7, k = tid >> 3;
  const JpegGeom g = jpeg_geom(p.images[b], p.coef_elems, p.pixels_bytes);
  const int total = g.nblk[0] + g.nblk[1] + g.nblk[2];
  const int ngroups = (total + kJpegGroup - 1) / kJpegGroup;
  __shared__ __attribute__((aligned(16))) int ws[kJpegGroup * kJpegLdsStride];
  int* mine = ws + k * kJpegLdsStride;
  for (int grp = blockIdx.y; grp < ngroups; grp += gridDim.y) {
    int j = grp * kJpegGroup + k;
    const bool live = j < total;
    const int c = jpeg_component_of(g, j);
    const long off = pick3(g.off, c);
    const int bw = pick3(g.bw, c);
    if (live) {                                                 // row t of the block, dequantised
      const long at = min(off + (long)j * 64, (p.coef_elems - 64) & ~7L) + t * 8;          // a multiple of 8
      const uint4 cv = *reinterpret_cast<const uint4*>(p.coef + at);
      const uint4 qv = *reinterpret_cast<const uint4*>(p.qtables + ((size_t)b * 3 + c) * 64 + t * 8);
      const unsigned cw4[4] = {cv.x, cv.y, cv.z, cv.w}, qw4[4] = {qv.x, qv.y, qv.z, qv.w};
      int v[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[2 * i] = (int)(short)(cw4[i] & 0xffffu) * (int)(qw4[i] & 0xffffu);
        v[2 * i + 1] = (int)(short)(cw4[i] >> 16) * (int)(qw4[i] >> 16);
      }
      *reinterpret_cast<int4*>(mine + t * 8) = make_int4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<int4*>(mine + t * 8 + 4) = make_int4(v[4], v[5], v[6], v[7]);
    }
    __syncthreads();
    if (live) {                                                 // column t: only this thread touches it
      int in[8], out[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) in[r] = mine[r * 8 + t];
      jpeg_idct_1d<11>(in, out);
#pragma unroll
      for (int r = 0; r < 8; ++r) mine[r * 8 + t] = out[r];
    }
    __syncthreads();
    if (live) {                                                 // row t, and its 8 samples
      const int4 lo = *reinterpret_cast<const int4*>(mine + t * 8), hi = *reinterpret_cast<const int4*>(mine + t * 8 + 4);
      const int in[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      int out[8];
      jpeg_idct_1d<18>(in, out);
      unsigned w0 = 0, w1 = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        w0 |= (unsigned)jpeg_sample_of(out[i]) << (8 * i);
        w1 |= (unsigned)jpeg_sample_of(out[4 + i]) << (8 * i);
      }
      const int by = j / bw, bx = j - by * bw;
      const long at = off + ((long)by * 8 + t) * ((long)bw * 8) + (long)bx * 8;                 // a multiple of 8
      if (at + 8 <= p.coef_elems) *reinterpret_cast<uint2*>(p.planes + at) = make_uint2(w0, w1);
    }
    __syncthreads();                                            // the next step overwrites the tile
  }
}

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const JpegParams p) {
  const int b = blockIdx.x;
  const JpegGeom g = jpeg_geom(p.images[b], p.coef_elems, p.pixels_bytes);
  const int quads = (g.w + 3) / 4;
  const long items = (long)quads * g.h;
  for (long q = (long)blockIdx.y * 256 + threadIdx.x; q < items; q += (long)gridDim.y * 256) {
    int y, x0;
    if (q <= 0x7fffffffL) { y = (int)((unsigned)q / (unsigned)quads); x0 = (int)((unsigned)q - (unsigned)y * (unsigned)quads) * 4; }
    else { y = (int)(q / quads); x0 = (int)(q - (long)y * quads) * 4; }
    const int n = min(4, g.w - x0);
    unsigned char o[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int rgb[3] = {0, 0, 0};
      if (i < n) jpeg_pixel_at(g, p.planes, p.coef_elems, x0 + i, y, rgb);
      o[3 * i] = (unsigned char)rgb[0]; o[3 * i + 1] = (unsigned char)rgb[1]; o[3 * i + 2] = (unsigned char)rgb[2];
    }
    const long at = g.pix + ((long)y * g.w + x0) * 3;
    unsigned char* dst = p.pixels + at;
    if (n == 4 && at + 12 <= p.pixels_bytes && ((uintptr_t)dst & 3) == 0) {
      unsigned* d4 = reinterpret_cast<unsigned*>(dst);
#pragma unroll
      for (int i = 0; i < 3; ++i)
        d4[i] = (unsigned)o[4 * i] | ((unsigned)o[4 * i + 1] << 8) | ((unsigned)o[4 * i + 2] << 16) | ((unsigned)o[4 * i + 3] << 24);
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i)
        if (i < 3 * n && at + i < p.pixels_bytes) dst[i] = o[i];
    }
  }
}

}  // namespace

hipError_t launch_jpeg_pixels(const JpegParams& p, hipStream_t st) {
  const dim3 grid((unsigned)p.B, (unsigned)p.parts);
  hipLaunchKernelGGL(jpeg_idct_kernel, grid, dim3(256), 0, st, p);
  hipLaunchKernelGGL(jpeg_colour_kernel, grid, dim3(256), 0, st, p);
  return hipGetLastError();
}
#endif  // MMT_JPEG_HOST_ONLY

}  // namespace mmt

extern "C" {

int mmt_jpeg_info(const uint8_t* bytes, int64_t len, mmt_jpeg_image* out) {
  int rc = mmt::check_bytes("mmt_jpeg_info", bytes, len);
  if (rc) return rc;
  if (!out) return mmt::fail(MMT_E_INVALID, "mmt_jpeg_info: out is NULL");
  mmt::Stream* s = new mmt::Stream();                           // 10 KB of tables: not on the caller's stack
  s->p = bytes; s->end = bytes + len;
  rc = mmt::read_headers(*s);
  if (rc == MMT_OK) mmt::fill_image(s->f, out);
  delete s;
  return rc;
}

int mmt_jpeg_coefficients(const uint8_t* bytes, int64_t len, const mmt_jpeg_image* image, int16_t* coef, int64_t coef_elems,
                          uint16_t* qtables_out) {
  int rc = mmt::check_bytes("mmt_jpeg_coefficients", bytes, len);
  if (rc) return rc;
  if (!image || !coef || !qtables_out) return mmt::fail(MMT_E_INVALID, "mmt_jpeg_coefficients: NULL argument (image, coef and qtables_out are required)");
  mmt::Stream* s = new mmt::Stream();
  s->p = bytes; s->end = bytes + len;
  rc = mmt::read_headers(*s);
  bool seen[3] = {false, false, false};
  if (rc == MMT_OK) {
    mmt_jpeg_image own;
    mmt::fill_image(s->f, &own);
    bool same = image->width == own.width && image->height == own.height && image->components == own.components;
    for (int c = 0; same && c < own.components; ++c) {
      same = image->h_samp[c] == own.h_samp[c] && image->v_samp[c] == own.v_samp[c] && image->blocks_w[c] == own.blocks_w[c] &&
             image->blocks_h[c] == own.blocks_h[c];
      const int64_t n = (int64_t)own.blocks_w[c] * own.blocks_h[c] * 64;
      if (same && (image->coef_offset[c] < 0 || image->coef_offset[c] > coef_elems || n > coef_elems - image->coef_offset[c]))
        rc = mmt::fail(MMT_E_INVALID, "mmt_jpeg_coefficients: the plane of component %d (%lld elements from %lld) leaves coef (%lld elements)",
                       c, (long long)n, (long long)image->coef_offset[c], (long long)coef_elems);
    }
    if (!same) rc = mmt::fail(MMT_E_INVALID, "mmt_jpeg_coefficients: image does not describe this stream (take it from mmt_jpeg_info)");
    if (rc == MMT_OK) {
      std::memset(qtables_out, 0, 3 * 64 * sizeof(uint16_t));
      for (int c = 0; c < own.components; ++c)
        std::memset(coef + image->coef_offset[c], 0, (size_t)own.blocks_w[c] * own.blocks_h[c] * 64 * sizeof(int16_t));
    }
  }
  while (rc == MMT_OK) {                                        // behind an SOS marker
    rc = mmt::read_scan(*s, *image, coef, qtables_out, seen);
    if (rc) break;
    int m;
    for (;;) {
      m = mmt::next_marker(*s);
      if (m < 0) { rc = mmt::fail(MMT_E_INVALID, "jpeg: truncated: the data ends without an EOI marker"); break; }
      if (m == 0xda || m == 0xd9) break;
      if (m >= 0xd0 && m <= 0xd7) { rc = mmt::fail(MMT_E_INVALID, "jpeg: corrupt: a restart marker outside a scan"); break; }
      if (mmt::bare_marker(m)) continue;
      if (m >= 0xc0 && m <= 0xcf && m != 0xc4) { rc = mmt::fail(MMT_E_INVALID, "jpeg: a second frame header"); break; }
      rc = mmt::read_segment(*s, m);
      if (rc) break;
    }
    if (rc || m == 0xd9) break;
  }
  if (rc == MMT_OK)
    for (int c = 0; c < s->f.nc; ++c)
      if (!seen[c]) { rc = mmt::fail(MMT_E_INVALID, "jpeg: truncated: no scan holds component %d", c); break; }
  delete s;
  return rc;
}

int mmt_jpeg_scan_plan(const uint8_t* bytes, int64_t len, const mmt_jpeg_image* image, int32_t subseq_bytes, mmt_jpeg_scan* scan_out,
                       uint32_t* huff_out, uint16_t* qtables_out, int32_t* segments_out, int64_t segment_capacity, int32_t* subseqs_out,
                       int64_t subseq_capacity) {
  int rc = mmt::check_bytes("mmt_jpeg_scan_plan", bytes, len);
  if (rc) return rc;
  if (!image || !scan_out) return mmt::fail(MMT_E_INVALID, "mmt_jpeg_scan_plan: NULL argument (image and scan_out are required)");
  if (subseq_bytes < 8 || subseq_bytes > 1024 || (subseq_bytes & (subseq_bytes - 1)))
    return mmt::fail(MMT_E_INVALID, "mmt_jpeg_scan_plan: subseq_bytes (%d) must be a power of two in [8, 1024]", subseq_bytes);
  const bool report = !segments_out && !subseqs_out;
  if (!report && (!segments_out || !subseqs_out || segment_capacity < 0 || subseq_capacity < 0))
    return mmt::fail(MMT_E_INVALID, "mmt_jpeg_scan_plan: segments_out and subseqs_out go together, with capacities >= 0");
  mmt::Stream* s = new mmt::Stream();
  s->p = bytes; s->end = bytes + len;
  rc = mmt::read_headers(*s);
  mmt::ScanComp sc[3];
  int ns = 0;
  unsigned short q[3 * 64];
  bool seen[3] = {false, false, false};
  if (rc == MMT_OK) {
    mmt_jpeg_image own;
    mmt::fill_image(s->f, &own);
    bool same = image->width == own.width && image->height == own.height && image->components == own.components;
    for (int c = 0; same && c < own.components; ++c)
      same = image->h_samp[c] == own.h_samp[c] && image->v_samp[c] == own.v_samp[c] && image->blocks_w[c] == own.blocks_w[c] &&
             image->blocks_h[c] == own.blocks_h[c];
    if (!same) rc = mmt::fail(MMT_E_INVALID, "mmt_jpeg_scan_plan: image does not describe this stream (take it from mmt_jpeg_info)");
    else if (own.coef_elems >= ((int64_t)1 << 31))
      rc = mmt::fail(MMT_E_UNSUPPORTED, "jpeg: %lld coefficients are too many for the device entropy decode: the host decode takes it",
                     (long long)own.coef_elems);
  }
  if (rc == MMT_OK) {
    std::memset(q, 0, sizeof(q));
    rc = mmt::read_scan_header(*s, sc, ns, q, seen);
  }
  if (rc == MMT_OK && ns != s->f.nc)
    rc = mmt::fail(MMT_E_UNSUPPORTED, "jpeg: more than one scan (the first holds %d of %d components): the host decode takes it", ns, s->f.nc);
  if (rc == MMT_OK && ns == 3 && (sc[0].c != 0 || sc[1].c != 1 || sc[2].c != 2))
    rc = mmt::fail(MMT_E_UNSUPPORTED, "jpeg: a scan whose components are not in frame order: the host decode takes it");
  if (rc == MMT_OK) {
    const mmt::Frame& f = s->f;
    const int64_t mcus = (int64_t)f.mcus_x * f.mcus_y;          // a lone component has h = v = 1: its blocks are the MCUs
    const int64_t expected = s->restart ? (mcus + s->restart - 1) / s->restart : 1;
    const unsigned char* first = s->p;
    int64_t nseg = 0, nsub = 0, longest = 0;
    bool fits = true;
    const unsigned char* scan_end = mmt::walk_segments(first, s->end, expected, [&](const unsigned char* b, const unsigned char* e) {
      const int64_t subs = e - b > subseq_bytes ? (e - b + subseq_bytes - 1) / subseq_bytes : 1;      // an empty segment has one too
      if (!report) {
        if (nseg < segment_capacity && nsub + subs <= subseq_capacity && e - first < ((int64_t)1 << 28)) {
          int32_t* g = segments_out + nseg * 4;
          g[0] = (int32_t)(b - first); g[1] = (int32_t)(e - first);
          g[2] = (int32_t)(nseg * s->restart); g[3] = (int32_t)nsub;
          for (int64_t i = 0; i < subs; ++i) subseqs_out[nsub + i] = (int32_t)nseg;
        } else {
          fits = false;
        }
      }
      ++nseg; nsub += subs;
      if (subs > longest) longest = subs;
    });
    if (scan_end - first >= ((int64_t)1 << 28) || nsub >= ((int64_t)1 << 30))
      rc = mmt::fail(MMT_E_UNSUPPORTED, "jpeg: a scan of %lld bytes is too long for the device entropy decode: the host decode takes it",
                     (long long)(scan_end - first));
    else if (!fits)
      rc = mmt::fail(MMT_E_INVALID, "mmt_jpeg_scan_plan: %lld segments and %lld subsequences needed, room for %lld and %lld given",
                     (long long)nseg, (long long)nsub, (long long)segment_capacity, (long long)subseq_capacity);
    if (rc == MMT_OK) {
      std::memset(scan_out, 0, sizeof(*scan_out));
      scan_out->byte_offset = first - bytes; scan_out->byte_count = scan_end - first;
      scan_out->n_segments = (int32_t)nseg; scan_out->n_subseq = (int32_t)nsub; scan_out->max_segment_subseq = (int32_t)longest;
      scan_out->components = ns; scan_out->restart_interval = s->restart; scan_out->mcus = (int32_t)mcus;
      scan_out->subseq_bytes = subseq_bytes;
      scan_out->uniform_tables = 1;
      for (int i = 0; i < ns; ++i) {
        scan_out->dc_table[i] = sc[i].td; scan_out->ac_table[i] = sc[i].ta;
        if (sc[i].td != sc[0].td || sc[i].ta != sc[0].ta) scan_out->uniform_tables = 0;
      }
      if (huff_out) {
        std::memset(huff_out, 0, 6 * MMT_JPEG_HUFF_WORDS * sizeof(uint32_t));
        for (int i = 0; i < ns; ++i) {
          mmt::device_huff(s->dc[sc[i].td], huff_out + (2 * i) * MMT_JPEG_HUFF_WORDS);
          mmt::device_huff(s->ac[sc[i].ta], huff_out + (2 * i + 1) * MMT_JPEG_HUFF_WORDS);
        }
      }
      if (qtables_out) std::memcpy(qtables_out, q, sizeof(q));
      s->p = scan_end;
    }
  }
  while (rc == MMT_OK) {                                        // behind the scan, as mmt_jpeg_coefficients goes on: up to EOI
    const int m = mmt::next_marker(*s);
    if (m < 0) { rc = mmt::fail(MMT_E_INVALID, "jpeg: truncated: the data ends without an EOI marker"); break; }
    if (m == 0xd9) break;
    if (m == 0xda) { rc = mmt::fail(MMT_E_UNSUPPORTED, "jpeg: more than one scan: the host decode takes it"); break; }
    if (m >= 0xd0 && m <= 0xd7) { rc = mmt::fail(MMT_E_INVALID, "jpeg: corrupt: a restart marker outside a scan"); break; }
    if (mmt::bare_marker(m)) continue;
    if (m >= 0xc0 && m <= 0xcf && m != 0xc4) { rc = mmt::fail(MMT_E_INVALID, "jpeg: a second frame header"); break; }
    rc = mmt::read_segment(*s, m);
  }
  delete s;
  return rc;
}

size_t mmt_jpeg_workspace_bytes(int64_t coef_elems) { return coef_elems < 64 ? 0 : (size_t)coef_elems; }

int mmt_jpeg_pixels_host(int32_t B, const mmt_jpeg_image* images, const int16_t* coef, int64_t coef_elems, const uint16_t* qtables,
                         uint8_t* pixels_out, int64_t pixels_bytes, void* workspace, size_t workspace_bytes) {
  const int rc = mmt::check_stage2("mmt_jpeg_pixels_host", B, images, coef, coef_elems, qtables, pixels_out, pixels_bytes, workspace, workspace_bytes);
  if (rc) return rc;
  unsigned char* planes = (unsigned char*)workspace;
  for (int b = 0; b < B; ++b) {
    const mmt::JpegGeom g = mmt::jpeg_geom(images[b], coef_elems, pixels_bytes);
    const int total = g.nblk[0] + g.nblk[1] + g.nblk[2];
    for (int blk = 0; blk < total; ++blk) {
      int j = blk;
      const int c = mmt::jpeg_component_of(g, j);
      const long src = g.off[c] + (long)j * 64 < coef_elems - 64 ? g.off[c] + (long)j * 64 : coef_elems - 64;
      const uint16_t* q = qtables + ((size_t)b * 3 + c) * 64;
      int tile[8][8];
      for (int t = 0; t < 8; ++t) {                             // columns
        int in[8], out[8];
        for (int r = 0; r < 8; ++r) in[r] = (int)coef[src + r * 8 + t] * (int)q[r * 8 + t];
        mmt::jpeg_idct_1d<11>(in, out);
        for (int r = 0; r < 8; ++r) tile[r][t] = out[r];
      }
      const int by = j / g.bw[c], bx = j - by * g.bw[c];
      for (int t = 0; t < 8; ++t) {                             // rows
        int out[8];
        mmt::jpeg_idct_1d<18>(tile[t], out);
        const long at = g.off[c] + ((long)by * 8 + t) * ((long)g.bw[c] * 8) + (long)bx * 8;
        if (at + 8 <= coef_elems)
          for (int i = 0; i < 8; ++i) planes[at + i] = (unsigned char)mmt::jpeg_sample_of(out[i]);
      }
    }
    for (int y = 0; y < g.h; ++y)
      for (int x = 0; x < g.w; ++x) {
        int rgb[3];
        mmt::jpeg_pixel_at(g, planes, coef_elems, x, y, rgb);
        const long at = g.pix + ((long)y * g.w + x) * 3;
        for (int i = 0; i < 3; ++i)
          if (at + i < pixels_bytes) pixels_out[at + i] = (unsigned char)rgb[i];
      }
  }
  return MMT_OK;
}

#ifndef MMT_JPEG_HOST_ONLY
int mmt_jpeg_pixels(int32_t B, const mmt_jpeg_image* images, const int16_t* coef, int64_t coef_elems, const uint16_t* qtables,
                    uint8_t* pixels_out, int64_t pixels_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = mmt::check_stage2("mmt_jpeg_pixels", B, images, coef, coef_elems, qtables, pixels_out, pixels_bytes, workspace, workspace_bytes);
  if (rc) return rc;
  if (B > 65535) return mmt::fail(MMT_E_UNSUPPORTED, "mmt_jpeg_pixels: B (%d) above 65535", B);
  mmt::JpegParams p;
  p.B = B;
  // about one workgroup per 4 steps of 32 blocks of an image of average size, between 8 and 256 per image
  const int64_t per_image = coef_elems / 64 / B / (4 * mmt::kJpegGroup);
  p.parts = per_image < 8 ? 8 : (per_image > 256 ? 256 : (int)per_image);
  p.images = images; p.coef = coef; p.coef_elems = coef_elems; p.qtables = qtables;
  p.pixels = pixels_out; p.pixels_bytes = pixels_bytes; p.planes = (unsigned char*)workspace;
  const hipError_t e = mmt::launch_jpeg_pixels(p, (hipStream_t)stream);
  return e == hipSuccess ? MMT_OK : mmt::fail(MMT_E_LAUNCH, "mmt_jpeg_pixels: %s", hipGetErrorString(e));
}
#endif

}  // extern "C"
