// PNG decode in front of the image front end (C ABI: include/mmt_layer.h, mmt_png_*): `tf.io.decode_image` of
// `decode_fn` (src/data/data_utils.py:195) for PNG bytes -- the reference's Fashion-Gen shards store PNG files
// (preprocessing/create_fashion_gen_split.py:31,66) -- as libpng decodes with palette and low-bit grey expansion.
// DESIGN.md section 4 "PNG decode" states the rules and the accepted files.
//
//   host    mmt_png_info, mmt_png_inflate: the chunk walk (CRC-32 of the critical chunks) and DEFLATE -- serial by
//           nature, plain C++ that a sanitizer checks; a corrupt file can do no harm there.  The inflate is the
//           library's own: a 64-bit bit buffer that is refilled across IDAT boundaries (the payloads are never
//           copied together), a 10-bit lookup per Huffman code with the canonical walk behind it for longer codes,
//           output straight into the caller's buffer, which also serves as the window.  Output: the filtered
//           scanlines, per pass rows x (1 + row bytes), and the palette.
//           mmt_png_gather: the same chunk walk without the DEFLATE -- the IDAT payloads back to back, for the inflate on
//           the device (png_inflate.hip).
//   device  one kernel, grid (images, 7), one wave per (image, pass): an anti-diagonal wavefront over bands of 64 rows.
//           Lane r of a band reconstructs filter unit x of its row at step x + r; the unit above comes from lane r - 1
//           by a lane shift (it was reconstructed one step earlier), the unit above left is the one received the step
//           before.  Lane 0 takes the row above from the row the previous band's lane 63 kept in the workspace, 64
//           units per coalesced load, one chunk ahead.  A lane loads the raw units of 32 steps ahead of their use, so
//           the dependency chain holds no memory access.  The step that reconstructs a unit also expands it (grey
//           scaling, palette lookup from LDS) and scatters its pixels to their Adam7 positions.  raw is only read.
//   mmt_png_pixels_host is the same arithmetic as loops over host memory, through the functions of png_decode.h.
//
// Bounds (the front end's rule): png_geom() and png_pass() clamp sizes, offsets and pass geometry into the buffers; on
// top of it no pixel is written at or beyond the end of pixels_out, and a palette index is a byte into 256 entries.
#include "../../include/mmt_attn.h"
#include "../../include/mmt_layer.h"

#include <cstdint>
#include <cstring>

#include "mmt_err.h"
#include "png_decode.h"

namespace mmt {
namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Host stage: checksums, chunks, inflate.
// ---------------------------------------------------------------------------------------------------------------------
struct CrcTable {
  uint32_t t[8][256];
  CrcTable() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (c & 1 ? 0xEDB88320u : 0u);
      t[0][i] = c;
    }
    for (uint32_t i = 0; i < 256; ++i)
      for (int k = 1; k < 8; ++k) t[k][i] = (t[k - 1][i] >> 8) ^ t[0][t[k - 1][i] & 255u];
  }
};

uint32_t crc32_of(const uint8_t* p, int64_t n) {
  static const CrcTable tab;                                    // initialised once, thread-safe
  uint32_t c = 0xFFFFFFFFu;
  while (n >= 8) {
    const uint32_t lo = c ^ ((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
    c = tab.t[7][lo & 255u] ^ tab.t[6][(lo >> 8) & 255u] ^ tab.t[5][(lo >> 16) & 255u] ^ tab.t[4][lo >> 24] ^
        tab.t[3][p[4]] ^ tab.t[2][p[5]] ^ tab.t[1][p[6]] ^ tab.t[0][p[7]];
    p += 8; n -= 8;
  }
  for (; n > 0; --n) c = tab.t[0][(c ^ *p++) & 255u] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

uint32_t adler32_of(const uint8_t* p, int64_t n) {
  uint32_t a = 1, b = 0;
  while (n > 0) {
    const int64_t m = n < 5552 ? n : 5552;                      // the most bytes before b can pass 2^32
    for (int64_t i = 0; i < m; ++i) { a += p[i]; b += a; }
    a %= 65521u; b %= 65521u;
    p += m; n -= m;
  }
  return (b << 16) | a;
}

inline uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3]; }
inline bool is_type(const uint8_t* p, const char* t) { return std::memcmp(p, t, 4) == 0; }

const uint8_t kSignature[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};

// One chunk at `at`: its payload and type, checked to lie inside the file.  MMT_E_INVALID when the file ends first.
struct Chunk {
  const uint8_t* type;
  const uint8_t* data;
  int64_t size;
};

int read_chunk(const uint8_t* bytes, int64_t len, int64_t at, Chunk& c) {
  if (len - at < 12) return fail(MMT_E_INVALID, "png: truncated: the file ends inside a chunk header at byte %lld", (long long)at);
  const uint32_t n = be32(bytes + at);
  if (n > 0x7fffffffu) return fail(MMT_E_INVALID, "png: corrupt: a chunk length above 2^31 - 1 at byte %lld", (long long)at);
  if ((int64_t)n > len - at - 12)
    return fail(MMT_E_INVALID, "png: truncated: the %.4s chunk at byte %lld (%u bytes) leaves the file", (const char*)(bytes + at + 4), (long long)at, n);
  c.type = bytes + at + 4; c.data = bytes + at + 8; c.size = n;
  return MMT_OK;
}

int check_crc(const Chunk& c) {
  if (crc32_of(c.type, c.size + 4) != be32(c.data + c.size))
    return fail(MMT_E_INVALID, "png: corrupt: CRC-32 mismatch on a %.4s chunk", (const char*)c.type);
  return MMT_OK;
}

struct Header {
  mmt_png_image im;
  const uint8_t* plte;                  // the PLTE payload, NULL without one
  int64_t first_idat;                   // offset of the first IDAT chunk
};

int64_t raw_size(int w, int h, int depth, int color_type, int interlace) {
  mmt_png_image im;
  std::memset(&im, 0, sizeof(im));
  im.width = w; im.height = h; im.bit_depth = depth; im.color_type = color_type; im.interlace = interlace;
  im.raw_bytes = (int64_t)1 << 62;
  const PngGeom g = png_geom(im, (int64_t)1 << 62, (int64_t)1 << 62);
  int64_t total = 0;
  for (int p = 0; p < g.passes; ++p) {
    PngPass s;
    png_pass_size(g, p, s);
    total += (int64_t)s.rows * (1 + s.rowbytes);
  }
  return total;
}

// Signature, IHDR and the chunks up to the first IDAT.
int read_header(const uint8_t* bytes, int64_t len, Header& h) {
  if (len < 1 || bytes[0] != kSignature[0]) return fail(MMT_E_UNSUPPORTED, "png: not a PNG file (the first byte is not 0x89)");
  if (len < 8) return fail(MMT_E_INVALID, "png: truncated: the file ends inside the signature");
  if (std::memcmp(bytes, kSignature, 8) != 0) return fail(MMT_E_INVALID, "png: corrupt: a wrong signature behind a correct first byte");
  Chunk c;
  int rc = read_chunk(bytes, len, 8, c);
  if (rc) return rc;
  if (!is_type(c.type, "IHDR") || c.size != 13) return fail(MMT_E_INVALID, "png: corrupt: the first chunk is not an IHDR of 13 bytes");
  if ((rc = check_crc(c))) return rc;
  const uint32_t w = be32(c.data), hgt = be32(c.data + 4);
  const int depth = c.data[8], ct = c.data[9], comp = c.data[10], filt = c.data[11], lace = c.data[12];
  if (w == 0 || hgt == 0 || w > 0x7fffffffu || hgt > 0x7fffffffu)
    return fail(MMT_E_INVALID, "png: invalid IHDR: width %u or height %u is 0 or above 2^31 - 1", w, hgt);
  const bool depth_ok = ct == 0 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16)
                                : (ct == 3 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8)
                                           : ((ct == 2 || ct == 4 || ct == 6) && (depth == 8 || depth == 16)));
  if (!depth_ok) return fail(MMT_E_INVALID, "png: invalid IHDR: colour type %d with bit depth %d", ct, depth);
  if (ct == 4 || ct == 6) return fail(MMT_E_UNSUPPORTED, "png: colour type %d has an alpha channel, which is not supported", ct);
  if (depth == 16) return fail(MMT_E_UNSUPPORTED, "png: bit depth 16 is not supported (the packed layout is uint8)");
  if (comp != 0) return fail(MMT_E_UNSUPPORTED, "png: compression method %d is not supported", comp);
  if (filt != 0) return fail(MMT_E_UNSUPPORTED, "png: filter method %d is not supported", filt);
  if (lace > 1) return fail(MMT_E_INVALID, "png: invalid IHDR: interlace method %d", lace);
  if (w > (uint32_t)kPngMaxSide || hgt > (uint32_t)kPngMaxSide)
    return fail(MMT_E_UNSUPPORTED, "png: width %u or height %u above 2^30 is not supported", w, hgt);
  std::memset(&h.im, 0, sizeof(h.im));
  h.im.width = (int32_t)w; h.im.height = (int32_t)hgt; h.im.bit_depth = depth; h.im.color_type = ct; h.im.interlace = lace;
  h.im.raw_bytes = raw_size((int)w, (int)hgt, depth, ct, lace);
  h.plte = nullptr;
  int64_t at = 8 + 12 + 13;
  for (;;) {
    if (at == len) return fail(MMT_E_INVALID, "png: truncated: the file ends without an IDAT chunk");
    if ((rc = read_chunk(bytes, len, at, c))) return rc;
    if (is_type(c.type, "IDAT")) break;
    if (is_type(c.type, "PLTE")) {
      if ((rc = check_crc(c))) return rc;
      if (h.plte) return fail(MMT_E_INVALID, "png: corrupt: a second PLTE chunk");
      if (c.size % 3 != 0 || c.size == 0) return fail(MMT_E_INVALID, "png: invalid PLTE: a length of %lld bytes is not a positive multiple of 3", (long long)c.size);
      if (ct == 3 && c.size / 3 > (1 << depth))
        return fail(MMT_E_INVALID, "png: invalid PLTE: %lld entries are more than bit depth %d can index", (long long)(c.size / 3), depth);
      if (c.size / 3 > 256) return fail(MMT_E_INVALID, "png: invalid PLTE: %lld entries are more than 256", (long long)(c.size / 3));
      h.plte = c.data;
      h.im.palette_entries = (int32_t)(c.size / 3);
    } else if (is_type(c.type, "tRNS")) {
      return fail(MMT_E_UNSUPPORTED, "png: a tRNS chunk (transparency) is not supported");
    } else if (is_type(c.type, "IEND")) {
      return fail(MMT_E_INVALID, "png: corrupt: IEND without an IDAT chunk");
    } else if (is_type(c.type, "IHDR")) {
      return fail(MMT_E_INVALID, "png: corrupt: a second IHDR chunk");
    } else if (!(c.type[0] & 0x20)) {
      return fail(MMT_E_UNSUPPORTED, "png: unknown critical chunk 0x%02x%02x%02x%02x", c.type[0], c.type[1], c.type[2], c.type[3]);
    }                                                           // ancillary: skipped, its CRC not looked at
    at += 12 + c.size;
  }
  if (ct == 3 && !h.plte) return fail(MMT_E_INVALID, "png: corrupt: a palette image without a PLTE chunk");
  if (h.im.raw_bytes / 1032 > len)                              // DEFLATE expands at most 1032 times
    return fail(MMT_E_INVALID, "png: truncated: %lld bytes cannot inflate to the %lld bytes the IHDR requires (inflated data shorter)",
                (long long)len, (long long)h.im.raw_bytes);
  h.first_idat = at;
  return MMT_OK;
}

// The IDAT payloads as one stream of bits, least significant first.  Behind the last IDAT it yields zero bytes and
// counts them: over() tells whether any of those has been consumed.
struct Bits {
  const uint8_t* file;
  int64_t len;
  int64_t next;                         // offset of the chunk behind the current one
  const uint8_t* p;
  const uint8_t* end;                   // the rest of the current IDAT payload
  uint64_t bits;
  int n;                                // valid bits
  int pad;                              // zero bytes fed behind the data
  int err;                              // a failure of the chunk walk (message set)

  bool advance() {                      // to the next IDAT chunk that follows directly
    while (!err && p == end) {
      Chunk c;
      if (next == len) return false;
      if ((err = read_chunk(file, len, next, c))) return false;
      if (!is_type(c.type, "IDAT")) return false;
      if ((err = check_crc(c))) return false;
      p = c.data; end = c.data + c.size; next += 12 + c.size;
    }
    return !err;
  }
  void refill() {                       // to at least 56 bits
    if (end - p >= 8) {
      uint64_t w;
      std::memcpy(&w, p, 8);            // little endian host
      bits |= w << n;
      p += (63 - n) >> 3;
      n |= 56;
      return;
    }
    while (n <= 56) {
      uint64_t byte = 0;
      if (p == end && !advance()) ++pad; else byte = *p++;
      bits |= byte << n;
      n += 8;
    }
  }
  bool over() const { return pad * 8 > n; }
  unsigned take(int k) { const unsigned v = (unsigned)(bits & ((1ull << k) - 1)); bits >>= k; n -= k; return v; }
};

constexpr int kFast = 10;

struct Huff {
  uint16_t fast[1 << kFast];            // symbol | length << 9 for codes of at most kFast bits, 0 otherwise
  uint16_t count[16];
  uint16_t symbol[288];
};

// zlib's rule: an over-subscribed set is invalid; an incomplete one too, unless it is a single code of one bit (or, for
// distances, no code at all).
int build_huff(Huff& h, const uint8_t* lengths, int n, const char* what) {
  std::memset(h.fast, 0, sizeof(h.fast));
  std::memset(h.count, 0, sizeof(h.count));
  for (int i = 0; i < n; ++i) h.count[lengths[i]]++;
  h.count[0] = 0;
  int left = 1, longest = 0;
  for (int l = 1; l <= 15; ++l) {
    left = (left << 1) - h.count[l];
    if (left < 0) return fail(MMT_E_INVALID, "png: invalid DEFLATE stream: an over-subscribed set of %s code lengths", what);
    if (h.count[l]) longest = l;
  }
  if (left > 0 && longest > 1) return fail(MMT_E_INVALID, "png: invalid DEFLATE stream: an incomplete set of %s code lengths", what);
  uint16_t offs[16];
  offs[1] = 0;
  for (int l = 1; l < 15; ++l) offs[l + 1] = offs[l] + h.count[l];
  uint16_t code[16];
  unsigned c = 0;
  for (int l = 1; l <= 15; ++l) { c = (c + h.count[l - 1]) << 1; code[l] = (uint16_t)c; }
  for (int i = 0; i < n; ++i) {
    const int l = lengths[i];
    if (!l) continue;
    h.symbol[offs[l]++] = (uint16_t)i;
    const unsigned cd = code[l]++;
    if (l <= kFast) {
      unsigned rev = 0;
      for (int k = 0; k < l; ++k) rev |= ((cd >> k) & 1u) << (l - 1 - k);
      for (unsigned at = rev; at < (1u << kFast); at += 1u << l) h.fast[at] = (uint16_t)(i | (l << 9));
    }
  }
  return MMT_OK;
}

inline int decode_symbol(const Huff& h, Bits& b) {
  const unsigned e = h.fast[b.bits & ((1u << kFast) - 1)];
  if (e) { b.bits >>= e >> 9; b.n -= e >> 9; return (int)(e & 511u); }
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= 15; ++l) {
    code |= (int)((b.bits >> (l - 1)) & 1u);
    const int cnt = h.count[l];
    if (code - cnt < first) { b.bits >>= l; b.n -= l; return h.symbol[index + (code - first)]; }
    index += cnt; first += cnt; first <<= 1; code <<= 1;
  }
  return -1;
}

const uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
const uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
const uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
const uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
const uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

int truncated_stream() { return fail(MMT_E_INVALID, "png: truncated: the IDAT data ends inside the DEFLATE stream (inflated data shorter than the IHDR requires)"); }
int too_long(int64_t cap) { return fail(MMT_E_INVALID, "png: corrupt: inflated data longer than the %lld bytes the IHDR requires", (long long)cap); }

// One zlib stream from `b` into out[0, cap): exactly cap bytes, or a refusal.
int inflate_zlib(Bits& b, uint8_t* out, int64_t cap) {
  b.refill();
  const unsigned cmf = b.take(8), flg = b.take(8);
  if (b.over()) return b.err ? b.err : truncated_stream();
  if ((cmf & 15u) != 8) return fail(MMT_E_INVALID, "png: bad zlib header: compression method %u is not 8 (deflate)", cmf & 15u);
  if ((cmf >> 4) > 7) return fail(MMT_E_INVALID, "png: bad zlib header: a window larger than 32 KiB");
  if (((cmf << 8) | flg) % 31 != 0) return fail(MMT_E_INVALID, "png: bad zlib header: the check bits do not match");
  if (flg & 0x20) return fail(MMT_E_INVALID, "png: bad zlib header: a preset dictionary");
  int64_t at = 0;
  Huff lit, dist;                       // 5 KB on the stack
  for (int last = 0; !last;) {
    b.refill();
    last = (int)b.take(1);
    const unsigned type = b.take(2);
    if (type == 3) return fail(MMT_E_INVALID, "png: invalid DEFLATE stream: reserved block type 3");
    if (type == 0) {
      b.take(b.n & 7);
      b.refill();
      const unsigned n = b.take(16), inv = b.take(16);
      if (b.over()) return b.err ? b.err : truncated_stream();
      if ((n ^ inv) != 0xffffu) return fail(MMT_E_INVALID, "png: invalid DEFLATE stream: the length of a stored block does not match its complement");
      if ((int64_t)n > cap - at) return too_long(cap);
      int64_t left = n;
      while (left > 0 && b.n >= 8) { out[at++] = (uint8_t)b.take(8); --left; }    // whole bytes the bit buffer holds
      if (b.over()) return b.err ? b.err : truncated_stream();
      if (left > 0) b.bits = 0;                                 // n == 0: drop what refill() read ahead, p moves on below
      while (left > 0) {
        if (b.p == b.end && !b.advance()) return b.err ? b.err : truncated_stream();
        const int64_t m = b.end - b.p < left ? b.end - b.p : left;
        std::memcpy(out + at, b.p, (size_t)m);
        b.p += m; at += m; left -= m;
      }
      continue;
    }
    if (type == 1) {
      uint8_t lens[288 + 32];
      for (int i = 0; i < 288; ++i) lens[i] = i < 144 ? 8 : (i < 256 ? 9 : (i < 280 ? 7 : 8));
      for (int i = 0; i < 32; ++i) lens[288 + i] = 5;
      build_huff(lit, lens, 288, "literal/length");             // symbols 286, 287, and distances 30, 31, are refused below
      build_huff(dist, lens + 288, 32, "distance");
    } else {
      const int nlen = (int)b.take(5) + 257, ndist = (int)b.take(5) + 1, ncode = (int)b.take(4) + 4;
      if (nlen > 286 || ndist > 30) return fail(MMT_E_INVALID, "png: invalid DEFLATE stream: a bad code-length set (%d length and %d distance codes)", nlen, ndist);
      uint8_t cl[19] = {0};
      b.refill();
      for (int i = 0; i < ncode; ++i) { if (b.n < 3) b.refill(); cl[kClOrder[i]] = (uint8_t)b.take(3); }
      if (b.over()) return b.err ? b.err : truncated_stream();
      int64_t complete = 0;
      for (int i = 0; i < 19; ++i) if (cl[i]) complete += 1 << (7 - cl[i]);
      if (complete != 128) return fail(MMT_E_INVALID, "png: invalid DEFLATE stream: a bad code-length set (the code-length code is not complete)");
      int rc = build_huff(lit, cl, 19, "code-length");           // lit serves as the code-length code first
      if (rc) return rc;
      uint8_t lens[286 + 30];
      int i = 0;
      while (i < nlen + ndist) {
        b.refill();
        const int sym = decode_symbol(lit, b);
        if (b.over()) return b.err ? b.err : truncated_stream();
        if (sym < 0) return fail(MMT_E_INVALID, "png: invalid DEFLATE stream: a bad code-length set (an unused code)");
        if (sym < 16) { lens[i++] = (uint8_t)sym; continue; }
        int rep, val = 0;
        if (sym == 16) {
          if (i == 0) return fail(MMT_E_INVALID, "png: invalid DEFLATE stream: a bad code-length set (a repeat with no length before it)");
          val = lens[i - 1]; rep = 3 + (int)b.take(2);
        } else if (sym == 17) {
          rep = 3 + (int)b.take(3);
        } else {
          rep = 11 + (int)b.take(7);
        }
        if (i + rep > nlen + ndist) return fail(MMT_E_INVALID, "png: invalid DEFLATE stream: a bad code-length set (a repeat past the last code)");
        while (rep--) lens[i++] = (uint8_t)val;
      }
      if (b.over()) return b.err ? b.err : truncated_stream();
      if (lens[256] == 0) return fail(MMT_E_INVALID, "png: invalid DEFLATE stream: a bad code-length set (no end-of-block code)");
      if ((rc = build_huff(lit, lens, nlen, "literal/length"))) return rc;
      if ((rc = build_huff(dist, lens + nlen, ndist, "distance"))) return rc;
    }
    for (;;) {                                                  // the symbols of a compressed block
      b.refill();                                               // 56 bits: a length code, its extra bits, a distance code, its extra bits
      int sym = decode_symbol(lit, b);
      if (sym < 256) {
        if (sym < 0) return b.over() ? (b.err ? b.err : truncated_stream()) : fail(MMT_E_INVALID, "png: invalid DEFLATE stream: an unused literal/length code");
        if (at >= cap) return b.over() ? (b.err ? b.err : truncated_stream()) : too_long(cap);
        out[at++] = (uint8_t)sym;
        continue;
      }
      if (b.pad && b.over()) return b.err ? b.err : truncated_stream();
      if (sym == 256) break;
      sym -= 257;
      if (sym >= 29) return fail(MMT_E_INVALID, "png: invalid DEFLATE stream: length symbol %d", sym + 257);
      const int n = kLenBase[sym] + (int)b.take(kLenExtra[sym]);
      const int ds = decode_symbol(dist, b);
      if (ds < 0 || ds >= 30) return b.over() ? (b.err ? b.err : truncated_stream()) : fail(MMT_E_INVALID, "png: invalid DEFLATE stream: an unused or reserved distance code");
      const int64_t d = kDistBase[ds] + (int64_t)b.take(kDistExtra[ds]);
      if (b.pad && b.over()) return b.err ? b.err : truncated_stream();
      if (d > at) return fail(MMT_E_INVALID, "png: invalid DEFLATE stream: a distance of %lld before the start of the stream (%lld bytes out)", (long long)d, (long long)at);
      if (n > cap - at) return too_long(cap);
      const uint8_t* src = out + at - d;
      uint8_t* dst = out + at;
      if (d >= 8 && n <= cap - at - 8) {                        // 8 bytes at a time; the tail of the last copy stays inside out
        for (int k = 0; k < n; k += 8) std::memcpy(dst + k, src + k, 8);
      } else {
        for (int k = 0; k < n; ++k) dst[k] = src[k];
      }
      at += n;
    }
  }
  b.take(b.n & 7);
  b.refill();
  const uint32_t stored = (uint32_t)b.take(8) << 24 | (uint32_t)b.take(8) << 16 | (uint32_t)b.take(8) << 8 | (uint32_t)b.take(8);
  if (b.over()) return b.err ? b.err : truncated_stream();
  if (at != cap) return fail(MMT_E_INVALID, "png: corrupt: inflated data shorter than the IHDR requires (%lld of %lld bytes)", (long long)at, (long long)cap);
  if (adler32_of(out, cap) != stored) return fail(MMT_E_INVALID, "png: corrupt: Adler-32 mismatch on the inflated data");
  return MMT_OK;
}

int check_bytes(const char* who, const uint8_t* bytes, int64_t len) {
  if (!bytes) return fail(MMT_E_INVALID, "%s: bytes is NULL", who);
  if (len < 0) return fail(MMT_E_INVALID, "%s: len (%lld) is negative", who, (long long)len);
  return MMT_OK;
}

int check_stage2(const char* who, int32_t B, const mmt_png_image* images, const uint8_t* raw, int64_t raw_bytes, const uint8_t* palettes,
                 uint8_t* pixels_out, int64_t pixels_bytes, void* workspace, size_t workspace_bytes) {
  if (B < 1) return fail(MMT_E_INVALID, "%s: B (%d) must be positive", who, B);
  if (!images || !raw || !palettes || !pixels_out)
    return fail(MMT_E_INVALID, "%s: NULL argument (images, raw, palettes and pixels_out are required)", who);
  if (raw_bytes < 1 || raw_bytes >= ((int64_t)1 << 60)) return fail(MMT_E_INVALID, "%s: raw_bytes %lld outside [1, 2^60)", who, (long long)raw_bytes);
  if (pixels_bytes < 1 || pixels_bytes >= ((int64_t)1 << 60))
    return fail(MMT_E_INVALID, "%s: pixels_bytes %lld outside [1, 2^60)", who, (long long)pixels_bytes);
  const size_t need = mmt_png_workspace_bytes(raw_bytes);
  if (!workspace || workspace_bytes < need)
    return fail(MMT_E_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", who, need, workspace ? workspace_bytes : (size_t)0);
  return MMT_OK;
}

// A unit of the kept row or of the raw row: BPP bytes from p, byte k in bits [8k, 8k + 8).
template <int BPP>
__host__ __device__ inline unsigned png_load_unit(const unsigned char* p) {
  unsigned v = 0;
#pragma unroll
  for (int k = 0; k < BPP; ++k) v |= (unsigned)p[k] << (8 * k);
  return v;
}

inline void pack_palette(const uint8_t* pal, unsigned* out) {
  for (int i = 0; i < 256; ++i) out[i] = (unsigned)pal[3 * i] | (unsigned)pal[3 * i + 1] << 8 | (unsigned)pal[3 * i + 2] << 16;
}

template <int BPP>
void png_pass_host(const PngParams& p, const PngGeom& g, const PngPass& s, const unsigned* pal) {
  unsigned char* keep = p.keep + s.off;                         // s.rowbytes bytes, inside the workspace
  for (int row = 0; row < s.rows; ++row) {
    const unsigned char* src = p.raw + s.off + (long)row * (1 + s.rowbytes);
    const int ft = src[0] > 4 ? 0 : src[0];
    unsigned cur = 0, corner = 0;
    for (int x = 0; x < s.units; ++x) {
      const unsigned up = row ? png_load_unit<BPP>(keep + (long)x * BPP) : 0u;
      cur = png_recon_unit<BPP>(ft, png_load_unit<BPP>(src + 1 + (long)x * BPP), x ? cur : 0u, up, x ? corner : 0u);
      corner = up;
      for (int k = 0; k < BPP; ++k) keep[(long)x * BPP + k] = (unsigned char)(cur >> (8 * k));
      png_emit(g, s, pal, row, x, cur, p.pixels, p.pixels_bytes);
    }
  }
}

}  // namespace

#ifndef MMT_PNG_HOST_ONLY
namespace {

template <int BPP>
__device__ inline void png_pass_wave(const PngParams& p, const PngGeom& g, const PngPass& s, const unsigned* pal) {
  const int lane = threadIdx.x;
  unsigned char* keep = p.keep + s.off;
  const int units = s.units;
  const int nsteps = units + kPngBand - 1;                      // lane 63 finishes its row 63 steps behind lane 0
  const int nbands = (s.rows + kPngBand - 1) / kPngBand;
  for (int band = 0; band < nbands; ++band) {
    const int row = band * kPngBand + lane;
    const bool live = row < s.rows;
    const unsigned char* src = p.raw + s.off + (long)(live ? row : 0) * (1 + s.rowbytes);
    int ft = src[0];
    if (ft > 4) ft = 0;
    ++src;
    // the unit of step t for this lane; a step outside the row reads the row's first unit and is not used
    auto raw_unit = [&](int t) {
      const int x = t - lane;
      return png_load_unit<BPP>(src + (x >= 0 && x < units ? (long)x * BPP : 0L));
    };
    // unit u of the row the previous band kept, for lane 0
    auto kept_unit = [&](int u) { return band > 0 && u < units ? png_load_unit<BPP>(keep + (long)u * BPP) : 0u; };
    unsigned buf[kPngGroup], nxt[kPngGroup];
#pragma unroll
    for (int i = 0; i < kPngGroup; ++i) buf[i] = raw_unit(i);
    unsigned above0 = kept_unit(lane), above1 = 0;
    unsigned cur = 0, upv = 0;
    for (int s0 = 0; s0 < nsteps; s0 += kPngGroup) {
#pragma unroll
      for (int i = 0; i < kPngGroup; ++i) nxt[i] = raw_unit(s0 + kPngGroup + i);
      if ((s0 & (kPngBand - 1)) == 0) above1 = kept_unit(s0 + kPngBand + lane);
#pragma unroll
      for (int i = 0; i < kPngGroup; ++i) {
        const int t = s0 + i, x = t - lane;
        unsigned up = __shfl_up(cur, 1);
        const unsigned top = __shfl(above0, t & (kPngBand - 1));
        if (lane == 0) up = top;
        const bool first = x == 0;
        const unsigned v = png_recon_unit<BPP>(ft, buf[i], first ? 0u : cur, up, first ? 0u : upv);
        upv = up;
        if (live && x >= 0 && x < units) {
          cur = v;
          png_emit(g, s, pal, row, x, v, p.pixels, p.pixels_bytes);
          if (lane == kPngBand - 1) {
#pragma unroll
            for (int k = 0; k < BPP; ++k) keep[(long)x * BPP + k] = (unsigned char)(v >> (8 * k));
          }
        }
      }
      if ((s0 & (kPngBand - 1)) == kPngBand - kPngGroup) above0 = above1;
#pragma unroll
      for (int i = 0; i < kPngGroup; ++i) buf[i] = nxt[i];
    }
    __syncthreads();                                            // the kept row is read by the next band
  }
}

__global__ __launch_bounds__(kPngBand) void png_pixels_kernel(const PngParams p) {
  const int b = blockIdx.x, pass = blockIdx.y;
  __shared__ unsigned pal[256];
  const unsigned char* pb = p.palettes + (size_t)b * 768;
  for (int i = threadIdx.x; i < 256; i += kPngBand) pal[i] = (unsigned)pb[3 * i] | (unsigned)pb[3 * i + 1] << 8 | (unsigned)pb[3 * i + 2] << 16;
  __syncthreads();
  const PngGeom g = png_geom(p.images[b], p.raw_bytes, p.pixels_bytes);
  if (pass >= g.passes) return;
  const PngPass s = png_pass(g, pass);
  if (s.rows == 0) return;
  if (g.bpp == 3) png_pass_wave<3>(p, g, s, pal);
  else png_pass_wave<1>(p, g, s, pal);
}

}  // namespace

hipError_t launch_png_pixels(const PngParams& p, hipStream_t st) {
  hipLaunchKernelGGL(png_pixels_kernel, dim3((unsigned)p.B, 7), dim3(kPngBand), 0, st, p);
  return hipGetLastError();
}
#endif  // MMT_PNG_HOST_ONLY

}  // namespace mmt

extern "C" {

int mmt_png_info(const uint8_t* bytes, int64_t len, mmt_png_image* out) {
  int rc = mmt::check_bytes("mmt_png_info", bytes, len);
  if (rc) return rc;
  if (!out) return mmt::fail(MMT_E_INVALID, "mmt_png_info: out is NULL");
  mmt::Header h;
  rc = mmt::read_header(bytes, len, h);
  if (rc == MMT_OK) *out = h.im;
  return rc;
}

int mmt_png_inflate(const uint8_t* bytes, int64_t len, const mmt_png_image* image, uint8_t* raw_out, int64_t raw_capacity,
                    uint8_t* palette_out) {
  int rc = mmt::check_bytes("mmt_png_inflate", bytes, len);
  if (rc) return rc;
  if (!image || !raw_out || !palette_out)
    return mmt::fail(MMT_E_INVALID, "mmt_png_inflate: NULL argument (image, raw_out and palette_out are required)");
  mmt::Header h;
  if ((rc = mmt::read_header(bytes, len, h))) return rc;
  const mmt_png_image& own = h.im;
  if (image->width != own.width || image->height != own.height || image->bit_depth != own.bit_depth || image->color_type != own.color_type ||
      image->interlace != own.interlace || image->palette_entries != own.palette_entries || image->raw_bytes != own.raw_bytes)
    return mmt::fail(MMT_E_INVALID, "mmt_png_inflate: image does not describe this stream (take it from mmt_png_info)");
  if (image->raw_offset < 0 || image->raw_offset > raw_capacity || own.raw_bytes > raw_capacity - image->raw_offset)
    return mmt::fail(MMT_E_INVALID, "mmt_png_inflate: the scanlines (%lld bytes from %lld) leave raw_out (%lld bytes)", (long long)own.raw_bytes,
                     (long long)image->raw_offset, (long long)raw_capacity);
  std::memset(palette_out, 0, 768);
  if (h.plte) std::memcpy(palette_out, h.plte, (size_t)own.palette_entries * 3);
  mmt::Bits b;
  b.file = bytes; b.len = len; b.next = h.first_idat; b.p = b.end = nullptr; b.bits = 0; b.n = 0; b.pad = 0; b.err = 0;
  uint8_t* raw = raw_out + image->raw_offset;
  rc = mmt::inflate_zlib(b, raw, own.raw_bytes);
  if (b.err) return b.err;                                      // a chunk failure outranks what the missing bytes caused
  if (rc) return rc;
  // every filter-type byte: the host knows where each row starts
  const mmt::PngGeom g = mmt::png_geom(own, (int64_t)1 << 62, (int64_t)1 << 62);
  int64_t at = 0;
  for (int p = 0; p < g.passes; ++p) {
    mmt::PngPass s;
    mmt::png_pass_size(g, p, s);
    for (int r = 0; r < s.rows; ++r, at += 1 + s.rowbytes)
      if (raw[at] > 4) return mmt::fail(MMT_E_INVALID, "png: corrupt: filter-type byte %d above 4 on row %d of pass %d", raw[at], r, p + 1);
  }
  // behind the stream: more IDAT (ignored, as libpng does, but for its CRC), ancillary chunks, IEND
  b.p = b.end;
  for (int64_t next = b.next;;) {
    mmt::Chunk c;
    if (next == len) return mmt::fail(MMT_E_INVALID, "png: truncated: the file ends without an IEND chunk");
    if ((rc = mmt::read_chunk(bytes, len, next, c))) return rc;
    if (mmt::is_type(c.type, "IEND")) return mmt::check_crc(c);
    if (mmt::is_type(c.type, "IDAT")) {
      if ((rc = mmt::check_crc(c))) return rc;
    } else if (mmt::is_type(c.type, "tRNS")) {
      return mmt::fail(MMT_E_UNSUPPORTED, "png: a tRNS chunk (transparency) is not supported");
    } else if (!(c.type[0] & 0x20) && !mmt::is_type(c.type, "PLTE")) {
      return mmt::fail(MMT_E_UNSUPPORTED, "png: unknown critical chunk 0x%02x%02x%02x%02x", c.type[0], c.type[1], c.type[2], c.type[3]);
    }
    next += 12 + c.size;
  }
}

// The host stage of the device inflate (png_inflate.hip): the chunk walk of mmt_png_inflate without its DEFLATE -- the
// same rules in the same order, the same messages -- with the IDAT payloads copied back to back.
int mmt_png_gather(const uint8_t* bytes, int64_t len, const mmt_png_image* image, uint8_t* comp_out, int64_t comp_capacity,
                   mmt_png_stream* stream, uint8_t* palette_out) {
  int rc = mmt::check_bytes("mmt_png_gather", bytes, len);
  if (rc) return rc;
  if (!image || !comp_out || !stream || !palette_out)
    return mmt::fail(MMT_E_INVALID, "mmt_png_gather: NULL argument (image, comp_out, stream and palette_out are required)");
  mmt::Header h;
  if ((rc = mmt::read_header(bytes, len, h))) return rc;
  const mmt_png_image& own = h.im;
  if (image->width != own.width || image->height != own.height || image->bit_depth != own.bit_depth || image->color_type != own.color_type ||
      image->interlace != own.interlace || image->palette_entries != own.palette_entries || image->raw_bytes != own.raw_bytes)
    return mmt::fail(MMT_E_INVALID, "mmt_png_gather: image does not describe this stream (take it from mmt_png_info)");
  if (stream->comp_offset < 0 || stream->comp_offset > comp_capacity)
    return mmt::fail(MMT_E_INVALID, "mmt_png_gather: comp_offset %lld outside comp_out (%lld bytes)", (long long)stream->comp_offset,
                     (long long)comp_capacity);
  std::memset(palette_out, 0, 768);
  if (h.plte) std::memcpy(palette_out, h.plte, (size_t)own.palette_entries * 3);
  uint8_t* comp = comp_out + stream->comp_offset;
  const int64_t room = comp_capacity - stream->comp_offset;
  int64_t n = 0, next = h.first_idat;
  int err = 0;
  while (next != len) {                                         // the IDAT chunks that follow each other directly
    mmt::Chunk c;
    if ((err = mmt::read_chunk(bytes, len, next, c))) break;
    if (!mmt::is_type(c.type, "IDAT")) break;
    if ((err = mmt::check_crc(c))) break;
    if (c.size > room - n)
      return mmt::fail(MMT_E_INVALID, "mmt_png_gather: the IDAT payloads leave comp_out (%lld bytes from %lld)", (long long)comp_capacity,
                       (long long)stream->comp_offset);
    std::memcpy(comp + n, c.data, (size_t)c.size);
    n += c.size; next += 12 + c.size;
  }
  if (n < 2) return err ? err : mmt::truncated_stream();
  const unsigned cmf = comp[0], flg = comp[1];
  if ((cmf & 15u) != 8) return mmt::fail(MMT_E_INVALID, "png: bad zlib header: compression method %u is not 8 (deflate)", cmf & 15u);
  if ((cmf >> 4) > 7) return mmt::fail(MMT_E_INVALID, "png: bad zlib header: a window larger than 32 KiB");
  if (((cmf << 8) | flg) % 31 != 0) return mmt::fail(MMT_E_INVALID, "png: bad zlib header: the check bits do not match");
  if (flg & 0x20) return mmt::fail(MMT_E_INVALID, "png: bad zlib header: a preset dictionary");
  if (err) return err;
  stream->comp_bytes = n;
  for (;;) {                                                    // behind the stream, as mmt_png_inflate walks on
    mmt::Chunk c;
    if (next == len) return mmt::fail(MMT_E_INVALID, "png: truncated: the file ends without an IEND chunk");
    if ((rc = mmt::read_chunk(bytes, len, next, c))) return rc;
    if (mmt::is_type(c.type, "IEND")) return mmt::check_crc(c);
    if (mmt::is_type(c.type, "IDAT")) {
      if ((rc = mmt::check_crc(c))) return rc;
    } else if (mmt::is_type(c.type, "tRNS")) {
      return mmt::fail(MMT_E_UNSUPPORTED, "png: a tRNS chunk (transparency) is not supported");
    } else if (!(c.type[0] & 0x20) && !mmt::is_type(c.type, "PLTE")) {
      return mmt::fail(MMT_E_UNSUPPORTED, "png: unknown critical chunk 0x%02x%02x%02x%02x", c.type[0], c.type[1], c.type[2], c.type[3]);
    }
    next += 12 + c.size;
  }
}

size_t mmt_png_workspace_bytes(int64_t raw_bytes) { return raw_bytes < 1 ? 0 : (size_t)raw_bytes; }

int mmt_png_pixels_host(int32_t B, const mmt_png_image* images, const uint8_t* raw, int64_t raw_bytes, const uint8_t* palettes,
                        uint8_t* pixels_out, int64_t pixels_bytes, void* workspace, size_t workspace_bytes) {
  const int rc = mmt::check_stage2("mmt_png_pixels_host", B, images, raw, raw_bytes, palettes, pixels_out, pixels_bytes, workspace, workspace_bytes);
  if (rc) return rc;
  mmt::PngParams p;
  p.B = B; p.images = images; p.raw = raw; p.raw_bytes = raw_bytes; p.palettes = palettes; p.pixels = pixels_out;
  p.pixels_bytes = pixels_bytes; p.keep = (unsigned char*)workspace;
  for (int b = 0; b < B; ++b) {
    const mmt::PngGeom g = mmt::png_geom(images[b], raw_bytes, pixels_bytes);
    unsigned pal[256];
    mmt::pack_palette(palettes + (size_t)b * 768, pal);
    for (int pass = 0; pass < g.passes; ++pass) {
      const mmt::PngPass s = mmt::png_pass(g, pass);
      if (s.rows == 0) continue;
      if (g.bpp == 3) mmt::png_pass_host<3>(p, g, s, pal);
      else mmt::png_pass_host<1>(p, g, s, pal);
    }
  }
  return MMT_OK;
}

#ifndef MMT_PNG_HOST_ONLY
int mmt_png_pixels(int32_t B, const mmt_png_image* images, const uint8_t* raw, int64_t raw_bytes, const uint8_t* palettes,
                   uint8_t* pixels_out, int64_t pixels_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = mmt::check_stage2("mmt_png_pixels", B, images, raw, raw_bytes, palettes, pixels_out, pixels_bytes, workspace, workspace_bytes);
  if (rc) return rc;
  mmt::PngParams p;
  p.B = B; p.images = images; p.raw = raw; p.raw_bytes = raw_bytes; p.palettes = palettes; p.pixels = pixels_out;
  p.pixels_bytes = pixels_bytes; p.keep = (unsigned char*)workspace;
  const hipError_t e = mmt::launch_png_pixels(p, (hipStream_t)stream);
  return e == hipSuccess ? MMT_OK : mmt::fail(MMT_E_LAUNCH, "mmt_png_pixels: %s", hipGetErrorString(e));
}
#endif

}  // extern "C"
