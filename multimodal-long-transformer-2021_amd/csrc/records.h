// CRC-32C over record payloads by pieces (records.hip; DESIGN.md section 4, "Records"): the tables, the register of one
// piece, the shifts that join pieces, and a record's clamped place in the blob, shared by the kernels and the host
// loops through __host__ __device__ functions.
//
// The register is the reflected one: bit 31 is x^0.  raw(m) is the register after m from 0 without the final xor;
// shift(c, k) = c * x^(8k) mod P is the register pushed through k zero bytes.  raw(a||b) = shift(raw(a), |b|) ^ raw(b)
// and crc(m) = raw(m) ^ shift(0xFFFFFFFF, |m|) ^ 0xFFFFFFFF; zero bytes in FRONT of m leave raw(m) as it is, which is
// why a payload is cut into pieces from its end: every piece but the first is whole, so inside a workgroup every join
// shifts by a whole number of pieces.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mmt_layer.h"

namespace mmt {

constexpr int kRecThreads = 256;                       // lanes of a workgroup = pieces of a part
constexpr int kRecPiece = MMT_RECORDS_PIECE;           // bytes of a piece: a lane's share
constexpr int kRecPieceLog = 7;
constexpr int kRecLevels = 8;                          // log2(kRecThreads): levels of the in-workgroup scan
constexpr uint32_t kCrc32cPoly = 0x82F63B78u;
static_assert((1 << kRecPieceLog) == kRecPiece && (1 << kRecLevels) == kRecThreads, "piece and part are powers of two");
static_assert(MMT_RECORDS_PART == kRecThreads * kRecPiece, "a part is one piece per lane");

// a * b mod P on reflected registers, 32 steps, no branch
__host__ __device__ constexpr uint32_t rec_gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 31; i >= 0; --i) {
    p ^= (0u - ((a >> i) & 1u)) & b;
    b = (b >> 1) ^ ((0u - (b & 1u)) & kCrc32cPoly);
  }
  return p;
}

struct RecTables {
  uint32_t slice[4][256];              // slice[k][v]: the register of byte v followed by k zero bytes
  uint32_t level[kRecLevels][32];      // level[j][i] = (1 << i) * x^(8 * PIECE * 2^j): the shift by 2^j pieces as a bit matrix
  uint32_t xpow[64];                   // xpow[j] = x^(8 * 2^j): the shift by 2^j bytes
};

constexpr RecTables rec_make_tables() {
  RecTables t{};
  for (uint32_t v = 0; v < 256; ++v) {
    uint32_t c = v;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((0u - (c & 1u)) & kCrc32cPoly);
    t.slice[0][v] = c;
  }
  for (int k = 1; k < 4; ++k)
    for (int v = 0; v < 256; ++v) t.slice[k][v] = (t.slice[k - 1][v] >> 8) ^ t.slice[0][t.slice[k - 1][v] & 0xFFu];
  uint32_t p = 0x00800000u;            // x^8
  for (int j = 0; j < 64; ++j) {
    t.xpow[j] = p;
    p = rec_gf_mul(p, p);
  }
  for (int j = 0; j < kRecLevels; ++j)
    for (int i = 0; i < 32; ++i) t.level[j][i] = rec_gf_mul(1u << i, t.xpow[kRecPieceLog + j]);
  return t;
}

// c * K for the K whose bit matrix is m (RecTables::level[j])
__host__ __device__ inline uint32_t rec_shift_level(const uint32_t* m, uint32_t c) {
  uint32_t r = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i) r ^= (0u - ((c >> i) & 1u)) & m[i];
  return r;
}

// shift(c, nbytes) for any count: one multiply per set bit of nbytes
__host__ __device__ inline uint32_t rec_shift_bytes(const uint32_t* xpow, uint32_t c, uint64_t nbytes) {
  for (int j = 0; nbytes != 0 && j < 64; ++j, nbytes >>= 1)
    if (nbytes & 1u) c = rec_gf_mul(c, xpow[j]);
  return c;
}

__host__ __device__ inline uint32_t rec_word(const uint32_t* slice, uint32_t c, uint32_t w) {
  c ^= w;
  return slice[768 + (c & 0xFFu)] ^ slice[512 + ((c >> 8) & 0xFFu)] ^ slice[256 + ((c >> 16) & 0xFFu)] ^ slice[c >> 24];
}

// raw(p[0 .. n)): bytes up to the first 4-byte aligned address, then 16-byte loads where the address is 16-byte aligned
// and 4-byte loads elsewhere, then the rest by bytes.  Every load lies inside [p, p + n).  slice: RecTables::slice, flat.
__host__ __device__ inline uint32_t rec_raw(const uint32_t* slice, const unsigned char* p, long n) {
  uint32_t c = 0;
  while (n > 0 && ((uintptr_t)p & 3u) != 0) {
    c = slice[(c ^ *p) & 0xFFu] ^ (c >> 8);
    ++p; --n;
  }
  while (n >= 4) {
    if (n >= 16 && ((uintptr_t)p & 15u) == 0) {
      uint32_t w[4];
      __builtin_memcpy(w, __builtin_assume_aligned(p, 16), 16);
      c = rec_word(slice, rec_word(slice, rec_word(slice, rec_word(slice, c, w[0]), w[1]), w[2]), w[3]);
      p += 16; n -= 16;
    } else {
      uint32_t w;
      __builtin_memcpy(&w, __builtin_assume_aligned(p, 4), 4);
      c = rec_word(slice, c, w);
      p += 4; n -= 4;
    }
  }
  while (n > 0) {
    c = slice[(c ^ *p) & 0xFFu] ^ (c >> 8);
    ++p; --n;
  }
  return c;
}

__host__ __device__ inline uint32_t rec_mask(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

struct RecPlace {                      // a record's payload clamped into the blob
  long off, len, pieces;
};
__host__ __device__ inline RecPlace rec_place(const mmt_record& r, long bytes_len) {
  RecPlace q;
  q.off = r.offset < 0 ? 0 : (r.offset > bytes_len ? bytes_len : r.offset);
  const long room = bytes_len - q.off;
  q.len = r.length < 0 ? 0 : (r.length > room ? room : r.length);
  q.pieces = (q.len + kRecPiece - 1) >> kRecPieceLog;
  return q;
}
// Piece k of q.pieces, counted from the front, cut from the end: bytes [begin, end) of the payload
__host__ __device__ inline void rec_piece(const RecPlace& q, long k, long& begin, long& end) {
  end = q.len - ((q.pieces - 1 - k) << kRecPieceLog);
  begin = end - kRecPiece < 0 ? 0 : end - kRecPiece;
}

}  // namespace mmt
