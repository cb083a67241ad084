// Launch parameters and table formats of the text front end (text_tokens.hip), shared with the host-only stand-in of
// the sanitizer build (asan/asan_stubs.cpp).  The formats are documented in include/mmt_layer.h.
#pragma once
#include <hip/hip_runtime.h>

namespace mmt {

constexpr int kTextMaxFields = 16;                   // field tokens travel in the kernel arguments
constexpr int kTextMaxWordChars = 100;               // a longer word is [UNK] (max_input_chars_per_word)
constexpr int kTextChunk = 256;                      // bytes of a field one staging step takes (one per thread)
constexpr int kTextKeep = kTextMaxWordChars + 1;     // characters of an unfinished word carried to the next chunk
constexpr unsigned kTextFirst = 0x80000000u;         // piece record: first piece of its word

constexpr unsigned kCodepoints = 0x110000u;          // entries of the code-point table in front of its side table
constexpr unsigned kCpValue = 0x1fffffu;             // entry: mapped character, or index into the side table
constexpr int kCpSoloBit = 21;                       // entry: the character is a word of its own (punctuation, CJK)
constexpr int kCpCountShift = 22;                    // entry: mapped characters, 0..3
constexpr int kCpSpaceBit = 24;                      // entry: the source character separates words

constexpr unsigned kVocabMagic = 0x5650574du;        // "MWPV"
constexpr int kVocabHeaderWords = 8;                 // magic, tokens, slots, first byte word, token bytes, 3 x reserved
constexpr unsigned kVocabMul = 0x01000193u;          // hash of a piece: sum of character[t] * kVocabMul^t mod 2^32
constexpr unsigned kVocabCont = 0x9e3779b9u;         // xor-ed into the hash of a `##` piece

__host__ __device__ inline unsigned vocab_mix(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

// Length (1..4) of the well-formed UTF-8 sequence (Unicode Table 3-7) that starts with b0, given `avail` bytes from
// there on (b1..b3 are read only as far as avail allows), and its code point; 0 when none starts here.
__host__ __device__ inline int utf8_decode(unsigned b0, unsigned b1, unsigned b2, unsigned b3, long avail, unsigned* c) {
  if (avail < 1) return 0;
  if (b0 < 0x80u) { *c = b0; return 1; }
  if (b0 < 0xc2u || b0 > 0xf4u) return 0;
  const bool t1 = avail > 1 && (b1 & 0xc0u) == 0x80u, t2 = avail > 2 && (b2 & 0xc0u) == 0x80u, t3 = avail > 3 && (b3 & 0xc0u) == 0x80u;
  if (b0 < 0xe0u) {
    if (!t1) return 0;
    *c = ((b0 & 0x1fu) << 6) | (b1 & 0x3fu);
    return 2;
  }
  if (b0 < 0xf0u) {
    if (!t1 || !t2 || (b0 == 0xe0u && b1 < 0xa0u) || (b0 == 0xedu && b1 > 0x9fu)) return 0;
    *c = ((b0 & 0x0fu) << 12) | ((b1 & 0x3fu) << 6) | (b2 & 0x3fu);
    return 3;
  }
  if (!t1 || !t2 || !t3 || (b0 == 0xf0u && b1 < 0x90u) || (b0 == 0xf4u && b1 > 0x8fu)) return 0;
  *c = ((b0 & 0x07u) << 18) | ((b1 & 0x3fu) << 12) | ((b2 & 0x3fu) << 6) | (b3 & 0x3fu);
  return 4;
}

struct TextParams {
  int B, F, T, budget;
  const unsigned char* bytes;
  long nbytes;
  const long* offsets;       // [B * F]
  const int* lengths;        // [B * F]
  const unsigned* vocab;     // the vocabulary image
  unsigned vocab_words;      // its size in 32-bit words
  const unsigned* cp;        // code-point table and side table
  unsigned cp_entries;
  int field_tok[kTextMaxFields];
  int sep, unk;
  int* ids;                  // [B, T]
  int* count;                // [B]
  unsigned char* wstart;     // [B, T]
  unsigned* pieces;          // workspace: [B * F, budget] piece records (id | kTextFirst)
  int* npieces;              // workspace: [B * F] pieces a field produced, at most budget
};

// The tokenise pass (one workgroup per field) and the row assembly (one per example), both on `st`.
hipError_t launch_text_tokens(const TextParams& p, hipStream_t st);

}  // namespace mmt
