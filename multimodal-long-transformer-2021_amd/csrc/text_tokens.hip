// Text front end on the device (C ABI: include/mmt_layer.h, mmt_text_tokens): the text half of the reference's
// `decode_fn` (src/data/data_utils.py:241-278) -- BERT tokenisation of each UTF-8 field, the round-robin trim to the
// text budget, field tokens and [SEP], padding, and the word starts whole-word masking reads.  The definition is
// DESIGN.md section 4, "Text front end"; the table formats are in include/mmt_layer.h.
//
// Two kernels:
//   1. tokenise: one workgroup of four waves per (example, field).  The field's bytes are taken in chunks of
//      kTextChunk, one byte per thread: a thread whose byte starts a well-formed UTF-8 sequence looks its code point up
//      in the code-point table and has 0..3 mapped characters.  Two scans over the workgroup -- "was there a break since
//      the last character" (a last-writer scan on ballots) and the counts of characters and word starts -- place the
//      characters and the word boundaries in LDS behind the unfinished word the previous chunk left (at most
//      kTextKeep characters of it are kept: a word that long is [UNK] whatever follows).  Then the finished words are
//      matched, a wave per word: the wave holds the word's prefix hashes S[k] = sum_{t<k} c[t] M^t in registers, so a
//      candidate [s, e) hashes to (S[e] - S[s]) M^-s in O(1); the 64 lanes test the 64 longest ends at once (two sweeps
//      for words over 64 characters), every hash hit is confirmed byte by byte against the vocabulary, and a ballot
//      picks the longest.  A start without a match withdraws the word's pieces: it becomes one [UNK].  Piece counts of
//      the four waves are summed in word order, so a field's pieces land in order; the field stops once it has
//      `budget` pieces, however many bytes are left.
//   2. assemble: one workgroup per example.  The shares a_f of the round-robin trim follow from the piece counts in
//      closed form (the largest level R with sum min(n_f, R) <= budget, then one more for the first fields that have
//      one, while budget remains); every element of the row, padding included, is written once.
// No atomics, no order that depends on timing: the same bytes give the same ids.
//
// Bounds: a field's offset is clamped into [0, bytes_len] and its length into what is left; table indices are clamped
// into the tables' sizes, a probe chain ends after `slots` steps.  Wrong metadata or a wrong table gives wrong ids,
// never a stray access; writes go to [B, T] and [B] only.
#include "../../include/mmt_attn.h"
#include "../../include/mmt_layer.h"

#include <cstdint>
#include <cstring>

#include "mmt_err.h"
#include "text_tokens.h"

#ifndef MMT_TEXT_TOKENS_HOST_ONLY
namespace mmt {
namespace {

constexpr int kWaves = kTextChunk / 64;
constexpr int kBufChars = kTextKeep + 3 * kTextChunk;

__device__ __forceinline__ int utf8_encode(unsigned c, unsigned char* o) {
  if (c < 0x80u) { o[0] = (unsigned char)c; return 1; }
  if (c < 0x800u) { o[0] = (unsigned char)(0xc0u | (c >> 6)); o[1] = (unsigned char)(0x80u | (c & 0x3fu)); return 2; }
  if (c < 0x10000u) {
    o[0] = (unsigned char)(0xe0u | (c >> 12)); o[1] = (unsigned char)(0x80u | ((c >> 6) & 0x3fu)); o[2] = (unsigned char)(0x80u | (c & 0x3fu));
    return 3;
  }
  o[0] = (unsigned char)(0xf0u | (c >> 18)); o[1] = (unsigned char)(0x80u | ((c >> 12) & 0x3fu));
  o[2] = (unsigned char)(0x80u | ((c >> 6) & 0x3fu)); o[3] = (unsigned char)(0x80u | (c & 0x3fu));
  return 4;
}

struct Vocab {
  const unsigned* slots;
  const unsigned char* image;   // the whole image as bytes
  unsigned nslots;              // power of two inside the image; 0: nothing matches
  unsigned long first_byte, last_byte;
};

__device__ __forceinline__ Vocab open_vocab(const TextParams& p) {
  Vocab v;
  v.slots = p.vocab + kVocabHeaderWords;
  v.image = reinterpret_cast<const unsigned char*>(p.vocab);
  const unsigned room = (p.vocab_words - kVocabHeaderWords) / 4u;
  unsigned n = p.vocab[0] == kVocabMagic ? min(p.vocab[2], room) : 0u;
  while (n & (n - 1u)) n &= n - 1u;               // the largest power of two inside the image
  v.nslots = n;
  v.last_byte = (unsigned long)p.vocab_words * 4ul - 1ul;
  v.first_byte = min((unsigned long)p.vocab[3] * 4ul, v.last_byte);
  return v;
}

// Id of the piece w[s, e) (a `##` piece when cont), or -1.  `key` is its hash.
__device__ int lookup(const Vocab& v, const unsigned* w, int s, int e, bool cont, unsigned key) {
  if (v.nslots == 0u) return -1;
  const unsigned mask = v.nslots - 1u;
  unsigned slot = vocab_mix(key) & mask;
  for (unsigned probe = 0; probe < v.nslots; ++probe, slot = (slot + 1u) & mask) {
    const unsigned* q = v.slots + (size_t)slot * 4u;
    const unsigned idp = q[0];
    if (idp == 0u) return -1;
    if (q[1] != key || (q[3] >> 31) != (cont ? 1u : 0u)) continue;
    const unsigned len = q[3] & 0x7fffffffu;
    const unsigned long at = v.first_byte + q[2];
    unsigned pos = 0;
    bool same = true;
    for (int k = s; k < e && same; ++k) {
      unsigned char enc[4];
      const int nb = utf8_encode(w[k] & kCpValue, enc);
      if (pos + (unsigned)nb > len) { same = false; break; }
      for (int j = 0; j < nb; ++j) same = same && v.image[min(at + pos + (unsigned)j, v.last_byte)] == enc[j];
      pos += (unsigned)nb;
    }
    if (same && pos == len) return (int)((idp - 1u) & 0x7fffffffu);
  }
  return -1;
}

// One word, by one wave (all 64 lanes arrive together): its piece records into out[0 .. return).
__device__ int match_word(const TextParams& p, const Vocab& v, const unsigned* w, int n, const unsigned* pw, const unsigned* ipw,
                          unsigned* out) {
  const int lane = threadIdx.x & 63;
  if (n > kTextMaxWordChars) {
    if (lane == 0) out[0] = (unsigned)p.unk | kTextFirst;
    return 1;
  }
  // prefix hashes: lane l holds S[l + 1] and S[l + 65]
  unsigned S[2] = {0u, 0u}, carry = 0u;
  for (int sweep = 0; sweep < 2; ++sweep) {
    const int k = sweep * 64 + lane;
    unsigned x = k < n ? (w[k] & kCpValue) * pw[k] : 0u;
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    S[sweep] = carry + x;
    carry += __shfl(x, 63);
  }
  auto prefix = [&](int i) -> unsigned {              // S[i], i in [0, 100]; every lane calls it
    const int j = max(i - 1, 0);
    const unsigned lo = __shfl(S[0], j & 63), hi = __shfl(S[1], j & 63);
    return i <= 0 ? 0u : (j < 64 ? lo : hi);
  };
  int s = 0, cnt = 0;
  while (s < n) {
    const unsigned Ss = prefix(s);
    int hit_end = -1, hit_id = -1;
    for (int top = n; top > s; top -= 64) {           // ends top, top - 1, ..: the longest first
      const int e = top - lane;
      const unsigned Se = prefix(min(max(e, 0), n));
      int id = -1;
      if (e > s) {
        const unsigned key = ((Se - Ss) * ipw[s]) ^ (s > 0 ? kVocabCont : 0u);
        id = lookup(v, w, s, e, s > 0, key);
      }
      const unsigned long long hits = __ballot(id >= 0);
      if (hits) {
        const int first = __ffsll((long long)hits) - 1;
        hit_end = top - first;
        hit_id = __shfl(id, first);
        break;
      }
    }
    if (hit_end < 0) {                                 // no piece starts here: the pieces so far are withdrawn
      if (lane == 0) out[0] = (unsigned)p.unk | kTextFirst;
      return 1;
    }
    if (lane == 0) out[cnt] = (unsigned)hit_id | (cnt == 0 ? kTextFirst : 0u);
    ++cnt;
    s = hit_end;
  }
  return cnt;
}

__global__ __launch_bounds__(kTextChunk) void text_tokenise_kernel(const TextParams p) {
  const int bf = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ unsigned cbuf[kBufChars];                 // characters of the chunk behind the carried word; bit 31: starts a word
  __shared__ int wst[kBufChars + 1];                   // first character of each word, and the end behind the last
  __shared__ unsigned pw[kTextKeep], ipw[kTextKeep];   // M^t and M^-t
  __shared__ unsigned pout[kWaves][kTextMaxWordChars];
  __shared__ int wcnt[kWaves];
  __shared__ int wave_op[kWaves], wave_sum[kWaves];

  if (tid < kTextKeep) {
    unsigned inv = kVocabMul;                          // Newton: the inverse of an odd number mod 2^32
    for (int i = 0; i < 5; ++i) inv *= 2u - kVocabMul * inv;
    unsigned a = 1u, b = 1u;
    for (int i = 0; i < tid; ++i) { a *= kVocabMul; b *= inv; }
    pw[tid] = a; ipw[tid] = b;
  }
  const Vocab v = open_vocab(p);
  const long base = min(max(p.offsets[bf], 0L), p.nbytes);
  const long len = min((long)max(p.lengths[bf], 0), p.nbytes - base);
  const unsigned char* src = p.bytes + base;
  unsigned* dst = p.pieces + (size_t)bf * (size_t)p.budget;
  const unsigned cp_last = p.cp_entries - 1u;

  int carried = 0;       // characters of the unfinished word at the front of cbuf
  int brk = 1;           // a space since the last character, or that character was a word of its own, or there was none
  int total = 0;         // pieces so far
  __syncthreads();
  for (long cs = 0; total < p.budget; cs += kTextChunk) {
    const bool final_chunk = cs + kTextChunk >= len;
    // ---- this thread's byte: 0..3 mapped characters, or a space, or nothing
    unsigned ch[3] = {0u, 0u, 0u};
    int solo[3] = {0, 0, 0};
    int ne = 0, op = 0;                                // op: 0 leaves the break state, 1 clears it, 2 sets it
    const long at = cs + tid;
    if (at < len) {
      const long avail = len - at;
      const unsigned b0 = src[at], b1 = avail > 1 ? src[at + 1] : 0u, b2 = avail > 2 ? src[at + 2] : 0u, b3 = avail > 3 ? src[at + 3] : 0u;
      unsigned c = 0u;
      if (utf8_decode(b0, b1, b2, b3, avail, &c) > 0) {
        const unsigned e = p.cp[min(c, cp_last)];
        ne = (int)((e >> kCpCountShift) & 3u);
        if (ne == 1) {
          ch[0] = e & kCpValue; solo[0] = (int)((e >> kCpSoloBit) & 1u);
        } else {
          for (int j = 0; j < ne; ++j) {
            const unsigned se = p.cp[min(kCodepoints + (e & kCpValue) + (unsigned)j, cp_last)];
            ch[j] = se & kCpValue; solo[j] = (int)((se >> kCpSoloBit) & 1u);
          }
        }
        if (ne > 0) op = solo[ne - 1] ? 2 : 1;
        else if ((e >> kCpSpaceBit) & 1u) op = 2;
      }
    }
    // ---- break state in front of each thread: the last writer below it
    const unsigned long long wrote = __ballot(op != 0), set = __ballot(op == 2);
    if (lane == 0) wave_op[wave] = wrote ? ((set >> (63 - __clzll((long long)wrote))) & 1ull ? 2 : 1) : 0;
    __syncthreads();
    int before = brk;
    for (int k = 0; k < wave; ++k)
      if (wave_op[k]) before = wave_op[k] == 2;
    const unsigned long long below = wrote & ((1ull << lane) - 1ull);
    if (below) before = (int)((set >> (63 - __clzll((long long)below))) & 1ull);
    for (int k = 0; k < kWaves; ++k)
      if (wave_op[k]) brk = wave_op[k] == 2;
    // ---- characters and word starts in front of each thread
    int st[3];
    st[0] = ne > 0 && (before || solo[0]);
    st[1] = ne > 1 && (solo[0] || solo[1]);
    st[2] = ne > 2 && (solo[1] || solo[2]);
    int x = ne | ((st[0] + st[1] + st[2]) << 16);
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    if (lane == 63) wave_sum[wave] = x;
    __syncthreads();
    int excl = x - (ne | ((st[0] + st[1] + st[2]) << 16)), all = 0;
    for (int k = 0; k < kWaves; ++k) {
      if (k < wave) excl += wave_sum[k];
      all += wave_sum[k];
    }
    const int first_word = carried > 0 ? 1 : 0;
    int pos = carried + (excl & 0xffff), word = first_word + (excl >> 16);
    for (int j = 0; j < ne; ++j, ++pos) {
      cbuf[pos] = ch[j] | (st[j] ? kTextFirst : 0u);
      if (st[j]) wst[word++] = pos;
    }
    const int nchar = carried + (all & 0xffff), nword = first_word + (all >> 16);
    if (tid == 0) {
      wst[nword] = nchar;
      if (carried > 0) wst[0] = 0;
    }
    __syncthreads();
    // ---- the finished words, four at a time in word order
    const int ready = final_chunk ? nword : max(nword - 1, 0);
    for (int r = 0; r < ready && total < p.budget; r += kWaves) {
      const int k = r + wave;
      int cnt = 0;
      if (k < ready) cnt = match_word(p, v, cbuf + wst[k], wst[k + 1] - wst[k], pw, ipw, pout[wave]);
      if (lane == 0) wcnt[wave] = cnt;
      __syncthreads();
      int off = total;
      for (int j = 0; j < kWaves; ++j) {
        if (j < wave) off += wcnt[j];
        total += wcnt[j];
      }
      for (int i = lane; i < cnt; i += 64)
        if (off + i < p.budget) dst[off + i] = pout[wave][i];
      __syncthreads();
    }
    if (final_chunk) break;
    // ---- the unfinished word moves to the front
    int keep = 0;
    unsigned moved = 0u;
    if (nword > 0) {
      const int from = wst[nword - 1];
      keep = min(nchar - from, kTextKeep);
      if (tid < keep) moved = cbuf[from + tid];
    }
    __syncthreads();
    if (tid < keep) cbuf[tid] = moved;
    carried = keep;
    __syncthreads();
  }
  if (tid == 0) p.npieces[bf] = min(total, p.budget);
}

__global__ __launch_bounds__(256) void text_assemble_kernel(const TextParams p) {
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ int start[kTextMaxFields + 1];            // row position of each field token, then of [SEP]
  if (tid == 0) {
    int n[kTextMaxFields];
    for (int f = 0; f < p.F; ++f) n[f] = min(max(p.npieces[(size_t)b * p.F + f], 0), p.budget);
    int lo = 0, hi = p.budget;                         // the largest level R with sum min(n_f, R) <= budget
    while (lo < hi) {
      const int mid = (lo + hi + 1) / 2;
      long sum = 0;
      for (int f = 0; f < p.F; ++f) sum += min(n[f], mid);
      if (sum <= p.budget) lo = mid; else hi = mid - 1;
    }
    int rem = p.budget;
    for (int f = 0; f < p.F; ++f) rem -= min(n[f], lo);
    int at = 0;
    for (int f = 0; f < p.F; ++f) {
      int a = min(n[f], lo);
      if (n[f] > lo && rem > 0) { ++a; --rem; }
      start[f] = at;
      at += 1 + a;
    }
    start[p.F] = at;
    p.count[b] = at + 1;
  }
  __syncthreads();
  const int sep_at = start[p.F];
  for (int t = tid; t < p.T; t += 256) {
    int id = 0, first = 0;
    if (t == sep_at) {
      id = p.sep; first = 1;
    } else if (t < sep_at) {
      int f = 0;
      while (f + 1 < p.F && start[f + 1] <= t) ++f;
      if (t == start[f]) {
        id = p.field_tok[f]; first = 1;
      } else {
        const unsigned rec = p.pieces[((size_t)b * p.F + f) * (size_t)p.budget + (size_t)(t - start[f] - 1)];
        id = (int)(rec & ~kTextFirst); first = (int)(rec >> 31);
      }
    }
    p.ids[(size_t)b * p.T + t] = id;
    p.wstart[(size_t)b * p.T + t] = (unsigned char)first;
  }
}

}  // namespace

hipError_t launch_text_tokens(const TextParams& p, hipStream_t st) {
  hipLaunchKernelGGL(text_tokenise_kernel, dim3((unsigned)(p.B * p.F)), dim3(kTextChunk), 0, st, p);
  hipLaunchKernelGGL(text_assemble_kernel, dim3((unsigned)p.B), dim3(256), 0, st, p);
  return hipGetLastError();
}

}  // namespace mmt
#endif  // MMT_TEXT_TOKENS_HOST_ONLY

namespace {

unsigned next_pow2(unsigned long long x) {
  unsigned n = 2u;
  while (n < x) n <<= 1;
  return n;
}

bool is_cont(const uint8_t* t, int64_t len) { return len > 2 && t[0] == '#' && t[1] == '#'; }

}  // namespace

extern "C" {

size_t mmt_wordpiece_vocab_bytes(int64_t n_tokens, int64_t token_bytes) {
  if (n_tokens < 1 || n_tokens > ((int64_t)1 << 28) || token_bytes < n_tokens || token_bytes > ((int64_t)1 << 30)) return 0;
  const size_t slots = next_pow2(2ull * (unsigned long long)n_tokens);
  return (size_t)mmt::kVocabHeaderWords * 4 + slots * 16 + (((size_t)token_bytes + 3) & ~(size_t)3);
}

int mmt_wordpiece_vocab_build(int64_t n_tokens, const uint8_t* token_bytes, const int64_t* token_offsets, void* image,
                              size_t image_bytes) {
  if (!token_bytes || !token_offsets || !image)
    return mmt::fail(MMT_E_INVALID, "mmt_wordpiece_vocab_build: NULL argument (token_bytes, token_offsets and image are required)");
  if (n_tokens < 1 || n_tokens > ((int64_t)1 << 28))
    return mmt::fail(MMT_E_INVALID, "mmt_wordpiece_vocab_build: n_tokens (%lld) outside [1, 2^28]", (long long)n_tokens);
  if (token_offsets[0] != 0) return mmt::fail(MMT_E_INVALID, "mmt_wordpiece_vocab_build: token_offsets[0] must be 0");
  for (int64_t i = 0; i < n_tokens; ++i) {
    if (token_offsets[i + 1] < token_offsets[i])
      return mmt::fail(MMT_E_INVALID, "mmt_wordpiece_vocab_build: token_offsets decrease at token %lld", (long long)i);
    if (token_offsets[i + 1] == token_offsets[i])
      return mmt::fail(MMT_E_INVALID, "mmt_wordpiece_vocab_build: token %lld is empty", (long long)i);
  }
  const int64_t total = token_offsets[n_tokens];
  const size_t need = mmt_wordpiece_vocab_bytes(n_tokens, total);
  if (need == 0) return mmt::fail(MMT_E_INVALID, "mmt_wordpiece_vocab_build: %lld token bytes outside [n_tokens, 2^30]", (long long)total);
  if (image_bytes < need)
    return mmt::fail(MMT_E_WORKSPACE, "mmt_wordpiece_vocab_build: image of %zu bytes needed, %zu given", need, image_bytes);
  if (((uintptr_t)image & 3) != 0) return mmt::fail(MMT_E_INVALID, "mmt_wordpiece_vocab_build: image must be 4-byte aligned");
  std::memset(image, 0, need);
  uint32_t* words = (uint32_t*)image;
  const uint32_t nslots = next_pow2(2ull * (unsigned long long)n_tokens), mask = nslots - 1u;
  const uint32_t first_word = (uint32_t)mmt::kVocabHeaderWords + 4u * nslots;
  words[0] = mmt::kVocabMagic; words[1] = (uint32_t)n_tokens; words[2] = nslots; words[3] = first_word;
  uint32_t* slots = words + mmt::kVocabHeaderWords;
  uint8_t* store = (uint8_t*)(words + first_word);
  uint32_t used = 0;
  for (int64_t i = 0; i < n_tokens; ++i) {
    const uint8_t* t = token_bytes + token_offsets[i];
    int64_t len = token_offsets[i + 1] - token_offsets[i];
    const bool cont = is_cont(t, len);
    if (cont) { t += 2; len -= 2; }
    uint32_t h = 0u, m = 1u;
    for (int64_t at = 0; at < len;) {
      const int64_t avail = len - at;
      unsigned c = 0u;
      const int nb = mmt::utf8_decode(t[at], avail > 1 ? t[at + 1] : 0u, avail > 2 ? t[at + 2] : 0u, avail > 3 ? t[at + 3] : 0u, (long)avail, &c);
      if (nb == 0) return mmt::fail(MMT_E_INVALID, "mmt_wordpiece_vocab_build: token %lld is not well-formed UTF-8", (long long)i);
      h += c * m; m *= mmt::kVocabMul;
      at += nb;
    }
    const uint32_t key = h ^ (cont ? mmt::kVocabCont : 0u), tag = (uint32_t)len | (cont ? 0x80000000u : 0u);
    uint32_t slot = mmt::vocab_mix(key) & mask;
    while (slots[4 * slot] != 0u) {
      const uint32_t* q = slots + 4 * slot;
      if (q[1] == key && q[3] == tag && std::memcmp(store + q[2], t, (size_t)len) == 0)
        return mmt::fail(MMT_E_INVALID, "mmt_wordpiece_vocab_build: token %lld duplicates token %lld", (long long)i, (long long)q[0] - 1);
      slot = (slot + 1u) & mask;
    }
    uint32_t* q = slots + 4 * slot;
    q[0] = (uint32_t)i + 1u; q[1] = key; q[2] = used; q[3] = tag;
    std::memcpy(store + used, t, (size_t)len);
    used += (uint32_t)len;
  }
  words[4] = used;
  return MMT_OK;
}

size_t mmt_text_tokens_workspace_bytes(int32_t B, int32_t F, int32_t budget) {
  if (B < 1 || F < 1 || budget < 0) return 0;
  return (size_t)B * (size_t)F * ((size_t)budget + 1) * 4;
}

int mmt_text_tokens(int32_t B, int32_t F, const uint8_t* bytes, int64_t bytes_len, const int64_t* offsets, const int32_t* lengths,
                    const void* vocab_image, size_t vocab_image_bytes, const uint32_t* codepoint_table, int64_t codepoint_entries,
                    const int32_t* field_token_ids, int32_t sep_id, int32_t unk_id, int32_t T, int32_t budget,
                    int32_t* token_ids_out, int32_t* num_wordpieces_out, uint8_t* word_start_out, void* workspace,
                    size_t workspace_bytes, void* stream) {
  if (B < 1 || F < 1 || T < 1)
    return mmt::fail(MMT_E_INVALID, "mmt_text_tokens: B (%d), F (%d) and T (%d) must be positive", B, F, T);
  if (F > mmt::kTextMaxFields)
    return mmt::fail(MMT_E_UNSUPPORTED, "mmt_text_tokens: F (%d) above %d fields", F, mmt::kTextMaxFields);
  if (budget < 0 || (int64_t)F + budget + 1 > T)
    return mmt::fail(MMT_E_INVALID, "mmt_text_tokens: F + budget + 1 (%d + %d + 1) must fit T (%d), budget >= 0", F, budget, T);
  if (!bytes || !offsets || !lengths || !vocab_image || !codepoint_table || !field_token_ids || !token_ids_out || !num_wordpieces_out ||
      !word_start_out)
    return mmt::fail(MMT_E_INVALID, "mmt_text_tokens: NULL argument (bytes, offsets, lengths, both tables, field_token_ids and the three outputs are required)");
  if (bytes_len < 0 || bytes_len >= ((int64_t)1 << 60))
    return mmt::fail(MMT_E_INVALID, "mmt_text_tokens: bytes_len %lld outside [0, 2^60)", (long long)bytes_len);
  if ((int64_t)B * F > 0x7fffffffLL || (int64_t)B * T > 0x7fffffffLL)
    return mmt::fail(MMT_E_UNSUPPORTED, "mmt_text_tokens: B * F and B * T must stay below 2^31");
  if (vocab_image_bytes < (size_t)mmt::kVocabHeaderWords * 4 + 32 || vocab_image_bytes > ((size_t)1 << 33))
    return mmt::fail(MMT_E_INVALID, "mmt_text_tokens: vocab_image_bytes %zu is no vocabulary image", vocab_image_bytes);
  if (codepoint_entries < (int64_t)mmt::kCodepoints || codepoint_entries > 0x7fffffffLL)
    return mmt::fail(MMT_E_INVALID, "mmt_text_tokens: codepoint_entries %lld below 0x110000", (long long)codepoint_entries);
  for (int f = 0; f < F; ++f)
    if (field_token_ids[f] < 0) return mmt::fail(MMT_E_INVALID, "mmt_text_tokens: field_token_ids[%d] is negative", f);
  if (sep_id < 0 || unk_id < 0) return mmt::fail(MMT_E_INVALID, "mmt_text_tokens: sep_id and unk_id must not be negative");
  if (((uintptr_t)offsets & 7) != 0 || (((uintptr_t)lengths | (uintptr_t)vocab_image | (uintptr_t)codepoint_table | (uintptr_t)token_ids_out |
                                         (uintptr_t)num_wordpieces_out) & 3) != 0)
    return mmt::fail(MMT_E_INVALID, "mmt_text_tokens: offsets must be 8-byte aligned; lengths, the tables and the int32 outputs 4-byte aligned");
  const size_t need = mmt_text_tokens_workspace_bytes(B, F, budget);
  if (!workspace || workspace_bytes < need)
    return mmt::fail(MMT_E_WORKSPACE, "mmt_text_tokens: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
  if (((uintptr_t)workspace & 3) != 0) return mmt::fail(MMT_E_INVALID, "mmt_text_tokens: workspace must be 4-byte aligned");
  mmt::TextParams p;
  p.B = B; p.F = F; p.T = T; p.budget = budget;
  p.bytes = bytes; p.nbytes = (long)bytes_len; p.offsets = (const long*)offsets; p.lengths = lengths;
  p.vocab = (const unsigned*)vocab_image; p.vocab_words = (unsigned)(vocab_image_bytes / 4);
  p.cp = codepoint_table; p.cp_entries = (unsigned)codepoint_entries;
  for (int f = 0; f < mmt::kTextMaxFields; ++f) p.field_tok[f] = f < F ? field_token_ids[f] : 0;
  p.sep = sep_id; p.unk = unk_id;
  p.ids = token_ids_out; p.count = num_wordpieces_out; p.wstart = word_start_out;
  p.pieces = (unsigned*)workspace;
  p.npieces = (int*)workspace + (size_t)B * (size_t)F * (size_t)budget;
  hipError_t e = mmt::launch_text_tokens(p, (hipStream_t)stream);
  return e == hipSuccess ? MMT_OK : mmt::fail(MMT_E_LAUNCH, "mmt_text_tokens: %s", hipGetErrorString(e));
}

}  // extern "C"
