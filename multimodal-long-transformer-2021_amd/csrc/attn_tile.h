// Tile-level building blocks shared by the forward and backward attention kernels (gfx950).
#pragma once
#include <type_traits>

#include "attn_kernels.h"

namespace mmt {

// DH = head size (64 | 128).  Every DH = 64 form below is the code the lean kernels were written against.
template <typename T, int DH = 64> struct Frag;

// Tile walk of a 32-row block at x0 under a pattern with the image-grid term (grid.ga > 0): the ascending union of
//   the band's tiles, the global tokens' tiles, and, for each image-row offset dr in [-a, a], the tiles of
//   [ia + dr P - a, ib + dr P + a] n [gs, gs + P^2), [ia, ib] = the block's rows inside the image,
// i.e. every tile that can hold an unmasked pair, each once (a tile counted twice would enter the online softmax and
// the dK/dV sums twice).  The pattern is symmetric in (q, k): the dK/dV pass walks the query tiles of a key block with
// the same walk.  Everything here is wave-uniform scalars; next(t) scans the <= 2a + 3 sources for the smallest tile
// >= t of the union (no runtime-indexed per-lane array: those go to scratch).  The split items of the global rows /
// keys walk their chunk [band_lo, band_hi] alone (empty global and grid sources).
struct GridWalk {
  static constexpr int kEnd = 0x7fffffff;
  int band_lo, band_hi, glob_lo, glob_hi;   // tile ranges (lo > hi: empty)
  int ia, ib, img_lo, img_hi;               // positions
  int a, P;
  __device__ __forceinline__ void init_band(const PatternDev& pat, const GridDev& grid, int x0, int S) {
    band_lo = max(x0 - pat.radius, 0) >> 5;
    band_hi = min(x0 + 31 + pat.radius, S - 1) >> 5;
    glob_lo = pat.ng > 0 ? pat.g0 >> 5 : 1;
    glob_hi = pat.ng > 0 ? (pat.g0 + pat.ng - 1) >> 5 : 0;
    img_lo = grid.gs; img_hi = grid.gs + grid.gI - 1;
    ia = max(x0, img_lo); ib = min(x0 + 31, img_hi);
    a = grid.ga; P = pat.P;
  }
  // Per-example origin: a block whose rows all lie in the example that starts at `start` -- its image is at
  // [start + g, start + g + P^2), cut at the end of the row (a start the caller clamped into [0, S): every tile the
  // walk names is a tile of the row).  The union is not cut at the example's end here: the caller walks PackWalk's
  // candidates over span() -- the id-range test leaves out what lies outside the example -- and keeps those has() names.
  __device__ __forceinline__ void init_origin(const PatternDev& pat, const GridDev& grid, int x0, int S, int start) {
    init_band(pat, grid, x0, S);
    img_lo = min(start + grid.gs, S - 1); img_hi = min(img_lo + grid.gI - 1, S - 1);
    ia = max(x0, img_lo); ib = min(x0 + 31, img_hi);
  }
  // Per-example global tokens (the GLB instantiations), after init_origin: the range moves with the example's start,
  // [start + g0, start + g0 + ng) cut at the end of the row.  Not cut at the example's end, as the image.
  __device__ __forceinline__ void init_origin_globals(const PatternDev& pat, int S, int start) {
    const int lo = start + pat.g0;
    const bool any = pat.ng > 0 && lo < S;
    glob_lo = any ? lo >> 5 : 1;
    glob_hi = any ? min(lo + pat.ng - 1, S - 1) >> 5 : 0;
  }
  // first and last tile of the union (the band is never empty: it holds the block's own tile)
  __device__ __forceinline__ void span(int& t_lo, int& t_hi) const {
    t_lo = next(0);
    t_hi = max(band_hi, glob_hi);
    if (ia <= ib) t_hi = max(t_hi, min(ib + a * P + a, img_hi) >> 5);
  }
  __device__ __forceinline__ bool has(int t) const { return next(t) == t; }
  __device__ __forceinline__ void init_chunk(int t0, int t1) {
    band_lo = t0; band_hi = t1; glob_lo = 1; glob_hi = 0; ia = 1; ib = 0; img_lo = img_hi = 0; a = 0; P = 1;
  }
  __device__ __forceinline__ int next(int t) const {
    int best = kEnd;
    if (max(band_lo, t) <= band_hi) best = max(band_lo, t);
    if (max(glob_lo, t) <= glob_hi) best = min(best, max(glob_lo, t));
    if (ia <= ib) {
      for (int dr = -a; dr <= a; ++dr) {       // intervals ascend with dr
        const int lo = max(ia + dr * P - a, img_lo), hi = min(ib + dr * P + a, img_hi);
        if (lo > hi) continue;
        const int c = max(lo >> 5, t);
        if (c >= best) break;
        if (c <= (hi >> 5)) best = c;
      }
    }
    return best;
  }
};

// Packed examples (MMT_FLAG_EXAMPLE_IDS): tile walk of a 32-row block whose segmented term is ids[x] == ids[y].
// The candidates are the tiles of the plain walk (`at(0 .. n_it)`: band, global tiles or a chunk); a candidate none of
// whose 32 ids lies in [lo, hi], the id range of the block's own rows, cannot hold an allowed pair and is left out
// BEFORE anything of it is fetched -- valid for any ids, effective for ids that came from breakpoints (monotone along
// the row).  Eight candidates are judged per step: lane (r, h) reads id r of candidates base + 2j + h, j = 0..3 (four
// independent coalesced 128-byte loads per half, one latency), a ballot per j gives the two hit bits.  Everything kept
// here is wave-uniform.  Positions >= S never hit.
struct PackWalk {
  static constexpr int kEnd = 0x7fffffff;
  const int32_t* ids;     // [S] example ids of the batch row
  int lo, hi;             // id range of the block's rows
  bool all;               // visit every candidate (no tile is left out)
  int S, n_it;
  int base;               // candidates [base, base + 8) have been judged
  unsigned hits;          // ... and these of them are still to visit
  // id of position x of the row (clamped to the sequence: callers mask x >= S themselves)
  __device__ __forceinline__ int id_at(int x) const { return ids[min(x, S - 1)]; }
  // start of the example of position x (MMT_FLAG_EXAMPLE_STARTS only: `ids` is plane 0 of the row's [2,S], the starts
  // are plane 1), clamped into [0, S)
  __device__ __forceinline__ int start_at(int x) const { return min(max(ids[S + min(x, S - 1)], 0), S - 1); }
  // Per-example global tokens, a block of several examples none of whose rows is a global one: the candidates run from
  // the lowest to the highest tile that the block's band or the global range of any of its rows' examples touches
  // (st = the row's example start, the same in both halves); the id-range test filters them.
  __device__ __forceinline__ void span_globals(const PatternDev& pat, int x0, int st, int& t_lo, int& t_hi) const {
    int mn = st, mx = st;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      mn = min(mn, __shfl_xor(mn, o, 64));
      mx = max(mx, __shfl_xor(mx, o, 64));
    }
    mn = __builtin_amdgcn_readfirstlane(mn);
    mx = __builtin_amdgcn_readfirstlane(mx);
    t_lo = max(min(x0 - pat.radius, mn + pat.g0), 0) >> 5;
    t_hi = min(max(x0 + 31 + pat.radius, mx + pat.g0 + pat.ng - 1), S - 1) >> 5;
  }
  // [lo, hi] over the 32 rows x0 .. x0 + 31 (own = id of row x0 + (lane & 31), the same in both halves)
  __device__ __forceinline__ void init(const int32_t* row_ids, int own, int S_, int n_it_, bool skip) {
    ids = row_ids; S = S_; n_it = n_it_; base = -8; hits = 0;
    int mn = own, mx = own;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      mn = min(mn, __shfl_xor(mn, o, 64));
      mx = max(mx, __shfl_xor(mx, o, 64));
    }
    lo = __builtin_amdgcn_readfirstlane(mn);
    hi = __builtin_amdgcn_readfirstlane(mx);
    all = !skip;
  }
  // next tile to visit (kEnd: none left); `at` maps a candidate number to its tile
  template <typename At>
  __device__ __forceinline__ int next(const At& at, int lane) {
    const int r = lane & 31, h = lane >> 5;
    while (hits == 0) {
      base += 8;
      if (base >= n_it) return kEnd;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = base + 2 * j + h;
        const int x = at(min(c, n_it - 1)) * 32 + r;
        const int id = id_at(x);
        const bool hit = c < n_it && x < S && (all || (id >= lo && id <= hi));
        const unsigned long long m = __ballot(hit);
        hits |= ((unsigned)m != 0u ? 1u : 0u) << (2 * j) | ((unsigned)(m >> 32) != 0u ? 1u : 0u) << (2 * j + 1);
      }
    }
    const int j = __builtin_ctz(hits);
    hits &= hits - 1;
    return at(base + j);
  }
};

// ------------------------------- bf16: 32x32x16 MFMA ---------------------------------
// MFMA k-index (8h + j) of step s is mapped to head-dim d = (DH/2)h + 8s + j, so each lane
// loads DH contiguous bytes of its row (DH/16 x 16 B).
template <int DH> struct Frag<__bf16, DH> {
  bf16x8 v[DH / 16];
  __device__ __forceinline__ void load_row(const __bf16* row, int h) {
#pragma unroll
    for (int s = 0; s < DH / 16; ++s) v[s] = *reinterpret_cast<const bf16x8*>(row + (DH / 2) * h + 8 * s);
  }
};
template <int DH>
__device__ __forceinline__ f32x16 mma_rows(const Frag<__bf16, DH>& a, const Frag<__bf16, DH>& b, f32x16 c) {
#pragma unroll
  for (int s = 0; s < DH / 16; ++s) c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v[s], b.v[s], c, 0, 0, 0);
  return c;
}

// ------------------------------- f32: 32x32x2 MFMA (exact f32) -----------------------
// MFMA k-index h of step s is mapped to d = (DH/2)h + s: each lane loads 2 DH contiguous bytes.
template <int DH> struct Frag<float, DH> {
  float v[DH / 2];
  __device__ __forceinline__ void load_row(const float* row, int h) {
#pragma unroll
    for (int s = 0; s < DH / 2; s += 4) {
      f32x4 t = *reinterpret_cast<const f32x4*>(row + (DH / 2) * h + s);
      v[s] = t[0]; v[s + 1] = t[1]; v[s + 2] = t[2]; v[s + 3] = t[3];
    }
  }
};
template <int DH>
__device__ __forceinline__ f32x16 mma_rows(const Frag<float, DH>& a, const Frag<float, DH>& b, f32x16 c) {
#pragma unroll
  for (int s = 0; s < DH / 2; ++s) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[s], b.v[s], c, 0, 0, 0);
  return c;
}

// V rows of one tile held in registers between the global load and their use.
template <typename T, int DH = 64> struct VTile;
template <> struct VTile<__bf16, 64> {   // 4 x 16-B chunks per lane -> written to the LDS tile
  bf16x8 c[4];
  __device__ __forceinline__ void load(const __bf16* V, unsigned vs1, int k0, int S, int lane, int) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ci = lane + 64 * u, row = ci >> 3, ch = ci & 7;
      const unsigned kk = (unsigned)min(k0 + row, S - 1);  // rows past the end repeat the last row; their p is 0
      c[u] = *reinterpret_cast<const bf16x8*>(V + (kk * vs1 + (unsigned)ch * 8u));
    }
  }
  // 32 rows x 128 B; the two 64-B halves of a row are swapped when bit 1 of the row is set,
  // which makes the 4-row transposed reads below bank-conflict free.
  __device__ __forceinline__ void to_lds(unsigned char* vlds, int lane) const {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ci = lane + 64 * u, row = ci >> 3, ch = ci & 7;
      const int off = row * 128 + ((((ch >> 2) ^ ((row >> 1) & 1))) << 6) + (ch & 3) * 16;
      *reinterpret_cast<bf16x8*>(vlds + off) = c[u];
    }
  }
};
template <> struct VTile<float, 64> {    // A operand of the 32x32x2 PV product, straight from L2
  float a0[16], a1[16];
  __device__ __forceinline__ void load(const float* V, unsigned vs1, int k0, int S, int lane, int) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const unsigned kk = (unsigned)min(k0 + kap(s, h), S - 1);
      const float* vr = V + kk * vs1;
      a0[s] = vr[r]; a1[s] = vr[32 + r];
    }
  }
  __device__ __forceinline__ void to_lds(unsigned char*, int) const {}
};

// DH = 128, bf16: 32 rows x 256 B.  A 256-B row spans all 64 banks, so the 128-B rows' half swap cannot work; the
// 16-B slot c of row r is stored at slot c ^ g(r), g(r) = 4 (r & 3) + ((r >> 2) & 3).  Bank pattern:
//  - ds_read_b64_tr_b16 (mma_xt): a 32-lane half reads rows 4i .. 4i+3, the same 64-B d-block db of each; the block of
//    row 4i + j lands in quarter db ^ j and its four slots are permuted by the constant i & 3 -- four quarters x four
//    slots x two 8-B halves = all 64 banks once: conflict-free;
//  - ds_read_b128 (frag_from_tile, one slot per lane): the rows of a 16-lane group, {0-3, 12-15, 20-27} or
//    {4-11, 16-19, 28-31}, have 16 distinct g(r): 16 distinct slots = 64 banks, conflict-free;
//  - ds_write_b128 (to_lds, bank = (a/4) mod 32): 8 consecutive lanes write slots c .. c+7 of one row, still distinct
//    mod 8 after the XOR: conflict-free.
__device__ __forceinline__ int swz256(int row, int slot) {
  return row * 256 + ((slot ^ (((row & 3) << 2) | ((row >> 2) & 3))) << 4);
}
template <> struct VTile<__bf16, 128> {   // 8 x 16-B chunks per lane (16 lanes per row) -> the LDS tile
  bf16x8 c[8];
  __device__ __forceinline__ void load(const __bf16* V, unsigned vs1, int k0, int S, int lane, int) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int ci = lane + 64 * u, row = ci >> 4, ch = ci & 15;
      const unsigned kk = (unsigned)min(k0 + row, S - 1);  // rows past the end repeat the last row; their p is 0
      c[u] = *reinterpret_cast<const bf16x8*>(V + (kk * vs1 + (unsigned)ch * 8u));
    }
  }
  __device__ __forceinline__ void to_lds(unsigned char* vlds, int lane) const {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int ci = lane + 64 * u, row = ci >> 4, ch = ci & 15;
      *reinterpret_cast<bf16x8*>(vlds + swz256(row, ch)) = c[u];
    }
  }
};
template <> struct VTile<float, 128> {   // A operand of the 32x32x2 products, four 32-column blocks
  float a[4][16];
  __device__ __forceinline__ void load(const float* V, unsigned vs1, int k0, int S, int lane, int) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const unsigned kk = (unsigned)min(k0 + kap(s, h), S - 1);
      const float* vr = V + kk * vs1;
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j][s] = vr[32 * j + r];
    }
  }
  __device__ __forceinline__ void to_lds(unsigned char*, int) const {}
};
// DH = 128, bf16, staged through a 32 x 128 B buffer: the two 64-column halves as DH = 64 tiles, written to the LDS
// one after the other by the product itself (mma_xt below).  For the dQ pass at Rp = 128, whose four waves' full
// 256-B tiles would pass the CU's 160 KiB (BwdLds).
struct HalfTile {
  VTile<__bf16, 64> lo, hi;
  __device__ __forceinline__ void load(const __bf16* V, unsigned vs1, int k0, int S, int lane, int) {
    lo.load(V, vs1, k0, S, lane, 0);
    hi.load(V + 64, vs1, k0, S, lane, 0);
  }
  __device__ __forceinline__ void to_lds(unsigned char*, int) const {}
};

// Row fragment (MFMA A/B operand, row = lane & 31) read back from a wave-private LDS tile that
// was written with VTile<__bf16>::to_lds: saves the second, fragment-shaped global load.
__device__ __forceinline__ void frag_from_tile(Frag<__bf16>& f, const unsigned char* lds, int lane) {
  const int r = lane & 31, h = lane >> 5;
  const unsigned char* row = lds + r * 128 + ((h ^ ((r >> 1) & 1)) << 6);
#pragma unroll
  for (int s = 0; s < 4; ++s) f.v[s] = *reinterpret_cast<const bf16x8*>(row + s * 16);
}

__device__ __forceinline__ void frag_from_tile(Frag<__bf16, 128>& f, const unsigned char* lds, int lane) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int s = 0; s < 8; ++s) f.v[s] = *reinterpret_cast<const bf16x8*>(lds + swz256(r, 8 * h + s));
}

__device__ __forceinline__ float half_xchg(float x) { return __shfl_xor(x, 32, 64); }
// Reductions over the lane pair (l, l ^ 32) with gfx950's v_permlane32_swap: after the swap
// `a` holds the low half's value and `b` the high half's in every lane -- one VALU op and no LDS
// round trip (ds_bpermute) in the per-tile dependency chain.
__device__ __forceinline__ void half_pair(float x, float& a, float& b) {
  a = x; b = x;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ float half_max(float x) { float a, b; half_pair(x, a, b); return fmaxf(a, b); }
__device__ __forceinline__ float half_sum(float x) { float a, b; half_pair(x, a, b); return a + b; }

// Row stride of the per-wave relative-score tables (floats).  Two access shapes matter: a column read by
// 32 lanes (address r * stride + c) and the DIAGONAL gather of a mixed-id tile, where lane r reads column
// c - r (address r * (stride - 1) + c).  Rp + 1 made the second a 32-way bank conflict (32 r + c hits two
// banks); with Rp + 2 the first walks 34 r (32 distinct even banks) and the second 33 r (all distinct).
constexpr int kTStride(int Rp) { return Rp + 2; }
constexpr float kRescaleThr = 6.0f;

// LDS carve per wave: T table [32][kTStride] f32, then (bf16 only) V tile 32 x 2 DH B.
template <typename T, int Rp, int DH = 64> struct WaveLds {
  static constexpr int kTBytes = 32 * kTStride(Rp) * 4;
  static constexpr int kTBytesAligned = (kTBytes + 15) & ~15;
  static constexpr int kVBytes = sizeof(T) == 2 ? 32 * 2 * DH : 0;
  static constexpr int kBytes = kTBytesAligned + kVBytes;
};

// Column of relative id `id` inside the LDS table.  For the 1-D generator the columns are
// permuted so that column = clamp(k - q, -m, m) + m: the hot loop then needs no sign
// handling (id <= m  <->  d = id;  m < id <= 2m  <->  d = m - id).
__device__ __forceinline__ int tcol(int perm_1d, int m, int id) {
  const int pc = id <= m ? m + id : 2 * m - id;
  return ((perm_1d != 0) & (id <= 2 * m)) ? pc : id;
}
// Inverse of tcol for the permuted (1-D) layout: the relative id whose score lives in table column c.  The lean
// kernels load E row icol(m, r) into fragment row r, so that the table product comes out in COLUMN order and is
// stored without a per-element tcol().
__device__ __forceinline__ int icol(int m, int c) {
  return c > 2 * m ? c : (c >= m ? c - m : 2 * m - c);
}


// acc^T[d x col] += X^T[d x row] . vals[row x col] for a 32-row tile X staged as a VTile:
// the 32x32 accumulator-layout values `vals` (16 per lane) are the B operand as they stand
// (guide: "an accumulator tile as the next MFMA's operand"); X^T fragments come from the
// wave-private LDS tile through ds_read_b64_tr_b16 (bf16) or straight from registers (f32).
// Eight f32 -> eight bf16 (round to nearest even) as FOUR v_cvt_pk_bf16_f32: a vector conversion.  Converted element by
// element, hipcc emits one conversion per value and merges the halves with v_perm_b32 -- 24 instructions for a 16-value
// fragment where 8 do.  (Not inline asm: an MFMA that reads a register an `asm` has just written gets no hazard padding
// from the compiler -- a hand-written v_cvt_pk in front of the peeled step's products gave infinities in 4-lane groups.)
typedef __attribute__((ext_vector_type(8))) float f32x8_t;
__device__ __forceinline__ bf16x8 pack8_bf16(const float* v) {
  const f32x8_t x = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]};
  return __builtin_convertvector(x, bf16x8);
}

__device__ __forceinline__ void mma_xt(f32x16& a0, f32x16& a1, const VTile<__bf16>&,
                                       const unsigned char* xlds, const float (&vals)[16], int lane) {
  const int h = lane >> 5, li = lane & 15, cb = (lane >> 4) & 1;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const bf16x8 pf = pack8_bf16(vals + 8 * s);
#pragma unroll
    for (int db = 0; db < 2; ++db) {
      const int row = 16 * s + 4 * h + (li >> 2);
      const int within = 32 * cb + 8 * (li & 3);  // byte offset inside the 64-B half
      const int off0 = row * 128 + ((db ^ ((row >> 1) & 1)) << 6) + within;
      const int row1 = row + 8;
      const int off1 = row1 * 128 + ((db ^ ((row1 >> 1) & 1)) << 6) + within;
      s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4*)(xlds + off0));
      s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4*)(xlds + off1));
      bf16x8 vf;
      bf16x4 lo4 = __builtin_bit_cast(bf16x4, lo), hi4 = __builtin_bit_cast(bf16x4, hi);
#pragma unroll
      for (int j = 0; j < 4; ++j) { vf[j] = lo4[j]; vf[4 + j] = hi4[j]; }
      if (db == 0) a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, a0, 0, 0, 0);
      else a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, a1, 0, 0, 0);
    }
  }
}
__device__ __forceinline__ void mma_xt(f32x16& a0, f32x16& a1, const VTile<float>& x,
                                       const unsigned char*, const float (&vals)[16], int) {
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x.a0[s], vals[s], a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x.a1[s], vals[s], a1, 0, 0, 0);
  }
}

// Same product with `vals` split into bf16 hi + lo parts (about 16 mantissa bits): used where
// the right-hand values are sums that must not be rounded to bf16 (dRel . E).
__device__ __forceinline__ void mma_xt_hilo(f32x16& a0, f32x16& a1, const VTile<__bf16>& x,
                                            const unsigned char* xlds, const float (&vals)[16], int lane) {
  float hi[16], lo[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { hi[i] = (float)(__bf16)vals[i]; lo[i] = vals[i] - hi[i]; }
  mma_xt(a0, a1, x, xlds, hi, lane);
  mma_xt(a0, a1, x, xlds, lo, lane);
}
__device__ __forceinline__ void mma_xt_hilo(f32x16& a0, f32x16& a1, const VTile<float>& x,
                                            const unsigned char* xlds, const float (&vals)[16], int lane) {
  mma_xt(a0, a1, x, xlds, vals, lane);
}

// DH = 128: the products into four accumulators a0 .. a3 (head dims 32j .. 32j+31 in a_j).
// bf16: as the DH = 64 form, four d-blocks (64-B quarters of the 256-B rows, swz256) per key step.
__device__ __forceinline__ void mma_xt(f32x16& a0, f32x16& a1, f32x16& a2, f32x16& a3, const VTile<__bf16, 128>&,
                                       const unsigned char* xlds, const float (&vals)[16], int lane) {
  const int h = lane >> 5, li = lane & 15, cb = (lane >> 4) & 1;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const bf16x8 pf = pack8_bf16(vals + 8 * s);
#pragma unroll
    for (int db = 0; db < 4; ++db) {
      const int row = 16 * s + 4 * h + (li >> 2);
      const int slot = 4 * db + 2 * cb + ((li & 3) >> 1), byte = 8 * (li & 1);   // 8 B at 32 cb + 8 (li & 3) of the block
      s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4*)(xlds + swz256(row, slot) + byte));
      s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4*)(xlds + swz256(row + 8, slot) + byte));
      bf16x8 vf;
      bf16x4 lo4 = __builtin_bit_cast(bf16x4, lo), hi4 = __builtin_bit_cast(bf16x4, hi);
#pragma unroll
      for (int j = 0; j < 4; ++j) { vf[j] = lo4[j]; vf[4 + j] = hi4[j]; }
      f32x16& a = db == 0 ? a0 : (db == 1 ? a1 : (db == 2 ? a2 : a3));
      a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, a, 0, 0, 0);
    }
  }
}
__device__ __forceinline__ void mma_xt(f32x16& a0, f32x16& a1, f32x16& a2, f32x16& a3, const VTile<float, 128>& x,
                                       const unsigned char*, const float (&vals)[16], int) {
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x.a[0][s], vals[s], a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x.a[1][s], vals[s], a1, 0, 0, 0);
    a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(x.a[2][s], vals[s], a2, 0, 0, 0);
    a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(x.a[3][s], vals[s], a3, 0, 0, 0);
  }
}
// HalfTile: each half written to the 32 x 128 B buffer right before its product (LDS accesses of one wave complete in
// order: the high half's stores follow the low half's reads)
__device__ __forceinline__ void mma_xt(f32x16& a0, f32x16& a1, f32x16& a2, f32x16& a3, const HalfTile& x,
                                       unsigned char* xlds, const float (&vals)[16], int lane) {
  x.lo.to_lds(xlds, lane);
  mma_xt(a0, a1, x.lo, xlds, vals, lane);
  x.hi.to_lds(xlds, lane);
  mma_xt(a2, a3, x.hi, xlds, vals, lane);
}
template <typename X>
__device__ __forceinline__ void mma_xt_hilo(f32x16& a0, f32x16& a1, f32x16& a2, f32x16& a3, const X& x,
                                            unsigned char* xlds, const float (&vals)[16], int lane) {
  if constexpr (std::is_same<X, VTile<float, 128>>::value) {
    mma_xt(a0, a1, a2, a3, x, xlds, vals, lane);
  } else {
    float hi[16], lo[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { hi[i] = (float)(__bf16)vals[i]; lo[i] = vals[i] - hi[i]; }
    mma_xt(a0, a1, a2, a3, x, xlds, hi, lane);
    mma_xt(a0, a1, a2, a3, x, xlds, lo, lane);
  }
}

}  // namespace mmt
