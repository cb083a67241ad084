// Stage 2 of the JPEG decode (jpeg_decode.hip): the geometry of one image with every size, grid and offset clamped
// into the caller's buffers, and the per-block and per-sample arithmetic, shared by the kernels and the host loop
// through __host__ __device__ functions.  The rules are libjpeg's defaults (JDCT_ISLOW, fancy upsampling) as DESIGN.md
// section 4 states them; everything is integer.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mmt_layer.h"

namespace mmt {

constexpr int kJpegGroup = 32;          // 8x8 blocks one workgroup of the IDCT pass takes per step (8 threads each)
constexpr int kJpegLdsStride = 72;      // ints per block in LDS: 64 + 8, so that the column reads of 4 blocks cover 32 banks

struct JpegParams {
  int B;
  int parts;                            // workgroups per image (grid.y) of both passes
  const mmt_jpeg_image* images;
  const short* coef;
  long coef_elems;
  const unsigned short* qtables;        // [B][3][64]
  unsigned char* pixels;
  long pixels_bytes;
  unsigned char* planes;                // workspace, coef_elems bytes: a component's plane starts at its coefficient offset
};

// One image, clamped: no field below lets an index leave [0, coef_elems) or [0, pixels_bytes).
struct JpegGeom {
  int nc;                               // 1 | 3
  int w, h;                             // w * h * 3 <= max(pixels_bytes, 3)
  int hs, vs;                           // luma samples per chroma sample, 1 | 2 each (vs == 2 only with hs == 2)
  int bw[3], bh[3];                     // block grids: bw * bh * 64 <= coef_elems
  int cw[3], ch[3];                     // real samples of the plane: ceil(w / hs) x ceil(h / vs) for chroma, inside the grid
  long off[3];                          // first coefficient (and first plane byte), a multiple of 8, <= coef_elems - 64
  long pix;                             // first output byte
  int nblk[3];                          // bw * bh
};

__host__ __device__ inline long jclampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }
__host__ __device__ inline int jclampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__host__ __device__ inline JpegGeom jpeg_geom(const mmt_jpeg_image& im, long coef_elems, long pixels_bytes) {
  JpegGeom g;
  g.nc = im.components == 3 ? 3 : 1;
  const long max_px = pixels_bytes / 3 > 1 ? pixels_bytes / 3 : 1;
  g.w = (int)jclampl(im.width, 1, max_px < 65535 ? max_px : 65535);
  g.h = (int)jclampl(im.height, 1, jclampl(max_px / g.w, 1, 65535));
  g.hs = g.nc == 3 && im.h_samp[0] == 2 ? 2 : 1;
  g.vs = g.hs == 2 && im.v_samp[0] == 2 ? 2 : 1;
  const long max_blk = coef_elems / 64;                   // >= 1: the entry points refuse coef_elems < 64
  for (int c = 0; c < 3; ++c) {
    g.bw[c] = (int)jclampl(im.blocks_w[c], 1, max_blk < 8192 ? max_blk : 8192);
    g.bh[c] = (int)jclampl(im.blocks_h[c], 1, jclampl(max_blk / g.bw[c], 1, 8192));
    g.nblk[c] = c < g.nc ? g.bw[c] * g.bh[c] : 0;         // <= 2^26
    g.off[c] = jclampl(im.coef_offset[c], 0, coef_elems - 64) & ~7L;
    const int sw = c == 0 ? g.w : (g.w + g.hs - 1) / g.hs, sh = c == 0 ? g.h : (g.h + g.vs - 1) / g.vs;
    g.cw[c] = jclampi(sw, 1, g.bw[c] * 8);
    g.ch[c] = jclampi(sh, 1, g.bh[c] * 8);
  }
  g.pix = jclampl(im.pixel_offset, 0, pixels_bytes - 1);
  return g;
}

// jidctint.c's slow-but-accurate 1-D pass on 8 values, CONST_BITS 13, FIX(x) = (int)(x * 8192 + 0.5); the sums wrap as
// unsigned 32-bit numbers (no signed overflow for any input; the same bits on well-formed data), the descale is an
// arithmetic shift with round-half-up.  SHIFT = 11 for the column pass (CONST_BITS - PASS1_BITS), 18 for the row pass.
template <int SHIFT>
__host__ __device__ inline void jpeg_idct_1d(const int (&in)[8], int (&out)[8]) {
  typedef unsigned U;
  const U i0 = (U)in[0], i1 = (U)in[1], i2 = (U)in[2], i3 = (U)in[3], i4 = (U)in[4], i5 = (U)in[5], i6 = (U)in[6], i7 = (U)in[7];
  const U z1e = (i2 + i6) * 4433u;                              // FIX(0.541196100)
  const U e2 = z1e + i6 * (U)-15137;                            // -FIX(1.847759065)
  const U e3 = z1e + i2 * 6270u;                                // FIX(0.765366865)
  const U e0 = (i0 + i4) << 13, e1 = (i0 - i4) << 13;
  const U t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  U o0 = i7, o1 = i5, o2 = i3, o3 = i1;
  U z1 = o0 + o3, z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
  const U z5 = (z3 + z4) * 9633u;                               // FIX(1.175875602)
  o0 *= 2446u;                                                  // FIX(0.298631336)
  o1 *= 16819u;                                                 // FIX(2.053119869)
  o2 *= 25172u;                                                 // FIX(3.072711026)
  o3 *= 12299u;                                                 // FIX(1.501321110)
  z1 *= (U)-7373;                                               // -FIX(0.899976223)
  z2 *= (U)-20995;                                              // -FIX(2.562915447)
  z3 *= (U)-16069;                                              // -FIX(1.961570560)
  z4 *= (U)-3196;                                               // -FIX(0.390180644)
  z3 += z5; z4 += z5;
  o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
  const U r = 1u << (SHIFT - 1);
  out[0] = (int)(t10 + o3 + r) >> SHIFT; out[7] = (int)(t10 - o3 + r) >> SHIFT;
  out[1] = (int)(t11 + o2 + r) >> SHIFT; out[6] = (int)(t11 - o2 + r) >> SHIFT;
  out[2] = (int)(t12 + o1 + r) >> SHIFT; out[5] = (int)(t12 - o1 + r) >> SHIFT;
  out[3] = (int)(t13 + o0 + r) >> SHIFT; out[4] = (int)(t13 - o0 + r) >> SHIFT;
}

__host__ __device__ inline int jpeg_sample_of(int v) { return jclampi(v + 128, 0, 255); }    // after the row pass

// A component plane in the workspace: rows of `stride` bytes from `off`; every address is capped at `last`.
struct JpegPlane {
  const unsigned char* base;
  long off, last;
  int stride;
  __host__ __device__ int operator()(int r, int c) const {
    const long a = off + (long)r * stride + c;
    return base[a < last ? a : last];
  }
};

// The chroma sample libjpeg's upsampler gives output pixel (x, y): cw x ch real samples, neighbours replicated at the
// edges (never read from the MCU padding); a plane at most 2 samples wide is replicated, not filtered.
__host__ __device__ inline int jpeg_chroma_at(const JpegPlane& s, int cw, int ch, int hs, int vs, int x, int y) {
  if (hs == 1) return s(y, x);
  const int i = x >> 1;
  if (cw <= 2) return s(vs == 2 ? y >> 1 : y, i);
  const int nb = x & 1 ? (i + 1 < cw ? i + 1 : cw - 1) : (i > 0 ? i - 1 : 0);
  if (vs == 1) return (3 * s(y, i) + s(y, nb) + (x & 1 ? 2 : 1)) >> 2;
  const int rn = y >> 1;
  const int rf = y & 1 ? (rn + 1 < ch ? rn + 1 : ch - 1) : (rn > 0 ? rn - 1 : 0);
  const int ci = 3 * s(rn, i) + s(rf, i), cn = 3 * s(rn, nb) + s(rf, nb);
  return (3 * ci + cn + (x & 1 ? 7 : 8)) >> 4;
}

// YCbCr -> RGB with libjpeg's 16-bit fixed point, F(x) = (int)(x * 65536 + 0.5); shifts are arithmetic.
__host__ __device__ inline void jpeg_rgb(int y, int cb, int cr, int (&rgb)[3]) {
  cb -= 128; cr -= 128;
  rgb[0] = jclampi(y + ((91881 * cr + 32768) >> 16), 0, 255);                    // F(1.402)
  rgb[1] = jclampi(y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255);      // F(0.34414), F(0.71414)
  rgb[2] = jclampi(y + ((116130 * cb + 32768) >> 16), 0, 255);                   // F(1.772)
}

// The three bytes of output pixel (x, y) of an image whose planes the IDCT pass has written.
__host__ __device__ inline void jpeg_pixel_at(const JpegGeom& g, const unsigned char* planes, long planes_bytes, int x, int y,
                                              int (&rgb)[3]) {
  const JpegPlane py = {planes, g.off[0], planes_bytes - 1, g.bw[0] * 8};
  const int Y = py(y, x);
  if (g.nc == 1) { rgb[0] = rgb[1] = rgb[2] = Y; return; }
  const JpegPlane pb = {planes, g.off[1], planes_bytes - 1, g.bw[1] * 8}, pr = {planes, g.off[2], planes_bytes - 1, g.bw[2] * 8};
  jpeg_rgb(Y, jpeg_chroma_at(pb, g.cw[1], g.ch[1], g.hs, g.vs, x, y), jpeg_chroma_at(pr, g.cw[2], g.ch[2], g.hs, g.vs, x, y), rgb);
}

// The IDCT pass and the upsampling + colour pass, both on `st`.
hipError_t launch_jpeg_pixels(const JpegParams& p, hipStream_t st);

}  // namespace mmt
