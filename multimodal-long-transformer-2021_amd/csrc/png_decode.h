// Stage 2 of the PNG decode (png_decode.hip): the geometry of one image and of its passes with every size and offset
// clamped into the caller's buffers, the reconstruction of a filtered byte, and the expansion of a reconstructed unit
// into output pixels, shared by the kernel and the host loop through __host__ __device__ functions.  The rules are the
// PNG specification's (filters, Adam7) and libpng's palette and low-bit grey expansion, as DESIGN.md section 4 states
// them; everything is integer.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mmt_layer.h"

namespace mmt {

constexpr int kPngBand = 64;            // rows a wave reconstructs together, one per lane, skewed by one unit per row
constexpr int kPngGroup = 32;           // steps whose raw units a lane loads ahead of their use (divides kPngBand)
constexpr int kPngMaxSide = 1 << 30;    // largest width and height the decode takes (the step counter is an int)

struct PngParams {
  int B;
  const mmt_png_image* images;
  const unsigned char* raw;
  long raw_bytes;
  const unsigned char* palettes;        // [B][256][3]
  unsigned char* pixels;
  long pixels_bytes;
  unsigned char* keep;                  // workspace, raw_bytes bytes: a pass keeps one reconstructed row at its raw offset
};

// One image, clamped: no field below lets an index leave [0, raw_bytes) or [0, pixels_bytes).
struct PngGeom {
  int w, h;                             // w * h * 3 <= max(pixels_bytes, 3), each <= kPngMaxSide
  int depth;                            // bits of a sample: 1 | 2 | 4 | 8 (8 for RGB)
  int kind;                             // 0 grey | 2 RGB | 3 palette
  int bpp;                              // bytes of a filter unit: 3 for RGB, 1 otherwise
  int ppu;                              // pixels a unit holds: 8 / depth for grey and palette, 1 for RGB
  int passes;                           // 1 | 7
  int entries;                          // palette entries, 0..256
  long raw, raw_end;                    // the image's scanlines: [raw, raw_end) inside [0, raw_bytes)
  long pix;                             // first output byte
};

// One pass of an image (the whole image without interlace).  rows == 0: nothing to do.  Otherwise the rows are
// rows x (1 + rowbytes) bytes from off, all inside [g.raw, g.raw_end), and units >= 1.
struct PngPass {
  int rows, pw, units;                  // rows, pixels per row, filter units per row
  long rowbytes;                        // units * bpp
  long off;
  int x0, y0, dx, dy;                   // pixel (i, j) of the pass is output pixel (y0 + i * dy, x0 + j * dx)
};

__host__ __device__ inline long pclampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

__host__ __device__ inline PngGeom png_geom(const mmt_png_image& im, long raw_bytes, long pixels_bytes) {
  PngGeom g;
  const long max_px = pixels_bytes / 3 > 1 ? pixels_bytes / 3 : 1;
  g.w = (int)pclampl(im.width, 1, max_px < kPngMaxSide ? max_px : kPngMaxSide);
  g.h = (int)pclampl(im.height, 1, pclampl(max_px / g.w, 1, kPngMaxSide));
  g.kind = im.color_type == 2 ? 2 : (im.color_type == 3 ? 3 : 0);
  const int d = im.bit_depth;
  g.depth = g.kind == 2 || !(d == 1 || d == 2 || d == 4) ? 8 : d;
  g.bpp = g.kind == 2 ? 3 : 1;
  g.ppu = g.kind == 2 ? 1 : 8 / g.depth;
  g.passes = im.interlace == 1 ? 7 : 1;
  g.entries = (int)pclampl(im.palette_entries, 0, 256);
  g.raw = pclampl(im.raw_offset, 0, raw_bytes - 1);           // raw_bytes >= 1: the entry points refuse less
  g.raw_end = g.raw + pclampl(im.raw_bytes, 0, raw_bytes - g.raw);
  g.pix = pclampl(im.pixel_offset, 0, pixels_bytes - 1);
  return g;
}

// Adam7 as nibbles, pass p in bits [4p, 4p + 4): first column and row, column and row step.
__host__ __device__ inline int png_nibble(unsigned table, int p) { return (int)((table >> (4 * p)) & 15u); }

// Rows and pixels per row of pass p before any clamping.
__host__ __device__ inline void png_pass_size(const PngGeom& g, int p, PngPass& s) {
  if (g.passes == 1) {
    s.x0 = s.y0 = 0; s.dx = s.dy = 1;
  } else {
    s.x0 = png_nibble(0x0102040u, p); s.y0 = png_nibble(0x1020400u, p);
    s.dx = png_nibble(0x1224488u, p); s.dy = png_nibble(0x2244888u, p);
  }
  s.pw = g.w > s.x0 ? (g.w - s.x0 + s.dx - 1) / s.dx : 0;
  s.rows = g.h > s.y0 ? (g.h - s.y0 + s.dy - 1) / s.dy : 0;
  if (s.pw == 0 || s.rows == 0) s.pw = s.rows = 0;
  s.units = g.kind == 2 ? s.pw : (s.pw + g.ppu - 1) / g.ppu;
  s.rowbytes = (long)s.units * g.bpp;
}

__host__ __device__ inline PngPass png_pass(const PngGeom& g, int p) {
  PngPass s;
  long off = g.raw;
  for (int q = 0; q < p; ++q) {                                 // the passes in front; an empty pass holds no byte
    png_pass_size(g, q, s);
    off += (long)s.rows * (1 + s.rowbytes);                     // <= h * (1 + 3 w): no overflow, w * h * 3 < 2^60
  }
  png_pass_size(g, p, s);
  s.off = off;
  const long room = off < g.raw_end ? g.raw_end - off : 0;
  const long fit = room / (1 + s.rowbytes);
  if (s.rows > fit) s.rows = (int)fit;
  return s;
}

__host__ __device__ inline int png_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
}

// Reconstructs one filter unit of BPP bytes, byte k in bits [8k, 8k + 8) of every word: the filtered bytes x, the units
// to the left (a), above (b) and above left (c).  ft above 4 has been turned into 0 (None) by the caller.
template <int BPP>
__host__ __device__ inline unsigned png_recon_unit(int ft, unsigned x, unsigned a, unsigned b, unsigned c) {
  unsigned out = 0;
#pragma unroll
  for (int k = 0; k < BPP; ++k) {
    const int xa = (int)((a >> (8 * k)) & 255u), xb = (int)((b >> (8 * k)) & 255u), xc = (int)((c >> (8 * k)) & 255u);
    const int pred = ft == 1 ? xa : (ft == 2 ? xb : (ft == 3 ? (xa + xb) >> 1 : (ft == 4 ? png_paeth(xa, xb, xc) : 0)));
    out |= (((x >> (8 * k)) + (unsigned)pred) & 255u) << (8 * k);
  }
  return out;
}

__host__ __device__ inline void png_put(unsigned char* pixels, long pixels_bytes, long at, unsigned rgb) {
  if (at >= 0 && at + 3 <= pixels_bytes) {
    pixels[at] = (unsigned char)(rgb & 255u);
    pixels[at + 1] = (unsigned char)((rgb >> 8) & 255u);
    pixels[at + 2] = (unsigned char)((rgb >> 16) & 255u);
  }
}

// Converts the reconstructed unit x of row `row` of a pass and stores its pixels.  pal: 256 words r | g << 8 | b << 16.
__host__ __device__ inline void png_emit(const PngGeom& g, const PngPass& s, const unsigned* pal, int row, int x, unsigned v,
                                         unsigned char* pixels, long pixels_bytes) {
  const long line = g.pix + ((long)s.y0 + (long)row * s.dy) * g.w * 3;
  if (g.kind == 2) {
    png_put(pixels, pixels_bytes, line + ((long)s.x0 + (long)x * s.dx) * 3, v & 0xffffffu);
    return;
  }
  const unsigned mask = (1u << g.depth) - 1u;
  const unsigned scale = g.depth == 8 ? 1u : (g.depth == 4 ? 17u : (g.depth == 2 ? 85u : 255u));
  for (int i = 0; i < g.ppu; ++i) {
    const long j = (long)x * g.ppu + i;
    if (j >= s.pw) break;
    const unsigned smp = (v >> (8 - g.depth * (i + 1))) & mask;
    const unsigned rgb = g.kind == 3 ? ((int)smp < g.entries ? pal[smp] : 0u) : smp * scale * 0x010101u;
    png_put(pixels, pixels_bytes, line + ((long)s.x0 + j * s.dx) * 3, rgb);
  }
}

// The one kernel on `st`: grid (images, 7 passes), one wave each.
hipError_t launch_png_pixels(const PngParams& p, hipStream_t st);

}  // namespace mmt
