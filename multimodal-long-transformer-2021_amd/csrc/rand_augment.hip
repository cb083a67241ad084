// RandAugment on the device (C ABI: include/mmt_layer.h, mmt_rand_augment): one of the reference's 14 operations per
// image (`RandAugment(num_layers=1)` with the list of src/data/data_utils.py:125-145), uint8 in and uint8 out at the
// source resolution, on the packed layout of mmt_image_patches -- the step of `decode_fn` (:199-202) in front of it.
// The definitions are those of DESIGN.md section 4; ids outside [0, 13] copy the image.
//
//   table ops      AutoContrast, Equalize, Posterize, Solarize, SolarizeAdd, Contrast, Brightness: v' = table[channel][v]
//   per-pixel ops  Color (blend against the pixel's grey), Sharpness (blend against the 3x3 smoothing), and the affine
//                  gather of Rotate / ShearX / ShearY / TranslateX / TranslateY (nearest source pixel, 128 outside)
//
// Two kernels behind one clear of the histograms:
//   1. statistics: images with op 0, 1 or 6 only.  Per-workgroup LDS histograms (R, G, B; grey for Contrast) over
//      chunks of kRandAugChunk pixels, merged into the workspace with integer atomicAdd -- integer sums do not depend
//      on the order, so the result is bitwise reproducible.  No float atomics anywhere.
//   2. apply: every workgroup of an image builds the image's [3][256] byte table in LDS from the histograms and the
//      arguments (a few hundred LDS operations; the table pass is merged in here), then streams its share of the
//      image: table ops as a flat byte stream with 16-byte loads and stores where source and destination share their
//      alignment (scalar head and tail), channel = byte index mod 3; the others one pixel per thread.
//
// All float arithmetic that reaches a pixel is fp32 with every product and sum rounded on its own: the unit is built
// with -ffp-contract=off (csrc/Makefile) and says so again below.
//
// Bounds (the front end's rule): h / w below 1 count as 1, the image's offset is clamped into the pixel buffer, the
// bytes an image covers are cut at the end of the buffer, every read address is clamped to pixels_bytes - 1 and no
// byte is written at or beyond pixels_bytes.  Bad metadata gives wrong pixels, never a stray access.
#include "../../include/mmt_attn.h"
#include "../../include/mmt_layer.h"

#include <cstdint>

#include "mmt_err.h"
#include "rand_augment.h"

#pragma clang fp contract(off)

#ifndef MMT_RAND_AUGMENT_HOST_ONLY
namespace mmt {
namespace {

struct Span {
  unsigned long base, last;      // first byte of the image, last byte of the buffer
  long npix, nbytes;             // pixels taken (h * w, at most pixels_bytes), bytes covered inside the buffer
  int h, w;
};

__device__ __forceinline__ Span image_span(const RandAugParams& p, int b) {
  Span s;
  s.h = max(p.heights[b], 1);
  s.w = max(p.widths[b], 1);
  s.last = (unsigned long)(p.pixels_bytes - 1);
  s.base = (unsigned long)min(max(p.offsets[b], 0L), p.pixels_bytes - 1);
  s.npix = min((long)s.h * (long)s.w, p.pixels_bytes);               // < 2^60: the * 3 below cannot wrap
  s.nbytes = min(s.npix * 3, p.pixels_bytes - (long)s.base);
  return s;
}

__device__ __forceinline__ int grey_of(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

// blend(a, b, f) with d = b - a: trunc(clip(a + f * d, 0, 255)), product and sum rounded separately.
__device__ __forceinline__ int blend(int a, int d, float f) {
  const float prod = f * (float)d;
  const float t = (float)a + prod;
  return (int)fminf(fmaxf(t, 0.f), 255.f);
}

__device__ __forceinline__ bool needs_stats(int op) { return op == 0 || op == 1 || op == 6; }
__device__ __forceinline__ bool is_pixel_op(int op) { return op == 2 || op == 5 || (op >= 8 && op <= 12); }

__global__ __launch_bounds__(256) void rand_augment_stats_kernel(const RandAugParams p) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int op = p.op[b];
  if (!needs_stats(op)) return;
  const Span s = image_span(p, b);
  const long nchunk = (s.npix + kRandAugChunk - 1) / kRandAugChunk;
  if ((long)blockIdx.y >= nchunk) return;
  __shared__ unsigned hist[4 * 256];
  for (int i = tid; i < 4 * 256; i += 256) hist[i] = 0u;
  __syncthreads();
  for (long c = blockIdx.y; c < nchunk; c += gridDim.y) {
    const long q1 = min((c + 1) * kRandAugChunk, s.npix);
    for (long q = c * kRandAugChunk + tid; q < q1; q += 256) {
      const unsigned long a = s.base + (unsigned long)q * 3ul;
      const int r = p.pixels[min(a, s.last)], g = p.pixels[min(a + 1, s.last)], bl = p.pixels[min(a + 2, s.last)];
      if (op == 6) {
        atomicAdd(&hist[768 + grey_of(r, g, bl)], 1u);
      } else {
        atomicAdd(&hist[r], 1u);
        atomicAdd(&hist[256 + g], 1u);
        atomicAdd(&hist[512 + bl], 1u);
      }
    }
  }
  __syncthreads();
  unsigned* dst = p.hist + (size_t)b * 1024;
  for (int i = tid; i < 4 * 256; i += 256)
    if (hist[i]) atomicAdd(&dst[i], hist[i]);
}

// The image's [3][256] table, by the 256 threads of a workgroup (thread = value v).  `sc` and `sc64` are 256-entry
// scratch arrays, `red` two ints.  Ends with a barrier: the table is complete for every thread.
__device__ void build_table(const RandAugParams& p, int b, int op, float a0, unsigned char* tab, unsigned* sc,
                            unsigned long long* sc64, int* red) {
  const int v = threadIdx.x;
  const unsigned* hist = p.hist + (size_t)b * 1024;
  if (op == 0 || op == 1) {
    for (int c = 0; c < 3; ++c) {
      const unsigned H = hist[c * 256 + v];
      if (v == 0) { red[0] = 256; red[1] = -1; }
      sc[v] = H;
      __syncthreads();
      if (H) { atomicMin(&red[0], v); atomicMax(&red[1], v); }
      for (int step = 1; step < 256; step <<= 1) {          // inclusive prefix sum of the bins (integers: any order)
        const unsigned add = v >= step ? sc[v - step] : 0u;
        __syncthreads();
        sc[v] += add;
        __syncthreads();
      }
      const int lo = red[0], hi = red[1];
      int out = v;
      if (op == 0) {
        if (hi > lo) {
          const float scale = 255.0f / (float)(hi - lo);
          const float off = -(float)lo * scale;
          const float prod = (float)v * scale;
          out = (int)fminf(fmaxf(prod + off, 0.f), 255.f);
        }
      } else {
        const unsigned total = sc[255];
        const unsigned last = hi >= 0 ? sc[hi] - (hi > 0 ? sc[hi - 1] : 0u) : 0u;
        const unsigned step = (total - last) / 255u;
        if (step > 0) out = v == 0 ? 0 : (int)min(255u, (sc[v] - H + step / 2u) / step);
      }
      tab[c * 256 + v] = (unsigned char)out;
      __syncthreads();
    }
    return;
  }
  int o0 = v, o1 = v, o2 = v;
  if (op == 3) {
    const int shift = 8 - min(max((int)a0, 0), 8);
    o0 = o1 = o2 = (v >> shift) << shift;
  } else if (op == 4) {
    o0 = o1 = o2 = v < (int)a0 ? v : 255 - v;
  } else if (op == 13) {
    const int add = min(max((int)a0, -255), 255);
    o0 = o1 = o2 = v < 128 ? min(max(v + add, 0), 255) : v;
  } else if (op == 7) {
    o0 = o1 = o2 = blend(0, v, a0);
  } else if (op == 6) {
    const unsigned H = hist[768 + v];
    sc[v] = H;
    sc64[v] = (unsigned long long)H * (unsigned)v;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
      if (v < step) { sc[v] += sc[v + step]; sc64[v] += sc64[v + step]; }
      __syncthreads();
    }
    const unsigned long long n = sc[0];
    const int m = n ? (int)((sc64[0] + n / 2) / n) : 0;
    o0 = o1 = o2 = blend(m, v - m, a0);
  }
  tab[v] = (unsigned char)o0; tab[256 + v] = (unsigned char)o1; tab[512 + v] = (unsigned char)o2;
  __syncthreads();
}

__global__ __launch_bounds__(256) void rand_augment_apply_kernel(const RandAugParams p) {
  const int b = blockIdx.x, tid = threadIdx.x;
  int op = p.op[b];
  if (op < 0 || op > 13) op = -1;
  const Span s = image_span(p, b);
  const float* arg = p.arg + (size_t)b * 8;
  const float a0 = arg[0];
  const unsigned char* src = p.pixels + s.base;
  unsigned char* dst = p.out + s.base;
  const long gt = (long)blockIdx.y * 256 + tid, stride = (long)gridDim.y * 256;

  if (!is_pixel_op(op)) {
    if (gt - tid >= s.nbytes) return;                       // nothing for this workgroup: skip the table
    __shared__ unsigned char tab[3 * 256];
    __shared__ unsigned sc[256];
    __shared__ unsigned long long sc64[256];
    __shared__ int red[2];
    build_table(p, b, op, a0, tab, sc, sc64, red);
    const bool wide = (((uintptr_t)src ^ (uintptr_t)dst) & 15) == 0;
    const long head = wide ? min(s.nbytes, (long)((16 - ((uintptr_t)src & 15)) & 15)) : s.nbytes;
    const long body = wide ? (s.nbytes - head) / 16 : 0;
    for (long i = gt; i < head; i += stride) dst[i] = tab[(int)(i % 3) * 256 + src[i]];
    for (long k = gt; k < body; k += stride) {
      const long i0 = head + k * 16;
      const uint4 in = *reinterpret_cast<const uint4*>(src + i0);
      const unsigned w4[4] = {in.x, in.y, in.z, in.w};
      unsigned r4[4];
      int ch = (int)(i0 % 3);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned r = 0;
#pragma unroll
        for (int k8 = 0; k8 < 4; ++k8) {
          r |= (unsigned)tab[ch * 256 + ((w4[j] >> (8 * k8)) & 255u)] << (8 * k8);
          ch = ch == 2 ? 0 : ch + 1;
        }
        r4[j] = r;
      }
      *reinterpret_cast<uint4*>(dst + i0) = make_uint4(r4[0], r4[1], r4[2], r4[3]);
    }
    for (long i = head + body * 16 + gt; i < s.nbytes; i += stride) dst[i] = tab[(int)(i % 3) * 256 + src[i]];
    return;
  }

  const float a1 = arg[1], a2 = arg[2], b0 = arg[3], b1 = arg[4], b2 = arg[5];
  const int h = s.h, w = s.w;
  auto px = [&](long y, long x, int c) -> int {             // as the front end's tap: capped before the * 3, then clamped
    const unsigned long rel = min((unsigned long)y * (unsigned long)w + (unsigned long)x, s.last);
    return p.pixels[min(s.base + rel * 3ul + (unsigned long)c, s.last)];
  };
  for (long q = gt; q < s.npix; q += stride) {
    long y, x;
    if (q <= 0x7fffffffL) { y = (unsigned)q / (unsigned)w; x = (unsigned)q - (unsigned)y * (unsigned)w; }
    else { y = q / w; x = q - y * w; }
    int o[3];
    if (op == 5) {
      const int r = px(y, x, 0), g = px(y, x, 1), bl = px(y, x, 2);
      const int gr = grey_of(r, g, bl);
      o[0] = blend(gr, r - gr, a0); o[1] = blend(gr, g - gr, a0); o[2] = blend(gr, bl - gr, a0);
    } else if (op == 8) {
      const bool interior = h >= 3 && w >= 3 && y > 0 && y < h - 1 && x > 0 && x < w - 1;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int v = px(y, x, c);
        o[c] = v;
        if (interior) {
          const int sum = px(y - 1, x - 1, c) + px(y - 1, x, c) + px(y - 1, x + 1, c) + px(y, x - 1, c) + px(y, x + 1, c) +
                          px(y + 1, x - 1, c) + px(y + 1, x, c) + px(y + 1, x + 1, c) + 5 * v;
          const int sm = sum / 13;
          o[c] = blend(sm, v - sm, a0);
        }
      }
    } else {                                                // the affine gather
      const float fx = (float)x, fy = (float)y;
      const float pxa = a0 * fx, pya = a1 * fy, pxb = b0 * fx, pyb = b1 * fy;
      const float sx = (pxa + pya) + a2, sy = (pxb + pyb) + b2;
      const float rx = floorf(sx + 0.5f), ry = floorf(sy + 0.5f);
      o[0] = o[1] = o[2] = 128;
      if (fabsf(rx) < 1073741824.f && fabsf(ry) < 1073741824.f) {       // false for NaN and infinity as well
        const int ix = (int)rx, iy = (int)ry;
        if (ix >= 0 && ix < w && iy >= 0 && iy < h) { o[0] = px(iy, ix, 0); o[1] = px(iy, ix, 1); o[2] = px(iy, ix, 2); }
      }
    }
    const long at = q * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (at + c < s.nbytes) dst[at + c] = (unsigned char)o[c];
  }
}

}  // namespace

hipError_t launch_rand_augment(const RandAugParams& p, hipStream_t st) {
  hipError_t e = hipMemsetAsync(p.hist, 0, (size_t)p.B * kRandAugHistBytes, st);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)p.B, (unsigned)p.parts);
  hipLaunchKernelGGL(rand_augment_stats_kernel, grid, dim3(256), 0, st, p);
  hipLaunchKernelGGL(rand_augment_apply_kernel, grid, dim3(256), 0, st, p);
  return hipGetLastError();
}

}  // namespace mmt
#endif  // MMT_RAND_AUGMENT_HOST_ONLY

extern "C" {

size_t mmt_rand_augment_workspace_bytes(int32_t B) { return B < 1 ? 0 : (size_t)B * mmt::kRandAugHistBytes; }

int mmt_rand_augment(int32_t B, const uint8_t* pixels, int64_t pixels_bytes, const int64_t* offsets, const int32_t* heights,
                     const int32_t* widths, const int32_t* op, const float* arg, uint8_t* out_pixels, void* workspace,
                     size_t workspace_bytes, void* stream) {
  if (B < 1) return mmt::fail(MMT_E_INVALID, "mmt_rand_augment: B (%d) must be positive", B);
  if (!pixels || !offsets || !heights || !widths || !op || !arg || !out_pixels)
    return mmt::fail(MMT_E_INVALID, "mmt_rand_augment: NULL argument (pixels, offsets, heights, widths, op, arg and out_pixels are required)");
  if (pixels_bytes < 1 || pixels_bytes >= ((int64_t)1 << 60))
    return mmt::fail(MMT_E_INVALID, "mmt_rand_augment: pixels_bytes %lld outside [1, 2^60)", (long long)pixels_bytes);
  const uintptr_t in_lo = (uintptr_t)pixels, out_lo = (uintptr_t)out_pixels;
  if (in_lo < out_lo + (uintptr_t)pixels_bytes && out_lo < in_lo + (uintptr_t)pixels_bytes)
    return mmt::fail(MMT_E_INVALID, "mmt_rand_augment: out_pixels overlaps pixels (the gather and the 3x3 window read neighbours)");
  const size_t need = mmt_rand_augment_workspace_bytes(B);
  if (!workspace || workspace_bytes < need)
    return mmt::fail(MMT_E_WORKSPACE, "mmt_rand_augment: workspace of %zu bytes needed, %zu given", need, workspace ? workspace_bytes : (size_t)0);
  if (((uintptr_t)workspace & 3) != 0)
    return mmt::fail(MMT_E_INVALID, "mmt_rand_augment: workspace must be 4-byte aligned");
  mmt::RandAugParams p;
  p.B = B;
  // Enough workgroups that the few images of a mixed plan under a slow operation (Sharpness: 27 byte loads per pixel) do
  // not set the call's time with a handful of workgroups each (256 images of 384 x 512, mixed plan: 751 us with 8 per
  // image, 346 us with 32).
  p.parts = 8192 / B < 8 ? 8 : (8192 / B > 256 ? 256 : 8192 / B);
  p.pixels = pixels; p.pixels_bytes = pixels_bytes; p.offsets = (const long*)offsets; p.heights = heights; p.widths = widths;
  p.op = op; p.arg = arg; p.out = out_pixels; p.hist = (unsigned*)workspace;
  hipError_t e = mmt::launch_rand_augment(p, (hipStream_t)stream);
  return e == hipSuccess ? MMT_OK : mmt::fail(MMT_E_LAUNCH, "mmt_rand_augment: %s", hipGetErrorString(e));
}

}  // extern "C"
