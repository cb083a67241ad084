// Image front end of the data layer (C ABI: include/mmt_layer.h, mmt_image_patches): decoded uint8 RGB images of
// mixed sizes -> patch features, the tensor half of `decode_fn` (src/data/data_utils.py:195-222) in one launch.
//
//   x  = u8 / 255                                         tf.io.decode_image(dtype=float32)              (:195-197)
//   r  = resize_bilinear(x, [image_size, image_size])     tf.image.resize, TF2 defaults: half-pixel centres,
//                                                         no antialiasing, 2x2 taps                       (:205, :207)
//   unnormalised = r,  normalised = (r - MEAN) / MEAN     the reference's literal line 204 divides by the MEAN, not
//                                                         by a standard deviation; kept as it is
//   flip: both outputs take column image_size - 1 - x                                                     (:209-211)
//   patches: P = image_size / patch_size (VALID), raster order, (row, column, channel) inside a patch     (:147-180)
//   label id: per-channel mean of the unnormalised patch * 255 -> 2^bits equal bins, channel 0 the least
//             significant digit                                                                           (:448-481)
//
// The reference normalises before it resizes; the map is affine per channel and the four tap weights sum to 1, so
// resizing once and normalising afterwards is the same function up to rounding.
//
// One wave per output patch, four patches per workgroup.  Lane l computes elements l, l + 64, ... of the patch
// vector, so a wave's stores are contiguous; the 2x2 taps are gathered from the uint8 source (a patch's taps span a
// few source rows, which the L2 serves).  The three channel sums of the label id go through the fixed-order wave
// butterfly (layer_common.h: wave_sum) -- no atomics, ids are bitwise reproducible.
//
// Bounds: taps are clamped to the image, h / w below 1 count as 1, the image's offset is clamped into the pixel
// buffer and every byte address to pixels_bytes - 1.  Bad metadata reads wrong pixels of the caller's buffer and
// never anything outside it.
#include "../../include/mmt_attn.h"
#include "../../include/mmt_layer.h"

#include <cmath>

#include "layer_common.h"
#include "mmt_err.h"

namespace mmt {

struct ImagePatchParams {
  long n_patches;          // B * P * P
  int image_size, patch_size, P, E;      // E = patch_size^2 * 3
  int bits;                // channel_bits; 0: no ids
  float mean[3];
  const unsigned char* pixels;
  long pixels_bytes;
  const long* offsets;
  const int *heights, *widths;
  const unsigned char* flip;
  void* norm;              // [n_patches, E] T
  float* unnorm;           // [n_patches, E] or NULL
  int* ids;                // [n_patches] or NULL
};

// Source taps of destination index d on an axis of `in` source samples (tf.image.resize, half-pixel centres):
//   src = (d + 0.5) * in / out - 0.5,  lo = max(floor(src), 0),  hi = min(ceil(src), in - 1),  t = src - floor(src).
// The coordinate is formed in fp64 (`scale` = in / out) so that t carries one fp32 rounding only: in fp32 the
// product loses |src| * 2^-24, which times a full-range pixel step would be most of the 1e-5 the output is held to.
__device__ __forceinline__ void resize_taps(int d, double scale, int in, int& lo, int& hi, float& t) {
  const double src = ((double)d + 0.5) * scale - 0.5;
  const double fl = floor(src);
  t = (float)(src - fl);
  lo = (int)fmax(fl, 0.0);
  hi = (int)fmin(ceil(src), (double)(in - 1));
}

template <typename T>
__global__ __launch_bounds__(256) void image_patches_kernel(const ImagePatchParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long patch = (long)blockIdx.x * 4 + wave;
  if (patch >= p.n_patches) return;                      // whole waves leave: the butterfly below sees full waves
  const int PP = p.P * p.P;
  const int b = (int)(patch / PP), pi = (int)(patch - (long)b * PP);
  const int pr = pi / p.P, pc = pi - pr * p.P;
  const int h = max(p.heights[b], 1), w = max(p.widths[b], 1);
  const unsigned long last = (unsigned long)(p.pixels_bytes - 1);
  const unsigned long base = (unsigned long)min(max(p.offsets[b], 0L), p.pixels_bytes - 1);
  const bool flip = p.flip != nullptr && p.flip[b] != 0;
  const double sy = (double)h / (double)p.image_size, sx = (double)w / (double)p.image_size;
  const bool want_ids = p.ids != nullptr && p.bits > 0;
  const unsigned row_elems = (unsigned)p.patch_size * 3u;
  T* norm = reinterpret_cast<T*>(p.norm) + patch * p.E;
  float* unnorm = p.unnorm ? p.unnorm + patch * p.E : nullptr;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int e = lane; e < p.E; e += 64) {
    const unsigned r = (unsigned)e / row_elems, rem = (unsigned)e - r * row_elems;
    const unsigned c = rem / 3u, ch = rem - c * 3u;
    const int y = pr * p.patch_size + (int)r;
    int x = pc * p.patch_size + (int)c;
    if (flip) x = p.image_size - 1 - x;
    int y0, y1, x0, x1;
    float ty, tx;
    resize_taps(y, sy, h, y0, y1, ty);
    resize_taps(x, sx, w, x0, x1, tx);
    // byte of pixel (yy, xx): base + (yy * w + xx) * 3 + ch.  yy * w + xx < 2^62; it is capped below pixels_bytes
    // (< 2^60, checked by the host) before the * 3, so nothing wraps, and the sum is clamped to the last byte.
    auto tap = [&](int yy, int xx) -> float {
      unsigned long rel = (unsigned long)yy * (unsigned long)w + (unsigned long)xx;
      rel = min(rel, last);
      const unsigned long addr = min(base + rel * 3ul + ch, last);
      return (float)p.pixels[addr] / 255.f;
    };
    const float tl = tap(y0, x0), tr = tap(y0, x1), bl = tap(y1, x0), br = tap(y1, x1);
    const float top = tl + (tr - tl) * tx;               // horizontal first, then vertical (TF's compute_lerp)
    const float bot = bl + (br - bl) * tx;
    const float v = top + (bot - top) * ty;
    const float m = ch == 0 ? p.mean[0] : (ch == 1 ? p.mean[1] : p.mean[2]);
    norm[e] = (T)((v - m) / m);
    if (unnorm) unnorm[e] = v;
    if (want_ids) {
      const float s = v * 255.f;
      if (ch == 0) s0 += s; else if (ch == 1) s1 += s; else s2 += s;
    }
  }
  if (want_ids) {
    const int nbins = 1 << p.bits;
    const float inv = 1.f / ((float)(p.patch_size * p.patch_size) * (float)(256 >> p.bits));
    const int d0 = min((int)(wave_sum(s0) * inv), nbins - 1);
    const int d1 = min((int)(wave_sum(s1) * inv), nbins - 1);
    const int d2 = min((int)(wave_sum(s2) * inv), nbins - 1);
    if (lane == 0) p.ids[patch] = d0 | (d1 << p.bits) | (d2 << (2 * p.bits));
  }
}

}  // namespace mmt

extern "C" {

int mmt_image_patches(const mmt_image_desc* d, const uint8_t* pixels, int64_t pixels_bytes, const int64_t* offsets,
                      const int32_t* heights, const int32_t* widths, const uint8_t* flip, void* normalised_out,
                      float* unnormalised_out, int32_t* label_ids_out, void* stream) {
  if (!d) return mmt::fail(MMT_E_INVALID, "mmt_image_patches: desc is NULL");
  if (!pixels || !offsets || !heights || !widths || !normalised_out)
    return mmt::fail(MMT_E_INVALID, "mmt_image_patches: NULL argument (pixels, offsets, heights, widths and normalised_out are required)");
  if (pixels_bytes <= 0 || pixels_bytes >= ((int64_t)1 << 60))
    return mmt::fail(MMT_E_INVALID, "mmt_image_patches: pixels_bytes %lld outside [1, 2^60)", (long long)pixels_bytes);
  if (d->B <= 0 || d->image_size <= 0 || d->patch_size <= 0)
    return mmt::fail(MMT_E_INVALID, "mmt_image_patches: B (%d), image_size (%d) and patch_size (%d) must be positive",
                     d->B, d->image_size, d->patch_size);
  if (d->patch_size > d->image_size)
    return mmt::fail(MMT_E_INVALID, "mmt_image_patches: patch_size %d exceeds image_size %d (no whole patch)",
                     d->patch_size, d->image_size);
  if (d->out_dtype != MMT_F32 && d->out_dtype != MMT_BF16)
    return mmt::fail(MMT_E_INVALID, "mmt_image_patches: bad out_dtype %d", d->out_dtype);
  if (d->channel_bits < 0 || d->channel_bits > 8)
    return mmt::fail(MMT_E_INVALID, "mmt_image_patches: channel_bits %d outside [0,8]", d->channel_bits);
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(d->mean[i]) || d->mean[i] == 0.f)
      return mmt::fail(MMT_E_INVALID, "mmt_image_patches: mean[%d] must be finite and non-zero (it divides)", i);
  // every product below is of two factors under 2^31, so int64 holds it before it is compared
  const int64_t P = d->image_size / d->patch_size, PP = P * P;
  const int64_t area = (int64_t)d->patch_size * d->patch_size;
  if (area > INT32_MAX / 3)
    return mmt::fail(MMT_E_INVALID, "mmt_image_patches: patch_size %d: more than 2^31 - 1 values per patch", d->patch_size);
  if (PP > INT32_MAX || (int64_t)d->B * PP > INT32_MAX)
    return mmt::fail(MMT_E_INVALID, "mmt_image_patches: B * P * P (%d * %lld * %lld) beyond the 2^31 - 1 patches the grid arithmetic holds",
                     d->B, (long long)P, (long long)P);
  const int64_t E = area * 3, n_patches = (int64_t)d->B * PP;
  mmt::ImagePatchParams p;
  p.n_patches = n_patches; p.image_size = d->image_size; p.patch_size = d->patch_size; p.P = (int)P; p.E = (int)E;
  p.bits = label_ids_out ? d->channel_bits : 0;
  for (int i = 0; i < 3; ++i) p.mean[i] = d->mean[i];
  p.pixels = pixels; p.pixels_bytes = pixels_bytes; p.offsets = (const long*)offsets; p.heights = heights; p.widths = widths;
  p.flip = flip; p.norm = normalised_out; p.unnorm = unnormalised_out; p.ids = p.bits > 0 ? label_ids_out : nullptr;
  const dim3 grid((unsigned)((n_patches + 3) / 4));
  hipStream_t st = (hipStream_t)stream;
  if (d->out_dtype == MMT_BF16) hipLaunchKernelGGL((mmt::image_patches_kernel<__bf16>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((mmt::image_patches_kernel<float>), grid, dim3(256), 0, st, p);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? MMT_OK : mmt::fail(MMT_E_LAUNCH, "mmt_image_patches: %s", hipGetErrorString(e));
}

}  // extern "C"
