// PNG inflate on the device (C ABI: include/mmt_layer.h, mmt_png_scanlines*): the IDAT stream of every image of a batch
// inflated by one workgroup of 256 threads, in front of mmt_png_pixels and in place of the host's mmt_png_inflate.
// DESIGN.md section 4 "PNG inflate on the device" has the method (self-synchronising speculative Huffman decoding,
// Weissenberger and Schmidt 2018; multi-round resolution of the LZ77 copies, Sitaridi et al. 2016), the bounds, the
// statuses and the readings.
//
//   host    mmt_png_gather (png_decode.hip): the chunk walk, the IDAT payloads back to back, the zlib header, the palette.
//   device  one kernel, grid (images), 256 threads: rounds of stage / block header / speculative walk / offsets / write /
//           advance over the stream, then the Adler-32, the exact length and the filter-type bytes.  The output in global
//           memory is the LZ77 window; writes of a round are made visible by __syncthreads() before a lane reads them.
//           The group's whole state (the staged bytes, two Huffman tables, the lanes' exits and cursors) is LDS.
//   mmt_png_scanlines_host runs inf_image() of png_inflate.h -- the same text -- with the 256 lanes as a loop.
//
// Bounds: inf_view() clamps the stream and the scanlines of an image into comp and raw_out; inf_image() reads and
// writes only through those two ranges.
#include "../../include/mmt_attn.h"
#include "../../include/mmt_layer.h"

#include <cstdint>
#include <cstring>

#include "mmt_err.h"
#include "png_inflate.h"

namespace mmt {
namespace {

struct InfParams {
  int B;
  const mmt_png_image* images;
  const mmt_png_stream* streams;
  const unsigned char* comp;
  long comp_bytes;
  unsigned char* raw;
  long raw_bytes;
  int* status;
  int subseq;
};

struct InfView {
  const unsigned char* comp;
  long comp_n;
  unsigned char* out;
  long cap, want;
  PngGeom geom;
};

// Image b, clamped: [comp, comp + comp_n) inside the call's comp, [out, out + cap) inside the call's raw_out.
__host__ __device__ inline InfView inf_view(const InfParams& p, int b) {
  InfView v;
  const long off = pclampl(p.streams[b].comp_offset, 0, p.comp_bytes);
  v.comp = p.comp + off;
  v.comp_n = pclampl(p.streams[b].comp_bytes, 0, p.comp_bytes - off);
  v.geom = png_geom(p.images[b], p.raw_bytes, (long)1 << 62);
  v.out = p.raw + v.geom.raw;
  v.cap = v.geom.raw_end - v.geom.raw;
  v.want = p.images[b].raw_bytes;
  return v;
}

__host__ __device__ inline int inf_one(InfGroup& g, const InfParams& p, int b) {
  const InfView v = inf_view(p, b);
  int st = inf_image(g, v.comp, v.comp_n, v.out, v.cap, v.want, p.subseq);
  if (!st) st = inf_filter_bytes(g, p.raw, v.geom);
  return st;
}

int check_scanlines(const char* who, int32_t B, const mmt_png_image* images, const mmt_png_stream* streams, const uint8_t* comp,
                    int64_t comp_bytes, uint8_t* raw_out, int64_t raw_bytes, int32_t* status_out, int32_t subseq_bytes, void* workspace,
                    size_t workspace_bytes) {
  if (B < 1) return fail(MMT_E_INVALID, "%s: B (%d) must be positive", who, B);
  if (!images || !streams || !comp || !raw_out || !status_out)
    return fail(MMT_E_INVALID, "%s: NULL argument (images, streams, comp, raw_out and status_out are required)", who);
  if (comp_bytes < 1 || comp_bytes >= ((int64_t)1 << 60)) return fail(MMT_E_INVALID, "%s: comp_bytes %lld outside [1, 2^60)", who, (long long)comp_bytes);
  if (raw_bytes < 1 || raw_bytes >= ((int64_t)1 << 60)) return fail(MMT_E_INVALID, "%s: raw_bytes %lld outside [1, 2^60)", who, (long long)raw_bytes);
  if (subseq_bytes < kInfMinSubseq || subseq_bytes > kInfMaxSubseq || (subseq_bytes & (subseq_bytes - 1)))
    return fail(MMT_E_INVALID, "%s: subseq_bytes %d is not a power of two in [%d, %d]", who, subseq_bytes, kInfMinSubseq, kInfMaxSubseq);
  const size_t need = mmt_png_scanlines_workspace_bytes(B);
  if (!workspace || workspace_bytes < need)
    return fail(MMT_E_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", who, need, workspace ? workspace_bytes : (size_t)0);
  return MMT_OK;
}

InfParams make_params(int32_t B, const mmt_png_image* images, const mmt_png_stream* streams, const uint8_t* comp, int64_t comp_bytes,
                      uint8_t* raw_out, int64_t raw_bytes, int32_t* status_out, int32_t subseq_bytes) {
  InfParams p;
  p.B = B; p.images = images; p.streams = streams; p.comp = comp; p.comp_bytes = comp_bytes; p.raw = raw_out; p.raw_bytes = raw_bytes;
  p.status = status_out; p.subseq = subseq_bytes;
  return p;
}

}  // namespace

#ifndef MMT_PNG_HOST_ONLY
namespace {

__global__ __launch_bounds__(kInfLanes) void png_inflate_kernel(const InfParams p) {
  __shared__ InfGroup g;
  const int b = blockIdx.x;
  const int st = inf_one(g, p, b);
  if (threadIdx.x == 0) p.status[b] = st;
}

}  // namespace
#endif  // MMT_PNG_HOST_ONLY

}  // namespace mmt

extern "C" {

size_t mmt_png_scanlines_workspace_bytes(int32_t B) { return B < 1 ? 0 : sizeof(mmt::InfGroup) + 64; }

int mmt_png_scanlines_host(int32_t B, const mmt_png_image* images, const mmt_png_stream* streams, const uint8_t* comp, int64_t comp_bytes,
                           uint8_t* raw_out, int64_t raw_bytes, int32_t* status_out, int32_t subseq_bytes, void* workspace,
                           size_t workspace_bytes) {
  const int rc = mmt::check_scanlines("mmt_png_scanlines_host", B, images, streams, comp, comp_bytes, raw_out, raw_bytes, status_out, subseq_bytes,
                                      workspace, workspace_bytes);
  if (rc) return rc;
  const mmt::InfParams p = mmt::make_params(B, images, streams, comp, comp_bytes, raw_out, raw_bytes, status_out, subseq_bytes);
  mmt::InfGroup* g = (mmt::InfGroup*)(((uintptr_t)workspace + 63) & ~(uintptr_t)63);
  for (int b = 0; b < B; ++b) status_out[b] = mmt::inf_one(*g, p, b);
  return MMT_OK;
}

#ifndef MMT_PNG_HOST_ONLY
int mmt_png_scanlines(int32_t B, const mmt_png_image* images, const mmt_png_stream* streams, const uint8_t* comp, int64_t comp_bytes,
                      uint8_t* raw_out, int64_t raw_bytes, int32_t* status_out, int32_t subseq_bytes, void* workspace, size_t workspace_bytes,
                      void* stream) {
  const int rc = mmt::check_scanlines("mmt_png_scanlines", B, images, streams, comp, comp_bytes, raw_out, raw_bytes, status_out, subseq_bytes,
                                      workspace, workspace_bytes);
  if (rc) return rc;
  const mmt::InfParams p = mmt::make_params(B, images, streams, comp, comp_bytes, raw_out, raw_bytes, status_out, subseq_bytes);
  hipLaunchKernelGGL(mmt::png_inflate_kernel, dim3((unsigned)B), dim3(mmt::kInfLanes), 0, (hipStream_t)stream, p);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MMT_OK : mmt::fail(MMT_E_LAUNCH, "mmt_png_scanlines: %s", hipGetErrorString(e));
}
#endif

}  // extern "C"
