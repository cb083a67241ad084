// Launch parameters of the RandAugment kernels (rand_augment.hip), shared with the host-only stand-in of the sanitizer
// build (asan/asan_stubs.cpp).
#pragma once
#include <hip/hip_runtime.h>

namespace mmt {

constexpr int kRandAugChunk = 4096;                  // pixels one workgroup of the statistics pass takes per step
constexpr size_t kRandAugHistBytes = 4 * 256 * 4;    // per image: R, G, B and grey histograms, 256 uint32 bins each

struct RandAugParams {
  int B;
  int parts;               // workgroups per image (grid.y) of both passes
  const unsigned char* pixels;
  long pixels_bytes;
  const long* offsets;
  const int *heights, *widths, *op;
  const float* arg;        // [B, 8]
  unsigned char* out;
  unsigned* hist;          // [B, 4, 256] in the caller's workspace
};

// Clears the histograms, then the statistics pass and the apply pass, all on `st`.
hipError_t launch_rand_augment(const RandAugParams& p, hipStream_t st);

}  // namespace mmt
