/* C driver of the JPEG sanitizer build (`make asan-jpeg`, CPU only): the host side of jpeg_decode.hip -- marker parsing,
 * Huffman decoding, and stage 2 as its host loop -- under -fsanitize=address,undefined, over the fixtures of
 * tests/golden/jpeg (argv[1]).  Every input lives in a heap block of exactly its length and every output in one of
 * exactly the size the library was told, so a read or write past either is reported.  Nothing touches a GPU. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/mmt_attn.h"
#include "../../../include/mmt_layer.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "jpeg asan driver: %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, mmt_last_error()); return 1; } } while (0)
#define MAX_COEF ((int64_t)1 << 22)     /* a corrupted header may claim 65535 x 65535: such a file is parsed, not decoded */

static long g_ok, g_refused, g_skipped;

static unsigned char* read_file(const char* dir, const char* name, const char* ext, long* len) {
  char path[1024];
  snprintf(path, sizeof(path), "%s/%s%s", dir, name, ext);
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "jpeg asan driver: cannot open %s\n", path); return NULL; }
  fseek(f, 0, SEEK_END);
  *len = ftell(f);
  fseek(f, 0, SEEK_SET);
  unsigned char* buf = (unsigned char*)malloc(*len ? (size_t)*len : 1);
  if (fread(buf, 1, (size_t)*len, f) != (size_t)*len) { fclose(f); free(buf); return NULL; }
  fclose(f);
  return buf;
}

/* The three calls on `len` bytes copied into a block of exactly that size.  Returns 0 when every return code is one of
 * MMT_OK, MMT_E_INVALID and MMT_E_UNSUPPORTED (with a message); must_decode: MMT_OK is required throughout. */
static int decode_once(const unsigned char* src, long len, int must_decode) {
  unsigned char* bytes = (unsigned char*)malloc(len ? (size_t)len : 1);
  memcpy(bytes, src, (size_t)len);
  mmt_jpeg_image im;
  int rc = mmt_jpeg_info(bytes, len, &im);
  if (rc == MMT_OK && im.coef_elems > MAX_COEF) { ++g_skipped; free(bytes); CHECK(!must_decode); return 0; }
  if (rc == MMT_OK) {
    CHECK(im.coef_elems >= 64 && im.coef_elems % 64 == 0 && im.width >= 1 && im.height >= 1);
    int16_t* coef = (int16_t*)aligned_alloc(16, (size_t)im.coef_elems * 2);
    uint16_t* q = (uint16_t*)aligned_alloc(16, 3 * 64 * 2);
    rc = mmt_jpeg_coefficients(bytes, len, &im, coef, im.coef_elems, q);
    if (rc == MMT_OK) {
      const int64_t n = (int64_t)im.width * im.height * 3;
      uint8_t* out = (uint8_t*)malloc((size_t)n);
      void* work = aligned_alloc(16, (size_t)im.coef_elems);
      CHECK(mmt_jpeg_workspace_bytes(im.coef_elems) == (size_t)im.coef_elems);
      CHECK(mmt_jpeg_pixels_host(1, &im, coef, im.coef_elems, q, out, n, work, (size_t)im.coef_elems) == MMT_OK);
      free(work); free(out);
      ++g_ok;
    }
    free(q); free(coef);
  }
  free(bytes);
  if (rc != MMT_OK) {
    ++g_refused;
    CHECK(!must_decode);
    CHECK(rc == MMT_E_INVALID || rc == MMT_E_UNSUPPORTED);
    CHECK(mmt_last_error()[0] != 0);
  }
  return 0;
}

/* Stage 2 on a decoded file with wrong metadata: the clamping must keep every access inside the exact-size buffers. */
static int wrong_metadata(const unsigned char* bytes, long len) {
  mmt_jpeg_image good;
  CHECK(mmt_jpeg_info(bytes, len, &good) == MMT_OK);
  const int64_t ne = good.coef_elems, np = (int64_t)good.width * good.height * 3;
  int16_t* coef = (int16_t*)aligned_alloc(16, (size_t)ne * 2);
  uint16_t* q = (uint16_t*)aligned_alloc(16, 2 * 3 * 64 * 2);
  CHECK(mmt_jpeg_coefficients(bytes, len, &good, coef, ne, q) == MMT_OK);
  memcpy(q + 192, q, 192 * 2);
  uint8_t* out = (uint8_t*)malloc((size_t)np);
  void* work = aligned_alloc(16, (size_t)ne);
  const int64_t offsets[] = {-1, -((int64_t)1 << 40), 1, 7, ne - 64, ne - 1, ne, ne + 12345, (int64_t)1 << 50, INT64_MAX, INT64_MIN};
  const int32_t sizes[] = {0, -5, 1, 2, 3, 1000, 65535, 1 << 30, INT32_MAX, INT32_MIN};
  for (size_t a = 0; a < sizeof(offsets) / sizeof(offsets[0]); ++a)
    for (size_t s = 0; s < sizeof(sizes) / sizeof(sizes[0]); ++s)
      for (int variant = 0; variant < 6; ++variant) {
        mmt_jpeg_image im[2] = {good, good};
        mmt_jpeg_image* m = &im[1];
        if (variant == 0) { m->coef_offset[0] = offsets[a]; m->coef_offset[2] = offsets[(a + 3) % 11]; m->blocks_w[1] = sizes[s]; }
        if (variant == 1) { m->pixel_offset = offsets[a]; m->width = sizes[s]; }
        if (variant == 2) { m->pixel_offset = offsets[a]; m->height = sizes[s]; m->width = sizes[(s + 4) % 10]; }
        if (variant == 3) { for (int c = 0; c < 3; ++c) { m->blocks_w[c] = sizes[s]; m->blocks_h[c] = sizes[(s + a) % 10]; m->coef_offset[c] = offsets[(a + c) % 11]; } }
        if (variant == 4) { m->components = sizes[s]; m->h_samp[0] = 2; m->v_samp[0] = 2; m->coef_offset[1] = offsets[a]; }
        if (variant == 5) { m->components = 3; m->h_samp[0] = 2; m->v_samp[0] = (int)(a % 3); m->blocks_h[0] = sizes[s]; m->blocks_w[2] = 1; m->coef_offset[1] = offsets[a]; }
        CHECK(mmt_jpeg_pixels_host(2, im, coef, ne, q, out, np, work, (size_t)ne) == MMT_OK);
      }
  /* argument errors */
  CHECK(mmt_jpeg_pixels_host(0, &good, coef, ne, q, out, np, work, (size_t)ne) == MMT_E_INVALID);
  CHECK(mmt_jpeg_pixels_host(1, NULL, coef, ne, q, out, np, work, (size_t)ne) == MMT_E_INVALID);
  CHECK(mmt_jpeg_pixels_host(1, &good, coef, 63, q, out, np, work, (size_t)ne) == MMT_E_INVALID);
  CHECK(mmt_jpeg_pixels_host(1, &good, coef, ne, q, out, 0, work, (size_t)ne) == MMT_E_INVALID);
  CHECK(mmt_jpeg_pixels_host(1, &good, coef + 1, ne, q, out, np, work, (size_t)ne) == MMT_E_INVALID);
  CHECK(mmt_jpeg_pixels_host(1, &good, coef, ne, q, out, np, work, (size_t)ne - 1) == MMT_E_WORKSPACE);
  CHECK(strstr(mmt_last_error(), "bytes needed") != NULL);
  CHECK(mmt_jpeg_info(NULL, 4, &good) == MMT_E_INVALID);
  CHECK(mmt_jpeg_info(bytes, -1, &good) == MMT_E_INVALID);
  CHECK(mmt_jpeg_info(bytes, len, NULL) == MMT_E_INVALID);
  CHECK(mmt_jpeg_coefficients(bytes, len, &good, NULL, ne, q) == MMT_E_INVALID);
  free(work); free(out); free(q); free(coef);
  return 0;
}

int main(int argc, char** argv) {
  const char* dir = argc > 1 ? argv[1] : "../../tests/golden/jpeg";
  char list[1024];
  snprintf(list, sizeof(list), "%s/fixtures.txt", dir);
  FILE* f = fopen(list, "r");
  if (!f) { fprintf(stderr, "jpeg asan driver: cannot open %s\n", list); return 1; }
  char name[256];
  int files = 0;
  while (fgets(name, sizeof(name), f)) {
    name[strcspn(name, "\r\n")] = 0;
    if (!name[0]) continue;
    long len = 0;
    unsigned char* bytes = read_file(dir, name, ".jpg", &len);
    CHECK(bytes != NULL);
    CHECK(decode_once(bytes, len, 1) == 0);
    free(bytes);
    ++files;
  }
  fclose(f);
  CHECK(files > 0 && g_ok == files);

  const char* refusals[] = {"refuse_progressive.jpg", "refuse_cmyk.jpg", "refuse_arithmetic.jpg", "refuse_signature.png"};
  for (int i = 0; i < 4; ++i) {
    long len = 0;
    unsigned char* bytes = read_file(dir, refusals[i], "", &len);
    CHECK(bytes != NULL);
    mmt_jpeg_image im;
    CHECK(mmt_jpeg_info(bytes, len, &im) == MMT_E_UNSUPPORTED && mmt_last_error()[0] != 0);
    free(bytes);
  }

  const char* small[] = {"17x9_420_q30_rst1", "9x3_444_q90", "16x16_grey_q80"};
  for (int i = 0; i < 3; ++i) {
    long len = 0;
    unsigned char* bytes = read_file(dir, small[i], ".jpg", &len);
    CHECK(bytes != NULL);
    for (long cut = 0; cut < len; ++cut) CHECK(decode_once(bytes, cut, 0) == 0);             /* every prefix */
    for (long at = 0; at < len && at < 700; ++at) {                                           /* every single-byte corruption */
      const unsigned char keep = bytes[at];
      const unsigned char values[3] = {0x00, 0xFF, (unsigned char)~keep};
      for (int v = 0; v < 3; ++v) {
        bytes[at] = values[v];
        CHECK(decode_once(bytes, len, 0) == 0);
      }
      bytes[at] = keep;
    }
    CHECK(wrong_metadata(bytes, len) == 0);
    free(bytes);
  }
  printf("jpeg asan driver ok (%d fixtures, %ld decodes, %ld refusals, %ld oversize headers skipped)\n", files, g_ok, g_refused, g_skipped);
  return 0;
}
