/* C driver of the PNG sanitizer build (`make asan-png`, CPU only): the host side of png_decode.hip -- the chunk walk, the
 * inflate, and stage 2 as its host loop -- under -fsanitize=address,undefined, over the fixtures of tests/golden/png
 * (argv[1]).  Every input lives in a heap block of exactly its length and every output in one of exactly the size the
 * library was told, so a read or write past either is reported.  Nothing touches a GPU. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/mmt_attn.h"
#include "../../../include/mmt_layer.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "png asan driver: %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, mmt_last_error()); return 1; } } while (0)

static long g_ok, g_refused;

static unsigned char* read_file(const char* dir, const char* name, const char* ext, long* len) {
  char path[1024];
  snprintf(path, sizeof(path), "%s/%s%s", dir, name, ext);
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "png asan driver: cannot open %s\n", path); return NULL; }
  fseek(f, 0, SEEK_END);
  *len = ftell(f);
  fseek(f, 0, SEEK_SET);
  unsigned char* buf = (unsigned char*)malloc(*len ? (size_t)*len : 1);
  if (fread(buf, 1, (size_t)*len, f) != (size_t)*len) { fclose(f); free(buf); return NULL; }
  fclose(f);
  return buf;
}

/* The three calls on `len` bytes copied into a block of exactly that size.  Returns 0 when every return code is one of
 * MMT_OK, MMT_E_INVALID and MMT_E_UNSUPPORTED (with a message).  want: the pixels a decode must give, or NULL when a
 * refusal is as good as a result. */
static int decode_once(const unsigned char* src, long len, const unsigned char* want) {
  unsigned char* bytes = (unsigned char*)malloc(len ? (size_t)len : 1);
  memcpy(bytes, src, (size_t)len);
  mmt_png_image im;
  int rc = mmt_png_info(bytes, len, &im);
  if (rc == MMT_OK) {
    CHECK(im.width >= 1 && im.height >= 1 && im.raw_bytes >= 2 && im.raw_bytes / 1032 <= len);
    uint8_t* raw = (uint8_t*)malloc((size_t)im.raw_bytes);
    uint8_t* pal = (uint8_t*)malloc(768);
    rc = mmt_png_inflate(bytes, len, &im, raw, im.raw_bytes, pal);
    if (rc == MMT_OK) {
      const int64_t n = (int64_t)im.width * im.height * 3;
      uint8_t* out = (uint8_t*)malloc((size_t)n);
      void* work = malloc((size_t)im.raw_bytes);
      CHECK(mmt_png_workspace_bytes(im.raw_bytes) == (size_t)im.raw_bytes);
      CHECK(mmt_png_pixels_host(1, &im, raw, im.raw_bytes, pal, out, n, work, (size_t)im.raw_bytes) == MMT_OK);
      if (want) CHECK(memcmp(out, want, (size_t)n) == 0);
      free(work); free(out);
      ++g_ok;
    }
    free(pal); free(raw);
  }
  free(bytes);
  if (rc != MMT_OK) {
    ++g_refused;
    CHECK(!want);
    CHECK(rc == MMT_E_INVALID || rc == MMT_E_UNSUPPORTED);
    CHECK(mmt_last_error()[0] != 0);
  }
  return 0;
}

/* Stage 2 on an inflated file with wrong metadata and filter bytes: the clamping must keep every access inside the
 * exact-size buffers. */
static int wrong_metadata(const unsigned char* bytes, long len) {
  mmt_png_image good;
  CHECK(mmt_png_info(bytes, len, &good) == MMT_OK);
  const int64_t nr = good.raw_bytes, np = (int64_t)good.width * good.height * 3;
  uint8_t* raw = (uint8_t*)malloc((size_t)nr);
  uint8_t* pal = (uint8_t*)malloc(2 * 768);
  CHECK(mmt_png_inflate(bytes, len, &good, raw, nr, pal) == MMT_OK);
  memcpy(pal + 768, pal, 768);
  uint8_t* out = (uint8_t*)malloc((size_t)np);
  void* work = malloc((size_t)nr);
  const int64_t offsets[] = {-1, -((int64_t)1 << 40), 1, 7, nr - 1, nr, nr + 12345, np - 2, (int64_t)1 << 50, INT64_MAX, INT64_MIN};
  const int32_t sizes[] = {0, -5, 1, 2, 3, 8, 1000, 65535, 1 << 30, INT32_MAX, INT32_MIN};
  const int32_t depths[] = {1, 2, 4, 8, 16, 0, -1, 3};
  const int32_t types[] = {0, 2, 3, 4, 6, -1, 99};
  for (size_t a = 0; a < sizeof(offsets) / sizeof(offsets[0]); ++a)
    for (size_t s = 0; s < sizeof(sizes) / sizeof(sizes[0]); ++s)
      for (int variant = 0; variant < 6; ++variant) {
        mmt_png_image im[2] = {good, good};
        mmt_png_image* m = &im[1];
        if (variant == 0) { m->raw_offset = offsets[a]; m->width = sizes[s]; }
        if (variant == 1) { m->pixel_offset = offsets[a]; m->height = sizes[s]; m->width = sizes[(s + 4) % 11]; }
        if (variant == 2) { m->raw_bytes = offsets[a]; m->width = sizes[s]; m->interlace = (int32_t)(a % 3); }
        if (variant == 3) { m->bit_depth = depths[(a + s) % 8]; m->color_type = types[s % 7]; m->interlace = 1; m->raw_offset = offsets[(a + 2) % 11]; }
        if (variant == 4) { m->palette_entries = sizes[s]; m->color_type = 3; m->bit_depth = depths[a % 8]; m->pixel_offset = offsets[a]; }
        if (variant == 5) { m->width = sizes[s]; m->height = sizes[(s + a) % 11]; m->color_type = types[a % 7]; m->raw_offset = offsets[a]; m->raw_bytes = offsets[(a + 5) % 11]; }
        CHECK(mmt_png_pixels_host(2, im, raw, nr, pal, out, np, work, (size_t)nr) == MMT_OK);
      }
  /* every filter-type byte from 5 to 255 counts as None: patched into the scanlines, one value per row start and beyond */
  for (int v = 5; v <= 255; ++v) {
    for (int64_t at = (v * 7) % nr, k = 0; k < 6; ++k, at = (at + nr / 5 + 1) % nr) raw[at] = (uint8_t)v;
    raw[0] = (uint8_t)v;
    CHECK(mmt_png_pixels_host(1, &good, raw, nr, pal, out, np, work, (size_t)nr) == MMT_OK);
  }
  /* argument errors */
  CHECK(mmt_png_pixels_host(0, &good, raw, nr, pal, out, np, work, (size_t)nr) == MMT_E_INVALID);
  CHECK(mmt_png_pixels_host(1, NULL, raw, nr, pal, out, np, work, (size_t)nr) == MMT_E_INVALID);
  CHECK(mmt_png_pixels_host(1, &good, raw, 0, pal, out, np, work, (size_t)nr) == MMT_E_INVALID);
  CHECK(mmt_png_pixels_host(1, &good, raw, nr, pal, out, 0, work, (size_t)nr) == MMT_E_INVALID);
  CHECK(mmt_png_pixels_host(1, &good, raw, nr, NULL, out, np, work, (size_t)nr) == MMT_E_INVALID);
  CHECK(mmt_png_pixels_host(1, &good, raw, nr, pal, out, np, work, (size_t)nr - 1) == MMT_E_WORKSPACE);
  CHECK(strstr(mmt_last_error(), "bytes needed") != NULL);
  CHECK(mmt_png_info(NULL, 4, &good) == MMT_E_INVALID);
  CHECK(mmt_png_info(bytes, -1, &good) == MMT_E_INVALID);
  CHECK(mmt_png_info(bytes, len, NULL) == MMT_E_INVALID);
  CHECK(mmt_png_inflate(bytes, len, &good, NULL, nr, pal) == MMT_E_INVALID);
  CHECK(mmt_png_inflate(bytes, len, &good, raw, nr - 1, pal) == MMT_E_INVALID);
  free(work); free(out); free(pal); free(raw);
  return 0;
}

int main(int argc, char** argv) {
  const char* dir = argc > 1 ? argv[1] : "../../tests/golden/png";
  char list[1024];
  snprintf(list, sizeof(list), "%s/fixtures.txt", dir);
  FILE* f = fopen(list, "r");
  if (!f) { fprintf(stderr, "png asan driver: cannot open %s\n", list); return 1; }
  long want_len = 0, at = 0;
  unsigned char* want = read_file(dir, "expected_pixels", ".rgb", &want_len);
  CHECK(want != NULL);
  char name[256];
  int files = 0;
  while (fgets(name, sizeof(name), f)) {
    name[strcspn(name, "\r\n")] = 0;
    if (!name[0]) continue;
    long len = 0;
    unsigned char* bytes = read_file(dir, name, ".png", &len);
    CHECK(bytes != NULL && len >= 24);
    const long n = ((long)bytes[18] << 8 | bytes[19]) * ((long)bytes[22] << 8 | bytes[23]) * 3;      /* IHDR: width, height */
    CHECK(at + n <= want_len);
    unsigned char* pixels = (unsigned char*)malloc((size_t)n);                                       /* exactly this file's */
    memcpy(pixels, want + at, (size_t)n);
    CHECK(decode_once(bytes, len, pixels) == 0);
    free(pixels); free(bytes);
    at += n;
    ++files;
  }
  fclose(f);
  free(want);
  CHECK(files > 0 && g_ok == files && at == want_len);

  /* one stored, one dynamic-Huffman Adam7, one palette file */
  const char* small[] = {"9x17_g8_f0_i0_stored", "64x3_g8_f1_i1_dynamic", "9x17_p2_f0_i0_fixed"};
  for (int i = 0; i < 3; ++i) {
    long len = 0;
    unsigned char* bytes = read_file(dir, small[i], ".png", &len);
    CHECK(bytes != NULL);
    for (long cut = 0; cut < len; ++cut) CHECK(decode_once(bytes, cut, NULL) == 0);                 /* every prefix */
    for (long b = 0; b < len; ++b) {                                                              /* every single-byte corruption */
      const unsigned char keep = bytes[b];
      const unsigned char values[4] = {0x00, 0xFF, (unsigned char)~keep, (unsigned char)(keep ^ 1)};
      for (int v = 0; v < 4; ++v) {
        bytes[b] = values[v];
        CHECK(decode_once(bytes, len, NULL) == 0);
      }
      bytes[b] = keep;
    }
    CHECK(wrong_metadata(bytes, len) == 0);
    free(bytes);
  }
  printf("png asan driver ok (%d fixtures, %ld decodes, %ld refusals)\n", files, g_ok, g_refused);
  return 0;
}
