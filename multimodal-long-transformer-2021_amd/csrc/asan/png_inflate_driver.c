/* C driver of the sanitizer build of the device inflate's host side (`make asan-png-inflate`, CPU only): mmt_png_gather
 * of png_decode.hip and mmt_png_scanlines_host of png_inflate.hip -- the functions of png_inflate.h that the kernel runs,
 * with the 256 lanes as a loop -- under -fsanitize=address,undefined, over the fixtures of tests/golden/png (argv[1]).
 * Every input lives in a heap block of exactly its length and every output in one of exactly the size the library was
 * told, so a read or write past either is reported.  The contract checked is the equivalence: the status is 0 exactly
 * when mmt_png_inflate accepts the file, and then the scanlines are the same bytes.  Nothing touches a GPU. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/mmt_attn.h"
#include "../../../include/mmt_layer.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "png inflate asan driver: %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, mmt_last_error()); return 1; } } while (0)

static long g_ok, g_refused, g_wrong;
static const int kSubseq[3] = {8, 32, 128};

static unsigned char* read_file(const char* dir, const char* name, const char* ext, long* len) {
  char path[1024];
  snprintf(path, sizeof(path), "%s/%s%s", dir, name, ext);
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "png inflate asan driver: cannot open %s\n", path); return NULL; }
  fseek(f, 0, SEEK_END);
  *len = ftell(f);
  fseek(f, 0, SEEK_SET);
  unsigned char* buf = (unsigned char*)malloc(*len ? (size_t)*len : 1);
  if (fread(buf, 1, (size_t)*len, f) != (size_t)*len) { fclose(f); free(buf); return NULL; }
  fclose(f);
  return buf;
}

/* The host inflate and, at every subseq_bytes of `subseqs`, the gather and the host variant on `len` bytes copied into a
 * block of exactly that size.  must_pass: the file is a fixture and has to be accepted. */
static int inflate_once(const unsigned char* src, long len, int must_pass, int n_subseq) {
  unsigned char* bytes = (unsigned char*)malloc(len ? (size_t)len : 1);
  memcpy(bytes, src, (size_t)len);
  mmt_png_image im;
  int rc = mmt_png_info(bytes, len, &im);
  if (rc != MMT_OK) { CHECK(!must_pass); ++g_refused; free(bytes); return 0; }
  uint8_t* want = (uint8_t*)malloc((size_t)im.raw_bytes);
  uint8_t* pal = (uint8_t*)malloc(768);
  uint8_t* pal2 = (uint8_t*)malloc(768);
  const int host = mmt_png_inflate(bytes, len, &im, want, im.raw_bytes, pal);
  CHECK(host == MMT_OK || !must_pass);
  uint8_t* comp = (uint8_t*)malloc((size_t)len);
  mmt_png_stream st = {0, 0};
  rc = mmt_png_gather(bytes, len, &im, comp, len, &st, pal2);
  if (rc != MMT_OK) {
    CHECK(host != MMT_OK);                                       /* a refusal of the gather is one of the host inflate */
    CHECK(rc == MMT_E_INVALID || rc == MMT_E_UNSUPPORTED);
    CHECK(mmt_last_error()[0] != 0);
    ++g_refused;
  } else {
    CHECK(st.comp_bytes >= 2 && st.comp_bytes <= len);
    CHECK(host != MMT_OK || memcmp(pal, pal2, 768) == 0);
    uint8_t* exact = (uint8_t*)malloc((size_t)st.comp_bytes);   /* the stream alone, so a read behind it is seen */
    memcpy(exact, comp, (size_t)st.comp_bytes);
    const size_t need = mmt_png_scanlines_workspace_bytes(1);
    void* work = malloc(need);
    for (int s = 0; s < n_subseq; ++s) {
      uint8_t* raw = (uint8_t*)malloc((size_t)im.raw_bytes);
      int32_t status = -1;
      CHECK(mmt_png_scanlines_host(1, &im, &st, exact, st.comp_bytes, raw, im.raw_bytes, &status, kSubseq[s], work, need) == MMT_OK);
      CHECK(status >= 0 && status <= MMT_PNG_ST_NO_PROGRESS);
      CHECK((status == 0) == (host == MMT_OK));
      if (host == MMT_OK) CHECK(memcmp(raw, want, (size_t)im.raw_bytes) == 0);
      free(raw);
    }
    free(work); free(exact);
    if (host == MMT_OK) ++g_ok; else ++g_refused;
  }
  free(comp); free(pal2); free(pal); free(want); free(bytes);
  return 0;
}

static uint32_t crc32_of(const unsigned char* p, long n) {
  uint32_t c = 0xFFFFFFFFu;
  for (long i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (c & 1 ? 0xEDB88320u : 0u);
  }
  return c ^ 0xFFFFFFFFu;
}

static void put_be32(unsigned char* p, uint32_t v) { p[0] = (unsigned char)(v >> 24); p[1] = (unsigned char)(v >> 16); p[2] = (unsigned char)(v >> 8); p[3] = (unsigned char)v; }

/* Every prefix and every single-byte corruption of the file's zlib stream, each wrapped again as the file's one IDAT
 * chunk with a fresh CRC-32: the chunk walk accepts them all, so the inflate decides. */
static int stream_mutations(const unsigned char* bytes, long len) {
  mmt_png_image im;
  CHECK(mmt_png_info(bytes, len, &im) == MMT_OK);
  unsigned char* stream = (unsigned char*)malloc((size_t)len);
  uint8_t pal[768];
  mmt_png_stream st = {0, 0};
  CHECK(mmt_png_gather(bytes, len, &im, stream, len, &st, pal) == MMT_OK);
  const long n = st.comp_bytes;
  long head = 8;                                                 /* the chunks in front of the first IDAT */
  while (memcmp(bytes + head + 4, "IDAT", 4) != 0) head += 12 + (long)(((uint32_t)bytes[head] << 24) | (bytes[head + 1] << 16) | (bytes[head + 2] << 8) | bytes[head + 3]);
  unsigned char* file = (unsigned char*)malloc((size_t)(head + 12 + n + 12));
  unsigned char* work = (unsigned char*)malloc((size_t)n + 1);
  for (long variant = 0; variant < n + 1 + 4 * n; ++variant) {
    long m = n;
    memcpy(work, stream, (size_t)n);
    if (variant <= n) {
      m = variant;                                               /* a prefix (the last one is the whole stream) */
    } else {
      const long at = (variant - n - 1) / 4;
      const int v = (int)((variant - n - 1) % 4);
      const unsigned char keep = work[at];
      work[at] = v == 0 ? 0x00 : (v == 1 ? 0xFF : (v == 2 ? (unsigned char)~keep : (unsigned char)(keep ^ 1)));
    }
    memcpy(file, bytes, (size_t)head);
    put_be32(file + head, (uint32_t)m);
    memcpy(file + head + 4, "IDAT", 4);
    memcpy(file + head + 8, work, (size_t)m);
    put_be32(file + head + 8 + m, crc32_of(file + head + 4, 4 + m));
    memcpy(file + head + 12 + m, "\0\0\0\0IEND\xae\x42\x60\x82", 12);
    CHECK(inflate_once(file, head + 12 + m + 12, 0, 3) == 0);
  }
  free(work); free(file); free(stream);
  return 0;
}

/* Wrong stream and image descriptors on a gathered file: the clamping must keep every access inside the exact-size
 * buffers, the call must return MMT_OK and write a status word. */
static int wrong_descriptors(const unsigned char* bytes, long len) {
  mmt_png_image good[2];
  mmt_png_stream gs[2];
  CHECK(mmt_png_info(bytes, len, &good[0]) == MMT_OK);
  good[1] = good[0];
  const int64_t nr = good[0].raw_bytes;
  good[1].raw_offset = nr;
  uint8_t* comp = (uint8_t*)malloc((size_t)(2 * len));
  uint8_t* pal = (uint8_t*)malloc(768);
  gs[0].comp_offset = 0;
  CHECK(mmt_png_gather(bytes, len, &good[0], comp, 2 * len, &gs[0], pal) == MMT_OK);
  gs[1].comp_offset = gs[0].comp_bytes;
  CHECK(mmt_png_gather(bytes, len, &good[0], comp, 2 * len, &gs[1], pal) == MMT_OK);
  const int64_t nc = gs[0].comp_bytes + gs[1].comp_bytes;
  uint8_t* exact = (uint8_t*)malloc((size_t)nc);
  memcpy(exact, comp, (size_t)nc);
  uint8_t* raw = (uint8_t*)malloc((size_t)(2 * nr));
  const size_t need = mmt_png_scanlines_workspace_bytes(2);
  void* work = malloc(need);
  const int64_t offsets[] = {-1, -((int64_t)1 << 40), 1, 7, nr - 1, nr, 2 * nr, 2 * nr + 12345, nc - 2, nc, (int64_t)1 << 50, INT64_MAX, INT64_MIN};
  const int32_t sizes[] = {0, -5, 1, 2, 3, 8, 1000, 65535, 1 << 30, INT32_MAX, INT32_MIN};
  const int32_t depths[] = {1, 2, 4, 8, 16, 0, -1, 3};
  const int32_t types[] = {0, 2, 3, 4, 6, -1, 99};
  for (size_t a = 0; a < sizeof(offsets) / sizeof(offsets[0]); ++a)
    for (size_t s = 0; s < sizeof(sizes) / sizeof(sizes[0]); ++s)
      for (int variant = 0; variant < 7; ++variant)
        for (int q = 0; q < 3; ++q) {
          mmt_png_image im[2] = {good[0], good[1]};
          mmt_png_stream st[2] = {gs[0], gs[1]};
          mmt_png_image* m = &im[(a + s) & 1];
          mmt_png_stream* t = &st[(a + variant) & 1];
          if (variant == 0) { t->comp_offset = offsets[a]; }
          if (variant == 1) { t->comp_bytes = offsets[a]; t->comp_offset = offsets[(a + s) % 13]; }
          if (variant == 2) { m->raw_offset = offsets[a]; m->width = sizes[s]; }
          if (variant == 3) { m->raw_bytes = offsets[a]; m->height = sizes[s]; m->interlace = (int32_t)(a % 3); }
          if (variant == 4) { m->width = sizes[s]; m->height = sizes[(s + a) % 11]; m->bit_depth = depths[(a + s) % 8]; m->color_type = types[s % 7]; }
          if (variant == 5) { m->raw_offset = offsets[a]; m->raw_bytes = offsets[(a + 5) % 13]; t->comp_bytes = sizes[s]; m->interlace = 1; }
          if (variant == 6) { t->comp_offset = sizes[s]; t->comp_bytes = offsets[a]; m->raw_bytes = sizes[(s + 3) % 11]; }
          int32_t status[2] = {-1, -1};
          CHECK(mmt_png_scanlines_host(2, im, st, exact, nc, raw, 2 * nr, status, kSubseq[q], work, need) == MMT_OK);
          CHECK(status[0] >= 0 && status[0] <= MMT_PNG_ST_NO_PROGRESS && status[1] >= 0 && status[1] <= MMT_PNG_ST_NO_PROGRESS);
          ++g_wrong;
        }
  /* argument errors */
  int32_t status[2];
  CHECK(mmt_png_scanlines_host(0, good, gs, exact, nc, raw, 2 * nr, status, 32, work, need) == MMT_E_INVALID);
  CHECK(mmt_png_scanlines_host(2, NULL, gs, exact, nc, raw, 2 * nr, status, 32, work, need) == MMT_E_INVALID);
  CHECK(mmt_png_scanlines_host(2, good, gs, exact, 0, raw, 2 * nr, status, 32, work, need) == MMT_E_INVALID);
  CHECK(mmt_png_scanlines_host(2, good, gs, exact, nc, raw, 0, status, 32, work, need) == MMT_E_INVALID);
  CHECK(mmt_png_scanlines_host(2, good, gs, exact, nc, raw, 2 * nr, status, 24, work, need) == MMT_E_INVALID);
  CHECK(mmt_png_scanlines_host(2, good, gs, exact, nc, raw, 2 * nr, status, 256, work, need) == MMT_E_INVALID);
  CHECK(mmt_png_scanlines_host(2, good, gs, exact, nc, raw, 2 * nr, status, 32, work, need - 1) == MMT_E_WORKSPACE);
  CHECK(strstr(mmt_last_error(), "bytes needed") != NULL);
  CHECK(mmt_png_gather(bytes, len, &good[0], comp, gs[0].comp_bytes - 1, &gs[0], pal) == MMT_E_INVALID);
  CHECK(mmt_png_gather(bytes, len, &good[0], NULL, 2 * len, &gs[0], pal) == MMT_E_INVALID);
  CHECK(mmt_png_gather(NULL, len, &good[0], comp, 2 * len, &gs[0], pal) == MMT_E_INVALID);
  free(work); free(raw); free(exact); free(pal); free(comp);
  return 0;
}

int main(int argc, char** argv) {
  const char* dir = argc > 1 ? argv[1] : "../../tests/golden/png";
  char list[1024];
  snprintf(list, sizeof(list), "%s/fixtures.txt", dir);
  FILE* f = fopen(list, "r");
  if (!f) { fprintf(stderr, "png inflate asan driver: cannot open %s\n", list); return 1; }
  char name[256];
  int files = 0;
  while (fgets(name, sizeof(name), f)) {
    name[strcspn(name, "\r\n")] = 0;
    if (!name[0]) continue;
    long len = 0;
    unsigned char* bytes = read_file(dir, name, ".png", &len);
    CHECK(bytes != NULL && len >= 24);
    CHECK(inflate_once(bytes, len, 1, 3) == 0);
    free(bytes);
    ++files;
  }
  fclose(f);
  CHECK(files > 0 && g_ok == files && g_refused == 0);

  /* one stored, one dynamic-Huffman Adam7, one palette file */
  const char* small[] = {"9x17_g8_f0_i0_stored", "64x3_g8_f1_i1_dynamic", "9x17_p2_f0_i0_fixed"};
  for (int i = 0; i < 3; ++i) {
    long len = 0;
    unsigned char* bytes = read_file(dir, small[i], ".png", &len);
    CHECK(bytes != NULL);
    for (long cut = 0; cut < len; ++cut) CHECK(inflate_once(bytes, cut, 0, 3) == 0);              /* every prefix */
    for (long b = 0; b < len; ++b) {                                                            /* every single-byte corruption */
      const unsigned char keep = bytes[b];
      const unsigned char values[4] = {0x00, 0xFF, (unsigned char)~keep, (unsigned char)(keep ^ 1)};
      for (int v = 0; v < 4; ++v) {
        bytes[b] = values[v];
        CHECK(inflate_once(bytes, len, 0, 3) == 0);
      }
      bytes[b] = keep;
    }
    CHECK(stream_mutations(bytes, len) == 0);
    CHECK(wrong_descriptors(bytes, len) == 0);
    free(bytes);
  }
  printf("png inflate asan driver ok (%d fixtures, %ld accepted, %ld refused, %ld wrong descriptors)\n", files, g_ok, g_refused, g_wrong);
  return 0;
}
