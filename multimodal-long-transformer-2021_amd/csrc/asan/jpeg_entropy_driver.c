/* C driver of the sanitizer build of the device entropy decode's host side (`make asan-jpeg-entropy`, CPU only):
 * mmt_jpeg_scan_plan and mmt_jpeg_entropy_host -- the functions of jpeg_entropy.h that the kernels run, as plain loops --
 * under -fsanitize=address,undefined, over the fixtures of tests/golden/jpeg (argv[1]).  Every input lives in a heap
 * block of exactly its length and every output in one of exactly the size the library was told, so a read or write past
 * either is reported.  Nothing touches a GPU. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/mmt_attn.h"
#include "../../../include/mmt_layer.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "jpeg entropy asan driver: %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, mmt_last_error()); return 1; } } while (0)
#define MAX_COEF ((int64_t)1 << 22)     /* a corrupted header may claim 65535 x 65535: such a file is parsed, not decoded */

static long g_exact, g_status, g_refused, g_skipped, g_wrong;

static void* block(size_t n) {          /* exactly n bytes, 16-byte aligned */
  void* p = NULL;
  if (posix_memalign(&p, 16, n ? n : 1) != 0) abort();
  return p;
}

static unsigned char* read_file(const char* dir, const char* name, const char* ext, long* len) {
  char path[1024];
  snprintf(path, sizeof(path), "%s/%s%s", dir, name, ext);
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "jpeg entropy asan driver: cannot open %s\n", path); return NULL; }
  fseek(f, 0, SEEK_END);
  *len = ftell(f);
  fseek(f, 0, SEEK_SET);
  unsigned char* buf = (unsigned char*)malloc(*len ? (size_t)*len : 1);
  if (fread(buf, 1, (size_t)*len, f) != (size_t)*len) { fclose(f); free(buf); return NULL; }
  fclose(f);
  return buf;
}

/* One image's plan in exact-size blocks. */
typedef struct plan {
  mmt_jpeg_scan scan;
  uint32_t* huff;
  uint16_t* q;
  int32_t* seg;
  int32_t* sub;
} plan;

static void plan_free(plan* p) { free(p->huff); free(p->q); free(p->seg); free(p->sub); }

/* Returns the plan call's code; on MMT_OK the blocks are filled. */
static int plan_make(const unsigned char* bytes, long len, const mmt_jpeg_image* im, int sb, plan* p) {
  memset(p, 0, sizeof(*p));
  int rc = mmt_jpeg_scan_plan(bytes, len, im, sb, &p->scan, NULL, NULL, NULL, 0, NULL, 0);
  if (rc != MMT_OK) return rc;
  p->huff = (uint32_t*)block(6 * MMT_JPEG_HUFF_WORDS * 4);
  p->q = (uint16_t*)block(3 * 64 * 2);
  p->seg = (int32_t*)block((size_t)p->scan.n_segments * 16);
  p->sub = (int32_t*)block((size_t)p->scan.n_subseq * 4);
  rc = mmt_jpeg_scan_plan(bytes, len, im, sb, &p->scan, p->huff, p->q, p->seg, p->scan.n_segments, p->sub, p->scan.n_subseq);
  if (rc != MMT_OK) plan_free(p);
  return rc;
}

/* mmt_jpeg_entropy_host on one image with its plan; the status word comes back. */
static int entropy_once(const unsigned char* bytes, long len, const mmt_jpeg_image* im, const plan* p, int sb, int rounds, int16_t* coef,
                        int32_t* status) {
  const size_t need = mmt_jpeg_entropy_workspace_bytes(1, p->scan.n_subseq, p->scan.n_subseq, sb, rounds);
  CHECK(need > 0);
  void* work = block(need);
  memset(work, 0xA5, need);
  const int rc = mmt_jpeg_entropy_host(1, bytes, len, im, &p->scan, p->huff, p->seg, p->scan.n_segments, p->sub, p->scan.n_subseq,
                                       p->scan.n_subseq, sb, rounds, coef, im->coef_elems, status, work, need);
  free(work);
  CHECK(rc == MMT_OK);
  return 0;
}

/* Plan + entropy decode of `len` bytes in a block of exactly that size, beside the host decode of the same bytes.
 * must_decode: both must succeed and agree.  Otherwise every outcome is allowed but one: a status of 0 on a file the host
 * decode refuses, or with other coefficients -- whatever the device path accepts it must decode as the host path does. */
static int decode_once(const unsigned char* src, long len, int sb, int must_decode) {
  unsigned char* bytes = (unsigned char*)block((size_t)len);
  memcpy(bytes, src, (size_t)len);
  mmt_jpeg_image im;
  int rc = mmt_jpeg_info(bytes, len, &im);
  if (rc == MMT_OK && im.coef_elems > MAX_COEF) { ++g_skipped; free(bytes); CHECK(!must_decode); return 0; }
  if (rc != MMT_OK) { ++g_refused; free(bytes); CHECK(!must_decode); return 0; }
  plan p;
  rc = plan_make(bytes, len, &im, sb, &p);
  if (rc != MMT_OK) {
    ++g_refused;
    CHECK(!must_decode);
    CHECK(rc == MMT_E_INVALID || rc == MMT_E_UNSUPPORTED);
    CHECK(mmt_last_error()[0] != 0);
    free(bytes);
    return 0;
  }
  int16_t* want = (int16_t*)block((size_t)im.coef_elems * 2);
  int16_t* got = (int16_t*)block((size_t)im.coef_elems * 2);
  uint16_t* q = (uint16_t*)block(3 * 64 * 2);
  memset(got, 0x55, (size_t)im.coef_elems * 2);
  const int host_rc = mmt_jpeg_coefficients(bytes, len, &im, want, im.coef_elems, q);
  int rounds = must_decode ? p.scan.max_segment_subseq : (p.scan.max_segment_subseq < 24 ? p.scan.max_segment_subseq : 24);
  if (rounds < 1) rounds = 1;
  int32_t status = -99;
  CHECK(entropy_once(bytes, len, &im, &p, sb, rounds, got, &status) == 0);
  CHECK(status == MMT_JPEG_ST_OK || status == MMT_JPEG_ST_NOT_CONVERGED || (status >= MMT_JPEG_ST_BAD_CODE && status <= MMT_JPEG_ST_BLOCKS));
  if (must_decode) CHECK(status == MMT_JPEG_ST_OK && host_rc == MMT_OK);
  if (status == MMT_JPEG_ST_OK) {
    CHECK(host_rc == MMT_OK);
    CHECK(memcmp(got, want, (size_t)im.coef_elems * 2) == 0);
    CHECK(memcmp(p.q, q, 3 * 64 * 2) == 0);
    ++g_exact;
  } else {
    ++g_status;
  }
  free(q); free(got); free(want);
  plan_free(&p);
  free(bytes);
  return 0;
}

/* A good file with wrong plans: the clamping must keep every access inside the exact-size blocks, and every loop must end. */
static int wrong_plans(const unsigned char* src, long len, int sb) {
  unsigned char* bytes = (unsigned char*)block((size_t)len);
  memcpy(bytes, src, (size_t)len);
  mmt_jpeg_image im;
  CHECK(mmt_jpeg_info(bytes, len, &im) == MMT_OK);
  plan good;
  CHECK(plan_make(bytes, len, &im, sb, &good) == MMT_OK);
  int16_t* coef = (int16_t*)block((size_t)im.coef_elems * 2);
  const int64_t offsets[] = {-1, -((int64_t)1 << 40), 1, 7, len - 1, len, len + 12345, (int64_t)1 << 50, INT64_MAX, INT64_MIN};
  const int32_t counts[] = {0, -5, 1, 2, 3, 1000, 65535, 1 << 30, INT32_MAX, INT32_MIN};
  const int nseg = good.scan.n_segments, nsub = good.scan.n_subseq;
  const size_t seg_bytes = (size_t)nseg * 16, sub_bytes = (size_t)nsub * 4;
  for (int a = 0; a < 10; ++a)
    for (int s = 0; s < 10; ++s)
      for (int variant = 0; variant < 8; ++variant) {
        plan p = good;
        p.seg = (int32_t*)block(seg_bytes);
        p.sub = (int32_t*)block(sub_bytes);
        p.huff = (uint32_t*)block(6 * MMT_JPEG_HUFF_WORDS * 4);
        memcpy(p.seg, good.seg, seg_bytes); memcpy(p.sub, good.sub, sub_bytes); memcpy(p.huff, good.huff, 6 * MMT_JPEG_HUFF_WORDS * 4);
        mmt_jpeg_image m = im;
        if (variant == 0) { p.scan.byte_offset = offsets[a]; p.scan.byte_count = offsets[(a + s) % 10]; }
        if (variant == 1) { p.scan.segment_offset = offsets[a]; p.scan.n_segments = counts[s]; }
        if (variant == 2) { p.scan.subseq_offset = offsets[a]; p.scan.n_subseq = counts[s]; }
        if (variant == 3) { p.scan.restart_interval = counts[s]; p.scan.mcus = counts[(s + a) % 10]; p.scan.components = counts[a]; }
        if (variant == 4) { for (int i = 0; i < nseg * 4; ++i) p.seg[i] = (i + a) % 3 ? counts[(s + i) % 10] : (int32_t)offsets[(a + i) % 10]; }
        if (variant == 5) { for (int i = 0; i < nsub; ++i) p.sub[i] = counts[(s + i + a) % 10]; }
        if (variant == 6) { for (int i = 0; i < 6 * MMT_JPEG_HUFF_WORDS; ++i) p.huff[i] = (uint32_t)counts[(s + i) % 10] ^ (uint32_t)(i * 2654435761u + (uint32_t)a); }
        if (variant == 7) { m.blocks_w[0] = counts[s]; m.blocks_h[1] = counts[(s + a) % 10]; m.coef_offset[2] = offsets[a]; m.h_samp[0] = a % 3; p.seg[0] = counts[a]; }
        const size_t need = mmt_jpeg_entropy_workspace_bytes(1, nsub, nsub, sb, 3);
        void* work = block(need);
        memset(work, (a * 16 + s) & 0xFF, need);                /* the workspace needs no initialisation: any content */
        int32_t status = -99;
        CHECK(mmt_jpeg_entropy_host(1, bytes, len, &m, &p.scan, p.huff, p.seg, nseg, p.sub, nsub, nsub, sb, 3, coef, im.coef_elems, &status,
                                    work, need) == MMT_OK);
        CHECK(status >= 0 && status <= MMT_JPEG_ST_NOT_CONVERGED);
        free(work); free(p.seg); free(p.sub); free(p.huff);
        ++g_wrong;
      }
  /* argument errors */
  const size_t need = mmt_jpeg_entropy_workspace_bytes(1, nsub, nsub, sb, 2);
  void* work = block(need);
  int32_t status = 0;
#define CALL(B, BYTES, ROUNDS, COEF, WS) mmt_jpeg_entropy_host(B, BYTES, len, &im, &good.scan, good.huff, good.seg, nseg, good.sub, nsub, nsub, sb, ROUNDS, COEF, im.coef_elems, &status, work, WS)
  CHECK(CALL(1, bytes, 2, coef, need) == MMT_OK);
  CHECK(CALL(0, bytes, 2, coef, need) == MMT_E_INVALID);
  CHECK(CALL(1, NULL, 2, coef, need) == MMT_E_INVALID);
  CHECK(CALL(1, bytes + 1, 2, coef, need) == MMT_E_INVALID);
  CHECK(CALL(1, bytes, 0, coef, need) == MMT_E_INVALID);
  CHECK(CALL(1, bytes, 2, NULL, need) == MMT_E_INVALID);
  CHECK(CALL(1, bytes, 2, coef, need - 1) == MMT_E_WORKSPACE);
  CHECK(strstr(mmt_last_error(), "bytes needed") != NULL);
#undef CALL
  CHECK(mmt_jpeg_entropy_workspace_bytes(1, nsub, nsub, 96, 2) == 0 && mmt_jpeg_entropy_workspace_bytes(1, nsub, nsub + 1, sb, 2) == 0);
  mmt_jpeg_scan scan;
  CHECK(mmt_jpeg_scan_plan(NULL, 4, &im, sb, &scan, NULL, NULL, NULL, 0, NULL, 0) == MMT_E_INVALID);
  CHECK(mmt_jpeg_scan_plan(bytes, len, NULL, sb, &scan, NULL, NULL, NULL, 0, NULL, 0) == MMT_E_INVALID);
  CHECK(mmt_jpeg_scan_plan(bytes, len, &im, 12, &scan, NULL, NULL, NULL, 0, NULL, 0) == MMT_E_INVALID);
  CHECK(mmt_jpeg_scan_plan(bytes, len, &im, sb, &scan, NULL, NULL, good.seg, nseg, NULL, 0) == MMT_E_INVALID);
  CHECK(mmt_jpeg_scan_plan(bytes, len, &im, sb, &scan, NULL, NULL, good.seg, nseg - 1, good.sub, nsub) == MMT_E_INVALID);
  free(work); free(coef);
  plan_free(&good);
  free(bytes);
  return 0;
}

int main(int argc, char** argv) {
  const char* dir = argc > 1 ? argv[1] : "../../tests/golden/jpeg";
  char list[1024];
  snprintf(list, sizeof(list), "%s/fixtures.txt", dir);
  FILE* f = fopen(list, "r");
  if (!f) { fprintf(stderr, "jpeg entropy asan driver: cannot open %s\n", list); return 1; }
  char name[256];
  int files = 0;
  const int sizes[] = {8, 128, 1024};
  while (fgets(name, sizeof(name), f)) {
    name[strcspn(name, "\r\n")] = 0;
    if (!name[0]) continue;
    long len = 0;
    unsigned char* bytes = read_file(dir, name, ".jpg", &len);
    CHECK(bytes != NULL);
    for (int i = 0; i < 3; ++i) CHECK(decode_once(bytes, len, sizes[i], 1) == 0);
    free(bytes);
    ++files;
  }
  fclose(f);
  CHECK(files > 0 && g_exact == 3 * files);

  const char* refusals[] = {"refuse_progressive.jpg", "refuse_cmyk.jpg", "refuse_arithmetic.jpg", "refuse_signature.png"};
  for (int i = 0; i < 4; ++i) {
    long len = 0;
    unsigned char* bytes = read_file(dir, refusals[i], "", &len);
    CHECK(bytes != NULL);
    CHECK(decode_once(bytes, len, 128, 0) == 0);
    free(bytes);
  }

  const char* small[] = {"17x9_420_q30_rst1", "9x3_444_q90", "16x16_grey_q80"};
  for (int i = 0; i < 3; ++i) {
    long len = 0;
    unsigned char* bytes = read_file(dir, small[i], ".jpg", &len);
    CHECK(bytes != NULL);
    const int sb = i == 1 ? 16 : 8;
    for (long cut = 0; cut < len; ++cut) CHECK(decode_once(bytes, cut, sb, 0) == 0);         /* every prefix */
    for (long at = 0; at < len && at < 700; ++at) {                                           /* every single-byte corruption */
      const unsigned char keep = bytes[at];
      const unsigned char values[3] = {0x00, 0xFF, (unsigned char)~keep};
      for (int v = 0; v < 3; ++v) {
        bytes[at] = values[v];
        CHECK(decode_once(bytes, len, sb, 0) == 0);
      }
      bytes[at] = keep;
    }
    CHECK(wrong_plans(bytes, len, sb) == 0);
    free(bytes);
  }
  printf("jpeg entropy asan driver ok (%d fixtures, %ld exact decodes, %ld status words, %ld refusals, %ld oversize headers skipped, %ld wrong plans)\n",
         files, g_exact, g_status, g_refused, g_skipped, g_wrong);
  return 0;
}
