/* C driver of the sanitizer build of the LAMB step's host side (`make asan-lamb`, CPU only): the argument checks of
 * lamb.hip and mmt_lamb_step_host -- the functions of lamb.h that the kernels run, as plain loops -- under
 * -fsanitize=address,undefined.  Every slab, table and workspace lives in a heap block of exactly the size the library
 * was told, so a read or write past either is reported.  The numbers are checked against a double-precision restatement
 * of the definition that works on whole parameters and knows nothing of chunks.  Nothing touches a GPU. */
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/mmt_attn.h"
#include "../../../include/mmt_layer.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "lamb asan driver: %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, mmt_last_error()); return 1; } } while (0)
#define MAX_SEG 8
#define BOUND 2e-6

static long g_steps, g_refused, g_tables;

static void* block(size_t n, size_t align) {          /* exactly n bytes */
  void* p = NULL;
  if (posix_memalign(&p, align < sizeof(void*) ? sizeof(void*) : align, n ? n : 1) != 0) abort();
  return p;
}

static uint32_t g_rng = 12345u;
static float rnd(void) {                               /* roughly normal, in (-3, 3) */
  float s = 0.f;
  for (int k = 0; k < 4; ++k) { g_rng = g_rng * 1664525u + 1013904223u; s += (float)(g_rng >> 8) * (1.f / 16777216.f) - 0.5f; }
  return s * 1.7320508f;
}

static uint16_t bf16_bits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0u;
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

typedef struct slab {
  int n_seg;
  long n, n_chunks, size[MAX_SEG], off[MAX_SEG];
  float *param, *grad, *m, *v, *wd;
  uint16_t* shadow;
  int32_t *seg, *adapt;
  void* work;
  size_t work_bytes;
  double *rw, *rm, *rv;                                /* the reference's state, same layout */
} slab;

static void slab_make(slab* s, int n_seg, const long* sizes, const int* excluded, float wd) {
  s->n_seg = n_seg;
  long off = 0;
  for (int i = 0; i < n_seg; ++i) { s->size[i] = sizes[i]; s->off[i] = off; off += (sizes[i] + 1023) & ~1023L; }
  s->n = off; s->n_chunks = off >> 10;
  s->param = (float*)block((size_t)s->n * 4, 16); s->grad = (float*)block((size_t)s->n * 4, 16);
  s->m = (float*)block((size_t)s->n * 4, 16); s->v = (float*)block((size_t)s->n * 4, 16);
  s->shadow = (uint16_t*)block((size_t)s->n * 2, 8);
  s->wd = (float*)block((size_t)s->n_chunks * 4, 4);
  s->seg = (int32_t*)block((size_t)(n_seg + 1) * 4, 4); s->adapt = (int32_t*)block((size_t)n_seg * 4, 4);
  s->work_bytes = mmt_lamb_workspace_bytes(s->n);
  s->work = block(s->work_bytes, 16);
  s->rw = (double*)calloc((size_t)s->n, 8); s->rm = (double*)calloc((size_t)s->n, 8); s->rv = (double*)calloc((size_t)s->n, 8);
  memset(s->param, 0, (size_t)s->n * 4); memset(s->grad, 0, (size_t)s->n * 4);
  memset(s->m, 0, (size_t)s->n * 4); memset(s->v, 0, (size_t)s->n * 4); memset(s->shadow, 0, (size_t)s->n * 2);
  memset(s->work, 0, s->work_bytes);
  for (int i = 0; i < n_seg; ++i) {
    s->seg[i] = (int32_t)(s->off[i] >> 10);
    s->adapt[i] = excluded[i] ? 0 : 1;
    for (long c = s->off[i] >> 10; c < (s->off[i] + s->size[i] + 1023) >> 10; ++c) s->wd[c] = excluded[i] ? 0.f : wd;
    for (long k = 0; k < s->size[i]; ++k) { s->param[s->off[i] + k] = rnd(); s->rw[s->off[i] + k] = (double)s->param[s->off[i] + k]; }
  }
  s->seg[n_seg] = (int32_t)s->n_chunks;
}

static void slab_free(slab* s) {
  free(s->param); free(s->grad); free(s->m); free(s->v); free(s->shadow); free(s->wd); free(s->seg); free(s->adapt); free(s->work);
  free(s->rw); free(s->rm); free(s->rv);
}

static void desc_fill(mmt_lamb_desc* d, const slab* s, int t, float lr) {
  memset(d, 0, sizeof(*d));
  d->n = s->n; d->lr = lr; d->beta1 = 0.9f; d->beta2 = 0.999f; d->eps = 1e-6f;
  d->bias_correction1 = (float)(1.0 - pow(0.9, t)); d->bias_correction2 = (float)(1.0 - pow(0.999, t));
  d->zero_grad = 1; d->n_segments = s->n_seg; d->hyper = NULL;
}

/* the definition on whole parameters, in double; the gradient is read from s->grad before the library overwrites it */
static void reference_step(slab* s, int t, double lr, double scale, double wd) {
  const double b1 = 0.9, b2 = 0.999, eps = (double)1e-6f;
  for (int i = 0; i < s->n_seg; ++i) {
    const long o = s->off[i], k = s->size[i];
    double* u = (double*)malloc((size_t)k * 8);
    double w2 = 0, u2 = 0;
    for (long j = 0; j < k; ++j) {
      const double g = (double)s->grad[o + j] * scale;
      s->rm[o + j] = b1 * s->rm[o + j] + (1 - b1) * g;
      s->rv[o + j] = b2 * s->rv[o + j] + (1 - b2) * g * g;
      u[j] = (s->rm[o + j] / (1 - pow(b1, t))) / (sqrt(s->rv[o + j] / (1 - pow(b2, t))) + eps);
      if (s->adapt[i]) u[j] += wd * s->rw[o + j];      /* in these slabs "excluded" means from decay and adaptation alike */
      w2 += s->rw[o + j] * s->rw[o + j]; u2 += u[j] * u[j];
    }
    const double r = (s->adapt[i] && w2 > 0 && u2 > 0) ? sqrt(w2) / sqrt(u2) : 1.0;
    for (long j = 0; j < k; ++j) s->rw[o + j] -= lr * r * u[j];
    free(u);
  }
}

static int run_slab(int n_seg, const long* sizes, const int* excluded) {
  slab s;
  const float wd = 0.01f, lr = 1e-2f;
  slab_make(&s, n_seg, sizes, excluded, wd);
  CHECK(s.work_bytes == (((size_t)s.n_chunks * 12 + 15) & ~(size_t)15));
  float* scale = (float*)block(4, 4);
  for (int t = 1; t <= 3; ++t) {
    for (int i = 0; i < n_seg; ++i)
      for (long k = 0; k < s.size[i]; ++k) s.grad[s.off[i] + k] = rnd() * (t == 2 ? 3.0f : 0.1f);
    *scale = t == 2 ? 0.37f : 1.0f;
    reference_step(&s, t, (double)lr, (double)*scale, (double)wd);
    mmt_lamb_desc d;
    desc_fill(&d, &s, t, lr);
    CHECK(mmt_lamb_step_host(&d, s.param, s.grad, s.m, s.v, s.shadow, s.wd, s.seg, s.adapt, t == 3 ? NULL : scale, s.work, s.work_bytes) == MMT_OK);
    ++g_steps;
    for (long i = 0; i < s.n; ++i) {
      CHECK(fabs((double)s.param[i] - s.rw[i]) < BOUND && fabs((double)s.m[i] - s.rm[i]) < BOUND && fabs((double)s.v[i] - s.rv[i]) < BOUND);
      CHECK(s.grad[i] == 0.f && s.shadow[i] == bf16_bits(s.param[i]));
    }
    for (int i = 0; i < n_seg; ++i)                     /* padding stays exactly zero */
      for (long k = s.off[i] + s.size[i]; k < (i + 1 < n_seg ? s.off[i + 1] : s.n); ++k)
        CHECK(s.param[k] == 0.f && s.m[k] == 0.f && s.v[k] == 0.f && s.shadow[k] == 0);
  }
  /* the device-resident scalars' form (on the host: an array of three floats), and zero_grad off: grad holds u */
  {
    mmt_lamb_desc d;
    desc_fill(&d, &s, 4, lr);
    float* hyper = (float*)block(12, 4);
    hyper[0] = d.lr; hyper[1] = d.bias_correction1; hyper[2] = d.bias_correction2;
    size_t bytes = (size_t)s.n * 4;
    float *p2 = (float*)block(bytes, 16), *g2 = (float*)block(bytes, 16), *m2 = (float*)block(bytes, 16), *v2 = (float*)block(bytes, 16);
    for (int i = 0; i < n_seg; ++i)
      for (long k = 0; k < s.size[i]; ++k) s.grad[s.off[i] + k] = rnd() * 0.1f;
    memcpy(p2, s.param, bytes); memcpy(g2, s.grad, bytes); memcpy(m2, s.m, bytes); memcpy(v2, s.v, bytes);
    CHECK(mmt_lamb_step_host(&d, s.param, s.grad, s.m, s.v, NULL, s.wd, s.seg, s.adapt, NULL, s.work, s.work_bytes) == MMT_OK);
    d.lr = 123.f; d.bias_correction1 = 0.5f; d.bias_correction2 = 0.25f; d.hyper = hyper; d.zero_grad = 0;
    CHECK(mmt_lamb_step_host(&d, p2, g2, m2, v2, NULL, s.wd, s.seg, s.adapt, NULL, s.work, s.work_bytes) == MMT_OK);
    g_steps += 2;
    CHECK(memcmp(p2, s.param, bytes) == 0 && memcmp(m2, s.m, bytes) == 0 && memcmp(v2, s.v, bytes) == 0);
    free(hyper); free(p2); free(g2); free(m2); free(v2);
  }
  free(scale);
  slab_free(&s);
  return 0;
}

static int refusals(void) {
  const long sizes[2] = {1500, 5};
  const int excluded[2] = {0, 1};
  slab s;
  slab_make(&s, 2, sizes, excluded, 0.01f);
  mmt_lamb_desc d;
  desc_fill(&d, &s, 1, 1e-2f);
#define CALL(dd, p, g, m, v, wd, sg, ad, wk, wb) mmt_lamb_step_host(dd, p, g, m, v, s.shadow, wd, sg, ad, NULL, wk, wb)
#define REFUSED(call, code) do { CHECK((call) == (code)); CHECK(mmt_last_error()[0] != 0); ++g_refused; } while (0)
  REFUSED(CALL(NULL, s.param, s.grad, s.m, s.v, s.wd, s.seg, s.adapt, s.work, s.work_bytes), MMT_E_INVALID);
  REFUSED(CALL(&d, NULL, s.grad, s.m, s.v, s.wd, s.seg, s.adapt, s.work, s.work_bytes), MMT_E_INVALID);
  REFUSED(CALL(&d, s.param, NULL, s.m, s.v, s.wd, s.seg, s.adapt, s.work, s.work_bytes), MMT_E_INVALID);
  REFUSED(CALL(&d, s.param, s.grad, NULL, s.v, s.wd, s.seg, s.adapt, s.work, s.work_bytes), MMT_E_INVALID);
  REFUSED(CALL(&d, s.param, s.grad, s.m, NULL, s.wd, s.seg, s.adapt, s.work, s.work_bytes), MMT_E_INVALID);
  REFUSED(CALL(&d, s.param, s.grad, s.m, s.v, NULL, s.seg, s.adapt, s.work, s.work_bytes), MMT_E_INVALID);
  REFUSED(CALL(&d, s.param, s.grad, s.m, s.v, s.wd, NULL, s.adapt, s.work, s.work_bytes), MMT_E_INVALID);
  REFUSED(CALL(&d, s.param, s.grad, s.m, s.v, s.wd, s.seg, NULL, s.work, s.work_bytes), MMT_E_INVALID);
  REFUSED(CALL(&d, s.param, s.grad, s.m, s.v, s.wd, s.seg, s.adapt, NULL, s.work_bytes), MMT_E_WORKSPACE);
  REFUSED(CALL(&d, s.param, s.grad, s.m, s.v, s.wd, s.seg, s.adapt, s.work, s.work_bytes - 1), MMT_E_WORKSPACE);
  REFUSED(CALL(&d, s.param, s.grad, s.m, s.v, s.wd, s.seg, s.adapt, s.work, 0), MMT_E_WORKSPACE);
  REFUSED(CALL(&d, s.param + 1, s.grad, s.m, s.v, s.wd, s.seg, s.adapt, s.work, s.work_bytes), MMT_E_INVALID);
  const int64_t bad_n[] = {0, -1024, 1000, 1025, INT64_MIN};
  for (int i = 0; i < 5; ++i) {
    mmt_lamb_desc e = d;
    e.n = bad_n[i];
    REFUSED(CALL(&e, s.param, s.grad, s.m, s.v, s.wd, s.seg, s.adapt, s.work, s.work_bytes), MMT_E_INVALID);
    CHECK(mmt_lamb_workspace_bytes(bad_n[i]) == 0);
  }
  const float bad_bc[] = {0.f, -0.1f, NAN};
  for (int i = 0; i < 3; ++i) {
    mmt_lamb_desc e = d;
    e.bias_correction1 = bad_bc[i];
    REFUSED(CALL(&e, s.param, s.grad, s.m, s.v, s.wd, s.seg, s.adapt, s.work, s.work_bytes), MMT_E_INVALID);
    e = d;
    e.bias_correction2 = bad_bc[i];
    REFUSED(CALL(&e, s.param, s.grad, s.m, s.v, s.wd, s.seg, s.adapt, s.work, s.work_bytes), MMT_E_INVALID);
  }
  const int32_t bad_seg[] = {0, -1, INT32_MIN};
  for (int i = 0; i < 3; ++i) {
    mmt_lamb_desc e = d;
    e.n_segments = bad_seg[i];
    REFUSED(CALL(&e, s.param, s.grad, s.m, s.v, s.wd, s.seg, s.adapt, s.work, s.work_bytes), MMT_E_INVALID);
  }
  /* nothing was written by a refused call */
  for (long i = 0; i < s.n; ++i) CHECK(s.m[i] == 0.f && s.v[i] == 0.f && s.grad[i] == 0.f);
  slab_free(&s);
  return 0;
}

/* wrong segment tables against the clamping: whatever the table says, nothing outside the slabs and the workspace is
 * touched, the moments are those of the right table, and a chunk that no segment covers keeps its parameters (the
 * workspace starts as zeros here, so such a chunk's ratio is 0) */
static int wrong_tables(void) {
  const long sizes[3] = {2100, 1024, 7};               /* 3 + 1 + 1 chunks */
  const int excluded[3] = {0, 0, 0};
  slab s;
  slab_make(&s, 3, sizes, excluded, 0.01f);
  const size_t bytes = (size_t)s.n * 4;
  for (long i = 0; i < s.n; ++i) s.grad[i] = 0.f;
  for (int i = 0; i < 3; ++i)
    for (long k = 0; k < s.size[i]; ++k) s.grad[s.off[i] + k] = rnd() * 0.1f;
  float *p0 = (float*)block(bytes, 16), *g0 = (float*)block(bytes, 16), *m_ok = (float*)block(bytes, 16), *v_ok = (float*)block(bytes, 16);
  memcpy(p0, s.param, bytes); memcpy(g0, s.grad, bytes);
  mmt_lamb_desc d;
  desc_fill(&d, &s, 1, 1e-2f);
  CHECK(mmt_lamb_step_host(&d, s.param, s.grad, s.m, s.v, s.shadow, s.wd, s.seg, s.adapt, NULL, s.work, s.work_bytes) == MMT_OK);
  memcpy(m_ok, s.m, bytes); memcpy(v_ok, s.v, bytes);
  const int32_t vals[] = {INT32_MIN, -1, 0, 2, (int32_t)s.n_chunks, (int32_t)s.n_chunks + 1, INT32_MAX};
  const int nv = (int)(sizeof(vals) / sizeof(vals[0]));
  for (int a = 0; a < nv; ++a)
    for (int b = 0; b < nv; ++b)
      for (int c = 0; c < nv; ++c) {                   /* 343 tables of two segments: negative, decreasing, beyond the slab */
        int32_t* seg = (int32_t*)block(3 * 4, 4);
        seg[0] = vals[a]; seg[1] = vals[b]; seg[2] = vals[c];
        memcpy(s.param, p0, bytes); memcpy(s.grad, g0, bytes);
        memset(s.m, 0, bytes); memset(s.v, 0, bytes); memset(s.work, 0, s.work_bytes);
        mmt_lamb_desc e = d;
        e.n_segments = 2;
        CHECK(mmt_lamb_step_host(&e, s.param, s.grad, s.m, s.v, s.shadow, s.wd, seg, s.adapt, NULL, s.work, s.work_bytes) == MMT_OK);
        ++g_tables;
        CHECK(memcmp(s.m, m_ok, bytes) == 0 && memcmp(s.v, v_ok, bytes) == 0);
        long lo[2], hi[2];
        for (int k = 0; k < 2; ++k) {
          long x = seg[k], y = seg[k + 1];
          lo[k] = x < 0 ? 0 : (x > s.n_chunks ? s.n_chunks : x);
          hi[k] = y < 0 ? 0 : (y > s.n_chunks ? s.n_chunks : y);
        }
        for (long ch = 0; ch < s.n_chunks; ++ch) {
          const int covered = (ch >= lo[0] && ch < hi[0]) || (ch >= lo[1] && ch < hi[1]);
          for (long i = ch << 10; i < (ch + 1) << 10; ++i) {
            CHECK(isfinite(s.param[i]) && s.grad[i] == 0.f);
            if (!covered) CHECK(s.param[i] == p0[i]);
          }
        }
        free(seg);
      }
  free(p0); free(g0); free(m_ok); free(v_ok);
  slab_free(&s);
  return 0;
}

int main(void) {
  const long one[1] = {3 * 1024};
  const int one_x[1] = {0};
  const long two[2] = {130 * 70, 130};
  const int two_x[2] = {0, 1};
  const long seven[7] = {3075, 70, 70, 1024, 1, 33, 5};   /* a last segment of one chunk */
  const int seven_x[7] = {0, 1, 1, 0, 0, 0, 0};
  CHECK(run_slab(1, one, one_x) == 0);
  CHECK(run_slab(2, two, two_x) == 0);
  CHECK(run_slab(7, seven, seven_x) == 0);
  CHECK(refusals() == 0);
  CHECK(wrong_tables() == 0);
  printf("lamb asan driver ok: %ld steps, %ld refusals, %ld wrong segment tables\n", g_steps, g_refused, g_tables);
  return 0;
}
