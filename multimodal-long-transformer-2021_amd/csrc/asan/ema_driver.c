/* C driver of the sanitizer build of the weight averages' host side (`make asan-ema`, CPU only): the argument checks of
 * ema.hip, mmt_ema_step_host and mmt_ema_swap_host -- the functions of ema.h that the kernels run, as plain loops --
 * under -fsanitize=address,undefined.  Every slab lives in a heap block of exactly the size the library was told, so a
 * read or write past either end is reported.  The numbers are checked against a double-precision restatement of the
 * definition.  Nothing touches a GPU. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/mmt_attn.h"
#include "../../../include/mmt_layer.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "ema asan driver: %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, mmt_last_error()); return 1; } } while (0)

static long g_steps, g_refused, g_swaps;

static void* block(size_t n, size_t align) {          /* exactly n bytes */
  void* p = NULL;
  if (posix_memalign(&p, align < sizeof(void*) ? sizeof(void*) : align, n ? n : 1) != 0) abort();
  return p;
}

static uint32_t g_rng = 2024u;
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

/* slabs of `chunks` chunks whose last `pad` elements are padding (zero), over a few steps of rising decay */
static int run_slab(int chunks, long pad) {
  const long n = (long)chunks * 1024, used = n - pad;
  const size_t bytes = (size_t)n * 4;
  float *param = (float*)block(bytes, 16), *avg = (float*)block(bytes, 16), *avg2 = (float*)block(bytes, 16);
  double* ref = (double*)calloc((size_t)n, 8);
  memset(param, 0, bytes);
  for (long i = 0; i < used; ++i) param[i] = rnd();
  memcpy(avg, param, bytes);                           /* the averages start as the parameters */
  for (long i = 0; i < n; ++i) ref[i] = (double)avg[i];
  mmt_ema_desc d;
  memset(&d, 0, sizeof(d));
  d.n = n;
  for (int t = 1; t <= 5; ++t) {
    for (long i = 0; i < used; ++i) param[i] += 0.05f * rnd();      /* the optimizer's step */
    const double decay = t < 2 ? 0.0 : fmin(0.99, (1.0 + (t - 2)) / (10.0 + (t - 2)));
    d.one_minus_decay = (float)(1.0 - decay);
    /* the decay word's form (on the host: a float) with the field poisoned gives the same bits */
    float* word = (float*)block(4, 4);
    *word = d.one_minus_decay;
    memcpy(avg2, avg, bytes);
    mmt_ema_desc e = d;
    e.one_minus_decay = 7.f; e.one_minus_decay_dev = word;
    CHECK(mmt_ema_step_host(&e, param, avg2) == MMT_OK);
    CHECK(mmt_ema_step_host(&d, param, avg) == MMT_OK);
    g_steps += 2;
    CHECK(memcmp(avg, avg2, bytes) == 0);
    free(word);
    for (long i = 0; i < n; ++i) {
      /* one rounding of the difference and one of the result: 2^-23 of the larger magnitude covers both */
      ref[i] = ref[i] + (double)d.one_minus_decay * ((double)param[i] - ref[i]);
      const double mag = fmax(fabs((double)param[i]), fabs(ref[i]));
      CHECK(fabs((double)avg[i] - ref[i]) <= (double)t * 1.2e-7 * mag);
      if (decay == 0.0) CHECK(avg[i] == param[i]);
    }
    for (long i = used; i < n; ++i) CHECK(avg[i] == 0.f && param[i] == 0.f);     /* padding stays exactly zero */
  }
  /* one_minus_decay 1: the parameter itself, whatever the magnitudes; 0: untouched, also beside an infinity */
  for (long i = 0; i < used; ++i) { param[i] = rnd() * 1e-10f; avg[i] = rnd() * 1e10f; }
  if (used > 2) { param[1] = INFINITY; param[2] = -0.f; }
  memcpy(avg2, avg, bytes);
  d.one_minus_decay = 0.f;
  CHECK(mmt_ema_step_host(&d, param, avg) == MMT_OK);
  CHECK(memcmp(avg, avg2, bytes) == 0);
  d.one_minus_decay = 1.f;
  CHECK(mmt_ema_step_host(&d, param, avg) == MMT_OK);
  CHECK(memcmp(avg, param, bytes) == 0);
  g_steps += 2;
  /* swap: exact exchange, the shadow is bf16 of the new parameter, twice is the identity, NULL shadow is taken */
  uint16_t *shadow = (uint16_t*)block((size_t)n * 2, 8), *shadow0 = (uint16_t*)block((size_t)n * 2, 8);
  float *p0 = (float*)block(bytes, 16), *a0 = (float*)block(bytes, 16);
  for (long i = 0; i < used; ++i) avg[i] = rnd();
  for (long i = 0; i < n; ++i) shadow[i] = bf16_bits(param[i]);
  memcpy(p0, param, bytes); memcpy(a0, avg, bytes); memcpy(shadow0, shadow, (size_t)n * 2);
  CHECK(mmt_ema_swap_host(n, param, avg, shadow) == MMT_OK);
  CHECK(memcmp(param, a0, bytes) == 0 && memcmp(avg, p0, bytes) == 0);
  for (long i = 0; i < n; ++i) CHECK(shadow[i] == bf16_bits(a0[i]));
  CHECK(mmt_ema_swap_host(n, param, avg, shadow) == MMT_OK);
  CHECK(memcmp(param, p0, bytes) == 0 && memcmp(avg, a0, bytes) == 0 && memcmp(shadow, shadow0, (size_t)n * 2) == 0);
  CHECK(mmt_ema_swap_host(n, param, avg, NULL) == MMT_OK);
  CHECK(memcmp(param, a0, bytes) == 0 && memcmp(avg, p0, bytes) == 0 && memcmp(shadow, shadow0, (size_t)n * 2) == 0);
  g_swaps += 3;
  free(param); free(avg); free(avg2); free(ref); free(shadow); free(shadow0); free(p0); free(a0);
  return 0;
}

static int refusals(void) {
  const long n = 2048;
  float *param = (float*)block((size_t)n * 4, 16), *avg = (float*)block((size_t)n * 4, 16);
  uint16_t* shadow = (uint16_t*)block((size_t)n * 2, 8);
  for (long i = 0; i < n; ++i) { param[i] = 1.f; avg[i] = 2.f; shadow[i] = 3; }
  mmt_ema_desc d;
  memset(&d, 0, sizeof(d));
  d.n = n; d.one_minus_decay = 0.5f;
#define REFUSED(call) do { CHECK((call) == MMT_E_INVALID); CHECK(mmt_last_error()[0] != 0); ++g_refused; } while (0)
  REFUSED(mmt_ema_step_host(NULL, param, avg));
  REFUSED(mmt_ema_step_host(&d, NULL, avg));
  REFUSED(mmt_ema_step_host(&d, param, NULL));
  REFUSED(mmt_ema_step_host(&d, param, param));
  REFUSED(mmt_ema_step_host(&d, param + 1, avg));
  REFUSED(mmt_ema_step_host(&d, param, avg + 1));
  REFUSED(mmt_ema_swap_host(n, NULL, avg, shadow));
  REFUSED(mmt_ema_swap_host(n, param, NULL, shadow));
  REFUSED(mmt_ema_swap_host(n, param, param, shadow));
  REFUSED(mmt_ema_swap_host(n, param + 1, avg, shadow));
  REFUSED(mmt_ema_swap_host(n, param, avg, shadow + 1));
  const int64_t bad_n[] = {0, -1024, 1000, 1025, INT64_MIN};
  for (int i = 0; i < 5; ++i) {
    mmt_ema_desc e = d;
    e.n = bad_n[i];
    REFUSED(mmt_ema_step_host(&e, param, avg));
    REFUSED(mmt_ema_swap_host(bad_n[i], param, avg, shadow));
  }
  const float bad_omd[] = {-1e-6f, 1.0000001f, -INFINITY, INFINITY, NAN};
  float* word = (float*)block(4, 4);
  *word = 0.f;                                         /* 1 - decay 0: a taken call changes nothing either */
  for (int i = 0; i < 5; ++i) {
    mmt_ema_desc e = d;
    e.one_minus_decay = bad_omd[i];
    REFUSED(mmt_ema_step_host(&e, param, avg));
    e.one_minus_decay_dev = word;                      /* with a decay word the field is not read */
    CHECK(mmt_ema_step_host(&e, param, avg) == MMT_OK);
  }
  free(word);
  /* nothing was written by a refused call */
  for (long i = 0; i < n; ++i) CHECK(param[i] == 1.f && avg[i] == 2.f && shadow[i] == 3);
  free(param); free(avg); free(shadow);
  return 0;
}

int main(void) {
  CHECK(run_slab(1, 0) == 0);
  CHECK(run_slab(2, 1023) == 0);
  CHECK(run_slab(7, 130) == 0);
  CHECK(refusals() == 0);
  printf("ema asan driver ok: %ld steps, %ld refusals, %ld swaps\n", g_steps, g_refused, g_swaps);
  return 0;
}
