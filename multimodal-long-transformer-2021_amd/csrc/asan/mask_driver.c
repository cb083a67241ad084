/* C driver of the sanitizer build of the item masking's host side (`make asan-mask`, CPU only): the argument checks of
 * item_masking.hip and mmt_item_masking_host -- the functions of item_masking.h that the kernel runs, as plain loops --
 * under -fsanitize=address,undefined.  Every input and output lives in a heap block of exactly the size the library was
 * told, so a read or write past either is reported.  The rows are checked against a restatement of the definition that
 * ranks every pair of keys with float comparisons and knows nothing of key images, histograms or prefix sums.  Nothing
 * touches a GPU. */
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/mmt_attn.h"
#include "../../../include/mmt_layer.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "mask asan driver: %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, mmt_last_error()); return 1; } } while (0)

static long g_calls, g_refused, g_wild, g_chosen;

static void* block(size_t n) {                         /* exactly n bytes */
  void* p = malloc(n ? n : 1);
  if (!p) abort();
  memset(p, 0x5A, n);
  return p;
}

static uint32_t g_rng = 2463534242u;
static uint32_t rnd(void) { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }
static float unit(void) { return (float)(rnd() >> 8) / 16777216.f; }

typedef struct batch {
  mmt_item_masking_desc d;
  int32_t *tok, *rid, *masked, *pos, *lab;
  int64_t *n, *n_masked;
  int32_t* n32;
  uint8_t* ws;
  float *keys, *u;
  int use_ws;
} batch;

static const int32_t UNSEL[4] = {101, 102, 103, 1};

static void batch_make(batch* b, int B, int T, int use_ws) {
  memset(b, 0, sizeof *b);
  const size_t n = (size_t)B * T;
  b->d.B = B; b->d.T = T; b->d.max_selections = T; b->d.mask_token_id = 104; b->d.n_unselectable = 4;
  memcpy(b->d.unselectable, UNSEL, sizeof UNSEL);
  b->d.n_tokens_i64 = 1; b->d.selection_rate = 0.15f; b->d.mask_threshold = 0.8f; b->d.random_threshold = (float)(0.8 + 0.1);
  b->tok = (int32_t*)block(n * 4); b->rid = (int32_t*)block(n * 4); b->masked = (int32_t*)block(n * 4); b->pos = (int32_t*)block(n * 4);
  b->lab = (int32_t*)block(n * 4); b->n = (int64_t*)block((size_t)B * 8); b->n32 = (int32_t*)block((size_t)B * 4);
  b->n_masked = (int64_t*)block((size_t)B * 8); b->ws = (uint8_t*)block(n); b->keys = (float*)block(n * 4); b->u = (float*)block(n * 4);
  b->use_ws = use_ws;
  for (size_t i = 0; i < n; ++i) {
    b->tok[i] = rnd() % 20u == 0 ? UNSEL[rnd() % 4u] : (int32_t)(1000 + rnd() % 2000u);
    b->rid[i] = (int32_t)rnd();
    b->ws[i] = (uint8_t)(rnd() % 5u < 3 ? 1 + rnd() % 255u : 0);
    b->keys[i] = unit(); b->u[i] = unit();
  }
  for (int r = 0; r < B; ++r) b->n[r] = r == 0 ? 0 : (r == 1 ? T : (int64_t)(1 + rnd() % (uint32_t)T));
}

static void batch_free(batch* b) {
  free(b->tok); free(b->rid); free(b->masked); free(b->pos); free(b->lab); free(b->n); free(b->n32); free(b->n_masked); free(b->ws);
  free(b->keys); free(b->u);
}

static int batch_call(batch* b) {
  ++g_calls;
  if (!b->d.n_tokens_i64)
    for (int r = 0; r < b->d.B; ++r) b->n32[r] = b->n[r] > INT_MAX ? INT_MAX : (b->n[r] < INT_MIN ? INT_MIN : (int32_t)b->n[r]);
  return mmt_item_masking_host(&b->d, b->tok, b->d.n_tokens_i64 ? (const void*)b->n : (const void*)b->n32, b->use_ws ? b->ws : NULL, b->keys,
                               b->u, b->rid, b->masked, b->pos, b->n_masked, b->lab);
}

/* ascending float order of the reference: NaN above everything and equal to NaN, -0 == +0 */
static int key_less(float a, float b) { return (a < b) || (isnan(b) && !isnan(a)); }

static int batch_verify(const batch* b) {
  const mmt_item_masking_desc* d = &b->d;
  const int T = d->T;
  int* item = (int*)malloc((size_t)T * sizeof(int)); int* exists = (int*)malloc((size_t)T * sizeof(int));
  int* unsel = (int*)malloc((size_t)T * sizeof(int)); int* chosen = (int*)malloc((size_t)T * sizeof(int));
  float* key = (float*)malloc((size_t)T * sizeof(float));
  int ok = 1;
  for (int r = 0; r < d->B && ok; ++r) {
    const long row = (long)r * T;
    const int64_t n64 = b->n[r];
    const int n = n64 < 0 ? 0 : (n64 > T ? T : (int)n64);
    int starts = 0;
    memset(exists, 0, (size_t)T * sizeof(int)); memset(unsel, 0, (size_t)T * sizeof(int));
    for (int t = 0; t < n; ++t) {
      starts += b->use_ws ? b->ws[row + t] != 0 : 1;
      item[t] = starts > 0 ? starts - 1 : 0;
      exists[item[t]] = 1;
      for (int k = 0; k < d->n_unselectable; ++k) unsel[item[t]] |= b->tok[row + t] == d->unselectable[k];
    }
    int n_selectable = 0;
    for (int i = 0; i < T; ++i) {
      const int s = exists[i] && !unsel[i];
      n_selectable += s;
      key[i] = s ? b->keys[row + i] : INFINITY;
    }
    volatile float prod = (float)n_selectable * d->selection_rate;
    float want = ceilf(prod);
    if (want > (float)d->max_selections) want = (float)d->max_selections;
    long masked = 0;
    for (int i = 0; i < T; ++i) {
      long rank = 0;
      for (int j = 0; j < T; ++j) rank += key_less(key[j], key[i]) || (j < i && !key_less(key[i], key[j]));
      chosen[i] = exists[i] && !unsel[i] && (float)rank < want;
    }
    for (int t = 0; t < T && ok; ++t) {
      int32_t out = b->tok[row + t];
      if (t < n && chosen[item[t]]) {
        const float u = b->u[row + item[t]];
        if (u < d->mask_threshold) out = d->mask_token_id;
        else if (u < d->random_threshold) out = b->rid[row + t];
        ok = masked < T && b->pos[row + masked] == t && b->lab[row + masked] == b->tok[row + t];
        ++masked;
      }
      ok = ok && b->masked[row + t] == out;
    }
    ok = ok && b->n_masked[r] == masked;
    for (long o = masked; o < T && ok; ++o) ok = b->pos[row + o] == 0 && b->lab[row + o] == 0;
    g_chosen += masked;
  }
  free(item); free(exists); free(unsel); free(chosen); free(key);
  return ok;
}

static int refusals(void) {
  batch b;
  batch_make(&b, 3, 16, 1);
  CHECK(batch_call(&b) == MMT_OK && batch_verify(&b));
#define REFUSED(stmt, undo, code, text) do { stmt; CHECK(batch_call(&b) == (code)); CHECK(strstr(mmt_last_error(), text) != NULL); undo; ++g_refused; } while (0)
  void* keep;
  REFUSED(keep = b.tok; b.tok = NULL, b.tok = (int32_t*)keep, MMT_E_INVALID, "NULL argument");
  REFUSED(keep = b.keys; b.keys = NULL, b.keys = (float*)keep, MMT_E_INVALID, "NULL argument");
  REFUSED(keep = b.n_masked; b.n_masked = NULL, b.n_masked = (int64_t*)keep, MMT_E_INVALID, "NULL argument");
  REFUSED(keep = b.lab; b.lab = NULL, b.lab = (int32_t*)keep, MMT_E_INVALID, "NULL argument");
  REFUSED(b.d.B = 0, b.d.B = 3, MMT_E_INVALID, "at least 1");
  REFUSED(b.d.T = -4, b.d.T = 16, MMT_E_INVALID, "at least 1");
  REFUSED(b.d.n_unselectable = -1, b.d.n_unselectable = 4, MMT_E_INVALID, "must not be negative");
  REFUSED(b.d.B = INT_MAX, b.d.B = 3, MMT_E_INVALID, "below 2^31");
  REFUSED(b.d.T = MMT_MASK_MAX_TOKENS + 1, b.d.T = 16, MMT_E_UNSUPPORTED, "MMT_MASK_MAX_TOKENS");
  REFUSED(b.d.n_unselectable = MMT_MASK_MAX_UNSELECTABLE + 1, b.d.n_unselectable = 4, MMT_E_UNSUPPORTED, "MMT_MASK_MAX_UNSELECTABLE");
  CHECK(mmt_item_masking_host(NULL, b.tok, b.n, b.ws, b.keys, b.u, b.rid, b.masked, b.pos, b.n_masked, b.lab) == MMT_E_INVALID);
  CHECK(batch_call(&b) == MMT_OK && batch_verify(&b));
  batch_free(&b);
  return 0;
}

/* the corner list of tests/test_item_masking_host.py at one size */
static int corners(int T) {
  static const float special[] = {INFINITY, -INFINITY, NAN, -0.0f, 0.0f, 0.25f};
  for (int use_ws = 0; use_ws < 2; ++use_ws) {
    for (int variant = 0; variant < 9; ++variant) {
      batch b;
      batch_make(&b, 5, T, use_ws);
      const long n = 5L * T;
      switch (variant) {
        case 0: break;
        case 1: for (long i = 0; i < n; ++i) b.keys[i] = (float)(rnd() % 4u) / 4.f; b.d.selection_rate = 0.5f; break;      /* ties */
        case 2: for (long i = 0; i < n; ++i) if (rnd() % 10u < 7) b.keys[i] = special[rnd() % 6u]; b.d.selection_rate = 0.6f; break;
        case 3: for (long i = 0; i < n; ++i) if (rnd() % 10u < 7) b.keys[i] = special[rnd() % 6u]; b.d.selection_rate = 1.f; b.d.max_selections = T + 5; break;
        case 4: for (long i = 0; i < n; ++i) b.tok[i] = UNSEL[0]; b.d.selection_rate = 1.f; break;                          /* nothing selectable */
        case 5: {                                                                                                            /* the thresholds */
          const float th[] = {0.8f, nextafterf(0.8f, 0.f), nextafterf(0.8f, 1.f), b.d.random_threshold, nextafterf(b.d.random_threshold, 0.f),
                              nextafterf(b.d.random_threshold, 1.f), 0.f, 1.f, NAN};
          for (long i = 0; i < n; ++i) b.u[i] = th[rnd() % 9u];
          b.d.selection_rate = 1.f;
          break;
        }
        case 6: b.d.selection_rate = 0.f; break;
        case 7: b.d.selection_rate = 0.5f; b.d.max_selections = T / 8; break;
        case 8: b.d.selection_rate = 1.f; b.d.n_tokens_i64 = 0; if (use_ws) for (int r = 0; r < 5; ++r) b.ws[(long)r * T] = 0; break;   /* no start at 0, int32 lengths */
      }
      for (int r = 0; r < 5; ++r)                                    /* behind n_tokens: word starts and unselectable ids that must not count */
        for (long t = b.n[r] < 0 ? 0 : b.n[r]; t < T; ++t) { b.ws[(long)r * T + t] = 1; b.tok[(long)r * T + t] = UNSEL[1]; }
      CHECK(batch_call(&b) == MMT_OK);
      CHECK(batch_verify(&b));
      batch_free(&b);
    }
  }
  return 0;
}

/* n_tokens of every kind, in both widths: the rows are those of the clamped lengths, and nothing leaves a block */
static int wild(void) {
  static const int64_t odd[] = {0, -1, 1, INT_MIN, INT_MAX, (int64_t)1 << 40, -((int64_t)1 << 40), 7, 8, 9, INT64_MAX, INT64_MIN};
  for (int round = 0; round < 300; ++round) {
    const int T = 1 + (int)(rnd() % 70u), B = 1 + (int)(rnd() % 4u);
    batch b;
    batch_make(&b, B, T, (int)(rnd() & 1u));
    for (int r = 0; r < B; ++r) b.n[r] = (rnd() & 1u) ? odd[rnd() % 12u] : (int64_t)(rnd() % (uint32_t)(T + 3)) - 1;
    b.d.n_tokens_i64 = (int)(rnd() & 1u);
    if (!b.d.n_tokens_i64)
      for (int r = 0; r < B; ++r) b.n[r] = b.n[r] > INT_MAX ? INT_MAX : (b.n[r] < INT_MIN ? INT_MIN : b.n[r]);
    b.d.selection_rate = unit() * 1.2f;
    b.d.max_selections = (rnd() & 3u) ? (int)(rnd() % (uint32_t)(T + 2)) : (int)rnd();
    for (long i = 0; i < (long)B * T; ++i) b.rid[i] = (rnd() & 1u) ? INT_MIN : INT_MAX;
    CHECK(batch_call(&b) == MMT_OK);
    CHECK(batch_verify(&b));
    batch_free(&b);
    ++g_wild;
  }
  return 0;
}

int main(void) {
  static const int sizes[] = {1, 2, 63, 64, 65, 257, 1000};
  if (refusals()) return 1;
  for (int i = 0; i < 7; ++i)
    if (corners(sizes[i])) return 1;
  {                                                                  /* the longest row, in blocks of exactly its size */
    batch b;
    batch_make(&b, 1, MMT_MASK_MAX_TOKENS, 1);
    b.n[0] = MMT_MASK_MAX_TOKENS;
    CHECK(batch_call(&b) == MMT_OK);
    CHECK(b.n_masked[0] > 0 && b.n_masked[0] <= MMT_MASK_MAX_TOKENS);
    batch_free(&b);
  }
  if (wild()) return 1;
  CHECK(g_chosen > 1000);
  printf("mask asan driver ok: %ld calls, %ld refusals, %ld batches of wrong lengths, %ld tokens chosen\n", g_calls, g_refused, g_wild, g_chosen);
  return 0;
}
