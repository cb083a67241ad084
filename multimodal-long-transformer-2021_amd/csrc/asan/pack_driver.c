/* C driver of the sanitizer build of the row packing's host side (`make asan-pack`, CPU only): the argument checks of
 * pack_rows.hip and mmt_pack_rows_host -- the functions of pack_rows.h that the kernels run, as plain loops -- under
 * -fsanitize=address,undefined.  Every input, output and the workspace lives in a heap block of exactly the size the
 * library was told, so a read or write past either is reported.  The rows are checked against a restatement of the
 * next-fit rule that walks the examples once and knows nothing of prefix sums or searches.  Nothing touches a GPU. */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/mmt_attn.h"
#include "../../../include/mmt_layer.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "pack asan driver: %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, mmt_last_error()); return 1; } } while (0)

static long g_calls, g_refused, g_wild;

static void* block(size_t n) {                         /* exactly n bytes */
  void* p = malloc(n ? n : 1);
  if (!p) abort();
  memset(p, 0x5A, n);
  return p;
}

static uint32_t g_rng = 2463534242u;
static uint32_t rnd(void) { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

typedef struct batch {
  mmt_pack_desc d;
  int32_t *word, *seg, *len, *mlm, *mpp;
  int32_t *o_word, *o_seg, *ids, *starts, *slots, *o_mlm, *o_mpp, *consumed;
  int64_t* first;
  float* weight;
  void* ws;
  size_t ws_bytes;
} batch;

static void batch_make(batch* b, int E, int S, int R, int S_row, int E_max, int n_mlm, int n_mpp) {
  memset(b, 0, sizeof *b);
  b->d.E = E; b->d.S = S; b->d.R = R; b->d.S_row = S_row; b->d.E_max = E_max; b->d.n_mlm = n_mlm; b->d.n_mpp = n_mpp;
  const size_t rows = (size_t)R * S_row * 4;
  b->word = (int32_t*)block((size_t)E * S * 4); b->seg = (int32_t*)block((size_t)E * S * 4); b->len = (int32_t*)block((size_t)E * 4);
  b->mlm = n_mlm ? (int32_t*)block((size_t)E * n_mlm * 4) : NULL; b->mpp = n_mpp ? (int32_t*)block((size_t)E * n_mpp * 4) : NULL;
  b->o_word = (int32_t*)block(rows); b->o_seg = (int32_t*)block(rows); b->ids = (int32_t*)block(rows);
  b->starts = (int32_t*)block(rows); b->slots = (int32_t*)block(rows);
  b->first = (int64_t*)block((size_t)E_max * 16); b->weight = (float*)block((size_t)E_max * 4);
  b->o_mlm = n_mlm ? (int32_t*)block((size_t)E_max * n_mlm * 4) : NULL; b->o_mpp = n_mpp ? (int32_t*)block((size_t)E_max * n_mpp * 4) : NULL;
  b->consumed = (int32_t*)block(4);
  b->ws_bytes = mmt_pack_rows_workspace_bytes(&b->d);
  b->ws = block(b->ws_bytes);
  for (long i = 0; i < (long)E * S; ++i) { b->word[i] = (int32_t)(1 + rnd() % 30000u); b->seg[i] = (int32_t)(rnd() % 3u); }
}

static void batch_free(batch* b) {
  free(b->word); free(b->seg); free(b->len); free(b->mlm); free(b->mpp); free(b->o_word); free(b->o_seg); free(b->ids);
  free(b->starts); free(b->slots); free(b->first); free(b->weight); free(b->o_mlm); free(b->o_mpp); free(b->consumed); free(b->ws);
}

static int batch_call(batch* b) {
  ++g_calls;
  return mmt_pack_rows_host(&b->d, b->word, b->seg, b->len, b->mlm, b->mpp, b->o_word, b->o_seg, b->ids, b->starts, b->slots,
                            b->first, b->weight, b->o_mlm, b->o_mpp, b->consumed, b->ws, b->ws_bytes);
}

static int clampi(long x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : (int)x); }

/* The rule, walked once: fills the expected rows into freshly zeroed arrays and compares everything. */
static int batch_verify(const batch* b, int positions_in_range) {
  const mmt_pack_desc* d = &b->d;
  const long n = (long)d->R * d->S_row;
  int32_t *word = (int32_t*)calloc((size_t)n, 4), *seg = (int32_t*)calloc((size_t)n, 4), *ids = (int32_t*)calloc((size_t)n, 4),
          *starts = (int32_t*)calloc((size_t)n, 4), *slots = (int32_t*)malloc((size_t)n * 4);
  int* row_of = (int*)calloc((size_t)d->E_max, sizeof(int)); int* first_of = (int*)calloc((size_t)d->E_max, sizeof(int));
  int* count = (int*)calloc((size_t)d->R, sizeof(int)); int* used_of = (int*)calloc((size_t)d->R, sizeof(int));
  for (long i = 0; i < n; ++i) slots[i] = -1;
  int row = 0, used = 0, taken = 0;
  for (int e = 0; e < d->E && e < d->E_max; ++e) {
    const int len = clampi(b->len[e], 1, d->S);
    if (used + len > d->S_row) {
      if (row + 1 == d->R) break;
      ++row; used = 0;
    }
    row_of[e] = row; first_of[e] = used;
    for (int s = 0; s < len; ++s) {
      const long o = (long)row * d->S_row + used + s;
      word[o] = b->word[(long)e * d->S + s]; seg[o] = b->seg[(long)e * d->S + s]; starts[o] = used; slots[o] = e;
    }
    used += len; ++count[row]; used_of[row] = used; ++taken;
  }
  for (int e = 0; e < taken; ++e) {                    /* ids fall from the row's count to 1 */
    const int len = clampi(b->len[e], 1, d->S);
    int rank = 0;
    for (int f = e; f < taken && row_of[f] == row_of[e]; ++f) ++rank;
    for (int s = 0; s < len; ++s) ids[(long)row_of[e] * d->S_row + first_of[e] + s] = rank;
  }
  for (int r = 0; r < d->R; ++r)
    for (int s = used_of[r]; s < d->S_row; ++s) starts[(long)r * d->S_row + s] = used_of[r];
  int ok = b->consumed[0] == taken && !memcmp(word, b->o_word, (size_t)n * 4) && !memcmp(seg, b->o_seg, (size_t)n * 4) &&
           !memcmp(ids, b->ids, (size_t)n * 4) && !memcmp(starts, b->starts, (size_t)n * 4) && !memcmp(slots, b->slots, (size_t)n * 4);
  for (int e = 0; e < d->E_max && ok; ++e) {
    const int here = e < taken;
    ok = b->first[2 * e] == (here ? row_of[e] : 0) && b->first[2 * e + 1] == (here ? first_of[e] : 0) && b->weight[e] == (here ? 1.f : 0.f);
    for (int k = 0; k < 2 && ok; ++k) {
      const int32_t* in = k ? b->mpp : b->mlm; const int32_t* out = k ? b->o_mpp : b->o_mlm; const int cols = k ? d->n_mpp : d->n_mlm;
      for (int j = 0; in && j < cols && ok; ++j) {
        const long got = out[(long)e * cols + j];
        if (!here) ok = got == 0;
        else if (positions_in_range) ok = got == (long)row_of[e] * d->S_row + first_of[e] + in[(long)e * cols + j];
        else ok = got >= 0 && got < n;
      }
    }
  }
  free(word); free(seg); free(ids); free(starts); free(slots); free(row_of); free(first_of); free(count); free(used_of);
  return ok;
}

static int run_case(int S, int S_row, int R, int E_max, const int32_t* lengths, int E, int n_mlm, int n_mpp) {
  batch b;
  batch_make(&b, E, S, R, S_row, E_max, n_mlm, n_mpp);
  memcpy(b.len, lengths, (size_t)E * 4);
  for (int e = 0; e < E; ++e) {
    const int len = clampi(lengths[e], 1, S);
    for (int j = 0; j < n_mlm; ++j) b.mlm[e * n_mlm + j] = (int32_t)(rnd() % (uint32_t)len);
    for (int j = 0; j < n_mpp; ++j) b.mpp[e * n_mpp + j] = (int32_t)(rnd() % (uint32_t)len);
  }
  CHECK(batch_call(&b) == MMT_OK);
  CHECK(batch_verify(&b, 1));
  batch_free(&b);
  return 0;
}

static int refusals(void) {
  batch b;
  batch_make(&b, 3, 8, 2, 16, 4, 2, 0);
  b.len[0] = b.len[1] = b.len[2] = 5; memset(b.mlm, 0, 3 * 2 * 4);
  CHECK(batch_call(&b) == MMT_OK && b.consumed[0] == 3);
#define REFUSED(stmt, undo, code, text) do { stmt; CHECK(batch_call(&b) == (code)); CHECK(strstr(mmt_last_error(), text) != NULL); undo; ++g_refused; } while (0)
  void* keep;
  REFUSED(keep = b.word; b.word = NULL, b.word = (int32_t*)keep, MMT_E_INVALID, "NULL argument");
  REFUSED(keep = b.len; b.len = NULL, b.len = (int32_t*)keep, MMT_E_INVALID, "NULL argument");
  REFUSED(keep = b.slots; b.slots = NULL, b.slots = (int32_t*)keep, MMT_E_INVALID, "NULL argument");
  REFUSED(keep = b.consumed; b.consumed = NULL, b.consumed = (int32_t*)keep, MMT_E_INVALID, "NULL argument");
  REFUSED(b.d.E = 0, b.d.E = 3, MMT_E_INVALID, "at least 1");
  REFUSED(b.d.R = -1, b.d.R = 2, MMT_E_INVALID, "at least 1");
  REFUSED(b.d.E_max = 0, b.d.E_max = 4, MMT_E_INVALID, "at least 1");
  REFUSED(b.d.S_row = 7, b.d.S_row = 16, MMT_E_INVALID, "at least S");
  REFUSED(b.d.E = MMT_PACK_MAX_EXAMPLES + 1, b.d.E = 3, MMT_E_INVALID, "MMT_PACK_MAX_EXAMPLES");
  REFUSED(b.d.E_max = INT_MAX, b.d.E_max = 4, MMT_E_INVALID, "MMT_PACK_MAX_EXAMPLES");
  REFUSED(b.d.R = INT_MAX, b.d.R = 2, MMT_E_INVALID, "below 2^31");
  REFUSED(b.d.n_mlm = 0, b.d.n_mlm = 2, MMT_E_INVALID, "a position table needs");
  REFUSED(keep = b.o_mlm; b.o_mlm = NULL, b.o_mlm = (int32_t*)keep, MMT_E_INVALID, "a position table needs");
  REFUSED(b.ws_bytes -= 1, b.ws_bytes += 1, MMT_E_WORKSPACE, "workspace of");
  CHECK(mmt_pack_rows_host(NULL, b.word, b.seg, b.len, b.mlm, b.mpp, b.o_word, b.o_seg, b.ids, b.starts, b.slots, b.first, b.weight,
                           b.o_mlm, b.o_mpp, b.consumed, b.ws, b.ws_bytes) == MMT_E_INVALID);
  CHECK(batch_call(&b) == MMT_OK && batch_verify(&b, 1));
  batch_free(&b);
  return 0;
}

/* Wrong lengths and positions of every kind: the rows are still those of the clamped lengths, and nothing leaves a block. */
static int wild(void) {
  static const int32_t odd[] = {0, -1, 1, INT_MIN, INT_MAX, 7, 8, 9, 1 << 20, -(1 << 20)};
  for (int round = 0; round < 300; ++round) {
    const int S = 1 + (int)(rnd() % 12u), S_row = S + (int)(rnd() % 20u), R = 1 + (int)(rnd() % 6u), E = 1 + (int)(rnd() % 40u);
    const int E_max = 1 + (int)(rnd() % 48u), n_mlm = (int)(rnd() % 4u), n_mpp = (int)(rnd() % 3u);
    batch b;
    batch_make(&b, E, S, R, S_row, E_max, n_mlm, n_mpp);
    for (int e = 0; e < E; ++e) b.len[e] = (rnd() & 1u) ? odd[rnd() % 10u] : (int32_t)(rnd() % (uint32_t)(S + 3));
    for (int i = 0; i < E * n_mlm; ++i) b.mlm[i] = (rnd() & 1u) ? odd[rnd() % 10u] : (int32_t)rnd();
    for (int i = 0; i < E * n_mpp; ++i) b.mpp[i] = (rnd() & 1u) ? odd[rnd() % 10u] : (int32_t)rnd();
    CHECK(batch_call(&b) == MMT_OK);
    CHECK(batch_verify(&b, 0));
    batch_free(&b);
    ++g_wild;
  }
  return 0;
}

int main(void) {
  if (refusals()) return 1;
  { const int32_t l[] = {5, 6, 7, 3, 8}; if (run_case(8, 20, 3, 8, l, 5, 3, 2)) return 1; }               /* all fit, absent slots */
  { const int32_t l[] = {8, 8, 4, 6, 6, 2}; if (run_case(8, 16, 3, 5, l, 6, 3, 2)) return 1; }            /* a row filled exactly */
  { const int32_t l[] = {8, 7, 2, 8, 8, 1}; if (run_case(8, 16, 3, 6, l, 6, 3, 0)) return 1; }            /* one over opens a row */
  { const int32_t l[] = {8, 7, 2, 8, 8, 1, 3, 3, 3}; if (run_case(8, 16, 2, 9, l, 9, 0, 2)) return 1; }   /* the stop at row R */
  { const int32_t l[] = {5, 6, 7, 3, 8}; if (run_case(8, 64, 2, 3, l, 5, 0, 0)) return 1; }               /* the stop at E_max */
  { const int32_t l[] = {6}; if (run_case(8, 11, 2, 1, l, 1, 3, 2)) return 1; }                           /* E = 1 */
  { const int32_t l[] = {4, 8, 7, 5}; if (run_case(8, 19, 1, 6, l, 4, 3, 2)) return 1; }                  /* R = 1 */
  { const int32_t l[] = {12, 3, 12, 9, 3}; if (run_case(12, 12, 4, 5, l, 5, 3, 2)) return 1; }            /* a length equal to S_row */
  { const int32_t l[] = {0, -5, 100, 3, INT_MAX, INT_MIN, 8}; if (run_case(8, 16, 4, 7, l, 7, 3, 2)) return 1; }
  {                                                                                                       /* the limit */
    int32_t* l = (int32_t*)malloc(MMT_PACK_MAX_EXAMPLES * 4);
    for (int e = 0; e < MMT_PACK_MAX_EXAMPLES; ++e) l[e] = (int32_t)(1 + rnd() % 4u);
    const int rc = run_case(4, 8, 2100, MMT_PACK_MAX_EXAMPLES, l, MMT_PACK_MAX_EXAMPLES, 1, 1);
    free(l);
    if (rc) return 1;
  }
  if (wild()) return 1;
  printf("pack asan driver ok: %ld calls, %ld refusals, %ld batches of wrong lengths and positions\n", g_calls, g_refused, g_wild);
  return 0;
}
