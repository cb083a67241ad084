/* Route table of the attention dispatch (`make routes`, CPU only): walks a fixed list of descriptors through
 * mmt_workspace_bytes, mmt_attn_fwd and mmt_attn_bwd on the host side of mmt_api.hip and prints, per descriptor, what
 * each returned and which stand-in launchers (asan_stubs.cpp) were called with which routing fields and workspace
 * offsets.  tests/golden/attn_routes.txt is this program's output; tests/test_attn_routes.py compares. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/mmt_attn.h"

extern const unsigned char* g_ws_lo;
extern const unsigned char* g_ws_hi;
extern char g_trace[];
void stub_trace_reset(void);

enum { IDS_NONE, IDS_1D_M3, IDS_1D_M12, IDS_1D_WIDE, IDS_2D, IDS_IMG0, IDS_IMG2, N_IDS };
static const char* const kIdsName[N_IDS] = {"none", "1d-m3", "1d-m12", "1d-R<2m+1", "2d-P4r1", "2dimage@0", "2dimage@2"};
enum { PACK_NONE, PACK_IDS, PACK_STARTS };
#define NG_LISTED (-1)

typedef struct {
  int dtype, D, R, ids, grid, pack, dense, ng, radius, S, sync;
  float dropout;
  uint32_t tuning;
} Case;

static const Case kBase = {MMT_BF16, 64, 32, IDS_1D_M3, 0, PACK_NONE, 0, 8, 64, 512, 1, 0.f, 0u};

static char dummy[64];
static uint32_t sync_words[16];
static int32_t listed[3] = {3, 9, 200};
static int n_case = 0;

static void run(const Case* c) {
  mmt_attn_desc d;
  memset(&d, 0, sizeof(d));
  d.B = 2; d.S = c->S; d.N = 2; d.D = c->D; d.R = c->R; d.dtype = c->dtype;
  const int64_t st[3] = {(int64_t)c->S * 2 * c->D, 2 * c->D, c->D};
  for (int i = 0; i < 3; ++i) d.q_stride[i] = d.k_stride[i] = d.v_stride[i] = d.o_stride[i] = st[i];
  d.scale = 0.125f; d.mask_value = -10000.f;
  d.dropout_p = c->dropout; d.dropout_seed = 7;
  d.tuning = c->tuning;
  if (c->sync) { d.sync = sync_words; d.sync_words = 4; }
  mmt_mask_desc* m = &d.mask;
  m->local_radius = c->radius;
  if (c->ng == NG_LISTED) { m->global_index = listed; m->n_global = 3; }
  else { m->n_global = c->ng; m->global_start = c->ng ? c->S / 2 - c->ng / 2 : 0; }
  int origin = 2;                       /* first image position of the grid word */
  switch (c->ids) {
    case IDS_NONE: m->id_mode = MMT_IDS_NONE; break;
    case IDS_1D_M3: m->id_mode = MMT_IDS_1D; m->max_dist = 3; break;
    case IDS_1D_M12: m->id_mode = MMT_IDS_1D; m->max_dist = 12; break;
    case IDS_1D_WIDE: m->id_mode = MMT_IDS_1D; m->max_dist = c->R > 3 ? c->R : 3; break;    /* 2m + 1 > R */
    case IDS_2D: m->id_mode = MMT_IDS_2D; m->max_dist = 3; m->core_layers = 1; break;
    case IDS_IMG0: m->id_mode = MMT_IDS_2D_IMAGE; m->max_dist = 3; m->core_layers = 1; origin = 0; break;
    case IDS_IMG2: m->id_mode = MMT_IDS_2D_IMAGE; m->max_dist = 3; m->core_layers = 1; break;
  }
  m->patches_per_row = 4;
  if (c->grid || c->ids == IDS_IMG2) m->image_grid = MMT_IMAGE_GRID(c->grid, origin);
  if (c->pack != PACK_NONE) {
    d.flags |= MMT_FLAG_EXAMPLE_IDS | (c->pack == PACK_STARTS ? MMT_FLAG_EXAMPLE_STARTS : 0u);
    m->valid_len = (const int32_t*)dummy;      /* never read on the host */
  }
  /* one line per descriptor: what differs from the base case, then the workspace size and what the forward and the backward
   * did -- or, where an earlier descriptor's did the very same, that one's number (for the whole line if all three agree) */
  static char* seen[3][2048];
  char label[256], part[3][4096 + 640];
  int n = 0;
  label[0] = 0;
#define DIFF(field, fmt, val) if (c->field != kBase.field) n += snprintf(label + n, sizeof(label) - n, " " fmt, val)
  DIFF(dtype, "%s", "f32"); DIFF(D, "D=%d", c->D); DIFF(R, "R=%d", c->R); DIFF(ids, "ids=%s", kIdsName[c->ids]); DIFF(grid, "grid=%d", c->grid);
  DIFF(pack, "pack=%d", c->pack); DIFF(dense, "%s", "dense"); DIFF(ng, "ng=%d", c->ng); DIFF(radius, "radius=%d", c->radius);
  DIFF(S, "S=%d", c->S); DIFF(sync, "%s", "nosync"); DIFF(dropout, "dropout=%g", (double)c->dropout); DIFF(tuning, "tuning=0x%x", c->tuning);
  const size_t need = mmt_workspace_bytes(&d);
  printf("#%d%s:", n_case, label);
  snprintf(part[2], sizeof(part[2]), need ? " %zu" : " %zu \"%s\"", need, mmt_last_error());
  unsigned char* ws = (unsigned char*)malloc(need ? need : 1);    /* exact size: the stand-ins abort on a pointer outside */
  if (!ws) exit(2);
  g_ws_lo = ws; g_ws_hi = ws + need;
  const int32_t* att_mask = c->dense ? (const int32_t*)dummy : NULL;
  const void* emb = c->R ? dummy : NULL;
  stub_trace_reset();
  int rc = mmt_attn_fwd(&d, dummy, dummy, dummy, emb, NULL, att_mask, NULL, dummy, (float*)dummy, need ? ws : NULL, need, NULL);
  if (rc) snprintf(part[0], sizeof(part[0]), " %d \"%s\"", rc, mmt_last_error()); else snprintf(part[0], sizeof(part[0]), "%s", g_trace);
  stub_trace_reset();
  rc = mmt_attn_bwd(&d, dummy, dummy, dummy, emb, NULL, att_mask, NULL, dummy, dummy, (const float*)dummy, dummy, dummy, dummy,
                    c->R ? (float*)dummy : NULL, NULL, need ? ws : NULL, need, NULL);
  if (rc) snprintf(part[1], sizeof(part[1]), " %d \"%s\"", rc, mmt_last_error()); else snprintf(part[1], sizeof(part[1]), "%s", g_trace);
  free(ws);
  static const char* const kPart[3] = {"; fwd", "; bwd", " ws"};
  int same[3];
  for (int k = 0; k < 3; ++k) {
    for (same[k] = 0; same[k] < n_case && strcmp(seen[k][same[k]], part[k]); ) ++same[k];
    seen[k][n_case] = strdup(part[k]);
  }
  if (same[0] < n_case && same[0] == same[1] && same[0] == same[2]) printf(" as #%d", same[0]);
  else
    for (int i = 0; i < 3; ++i) {
      const int k = (i + 2) % 3;      /* ws, fwd, bwd */
      if (same[k] < n_case && strlen(part[k]) > 12) printf("%s as #%d", kPart[k], same[k]); else printf("%s%s", kPart[k], part[k]);
    }
  printf("\n");
  ++n_case;
}

#define COUNT(a) ((int)(sizeof(a) / sizeof((a)[0])))

int main(void) {
  printf("base: bf16 D=64 R=32 ids=1d-m3 grid=0 pack=0 structured ng=8 (mid-sequence) radius=64 B=N=2 S=512 counters dropout=0 tuning=0; "
         "fields at 0 (offsets: -1 = NULL; parts, pscale, bf16: 1) are left out\n");
  static const int dtypes[] = {MMT_BF16, MMT_F32};
  static const int heads[] = {64, 128};
  static const int widths[] = {0, 9, 25, 32, 33, 49, 64, 65, 100, 128};
  static const int globals[] = {0, 1, 8, 9, 16, 17, 40, 200, NG_LISTED};
  static const int radii[] = {16, 32, 64, 96, 1 << 20};
  static const int lengths[] = {96, 512, 4096, 8192};
  static const uint32_t tunings[] = {MMT_TUNE_FWD_WALK, MMT_TUNE_FWD_NO_WIN, MMT_TUNE_FWD_FORCE_WIN, MMT_TUNE_BWD_NO_HANDOVER,
                                     MMT_TUNE_BWD_HO_PER_WAVE, MMT_TUNE_BWD_NO_PEEL_DQ, MMT_TUNE_BWD_NO_PEEL_DKV,
                                     MMT_TUNE_BWD_DQ_PLANE_MAJOR, MMT_TUNE_FWD_PWIN, MMT_TUNE_FWD_ROWS_ONE_WG,
                                     MMT_TUNE_FWD_FORCE_WIN | MMT_TUNE_FWD_ROWS_ONE_WG};
  Case c;
  /* the features that exclude the lean kernels, crossed with each other */
  for (int t = 0; t < 2; ++t) for (int h = 0; h < 2; ++h) for (int g = 0; g < 2; ++g) for (int k = 0; k < 3; ++k)
    for (int dn = 0; dn < 2; ++dn) for (int i = 0; i < N_IDS; ++i) for (int ng = 0; ng <= 8; ng += 8) {
      c = kBase; c.dtype = dtypes[t]; c.D = heads[h]; c.grid = g; c.pack = k; c.dense = dn; c.ids = i; c.ng = ng;
      run(&c);
    }
  /* the table width, crossed with the ids and the dtype */
  for (int w = 0; w < COUNT(widths); ++w) for (int i = 0; i < N_IDS; ++i) for (int t = 0; t < 2; ++t) {
    c = kBase; c.R = widths[w]; c.ids = i; c.dtype = dtypes[t];
    run(&c);
  }
  /* the shape: length, radius, global tokens, arrival counters */
  for (int s = 0; s < COUNT(lengths); ++s) for (int r = 0; r < COUNT(radii); ++r) for (int g = 0; g < COUNT(globals); ++g)
    for (int sy = 1; sy >= 0; --sy) {
      c = kBase; c.S = lengths[s]; c.radius = radii[r]; c.ng = globals[g]; c.sync = sy;
      run(&c);
    }
  /* the tuning switches */
  for (int t = 0; t < COUNT(tunings); ++t) for (int s = 1; s <= 3; s += 2) for (int r = 1; r <= 2; ++r) for (int g = 0; g <= 16; g += 8) {
    c = kBase; c.tuning = tunings[t]; c.S = lengths[s]; c.radius = radii[r]; c.ng = g;
    run(&c);
  }
  /* dropout (the lean kernels leave 1 / keep of the global rows to the combine) */
  for (int t = 0; t < 2; ++t) for (int s = 1; s <= 3; s += 2) for (int g = 0; g < COUNT(globals); g += 2) {
    if (globals[g] > 40) break;               /* 0, 8, 16, 40 */
    c = kBase; c.dropout = 0.1f; c.dtype = dtypes[t]; c.S = lengths[s]; c.ng = globals[g];
    run(&c);
  }
  return 0;
}
