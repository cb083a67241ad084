/* C driver of the sanitizer build (`make asan`, CPU only): descriptor validation, error channel and workspace
 * sizing of the C-ABI shim (mmt_api.hip, host side) under -fsanitize=address,undefined.  The kernel launchers are
 * the stand-ins of asan_stubs.cpp: nothing touches a GPU. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/mmt_attn.h"
#include "../../../include/mmt_layer.h"

extern const unsigned char* g_ws_lo;
extern const unsigned char* g_ws_hi;
extern int g_launches, g_last_kind, g_last_handover;
extern const void* g_last_epoch;
extern int g_last_pack;
extern int g_last_family, g_last_tu;   /* backward: 0 general, 1 lean kernels; general launchers: 0 plain, 1 origin, 2 image unit */

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "asan driver: %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, mmt_last_error()); return 1; } } while (0)

static mmt_attn_desc base_desc(int B, int S, int N, int R, int dtype) {
  mmt_attn_desc d;
  memset(&d, 0, sizeof(d));
  d.B = B; d.S = S; d.N = N; d.D = 64; d.R = R; d.dtype = dtype;
  int64_t st[3] = {(int64_t)S * N * 64, (int64_t)N * 64, 64};
  for (int i = 0; i < 3; ++i) d.q_stride[i] = d.k_stride[i] = d.v_stride[i] = d.o_stride[i] = st[i];
  d.scale = 0.125f; d.mask_value = -10000.f;
  d.mask.local_radius = 64; d.mask.id_mode = R ? MMT_IDS_1D : MMT_IDS_NONE; d.mask.max_dist = 12;
  return d;
}

int main(void) {
  char dummy[64];
  CHECK(mmt_abi_version() == MMT_ABI_VERSION);
  /* ---- argument errors: codes + message, no launch ---- */
  CHECK(mmt_attn_fwd(NULL, dummy, dummy, dummy, NULL, NULL, NULL, NULL, dummy, NULL, NULL, 0, NULL) == MMT_E_INVALID);
  CHECK(strstr(mmt_last_error(), "desc is NULL") != NULL);
  mmt_attn_desc d = base_desc(2, 300, 3, 32, MMT_BF16);
  d.D = 32;
  CHECK(mmt_attn_fwd(&d, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, NULL, 0, NULL) == MMT_E_UNSUPPORTED);
  CHECK(mmt_workspace_bytes(&d) == 0);
  d = base_desc(2, 300, 3, 129, MMT_BF16);      /* tables are built up to 128 ids wide */
  CHECK(mmt_attn_fwd(&d, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, NULL, 0, NULL) == MMT_E_UNSUPPORTED);
  d = base_desc(2, 300, 3, 32, MMT_BF16);
  d.q_stride[1] = 7;                         /* not a multiple of 8 elements */
  CHECK(mmt_attn_fwd(&d, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, NULL, 0, NULL) == MMT_E_INVALID);
  d = base_desc(2, 300, 3, 32, MMT_BF16);
  d.mask.global_start = 290; d.mask.n_global = 20;   /* range past the sequence */
  CHECK(mmt_attn_fwd(&d, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, NULL, 0, NULL) == MMT_E_INVALID);
  d = base_desc(2, 300, 3, 32, MMT_BF16);
  d.dropout_p = 1.0f;
  CHECK(mmt_attn_fwd(&d, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, NULL, 0, NULL) == MMT_E_INVALID);
  d = base_desc(2, 300, 3, 32, MMT_BF16);
  CHECK(mmt_attn_fwd(&d, NULL, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, NULL, 0, NULL) == MMT_E_INVALID);
  CHECK(mmt_attn_fwd(&d, dummy, dummy, dummy, NULL, NULL, NULL, NULL, dummy, NULL, NULL, 0, NULL) == MMT_E_INVALID);   /* R > 0, no table */
  int32_t gidx[3] = {3, 9, 200};
  d.mask.global_index = gidx; d.mask.n_global = 3;
  CHECK(mmt_attn_fwd(&d, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, NULL, 0, NULL) == MMT_E_UNSUPPORTED);
  CHECK(strstr(mmt_last_error(), "listed global-token set") != NULL);
  CHECK(g_launches == 0);

  /* ---- workspace sizing: every derived pointer stays inside what mmt_workspace_bytes asked for ---- */
  static const int shapes[][6] = {   /* B, S, N, R, n_global, dtype */
      {1, 20, 1, 9, 1, MMT_F32},  {2, 300, 3, 32, 8, MMT_BF16}, {1, 1024, 2, 32, 8, MMT_F32},
      {4, 4096, 12, 32, 8, MMT_BF16}, {2, 8192, 12, 32, 128, MMT_BF16}, {1, 513, 5, 49, 40, MMT_BF16},
      {1, 96, 1, 0, 0, MMT_BF16}};
  for (unsigned i = 0; i < sizeof(shapes) / sizeof(shapes[0]); ++i) {
    const int* s = shapes[i];
    d = base_desc(s[0], s[1], s[2], s[3], s[5]);
    d.mask.n_global = s[4]; d.mask.global_start = s[4] ? s[1] / 2 - s[4] / 2 : 0;
    const size_t need = mmt_workspace_bytes(&d);
    CHECK(need > 0 || s[4] == 0);
    unsigned char* ws = (unsigned char*)malloc(need ? need : 1);    /* exact size: an overrun is an ASan report */
    CHECK(ws != NULL);
    g_ws_lo = ws; g_ws_hi = ws + need;
    const int before = g_launches;
    if (need > 16) {   /* one byte short is refused, with the requirement in the message */
      CHECK(mmt_attn_bwd(&d, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, dummy, (const float*)dummy, dummy, dummy, dummy,
                         (float*)dummy, NULL, ws, need - 1, NULL) == MMT_E_WORKSPACE);
      CHECK(g_launches == before);
    }
    CHECK(mmt_attn_fwd(&d, dummy, dummy, dummy, s[3] ? dummy : NULL, NULL, NULL, NULL, dummy, (float*)dummy, ws, need, NULL) == MMT_OK);
    CHECK(mmt_attn_bwd(&d, dummy, dummy, dummy, s[3] ? dummy : NULL, NULL, NULL, NULL, dummy, dummy, (const float*)dummy, dummy, dummy, dummy,
                       s[3] ? (float*)dummy : NULL, NULL, ws, need, NULL) == MMT_OK);
    CHECK(g_launches > before);
    CHECK(g_last_kind == 5 && g_last_family == (s[5] == MMT_BF16));   /* f32: the general kernels (plain unit); these bf16 shapes: the lean ones */
    CHECK(s[5] == MMT_BF16 || g_last_tu == 0);
    free(ws);
  }

  /* ---- image grid (ABI 4): the general kernels, forward and backward, whatever the tuning switches ---- */
  {
    const uint32_t tunings[] = {0u, MMT_TUNE_FWD_WALK, MMT_TUNE_FWD_PWIN, MMT_TUNE_FWD_FORCE_WIN, MMT_TUNE_BWD_HO_PER_WAVE};
    for (unsigned t = 0; t < sizeof(tunings) / sizeof(tunings[0]); ++t) {
      d = base_desc(4, 4096, 12, 32, MMT_BF16);
      d.mask.patches_per_row = 63; d.mask.image_grid = MMT_IMAGE_GRID(1, 2);
      d.tuning = tunings[t];
      uint32_t sync[48] = {0};
      d.sync = sync; d.sync_words = 48;
      const size_t need = mmt_workspace_bytes(&d);
      unsigned char* ws = (unsigned char*)malloc(need);
      CHECK(ws != NULL);
      g_ws_lo = ws; g_ws_hi = ws + need;
      CHECK(mmt_attn_fwd(&d, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, (float*)dummy, ws, need, NULL) == MMT_OK);
      CHECK(g_last_kind == 1);      /* the general kernel: no lean, window, walk or sliding-window kernel */
      CHECK(g_last_tu == 0);
      CHECK(mmt_attn_bwd(&d, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, dummy, (const float*)dummy, dummy, dummy, dummy,
                         (float*)dummy, NULL, ws, need, NULL) == MMT_OK);
      CHECK(g_last_kind == 5 && g_last_handover == 0);
      CHECK(g_last_family == 0 && g_last_tu == 0);
      free(ws);
    }
  }

  /* ---- head size 128: the general kernels, forward and backward, whatever the tuning switches; every derived
   *      workspace pointer inside what mmt_workspace_bytes asked for (exact-size allocations) ---- */
  {
    static const int shapes[][8] = {   /* B, S, N, R, n_global, dtype, 2-D ids, grid radius */
        {2, 512, 2, 9, 8, MMT_BF16, 0, 0},   {1, 300, 3, 0, 0, MMT_F32, 0, 0},  {2, 1024, 2, 49, 0, MMT_BF16, 1, 0},
        {1, 4096, 6, 100, 8, MMT_BF16, 0, 0}, {2, 200, 2, 32, 8, MMT_F32, 0, 0}, {1, 640, 2, 32, 8, MMT_BF16, 0, 1},
        {1, 520, 1, 100, 40, MMT_BF16, 1, 2}};
    const uint32_t tunings[] = {0u, MMT_TUNE_FWD_WALK, MMT_TUNE_FWD_PWIN, MMT_TUNE_FWD_FORCE_WIN, MMT_TUNE_BWD_HO_PER_WAVE};
    for (unsigned i = 0; i < sizeof(shapes) / sizeof(shapes[0]); ++i) {
      for (unsigned t = 0; t < sizeof(tunings) / sizeof(tunings[0]); ++t) {
        const int* s = shapes[i];
        d = base_desc(s[0], s[1], s[2], s[3], s[5]);
        d.D = 128;
        const int64_t st[3] = {(int64_t)s[1] * s[2] * 128, (int64_t)s[2] * 128, 128};
        for (int j = 0; j < 3; ++j) d.q_stride[j] = d.k_stride[j] = d.v_stride[j] = d.o_stride[j] = st[j];
        d.mask.n_global = s[4]; d.mask.global_start = s[4] ? s[1] / 2 - s[4] / 2 : 0;
        if (s[6]) { d.mask.id_mode = MMT_IDS_2D; d.mask.patches_per_row = 16; d.mask.core_layers = 1; }
        if (s[7]) { d.mask.patches_per_row = 16; d.mask.image_grid = MMT_IMAGE_GRID(s[7], 2); }
        d.tuning = tunings[t];
        uint32_t sync[16] = {0};
        d.sync = sync; d.sync_words = 16;
        const size_t need = mmt_workspace_bytes(&d);
        CHECK(need > 0);
        unsigned char* ws = (unsigned char*)malloc(need);
        CHECK(ws != NULL);
        g_ws_lo = ws; g_ws_hi = ws + need;
        CHECK(mmt_attn_fwd(&d, dummy, dummy, dummy, s[3] ? dummy : NULL, NULL, NULL, NULL, dummy, (float*)dummy, ws, need, NULL) == MMT_OK);
        CHECK(g_last_kind == (s[4] ? 4 : 1));    /* the general kernel (+ its global-rows combine) */
        CHECK(mmt_attn_bwd(&d, dummy, dummy, dummy, s[3] ? dummy : NULL, NULL, NULL, NULL, dummy, dummy, (const float*)dummy, dummy, dummy, dummy,
                           s[3] ? (float*)dummy : NULL, NULL, ws, need, NULL) == MMT_OK);
        CHECK(g_last_kind == 5 && g_last_handover == 0);
        CHECK(g_last_family == 0 && g_last_tu == 0);
        /* the dense operator (att_mask given) */
        CHECK(mmt_attn_fwd(&d, dummy, dummy, dummy, s[3] ? dummy : NULL, NULL, (const int32_t*)dummy, NULL, dummy, (float*)dummy, ws, need, NULL) == MMT_OK);
        CHECK(g_last_kind == 1);
        CHECK(mmt_attn_bwd(&d, dummy, dummy, dummy, s[3] ? dummy : NULL, NULL, (const int32_t*)dummy, NULL, dummy, dummy, (const float*)dummy, dummy, dummy, dummy,
                           s[3] ? (float*)dummy : NULL, NULL, ws, need, NULL) == MMT_OK);
        free(ws);
      }
    }
    const int refused[] = {0, 32, 96, 256};
    for (unsigned i = 0; i < sizeof(refused) / sizeof(refused[0]); ++i) {
      d = base_desc(2, 300, 3, 32, MMT_BF16);
      d.D = refused[i];
      CHECK(mmt_workspace_bytes(&d) == 0);
      CHECK(strstr(mmt_last_error(), "head size 64") != NULL);
    }
  }

  /* ---- packed examples (MMT_FLAG_EXAMPLE_IDS): mask.valid_len names [B,S] example ids; the general kernels, forward and
   *      backward, whatever the tuning switches; exact-size workspaces; the argument errors ---- */
  {
    static const int shapes[][8] = {   /* B, S, N, R, n_global, dtype, 2-D ids, D */
        {4, 4096, 12, 32, 8, MMT_BF16, 0, 64}, {2, 300, 3, 32, 0, MMT_F32, 0, 64}, {2, 1024, 2, 49, 8, MMT_BF16, 1, 64},
        {1, 520, 1, 100, 40, MMT_BF16, 1, 128}, {1, 96, 1, 0, 0, MMT_BF16, 0, 64}, {1, 1000, 2, 32, 8, MMT_F32, 0, 128}};
    const uint32_t tunings[] = {0u, MMT_TUNE_FWD_WALK, MMT_TUNE_FWD_PWIN, MMT_TUNE_FWD_ROWS_ONE_WG, MMT_TUNE_FWD_NO_WIN, MMT_TUNE_FWD_FORCE_WIN,
                                MMT_TUNE_BWD_NO_HANDOVER, MMT_TUNE_BWD_HO_PER_WAVE, MMT_TUNE_BWD_NO_PEEL_DQ, MMT_TUNE_BWD_NO_PEEL_DKV,
                                MMT_TUNE_BWD_DQ_PLANE_MAJOR};
    for (unsigned i = 0; i < sizeof(shapes) / sizeof(shapes[0]); ++i) {
      for (unsigned t = 0; t < sizeof(tunings) / sizeof(tunings[0]); ++t) {
        const int* s = shapes[i];
        d = base_desc(s[0], s[1], s[2], s[3], s[5]);
        d.D = s[7];
        const int64_t st[3] = {(int64_t)s[1] * s[2] * s[7], (int64_t)s[2] * s[7], s[7]};
        for (int j = 0; j < 3; ++j) d.q_stride[j] = d.k_stride[j] = d.v_stride[j] = d.o_stride[j] = st[j];
        d.mask.n_global = s[4]; d.mask.global_start = s[4] ? s[1] / 2 - s[4] / 2 : 0;
        if (s[6]) { d.mask.id_mode = MMT_IDS_2D; d.mask.patches_per_row = 16; d.mask.core_layers = 1; }
        d.flags = MMT_FLAG_EXAMPLE_IDS | (t & 1 ? MMT_FLAG_SCALE_BEFORE_ADD : 0u);
        d.mask.valid_len = (const int32_t*)dummy;      /* the [B,S] ids (never read on the host) */
        d.tuning = tunings[t];
        uint32_t sync[48] = {0};
        d.sync = sync; d.sync_words = 48;
        const size_t need = mmt_workspace_bytes(&d);
        CHECK(need > 0);
        unsigned char* ws = (unsigned char*)malloc(need);
        CHECK(ws != NULL);
        g_ws_lo = ws; g_ws_hi = ws + need;
        CHECK(mmt_attn_fwd(&d, dummy, dummy, dummy, s[3] ? dummy : NULL, NULL, NULL, NULL, dummy, (float*)dummy, ws, need, NULL) == MMT_OK);
        CHECK(g_last_kind == (s[4] ? 4 : 1) && g_last_pack == 1);   /* the general kernel (+ its global-rows combine) */
        CHECK(mmt_attn_bwd(&d, dummy, dummy, dummy, s[3] ? dummy : NULL, NULL, NULL, NULL, dummy, dummy, (const float*)dummy, dummy, dummy, dummy,
                           s[3] ? (float*)dummy : NULL, NULL, ws, need, NULL) == MMT_OK);
        CHECK(g_last_kind == 5 && g_last_handover == 0 && g_last_pack == 1);
        CHECK(g_last_family == 0 && g_last_tu == 0);
        CHECK(mmt_attn_bwd(&d, dummy, dummy, dummy, s[3] ? dummy : NULL, NULL, NULL, NULL, dummy, dummy, (const float*)dummy, dummy, dummy, dummy,
                           s[3] ? (float*)dummy : NULL, NULL, ws, need - 1, NULL) == MMT_E_WORKSPACE);
        /* with a dense att_mask the flag is ignored like the rest of desc->mask */
        CHECK(mmt_attn_fwd(&d, dummy, dummy, dummy, s[3] ? dummy : NULL, NULL, (const int32_t*)dummy, NULL, dummy, (float*)dummy, ws, need, NULL) == MMT_OK);
        CHECK(g_last_kind == 1 && g_last_pack == 0);
        CHECK(mmt_attn_bwd(&d, dummy, dummy, dummy, s[3] ? dummy : NULL, NULL, (const int32_t*)dummy, NULL, dummy, dummy, (const float*)dummy, dummy, dummy, dummy,
                           s[3] ? (float*)dummy : NULL, NULL, ws, need, NULL) == MMT_OK);
        CHECK(g_last_pack == 0);
        free(ws);
      }
    }
    const int before = g_launches;
    d = base_desc(2, 300, 3, 32, MMT_BF16);
    d.flags = MMT_FLAG_EXAMPLE_IDS;                 /* flag without the ids */
    CHECK(mmt_workspace_bytes(&d) == 0);
    CHECK(strstr(mmt_last_error(), "example ids") != NULL);
    CHECK(mmt_attn_fwd(&d, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, dummy, 64, NULL) == MMT_E_INVALID);
    CHECK(strstr(mmt_last_error(), "example ids") != NULL);
    CHECK(mmt_attn_bwd(&d, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, dummy, (const float*)dummy, dummy, dummy, dummy,
                       (float*)dummy, NULL, dummy, 64, NULL) == MMT_E_INVALID);
    d.mask.valid_len = (const int32_t*)dummy;       /* ids with an image grid */
    d.mask.patches_per_row = 16; d.mask.image_grid = MMT_IMAGE_GRID(1, 2);
    CHECK(mmt_workspace_bytes(&d) == 0);
    CHECK(mmt_attn_fwd(&d, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, dummy, 64, NULL) == MMT_E_UNSUPPORTED);
    CHECK(strstr(mmt_last_error(), "image grid") != NULL);
    CHECK(mmt_attn_bwd(&d, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, dummy, (const float*)dummy, dummy, dummy, dummy,
                       (float*)dummy, NULL, dummy, 64, NULL) == MMT_E_UNSUPPORTED);
    d.mask.image_grid = 0;                          /* ids with a listed global set: refused as without them */
    int32_t listed[3] = {3, 9, 200};
    d.mask.global_index = listed; d.mask.n_global = 3;
    CHECK(mmt_attn_fwd(&d, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, dummy, 64, NULL) == MMT_E_UNSUPPORTED);
    CHECK(strstr(mmt_last_error(), "listed global-token set") != NULL);
    CHECK(g_launches == before);
  }

  /* ---- the general kernels' translation units: example starts -> origin unit; MMT_IDS_2D_IMAGE away from origin 0 -> image
   *      unit (whatever the packing), unless the lean kernels hold the ids (bf16, head size 64, no grid, no packing) ---- */
  {
    static const int cases[][6] = {   /* dtype, D, pack flags, 2-D image ids at origin 2, expected family, expected unit */
        {MMT_BF16, 64, MMT_FLAG_EXAMPLE_IDS | MMT_FLAG_EXAMPLE_STARTS, 0, 0, 1}, {MMT_F32, 128, MMT_FLAG_EXAMPLE_IDS | MMT_FLAG_EXAMPLE_STARTS, 0, 0, 1},
        {MMT_BF16, 64, MMT_FLAG_EXAMPLE_IDS | MMT_FLAG_EXAMPLE_STARTS, 1, 0, 2}, {MMT_BF16, 64, MMT_FLAG_EXAMPLE_IDS, 1, 0, 2},
        {MMT_F32, 64, 0, 1, 0, 2}, {MMT_BF16, 128, 0, 1, 0, 2}, {MMT_BF16, 64, 0, 1, 1, 0}};
    for (unsigned i = 0; i < sizeof(cases) / sizeof(cases[0]); ++i) {
      const int* s = cases[i];
      d = base_desc(2, 512, 2, 49, s[0]);
      d.D = s[1];
      const int64_t st[3] = {(int64_t)512 * 2 * s[1], (int64_t)2 * s[1], s[1]};
      for (int j = 0; j < 3; ++j) d.q_stride[j] = d.k_stride[j] = d.v_stride[j] = d.o_stride[j] = st[j];
      d.flags = (uint32_t)s[2];
      if (s[2]) d.mask.valid_len = (const int32_t*)dummy;
      if (s[3]) { d.mask.id_mode = MMT_IDS_2D_IMAGE; d.mask.patches_per_row = 4; d.mask.core_layers = 1; d.mask.max_dist = 3; d.mask.image_grid = MMT_IMAGE_GRID(0, 2); }
      const size_t need = mmt_workspace_bytes(&d);
      CHECK(need > 0);
      unsigned char* ws = (unsigned char*)malloc(need);
      CHECK(ws != NULL);
      g_ws_lo = ws; g_ws_hi = ws + need;
      CHECK(mmt_attn_fwd(&d, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, (float*)dummy, ws, need, NULL) == MMT_OK);
      CHECK(s[4] ? g_last_kind == 2 : (g_last_kind == 1 && g_last_tu == s[5]));
      CHECK(mmt_attn_bwd(&d, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, dummy, (const float*)dummy, dummy, dummy, dummy,
                         (float*)dummy, NULL, ws, need, NULL) == MMT_OK);
      CHECK(g_last_kind == 5 && g_last_family == s[4] && (s[4] || g_last_tu == s[5]));
      free(ws);
    }
  }

  /* ---- side inputs: the reference generator's argument errors (feature_utils.py:60-65) ---- */
  mmt_mask_desc m;
  memset(&m, 0, sizeof(m));
  m.id_mode = MMT_IDS_2D; m.patches_per_row = 0; m.core_layers = 1; m.max_dist = 3;
  CHECK(mmt_side_inputs(&m, 1, 64, NULL, NULL, 0, NULL, (int32_t*)dummy, NULL, NULL) == MMT_E_INVALID);
  CHECK(strstr(mmt_last_error(), "num_patch_per_row") != NULL);
  m.patches_per_row = 4; m.core_layers = 0;
  CHECK(mmt_side_inputs(&m, 1, 64, NULL, NULL, 0, NULL, (int32_t*)dummy, NULL, NULL) == MMT_E_INVALID);
  m.core_layers = 1; m.max_dist = -1;
  CHECK(mmt_side_inputs(&m, 1, 64, NULL, NULL, 0, NULL, (int32_t*)dummy, NULL, NULL) == MMT_E_INVALID);
  m.max_dist = 3;
  CHECK(mmt_side_inputs(&m, 1, 8, NULL, NULL, 0, NULL, (int32_t*)dummy, NULL, NULL) == MMT_E_INVALID);   /* image longer than S */
  CHECK(mmt_side_inputs(&m, 1, 64, NULL, NULL, 0, NULL, (int32_t*)dummy, NULL, NULL) == MMT_OK && g_last_kind == 6);
  CHECK(mmt_side_inputs(NULL, 1, 64, NULL, NULL, 0, NULL, NULL, NULL, NULL) == MMT_E_INVALID);
  /* ---- per-step scalars in device memory (ABI 4: named by the descriptors, no registration in the library) ---- */
  CHECK(mmt_write_step_scalars(NULL, NULL, 1, 1e-4f, 0.1f, 0.001f, NULL) == MMT_E_INVALID);
  CHECK(mmt_write_step_scalars((uint64_t*)dummy, (float*)dummy, 1, 1e-4f, 0.1f, 0.001f, NULL) == MMT_OK && g_last_kind == 7);
  {   /* two descriptors with different epoch words in one process: each launch gets its own */
    uint64_t epoch_a = 1, epoch_b = 2;
    mmt_attn_desc da = base_desc(1, 256, 2, 32, MMT_BF16), db = base_desc(1, 256, 2, 32, MMT_BF16);
    da.dropout_p = db.dropout_p = 0.1f;
    da.dropout_epoch = &epoch_a; db.dropout_epoch = &epoch_b;
    unsigned char* ws = (unsigned char*)malloc(mmt_workspace_bytes(&da) + 1);
    g_ws_lo = ws; g_ws_hi = ws + mmt_workspace_bytes(&da) + 1;
    CHECK(mmt_attn_fwd(&da, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, ws, mmt_workspace_bytes(&da), NULL) == MMT_OK);
    CHECK(g_last_epoch == (const void*)&epoch_a);
    CHECK(mmt_attn_fwd(&db, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, ws, mmt_workspace_bytes(&db), NULL) == MMT_OK);
    CHECK(g_last_epoch == (const void*)&epoch_b);
    CHECK(mmt_attn_bwd(&da, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, dummy, (const float*)dummy, dummy, dummy, dummy,
                       (float*)dummy, NULL, ws, mmt_workspace_bytes(&da), NULL) == MMT_OK);
    CHECK(g_last_epoch == (const void*)&epoch_a);
    db.dropout_p = 0.f;                       /* no dropout: the word is not even passed on */
    CHECK(mmt_attn_fwd(&db, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, ws, mmt_workspace_bytes(&db), NULL) == MMT_OK);
    CHECK(g_last_epoch == NULL);
    /* kernel-selection switches travel in the descriptor too (they were environment variables until ABI 3) */
    da.tuning = MMT_TUNE_FWD_NO_WIN;
    CHECK(mmt_attn_fwd(&da, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, ws, mmt_workspace_bytes(&da), NULL) == MMT_OK && g_last_kind == 2);
    da.tuning = MMT_TUNE_FWD_FORCE_WIN;
    CHECK(mmt_attn_fwd(&da, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, ws, mmt_workspace_bytes(&da), NULL) == MMT_OK && g_last_kind == 3);
    {   /* the plane-walk forward needs the caller's arrival counters when there are global tokens (ABI 4: desc.sync) */
      mmt_attn_desc dw = base_desc(4, 4096, 12, 32, MMT_BF16);
      dw.mask.n_global = 8; dw.mask.global_start = 3971;
      const size_t need = mmt_workspace_bytes(&dw);
      unsigned char* w2 = (unsigned char*)malloc(need);
      g_ws_lo = w2; g_ws_hi = w2 + need;
      CHECK(mmt_attn_fwd(&dw, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, w2, need, NULL) == MMT_OK && g_last_kind == 3);   /* default: window kernel */
      dw.tuning = MMT_TUNE_FWD_WALK;                             /* asked for, but no counters: still the window kernel */
      CHECK(mmt_attn_fwd(&dw, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, w2, need, NULL) == MMT_OK && g_last_kind == 3);
      dw.sync = (uint32_t*)dummy; dw.sync_words = 47;            /* too few words for 48 planes */
      CHECK(mmt_attn_fwd(&dw, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, w2, need, NULL) == MMT_OK && g_last_kind == 3);
      dw.sync_words = 48;
      CHECK(mmt_attn_fwd(&dw, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, w2, need, NULL) == MMT_OK && g_last_kind == 8);
      dw.tuning = MMT_TUNE_FWD_PWIN;                             /* likewise opt-in: the sliding-window kernel */
      CHECK(mmt_attn_fwd(&dw, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, w2, need, NULL) == MMT_OK && g_last_kind == 9);
      dw.tuning = 0;                                             /* the default stays the window kernel, counters or not */
      CHECK(mmt_attn_fwd(&dw, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, NULL, w2, need, NULL) == MMT_OK && g_last_kind == 3);
      free(w2);
      g_ws_lo = ws; g_ws_hi = ws + mmt_workspace_bytes(&da) + 1;
    }
    da.tuning = MMT_TUNE_BWD_NO_HANDOVER;
    CHECK(mmt_attn_bwd(&da, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, dummy, (const float*)dummy, dummy, dummy, dummy,
                       (float*)dummy, NULL, ws, mmt_workspace_bytes(&da), NULL) == MMT_OK && g_last_handover == 0);
    da.tuning = 0;
    CHECK(mmt_attn_bwd(&da, dummy, dummy, dummy, dummy, NULL, NULL, NULL, dummy, dummy, (const float*)dummy, dummy, dummy, dummy,
                       (float*)dummy, NULL, ws, mmt_workspace_bytes(&da), NULL) == MMT_OK && g_last_handover == 1);
    free(ws);
  }
  /* ---- RandAugment (mmt_rand_augment): every refusal, then one accepted call on an exact-size workspace ---- */
  {
    enum { NB = 5, NBYTES = 1000 };
    uint8_t* in = (uint8_t*)malloc(NBYTES);
    uint8_t* out = (uint8_t*)malloc(NBYTES);
    uint8_t* both = (uint8_t*)malloc(2 * NBYTES - 1);
    const size_t need = mmt_rand_augment_workspace_bytes(NB);
    unsigned char* ws = (unsigned char*)malloc(need);
    CHECK(in && out && both && ws);
    CHECK(mmt_rand_augment_workspace_bytes(0) == 0 && mmt_rand_augment_workspace_bytes(-1) == 0);
    CHECK(need == (size_t)NB * 4 * 256 * 4);
    const int64_t* offs = (const int64_t*)dummy;
    const int32_t* i32 = (const int32_t*)dummy;
    const float* f32 = (const float*)dummy;
    g_ws_lo = ws; g_ws_hi = ws + need;
    const int before = g_launches;
    CHECK(mmt_rand_augment(0, in, NBYTES, offs, i32, i32, i32, f32, out, ws, need, NULL) == MMT_E_INVALID);
    CHECK(strstr(mmt_last_error(), "must be positive") != NULL);
    CHECK(mmt_rand_augment(-4, in, NBYTES, offs, i32, i32, i32, f32, out, ws, need, NULL) == MMT_E_INVALID);
    CHECK(mmt_rand_augment(NB, NULL, NBYTES, offs, i32, i32, i32, f32, out, ws, need, NULL) == MMT_E_INVALID);
    CHECK(strstr(mmt_last_error(), "NULL argument") != NULL);
    CHECK(mmt_rand_augment(NB, in, NBYTES, NULL, i32, i32, i32, f32, out, ws, need, NULL) == MMT_E_INVALID);
    CHECK(mmt_rand_augment(NB, in, NBYTES, offs, NULL, i32, i32, f32, out, ws, need, NULL) == MMT_E_INVALID);
    CHECK(mmt_rand_augment(NB, in, NBYTES, offs, i32, NULL, i32, f32, out, ws, need, NULL) == MMT_E_INVALID);
    CHECK(mmt_rand_augment(NB, in, NBYTES, offs, i32, i32, NULL, f32, out, ws, need, NULL) == MMT_E_INVALID);
    CHECK(mmt_rand_augment(NB, in, NBYTES, offs, i32, i32, i32, NULL, out, ws, need, NULL) == MMT_E_INVALID);
    CHECK(mmt_rand_augment(NB, in, NBYTES, offs, i32, i32, i32, f32, NULL, ws, need, NULL) == MMT_E_INVALID);
    CHECK(mmt_rand_augment(NB, in, 0, offs, i32, i32, i32, f32, out, ws, need, NULL) == MMT_E_INVALID);
    CHECK(strstr(mmt_last_error(), "pixels_bytes") != NULL);
    CHECK(mmt_rand_augment(NB, in, -1, offs, i32, i32, i32, f32, out, ws, need, NULL) == MMT_E_INVALID);
    CHECK(mmt_rand_augment(NB, in, (int64_t)1 << 60, offs, i32, i32, i32, f32, out, ws, need, NULL) == MMT_E_INVALID);
    CHECK(mmt_rand_augment(NB, in, NBYTES, offs, i32, i32, i32, f32, in, ws, need, NULL) == MMT_E_INVALID);          /* in place */
    CHECK(strstr(mmt_last_error(), "overlaps") != NULL);
    CHECK(mmt_rand_augment(NB, both, NBYTES, offs, i32, i32, i32, f32, both + NBYTES - 1, ws, need, NULL) == MMT_E_INVALID);   /* one byte shared */
    CHECK(mmt_rand_augment(NB, both + NBYTES - 1, NBYTES, offs, i32, i32, i32, f32, both, ws, need, NULL) == MMT_E_INVALID);
    CHECK(mmt_rand_augment(NB, in, NBYTES, offs, i32, i32, i32, f32, out, NULL, need, NULL) == MMT_E_WORKSPACE);
    CHECK(mmt_rand_augment(NB, in, NBYTES, offs, i32, i32, i32, f32, out, ws, need - 1, NULL) == MMT_E_WORKSPACE);
    CHECK(strstr(mmt_last_error(), "bytes needed") != NULL);
    CHECK(mmt_rand_augment(NB, in, NBYTES, offs, i32, i32, i32, f32, out, ws, 0, NULL) == MMT_E_WORKSPACE);
    CHECK(g_launches == before);
    CHECK(mmt_rand_augment(NB, in, NBYTES, offs, i32, i32, i32, f32, out, ws, need, NULL) == MMT_OK);
    CHECK(g_launches == before + 1 && g_last_kind == 10);
    CHECK(mmt_rand_augment(NB, both, NBYTES - 1, offs, i32, i32, i32, f32, both + NBYTES - 1, ws, need, NULL) == MMT_OK);      /* adjacent, not overlapping */
    free(in); free(out); free(both); free(ws);
  }
  /* ---- text front end: the vocabulary builder on exact-size buffers (every slot and byte it writes is inside what
   *      mmt_wordpiece_vocab_bytes asked for), its refusals, then every refusal of mmt_text_tokens and one accepted call ---- */
  {
    static const char* toks[] = {"[PAD]", "[UNK]", "[SEP]", "a", "ab", "abc", "##b", "##bc", "##", "#", "\xc3\xa9t\xc3\xa9", "##\xe4\xb8\xad", "\xf0\x9f\x98\x80"};
    enum { NT = sizeof(toks) / sizeof(toks[0]) };
    int64_t offs[NT + 1];
    size_t nb = 0;
    for (int i = 0; i < NT; ++i) { offs[i] = (int64_t)nb; nb += strlen(toks[i]); }
    offs[NT] = (int64_t)nb;
    uint8_t* tb = (uint8_t*)malloc(nb);
    CHECK(tb != NULL);
    for (int i = 0; i < NT; ++i) memcpy(tb + offs[i], toks[i], strlen(toks[i]));
    const size_t vbytes = mmt_wordpiece_vocab_bytes(NT, (int64_t)nb);
    CHECK(vbytes == 32 + 32 * 16 + ((nb + 3) & ~(size_t)3));
    CHECK(mmt_wordpiece_vocab_bytes(0, 0) == 0 && mmt_wordpiece_vocab_bytes(-1, 5) == 0 && mmt_wordpiece_vocab_bytes(4, 3) == 0);
    uint32_t* image = (uint32_t*)malloc(vbytes);
    CHECK(image != NULL);
    CHECK(mmt_wordpiece_vocab_build(NT, tb, offs, image, vbytes) == MMT_OK);
    CHECK(image[1] == NT && image[2] == 32 && image[3] == 8 + 4 * 32);
    { unsigned used = 0; for (unsigned s = 0; s < 32; ++s) used += image[8 + 4 * s] != 0; CHECK(used == NT); }
    CHECK(mmt_wordpiece_vocab_build(NT, tb, offs, image, vbytes - 1) == MMT_E_WORKSPACE);
    CHECK(strstr(mmt_last_error(), "bytes needed") != NULL);
    CHECK(mmt_wordpiece_vocab_build(NT, NULL, offs, image, vbytes) == MMT_E_INVALID);
    CHECK(mmt_wordpiece_vocab_build(NT, tb, NULL, image, vbytes) == MMT_E_INVALID);
    CHECK(mmt_wordpiece_vocab_build(NT, tb, offs, NULL, vbytes) == MMT_E_INVALID);
    CHECK(mmt_wordpiece_vocab_build(0, tb, offs, image, vbytes) == MMT_E_INVALID);
    {
      int64_t bad[4] = {0, 1, 1, 2};                           /* "a", "", "b" */
      CHECK(mmt_wordpiece_vocab_build(3, tb + offs[3], bad, image, vbytes) == MMT_E_INVALID);
      CHECK(strstr(mmt_last_error(), "is empty") != NULL);
      int64_t dec[3] = {0, 2, 1};
      CHECK(mmt_wordpiece_vocab_build(2, tb, dec, image, vbytes) == MMT_E_INVALID);
      const uint8_t dup[] = "ab##bab";                         /* "ab", "##b", "ab" */
      int64_t d3[4] = {0, 2, 5, 7};
      CHECK(mmt_wordpiece_vocab_build(3, dup, d3, image, vbytes) == MMT_E_INVALID);
      CHECK(strstr(mmt_last_error(), "token 2 duplicates token 0") != NULL);
      const uint8_t ill[] = {'a', 0xc0, 0x80};                 /* an overlong form */
      int64_t i2[3] = {0, 1, 3};
      CHECK(mmt_wordpiece_vocab_build(2, ill, i2, image, vbytes) == MMT_E_INVALID);
      CHECK(strstr(mmt_last_error(), "well-formed") != NULL);
    }
    enum { TB = 3, TF = 2, TT = 16, TBUD = 13 };
    const size_t need = mmt_text_tokens_workspace_bytes(TB, TF, TBUD);
    CHECK(need == (size_t)TB * TF * (TBUD + 1) * 4);
    CHECK(mmt_text_tokens_workspace_bytes(0, 1, 1) == 0 && mmt_text_tokens_workspace_bytes(1, 0, 1) == 0 && mmt_text_tokens_workspace_bytes(1, 1, -1) == 0);
    unsigned char* ws = (unsigned char*)malloc(need);
    CHECK(ws != NULL);
    g_ws_lo = ws; g_ws_hi = ws + need;
    int64_t aligned[8] = {0};                                /* the alignment checks want real alignment */
    char* dm = (char*)aligned;
    const uint8_t* by = (const uint8_t*)dm;
    const int64_t* i64 = (const int64_t*)dm;
    const int32_t* i32 = (const int32_t*)dm;
    const uint32_t* cp = (const uint32_t*)dm;
    int32_t* o32 = (int32_t*)dm;
    uint8_t* o8 = (uint8_t*)dm;
    const int32_t ftok[2] = {5, 6};
    const int64_t CPN = 0x110000;
    const int before = g_launches;
#define TEXT(B, F, bytes, offsets, lengths, vocab, vb, table, tn, ft, sep, T, budget, ids, cnt, st, w, wb) \
    mmt_text_tokens(B, F, bytes, 64, offsets, lengths, vocab, vb, table, tn, ft, sep, 1, T, budget, ids, cnt, st, w, wb, NULL)
    CHECK(TEXT(0, TF, by, i64, i32, image, vbytes, cp, CPN, ftok, 2, TT, TBUD, o32, o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(strstr(mmt_last_error(), "must be positive") != NULL);
    CHECK(TEXT(TB, 0, by, i64, i32, image, vbytes, cp, CPN, ftok, 2, TT, TBUD, o32, o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(TEXT(TB, TF, by, i64, i32, image, vbytes, cp, CPN, ftok, 2, 0, 0, o32, o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(TEXT(TB, 17, by, i64, i32, image, vbytes, cp, CPN, ftok, 2, 64, TBUD, o32, o32, o8, ws, need) == MMT_E_UNSUPPORTED);
    CHECK(TEXT(TB, TF, by, i64, i32, image, vbytes, cp, CPN, ftok, 2, TT, TBUD + 1, o32, o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(strstr(mmt_last_error(), "must fit T") != NULL);
    CHECK(TEXT(TB, TF, by, i64, i32, image, vbytes, cp, CPN, ftok, 2, TT, -1, o32, o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(TEXT(TB, TF, NULL, i64, i32, image, vbytes, cp, CPN, ftok, 2, TT, TBUD, o32, o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(strstr(mmt_last_error(), "NULL argument") != NULL);
    CHECK(TEXT(TB, TF, by, NULL, i32, image, vbytes, cp, CPN, ftok, 2, TT, TBUD, o32, o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(TEXT(TB, TF, by, i64, NULL, image, vbytes, cp, CPN, ftok, 2, TT, TBUD, o32, o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(TEXT(TB, TF, by, i64, i32, NULL, vbytes, cp, CPN, ftok, 2, TT, TBUD, o32, o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(TEXT(TB, TF, by, i64, i32, image, vbytes, NULL, CPN, ftok, 2, TT, TBUD, o32, o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(TEXT(TB, TF, by, i64, i32, image, vbytes, cp, CPN, NULL, 2, TT, TBUD, o32, o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(TEXT(TB, TF, by, i64, i32, image, vbytes, cp, CPN, ftok, 2, TT, TBUD, NULL, o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(TEXT(TB, TF, by, i64, i32, image, vbytes, cp, CPN, ftok, 2, TT, TBUD, o32, NULL, o8, ws, need) == MMT_E_INVALID);
    CHECK(TEXT(TB, TF, by, i64, i32, image, vbytes, cp, CPN, ftok, 2, TT, TBUD, o32, o32, NULL, ws, need) == MMT_E_INVALID);
    CHECK(TEXT(TB, TF, by, i64, i32, image, 40, cp, CPN, ftok, 2, TT, TBUD, o32, o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(strstr(mmt_last_error(), "no vocabulary image") != NULL);
    CHECK(TEXT(TB, TF, by, i64, i32, image, vbytes, cp, CPN - 1, ftok, 2, TT, TBUD, o32, o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(strstr(mmt_last_error(), "codepoint_entries") != NULL);
    CHECK(TEXT(TB, TF, by, i64, i32, image, vbytes, cp, CPN, ftok, -2, TT, TBUD, o32, o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(TEXT(TB, TF, by, (const int64_t*)(dm + 4), i32, image, vbytes, cp, CPN, ftok, 2, TT, TBUD, o32, o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(strstr(mmt_last_error(), "aligned") != NULL);
    CHECK(TEXT(TB, TF, by, i64, (const int32_t*)(dm + 2), image, vbytes, cp, CPN, ftok, 2, TT, TBUD, o32, o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(TEXT(TB, TF, by, i64, i32, image, vbytes, cp, CPN, ftok, 2, TT, TBUD, (int32_t*)(dm + 1), o32, o8, ws, need) == MMT_E_INVALID);
    CHECK(TEXT(TB, TF, by, i64, i32, image, vbytes, cp, CPN, ftok, 2, TT, TBUD, o32, o32, o8, ws + 2, need) == MMT_E_INVALID);
    CHECK(TEXT(TB, TF, by, i64, i32, image, vbytes, cp, CPN, ftok, 2, TT, TBUD, o32, o32, o8, NULL, need) == MMT_E_WORKSPACE);
    CHECK(TEXT(TB, TF, by, i64, i32, image, vbytes, cp, CPN, ftok, 2, TT, TBUD, o32, o32, o8, ws, need - 1) == MMT_E_WORKSPACE);
    CHECK(strstr(mmt_last_error(), "bytes needed") != NULL);
    CHECK(g_launches == before);
    CHECK(TEXT(TB, TF, by, i64, i32, image, vbytes, cp, CPN, ftok, 2, TT, TBUD, o32, o32, o8, ws, need) == MMT_OK);
    CHECK(g_launches == before + 1 && g_last_kind == 11);
    CHECK(TEXT(1, 1, by, i64, i32, image, vbytes, cp, CPN, ftok, 2, 2, 0, o32, o32, o8, ws, 4) == MMT_OK);      /* budget 0: counts only */
#undef TEXT
    free(tb); free(image); free(ws);
  }
  printf("asan driver ok: %d stand-in launches, no sanitizer report\n", g_launches);
  return 0;
}
