// Forward of QkvRelativeAttention for gfx950 (MI355X).
//
// Replaces the dense einsum / one-hot / softmax chain the reference runs behind
// `RelativeTransformerLayers(inputs, att_mask, relative_att_ids)`
// (src/modeling/models/mmt_encoder.py:220-224; math: SURVEY.md App. A.3) with a
// flash-style kernel that never materialises [S,S] tensors:
//
//   one wave = 32 query rows of one (batch, head); it walks 32-key tiles.
//   S^T = K.Q^T by MFMA (keys in registers, query row on the lane), relative scores are
//   gathered from a per-wave LDS table T[q][col(id)] = (q.E[id] + bias[id]) built once per
//   q-block by MFMA, softmax state is lane-local, O^T += V^T.P^T by MFMA with the P
//   accumulator reused as the B operand (no LDS round trip for P) and V^T fragments read
//   with ds_read_b64_tr_b16 from a wave-private, bank-swizzled LDS tile.  The next tile's
//   K fragments and V rows are prefetched into registers while the current tile computes.
//
// Work items of one launch
//   band items : 32 query rows x (band tiles U global-key tiles), final output        [K1]
//   rows items : 32 global query rows x one chunk of keys, partial (O,m,l) output     [K2]
//   (kDense)   : literal reference operator, att_mask / rel_ids int32 [B,S,S] from HBM [K3]
#include "attn_tile.h"

namespace mmt {

// MMT_IMAGE_TU (this file compiled as attn_fwd_image.hip): the id-generating instantiations a third time, with the image
// origin of MMT_IDS_2D_IMAGE (ids_go) read by rel_id, under a kernel name of their own.  Every other instantiation never
// reads the origin and is the kernel it was.
#ifdef MMT_IMAGE_TU
#define attn_fwd_kernel attn_fwd_image_kernel
constexpr bool kImageTU = true;
#else
constexpr bool kImageTU = false;
#endif

// GEN = true: ids/mask through the generic per-element generators (2-D ids, or 1-D ids whose
// vocabulary is smaller than 2m+1); GEN = false: no ids or 1-D ids with the permuted table.
// GRID = true (kBand only): the pattern has the image-grid term -- the tile walk is GridWalk's union and the
// per-element mask ORs in_grid; GRID = false instantiations (every pattern without a grid) are the kernels as before.
// DH = head size, 64 or 128: fragments and V tile scale with it; DH = 128 adds the O accumulators o2, o3.
// PACK = true (kBand without a grid only): packed examples -- p.valid_len names the [B,S] example ids, the segmented term
// is ids[q] == ids[k], and the walk is PackWalk's: key tiles with no id in the row block's id range are never fetched.
// PACK = false instantiations are the kernels as before.
// ORG = true (PACK only; attn_fwd_origin.hip): per-example origin -- p.valid_len names [B,2,S], the ids and each position's
// example start; rel_id and the grid term take the positions local to their example (lq = q - start[q], lk likewise), the
// band and the dropout hash keep row positions.  With GRID the walk is PackWalk's in both cases -- candidates judged
// eight at a time by the id-range test -- over the span of GridWalk's union around the example's image, keeping the
// tiles of that union, for a block whose 32 rows lie in one example (so the walk is cut to the example: with ids that
// name one run each, nothing outside it passes the test), and over every tile of the row for a block that straddles
// examples.  No rows items: n_global > 0 comes with GLB only.
// GLB = true (ORG only; attn_fwd_globals.hip, MMT_FLAG_EXAMPLE_GLOBALS): per-example global tokens -- the global term reads
// local positions, global(lq) || global(lk).  Per-example global rows are scattered over the row, so there are no rows items
// and no split-rows plan; the band item walks, with or without a grid, the way the ORG + GRID forms do:
//   a row of the block is a global row  -> every tile of the row is a candidate, the id-range test cuts the walk to the
//                                          block's example(s), which it walks whole;
//   else, one example in the block      -> GridWalk's union (band, the tiles of [start + g0, start + g0 + ng), grid
//                                          intervals) over its span, kept where has() names the tile;
//   else (several examples)             -> the tiles from the lowest to the highest that any row's band or global range
//                                          touches (PackWalk::span_globals; with a grid the whole row), id-range filtered.
// Candidates ascend and each is judged once: no tile is visited twice.  All three are supersets of the allowed pairs;
// the element test decides.  GLB = false instantiations are the kernels as before.
// The ORG bf16 head-size-64 forms are held to two workgroups per CU (256 VGPRs): left to itself the allocator takes 260 for
// some of them and halves the occupancy (207 -> 363 us at 16 x 256, 2-D ids).
template <typename T, int MODE, int Rp, bool GEN, bool GRID, int DH, bool PACK = false, bool ORG = false, bool GLB = false>
__global__ __launch_bounds__(256, (ORG && sizeof(T) == 2 && DH == 64) ? 2 : 1) void attn_fwd_kernel(const FwdParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  unsigned char* wl = smem + wave * WaveLds<T, Rp, DH>::kBytes;
  float* tab = reinterpret_cast<float*>(wl);
  unsigned char* vlds = wl + WaveLds<T, Rp, DH>::kTBytesAligned;

  // ---- which 32 query rows does this wave own? ------------------------------------
  const int n_tiles = (p.S + 31) >> 5;
  const int nqb = (p.S + 127) >> 7;
  const bool rows_item = MODE == kBand && (int)blockIdx.x >= p.n_band_blocks;
  int bn, q0, chunk = 0, rowblk = 0;
  if (rows_item) {
    const int per_bn = (p.n_chunks * p.n_rowblk + 3) >> 2;
    const int rb = blockIdx.x - p.n_band_blocks;
    bn = rb / per_bn;
    const int item = (rb - bn * per_bn) * 4 + wave;
    if (item >= p.n_chunks * p.n_rowblk) return;
    rowblk = item / p.n_chunks;
    chunk = item - rowblk * p.n_chunks;
    q0 = p.pat.g0 + rowblk * 32;
  } else {
    const int wg = xcd_remap(blockIdx.x, p.n_band_blocks);
    bn = wg / nqb;
    q0 = (wg - bn * nqb) * 128 + wave * 32;
    if (q0 >= p.S) return;
  }
  const int b = bn / p.N, n = bn - b * p.N;
  const int q = q0 + r;
  const bool q_ok = q < p.S;
  const int valid_len = PACK ? 0 : (p.valid_len ? p.valid_len[b] : p.S);
  constexpr bool CUR = GRID || PACK;      // the walk is a cursor (t_cur, t_nxt), not a count
  constexpr bool OG = ORG && (GRID || GLB);   // origin + grid / per-example globals: GridWalk (one example in the rows) or PackWalk over the row

  const T* Q = reinterpret_cast<const T*>(p.q) + (long)b * p.qs[0] + (long)n * p.qs[2];
  const T* K = reinterpret_cast<const T*>(p.k) + (long)b * p.ks[0] + (long)n * p.ks[2];
  const T* V = reinterpret_cast<const T*>(p.v) + (long)b * p.vs[0] + (long)n * p.vs[2];
  // row offsets inside one (b, n) plane fit 32 bits (checked on the host)
  const unsigned qs1 = (unsigned)p.qs[1], ks1 = (unsigned)p.ks[1], vs1 = (unsigned)p.vs[1];

  // ---- tile walk: [a0, a0+lenA) U [b0, b0+lenB) U [c0, c0+lenC), ascending ------------
  int a0 = 0, lenA = 0, b0 = 0, lenB = n_tiles, c0 = 0, lenC = 0;
  if (MODE == kBand) {
    if (rows_item) {
      b0 = chunk * p.chunk_tiles;
      lenB = min(n_tiles, b0 + p.chunk_tiles) - b0;
    } else if (OG) {
      // every tile of the row is a candidate (b0 = 0, lenB = n_tiles)
    } else {
      const int lo = max(q0 - p.pat.radius, 0), hi = min(q0 + 31 + p.pat.radius, p.S - 1);
      b0 = lo >> 5;
      const int b1 = hi >> 5;
      lenB = b1 - b0 + 1;
      if (p.pat.ng > 0) {
        const int g_lo = p.pat.g0 >> 5, g_hi = (p.pat.g0 + p.pat.ng - 1) >> 5;
        a0 = g_lo; lenA = max(0, min(g_hi, b0 - 1) - g_lo + 1);
        c0 = max(g_lo, b1 + 1); lenC = max(0, g_hi - c0 + 1);
      }
    }
  }
  const int n_it = lenA + lenB + lenC;
  auto tile_at = [&](int it) {
    return it < lenA ? a0 + it : (it < lenA + lenB ? b0 + (it - lenA) : c0 + (it - lenA - lenB));
  };
  // GRID: the walk is a cursor over GridWalk's union (t_cur, and t_nxt found under the tile's math); n_it unused
  GridWalk gw;
  int t_cur = 0, t_nxt = 0;
  if constexpr (GRID && !ORG) {
    if (rows_item) gw.init_chunk(b0, b0 + lenB - 1);
    else gw.init_band(p.pat, p.grid, q0, p.S);
    t_cur = gw.next(0);
  }
  // PACK: the row's own id, the cursor over the tiles that can hold an allowed pair, and id r of the current / next tile.
  // A chunk of the global rows may have no such tile: its partial is then the empty one (max = -inf, sum = 0, O = 0),
  // which the combine takes as long as all chunks are reduced in one pass (<= 64 of them); beyond, nothing is left out.
  PackWalk pw;
  bool one_ex = false;                         // OG: the block's rows lie in one example
  auto og_next = [&]() {                       // OG: next candidate the id-range test lets through (one_ex: of GridWalk's union)
    int t = pw.next(tile_at, lane);
    while (one_ex && t != PackWalk::kEnd && !gw.has(t)) t = pw.next(tile_at, lane);
    return t;
  };
  int qid = 0, kid = 0, kid_nxt = 0;
  int qst = 0, lq = 0, kst = 0, kst_nxt = 0;   // ORG: the row's example start and local position, start r of the current / next tile
  if constexpr (PACK) {
    const int32_t* ids = p.valid_len + (long)b * (ORG ? 2 : 1) * p.S;
    qid = ids[min(q, p.S - 1)];
    pw.init(ids, qid, p.S, n_it, !rows_item || p.n_chunks <= 64);
    if constexpr (ORG) {
      qst = pw.start_at(q);
      lq = local_pos(q, qst, p.S);
    }
    if constexpr (OG) {
      const int st0 = __builtin_amdgcn_readfirstlane(qst);
      one_ex = pw.lo == pw.hi && __all(qst == st0);
      bool grow = false;                       // GLB: a row of the block is a global row -- it sees its whole example
      if constexpr (GLB) {
        grow = __any(q_ok && is_global(p.pat, lq));      // (rows past S take the last row's start: not rows)
        one_ex = one_ex && !grow;
      }
      if (one_ex) {
        int t_hi;
        gw.init_origin(p.pat, p.grid, q0, p.S, st0);
        if constexpr (GLB) gw.init_origin_globals(p.pat, p.S, st0);
        gw.span(b0, t_hi);
        lenB = t_hi - b0 + 1;
        pw.n_it = lenB;
      } else if constexpr (GLB && !GRID) {
        if (!grow) {
          int t_hi;
          pw.span_globals(p.pat, q0, qst, b0, t_hi);
          lenB = t_hi - b0 + 1;
          pw.n_it = lenB;
        }
      }
      t_cur = og_next();
    } else {
      t_cur = pw.next(tile_at, lane);
    }
    if (t_cur != PackWalk::kEnd) {
      kid = pw.id_at(t_cur * 32 + r);
      if constexpr (ORG) kst = pw.start_at(t_cur * 32 + r);
    }
  }

  Frag<T, DH> qf;
  qf.load_row(Q + (unsigned)min(q, p.S - 1) * qs1, h);

  // prefetch of the first tile overlaps the table construction
  Frag<T, DH> kf;
  VTile<T, DH> vt;
  {
    const int k0 = (PACK && t_cur == PackWalk::kEnd) ? 0 : (CUR ? t_cur : tile_at(0)) * 32;
    kf.load_row(K + (unsigned)min(k0 + r, p.S - 1) * ks1, h);
    vt.load(V, vs1, k0, p.S, lane, 0);
  }

  // ---- relative-score table T[q][col(id)] = (q.E[id] + bias[id]) * tscale  (log2 domain) --
  const int id_mode = p.pat.id_mode, mdist = p.pat.m;
  if (p.R > 0) {
    const T* E = reinterpret_cast<const T*>(p.emb) + (long)n * DH;
#pragma unroll
    for (int rb = 0; rb < Rp / 32; ++rb) {
      const int rr = rb * 32 + r;
      Frag<T, DH> ef;
      ef.load_row(E + (long)min(rr, p.R - 1) * p.N * DH, h);   // columns >= R are never read
      f32x16 c = {0};
      c = mma_rows(ef, qf, c);  // [id x q]
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int id = rb * 32 + kap(i, h);
        float bias = 0.f;
        if (p.bias) bias = (float)reinterpret_cast<const T*>(p.bias)[(long)min(id, p.R - 1) * p.N + n];
        const int col = (MODE == kDense || GEN) ? id : tcol(p.perm_1d, mdist, id);
        tab[r * kTStride(Rp) + col] = (c[i] + bias) * p.tscale;
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();

  f32x16 o0 = {0}, o1 = {0};
  f32x16 o2 = {0}, o3 = {0};   // DH = 128: head dims 64 .. 127
  float m_run = -INFINITY, l_run = 0.f;
  const float* trow = tab + r * kTStride(Rp);
  // whole q-block on one side of valid_len?  (needed for the fast path)
  const bool qblk_valid = q0 + 31 < valid_len, qblk_pad = q0 >= valid_len;
  // (GLB: a tile the fast path takes lies inside one example and inside the band -- every pair is allowed, global or not)
  const bool qblk_plain = q0 + 31 < p.S && (GLB || !(p.pat.ng > 0 && q0 + 31 >= p.pat.g0 && q0 < p.pat.g0 + p.pat.ng));

  for (int it = 0; CUR ? t_cur != GridWalk::kEnd : it < n_it; ++it, t_cur = t_nxt, kid = kid_nxt, kst = kst_nxt) {
    const int k0 = (CUR ? t_cur : tile_at(it)) * 32;
    vt.to_lds(vlds, lane);

    f32x16 c = {0};
    c = mma_rows(kf, qf, c);

    VTile<T, DH> vcur;
    if constexpr (sizeof(T) == 4) vcur = vt;
    if constexpr (OG) t_nxt = og_next();
    else if constexpr (GRID) t_nxt = gw.next(t_cur + 1);
    else if constexpr (PACK) t_nxt = pw.next(tile_at, lane);
    if (CUR ? t_nxt != GridWalk::kEnd : it + 1 < n_it) {   // prefetch the next tile (registers) under this tile's math
      const int k1 = (CUR ? t_nxt : tile_at(it + 1)) * 32;
      kf.load_row(K + (unsigned)min(k1 + r, p.S - 1) * ks1, h);
      vt.load(V, vs1, k1, p.S, lane, 0);
      if constexpr (PACK) kid_nxt = pw.id_at(k1 + r);
      if constexpr (ORG) kst_nxt = pw.start_at(k1 + r);
    }

    // ---- scores in the log2 domain --------------------------------------------------------
    float s2[16];
    float tmax = -INFINITY;
    bool fast = false;
    if (MODE == kBand) {
      // wave-uniform classification: every (q,k) of the tile unmasked and 1-D (or no) ids
      bool seg_all;
      if constexpr (PACK) seg_all = pw.lo == pw.hi && __all(kid == pw.lo);    // one example in the rows and in the keys
      else seg_all = (qblk_valid && k0 + 31 < valid_len) || (qblk_pad && k0 >= valid_len);
      const bool band_all = (k0 - (q0 + 31) >= -p.pat.radius) && (k0 + 31 - q0 <= p.pat.radius);
      fast = !GEN && seg_all && band_all && qblk_plain && k0 + 31 < p.S;
    }
    constexpr bool cheap_ids = MODE == kBand && !GEN;
    if (!GEN && fast) {
      const int d0 = k0 - q + 4 * h;
      if (id_mode == 1) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int d = d0 + (i & 3) + 8 * (i >> 2);
          const int col = min(max(d, -mdist), mdist) + mdist;  // < R: perm_1d implies R >= 2m+1
          s2[i] = fmaf(c[i], p.sscale, trow[col]);
          tmax = fmaxf(tmax, s2[i]);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) { s2[i] = c[i] * p.sscale; tmax = fmaxf(tmax, s2[i]); }
      }
    } else if constexpr (cheap_ids) {
      // branch-free pattern mask, 1-D (permuted table) or no ids
      const int kb = k0 + 4 * h, d0 = kb - q;
      const unsigned W = (unsigned)p.pat.radius;
      const bool qv = q < valid_len, gq = is_global(p.pat, GLB ? lq : q);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int ci = (i & 3) + 8 * (i >> 2);
        const int kk = kb + ci, d = d0 + ci;
        const bool near = (unsigned)(d + (int)W) <= 2u * W;
        const bool gk = (unsigned)(kk - p.pat.g0) < (unsigned)p.pat.ng;
        const bool seg = PACK ? __shfl(kid, 4 * h + ci, 64) == qid : (kk < valid_len) == qv;
        bool keep;
        if constexpr (GLB) {
          const int lk = local_pos(kk, __shfl(kst, 4 * h + ci, 64), p.S);
          keep = (int)seg & ((int)near | (int)gq | (int)is_global(p.pat, lk) | (int)(GRID && in_grid(p.pat, p.grid, lq, lk)));
        }
        else if constexpr (ORG) keep = (int)seg & ((int)near | (int)(GRID && in_grid(p.pat, p.grid, lq, local_pos(kk, __shfl(kst, 4 * h + ci, 64), p.S))));
        else keep = (int)seg & ((int)near | (int)gk | (int)gq | (int)(GRID && in_grid(p.pat, p.grid, q, kk)));
        float rel = 0.f;
        if (id_mode == 1) rel = trow[min(max(d, -mdist), mdist) + mdist];
        float s = fmaf(c[i], p.sscale, rel);
        s = keep ? s : s + p.mask_add;
        s = kk < p.S ? s : -INFINITY;
        s2[i] = s;
        tmax = fmaxf(tmax, s);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int kk = k0 + kap(i, h);
        bool keep;
        int id = -1;
        if (MODE == kDense) {
          const long off = ((long)b * p.S + (q_ok ? q : 0)) * p.S + (kk < p.S ? kk : 0);
          keep = p.att_mask ? p.att_mask[off] != 0 : true;
          if (p.rel_ids) id = p.rel_ids[off];
        } else {
          int lk = kk;
          if constexpr (ORG) lk = local_pos(kk, __shfl(kst, kap(i, h), 64), p.S);
          if constexpr (ORG) keep = pattern_mask_origin<GRID, GLB>(p.pat, p.grid, __shfl(kid, kap(i, h), 64) == qid, q, kk, lq, lk);
          else if constexpr (PACK) keep = pattern_mask_packed(p.pat, __shfl(kid, kap(i, h), 64) == qid, q, kk);
          else keep = pattern_mask<GRID>(p.pat, p.grid, valid_len, q, kk);
          if (id_mode) id = ORG ? rel_id<kImageTU>(p.pat, lq, lk, p.ids_go) : rel_id<kImageTU>(p.pat, q, kk, p.ids_go);
        }
        float rel = 0.f;
        if ((unsigned)id < (unsigned)p.R) rel = trow[id];
        float s = fmaf(c[i], p.sscale, rel);
        if (!keep) s += p.mask_add;
        if (kk >= p.S) s = -INFINITY;
        s2[i] = s;
        tmax = fmaxf(tmax, s);
      }
    }
    tmax = half_max(tmax);
    // Deferred rescale: the running reference m_run only moves when some row's tile maximum
    // exceeds it by more than kRescaleThr (log2 units), so p stays <= 2^kRescaleThr; O, l and
    // p always share one reference, hence the normalised result is unchanged.
    if (__any(tmax > m_run + kRescaleThr)) {
      const float m_new = fmaxf(m_run, tmax);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      l_run *= alpha;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        o0[i] *= alpha; o1[i] *= alpha;
        if constexpr (DH == 128) { o2[i] *= alpha; o3[i] *= alpha; }
      }
    }
    float psum = 0.f;
    float pr[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      pr[i] = __builtin_amdgcn_exp2f(s2[i] - m_run);
      psum += pr[i];
    }
    l_run += psum;

    if (p.drop_thresh) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint32_t bits = drop_bits16(drop_row_base(effective_seed(p.seed_lo, p.seed_hi, p.epoch).lo, effective_seed(p.seed_lo, p.seed_hi, p.epoch).hi, (uint32_t)bn, (uint32_t)q),
                                          (uint32_t)(k0 + kap(i, h)));
        pr[i] = bits >= p.drop_thresh ? pr[i] * p.inv_keep : 0.f;
      }
    }

    // ---- O^T[d x q] += V^T[d x key] . P^T[key x q] -------------------------------------------
    if constexpr (DH == 128) {
      if constexpr (sizeof(T) == 2) mma_xt(o0, o1, o2, o3, vt, vlds, pr, lane);
      else mma_xt(o0, o1, o2, o3, vcur, vlds, pr, lane);
    } else {
      if constexpr (sizeof(T) == 2) mma_xt(o0, o1, vt, vlds, pr, lane);
      else mma_xt(o0, o1, vcur, vlds, pr, lane);
    }
  }

  // ---- epilogue --------------------------------------------------------------------------
  const float l_tot = half_sum(l_run);
  if (rows_item) {
    // partial, unnormalised: part_o[bn][rowblk][chunk][q 32][d DH], part_ml[...][2][32]
    const long slot = ((long)bn * p.n_rowblk + rowblk) * p.n_chunks + chunk;
    float* po = p.part_o + slot * (32 * DH) + r * DH;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      *reinterpret_cast<f32x4*>(po + 8 * g + 4 * h) = f32x4{o0[4 * g], o0[4 * g + 1], o0[4 * g + 2], o0[4 * g + 3]};
      *reinterpret_cast<f32x4*>(po + 32 + 8 * g + 4 * h) = f32x4{o1[4 * g], o1[4 * g + 1], o1[4 * g + 2], o1[4 * g + 3]};
      if constexpr (DH == 128) {
        *reinterpret_cast<f32x4*>(po + 64 + 8 * g + 4 * h) = f32x4{o2[4 * g], o2[4 * g + 1], o2[4 * g + 2], o2[4 * g + 3]};
        *reinterpret_cast<f32x4*>(po + 96 + 8 * g + 4 * h) = f32x4{o3[4 * g], o3[4 * g + 1], o3[4 * g + 2], o3[4 * g + 3]};
      }
    }
    if (h == 0) {
      p.part_ml[slot * 64 + r] = m_run;
      p.part_ml[slot * 64 + 32 + r] = l_tot;
    }
    return;
  }
  if (!q_ok) return;
  if (MODE == kBand && p.skip_global_rows && is_global(p.pat, q)) return;
  const float inv = 1.f / l_tot;
  T* O = reinterpret_cast<T*>(p.out) + (long)b * p.os[0] + (long)q * p.os[1] + (long)n * p.os[2];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int d = 8 * g + 4 * h;
    if constexpr (sizeof(T) == 2) {
      bf16x4 a, c2;
#pragma unroll
      for (int j = 0; j < 4; ++j) { a[j] = (__bf16)(o0[4 * g + j] * inv); c2[j] = (__bf16)(o1[4 * g + j] * inv); }
      *reinterpret_cast<bf16x4*>(O + d) = a;
      *reinterpret_cast<bf16x4*>(O + 32 + d) = c2;
      if constexpr (DH == 128) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { a[j] = (__bf16)(o2[4 * g + j] * inv); c2[j] = (__bf16)(o3[4 * g + j] * inv); }
        *reinterpret_cast<bf16x4*>(O + 64 + d) = a;
        *reinterpret_cast<bf16x4*>(O + 96 + d) = c2;
      }
    } else {
      *reinterpret_cast<f32x4*>(O + d) = f32x4{o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv};
      *reinterpret_cast<f32x4*>(O + 32 + d) = f32x4{o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv};
      if constexpr (DH == 128) {
        *reinterpret_cast<f32x4*>(O + 64 + d) = f32x4{o2[4 * g] * inv, o2[4 * g + 1] * inv, o2[4 * g + 2] * inv, o2[4 * g + 3] * inv};
        *reinterpret_cast<f32x4*>(O + 96 + d) = f32x4{o3[4 * g] * inv, o3[4 * g + 1] * inv, o3[4 * g + 2] * inv, o3[4 * g + 3] * inv};
      }
    }
  }
  if (p.lse && h == 0) p.lse[((long)b * p.N + n) * p.S + q] = (m_run + log2f(l_tot)) * kLn2;
}

// Combine the per-chunk partials of the global rows: DH threads per (row, bn), thread = d (at DH = 128 each of the two
// waves reduces the chunk statistics itself, in the same order: the same L and M).
// The chunk statistics are fetched one chunk per LANE (one load instruction, wave reductions) and the
// partial rows with all loads of a group of eight in flight -- a loop of dependent scalar loads made this
// 2 KB-per-wave kernel take 10 us, one L2 latency per chunk.
template <typename T, int DH>
__global__ __launch_bounds__(DH) void attn_rows_combine_kernel(const FwdParams p) {
  const int bn = blockIdx.y;
  const int row = blockIdx.x;  // 0 .. ng-1
  const int d = threadIdx.x;
  const int rowblk = row >> 5, rr = row & 31;
  const int b = bn / p.N, n = bn - b * p.N;
  const long slot0 = ((long)bn * p.n_rowblk + rowblk) * p.n_chunks;
  float L = 0.f, acc = 0.f, M = -INFINITY;
  for (int c0 = 0; c0 < p.n_chunks; c0 += 64) {             // 64 chunks per pass (one pass in practice)
    const int c = c0 + (DH == 64 ? d : (d & 63));
    const bool live = c < p.n_chunks;
    const float mc = live ? p.part_ml[(slot0 + c) * 64 + rr] : -INFINITY;
    const float lc = live ? p.part_ml[(slot0 + c) * 64 + 32 + rr] : 0.f;
    float Mn = mc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) Mn = fmaxf(Mn, __shfl_xor(Mn, o, 64));
    Mn = fmaxf(Mn, M);
    const float rescale = exp2f(M - Mn);                    // 0 on the first pass (M = -inf)
    const float wc = live ? exp2f(mc - Mn) : 0.f;
    float ls = wc * lc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ls += __shfl_xor(ls, o, 64);
    L = L * rescale + ls;
    acc *= rescale;
    M = Mn;
    const int cnt = min(64, p.n_chunks - c0);
    const float* po = p.part_o + (slot0 + c0) * (32 * DH) + rr * DH + d;
    int i = 0;
    for (; i + 8 <= cnt; i += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = po[(long)(i + u) * (32 * DH)];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = fmaf(__shfl(wc, i + u, 64), v[u], acc);
    }
    for (; i < cnt; ++i) acc = fmaf(__shfl(wc, i, 64), po[(long)i * (32 * DH)], acc);
  }
  const int q = p.pat.g0 + row;
  T* O = reinterpret_cast<T*>(p.out) + (long)b * p.os[0] + (long)q * p.os[1] + (long)n * p.os[2];
  O[d] = (T)(acc * p.part_scale / L);
  if (p.lse && d == 0) p.lse[((long)b * p.N + n) * p.S + q] = (M + log2f(L)) * kLn2;
}

// ------------------------------------ launchers -----------------------------------------
template <typename T, int MODE, int Rp, bool GEN, bool GRID, int DH, bool PACK, bool ORG, bool GLB>
static hipError_t launch_one(const FwdParams& p, dim3 grid, hipStream_t st) {
  const int lds = 4 * WaveLds<T, Rp, DH>::kBytes;
  if (lds > 64 * 1024)               // (the 128-wide table: relative vocabularies of 65..128 ids; DH = 128 from Rp = 64)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fwd_kernel<T, MODE, Rp, GEN, GRID, DH, PACK, ORG, GLB>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  hipLaunchKernelGGL((attn_fwd_kernel<T, MODE, Rp, GEN, GRID, DH, PACK, ORG, GLB>), grid, dim3(256), lds, st, p);
  return hipGetLastError();
}

template <typename T, int MODE, bool GEN, bool GRID, int DH, bool PACK = false, bool ORG = false, bool GLB = false>
static hipError_t launch_rp(const FwdParams& p, dim3 grid, hipStream_t st) {
  if (p.R <= 32) return launch_one<T, MODE, 32, GEN, GRID, DH, PACK, ORG, GLB>(p, grid, st);
  if (p.R <= 64) return launch_one<T, MODE, 64, GEN, GRID, DH, PACK, ORG, GLB>(p, grid, st);
  return launch_one<T, MODE, 128, GEN, GRID, DH, PACK, ORG, GLB>(p, grid, st);
}

// GEN and GRID of one (PACK, ORG) pair, as far as this translation unit holds them (kTu, attn_kernels.h).  GRIDS = false:
// the pair has no GRID instantiation (example ids never come with a grid: refused on the host).
template <typename T, int DH, bool PACK, bool ORG, bool GRIDS, bool GLB = false>
static hipError_t launch_band(const FwdParams& p, dim3 grid, hipStream_t st) {
  const bool table = kTu.table_ids && (p.pat.id_mode == 0 || p.perm_1d), grd = GRIDS && p.grid.ga > 0;
  if constexpr (kTu.table_ids && GRIDS) if (table && grd) return launch_rp<T, kBand, false, true, DH, PACK, ORG, GLB>(p, grid, st);
  if constexpr (kTu.table_ids) if (table) return launch_rp<T, kBand, false, false, DH, PACK, ORG, GLB>(p, grid, st);
  if constexpr (GRIDS) if (grd) return launch_rp<T, kBand, true, true, DH, PACK, ORG, GLB>(p, grid, st);      // image grid: its own instantiations
  return launch_rp<T, kBand, true, false, DH, PACK, ORG, GLB>(p, grid, st);
}

template <typename T, int DH>
static hipError_t launch_t(const FwdParams& p, int mode, int pack, dim3 grid, hipStream_t st) {
  if constexpr (kTu.dense) if (mode == kDense) return launch_rp<T, kDense, true, false, DH>(p, grid, st);
  if constexpr (kTu.pack_origin) if (pack == kPackOrigin) return launch_band<T, DH, true, true, true, kTu.globals>(p, grid, st);
  if constexpr (kTu.pack_ids) if (pack == kPackIds) return launch_band<T, DH, true, false, false>(p, grid, st);
  if constexpr (kTu.pack_none) if (pack == kPackNone) return launch_band<T, DH, false, false, true>(p, grid, st);
  return hipErrorInvalidValue;
}

hipError_t MMT_TU(launch_attn_fwd)(const FwdParams& p, int mode, bool bf16, int pack, hipStream_t st) {
  // band items first, then (kBand only) the global-row items of the same launch (none with example starts: n_rowblk = 0)
  const int per_bn = (p.n_chunks * p.n_rowblk + 3) / 4;
  dim3 grid(p.n_band_blocks + (mode == kBand ? per_bn * p.B * p.N : 0));
  if (p.D == 128) return bf16 ? launch_t<__bf16, 128>(p, mode, pack, grid, st) : launch_t<float, 128>(p, mode, pack, grid, st);
  return bf16 ? launch_t<__bf16, 64>(p, mode, pack, grid, st) : launch_t<float, 64>(p, mode, pack, grid, st);
}

#if !defined(MMT_IMAGE_TU) && !defined(MMT_ORIGIN_TU) && !defined(MMT_GLOBALS_TU)
template <int DH>
static hipError_t launch_rows_combine_dh(const FwdParams& p, bool bf16, hipStream_t st) {
  dim3 grid(p.pat.ng, p.B * p.N);
  if (bf16) hipLaunchKernelGGL((attn_rows_combine_kernel<__bf16, DH>), grid, dim3(DH), 0, st, p);
  else hipLaunchKernelGGL((attn_rows_combine_kernel<float, DH>), grid, dim3(DH), 0, st, p);
  return hipGetLastError();
}

hipError_t launch_rows_combine(const FwdParams& p, bool bf16, hipStream_t st) {
  return p.D == 128 ? launch_rows_combine_dh<128>(p, bf16, st) : launch_rows_combine_dh<64>(p, bf16, st);
}
#endif

}  // namespace mmt
