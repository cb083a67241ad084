// Host-side planning of the window / plane-walk / sliding-window forward kernels (LDS need, grid, workspace) and the constants
// it shares with them.  One copy: read by the kernel files, the dispatch (mmt_api.hip) and the host stand-ins (asan/).
#pragma once
#include <algorithm>
#include "attn_kernels.h"

namespace mmt {
constexpr int kWinTiles = 8;
// window kernel (attn_fwd_win.hip): LDS bytes of one workgroup (`tstride` as chosen by the caller)
inline int fwd_win_lds_bytes(int ng, int tstride) {
  const int ngrp = (ng + 7) / 8;
  const int band = 2 * kWinTiles * 4096 + (ngrp ? (2 * ngrp + 1) * 1024 : 0) + 4 * 32 * tstride * 4;
  const int rows = 8 * (2 * 4096 + 512 + 64) + 8 * 34 * 4 + 4096;          // fwd_rows_body's carve (used when 0 < ng <= 16)
  return (ng > 0 && ng <= 16 && rows > band) ? rows : band;
}
// plane-walk kernel (attn_fwd_walk.hip)
constexpr int kSlotBytes = 16384;        // K tile 2T | K tile 2T + 1 | V tile 2T | V tile 2T + 1
constexpr int kRowsState = 2048 + 1024 + 64;      // O^T of 8 rows (16 lanes x 32 floats) | per-lane row sums | 8 maxima
struct WalkLds { int tab, eimg, btab, gk, gv, rst, pbuf, tabg, qimg, flag, total; };
__host__ __device__ inline WalkLds walk_lds(int ng, int tstride, bool rel) {
  const int ngrp = (ng + 7) / 8;
  WalkLds L;
  int o = 2 * kSlotBytes;
  L.tab = o; o += rel ? 8 * 32 * tstride * 4 : 0;
  L.eimg = o; o += rel ? 4096 : 0;
  L.btab = o; o += rel ? 128 : 0;
  L.gk = o; o += ngrp * 1024;
  L.gv = o; o += ngrp ? (ngrp + 1) * 1024 : 0;
  L.rst = o; o += ng ? 2 * kRowsState : 0;
  L.pbuf = o; o += ng ? 2 * 512 : 0;
  L.tabg = o; o += (ng && rel) ? 8 * tstride * 4 : 0;
  L.qimg = o; o += ng ? 1024 : 0;
  L.flag = o; o += 16 + 32;
  L.total = o;
  return L;
}
inline int fwd_walk_lds_bytes(int ng, int tstride, bool rel) { return walk_lds(ng, tstride, rel).total; }
// Runs per plane: as many workgroups as fit the chip at once (2 per CU), shared out over the planes; a run is at least
// one pair of row blocks.  Fills the walk_* fields of `p`; returns the grid size.
inline int fwd_walk_plan(FwdParams& p, int target_wgs) {
  const int BN = p.B * p.N, NT = (p.S + 31) / 32, U = (NT + 1) / 2;
  const int ngroups = (BN % 8) == 0 ? 8 : 1, ppg = BN / ngroups;
  int per_group = target_wgs / ngroups;
  if (per_group > ppg * U) per_group = ppg * U;
  if (per_group < ppg) per_group = ppg;
  p.walk_groups = ngroups;
  p.walk_nseg = per_group / ppg;
  p.walk_nhi = per_group % ppg;
  p.walk_maxseg = p.walk_nseg + (p.walk_nhi ? 1 : 0);
  return ngroups * per_group;
}
inline size_t fwd_walk_workspace_bytes(int B, int N, int S) {      // upper bound over every plan: U runs per plane
  const int NT = (S + 31) / 32, U = (NT + 1) / 2;
  return (size_t)B * N * U * 8 * 66 * sizeof(float);
}
// sliding-window kernel (attn_fwd_pwin.hip)
constexpr int kPwState = 512 + 256 + 16;      // floats of one rows stream: O^T of 8 rows (16 lanes x 32) | per-lane row sums | 8 maxima (+ pad)
// Blocks per walk so that all workgroups are resident at once (two per CU); fills pw_walk / walk_maxseg; returns the grid.
inline int fwd_pwin_plan(FwdParams& p, int target_wgs) {
  const int nqb = (p.S + 127) / 128, total = p.B * p.N * nqb;
  int walk = (total + target_wgs - 1) / target_wgs;
  if (walk < 1) walk = 1;
  p.pw_walk = walk;
  p.walk_maxseg = (nqb + walk - 1) / walk + 1;               // walks that can hold blocks of one plane
  return (total + walk - 1) / walk;
}
inline size_t fwd_pwin_workspace_bytes(int B, int N, int S, int target_wgs) {
  const int nqb = (S + 127) / 128, total = B * N * nqb;
  const int walk = std::max(1, (total + target_wgs - 1) / target_wgs);
  const size_t grid = (size_t)(total + walk - 1) / walk;
  const size_t maxseg = (size_t)(nqb + walk - 1) / walk + 1;
  return (grid * (8 * 34 + 4 * kPwState) + (size_t)B * N * maxseg * 4 * 8 * 66) * sizeof(float);
}

}  // namespace mmt
