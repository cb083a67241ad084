// Host-only stand-ins for the kernel launchers, for the sanitizer build of the C-ABI shim (`make asan`) and the route
// table (`make routes`): they launch nothing, check that every workspace pointer the shim derived lies inside the
// caller's workspace, and record what was asked for -- which launcher (kernel family, translation unit) with which
// routing fields -- so that the drivers can assert on it and print it.  The planning formulas are the shipped ones
// (attn_plan.h).  CPU only -- never built into libmmt_attn.so.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "../attn_plan.h"
#include "../rand_augment.h"
#include "../text_tokens.h"

extern "C" {
const unsigned char* g_ws_lo = nullptr;
const unsigned char* g_ws_hi = nullptr;
int g_launches = 0;
int g_last_kind = 0;   // 1 fwd general, 2 fwd band, 3 fwd window, 4 rows combine, 5 bwd, 6 side inputs, 7 step scalars, 8 fwd plane walk, 9 fwd sliding window, 10 rand augment, 11 text tokens
int g_last_handover = 0;   // the last backward asked for the P hand-over
const void* g_last_epoch = nullptr;   // the device epoch word the last attention launch was given
int g_last_pack = 0;       // the last general forward / backward launch was asked for the PACK (example ids) instantiations
int g_last_family = 0;     // the last backward launcher called: 0 the general kernels, 1 the lean ones
int g_last_tu = 0;         // the last general forward / backward launcher called: 0 plain, 1 origin, 2 image, 3 globals translation unit
char g_trace[4096] = "";   // every stand-in called since the last reset, with the routing fields it was given (route table only)
int g_trace_len = -1;      // -1: not recording
void stub_trace_reset(void) { g_trace[0] = 0; g_trace_len = 0; }
}

namespace {
void inside(const void* p, size_t bytes, const char* what) {
  if (!p) return;
  const unsigned char* b = static_cast<const unsigned char*>(p);
  if (b < g_ws_lo || b + bytes > g_ws_hi) {
    std::fprintf(stderr, "asan driver: %s [%p, +%zu) outside the workspace [%p, %p)\n", what, p, bytes, (const void*)g_ws_lo, (const void*)g_ws_hi);
    std::abort();
  }
}

void trace(const char* fmt, ...) {
  if (g_trace_len < 0) return;
  va_list ap;
  va_start(ap, fmt);
  const int n = std::vsnprintf(g_trace + g_trace_len, sizeof(g_trace) - g_trace_len, fmt, ap);
  va_end(ap);
  if (n > 0) g_trace_len = std::min<int>(g_trace_len + n, sizeof(g_trace) - 1);
}
long off(const void* p) { return p ? (long)(static_cast<const unsigned char*>(p) - g_ws_lo) : -1; }   // workspace offset, -1 = NULL
const char* const kTuName[] = {"plain", "origin", "image", "globals"};

void kv(const char* key, long v, long dflt = 0) { if (v != dflt) trace(" %s=%ld", key, v); }   // fields at their default are left out

void trace_fwd(const char* name, const mmt::FwdParams& p) {      // name "": the caller has traced the launcher's name
  if (*name) trace(" | %s", name);
  kv("idm", p.pat.id_mode); kv("go", p.ids_go); kv("ga", p.grid.ga); kv("perm", p.perm_1d); kv("lean_rp", p.lean_rp);
  kv("skipg", p.skip_global_rows); kv("rowblk", p.n_rowblk); kv("chunks", p.n_chunks); kv("parts", p.rows_parts, 1);
  kv("rows_only", p.rows_only);
  if (p.part_scale != 1.f) trace(" pscale=%g", (double)p.part_scale);
  kv("tstride", p.tstride); kv("drop", p.drop_thresh);
  if (p.walk_groups) trace(" walk=%d/%d/%d", p.walk_groups, p.walk_nseg, p.walk_nhi);
  kv("maxseg", p.walk_maxseg); kv("pw", p.pw_walk);
  kv("part_o", off(p.part_o), -1); kv("part_ml", off(p.part_ml), -1); kv("walk_part", off(p.walk_part), -1); kv("sync", p.sync != nullptr);
}

hipError_t fwd_general(const mmt::FwdParams& p, int mode, bool bf16, int pack, int tu) {
  ++g_launches; g_last_kind = 1; g_last_epoch = p.epoch; g_last_pack = pack; g_last_tu = tu;
  trace(" | fwd_general[%s]", kTuName[tu]);
  kv("mode", mode); kv("bf16", bf16, 1); kv("pack", pack);
  trace_fwd("", p);
  const size_t slots = (size_t)p.B * p.N * p.n_rowblk * p.n_chunks;
  inside(p.part_o, slots * 32 * p.D * 4, "part_o");
  inside(p.part_ml, slots * 64 * 4, "part_ml");
  return hipSuccess;
}

hipError_t bwd_any(const mmt::BwdParams& p, const char* name, int pack) {
  ++g_launches; g_last_kind = 5; g_last_handover = p.ho != nullptr; g_last_epoch = p.epoch; g_last_pack = pack;
  if (*name) trace(" | %s", name);
  kv("idm", p.pat.id_mode); kv("go", p.ids_go); kv("ga", p.grid.ga); kv("perm", p.perm_1d); kv("Rp", p.Rp); kv("lean2d", p.lean2d);
  kv("skipg", p.skip_global); kv("gblk", p.n_gblk); kv("chunks", p.n_chunks); kv("split", p.n_split); kv("peel", p.peel_gkeys);
  kv("ho_slots", p.ho_slots); kv("dkv_slots", p.dkv_slots); kv("plane_major", p.dq_plane_major); kv("ho_per_wave", p.ho_per_wave);
  kv("drop", p.drop_thresh);
  trace(" ws=%ld/%ld/%ld/%ld/%ld/%ld/%ld/%ld", off(p.delta), off(p.relfar), off(p.drel), off(p.part_dq), off(p.part_dtab), off(p.part_dkv),
        off(p.part_red), off(p.ho));      // delta / relfar / drel / part_dq / part_dtab / part_dkv / part_red / ho
  if (pack && (p.peel_gkeys || p.lean2d)) { std::fprintf(stderr, "asan driver: example ids with a peeled step or the lean 2-D width\n"); std::abort(); }
  const size_t bn = (size_t)p.B * p.N, slots = bn * p.n_gblk * p.n_chunks;
  inside(p.delta, bn * p.S * 4, "delta");
  inside(p.relfar, bn * p.S * 2 * 4, "relfar");
  inside(p.drel, bn * (size_t)p.pat.ng * p.Rp * 4, "drel");
  inside(p.part_dq, slots * 32 * p.D * 4, "part_dq");
  inside(p.part_dtab, slots * 32 * p.Rp * 4, "part_dtab");
  inside(p.part_dkv, bn * p.n_gblk * (size_t)p.dkv_slots * 2 * 32 * p.D * 4, "part_dkv");
  if (p.ho) {          // P hand-over: band tiles, global-key strips, global-row tiles (attn_kernels.h)
    const size_t n_tiles = (size_t)(p.S + 31) / 32;
    inside(p.ho, bn * n_tiles * ((size_t)p.ho_slots * 2048 + 512 + 512), "ho");
    if (p.dkv_slots != p.n_chunks + (p.n_gblk > 0 ? 1 : 0)) { std::fprintf(stderr, "asan driver: hand-over without its partial slot\n"); std::abort(); }
  }
  inside(p.part_red, bn * ((p.S + 127) / 128) * 4 * ((size_t)p.Rp * p.D + p.Rp) * 4, "part_red");
  return hipSuccess;
}

hipError_t bwd_general(const mmt::BwdParams& p, int mode, bool bf16, int pack, int tu) {
  g_last_family = 0; g_last_tu = tu;
  trace(" | bwd_general[%s]", kTuName[tu]);
  kv("mode", mode); kv("bf16", bf16, 1); kv("pack", pack);
  return bwd_any(p, "", pack);
}
}  // namespace

// the lean 2-D backward zeroes the gradient rows no id can reach (mmt_api.hip): recorded, nothing is written
extern "C" hipError_t hipMemsetAsync(void*, int, size_t bytes, hipStream_t) { trace(" | memset bytes=%zu", bytes); return hipSuccess; }

namespace mmt {
hipError_t launch_attn_fwd(const FwdParams& p, int mode, bool bf16, int pack, hipStream_t) { return fwd_general(p, mode, bf16, pack, 0); }
hipError_t launch_attn_fwd_origin(const FwdParams& p, int mode, bool bf16, int pack, hipStream_t) { return fwd_general(p, mode, bf16, pack, 1); }
hipError_t launch_attn_fwd_image(const FwdParams& p, int mode, bool bf16, int pack, hipStream_t) { return fwd_general(p, mode, bf16, pack, 2); }
hipError_t launch_attn_fwd_globals(const FwdParams& p, int mode, bool bf16, int pack, hipStream_t) { return fwd_general(p, mode, bf16, pack, 3); }
hipError_t launch_attn_fwd_band_bf16(const FwdParams& p, hipStream_t) {
  ++g_launches; g_last_kind = 2; g_last_epoch = p.epoch; g_last_pack = 0;
  trace_fwd("fwd_lean", p);
  const size_t slots = (size_t)p.B * p.N * p.n_rowblk * p.n_chunks;
  inside(p.part_o, slots * 32 * p.D * 4, "part_o");
  inside(p.part_ml, slots * 64 * 4, "part_ml");
  return hipSuccess;
}
hipError_t launch_attn_fwd_win_bf16(const FwdParams& p, hipStream_t) {
  ++g_launches; g_last_kind = 3; g_last_epoch = p.epoch;
  trace_fwd("fwd_win", p);
  if (p.rows_parts < 1 || p.rows_parts > 4) { std::fprintf(stderr, "asan driver: rows_parts %d\n", p.rows_parts); std::abort(); }
  if (p.rows_parts > 1) {                     // the row groups' parts live in the caller's workspace, the ticket in its counters
    inside(p.walk_part, (size_t)p.B * p.N * p.n_rowblk * p.rows_parts * 8 * 66 * 4, "rows parts");
    if (!p.sync) { std::fprintf(stderr, "asan driver: split row groups without arrival counters\n"); std::abort(); }
  }
  return hipSuccess;
}
hipError_t launch_attn_fwd_walk_bf16(const FwdParams& p, int grid, hipStream_t) {
  ++g_launches; g_last_kind = 8; g_last_epoch = p.epoch;
  trace(" | fwd_walk grid=%d", grid);
  trace_fwd("", p);
  if (p.pat.ng > 0) inside(p.walk_part, (size_t)p.B * p.N * p.walk_maxseg * 8 * 66 * 4, "walk_part");
  const int per_group = grid / p.walk_groups, ppg = p.B * p.N / p.walk_groups;
  if (grid <= 0 || per_group != ppg * p.walk_nseg + p.walk_nhi || p.walk_nseg < 1 || p.walk_maxseg > ((p.S + 31) / 32 + 1) / 2) {
    std::fprintf(stderr, "asan driver: inconsistent plane-walk plan\n"); std::abort();
  }
  return hipSuccess;
}
hipError_t launch_attn_fwd_pwin_bf16(const FwdParams& p, int grid, hipStream_t) {
  ++g_launches; g_last_kind = 9; g_last_epoch = p.epoch;
  trace(" | fwd_pwin grid=%d", grid);
  trace_fwd("", p);
  const int nqb = (p.S + 127) / 128, total = p.B * p.N * nqb;
  if (grid <= 0 || p.pw_walk < 1 || (long)grid * p.pw_walk < total || (long)(grid - 1) * p.pw_walk >= total) { std::fprintf(stderr, "asan driver: inconsistent sliding-window plan\n"); std::abort(); }
  if (p.pat.ng > 0) inside(p.walk_part, ((size_t)grid * (8 * 34 + 4 * kPwState) + (size_t)p.B * p.N * p.walk_maxseg * 4 * 8 * 66) * 4, "pwin workspace");
  return hipSuccess;
}
hipError_t launch_rows_combine(const FwdParams& p, bool, hipStream_t) {
  ++g_launches; g_last_kind = 4;
  trace(" | rows_combine rowblk=%d chunks=%d", p.n_rowblk, p.n_chunks);
  if (p.part_scale != 1.f) trace(" pscale=%g", (double)p.part_scale);
  return hipSuccess;
}
hipError_t launch_attn_bwd(const BwdParams& p, int mode, bool bf16, int pack, hipStream_t) { return bwd_general(p, mode, bf16, pack, 0); }
hipError_t launch_attn_bwd_origin(const BwdParams& p, int mode, bool bf16, int pack, hipStream_t) { return bwd_general(p, mode, bf16, pack, 1); }
hipError_t launch_attn_bwd_image(const BwdParams& p, int mode, bool bf16, int pack, hipStream_t) { return bwd_general(p, mode, bf16, pack, 2); }
hipError_t launch_attn_bwd_globals(const BwdParams& p, int mode, bool bf16, int pack, hipStream_t) { return bwd_general(p, mode, bf16, pack, 3); }
hipError_t launch_attn_bwd_band_bf16(const BwdParams& p, hipStream_t) { g_last_family = 1; return bwd_any(p, "bwd_lean", 0); }
hipError_t launch_side_inputs(const SideParams&, hipStream_t) { ++g_launches; g_last_kind = 6; return hipSuccess; }
hipError_t launch_rand_augment(const RandAugParams& p, hipStream_t) {     // rand_augment.hip built with MMT_RAND_AUGMENT_HOST_ONLY
  ++g_launches; g_last_kind = 10;
  trace(" | rand_augment B=%d parts=%d", p.B, p.parts);
  if (p.B < 1 || p.parts < 8 || p.parts > 256) { std::fprintf(stderr, "asan driver: rand augment grid %d x %d\n", p.B, p.parts); std::abort(); }
  inside(p.hist, (size_t)p.B * kRandAugHistBytes, "rand augment histograms");
  return hipSuccess;
}
hipError_t launch_text_tokens(const TextParams& p, hipStream_t) {       // text_tokens.hip built with MMT_TEXT_TOKENS_HOST_ONLY
  ++g_launches; g_last_kind = 11;
  trace(" | text_tokens B=%d F=%d T=%d budget=%d", p.B, p.F, p.T, p.budget);
  if (p.B < 1 || p.F < 1 || p.F > kTextMaxFields || p.budget < 0 || p.F + p.budget + 1 > p.T) { std::fprintf(stderr, "asan driver: text tokens shape %d %d %d %d\n", p.B, p.F, p.T, p.budget); std::abort(); }
  inside(p.pieces, (size_t)p.B * p.F * p.budget * 4, "text piece records");
  inside(p.npieces, (size_t)p.B * p.F * 4, "text piece counts");
  return hipSuccess;
}
hipError_t launch_write_step_scalars(unsigned long long*, float*, unsigned long long, float, float, float, hipStream_t) { ++g_launches; g_last_kind = 7; return hipSuccess; }
}  // namespace mmt
