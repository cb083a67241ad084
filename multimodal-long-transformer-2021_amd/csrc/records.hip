// Record container of the data layer (C ABI: include/mmt_layer.h, mmt_records_* and mmt_example_fields; DESIGN.md
// section 4, "Records"): the TFRecord frame walk and the tf.train.Example field lookup as plain host C++, and the
// payload checksums (CRC-32C) of a batch of records as kernels on the blob the loader uploads anyway.  records.h has the
// tables, the register of one piece and the shifts, which the kernels and mmt_records_crc_host share.
//
//   launches of mmt_records_crc, 256 threads
//   1. prep     one workgroup: clamps every record into the blob, counts its pieces (PIECE bytes, cut from the payload's
//               end), writes the exclusive prefix sum start[0 .. n] and seeds crc_out[i] with shift(~0, len) ^ ~0
//   2. pieces   a workgroup per PART bytes of pieces (grid-stride beyond the grid): a lane finds its piece's record by
//               bisection of start[], takes raw(piece) with the slice-by-4 tables in LDS, a segmented scan over the
//               workgroup joins the pieces of one record (every join shifts by 2^level whole pieces: one bit matrix per
//               level), and the last lane of every run shifts by the pieces still to come and xors into crc_out --
//               integer xor, so the order of arrival does not show
//   3. finish   bad_out[i] = mask(crc_out[i]) != stored
//
// Bounds: rec_place() clamps offset and length into [0, bytes_len]; a piece lies inside its payload, and rec_raw() loads
// 4 or 16 bytes only at addresses aligned to that and wholly inside the piece.
#include "../../include/mmt_attn.h"
#include "../../include/mmt_layer.h"

#include <cstdint>
#include <cstring>

#include "mmt_err.h"
#include "records.h"

namespace mmt {
namespace {

const RecTables kRecTablesHost = rec_make_tables();

inline uint32_t crc32c_host(const unsigned char* p, long n) {
  return rec_raw(&kRecTablesHost.slice[0][0], p, n) ^ rec_shift_bytes(kRecTablesHost.xpow, 0xFFFFFFFFu, (uint64_t)n) ^ 0xFFFFFFFFu;
}

inline uint32_t load_le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// ---- protobuf wire format: positions are bytes from the start of the payload ---------------------------------------
struct Wire {
  const uint8_t* b;
};

int rd_varint(const Wire& w, int64_t end, int64_t& pos, uint64_t& v) {
  const int64_t at = pos;
  v = 0;
  for (int i = 0; i < 10; ++i) {
    if (pos >= end) return fail(MMT_E_INVALID, "mmt_example_fields: truncated varint at byte %lld", (long long)at);
    const uint8_t c = w.b[pos++];
    v |= (uint64_t)(c & 0x7Fu) << (7 * i);
    if (!(c & 0x80u)) return MMT_OK;
  }
  return fail(MMT_E_INVALID, "mmt_example_fields: varint of more than 10 bytes at byte %lld", (long long)at);
}

int rd_tag(const Wire& w, int64_t end, int64_t& pos, uint64_t& field, int& wt) {
  const int64_t at = pos;
  uint64_t tag;
  if (const int rc = rd_varint(w, end, pos, tag)) return rc;
  field = tag >> 3;
  wt = (int)(tag & 7u);
  if (field == 0) return fail(MMT_E_INVALID, "mmt_example_fields: field number 0 at byte %lld", (long long)at);
  return MMT_OK;
}

int rd_len(const Wire& w, int64_t end, int64_t& pos, int64_t& sub_end) {
  const int64_t at = pos;
  uint64_t n;
  if (const int rc = rd_varint(w, end, pos, n)) return rc;
  if (n > (uint64_t)(end - pos))
    return fail(MMT_E_INVALID, "mmt_example_fields: length %llu at byte %lld leaves its message (%lld bytes remain)", (unsigned long long)n,
                (long long)at, (long long)(end - pos));
  sub_end = pos + (int64_t)n;
  return MMT_OK;
}

int skip_field(const Wire& w, int64_t end, int64_t& pos, int wt, int64_t tag_at) {
  uint64_t v;
  int64_t sub_end;
  switch (wt) {
    case 0: return rd_varint(w, end, pos, v);
    case 1:
      if (end - pos < 8) return fail(MMT_E_INVALID, "mmt_example_fields: truncated 64-bit field at byte %lld", (long long)tag_at);
      pos += 8;
      return MMT_OK;
    case 2:
      if (const int rc = rd_len(w, end, pos, sub_end)) return rc;
      pos = sub_end;
      return MMT_OK;
    case 5:
      if (end - pos < 4) return fail(MMT_E_INVALID, "mmt_example_fields: truncated 32-bit field at byte %lld", (long long)tag_at);
      pos += 4;
      return MMT_OK;
    case 3: case 4: return fail(MMT_E_INVALID, "mmt_example_fields: group at byte %lld", (long long)tag_at);
    default: return fail(MMT_E_INVALID, "mmt_example_fields: wire type %d at byte %lld", wt, (long long)tag_at);
  }
}

int parse_list(const Wire& w, int64_t pos, int64_t end, int kind, mmt_example_field& out) {
  std::memset(&out, 0, sizeof(out));
  out.kind = kind;
  while (pos < end) {
    const int64_t at = pos;
    uint64_t field;
    int wt;
    if (const int rc = rd_tag(w, end, pos, field, wt)) return rc;
    int64_t sub_end;
    if (field == 1 && kind == MMT_FIELD_BYTES && wt == 2) {
      if (const int rc = rd_len(w, end, pos, sub_end)) return rc;
      if (out.count == 0) { out.offset = pos; out.length = sub_end - pos; }
      ++out.count;
      pos = sub_end;
    } else if (field == 1 && kind == MMT_FIELD_FLOAT && wt == 5) {
      if (end - pos < 4) return fail(MMT_E_INVALID, "mmt_example_fields: truncated float at byte %lld", (long long)at);
      if (out.count == 0) { const uint32_t u = load_le32(w.b + pos); std::memcpy(&out.float_value, &u, 4); }
      ++out.count;
      pos += 4;
    } else if (field == 1 && kind == MMT_FIELD_FLOAT && wt == 2) {
      if (const int rc = rd_len(w, end, pos, sub_end)) return rc;
      if ((sub_end - pos) & 3) return fail(MMT_E_INVALID, "mmt_example_fields: packed floats of %lld bytes at byte %lld", (long long)(sub_end - pos), (long long)at);
      if (out.count == 0 && sub_end - pos >= 4) { const uint32_t u = load_le32(w.b + pos); std::memcpy(&out.float_value, &u, 4); }
      out.count += (sub_end - pos) >> 2;
      pos = sub_end;
    } else if (field == 1 && kind == MMT_FIELD_INT64 && wt == 0) {
      uint64_t v;
      if (const int rc = rd_varint(w, end, pos, v)) return rc;
      if (out.count == 0) out.int_value = (int64_t)v;
      ++out.count;
    } else if (field == 1 && kind == MMT_FIELD_INT64 && wt == 2) {
      if (const int rc = rd_len(w, end, pos, sub_end)) return rc;
      while (pos < sub_end) {
        uint64_t v;
        if (const int rc = rd_varint(w, sub_end, pos, v)) return rc;
        if (out.count == 0) out.int_value = (int64_t)v;
        ++out.count;
      }
    } else if (const int rc = skip_field(w, end, pos, wt, at)) {
      return rc;
    }
  }
  return MMT_OK;
}

int parse_feature(const Wire& w, int64_t pos, int64_t end, mmt_example_field& out) {
  std::memset(&out, 0, sizeof(out));
  while (pos < end) {
    const int64_t at = pos;
    uint64_t field;
    int wt;
    if (const int rc = rd_tag(w, end, pos, field, wt)) return rc;
    if (wt == 2 && field >= 1 && field <= 3) {
      int64_t sub_end;
      if (const int rc = rd_len(w, end, pos, sub_end)) return rc;
      const int kind = field == 1 ? MMT_FIELD_BYTES : (field == 2 ? MMT_FIELD_FLOAT : MMT_FIELD_INT64);
      if (const int rc = parse_list(w, pos, sub_end, kind, out)) return rc;      // a oneof: the last one set holds
      pos = sub_end;
    } else if (const int rc = skip_field(w, end, pos, wt, at)) {
      return rc;
    }
  }
  return MMT_OK;
}

int parse_entry(const Wire& w, int64_t pos, int64_t end, int32_t n_names, const char* const* names, mmt_example_field* out) {
  int64_t key_at = 0, key_len = -1, val_at = 0, val_end = -1;
  while (pos < end) {
    const int64_t at = pos;
    uint64_t field;
    int wt;
    if (const int rc = rd_tag(w, end, pos, field, wt)) return rc;
    int64_t sub_end;
    if (wt == 2 && (field == 1 || field == 2)) {
      if (const int rc = rd_len(w, end, pos, sub_end)) return rc;
      if (field == 1) { key_at = pos; key_len = sub_end - pos; }
      else { val_at = pos; val_end = sub_end; }
      pos = sub_end;
    } else if (const int rc = skip_field(w, end, pos, wt, at)) {
      return rc;
    }
  }
  if (key_len < 0) key_len = 0;                                  // an absent key is the empty string
  mmt_example_field f;
  std::memset(&f, 0, sizeof(f));
  if (val_end >= 0)
    if (const int rc = parse_feature(w, val_at, val_end, f)) return rc;
  for (int32_t i = 0; i < n_names; ++i)
    if ((int64_t)std::strlen(names[i]) == key_len && std::memcmp(names[i], w.b + key_at, (size_t)key_len) == 0) out[i] = f;
  return MMT_OK;
}

int parse_features(const Wire& w, int64_t pos, int64_t end, int32_t n_names, const char* const* names, mmt_example_field* out) {
  while (pos < end) {
    const int64_t at = pos;
    uint64_t field;
    int wt;
    if (const int rc = rd_tag(w, end, pos, field, wt)) return rc;
    if (wt == 2 && field == 1) {
      int64_t sub_end;
      if (const int rc = rd_len(w, end, pos, sub_end)) return rc;
      if (const int rc = parse_entry(w, pos, sub_end, n_names, names, out)) return rc;
      pos = sub_end;
    } else if (const int rc = skip_field(w, end, pos, wt, at)) {
      return rc;
    }
  }
  return MMT_OK;
}

// ---- payload checksums ----------------------------------------------------------------------------------------------
struct RecParams {
  const unsigned char* bytes;
  long bytes_len, n;
  const mmt_record* rec;
  uint32_t* crc;
  int32_t* bad;
  long* start;                         // [n + 1] in the workspace
};

int check_crc(const char* who, const uint8_t* bytes, int64_t bytes_len, int64_t n, const mmt_record* records, uint32_t* crc_out,
              int32_t* bad_out, void* workspace, size_t workspace_bytes, RecParams& p) {
  if (n < 0 || n >= ((int64_t)1 << 31)) return fail(MMT_E_INVALID, "%s: n %lld outside [0, 2^31)", who, (long long)n);
  if (bytes_len < 0 || bytes_len >= ((int64_t)1 << 48)) return fail(MMT_E_INVALID, "%s: bytes_len %lld outside [0, 2^48)", who, (long long)bytes_len);
  if ((bytes_len > 0 && !bytes) || !workspace || (n > 0 && (!records || !crc_out || !bad_out)))
    return fail(MMT_E_INVALID, "%s: NULL argument (only the stream may be NULL)", who);
  if (((uintptr_t)records & 7) != 0 || (((uintptr_t)crc_out | (uintptr_t)bad_out) & 3) != 0 || ((uintptr_t)workspace & 15) != 0)
    return fail(MMT_E_INVALID, "%s: records must be 8-byte, crc_out and bad_out 4-byte and the workspace 16-byte aligned", who);
  const size_t need = mmt_records_crc_workspace_bytes(n);
  if (workspace_bytes < need) return fail(MMT_E_WORKSPACE, "%s: workspace of %zu bytes needed, %zu given", who, need, workspace_bytes);
  p.bytes = bytes; p.bytes_len = bytes_len; p.n = n; p.rec = records; p.crc = crc_out; p.bad = bad_out;
  p.start = (long*)workspace;
  return MMT_OK;
}

#ifndef MMT_RECORDS_HOST_ONLY
__device__ const RecTables kRecTablesDev = rec_make_tables();

__global__ __launch_bounds__(256) void rec_prep_kernel(const RecParams p) {
  __shared__ long s[kRecThreads];
  const int t = threadIdx.x;
  long carry = 0;                                                // the same in every lane
  for (long base = 0; base < p.n; base += kRecThreads) {
    const long i = base + t;
    RecPlace q = {0, 0, 0};
    if (i < p.n) q = rec_place(p.rec[i], p.bytes_len);
    s[t] = q.pieces;
    __syncthreads();
    for (int d = 1; d < kRecThreads; d <<= 1) {
      const long add = t >= d ? s[t - d] : 0;
      __syncthreads();
      s[t] += add;
      __syncthreads();
    }
    if (i < p.n) {
      p.start[i] = carry + s[t] - q.pieces;
      p.crc[i] = rec_shift_bytes(kRecTablesDev.xpow, 0xFFFFFFFFu, (uint64_t)q.len) ^ 0xFFFFFFFFu;
    }
    carry += s[kRecThreads - 1];
    __syncthreads();
  }
  if (t == 0) p.start[p.n] = carry;
}

__global__ __launch_bounds__(256) void rec_pieces_kernel(const RecParams p) {
  __shared__ uint32_t slice[4 * 256];
  __shared__ uint32_t level[kRecLevels * 32];
  __shared__ uint32_t val[2][kRecThreads];
  __shared__ int seg[kRecThreads];
  const int t = threadIdx.x;
  const long total = p.start[p.n];
  if ((long)blockIdx.x * kRecThreads >= total) return;
  for (int i = t; i < 4 * 256; i += kRecThreads) slice[i] = (&kRecTablesDev.slice[0][0])[i];
  level[t] = (&kRecTablesDev.level[0][0])[t];
  __syncthreads();
  for (long part = blockIdx.x; part * kRecThreads < total; part += gridDim.x) {
    const long g = part * kRecThreads + t;
    const bool live = g < total;
    long r = 0, k = 0;
    RecPlace q = {0, 0, 0};
    uint32_t v = 0;
    if (live) {
      long lo = 0, hi = p.n;                                     // start[lo] <= g < start[hi]
      while (hi - lo > 1) {
        const long mid = lo + ((hi - lo) >> 1);
        if (p.start[mid] <= g) lo = mid; else hi = mid;
      }
      r = lo;
      q = rec_place(p.rec[r], p.bytes_len);
      k = g - p.start[r];
      if (k < 0) k = 0;
      if (k > q.pieces - 1) k = q.pieces - 1;
      if (q.pieces > 0) {
        long begin, end;
        rec_piece(q, k, begin, end);
        v = rec_raw(slice, p.bytes + q.off + begin, end - begin);
      }
    }
    seg[t] = live ? (int)r : -1;
    val[0][t] = v;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kRecLevels; ++j) {
      const int d = 1 << j, cur = j & 1;
      uint32_t x = val[cur][t];
      if (t >= d && seg[t] >= 0 && seg[t - d] == seg[t]) x ^= rec_shift_level(level + 32 * j, val[cur][t - d]);
      val[cur ^ 1][t] = x;
      __syncthreads();
    }
    if (live && q.pieces > 0 && (t == kRecThreads - 1 || seg[t + 1] != seg[t])) {
      const uint64_t behind = (uint64_t)(q.pieces - 1 - k) << kRecPieceLog;
      atomicXor(p.crc + r, rec_shift_bytes(kRecTablesDev.xpow, val[kRecLevels & 1][t], behind));
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void rec_finish_kernel(const RecParams p) {
  const long i = (long)blockIdx.x * kRecThreads + threadIdx.x;
  if (i < p.n) p.bad[i] = rec_mask(p.crc[i]) != p.rec[i].crc ? 1 : 0;
}

hipError_t launch_records_crc(const RecParams& p, hipStream_t st) {
  if (p.n == 0) return hipSuccess;
  // at most bytes_len / PIECE + n pieces when the records do not overlap; the grid-stride loop serves whatever is beyond
  long parts = ((p.bytes_len >> kRecPieceLog) + p.n + kRecThreads - 1) / kRecThreads;
  if (parts < 1) parts = 1;
  if (parts > 65536) parts = 65536;
  hipLaunchKernelGGL(rec_prep_kernel, dim3(1), dim3(kRecThreads), 0, st, p);
  hipLaunchKernelGGL(rec_pieces_kernel, dim3((unsigned)parts), dim3(kRecThreads), 0, st, p);
  hipLaunchKernelGGL(rec_finish_kernel, dim3((unsigned)((p.n + kRecThreads - 1) / kRecThreads)), dim3(kRecThreads), 0, st, p);
  return hipGetLastError();
}
#endif  // MMT_RECORDS_HOST_ONLY

}  // namespace
}  // namespace mmt

extern "C" {

int mmt_records_scan(const uint8_t* bytes, int64_t len, mmt_record* records_out, int64_t capacity, int64_t* n_out, int64_t* consumed_out) {
  using namespace mmt;
  if (len < 0 || capacity < 0 || (len > 0 && !bytes) || (capacity > 0 && !records_out) || !n_out || !consumed_out)
    return fail(MMT_E_INVALID, "mmt_records_scan: NULL argument or negative len / capacity");
  uint64_t pos = 0;
  const uint64_t size = (uint64_t)len;
  int64_t n = 0;
  while (n < capacity && size - pos >= 12) {
    const uint8_t* h = bytes + pos;
    const uint32_t want = load_le32(h + 8), got = rec_mask(crc32c_host(h, 8));
    if (want != got)
      return fail(MMT_E_INVALID, "mmt_records_scan: length checksum of the frame at byte %llu is %08x, its length bytes give %08x",
                  (unsigned long long)pos, want, got);
    const uint64_t length = (uint64_t)load_le32(h) | (uint64_t)load_le32(h + 4) << 32;
    const uint64_t room = size - pos - 12;                       // behind the header; the frame needs length + 4 of it
    if (room < 4 || length > room - 4) break;
    records_out[n].offset = (int64_t)(pos + 12);
    records_out[n].length = (int64_t)length;
    records_out[n].crc = load_le32(h + 12 + length);
    records_out[n].reserved = 0;
    ++n;
    pos += 12 + length + 4;
  }
  *n_out = n;
  *consumed_out = (int64_t)pos;
  return MMT_OK;
}

int mmt_example_fields(const uint8_t* payload, int64_t len, int32_t n_names, const char* const* names, mmt_example_field* fields_out) {
  using namespace mmt;
  if (len < 0 || n_names < 0 || (len > 0 && !payload) || (n_names > 0 && (!names || !fields_out)))
    return fail(MMT_E_INVALID, "mmt_example_fields: NULL argument or negative len / n_names");
  for (int32_t i = 0; i < n_names; ++i) {
    if (!names[i]) return fail(MMT_E_INVALID, "mmt_example_fields: names[%d] is NULL", i);
    std::memset(&fields_out[i], 0, sizeof(mmt_example_field));
  }
  const Wire w = {payload};
  int64_t pos = 0;
  while (pos < len) {
    const int64_t at = pos;
    uint64_t field;
    int wt;
    if (const int rc = rd_tag(w, len, pos, field, wt)) return rc;
    if (wt == 2 && field == 1) {
      int64_t sub_end;
      if (const int rc = rd_len(w, len, pos, sub_end)) return rc;
      if (const int rc = parse_features(w, pos, sub_end, n_names, names, fields_out)) return rc;
      pos = sub_end;
    } else if (const int rc = skip_field(w, len, pos, wt, at)) {
      return rc;
    }
  }
  return MMT_OK;
}

size_t mmt_records_crc_workspace_bytes(int64_t n) {
  if (n < 0 || n >= ((int64_t)1 << 31)) return 0;
  return (((size_t)n + 1) * 8 + 15) & ~(size_t)15;
}

int mmt_records_crc_host(const uint8_t* bytes, int64_t bytes_len, int64_t n, const mmt_record* records, uint32_t* crc_out, int32_t* bad_out,
                         void* workspace, size_t workspace_bytes) {
  using namespace mmt;
  RecParams p;
  const int rc = check_crc("mmt_records_crc_host", bytes, bytes_len, n, records, crc_out, bad_out, workspace, workspace_bytes, p);
  if (rc) return rc;
  const RecTables& T = kRecTablesHost;
  long run = 0;
  for (long i = 0; i < n; ++i) {
    const RecPlace q = rec_place(records[i], bytes_len);
    p.start[i] = run;
    run += q.pieces;
    uint32_t acc = 0;
    for (long k = 0; k < q.pieces; ++k) {                        // the join of the kernel's first level, piece after piece
      long begin, end;
      rec_piece(q, k, begin, end);
      acc = rec_shift_level(T.level[0], acc) ^ rec_raw(&T.slice[0][0], bytes + q.off + begin, end - begin);
    }
    crc_out[i] = acc ^ rec_shift_bytes(T.xpow, 0xFFFFFFFFu, (uint64_t)q.len) ^ 0xFFFFFFFFu;
    bad_out[i] = rec_mask(crc_out[i]) != records[i].crc ? 1 : 0;
  }
  p.start[n] = run;
  return MMT_OK;
}

#ifndef MMT_RECORDS_HOST_ONLY
int mmt_records_crc(const uint8_t* bytes, int64_t bytes_len, int64_t n, const mmt_record* records, uint32_t* crc_out, int32_t* bad_out,
                    void* workspace, size_t workspace_bytes, void* stream) {
  mmt::RecParams p;
  const int rc = mmt::check_crc("mmt_records_crc", bytes, bytes_len, n, records, crc_out, bad_out, workspace, workspace_bytes, p);
  if (rc) return rc;
  const hipError_t e = mmt::launch_records_crc(p, (hipStream_t)stream);
  return e == hipSuccess ? MMT_OK : mmt::fail(MMT_E_LAUNCH, "mmt_records_crc: %s", hipGetErrorString(e));
}
#endif

}  // extern "C"
