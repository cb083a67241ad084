/* C driver of the sanitizer build of the record container's host side (`make asan-records`, CPU only): mmt_records_scan,
 * mmt_example_fields and mmt_records_crc_host -- the functions of records.h that the kernels run, as plain loops -- under
 * -fsanitize=address,undefined.  The shard is built here in memory (a bytewise CRC-32C and a small Example encoder of the
 * driver's own); every input lives in a heap block of exactly its length and every output in one of exactly the size the
 * library was told, so a read or write past either is reported.  Nothing touches a GPU. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/mmt_attn.h"
#include "../../../include/mmt_layer.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "records asan driver: %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, mmt_last_error()); return 1; } } while (0)
#define MAX_RECORDS 16

static long g_scans, g_lookups, g_refused, g_crcs;

static void* block(size_t n, size_t align) {          /* exactly n bytes */
  void* p = NULL;
  if (posix_memalign(&p, align < sizeof(void*) ? sizeof(void*) : align, n ? n : 1) != 0) abort();
  return p;
}

static uint32_t crc32c(const unsigned char* p, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? 0x82F63B78u : 0u);
  }
  return c ^ 0xFFFFFFFFu;
}
static uint32_t mask(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

typedef struct buf { unsigned char d[8192]; size_t n; } buf;
static void put(buf* b, const void* p, size_t n) { if (b->n + n > sizeof(b->d)) abort(); memcpy(b->d + b->n, p, n); b->n += n; }
static void put_varint(buf* b, uint64_t v) { do { unsigned char c = (unsigned char)((v & 0x7F) | (v >= 0x80 ? 0x80 : 0)); put(b, &c, 1); v >>= 7; } while (v); }
static void put_ld(buf* b, int field, const void* p, size_t n) { put_varint(b, (uint64_t)field << 3 | 2); put_varint(b, n); put(b, p, n); }
static void put_le32(buf* b, uint32_t v) { unsigned char c[4] = {(unsigned char)v, (unsigned char)(v >> 8), (unsigned char)(v >> 16), (unsigned char)(v >> 24)}; put(b, c, 4); }

/* features { feature { key: name value { <kind field>: { value: ... } } } } appended to `features` */
static void put_bytes_feature(buf* features, const char* name, const void* v, size_t n, int unknown) {
  buf list = {{0}, 0}, feat = {{0}, 0}, ent = {{0}, 0};
  put_ld(&list, 1, v, n);
  if (unknown) { put_varint(&feat, 9 << 3 | 0); put_varint(&feat, 1234567); put_varint(&feat, 10 << 3 | 5); put_le32(&feat, 7); }
  put_ld(&feat, 1, list.d, list.n);
  put_ld(&ent, 1, name, strlen(name));
  put_ld(&ent, 2, feat.d, feat.n);
  put_ld(features, 1, ent.d, ent.n);
}
static void put_int_feature(buf* features, const char* name, const int64_t* v, int n, int packed) {
  buf vals = {{0}, 0}, list = {{0}, 0}, feat = {{0}, 0}, ent = {{0}, 0};
  for (int i = 0; i < n; ++i) {
    if (packed) put_varint(&vals, (uint64_t)v[i]);
    else { put_varint(&list, 1 << 3 | 0); put_varint(&list, (uint64_t)v[i]); }
  }
  if (packed) put_ld(&list, 1, vals.d, vals.n);
  put_ld(&feat, 3, list.d, list.n);
  put_ld(&ent, 1, name, strlen(name));
  put_ld(&ent, 2, feat.d, feat.n);
  put_ld(features, 1, ent.d, ent.n);
}
static void put_float_feature(buf* features, const char* name, float v) {
  buf list = {{0}, 0}, feat = {{0}, 0}, ent = {{0}, 0};
  uint32_t u;
  memcpy(&u, &v, 4);
  put_varint(&list, 1 << 3 | 5);
  put_le32(&list, u);
  put_ld(&feat, 2, list.d, list.n);
  put_ld(&ent, 1, name, strlen(name));
  put_ld(&ent, 2, feat.d, feat.n);
  put_ld(features, 1, ent.d, ent.n);
}
static void put_frame(buf* shard, const buf* payload) {
  unsigned char head[8];
  for (int i = 0; i < 8; ++i) head[i] = (unsigned char)((uint64_t)payload->n >> (8 * i));
  put(shard, head, 8);
  put_le32(shard, mask(crc32c(head, 8)));
  put(shard, payload->d, payload->n);
  put_le32(shard, mask(crc32c(payload->d, payload->n)));
}

static const char* const kNames[] = {"image_data", "image_key", "caption", "alt_text", "n", "f"};
#define N_NAMES 6

/* scan + lookup + CRC mirror over `len` bytes in an exact-size block; `pristine`: every result is checked as well */
static int run(const unsigned char* src, size_t len, int pristine, int want_records) {
  unsigned char* data = (unsigned char*)block(len, 1);
  memcpy(data, src, len);
  mmt_record* recs = (mmt_record*)block(sizeof(mmt_record) * MAX_RECORDS, 8);
  int64_t n = -1, used = -1;
  const int rc = mmt_records_scan(data, (int64_t)len, recs, MAX_RECORDS, &n, &used);
  ++g_scans;
  if (rc != MMT_OK) {
    CHECK(rc == MMT_E_INVALID && !pristine);
    ++g_refused;
    free(recs); free(data);
    return 0;
  }
  CHECK(n >= 0 && n <= MAX_RECORDS && used >= 0 && used <= (int64_t)len);
  if (pristine) CHECK(n == want_records);
  for (int64_t i = 0; i < n; ++i) {
    CHECK(recs[i].offset >= 12 && recs[i].length >= 0 && recs[i].offset + recs[i].length + 4 <= (int64_t)len);
    unsigned char* payload = (unsigned char*)block((size_t)recs[i].length, 1);      /* the lookup sees the payload alone */
    memcpy(payload, data + recs[i].offset, (size_t)recs[i].length);
    mmt_example_field* f = (mmt_example_field*)block(sizeof(mmt_example_field) * N_NAMES, 8);
    const int rf = mmt_example_fields(payload, recs[i].length, N_NAMES, kNames, f);
    ++g_lookups;
    if (rf == MMT_OK) {
      for (int k = 0; k < N_NAMES; ++k)
        if (f[k].kind == MMT_FIELD_BYTES && f[k].count > 0) CHECK(f[k].offset >= 0 && f[k].length >= 0 && f[k].offset + f[k].length <= recs[i].length);
      if (pristine && i == 0) CHECK(f[0].kind == MMT_FIELD_BYTES && f[0].count == 1 && f[0].length == 300 && f[3].kind == MMT_FIELD_MISSING);
      if (pristine && i == 1) CHECK(f[4].kind == MMT_FIELD_INT64 && f[4].count == 3 && f[4].int_value == -1 && f[5].kind == MMT_FIELD_FLOAT && f[5].float_value == 1.5f);
    } else {
      CHECK(rf == MMT_E_INVALID && !pristine);
      ++g_refused;
    }
    free(f); free(payload);
  }
  if (n > 0) {
    uint32_t* crc = (uint32_t*)block((size_t)n * 4, 4);
    int32_t* bad = (int32_t*)block((size_t)n * 4, 4);
    const size_t need = mmt_records_crc_workspace_bytes(n);
    CHECK(need > 0);
    void* work = block(need, 16);
    CHECK(mmt_records_crc_host(data, (int64_t)len, n, recs, crc, bad, work, need) == MMT_OK);
    ++g_crcs;
    for (int64_t i = 0; i < n; ++i) {
      CHECK(crc[i] == crc32c(data + recs[i].offset, (size_t)recs[i].length));
      if (pristine) CHECK(bad[i] == 0);
    }
    free(work); free(bad); free(crc);
  }
  free(recs); free(data);
  return 0;
}

/* wrong metadata against the clamping: whatever the records say, nothing outside [0, len) is read */
static int wrong_metadata(const unsigned char* src, size_t len) {
  static const int64_t offs[] = {-1, -((int64_t)1 << 62), 0, 5, 127, 128, 1000000, (int64_t)1 << 62, INT64_MAX, INT64_MIN};
  static const int64_t lens[] = {-1, INT64_MIN, 0, 1, 127, 129, 1000000, (int64_t)1 << 62, INT64_MAX};
  const int no = (int)(sizeof(offs) / sizeof(offs[0])), nl = (int)(sizeof(lens) / sizeof(lens[0])), n = no * nl;
  unsigned char* data = (unsigned char*)block(len, 1);
  memcpy(data, src, len);
  mmt_record* recs = (mmt_record*)block(sizeof(mmt_record) * (size_t)n, 8);
  for (int i = 0; i < n; ++i) { recs[i].offset = offs[i / nl]; recs[i].length = lens[i % nl]; recs[i].crc = 0; recs[i].reserved = 0; }
  uint32_t* crc = (uint32_t*)block((size_t)n * 4, 4);
  int32_t* bad = (int32_t*)block((size_t)n * 4, 4);
  const size_t need = mmt_records_crc_workspace_bytes(n);
  void* work = block(need, 16);
  CHECK(mmt_records_crc_host(data, (int64_t)len, n, recs, crc, bad, work, need) == MMT_OK);
  for (int i = 0; i < n; ++i) {
    int64_t o = recs[i].offset < 0 ? 0 : (recs[i].offset > (int64_t)len ? (int64_t)len : recs[i].offset);
    int64_t l = recs[i].length < 0 ? 0 : (recs[i].length > (int64_t)len - o ? (int64_t)len - o : recs[i].length);
    CHECK(crc[i] == crc32c(data + o, (size_t)l));
  }
  CHECK(mmt_records_crc_host(data, 0, n, recs, crc, bad, work, need) == MMT_OK);      /* an empty blob: every record is empty */
  for (int i = 0; i < n; ++i) CHECK(crc[i] == 0);
  CHECK(mmt_records_crc_host(data, (int64_t)len, n, recs, crc, bad, work, need - 1) == MMT_E_WORKSPACE);
  ++g_crcs;
  free(work); free(bad); free(crc); free(recs); free(data);
  return 0;
}

int main(void) {
  static buf shard, features, payload;
  unsigned char image[300];
  for (int i = 0; i < 300; ++i) image[i] = (unsigned char)(i * 7 + 3);
  /* record 0: image, key, caption; no alt_text.  record 1: int64 and float lists and unknown fields.  record 2: empty. */
  features.n = 0;
  put_bytes_feature(&features, "image_key", "key-0", 5, 0);
  put_bytes_feature(&features, "image_data", image, sizeof(image), 1);
  put_bytes_feature(&features, "caption", "a caption of some words", 23, 0);
  payload.n = 0;
  put_ld(&payload, 1, features.d, features.n);
  put_frame(&shard, &payload);
  const int64_t ints[3] = {-1, 300, 5};
  features.n = 0;
  put_int_feature(&features, "n", ints, 3, 1);
  put_int_feature(&features, "m", ints, 3, 0);
  put_float_feature(&features, "f", 1.5f);
  put_bytes_feature(&features, "alt_text", "", 0, 1);
  payload.n = 0;
  put_varint(&payload, 5 << 3 | 1);
  put(&payload, image, 8);
  put_ld(&payload, 1, features.d, features.n);
  put_frame(&shard, &payload);
  payload.n = 0;
  put_frame(&shard, &payload);

  CHECK(run(shard.d, shard.n, 1, 3) == 0);
  for (size_t cut = 0; cut < shard.n; ++cut) CHECK(run(shard.d, cut, 0, 0) == 0);          /* every prefix */
  unsigned char* bent = (unsigned char*)malloc(shard.n);
  for (size_t at = 0; at < shard.n; ++at)                                                     /* every single-byte corruption */
    for (int kind = 0; kind < 3; ++kind) {
      memcpy(bent, shard.d, shard.n);
      bent[at] = kind == 0 ? 0x00 : (kind == 1 ? 0xFF : (unsigned char)(bent[at] ^ (1u << (at % 8))));
      CHECK(run(bent, shard.n, 0, 0) == 0);
    }
  free(bent);
  CHECK(wrong_metadata(shard.d, shard.n) == 0);
  printf("records asan driver ok: %ld scans, %ld lookups, %ld checksum calls, %ld refusals\n", g_scans, g_lookups, g_crcs, g_refused);
  return 0;
}
