"""Record container without a GPU: the frame walk (mmt_records_scan), the tf.train.Example field lookup
(mmt_example_fields) and the host mirror of the payload checksums (mmt_records_crc_host, the functions the kernels run)
against constants produced independently and against the pure-Python oracle and writer of tests/_record_cases.py; the
chunked shard reader; and the sanitizer program (`make asan-records`)."""
import ctypes
import os
import struct

import numpy as np
import pytest

from tests import _record_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MMT_E_INVALID = -1


@pytest.fixture(scope='module')
def lib():
  import __graft_entry__  # noqa: F401  (sets sys.path)
  from mmt_amd import _lib
  _lib.build()
  return _lib


def host_crc(lib, blob, offsets, lengths, stored=None):
  """mmt_records_crc_host over numpy buffers: (crc uint32 [n], bad int32 [n])."""
  L = lib.lib()
  n = len(offsets)
  recs = (lib.Record * max(n, 1))()
  for i in range(n):
    recs[i].offset, recs[i].length = int(offsets[i]), int(lengths[i])
    recs[i].crc = 0 if stored is None else int(stored[i])
  crc, bad = np.full(max(n, 1), 0xDEADBEEF, dtype=np.uint32), np.full(max(n, 1), -7, dtype=np.int32)
  need = L.mmt_records_crc_workspace_bytes(n)
  assert need >= (n + 1) * 8
  ws = np.zeros(need // 8 + 2, dtype=np.int64)
  ws_ptr = (ws.ctypes.data + 15) & ~15
  lib.check(L.mmt_records_crc_host(R.np_ptr(blob), blob.size, n, ctypes.addressof(recs), R.np_ptr(crc), R.np_ptr(bad), ws_ptr, need))
  return crc[:n], bad[:n]


def scan(lib, data: bytes, capacity=64):
  L = lib.lib()
  buf = np.frombuffer(data, dtype=np.uint8).copy() if data else np.zeros(1, dtype=np.uint8)
  recs = (lib.Record * capacity)()
  n, used = ctypes.c_int64(-1), ctypes.c_int64(-1)
  rc = L.mmt_records_scan(R.np_ptr(buf), len(data), ctypes.addressof(recs), capacity, ctypes.byref(n), ctypes.byref(used))
  if rc != 0:
    return rc, L.mmt_last_error().decode(), None
  return 0, [(recs[i].offset, recs[i].length, recs[i].crc) for i in range(n.value)], used.value


def fields(lib, payload: bytes, names):
  L = lib.lib()
  buf = np.frombuffer(payload, dtype=np.uint8).copy() if payload else np.zeros(1, dtype=np.uint8)
  arr = (ctypes.c_char_p * len(names))(*[n.encode() for n in names])
  out = (lib.ExampleField * len(names))()
  rc = L.mmt_example_fields(R.np_ptr(buf), len(payload), len(names), arr, out)
  if rc != 0:
    return rc, L.mmt_last_error().decode()
  res = {}
  for name, f in zip(names, out):
    if f.kind == lib.MMT_FIELD_BYTES:
      res[name] = ('bytes', f.count, payload[f.offset:f.offset + f.length] if f.count else None)
    elif f.kind == lib.MMT_FIELD_INT64:
      res[name] = ('int64', f.count, f.int_value if f.count else None)
    elif f.kind == lib.MMT_FIELD_FLOAT:
      res[name] = ('float', f.count, f.float_value if f.count else None)
    else:
      res[name] = None
  return 0, res


# ---------------------------------------------------------------------------------------------------
# the constants
# ---------------------------------------------------------------------------------------------------
def test_crc_constants_through_the_oracle_and_the_host_mirror(lib):
  for data, want in R.CRC_VECTORS:
    assert R.crc32c(data) == want
  blob = np.frombuffer(b''.join(d for d, _ in R.CRC_VECTORS), dtype=np.uint8).copy()
  lens = [len(d) for d, _ in R.CRC_VECTORS]
  offs = np.cumsum([0] + lens[:-1])
  crc, bad = host_crc(lib, blob, offs, lens, stored=[R.mask(w) for _, w in R.CRC_VECTORS])
  assert [int(c) for c in crc] == [w for _, w in R.CRC_VECTORS]
  assert not bad.any()
  assert R.mask(R.crc32c(bytes(8))) == 0x07980329 and R.mask(R.crc32c(b'')) == 0xA282EAD8


def test_empty_frame_constant_through_the_writer_and_the_scan(lib):
  assert R.frame(b'') == R.EMPTY_FRAME
  rc, recs, used = scan(lib, R.EMPTY_FRAME * 3)
  assert rc == 0 and used == 48
  assert recs == [(12, 0, 0xA282EAD8), (28, 0, 0xA282EAD8), (44, 0, 0xA282EAD8)]


def test_example_constants_through_the_writer_and_the_lookup(lib):
  for feats, hexed in R.EXAMPLE_VECTORS:
    assert R.example(feats).hex() == hexed
  rc, got = fields(lib, bytes.fromhex(R.EXAMPLE_VECTORS[0][1]), ['k', 'n'])
  assert rc == 0 and got == {'k': ('bytes', 1, b'v'), 'n': None}
  rc, got = fields(lib, bytes.fromhex(R.EXAMPLE_VECTORS[1][1]), ['n'])
  assert rc == 0 and got == {'n': ('int64', 2, -1)}
  rc, got = fields(lib, bytes.fromhex(R.EXAMPLE_VECTORS[2][1]), ['f'])
  assert rc == 0 and got == {'f': ('float', 1, 1.0)}


# ---------------------------------------------------------------------------------------------------
# the scan
# ---------------------------------------------------------------------------------------------------
def _small_shard():
  payloads = [b'', b'a', bytes(range(40)), R.example({'k': ('bytes', [b'v' * 17])}), b'\x00' * 13]
  return payloads, b''.join(R.frame(p) for p in payloads)


def test_scan_at_every_prefix(lib):
  payloads, shard = _small_shard()
  ends, at = [], 0
  for p in payloads:
    at += 16 + len(p)
    ends.append(at)
  for cut in range(len(shard) + 1):
    rc, recs, used = scan(lib, shard[:cut])
    assert rc == 0, (cut, recs)
    whole = sum(1 for e in ends if e <= cut)
    assert len(recs) == whole and used == ([0] + ends)[whole], cut
    for (off, length, crc), p in zip(recs, payloads):
      assert shard[off:off + length] == p and crc == R.mask(R.crc32c(p))


def test_scan_stops_at_capacity_and_continues(lib):
  payloads, shard = _small_shard()
  rc, recs, used = scan(lib, shard, capacity=2)
  assert rc == 0 and len(recs) == 2 and used == 16 + 17
  rc, rest, used2 = scan(lib, shard[used:])
  assert rc == 0 and len(rest) == 3 and used + used2 == len(shard)


def test_scan_refuses_a_flipped_length_checksum(lib):
  _, shard = _small_shard()
  second = 16
  for at in (8, second + 3, second + 9):                   # the first frame's checksum; the second frame's length and checksum
    bad = bytearray(shard)
    bad[at] ^= 0x10
    rc, msg, _ = scan(lib, bytes(bad))
    assert rc == MMT_E_INVALID and f'byte {0 if at < second else second}' in msg, msg


def test_scan_does_not_wrap_on_a_huge_length(lib):
  for length in ((1 << 64) - 1, (1 << 64) - 16, (1 << 63), (1 << 63) - 1):
    head = struct.pack('<Q', length)
    data = R.frame(b'xy') + head + struct.pack('<I', R.mask(R.crc32c(head))) + b'\x00' * 40
    rc, recs, used = scan(lib, data)
    assert rc == 0 and len(recs) == 1 and used == 18, (length, recs, used)


# ---------------------------------------------------------------------------------------------------
# the field lookup
# ---------------------------------------------------------------------------------------------------
def test_lookup_in_any_field_order_with_a_missing_text_field(lib):
  feats = [('caption', 'bytes', [b'hello']), ('image_data', 'bytes', [b'\xff\xd8data']), ('image_key', 'bytes', [b'k1'])]
  names = ['image_data', 'image_key', 'caption', 'alt_text']
  want = {'image_data': ('bytes', 1, b'\xff\xd8data'), 'image_key': ('bytes', 1, b'k1'), 'caption': ('bytes', 1, b'hello'), 'alt_text': None}
  for order in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
    rc, got = fields(lib, R.example([feats[i] for i in order]), names)
    assert rc == 0 and got == want


def test_lookup_skips_unknown_fields_of_every_skippable_wire_type(lib):
  junk = R.varint(9 << 3 | 0) + R.varint(300) + R.varint(10 << 3 | 1) + b'\x01' * 8 + R.ld(11, b'abc') + R.varint(12 << 3 | 5) + b'\x02' * 4
  feat = R.ld(1, junk + R.ld(1, b'v') + junk + R.ld(1, b'w'))                    # BytesList with junk around two values
  ent = R.ld(1, junk + R.ld(1, b'k') + junk + R.ld(2, junk + feat + junk) + junk)
  payload = junk + R.ld(1, junk + ent + junk) + junk
  rc, got = fields(lib, payload, ['k'])
  assert rc == 0 and got == {'k': ('bytes', 2, b'v')}, got


def test_lookup_unpacked_lists_empty_value_repeats_and_no_kind(lib):
  rc, got = fields(lib, R.example([('n', 'int64', [5, -2], False), ('f', 'float', [2.5, 1.0, 0.0], False)]), ['n', 'f'])
  assert rc == 0 and got == {'n': ('int64', 2, 5), 'f': ('float', 3, 2.5)}
  rc, got = fields(lib, R.example([('e', 'bytes', [b'']), ('z', 'bytes', [])]), ['e', 'z'])
  assert rc == 0 and got == {'e': ('bytes', 1, b''), 'z': ('bytes', 0, None)}
  rc, got = fields(lib, R.example([('k', 'bytes', [b'first']), ('k', 'int64', [9])]), ['k'])       # a repeated key: the last
  assert rc == 0 and got == {'k': ('int64', 1, 9)}
  two = R.example([('a', 'bytes', [b'1'])]) + R.example([('b', 'bytes', [b'2']), ('a', 'bytes', [b'3'])])   # features merge
  rc, got = fields(lib, two, ['a', 'b'])
  assert rc == 0 and got == {'a': ('bytes', 1, b'3'), 'b': ('bytes', 1, b'2')}
  rc, got = fields(lib, R.example([('q', 'none', [])]), ['q'])
  assert rc == 0 and got == {'q': None}
  rc, got = fields(lib, b'', ['q'])
  assert rc == 0 and got == {'q': None}


def test_lookup_refusals(lib):
  good = R.example({'k': ('bytes', [b'v'])})
  for wt in (3, 4):                                          # a group tag at every level
    for payload in (R.varint(7 << 3 | wt) + good, R.ld(1, R.varint(7 << 3 | wt)), R.ld(1, R.ld(1, R.varint(7 << 3 | wt)))):
      rc, msg = fields(lib, payload, ['k'])
      assert rc == MMT_E_INVALID and 'byte' in msg, msg
  rc, msg = fields(lib, good[:1] + bytes([good[1] + 1]) + good[2:], ['k'])       # the outer length leaves the payload
  assert rc == MMT_E_INVALID and 'leaves' in msg
  inner = bytearray(good)
  inner[3] += 1                                              # the map entry's length leaves `features`
  rc, msg = fields(lib, bytes(inner), ['k'])
  assert rc == MMT_E_INVALID and 'leaves' in msg and 'byte 3' in msg, msg
  ten = b'\xff' * 9 + b'\x01'
  rc, got = fields(lib, R.example([('n', 'int64', [-1], False)]), ['n'])
  assert rc == 0 and got == {'n': ('int64', 1, -1)}
  body = R.varint(1 << 3 | 0) + ten
  assert R.example([('n', 'int64', [-1], False)]) == R.ld(1, R.entry('n', R.ld(3, body)))            # the 10-byte varint
  eleven = R.varint(1 << 3 | 0) + b'\xff' * 10 + b'\x01'
  rc, msg = fields(lib, R.ld(1, R.entry('n', R.ld(3, eleven))), ['n'])
  assert rc == MMT_E_INVALID and 'more than 10' in msg, msg
  rc, msg = fields(lib, R.ld(1, R.entry('n', R.ld(3, R.varint(1 << 3 | 0) + b'\xff\xff'))), ['n'])
  assert rc == MMT_E_INVALID and 'truncated' in msg, msg
  for cut in range(1, len(good)):                            # every truncation: an error or a clean partial answer, no fault
    rc, _ = fields(lib, good[:cut], ['k'])
    assert rc in (0, MMT_E_INVALID)


# ---------------------------------------------------------------------------------------------------
# the host mirror of the checksum kernels
# ---------------------------------------------------------------------------------------------------
def test_host_crc_on_the_length_and_alignment_grid(lib):
  blob, offs, lens, want = R.crc_grid(lib.MMT_RECORDS_PIECE, lib.MMT_RECORDS_PART)
  stored = np.asarray([R.mask(int(w)) for w in want], dtype=np.uint32)
  stored[5] ^= 1
  crc, bad = host_crc(lib, blob, offs, lens, stored)
  assert np.array_equal(crc, want)
  assert bad[5] == 1 and bad.sum() == 1


def test_host_crc_clamps_wrong_metadata(lib):
  blob = np.frombuffer(bytes(range(200)), dtype=np.uint8).copy()
  offs = [-5, 190, 500, 0, 1 << 62, -(1 << 62)]
  lens = [10, 100, 10, -3, 1 << 62, 1 << 62]
  crc, _ = host_crc(lib, blob, offs, lens)
  data = bytes(range(200))
  want = [R.crc32c(data[0:10]), R.crc32c(data[190:200]), 0, 0, 0, R.crc32c(data)]
  assert [int(c) for c in crc] == want


# ---------------------------------------------------------------------------------------------------
# the chunked reader
# ---------------------------------------------------------------------------------------------------
def test_shard_reader_carries_tails_and_grows(lib, tmp_path):
  from mmt_amd import records
  payloads = [os.urandom(n) for n in (0, 5, 300, 70, 1000, 1, 64, 2500, 12)]
  path = tmp_path / 'a.tfrecord'
  path.write_bytes(b''.join(R.frame(p) for p in payloads))
  for chunk in (16, 64, 256, 1 << 20):
    got = [bytes(p) for p, _ in records.read_shard(str(path), chunk_bytes=chunk)]
    assert got == payloads, chunk
  stored = [c for _, c in records.read_shard(str(path), chunk_bytes=64)]
  assert stored == [R.mask(R.crc32c(p)) for p in payloads]
  cut = tmp_path / 'cut.tfrecord'
  cut.write_bytes(path.read_bytes()[:-3])
  with pytest.raises(ValueError, match='truncated'):
    list(records.read_shard(str(cut), chunk_bytes=64))


def test_shard_reader_refuses_compressed_shards(lib, tmp_path):
  import gzip
  import zlib
  from mmt_amd import records
  raw = R.frame(b'payload')
  for name, data in (('g.tfrecord', gzip.compress(raw)), ('z.tfrecord', zlib.compress(raw))):
    (tmp_path / name).write_bytes(data)
    with pytest.raises(ValueError, match='compressed'):
      list(records.read_shard(str(tmp_path / name)))


def test_build_inputs_stays_synthetic_for_the_placeholder_and_refuses_an_empty_pattern(lib, tmp_path):
  from mmt_amd import pretrain_dataloader as pd
  vocab = tmp_path / 'vocab.txt'
  vocab.write_text('[PAD]\n')
  assert not pd.wants_records('', str(vocab)) and not pd.wants_records('gs://your_input_data_patterns', str(vocab))
  assert not pd.wants_records(str(tmp_path / '*.tfrecord'), '') and not pd.wants_records(str(tmp_path / '*.tfrecord'), str(tmp_path / 'no.txt'))
  assert pd.wants_records(str(tmp_path / '*.tfrecord'), str(vocab))
  with pytest.raises(ValueError, match='matches no file'):
    pd.check_input_patterns([str(tmp_path / '*.tfrecord')])


# ---------------------------------------------------------------------------------------------------
# the sanitizer program
# ---------------------------------------------------------------------------------------------------
def test_sanitizer_program_of_the_record_host_stage():
  """`make asan-records` (csrc/Makefile): mmt_records_scan, mmt_example_fields and mmt_records_crc_host under
  AddressSanitizer + UBSan, driven by a C program with its own main in exact-size heap blocks.  CPU only; nothing is
  loaded into Python."""
  import shutil
  import subprocess
  if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
    pytest.skip('no hipcc on this machine')
  csrc = os.path.join(ROOT, 'multimodal-long-transformer-2021_amd', 'csrc')
  res = subprocess.run(['make', '-s', '-C', csrc, 'asan-records'], capture_output=True, text=True, timeout=900)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
  assert 'records asan driver ok' in res.stdout and 'ERROR: AddressSanitizer' not in res.stderr and 'runtime error' not in res.stderr
