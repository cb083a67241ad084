"""Record container: the pure-Python oracle (CRC-32C bit by bit, the mask), the TFRecord / tf.train.Example writer and
the shard builders of tests/test_records.py (CPU) and tests/test_gpu_records.py (GPU).  No code of mmt_amd is used here.
The writer and the library's reader come from one hand, so both are pinned to the constants below, which were produced
independently: the CRCs by a bytewise table (and RFC 3720 B.4), the serialized messages by google.protobuf."""
import ctypes
import functools
import os
import struct

import numpy as np

from tests import _jpeg_cases as JC
from tests import _text_cases as TC

CRC_VECTORS = ((b'123456789', 0xE3069283), (bytes(32), 0x8A9136AA), (b'\xff' * 32, 0x62A8AB43), (bytes(range(32)), 0x46DD794E),
               (b'', 0))
EMPTY_FRAME = bytes.fromhex('0000000000000000' '29039807' 'd8ea82a2')
EXAMPLE_VECTORS = (
    ({'k': ('bytes', [b'v'])}, '0a0c0a0a0a016b12050a030a0176'),
    ({'n': ('int64', [-1, 300])}, '0a170a150a016e12101a0e0a0cffffffffffffffffff01ac02'),
    ({'f': ('float', [1.0])}, '0a0f0a0d0a0166120812060a040000803f'),
)


# ---------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table():
  t = []
  for v in range(256):
    c = v
    for _ in range(8):
      c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
    t.append(c)
  return tuple(t)


def crc32c(data) -> int:
  t = _table()
  c = 0xFFFFFFFF
  for b in bytes(data):
    c = t[(c ^ b) & 0xFF] ^ (c >> 8)
  return c ^ 0xFFFFFFFF


def mask(c: int) -> int:
  return (((c >> 15) | (c << 17)) + 0xa282ead8) & 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------
def frame(payload: bytes) -> bytes:
  head = struct.pack('<Q', len(payload))
  return head + struct.pack('<I', mask(crc32c(head))) + payload + struct.pack('<I', mask(crc32c(payload)))


def varint(v: int) -> bytes:
  v &= (1 << 64) - 1
  out = bytearray()
  while True:
    if v < 0x80:
      out.append(v)
      return bytes(out)
    out.append((v & 0x7F) | 0x80)
    v >>= 7


def ld(field: int, body: bytes) -> bytes:
  """A length-delimited field."""
  return varint(field << 3 | 2) + varint(len(body)) + body


def feature(kind: str, values, packed=True) -> bytes:
  if kind == 'bytes':
    return ld(1, b''.join(ld(1, bytes(v)) for v in values))
  if kind == 'float':
    if packed:
      return ld(2, ld(1, b''.join(struct.pack('<f', v) for v in values)))
    return ld(2, b''.join(varint(1 << 3 | 5) + struct.pack('<f', v) for v in values))
  if kind == 'int64':
    if packed:
      return ld(3, ld(1, b''.join(varint(v) for v in values)))
    return ld(3, b''.join(varint(1 << 3 | 0) + varint(v) for v in values))
  if kind == 'none':
    return b''
  raise ValueError(kind)


def entry(key, feature_bytes: bytes) -> bytes:
  key = key.encode() if isinstance(key, str) else key
  return ld(1, ld(1, key) + ld(2, feature_bytes))


def example(features) -> bytes:
  """features: a dict {name: (kind, values)} or a list of (name, kind, values[, packed]) in wire order."""
  items = [(k, *v) for k, v in features.items()] if isinstance(features, dict) else list(features)
  return ld(1, b''.join(entry(it[0], feature(it[1], it[2], *it[3:])) for it in items))


# ---------------------------------------------------------------------------------------------------
# shards for the loader: golden JPEG files and texts from the corpus
# ---------------------------------------------------------------------------------------------------
FIELD_DICT = {'caption': '[ATT]', 'alt_text': '[ALT]'}


def write_vocab(path) -> str:
  """The text tests' vocabulary as a vocab.txt, with the [PATCH] token the image half needs appended (ids unchanged)."""
  with open(path, 'wb') as f:
    f.write('\n'.join(TC.vocab_tokens() + ('[PATCH]',)).encode('utf-8') + b'\n')
  return str(path)


@functools.lru_cache(maxsize=None)
def image_names():
  """Fixtures the decoder accepts, smallest first so shards stay small."""
  ok = [n for n in JC.names() if n not in JC.REFUSALS and not n.startswith('refuse')]
  return tuple(sorted(ok, key=lambda n: len(JC.data(n)))[:12])


def loader_records(n, short_every=0, unique_texts=False):
  """n dicts {image, key, caption, alt_text}: image i is a golden file, the texts come from the corpus (at least 6
  wordpieces unless `short_every` makes every such record a one-word text; with unique_texts one caption per image)."""
  names = image_names()
  long_texts = [t for t in TC.corpus() if len(TC.field_pieces(TC.vocab_dict(), TC.enc(t), TC.special_ids()[1])) >= 8]
  recs = []
  for i in range(n):
    name = names[i % len(names)]
    cap = long_texts[(i % len(names)) if unique_texts else i]
    alt = '' if i % 3 == 0 else long_texts[-1 - i]
    if short_every and i % short_every == short_every - 1:
      cap, alt = 'ab', ''
    recs.append({'image': name, 'key': f'key-{i % len(names)}', 'caption': cap, 'alt_text': alt, 'short': cap == 'ab'})
  return recs


def record_payload(rec) -> bytes:
  feats = [('image_key', 'bytes', [rec['key'].encode()]), ('caption', 'bytes', [rec['caption'].encode('utf-8')]),
           ('image_data', 'bytes', [JC.data(rec['image'])]), ('other', 'int64', [7, 8])]
  if rec['alt_text'] != '':                                      # a missing text field is '' (FixedLenFeature default)
    feats.insert(1, ('alt_text', 'bytes', [rec['alt_text'].encode('utf-8')]))
  return example(feats)


def write_shards(directory, recs, n_shards, prefix='shard') -> list:
  """Deals the records round-robin over n_shards files; returns the sorted paths."""
  paths = []
  for s in range(n_shards):
    path = os.path.join(str(directory), f'{prefix}-{s:05d}-of-{n_shards:05d}.tfrecord')
    with open(path, 'wb') as f:
      for rec in recs[s::n_shards]:
        f.write(frame(record_payload(rec)))
    paths.append(path)
  return sorted(paths)


# ---------------------------------------------------------------------------------------------------
# ctypes helpers
# ---------------------------------------------------------------------------------------------------
def np_ptr(a):
  return a.ctypes.data_as(ctypes.c_void_p)


def crc_grid_lengths(piece, part):
  return (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, piece - 1, piece, piece + 1, part - 1, part, part + 1, 2 * part + 3,
          3 * part)


@functools.lru_cache(maxsize=None)
def crc_grid(piece, part):
  """One blob for the whole grid: every length at every start alignment 0..15 (pads of sentinel bytes in front, so a read
  outside a payload changes the result).  Returns (blob uint8, offsets, lengths, expected CRCs), computed once."""
  rng = np.random.default_rng(77)
  chunks, offs, lens, want, n = [], [], [], [], 0
  for length in crc_grid_lengths(piece, part):
    data = rng.integers(0, 256, size=length, dtype=np.uint8).tobytes()
    c = crc32c(data)
    for align in range(16):
      pad = (align - n) % 16 or 16
      chunks.append(b'\xa5' * pad)
      n += pad
      offs.append(n); lens.append(length); want.append(c)
      chunks.append(data)
      n += length
  blob = np.frombuffer(b''.join(chunks), dtype=np.uint8).copy()
  return blob, np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64), np.asarray(want, dtype=np.uint32)
