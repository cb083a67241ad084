"""PNG inflate on the device: the streams and the call helpers shared by tests/test_png_inflate.py (CPU, through
mmt_png_gather and mmt_png_scanlines_host) and tests/test_gpu_png_inflate.py (GPU, through mmt_png_scanlines).  Every
stream is built here, with Python's zlib or bit by bit with the writer of tests/test_png_decode.py, and wrapped as an
8-bit grey image whose rows start with the filter bytes 0 to 4 in turn; nothing is committed.  The reference is
zlib.decompress and the library's host inflate; parity is bit for bit."""
import ctypes
import functools
import struct
import zlib

import numpy as np

from tests import test_png_decode as D
from tests._png_cases import SIGNATURE, chunk, ihdr, idats

SUBSEQ = (8, 128)
ROUND = {s: 256 * s for s in (8, 32, 128)}                      # compressed bytes a round stages

ST = dict(OK=0, TRUNCATED=1, BLOCK_TYPE=2, STORED_LEN=3, CODE_LENGTHS=4, BAD_CODE=5, DISTANCE=6, TOO_LONG=7, TOO_SHORT=8, ADLER=9,
          FILTER=10, NO_PROGRESS=11)


def lines(content: bytes, w: int) -> bytes:
  """The scanlines of an 8-bit grey image w pixels wide whose samples are `content` (cut to whole rows): row r starts
  with filter byte r % 5."""
  h = len(content) // w
  rows = np.frombuffer(content[:h * w], dtype=np.uint8).reshape(h, w)
  out = np.empty((h, w + 1), dtype=np.uint8)
  out[:, 0] = np.arange(h) % 5
  out[:, 1:] = rows
  return out.tobytes()


def wrap(stream: bytes, w: int, h: int, split=None) -> bytes:
  """A grey 8-bit PNG file of h rows of 1 + w bytes around a zlib stream."""
  return SIGNATURE + ihdr(w, h, 8, 0) + idats(stream, split) + chunk(b'IEND')


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush=None, step=(300, 700), seed=0):
  """zlib's stream for raw; with `flush`, a flush of that kind every 300 to 700 bytes."""
  co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
  if flush is None:
    return co.compress(raw) + co.flush()
  rng = np.random.default_rng(seed)
  out, at = [], 0
  while at < len(raw):
    n = int(rng.integers(step[0], step[1] + 1))
    out.append(co.compress(raw[at:at + n]))
    out.append(co.flush(flush))
    at += n
  out.append(co.flush())
  return b''.join(out)


def text_like(n, seed=1):
  """Structured bytes: words of a small vocabulary, numbers and line ends."""
  rng = np.random.default_rng(seed)
  vocab = [bytes(rng.integers(97, 123, size=int(k), dtype=np.uint8)) for k in rng.integers(2, 10, size=3000)]
  out, size = [], 0
  while size < n:
    w = vocab[int(rng.zipf(1.3)) % len(vocab)]
    sep = b'\n' if rng.random() < 0.08 else (b' %d ' % int(rng.integers(0, 1000)) if rng.random() < 0.1 else b' ')
    out.append(w + sep)
    size += len(w) + len(sep)
  return b''.join(out)[:n]


def fixed_stream(symbols, data):
  """One final block of the fixed code around `symbols`, as a zlib stream that claims `data`."""
  w = D.BitWriter()
  D.fixed_block(w, symbols, 1)
  return D.zlib_stream(w, data)


@functools.lru_cache(maxsize=None)
def stress_cases():
  """{name: (file bytes, scanlines or None when the stream is invalid, expected status or None for 'any non-zero')}.
  Sized so that at subseq_bytes 128 the stream spans at least three rounds (3 * 32 KB compressed), except where the
  content compresses too well for that: those are sized for three rounds at subseq_bytes 8 (3 * 2 KB) and say so."""
  rng = np.random.default_rng(77)
  cases = {}

  def add(name, raw, stream, w, min_comp):
    assert len(raw) % (w + 1) == 0 and zlib.decompress(stream) == raw, name
    assert len(stream) >= min_comp, (name, len(stream))
    cases[name] = (wrap(stream, w, len(raw) // (w + 1)), raw, 0)

  big, small = 3 * ROUND[128], 3 * ROUND[8]
  # literals only: pure self-synchronisation across rounds
  noise = lines(rng.integers(0, 256, size=110 * 1000, dtype=np.uint8).tobytes(), 999)
  add('noise huffman-only', noise, deflate(noise, 6, zlib.Z_HUFFMAN_ONLY), 999, big)
  # many blocks and empty stored blocks, several end-of-block codes in a round, block starts at every bit offset
  text = lines(text_like(520 * 1000), 999)
  add('text sync-flush', text, deflate(text, 6, flush=zlib.Z_SYNC_FLUSH), 999, big)
  add('text full-flush', text, deflate(text, 6, flush=zlib.Z_FULL_FLUSH), 999, big)
  add('text fixed', text, deflate(text, 6, zlib.Z_FIXED, flush=zlib.Z_SYNC_FLUSH), 999, big)
  add('text rle', text, deflate(text, 6, zlib.Z_RLE, flush=zlib.Z_SYNC_FLUSH), 999, big)
  add('text filtered', text, deflate(text, 6, zlib.Z_FILTERED, flush=zlib.Z_SYNC_FLUSH), 999, big)
  # self-overlapping copies, a round that writes far more than it stages, a match chain as long as the round.  These
  # compress about a thousand times, so 300 KB would be one round of a few hundred bytes: sized for three rounds at 8.
  one = lines(bytes([3]) * (6400 * 1000), 3999)
  add('one value', one, deflate(one, 9), 3999, small)
  period3 = lines(b'\x01\x02\x03' * (6400 * 1000 // 3), 3999)
  add('period 3', period3, deflate(period3, 9), 3999, small)
  # dependent matches between lanes within a round (the resolution rule).  About twenty times: three rounds at 8 are
  # 6 KB; the size below gives more than three rounds at 32 as well.
  mut = bytearray(b'\x01\x02\x03' * (900 * 1000 // 3))
  at = 0
  while True:
    at += int(rng.integers(50, 91))
    if at >= len(mut):
      break
    mut[at] = int(rng.integers(4, 256))
  mutated = lines(bytes(mut), 999)
  add('period 3 mutated', mutated, deflate(mutated, 9), 999, 3 * ROUND[32])
  # the far edge of the window: 64 KB repeated at distance exactly 32768 (zlib never writes that distance), and the
  # status "distance before the start" on the first copy.  DEFLATE cannot code a distance of 32769 (the last distance
  # symbol ends at 24577 + 8191), so the copy that reaches one byte before the start is distance 32768 behind 32767 bytes.
  w = 32767
  head = b'\x00' + rng.integers(0, 256, size=w, dtype=np.uint8).tobytes()                     # one row: filter byte 0, 32767 samples
  far = head * 3                                                                             # rows two and three repeat the first
  copies = [(258, 32768)] * 254 + [(4, 32768)]                                               # 65536 bytes
  good = fixed_stream(list(head) + copies + [256], far)
  assert zlib.decompress(good) == far
  cases['distance 32768'] = (wrap(good, w, 3), far, 0)
  bad = fixed_stream(list(head[:-1]) + copies + [256], far)
  cases['distance 32768 behind 32767 bytes'] = (wrap(bad, w, 3), None, ST['DISTANCE'])
  # round boundaries: raw sizes 2 (the smallest image; size 1 is no image and is tested through the descriptors alone) and
  # the sizes one below, at and one above the bytes a round stages, as noise that the Huffman-only stream barely shrinks
  for n in (2, ROUND[8] - 1, ROUND[8], ROUND[8] + 1, ROUND[128] - 1, ROUND[128], ROUND[128] + 1):
    raw = lines(rng.integers(0, 256, size=n - 1, dtype=np.uint8).tobytes(), n - 1)
    cases[f'raw size {n}'] = (wrap(deflate(raw, 6, zlib.Z_HUFFMAN_ONLY), n - 1, 1), raw, 0)
  return cases


@functools.lru_cache(maxsize=None)
def corner_cases():
  """The hand-built corners of tests/test_png_decode.py, restated: {name: (file, scanlines)}."""
  rng = np.random.default_rng(9)
  noise = lambda n: b'\x00' + rng.integers(0, 256, size=n - 1, dtype=np.uint8).tobytes()
  out = {}
  data = noise(65535 + 10)
  w = D.BitWriter()
  D.stored_block(w, data[:10], 0); D.stored_block(w, b'', 0); D.stored_block(w, data[10:], 1)
  out['stored: empty and 65535 bytes'] = (D.zlib_stream(w, data), data)
  head = noise(32768)
  data = head + head[:258] + bytes([head[257]]) * 258 + b'\x07'
  w = D.BitWriter()
  D.stored_block(w, head, 0)
  D.fixed_block(w, [(258, 32768), (258, 1), 7, 256], 1)
  out['length 258 at distances 32768 and 1'] = (D.zlib_stream(w, data), data)
  lit = [0] * 286
  for s in range(8):
    lit[s] = 4
  for s in (97, 256, 261, 285):
    lit[s] = 3
  cl = [0] * 19
  for s in (0, 1, 2, 3, 4, 16, 17, 18):
    cl[s] = 3
  symbols = list(range(8)) + [97, (258, 1), (7, 1), 97, 256]
  data = bytes(range(8)) + b'a' * (1 + 258 + 7 + 1)
  w = D.BitWriter()
  used = D.dynamic_block(w, symbols, lit, [1], cl, 1)
  assert {16, 17, 18} <= used
  out['symbols 16, 17, 18 and a single distance code'] = (D.zlib_stream(w, data), data)
  return {k: (wrap(s, len(d) - 1, 1), d) for k, (s, d) in out.items() if zlib.decompress(s) == d}


@functools.lru_cache(maxsize=None)
def status_cases():
  """One hand-built stream per row of the MMT_PNG_ST_* enum: {name: (file, status)}.  The image is 3 rows of 1 + 4
  bytes.  MMT_PNG_ST_NO_PROGRESS has no stream: lane 0 enters a round at an exact token start, so a round either takes
  a token or ends the image with that token's status; the word guards the loop bound against a mistake in the code."""
  g8 = np.arange(12, dtype=np.uint8).reshape(3, 4)
  from tests import _png_cases as P
  raw = P.scanlines('g8', g8, 1)
  good = P.deflate(raw)

  def stream_of(build, data=raw):
    w = D.BitWriter()
    build(w)
    return D.zlib_stream(w, data)

  def oversubscribed(w):
    w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(0, 4)
    for n in (1, 1, 1, 0):
      w.bits(n, 3)

  f = lambda stream, w=4: wrap(stream, w, 3)
  return {
      'ok': (f(good), ST['OK']),
      'truncated': (f(good[:-6]), ST['TRUNCATED']),
      'block type': (f(stream_of(lambda w: w.bits(7, 3))), ST['BLOCK_TYPE']),
      'stored length': (f(stream_of(lambda w: (w.bits(1, 3), w.align(), w.raw(b'\x0f\x00\x0f\x00' + raw)))), ST['STORED_LEN']),
      'code lengths': (f(stream_of(oversubscribed)), ST['CODE_LENGTHS']),
      'bad code (length symbol 286)': (f(stream_of(lambda w: (w.bits(1, 1), w.bits(1, 2), w.code(0b11000110, 8)))), ST['BAD_CODE']),
      'bad code (distance symbol 30)': (f(stream_of(lambda w: (w.bits(1, 1), w.bits(1, 2), w.code(0b00110000, 8), w.code(1, 7), w.code(30, 5)))),
                                        ST['BAD_CODE']),
      'distance': (f(stream_of(lambda w: D.fixed_block(w, [0, 1, (3, 3), 256], 1))), ST['DISTANCE']),
      'too long': (f(P.deflate(raw + b'\x00')), ST['TOO_LONG']),
      'too long (stored)': (f(P.deflate(raw + b'\x00', 'stored')), ST['TOO_LONG']),
      'too short': (f(P.deflate(raw[:-1])), ST['TOO_SHORT']),
      'adler': (f(good[:-4] + bytes([good[-4] ^ 1]) + good[-3:]), ST['ADLER']),
      'filter byte': (f(P.deflate(raw[:5] + b'\x05' + raw[6:])), ST['FILTER']),
  }


# ---------------------------------------------------------------------------------------------------
# the calls
# ---------------------------------------------------------------------------------------------------
class Batch:
  """Files gathered for one mmt_png_scanlines call: images, streams, comp (uint8), pal, the raw layout, and per file the
  host inflate's verdict (`host_ok`) and scanlines (`host_raw`).  A file mmt_png_info or mmt_png_gather refuses is left
  out of the call (`refused`): the host inflate refuses it too, which is asserted here."""

  def __init__(self, lib, blobs, guard=0):
    L = lib.lib()
    self.refused, kept = [], []
    for i, b in enumerate(blobs):
      im = lib.PngImage()
      if L.mmt_png_info(b, len(b), ctypes.byref(im)) != 0:
        self.refused.append(i)
        continue
      kept.append((i, b, im))
    self.index = []
    images = (lib.PngImage * max(len(kept), 1))()
    streams = (lib.PngStream * max(len(kept), 1))()
    n_comp = sum(len(b) for _, b, _ in kept) or 1
    comp = np.zeros(n_comp, dtype=np.uint8)
    pal = np.zeros(max(len(kept), 1) * 768, dtype=np.uint8)
    self.host_ok, self.host_raw = [], []
    k, at_comp, at_raw = 0, 0, guard
    for i, b, im in kept:
      raw = np.zeros(max(im.raw_bytes, 1), dtype=np.uint8)
      hp = np.zeros(768, dtype=np.uint8)
      host_rc = L.mmt_png_inflate(b, len(b), ctypes.byref(im), raw.ctypes.data, im.raw_bytes, hp.ctypes.data)
      st = lib.PngStream(at_comp, 0)
      rc = L.mmt_png_gather(b, len(b), ctypes.byref(im), comp.ctypes.data, n_comp, ctypes.byref(st), pal.ctypes.data + 768 * k)
      if rc != 0:
        assert host_rc != 0, 'mmt_png_gather refuses a file the host inflate accepts'
        self.refused.append(i)
        continue
      assert host_rc != 0 or np.array_equal(hp, pal[768 * k:768 * k + 768])
      images[k] = im
      images[k].raw_offset = at_raw
      streams[k] = st
      at_comp += st.comp_bytes
      at_raw += im.raw_bytes
      self.index.append(i); self.host_ok.append(host_rc == 0); self.host_raw.append(raw[:im.raw_bytes])
      k += 1
    self.B, self.images, self.streams, self.comp, self.pal = k, images, streams, comp, pal
    self.n_comp, self.n_raw, self.guard = n_comp, at_raw + guard, guard

  def stream(self, k):
    s = self.streams[k]
    return bytes(self.comp[s.comp_offset:s.comp_offset + s.comp_bytes])

  def slice(self, raw, k):
    im = self.images[k]
    return raw[im.raw_offset:im.raw_offset + im.raw_bytes]


def run_host(lib, batch, subseq, sentinel=0):
  """mmt_png_scanlines_host on a Batch: (raw uint8 [n_raw], status int32 [B])."""
  L = lib.lib()
  raw = np.full(batch.n_raw, sentinel, dtype=np.uint8)
  status = np.full(batch.B, -7, dtype=np.int32)
  need = L.mmt_png_scanlines_workspace_bytes(batch.B)
  work = np.empty(need, dtype=np.uint8)
  lib.check(L.mmt_png_scanlines_host(batch.B, batch.images, batch.streams, batch.comp.ctypes.data, batch.n_comp, raw.ctypes.data, batch.n_raw,
                                     status.ctypes.data, subseq, work.ctypes.data, need))
  return raw, status


def run_device(lib, batch, subseq, sentinel=0):
  """mmt_png_scanlines on a Batch, on the current GPU: (raw uint8 [n_raw], status int32 [B]) as numpy."""
  import torch
  L = lib.lib()
  dev = lambda a: torch.from_numpy(np.frombuffer(bytes(a), dtype=np.uint8).copy()).cuda()
  images, streams, comp = dev(batch.images), dev(batch.streams), torch.from_numpy(batch.comp).cuda()
  raw = torch.full((batch.n_raw,), sentinel, dtype=torch.uint8, device='cuda')
  status = torch.full((batch.B,), -7, dtype=torch.int32, device='cuda')
  need = L.mmt_png_scanlines_workspace_bytes(batch.B)
  work = torch.empty(need, dtype=torch.uint8, device='cuda')
  lib.check(L.mmt_png_scanlines(batch.B, images.data_ptr(), streams.data_ptr(), comp.data_ptr(), batch.n_comp, raw.data_ptr(), batch.n_raw,
                                status.data_ptr(), subseq, work.data_ptr(), need, torch.cuda.current_stream().cuda_stream))
  torch.cuda.synchronize()
  return raw.cpu().numpy(), status.cpu().numpy()


def check_equivalence(batch, raw, status, where='', sentinel=0):
  """The contract: status 0 exactly when the host inflate accepts the file, and then the same bytes."""
  for k in range(batch.B):
    assert (status[k] == 0) == batch.host_ok[k], (where, batch.index[k], int(status[k]), batch.host_ok[k])
    assert 0 <= status[k] <= 11, (where, batch.index[k], int(status[k]))
    if batch.host_ok[k]:
      assert np.array_equal(batch.slice(raw, k), batch.host_raw[k]), (where, batch.index[k])
  if batch.guard:
    assert np.all(raw[:batch.guard] == sentinel) and np.all(raw[-batch.guard:] == sentinel), where


def mutations(blob):
  """Every prefix and every single-byte corruption (four values per byte) of a file's zlib stream, each wrapped again
  as the file's one IDAT chunk with a fresh CRC-32: the chunk walk accepts them all, so the inflate decides."""
  from tests import _png_cases as P
  cs = P.chunks_of(blob)
  stream = b''.join(c[1] for c in cs if c[0] == b'IDAT')
  first = [c[0] for c in cs].index(b'IDAT')
  head = SIGNATURE + b''.join(chunk(t, body) for t, body, _ in cs[:first])
  file_of = lambda s: head + chunk(b'IDAT', s) + chunk(b'IEND')
  out = [file_of(stream[:n]) for n in range(len(stream) + 1)]
  for at in range(len(stream)):
    keep = stream[at]
    for v in sorted({0x00, 0xFF, keep ^ 0xFF, keep ^ 1} - {keep}):
      out.append(file_of(stream[:at] + bytes([v]) + stream[at + 1:]))
  return out
