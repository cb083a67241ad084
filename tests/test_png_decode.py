"""PNG decode without a GPU: the numpy oracle against the committed Pillow decodes, the host stage (mmt_png_info,
mmt_png_inflate) against the oracle byte for byte, the library's inflate against zlib on streams built to reach its
corners, mmt_png_pixels_host and the Python entry points against the committed pixels -- all bit for bit -- every refusal
with its reason, the loader on a shard of PNG files, and the sanitizer program (`make asan-png`)."""
import ctypes
import io
import itertools
import json
import os
import struct
import types
import zlib

import numpy as np
import pytest

from tests import _jpeg_cases as J
from tests import _png_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope='module')
def lib():
  import __graft_entry__  # noqa: F401  (sets sys.path)
  from mmt_amd import _lib
  _lib.build()
  return _lib


def test_fixture_set_is_the_stated_one_and_small():
  plan = P.plan()
  assert list(P.names()) == [p[0] for p in plan] + list(P.EXTRA)
  assert len(plan) == len(P.SIZES) * len(P.KINDS) == 99
  pairs = lambda i, j: {(p[i], p[j]) for p in plan}
  size = lambda p: (p[1], p[2])
  assert len(pairs(3, 4)) == len(P.KINDS) * len(P.FILTERS)                # every (kind, filter)
  for field, values in ((4, P.FILTERS), (5, (0, 1)), (6, P.BLOCKS), (7, P.SPLITS)):
    assert {(size(p), p[field]) for p in plan} == {(s, v) for s in P.SIZES for v in values}, field      # every value at every size
  for name, *_ in plan:
    assert P.build(name) == P.data(name), name                   # the committed files are the writer's
  # zlib takes the cheapest block type, so the smallest files do not hold what their strategy names: the three real
  # types (the first block's BTYPE) still occur with both interlace methods
  first_block = lambda n: (b''.join(c[1] for c in P.chunks_of(P.data(n)) if c[0] == b'IDAT')[2] >> 1) & 3
  assert {(first_block(p[0]), p[5]) for p in plan} == {(t, lace) for t in (0, 1, 2) for lace in (0, 1)}
  files = os.listdir(P.GOLDEN)
  assert sorted(files) == sorted([n + '.png' for n in P.names()] + ['fixtures.txt', 'expected_pixels.rgb'])
  assert all(os.path.getsize(os.path.join(P.GOLDEN, n + '.png')) <= 16 * 1024 for n in P.names())
  assert sum(os.path.getsize(os.path.join(P.GOLDEN, f)) for f in files) <= 1024 * 1024
  short = P.decode('short_palette')
  assert short.palette_entries == 5 and int(np.frombuffer(short.raw, dtype=np.uint8).max()) >> 4 >= 5   # indices beyond the entries


def test_oracle_equals_the_committed_pillow_decode_on_every_fixture():
  for name in P.names():
    d = P.decode(name)
    assert d.rgb.shape == P.expected(name).shape, name
    assert np.array_equal(d.rgb, P.expected(name)), name


def test_oracle_and_committed_pixels_equal_a_live_pillow_decode():
  Image = pytest.importorskip('PIL.Image')
  for name in P.names():
    live = np.asarray(Image.open(io.BytesIO(P.data(name))).convert('RGB'))
    assert np.array_equal(live, P.expected(name)), name


def test_info_and_inflate_equal_the_oracle_and_stay_inside_the_raw_block(lib):
  L = lib.lib()
  for name in P.names():
    d, raw = P.decode(name), P.data(name)
    im = lib.PngImage()
    lib.check(L.mmt_png_info(raw, len(raw), ctypes.byref(im)))
    assert (im.width, im.height, im.bit_depth, im.color_type, im.interlace, im.palette_entries) == \
        (d.width, d.height, d.depth, d.color_type, d.interlace, d.palette_entries), name
    assert (im.raw_offset, im.raw_bytes, im.pixel_offset) == (0, len(d.raw), 0), name
    images, buf, pal, _, _ = P.host_stage(lib, [raw], guard=64)
    assert bytes(buf[64:-64]) == d.raw, name
    assert np.all(buf[:64] == P.SENTINEL) and np.all(buf[-64:] == P.SENTINEL), name
    assert np.array_equal(pal.reshape(256, 3), d.palette), name


def test_pixels_host_equals_the_expected_pixels(lib):
  L = lib.lib()
  names = list(P.names())
  for batch in [[n] for n in names] + [names[::-1]]:
    images, raw, pal, offs, n = P.host_stage(lib, [P.data(b) for b in batch])
    out = np.full(n + P.GUARD, P.SENTINEL, dtype=np.uint8)
    work = np.full(raw.size, 0xFF, dtype=np.uint8)
    lib.check(L.mmt_png_pixels_host(len(batch), images, raw.ctypes.data, raw.size, pal.ctypes.data, out.ctypes.data, n,
                                    work.ctypes.data, work.size))
    P.check_packed(out, [P.expected(b) for b in batch], offs)


# ---------------------------------------------------------------------------------------------------
# the inflate at its corners: streams written bit by bit, against zlib.decompress
# ---------------------------------------------------------------------------------------------------
class BitWriter:
  def __init__(self):
    self.out, self.acc, self.n = bytearray(), 0, 0

  def bits(self, value, n):                                      # least significant bit first
    self.acc |= value << self.n
    self.n += n
    while self.n >= 8:
      self.out.append(self.acc & 255)
      self.acc >>= 8
      self.n -= 8

  def code(self, code, n):                                       # a Huffman code: most significant bit first
    self.bits(int(format(code, f'0{n}b')[::-1], 2), n)

  def align(self):
    if self.n:
      self.bits(0, 8 - self.n)

  def raw(self, data):
    assert self.n == 0
    self.out += data


def canonical(lengths):
  """{symbol: (code, length)} of a list of code lengths (RFC 1951, 3.2.2)."""
  codes, code = {}, 0
  for n in range(1, 16):
    for s, l in enumerate(lengths):
      if l == n:
        codes[s] = (code, n)
        code += 1
    code <<= 1
  return codes


LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


def put_symbols(w, symbols, lit, dist):
  """symbols: ints (literals, 256 = end of block) and (length, distance) pairs."""
  for s in symbols:
    if isinstance(s, int):
      w.code(*lit[s])
      continue
    length, distance = s
    li = max(i for i in range(29) if LEN_BASE[i] <= length and (i == 28) == (length == 258))
    w.code(*lit[257 + li])
    w.bits(length - LEN_BASE[li], LEN_EXTRA[li])
    di = max(i for i in range(30) if DIST_BASE[i] <= distance)
    w.code(*dist[di])
    w.bits(distance - DIST_BASE[di], DIST_EXTRA[di])


def stored_block(w, data, final):
  w.bits(final, 1); w.bits(0, 2); w.align()
  w.raw(struct.pack('<HH', len(data), len(data) ^ 0xFFFF) + data)


def fixed_block(w, symbols, final):
  w.bits(final, 1); w.bits(1, 2)
  put_symbols(w, symbols, canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), canonical([5] * 30))


def dynamic_block(w, symbols, lit_lengths, dist_lengths, cl_lengths, final):
  """A dynamic block whose code lengths are run-length coded with symbols 16, 17 and 18 wherever they apply."""
  w.bits(final, 1); w.bits(2, 2)
  seq, used = list(lit_lengths) + list(dist_lengths), set()
  ops, i = [], 0
  while i < len(seq):
    run = 1
    while i + run < len(seq) and seq[i + run] == seq[i]:
      run += 1
    if seq[i] == 0 and run >= 11:
      n = min(run, 138); ops.append((18, n - 11, 7)); i += n
    elif seq[i] == 0 and run >= 3:
      ops.append((17, run - 3, 3)); i += run
    elif seq[i] != 0 and run >= 4:
      n = min(run - 1, 6); ops += [(seq[i], 0, 0), (16, n - 3, 2)]; i += 1 + n
    else:
      ops.append((seq[i], 0, 0)); i += 1
  used = {o[0] for o in ops}
  order = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
  assert all(cl_lengths[s] for s in used)
  ncode = max(i for i in range(19) if cl_lengths[order[i]]) + 1
  w.bits(len(lit_lengths) - 257, 5); w.bits(len(dist_lengths) - 1, 5); w.bits(ncode - 4, 4)
  for i in range(ncode):
    w.bits(cl_lengths[order[i]], 3)
  cl = canonical(cl_lengths)
  for sym, extra, nbits in ops:
    w.code(*cl[sym])
    w.bits(extra, nbits)
  put_symbols(w, symbols, canonical(lit_lengths), canonical(dist_lengths))
  return used


def zlib_stream(w, data):
  w.align()
  return b'\x78\x9c' + bytes(w.out) + struct.pack('>I', zlib.adler32(data))


def through_the_library(lib, stream, n):
  """The library's inflate on a zlib stream of n bytes: as the one scanline of an 8-bit grey file n - 1 pixels wide (the
  first byte is the filter type, so it must be at most 4)."""
  L = lib.lib()
  raw = P.SIGNATURE + P.ihdr(n - 1, 1, 8, 0) + P.chunk(b'IDAT', stream) + P.chunk(b'IEND')
  im = lib.PngImage()
  lib.check(L.mmt_png_info(raw, len(raw), ctypes.byref(im)))
  assert im.raw_bytes == n
  out = np.full(n + 32, P.SENTINEL, dtype=np.uint8)
  im.raw_offset = 16
  pal = np.zeros(768, dtype=np.uint8)
  lib.check(L.mmt_png_inflate(raw, len(raw), ctypes.byref(im), out.ctypes.data, out.size, pal.ctypes.data))
  assert np.all(out[:16] == P.SENTINEL) and np.all(out[-16:] == P.SENTINEL)
  return bytes(out[16:-16])


def test_inflate_equals_zlib_at_its_corners(lib):
  rng = np.random.default_rng(9)
  noise = lambda n: b'\x00' + rng.integers(0, 256, size=n - 1, dtype=np.uint8).tobytes()
  cases = {}
  # an empty stored block between two others, and a stored block of 65535 bytes
  data = noise(65535 + 10)
  w = BitWriter()
  stored_block(w, data[:10], 0); stored_block(w, b'', 0); stored_block(w, data[10:], 1)
  cases['stored'] = (zlib_stream(w, data), data)
  # length 258 at distance 1, and at distance 32768, by the fixed code
  head = noise(32768)
  data = head + head[:258] + bytes([head[257]]) * 258 + b'\x07'
  w = BitWriter()
  stored_block(w, head, 0)
  fixed_block(w, [(258, 32768), (258, 1), 7, 256], 1)
  cases['long matches'] = (zlib_stream(w, data), data)
  # a dynamic block whose lengths use the symbols 16, 17 and 18, with a single distance code (one bit, distance 1)
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
  w = BitWriter()
  used = dynamic_block(w, symbols, lit, [1], cl, 1)
  assert {16, 17, 18} <= used
  cases['dynamic'] = (zlib_stream(w, data), data)
  # what zlib itself writes for runs and noise, all three strategies
  mixed = b'\x00' + bytes(300) + noise(2000) + b'abcabcabc' * 400
  for block in P.BLOCKS:
    cases['zlib ' + block] = (P.deflate(mixed, block), mixed)
  for name, (stream, data) in cases.items():
    assert zlib.decompress(stream) == data, name                 # the stream is what it claims to be
    assert through_the_library(lib, stream, len(data)) == data, name


# ---------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------
def outcome(lib, raw):
  """(code, message) of mmt_png_info then mmt_png_inflate on a file: the first failure, or (0, '')."""
  L = lib.lib()
  im = lib.PngImage()
  rc = L.mmt_png_info(raw, len(raw), ctypes.byref(im))
  if rc == 0:
    out = np.zeros(max(im.raw_bytes, 1), dtype=np.uint8)
    pal = np.zeros(768, dtype=np.uint8)
    rc = L.mmt_png_inflate(raw, len(raw), ctypes.byref(im), out.ctypes.data, im.raw_bytes, pal.ctypes.data)
  return rc, (L.mmt_last_error().decode() if rc else '')


def file_of(header, stream, plte=b'', extra=b'', idat_crc=None, iend_crc=None):
  return P.SIGNATURE + header + plte + extra + P.chunk(b'IDAT', stream, idat_crc) + P.chunk(b'IEND', b'', iend_crc)


def test_every_refusal_returns_its_code_and_names_its_reason(lib):
  g8 = np.arange(12, dtype=np.uint8).reshape(3, 4)
  lines = P.scanlines('g8', g8, 1)                              # 3 rows of 1 + 4 bytes
  good = P.deflate(lines)
  h = lambda **kw: P.ihdr(**dict(dict(w=4, h=3, depth=8, ctype=0), **kw))
  pal = P.chunk(b'PLTE', bytes(range(12)))
  assert outcome(lib, file_of(h(), good)) == (OK, '')
  assert outcome(lib, file_of(h(), good) + b'trailing bytes') == (OK, '')                   # lenient, as libpng is
  assert outcome(lib, file_of(h(), good, extra=P.chunk(b'tEXt', b'k\x00v', crc=1))) == (OK, '')

  def stream_of(build, data=lines):
    w = BitWriter()
    build(w)
    return zlib_stream(w, data)

  def oversubscribed(w):                                         # three code-length codes of one bit
    w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(0, 4)
    for n in (1, 1, 1, 0):
      w.bits(n, 3)

  cases = [
      # MMT_E_UNSUPPORTED
      (UNSUPPORTED, 'depth 16', file_of(h(depth=16), good)),
      (UNSUPPORTED, 'depth 16', file_of(h(depth=16, ctype=2), good)),
      (UNSUPPORTED, 'alpha', file_of(h(ctype=4), good)),
      (UNSUPPORTED, 'alpha', file_of(h(ctype=6), good)),
      (UNSUPPORTED, 'tRNS', file_of(h(), good, extra=P.chunk(b'tRNS', b'\x00\x05'))),
      (UNSUPPORTED, 'tRNS', file_of(h(depth=2, ctype=3), good, plte=pal, extra=P.chunk(b'tRNS', b'\x00'))),
      (UNSUPPORTED, 'unknown critical chunk', file_of(h(), good, extra=P.chunk(b'ABcd', b'x'))),
      (UNSUPPORTED, 'unknown critical chunk', P.SIGNATURE + h() + P.chunk(b'IDAT', good) + P.chunk(b'ABcd', b'x') + P.chunk(b'IEND')),
      (UNSUPPORTED, 'compression method', file_of(h(comp=1), good)),
      (UNSUPPORTED, 'filter method', file_of(h(filt=1), good)),
      (UNSUPPORTED, 'not a PNG', b'\xff\xd8\xff\xe0' + bytes(20)),
      # MMT_E_INVALID
      (INVALID, 'signature', b'\x89PNG\r\n\x1a\x0b' + file_of(h(), good)[8:]),
      (INVALID, 'CRC-32 mismatch on a IHDR', P.SIGNATURE + P.chunk(b'IHDR', struct.pack('>IIBBBBB', 4, 3, 8, 0, 0, 0, 0), crc=7) + file_of(h(), good)[33:]),
      (INVALID, 'CRC-32 mismatch on a PLTE', file_of(h(depth=2, ctype=3), good, plte=P.chunk(b'PLTE', bytes(range(12)), crc=7))),
      (INVALID, 'CRC-32 mismatch on a IDAT', file_of(h(), good, idat_crc=7)),
      (INVALID, 'CRC-32 mismatch on a IDAT', P.SIGNATURE + h() + P.chunk(b'IDAT', good[:5]) + P.chunk(b'IDAT', good[5:], crc=7) + P.chunk(b'IEND')),
      (INVALID, 'CRC-32 mismatch on a IEND', file_of(h(), good, iend_crc=7)),
      (INVALID, 'truncated', file_of(h(), good)[:-1]),
      (INVALID, 'truncated', file_of(h(), good)[:-12]),
      (INVALID, 'truncated', file_of(h(), good)[:45]),
      (INVALID, 'truncated', file_of(h(), good)[:20]),
      (INVALID, 'truncated', P.SIGNATURE[:5]),
      (INVALID, 'truncated', P.SIGNATURE + h() + P.chunk(b'IDAT', good[:-6]) + P.chunk(b'IEND')),
      (INVALID, 'preset dictionary', file_of(h(), b'\x78\xbb' + good[2:])),
      (INVALID, 'window larger than 32 KiB', file_of(h(), b'\x88\x1c' + good[2:])),
      (INVALID, 'zlib header', file_of(h(), b'\x78\x9d' + good[2:])),
      (INVALID, 'zlib header', file_of(h(), b'\x79\x9c' + good[2:])),
      (INVALID, 'code-length set', file_of(h(), stream_of(oversubscribed))),
      (INVALID, 'before the start of the stream', file_of(h(), stream_of(lambda w: fixed_block(w, [0, 1, (3, 3), 256], 1)))),
      (INVALID, 'reserved block type', file_of(h(), stream_of(lambda w: w.bits(7, 3)))),
      (INVALID, 'complement', file_of(h(), stream_of(lambda w: (w.bits(1, 3), w.align(), w.raw(b'\x0f\x00\x0f\x00' + lines))))),
      (INVALID, 'Adler-32 mismatch', file_of(h(), good[:-4] + bytes([good[-4] ^ 1]) + good[-3:])),
      (INVALID, 'shorter than the IHDR requires', file_of(h(), P.deflate(lines[:-1]))),
      (INVALID, 'shorter than the IHDR requires', file_of(h(w=5), good)),
      (INVALID, 'longer than', file_of(h(), P.deflate(lines + b'\x00'))),
      (INVALID, 'longer than', file_of(h(), P.deflate(lines + b'\x00', 'stored'))),
      (INVALID, 'longer than', file_of(h(w=3), good)),
      (INVALID, 'filter-type byte 5', file_of(h(), P.deflate(lines[:5] + b'\x05' + lines[6:]))),
      (INVALID, 'without a PLTE', file_of(h(depth=8, ctype=3), good)),
      (INVALID, 'entries are more than bit depth 1', file_of(h(depth=1, ctype=3), good, plte=P.chunk(b'PLTE', bytes(9)))),
      (INVALID, 'more than 256', file_of(h(), good, plte=P.chunk(b'PLTE', bytes(3 * 257)))),
      (INVALID, 'multiple of 3', file_of(h(depth=2, ctype=3), good, plte=P.chunk(b'PLTE', bytes(7)))),
      (INVALID, 'width 0', file_of(h(w=0), good)),
      (INVALID, 'height 0', file_of(h(h=0), good)),
      (INVALID, 'above 2^31 - 1', file_of(h(w=2 ** 31), good)),
      (INVALID, 'above 2^31 - 1', file_of(h(h=2 ** 32 - 1), good)),
      (INVALID, 'colour type 2 with bit depth 4', file_of(h(depth=4, ctype=2), good)),
      (INVALID, 'colour type 5', file_of(h(ctype=5), good)),
      (INVALID, 'interlace method 2', file_of(h(lace=2), good)),
  ]
  for code, reason, raw in cases:
    rc, msg = outcome(lib, raw)
    assert rc == code and reason in msg, (code, reason, rc, msg)
  L = lib.lib()
  im = lib.PngImage()
  raw = file_of(h(), good)
  lib.check(L.mmt_png_info(raw, len(raw), ctypes.byref(im)))
  out, plt = np.zeros(64, dtype=np.uint8), np.zeros(768, dtype=np.uint8)
  assert L.mmt_png_inflate(raw, len(raw), ctypes.byref(im), out.ctypes.data, im.raw_bytes - 1, plt.ctypes.data) == INVALID
  assert b'leave raw_out' in L.mmt_last_error()
  im.width += 1
  assert L.mmt_png_inflate(raw, len(raw), ctypes.byref(im), out.ctypes.data, 64, plt.ctypes.data) == INVALID
  assert b'does not describe this stream' in L.mmt_last_error()
  assert L.mmt_png_info(None, 4, ctypes.byref(im)) == INVALID and L.mmt_png_info(raw, -1, ctypes.byref(im)) == INVALID


# ---------------------------------------------------------------------------------------------------
# the Python entry points
# ---------------------------------------------------------------------------------------------------
def test_decode_png_images_cpu_batch_equals_per_file_results_for_any_worker_count(lib):
  from mmt_amd import feature_pipeline as fp
  names = list(P.names())
  kinds = (bytes, bytearray, memoryview, lambda b: np.frombuffer(b, dtype=np.uint8))
  blobs = [kinds[i % 4](P.data(n)) for i, n in enumerate(names)]
  pixels, offsets, heights, widths = fp.decode_png_images(blobs, 'cpu', workers=1)
  assert pixels.numel() == sum(P.expected(n).size for n in names)
  for i, n in enumerate(names):
    e = P.expected(n)
    assert (int(heights[i]), int(widths[i])) == e.shape[:2]
    got = pixels[int(offsets[i]):int(offsets[i]) + e.size].numpy().reshape(e.shape)
    assert np.array_equal(got, e), n
    one = fp.decode_png_images([P.data(n)], 'cpu')[0].numpy().reshape(e.shape)             # alone, the file gives the same bytes
    assert np.array_equal(one, got), n
  for workers in (3, 16, 10 ** 6):                              # the last is clamped to 16
    other = fp.decode_png_images(blobs, 'cpu', workers=workers)
    for a, b in zip((pixels, offsets, heights, widths), other):
      assert a.dtype == b.dtype and np.array_equal(a.numpy(), b.numpy()), workers


def test_decode_png_images_refusal_names_the_example(lib):
  from mmt_amd import feature_pipeline as fp
  names = P.names()
  sixteen = P.SIGNATURE + P.ihdr(2, 2, 16, 0) + P.chunk(b'IDAT', P.deflate(bytes(10))) + P.chunk(b'IEND')
  with pytest.raises(ValueError, match=r'data\[1\] cannot be decoded: .*depth 16'):
    fp.decode_png_images([P.data(names[0]), sixteen, P.data(names[1])], 'cpu')
  with pytest.raises(ValueError, match=r'data\[2\] cannot be decoded: .*truncated'):
    fp.decode_png_images([P.data(names[0]), P.data(names[1]), P.data(names[60])[:-20]], 'cpu', workers=2)
  with pytest.raises(ValueError, match='empty'):
    fp.decode_png_images([], 'cpu')


def test_decode_images_routes_by_signature(lib):
  import torch
  from mmt_amd import feature_pipeline as fp
  jn = ['33x31_420_q75', '9x2_422_q50', '17x9_grey_q80']
  for kw in (dict(), dict(workers=2, entropy='device', subseq_bytes=64, max_rounds=3), dict(out=torch.full((9000,), 7, dtype=torch.uint8))):
    kw2 = dict(kw, out=kw['out'].clone()) if 'out' in kw else kw
    a = fp.decode_images([J.data(n) for n in jn], 'cpu', **kw)
    b = fp.decode_jpeg_images([J.data(n) for n in jn], 'cpu', **kw2)
    assert all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))
  for bad in ([J.data(jn[0]), b'GIF89a' + bytes(30)], [J.data('refuse_progressive.jpg')]):
    with pytest.raises(ValueError) as e1:
      fp.decode_images(bad, 'cpu')
    with pytest.raises(ValueError) as e2:
      fp.decode_jpeg_images(bad, 'cpu')
    assert str(e1.value) == str(e2.value)
  pn = [P.names()[i] for i in (3, 40, 77, 100, 103)]
  data = [P.data(pn[0]), J.data(jn[0]), J.data(jn[1]), P.data(pn[1]), P.data(pn[2]), J.data(jn[2]), P.data(pn[3]), P.data(pn[4])]
  want = [P.expected(pn[0]), J.expected(jn[0]), J.expected(jn[1]), P.expected(pn[1]), P.expected(pn[2]), J.expected(jn[2]), P.expected(pn[3]),
          P.expected(pn[4])]
  total = sum(e.size for e in want)
  for out in (None, torch.full((total + 50,), P.SENTINEL, dtype=torch.uint8)):
    for entropy in ('host', 'device'):
      pixels, offsets, heights, widths = fp.decode_images(data, 'cpu', out=out, entropy=entropy, workers=3)
      assert offsets.dtype == torch.int64 and heights.dtype == torch.int32 and widths.dtype == torch.int32
      spans = []
      for i, e in enumerate(want):
        o = int(offsets[i])
        assert (int(heights[i]), int(widths[i])) == e.shape[:2]
        assert np.array_equal(pixels[o:o + e.size].numpy().reshape(e.shape), e), i
        spans.append((o, o + e.size))
      spans.sort()
      assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == total    # disjoint, back to back
      if out is not None:
        assert pixels is out and bool((out[total:] == P.SENTINEL).all())
  with pytest.raises(ValueError, match=r'data\[3\] cannot be decoded: png'):
    fp.decode_images(data[:3] + [P.data(pn[1])[:-9]], 'cpu')
  with pytest.raises(ValueError, match=r'data\[2\] cannot be decoded: .*progressive'):
    fp.decode_images([data[0], data[1], J.data('refuse_progressive.jpg')], 'cpu')


def test_decode_image_features_takes_png_bytes_on_cpu(lib):
  """Raises ValueError without the PNG decode: `_maybe_decode` sent every encoded list to the JPEG decoder."""
  import torch
  from mmt_amd import feature_pipeline as fp
  cfg = types.SimpleNamespace(is_training=False, image_size=32, patch_size=16, output_channel_bits=3)
  names = [P.names()[i] for i in (0, 17, 45, 80, 90, 98, 99, 100, 101, 102, 103)]
  got = fp.decode_image_features(cfg, [P.data(n) for n in names], keep_unnormalized=True, device='cpu')
  ref = fp.decode_image_features(cfg, [torch.from_numpy(P.expected(n).copy()) for n in names], keep_unnormalized=True)
  assert set(got) == set(ref)
  for k in ref:
    if isinstance(ref[k], torch.Tensor):
      assert got[k].dtype == ref[k].dtype and torch.equal(got[k], ref[k]), k
    else:
      assert got[k] == ref[k], k
  pf = fp.images_to_patch_features([P.data(n) for n in names] + [J.data('9x3_444_q90')], 32, 16, device='cpu')
  assert torch.equal(pf['patch_embeddings'][:-1], ref['patch_embeddings'])


def test_loader_decodes_a_shard_of_png_files_on_cpu(lib, tmp_path, monkeypatch):
  """A shard whose image_data holds PNG files, as the reference's Fashion-Gen shards do, through the loader's stages that
  run without a GPU (files, interleave, decode with RandAugment and the flip coin, masking; the side inputs are HIP
  only) with fixed seeds: the features are those the same shard gives when the decode stage is handed the committed
  decoded pixels in place of the files.  Raises ValueError on the first record without the PNG decode."""
  import torch
  from mmt_amd import configs
  from mmt_amd import feature_pipeline as fp
  from mmt_amd import pretrain_dataloader as pd
  from tests import _record_cases as R
  recs = R.loader_records(8)
  names = [P.names()[i] for i in (5, 23, 41, 58, 76, 94, 101, 103)]
  expected = {P.data(n): P.expected(n) for n in names}
  path = os.path.join(str(tmp_path), 'fashion-00000-of-00001.tfrecord')
  with open(path, 'wb') as f:
    for rec, name in zip(recs, names):
      feats = [('image_key', 'bytes', [rec['key'].encode()]), ('caption', 'bytes', [rec['caption'].encode('utf-8')]),
               ('image_data', 'bytes', [P.data(name)])]
      if rec['alt_text']:
        feats.append(('alt_text', 'bytes', [rec['alt_text'].encode('utf-8')]))
      f.write(R.frame(R.example(feats)))
  vocab = R.write_vocab(tmp_path / 'vocab.txt')
  cfg = configs.MmtPretrainDataConfig(
      input_path=path, vocab_filename=vocab, is_training=True, use_rand_aug=True, global_batch_size=8, image_size=32, patch_size=16,
      max_seq_len=32, tasks='mlm', text_special_token_field_dict=json.dumps(R.FIELD_DICT), mlm_max_selections_per_seq=26,
      mpp_max_selections_per_seq=4, seed=11)

  def features():
    loader = pd.MmtPretrainDataLoader(cfg, device='cpu', entropy='auto')
    group = list(itertools.islice(loader._interleave(loader._file_stream(0, 1)), 8))      # a training stream repeats for ever
    gen = torch.Generator(device='cpu').manual_seed(5)
    decoded = loader._decode(group, gen)
    return decoded, loader._mask(decoded, gen)

  from_files = features()
  real = fp.decode_image_features
  seen = []

  def on_pixels(data_config, images, **kw):
    seen.append(len(images))
    kw.pop('uploaded')
    return real(data_config, [torch.from_numpy(expected[bytes(im)].copy()) for im in images], **kw)

  monkeypatch.setattr(pd.fp, 'decode_image_features', on_pixels)
  from_pixels = features()
  assert seen == [8]
  for a, b in zip(from_files, from_pixels):
    assert set(a) == set(b)
    for k in a:
      assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
  assert from_files[0]['patch_embeddings'].shape == (8, 4, 16 * 16 * 3)


def test_sanitizer_program_of_the_host_stage():
  """`make asan-png` (csrc/Makefile): the host side of png_decode.hip under AddressSanitizer + UBSan, driven by a C
  program over the fixtures, their truncations and corruptions, and wrong metadata.  CPU only."""
  import shutil
  import subprocess
  if not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')):
    pytest.skip('no hipcc on this machine')
  csrc = os.path.join(ROOT, 'multimodal-long-transformer-2021_amd', 'csrc')
  res = subprocess.run(['make', '-s', '-C', csrc, 'asan-png'], capture_output=True, text=True, timeout=900)
  assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
  assert 'png asan driver ok' in res.stdout and 'ERROR: AddressSanitizer' not in res.stderr and 'runtime error' not in res.stderr
