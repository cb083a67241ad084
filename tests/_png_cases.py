"""PNG decode: a PNG writer in plain Python (zlib.compressobj, zlib.crc32, struct), the numpy oracle, the fixture
loader and the packing helpers of tests/test_png_decode.py (CPU) and tests/test_gpu_png_decode.py (GPU).  The oracle is
a full decode from bytes -- its own chunk walk, zlib.decompress, and the unfilter, de-interlace and expansion rules of
DESIGN.md section 4 "PNG decode".  tests/golden/png holds the files with Pillow's (libpng's) decode of each, which pins
the oracle where Pillow is absent: parity is bit for bit, no tolerance anywhere.  No code of mmt_amd is used by the
writer or the oracle."""
import functools
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'png')
SIGNATURE = b'\x89PNG\r\n\x1a\n'
SENTINEL = 0xA5
GUARD = 256

SIZES = ((1, 1), (1, 40), (40, 1), (3, 3), (4, 5), (9, 17), (64, 3), (65, 5), (130, 7), (33, 70), (16, 200))      # height x width
KINDS = ('rgb8', 'g8', 'g4', 'g2', 'g1', 'p8', 'p4', 'p2', 'p1')
FILTERS = (0, 1, 2, 3, 4, 'cycle')
BLOCKS = ('stored', 'fixed', 'dynamic')
SPLITS = (None, 1, 7, 100)
CYCLE = (4, 3, 1, 2, 0)
EXTRA = ('pillow_optimize', 'pillow_palette', 'pillow_bilevel', 'ancillary_chunks', 'short_palette')
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))        # x0, y0, dx, dy


def plan():
  """The crossed fixtures as (name, height, width, kind, filter, interlace, block, split): every kind with every size,
  and filter, interlace, block kind and split chosen so that each value meets every size and every kind."""
  out = []
  for s, (h, w) in enumerate(SIZES):
    for k, kind in enumerate(KINDS):
      f = FILTERS[(k + s) % 6]
      lace = (k // 2 + s + (k + s) // 6) % 2
      block = BLOCKS[(k + 2 * s + (k + s) // 6) % 3]
      split = SPLITS[(k + s // 2) % 4]
      out.append((f'{h}x{w}_{kind}_f{f}_i{lace}_{block}', h, w, kind, f, lace, block, split))
  return out


# ---------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------
def chunk(ctype: bytes, body: bytes = b'', crc=None) -> bytes:
  crc = zlib.crc32(ctype + body) if crc is None else crc
  return struct.pack('>I', len(body)) + ctype + body + struct.pack('>I', crc & 0xFFFFFFFF)


def ihdr(w, h, depth, ctype, lace=0, comp=0, filt=0) -> bytes:
  return chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, ctype, comp, filt, lace))


def kind_fields(kind):
  """(colour type, bit depth) of a kind."""
  return {'rgb': 2, 'g': 0, 'p': 3}[kind.rstrip('0123456789')], int(kind.lstrip('rgbp'))


def _pack_rows(samples, depth):
  """[rows, n] samples of `depth` bits (or [rows, n, 3] bytes) -> list of row byte strings, MSB first, zero-padded."""
  if samples.ndim == 3:
    return [bytes(r.reshape(-1).astype(np.uint8)) for r in samples]
  per = 8 // depth
  rows, n = samples.shape
  pad = (-n) % per
  s = np.concatenate([samples.astype(np.int64), np.zeros((rows, pad), dtype=np.int64)], axis=1).reshape(rows, -1, per)
  shifts = np.array([8 - depth * (i + 1) for i in range(per)], dtype=np.int64)
  return [bytes(r.astype(np.uint8)) for r in (s << shifts).sum(axis=2)]


def _filter_row(ft, cur, prev, bpp):
  cur = np.frombuffer(cur, dtype=np.uint8).astype(np.int64)
  prev = np.frombuffer(prev, dtype=np.uint8).astype(np.int64)
  a = np.concatenate([np.zeros(bpp, dtype=np.int64), cur[:-bpp]]) if cur.size > bpp else np.zeros_like(cur)
  c = np.concatenate([np.zeros(bpp, dtype=np.int64), prev[:-bpp]]) if cur.size > bpp else np.zeros_like(cur)
  if ft == 0:
    pred = 0
  elif ft == 1:
    pred = a
  elif ft == 2:
    pred = prev
  elif ft == 3:
    pred = (a + prev) >> 1
  else:
    p = a + prev - c
    pa, pb, pc = abs(p - a), abs(p - prev), abs(p - c)
    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
  return bytes([ft]) + bytes(((cur - pred) & 255).astype(np.uint8))


def scanlines(kind, samples, filters='cycle', lace=0) -> bytes:
  """The filtered scanlines (what the IDAT stream inflates to).  filters: one type, 'cycle', or a sequence cycled over
  the rows of each pass."""
  _, depth = kind_fields(kind)
  bpp = 3 if kind == 'rgb8' else 1
  seq = CYCLE if filters == 'cycle' else ((filters,) if isinstance(filters, int) else tuple(filters))
  h, w = samples.shape[:2]
  out = []
  for x0, y0, dx, dy in (ADAM7 if lace else ((0, 0, 1, 1),)):
    sub = samples[y0::dy, x0::dx]
    if sub.shape[0] == 0 or sub.shape[1] == 0:
      continue
    rows = _pack_rows(sub, depth)
    prev = bytes(len(rows[0]))
    for i, row in enumerate(rows):
      out.append(_filter_row(seq[i % len(seq)], row, prev, bpp))
      prev = row
  return b''.join(out)


def deflate(raw: bytes, block='dynamic') -> bytes:
  if block == 'stored':
    co = zlib.compressobj(0)
  elif block == 'fixed':
    co = zlib.compressobj(9, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
  else:
    co = zlib.compressobj(9)
  return co.compress(raw) + co.flush()


def idats(stream: bytes, split=None) -> bytes:
  """One IDAT, or pieces: the first eight of `split` bytes (1 cuts inside the zlib header), the rest of 16 * split + 20."""
  if not split:
    return chunk(b'IDAT', stream)
  cuts = [min(i * split, len(stream)) for i in range(9)]
  cuts += list(range(cuts[-1] + 16 * split + 20, len(stream), 16 * split + 20)) + [len(stream)]
  return b''.join(chunk(b'IDAT', stream[a:b]) for a, b in zip(cuts, cuts[1:]) if b > a or a == 0)


def encode(kind, samples, *, palette=None, filters='cycle', lace=0, block='dynamic', split=None, before_idat=b'', after_idat=b'',
           stream=None) -> bytes:
  """A PNG file.  samples: uint8 [h, w, 3] for 'rgb8', [h, w] integers below 1 << depth otherwise; palette: uint8 [n, 3].
  stream: a zlib stream to store in place of the deflated scanlines."""
  ctype, depth = kind_fields(kind)
  h, w = samples.shape[:2]
  body = deflate(scanlines(kind, samples, filters, lace), block) if stream is None else stream
  plte = chunk(b'PLTE', bytes(np.asarray(palette, dtype=np.uint8).reshape(-1))) if palette is not None else b''
  return SIGNATURE + ihdr(w, h, depth, ctype, lace) + plte + before_idat + idats(body, split) + after_idat + chunk(b'IEND')


def content(kind, h, w, seed=0, palette_entries=None):
  """Deterministic samples (and a palette for 'p' kinds): a smooth ramp plus noise, so every filter has work to do."""
  rng = np.random.default_rng(1000 + seed)
  ctype, depth = kind_fields(kind)
  yy, xx = np.mgrid[0:h, 0:w]
  if kind == 'rgb8':
    base = np.stack([(xx * 7 + yy * 3) % 256, (xx * 2 + yy * 11 + 40) % 256, (xx * yy + 90) % 256], axis=2)
    return ((base + rng.integers(0, 24, size=base.shape)) % 256).astype(np.uint8), None
  top = 1 << depth
  smp = ((xx * 3 + yy * 5) // 2 + rng.integers(0, max(top // 4, 2), size=(h, w))) % top
  if ctype == 0:
    return smp.astype(np.uint8), None
  n = top if palette_entries is None else palette_entries
  return smp.astype(np.uint8), rng.integers(0, 256, size=(n, 3), dtype=np.uint8)


def build(name):
  """The bytes of a crossed fixture, from its plan entry."""
  for s, (n, h, w, kind, f, lace, block, split) in enumerate(plan()):
    if n == name:
      smp, pal = content(kind, h, w, seed=s)
      return encode(kind, smp, palette=pal, filters=f, lace=lace, block=block, split=split)
  raise KeyError(name)


# ---------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def names():
  with open(os.path.join(GOLDEN, 'fixtures.txt')) as f:
    return tuple(line.strip() for line in f if line.strip())


@functools.lru_cache(maxsize=None)
def data(name):
  with open(os.path.join(GOLDEN, name + '.png'), 'rb') as f:
    return f.read()


@functools.lru_cache(maxsize=None)
def _expected_all():
  flat = np.fromfile(os.path.join(GOLDEN, 'expected_pixels.rgb'), dtype=np.uint8)
  out, at = {}, 0
  for n in names():
    w, h = struct.unpack('>II', data(n)[16:24])
    out[n] = flat[at:at + h * w * 3].reshape(h, w, 3)
    out[n].setflags(write=False)
    at += h * w * 3
  assert at == flat.size
  return out


def expected(name):
  """Pillow's decode of the fixture as committed, uint8 [h, w, 3], read-only."""
  return _expected_all()[name]


# ---------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------
class Decoded:
  pass


def chunks_of(buf):
  """[(type, body, stored crc)] of a well-formed file."""
  assert buf[:8] == SIGNATURE
  at, out = 8, []
  while at < len(buf):
    n, = struct.unpack('>I', buf[at:at + 4])
    out.append((bytes(buf[at + 4:at + 8]), bytes(buf[at + 8:at + 8 + n]), struct.unpack('>I', buf[at + 8 + n:at + 12 + n])[0]))
    at += 12 + n
    if out[-1][0] == b'IEND':
      break
  return out


def _paeth(a, b, c):
  p = a + b - c
  pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
  return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def unfilter(raw, at, rows, rowbytes, bpp):
  """rows x rowbytes reconstructed bytes of one pass, from raw[at:]."""
  out = np.zeros((rows, rowbytes), dtype=np.uint8)
  prev = [0] * rowbytes
  for r in range(rows):
    ft = raw[at]
    line = raw[at + 1:at + 1 + rowbytes]
    cur = [0] * rowbytes
    for i in range(rowbytes):
      a = cur[i - bpp] if i >= bpp else 0
      c = prev[i - bpp] if i >= bpp else 0
      b = prev[i]
      pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[ft]
      cur[i] = (line[i] + pred) & 255
    out[r] = cur
    prev = cur
    at += 1 + rowbytes
  return out, at


@functools.lru_cache(maxsize=None)
def decode_bytes(buf) -> Decoded:
  """The oracle: fields of the IHDR, the inflated scanlines (`raw`), the zero-padded palette and the RGB pixels."""
  d = Decoded()
  cs = chunks_of(buf)
  d.width, d.height, d.depth, d.color_type, _, _, d.interlace = struct.unpack('>IIBBBBB', cs[0][1])
  plte = [c[1] for c in cs if c[0] == b'PLTE']
  d.palette = np.zeros((256, 3), dtype=np.uint8)
  d.palette_entries = 0
  if plte:
    d.palette_entries = len(plte[0]) // 3
    d.palette[:d.palette_entries] = np.frombuffer(plte[0], dtype=np.uint8).reshape(-1, 3)
  d.raw = zlib.decompress(b''.join(c[1] for c in cs if c[0] == b'IDAT'))
  w, h, depth = d.width, d.height, d.depth
  bpp = 3 if d.color_type == 2 else 1
  per = 1 if d.color_type == 2 else 8 // depth
  rgb = np.zeros((h, w, 3), dtype=np.uint8)
  at = 0
  for x0, y0, dx, dy in (ADAM7 if d.interlace else ((0, 0, 1, 1),)):
    pw, ph = len(range(x0, w, dx)), len(range(y0, h, dy))
    if pw == 0 or ph == 0:
      continue
    rowbytes = pw * 3 if d.color_type == 2 else (pw + per - 1) // per
    rec, at = unfilter(d.raw, at, ph, rowbytes, bpp)
    if d.color_type == 2:
      px = rec.reshape(ph, pw, 3)
    else:
      shifts = np.array([8 - depth * (i + 1) for i in range(per)])
      smp = ((rec[:, :, None].astype(np.int64) >> shifts) & ((1 << depth) - 1)).reshape(ph, -1)[:, :pw]
      if d.color_type == 0:
        px = np.repeat((smp * (255 // ((1 << depth) - 1)))[:, :, None], 3, axis=2).astype(np.uint8)
      else:
        px = d.palette[smp]                                     # an index beyond the entries reads a zero row
    rgb[y0::dy, x0::dx] = px
  assert at == len(d.raw)
  d.rgb = rgb
  return d


def decode(name) -> Decoded:
  return decode_bytes(data(name))


# ---------------------------------------------------------------------------------------------------
# the library's host stage, and packing
# ---------------------------------------------------------------------------------------------------
def host_stage(lib, blobs, guard=0):
  """mmt_png_info + mmt_png_inflate of each file into one raw buffer: (images ctypes array, raw uint8, palettes uint8
  [B * 768], pixel offsets, total pixel bytes).  `guard` sentinel bytes surround the raw block."""
  import ctypes
  L = lib.lib()
  B = len(blobs)
  images = (lib.PngImage * B)()
  n_raw, n_pix, offs = 0, 0, []
  for i, raw in enumerate(blobs):
    lib.check(L.mmt_png_info(raw, len(raw), ctypes.byref(images[i])))
    images[i].raw_offset, images[i].pixel_offset = guard + n_raw, n_pix
    n_raw += images[i].raw_bytes
    offs.append(n_pix)
    n_pix += images[i].width * images[i].height * 3
  buf = np.full(n_raw + 2 * guard, SENTINEL, dtype=np.uint8)
  pal = np.full(B * 768, SENTINEL, dtype=np.uint8)
  for i, raw in enumerate(blobs):
    lib.check(L.mmt_png_inflate(raw, len(raw), ctypes.byref(images[i]), buf.ctypes.data, buf.size, pal.ctypes.data + i * 768))
  return images, buf, pal, offs, n_pix


def check_packed(out, expected_list, offsets):
  """out: uint8 with GUARD sentinel bytes behind the packed images; every image equals its expected pixels."""
  end = 0
  for e, o in zip(expected_list, offsets):
    assert np.array_equal(out[o:o + e.size].reshape(e.shape), e)
    end = max(end, o + e.size)
  assert np.all(out[end:] == SENTINEL)
