"""JPEG decode: the numpy oracle, the fixture loader and the packing helpers of tests/test_jpeg_decode.py (CPU) and
tests/test_gpu_jpeg_decode.py (GPU).  The oracle is a full decode from bytes -- its own marker parser and Huffman decoder
in Python, the rules of DESIGN.md section 4 "JPEG decode" in numpy int64 -- and exposes the quantised coefficients as
well as the pixels.  tests/golden/jpeg holds the files with Pillow's (libjpeg-turbo's) decode of each, which pins the
oracle where Pillow is absent: parity is bit for bit, no tolerance anywhere."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg')
REFUSALS = ('refuse_progressive.jpg', 'refuse_cmyk.jpg', 'refuse_arithmetic.jpg', 'refuse_signature.png')
LARGE = '96x100_420_q75'               # more than one workgroup per image, whatever the tiling
SENTINEL = 0xA5
GUARD = 256

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
          62, 63)


# ---------------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def names():
  with open(os.path.join(GOLDEN, 'fixtures.txt')) as f:
    return tuple(line.strip() for line in f if line.strip())


def _shape(name):
  h, w = name.split('_', 1)[0].split('x')
  return int(h), int(w)


@functools.lru_cache(maxsize=None)
def _expected_all():
  out = {}
  for mode in sorted({n.split('_', 1)[1] for n in names()}):
    flat = np.load(os.path.join(GOLDEN, f'expected_{mode}.npz'))['pixels']
    at = 0
    for n in names():
      if n.split('_', 1)[1] == mode:
        h, w = _shape(n)
        out[n] = flat[at:at + h * w * 3].reshape(h, w, 3)
        out[n].setflags(write=False)
        at += h * w * 3
    assert at == flat.size, mode
  return out


def expected(name):
  """Pillow's decode of the fixture as committed, uint8 [h, w, 3], read-only."""
  return _expected_all()[name]


@functools.lru_cache(maxsize=None)
def data(name):
  path = os.path.join(GOLDEN, name if '.' in name else name + '.jpg')
  with open(path, 'rb') as f:
    return f.read()


# ---------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------
class _Bits:
  """Entropy-coded bits from `pos` on: 0xff00 is one 0xff byte; a marker or the end of the data is an error."""

  def __init__(self, buf, pos):
    self.buf, self.pos, self.acc, self.n = buf, pos, 0, 0

  def bit(self):
    if self.n == 0:
      b = self.buf[self.pos]
      if b == 0xFF:
        assert self.buf[self.pos + 1] == 0, 'marker inside coded data'
        self.pos += 1
      self.pos += 1
      self.acc, self.n = b, 8
    self.n -= 1
    return (self.acc >> self.n) & 1

  def bits(self, k):
    v = 0
    for _ in range(k):
      v = (v << 1) | self.bit()
    return v


def _huffman(counts, symbols):
  """{(length, code): symbol} of a DHT table."""
  table, code, k = {}, 0, 0
  for length in range(1, 17):
    for _ in range(counts[length - 1]):
      table[(length, code)] = symbols[k]
      code += 1
      k += 1
    code <<= 1
  return table


def _symbol(bits, table):
  code = 0
  for length in range(1, 17):
    code = (code << 1) | bits.bit()
    if (length, code) in table:
      return table[(length, code)]
  raise AssertionError('code not in the table')


def _extend(v, s):
  return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


class Decoded:
  """width, height, components, h_samp / v_samp / blocks_w / blocks_h per component, coef: one int16 array
  [blocks_h, blocks_w, 64] per component (natural order, padded to whole MCUs), qtables uint16 [3, 64], rgb uint8 [h, w, 3]."""


def _entropy_decode(buf):
  assert buf[0:2] == b'\xff\xd8'
  d = Decoded()
  q, dc, ac, restart, pos, frame = {}, {}, {}, 0, 2, None
  seen = set()
  while True:
    assert buf[pos] == 0xFF, hex(buf[pos])
    m = buf[pos + 1]
    pos += 2
    if m == 0xD9:
      break
    n = (buf[pos] << 8) | buf[pos + 1]
    seg = buf[pos + 2:pos + n]
    pos += n
    if m == 0xDB:
      while seg:
        assert seg[0] >> 4 == 0
        tab = np.zeros(64, dtype=np.uint16)
        tab[list(ZIGZAG)] = list(seg[1:65])
        q[seg[0] & 15] = tab
        seg = seg[65:]
    elif m == 0xC4:
      while seg:
        counts = list(seg[1:17])
        total = sum(counts)
        (ac if seg[0] >> 4 else dc)[seg[0] & 15] = _huffman(counts, list(seg[17:17 + total]))
        seg = seg[17 + total:]
    elif m == 0xDD:
      restart = (seg[0] << 8) | seg[1]
    elif m in (0xC0, 0xC1):
      assert seg[0] == 8
      d.height, d.width, d.components = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
      frame = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(d.components)]
      if d.components == 1:
        frame = [(frame[0][0], 1, 1, frame[0][3])]
      d.h_samp, d.v_samp = [f[1] for f in frame], [f[2] for f in frame]
      hmax, vmax = max(d.h_samp), max(d.v_samp)
      mx, my = -(-d.width // (8 * hmax)), -(-d.height // (8 * vmax))
      d.blocks_w, d.blocks_h = [mx * h for h in d.h_samp], [my * v for v in d.v_samp]
      d.coef = [np.zeros((bh, bw, 64), dtype=np.int16) for bh, bw in zip(d.blocks_h, d.blocks_w)]
      d.qtables = np.zeros((3, 64), dtype=np.uint16)
    elif m == 0xDA:
      ns = seg[0]
      comps = []
      for i in range(ns):
        c = [f[0] for f in frame].index(seg[1 + 2 * i])
        comps.append((c, dc[seg[2 + 2 * i] >> 4], ac[seg[2 + 2 * i] & 15]))
        if c not in seen:
          d.qtables[c] = q[frame[c][3]]
          seen.add(c)
      assert tuple(seg[1 + 2 * ns:4 + 2 * ns]) == (0, 63, 0)
      if ns == 1:
        c = comps[0][0]
        sx = -(-(-(-d.width * d.h_samp[c] // hmax)) // 8)
        sy = -(-(-(-d.height * d.v_samp[c] // vmax)) // 8)
      else:
        sx, sy = mx, my
      bits, pred, left, rst = _Bits(buf, pos), [0] * ns, restart, 0
      for y in range(sy):
        for x in range(sx):
          if restart and left == 0:
            assert buf[bits.pos] == 0xFF and buf[bits.pos + 1] == 0xD0 + rst
            bits = _Bits(buf, bits.pos + 2)
            pred, left, rst = [0] * ns, restart, (rst + 1) & 7
          for i, (c, tdc, tac) in enumerate(comps):
            nh, nv = (1, 1) if ns == 1 else (d.h_samp[c], d.v_samp[c])
            for v in range(nv):
              for h in range(nh):
                blk = d.coef[c][y * nv + v, x * nh + h]
                blk[:] = 0
                s = _symbol(bits, tdc)
                if s:
                  pred[i] += _extend(bits.bits(s), s)
                blk[0] = pred[i]
                k = 1
                while k < 64:
                  rs = _symbol(bits, tac)
                  r, s = rs >> 4, rs & 15
                  if s:
                    k += r
                    blk[ZIGZAG[k]] = _extend(bits.bits(s), s)
                    k += 1
                  elif r == 15:
                    k += 16
                  else:
                    break
          left -= 1
      pos = bits.pos
  assert len(seen) == d.components
  return d


def _idct_pass(v, shift):
  """jidctint.c's 1-D pass along the last axis of an int64 array."""
  i = [v[..., k] for k in range(8)]
  z1 = (i[2] + i[6]) * 4433
  e2, e3 = z1 - i[6] * 15137, z1 + i[2] * 6270
  e0, e1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
  t10, t13, t11, t12 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
  o0, o1, o2, o3 = i[7], i[5], i[3], i[1]
  z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
  z5 = (z3 + z4) * 9633
  o0, o1, o2, o3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
  z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
  o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
  out = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
  return np.stack([(x + (1 << (shift - 1))) >> shift for x in out], axis=-1)


def idct_planes(d):
  """One uint8-valued int64 plane [blocks_h * 8, blocks_w * 8] per component."""
  planes = []
  for c in range(d.components):
    bh, bw = d.blocks_h[c], d.blocks_w[c]
    x = d.coef[c].astype(np.int64).reshape(bh, bw, 8, 8) * d.qtables[c].astype(np.int64).reshape(8, 8)
    x = _idct_pass(x.swapaxes(-1, -2), 11).swapaxes(-1, -2)               # columns
    x = np.clip(_idct_pass(x, 18) + 128, 0, 255)                          # rows
    planes.append(x.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
  return planes


def _upsample(s, w, h, hs, vs):
  """s: the component's real samples [ch, cw].  libjpeg's fancy upsampling to [h, w]; a plane at most 2 wide is replicated."""
  ch, cw = s.shape
  x, y = np.arange(w), np.arange(h)
  if hs == 1:
    return s[:h, :w]
  i = x >> 1
  if cw <= 2:
    return s[(y >> 1) if vs == 2 else y][:, i]
  nb = np.where(x & 1, np.minimum(i + 1, cw - 1), np.maximum(i - 1, 0))
  if vs == 1:
    return (3 * s[:h, i] + s[:h, nb] + np.where(x & 1, 2, 1)) >> 2
  rn = y >> 1
  rf = np.where(y & 1, np.minimum(rn + 1, ch - 1), np.maximum(rn - 1, 0))
  c = 3 * s[rn] + s[rf]
  return (3 * c[:, i] + c[:, nb] + np.where(x & 1, 7, 8)) >> 4


@functools.lru_cache(maxsize=None)
def decode(name):
  """The oracle's decode of a fixture, computed once and shared (treat as read-only)."""
  d = _entropy_decode(data(name))
  planes = idct_planes(d)
  w, h = d.width, d.height
  if d.components == 1:
    rgb = np.repeat(planes[0][:h, :w, None], 3, axis=-1)
  else:
    hs, vs = d.h_samp[0], d.v_samp[0]
    cw, ch = -(-w // hs), -(-h // vs)
    Y = planes[0][:h, :w]
    cb = _upsample(planes[1][:ch, :cw], w, h, hs, vs) - 128
    cr = _upsample(planes[2][:ch, :cw], w, h, hs, vs) - 128
    r = Y + ((91881 * cr + 32768) >> 16)
    g = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = Y + ((116130 * cb + 32768) >> 16)
    rgb = np.clip(np.stack([r, g, b], axis=-1), 0, 255)
  d.rgb = rgb.astype(np.uint8)
  d.rgb.setflags(write=False)
  return d


# ---------------------------------------------------------------------------------------------------
# buffers for the C ABI: the library's own info and coefficients calls, and the packed output layout
# ---------------------------------------------------------------------------------------------------
def aligned(n, dtype, fill=0):
  """A numpy array of n elements whose data is 64-byte aligned."""
  item = np.dtype(dtype).itemsize
  raw = np.full(n * item + 64, 0, dtype=np.uint8)
  start = (-raw.ctypes.data) % 64
  out = raw[start:start + n * item].view(dtype)
  out[:] = fill
  return out


def host_stage(lib, name_list, gaps=(5, 16, 0, 7, 3, 1, 32, 2, 11, 13, 6, 9, 4, 8, 10, 17)):
  """mmt_jpeg_info and mmt_jpeg_coefficients over the fixtures: (images: ctypes array of JpegImage with batch offsets,
  coef int16, qtables uint16 [B*192], pixel offsets, n = pixels_bytes).  Images sit at mostly odd pixel offsets with
  gaps between them."""
  import ctypes
  L = lib.lib()
  B = len(name_list)
  images = (lib.JpegImage * B)()
  base, at = 0, gaps[0]
  offs = []
  for b, name in enumerate(name_list):
    raw = data(name)
    lib.check(L.mmt_jpeg_info(raw, len(raw), ctypes.byref(images[b])))
    for c in range(3):
      images[b].coef_offset[c] += base
    base += images[b].coef_elems
    images[b].pixel_offset = at
    offs.append(at)
    at += images[b].width * images[b].height * 3 + gaps[(b + 1) % len(gaps)]
  coef = aligned(base, np.int16, fill=0x5555)
  qtables = aligned(B * 192, np.uint16)
  for b, name in enumerate(name_list):
    raw = data(name)
    lib.check(L.mmt_jpeg_coefficients(raw, len(raw), ctypes.byref(images[b]), coef.ctypes.data, base,
                                      qtables[b * 192:].ctypes.data))
  return images, coef, qtables, offs, at


def check_packed(got, images_expected, offsets):
  """`got` (uint8, pre-filled with SENTINEL, GUARD bytes behind pixels_bytes) holds exactly the expected images; gaps and
  guard untouched."""
  want = np.full(got.shape, SENTINEL, dtype=np.uint8)
  for o, im in zip(offsets, images_expected):
    want[o:o + im.size] = im.reshape(-1)
  bad = np.nonzero(got != want)[0]
  assert bad.size == 0, f'{bad.size} bytes differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]} (offsets {list(offsets)})'
